"""Python side of the emulated R session (tests/r_emul/): loads tests/r_emul/libsinglet_hip_shim_emul.so -- the unchanged
singlet_amd/r/*.c linked against the emulated R C API -- builds R objects from numpy arrays, makes .Call()s through the
registration table and reads the results back in R's layout.  Used by test_r_shim_emulated.py (no device) and
test_gpu_r_shim.py."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(HERE, "r_emul", "libsinglet_hip_shim_emul.so")

NILSXP, SYMSXP, CHARSXP, LGLSXP, INTSXP, REALSXP, STRSXP, VECSXP, S4SXP = 0, 1, 9, 10, 13, 14, 16, 19, 25
NA_INTEGER = -2**31
OK, ERROR, INTERRUPT, REFUSED = 0, 1, 2, 3

_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
_SEXP = C.c_void_p


def _bind(lib):
    sig = {
        "emul_call": (_SEXP, [C.c_char_p, C.c_int, C.POINTER(_SEXP)]),
        "emul_last_kind": (C.c_int, []), "emul_last_message": (C.c_char_p, []),
        "emul_protect_delta": (C.c_int, []), "emul_protect_delta_at_exit": (C.c_int, []), "emul_protect_depth": (C.c_int, []),
        "emul_output": (C.c_char_p, []), "emul_polls": (C.c_long, []), "emul_arm_interrupt": (None, [C.c_long]),
        "emul_event_count": (C.c_int, []), "emul_event": (C.c_char_p, [C.c_int]), "emul_clear_events": (None, []),
        "emul_ralloc_blocks": (C.c_long, []), "emul_object_count": (C.c_long, []), "emul_poisoned_count": (C.c_long, []),
        "emul_dll": (C.c_void_p, []), "emul_dynamic_symbols": (C.c_int, []),
        "emul_entry_count": (C.c_int, []), "emul_entry_name": (C.c_char_p, [C.c_int]), "emul_entry_arity": (C.c_int, [C.c_int]),
        "emul_reset": (None, []), "TYPEOF": (C.c_int, [_SEXP]),
        "emul_make_real": (_SEXP, [_f64p, C.c_ssize_t]), "emul_make_int": (_SEXP, [_i32p, C.c_ssize_t]),
        "emul_make_lgl": (_SEXP, [_i32p, C.c_ssize_t]),
        "emul_make_real_matrix": (_SEXP, [_f64p, C.c_int, C.c_int]), "emul_make_int_matrix": (_SEXP, [_i32p, C.c_int, C.c_int]),
        "emul_make_string": (_SEXP, [C.c_char_p]), "emul_make_list": (_SEXP, [C.c_ssize_t]), "emul_make_s4": (_SEXP, [C.c_char_p]),
        "emul_set_slot": (None, [_SEXP, C.c_char_p, _SEXP]),
        "emul_make_dgc": (_SEXP, [_f64p, C.c_ssize_t, _i32p, C.c_ssize_t, _i32p, C.c_ssize_t, C.c_int, C.c_int]),
        "emul_type": (C.c_int, [_SEXP]), "emul_length": (C.c_longlong, [_SEXP]), "emul_alive": (C.c_int, [_SEXP]),
        "emul_data": (C.c_void_p, [_SEXP]), "emul_class": (C.c_char_p, [_SEXP]), "emul_dim": (C.c_int, [_SEXP, _i32p, C.c_int]),
        "emul_names_count": (C.c_int, [_SEXP]), "emul_name": (C.c_char_p, [_SEXP, C.c_int]),
        "emul_element": (_SEXP, [_SEXP, C.c_longlong]), "emul_slot": (_SEXP, [_SEXP, C.c_char_p]), "emul_slot_count": (C.c_int, [_SEXP]),
        "emul_chars": (C.c_char_p, [_SEXP]),
        # the R API itself, for the checks of the emulator on hand-made objects.  An R error raised by one of these while no
        # .Call is running is recorded as an event ("R error outside a call") and the function returns a harmless value
        "Rf_protect": (_SEXP, [_SEXP]), "Rf_unprotect": (None, [C.c_int]),
        "Rf_allocVector": (_SEXP, [C.c_uint, C.c_ssize_t]), "Rf_allocMatrix": (_SEXP, [C.c_uint, C.c_int, C.c_int]),
        "Rf_asReal": (C.c_double, [_SEXP]), "Rf_asInteger": (C.c_int, [_SEXP]), "Rf_asLogical": (C.c_int, [_SEXP]),
        "Rf_isMatrix": (C.c_int, [_SEXP]), "Rf_nrows": (C.c_int, [_SEXP]), "Rf_ncols": (C.c_int, [_SEXP]),
        "Rf_install": (_SEXP, [C.c_char_p]), "R_has_slot": (C.c_int, [_SEXP, _SEXP]), "XLENGTH": (C.c_ssize_t, [_SEXP]),
        "SET_VECTOR_ELT": (_SEXP, [_SEXP, C.c_ssize_t, _SEXP]),
        "R_init_singlet_hip_shim": (None, [C.c_void_p]), "R_unload_singlet_hip_shim": (None, [C.c_void_p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


_lib = None


def nil():
    """R_NilValue"""
    return C.c_void_p.in_dll(load(), "R_NilValue").value


def load():
    """The emulated session's shared object.  It is a build product (__graft_entry__.build() makes it after the library);
    the tests neither compile it nor skip without it."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError("%s is missing: run build() (python -c 'import __graft_entry__ as g; g.build()')" % SO_PATH)
        _lib = _bind(C.CDLL(SO_PATH))
        _lib.R_init_singlet_hip_shim(_lib.emul_dll())
    return _lib


class Result:
    """What one .Call() left: the value (a pointer, or None), the condition kind and message, and the call's bookkeeping."""

    def __init__(self, L, value):
        self.value = value
        self.kind = L.emul_last_kind()
        self.message = L.emul_last_message().decode()
        self.protect_delta = L.emul_protect_delta()
        self.protect_delta_at_exit = L.emul_protect_delta_at_exit()
        self.output = L.emul_output().decode()
        self.polls = L.emul_polls()
        self.events = [L.emul_event(q).decode() for q in range(min(L.emul_event_count(), 64))]
        self.ralloc_blocks = L.emul_ralloc_blocks()


class Session:
    """One emulated R session.  Every object a test builds is protected at once (the collector runs at every allocation and
    would poison it otherwise); close() empties the protect stack and frees the objects."""

    def __init__(self):
        self.L = load()
        self.L.emul_reset()
        self._keep = []   # numpy buffers handed to C stay alive while the session does

    def close(self):
        self.L.emul_arm_interrupt(0)
        self.L.emul_reset()
        self._keep = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- building ------------------------------------------------------------------------------------------------------
    def _p(self, s):
        assert s, "the emulator returned no object"
        self.L.Rf_protect(s)
        return s

    @staticmethod
    def _f64(a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        return a, a.ctypes.data_as(_f64p)

    @staticmethod
    def _i32(a):
        a = np.ascontiguousarray(a, dtype=np.int32).ravel()
        return a, a.ctypes.data_as(_i32p)

    def real(self, v):
        a, p = self._f64(np.atleast_1d(v))
        return self._p(self.L.emul_make_real(p, a.size))

    def integer(self, v):
        a, p = self._i32(np.atleast_1d(v))
        return self._p(self.L.emul_make_int(p, a.size))

    def logical(self, v):
        a, p = self._i32(np.atleast_1d(v))
        return self._p(self.L.emul_make_lgl(p, a.size))

    def string(self, text):
        return self._p(self.L.emul_make_string(text.encode()))

    def matrix(self, M):
        """a numeric R matrix with the values of the 2-D array M (stored column-major, as R does)"""
        M = np.asarray(M, dtype=np.float64)
        assert M.ndim == 2
        a, p = self._f64(np.asfortranarray(M).ravel(order="F"))
        return self._p(self.L.emul_make_real_matrix(p, M.shape[0], M.shape[1]))

    def int_matrix(self, M):
        M = np.asarray(M, dtype=np.int32)
        assert M.ndim == 2
        a, p = self._i32(np.asfortranarray(M).ravel(order="F"))
        return self._p(self.L.emul_make_int_matrix(p, M.shape[0], M.shape[1]))

    def rlist(self, items):
        lst = self._p(self.L.emul_make_list(len(items)))
        for q, it in enumerate(items):
            self.L.SET_VECTOR_ELT(lst, q, it)
        return lst

    def dgc(self, x, i, p, dim):
        """new("dgCMatrix", ...) from CSC arrays; the lengths are taken as given, so malformed matrices can be made"""
        xa, xp = self._f64(x)
        ia, ip = self._i32(i)
        pa, pp = self._i32(p)
        return self._p(self.L.emul_make_dgc(xp, xa.size, ip, ia.size, pp, pa.size, int(dim[0]), int(dim[1])))

    def s4(self, class_name, **slots):
        s = self._p(self.L.emul_make_s4(class_name.encode()))
        for name, value in slots.items():
            self.L.emul_set_slot(s, name.encode(), value)
        return s

    # ---- calling -------------------------------------------------------------------------------------------------------
    def call(self, name, *args):
        arr = (_SEXP * max(len(args), 1))(*args)
        value = self.L.emul_call(name.encode(), len(args), arr)
        return Result(self.L, value)

    # ---- reading -------------------------------------------------------------------------------------------------------
    def typeof(self, s):
        return self.L.emul_type(s)

    def length(self, s):
        return self.L.emul_length(s)

    def dim(self, s):
        out = (C.c_int32 * 4)()
        n = self.L.emul_dim(s, out, 4)
        return tuple(out[q] for q in range(min(n, 4))) if n else None

    def names(self, s):
        return [self.L.emul_name(s, q).decode() for q in range(self.L.emul_names_count(s))]

    def values(self, s):
        """a copy of the payload of a logical, integer or double vector, flat, in R's (column-major) order"""
        t, n = self.L.emul_type(s), self.L.emul_length(s)
        assert t in (LGLSXP, INTSXP, REALSXP), t
        ct, dt = (C.c_double, np.float64) if t == REALSXP else (C.c_int32, np.int32)
        if n == 0:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(C.cast(self.L.emul_data(s), C.POINTER(ct)), shape=(n,)).copy()

    def as_matrix(self, s):
        """an R matrix as a (nrow, ncol) array"""
        d = self.dim(s)
        assert d is not None and len(d) == 2, d
        return self.values(s).reshape((d[1], d[0])).T

    def element(self, s, q):
        return self.L.emul_element(s, q)

    def as_dict(self, s):
        """a named list as {name: pointer}, in the list's order"""
        assert self.L.emul_type(s) == VECSXP
        return {nm: self.L.emul_element(s, q) for q, nm in enumerate(self.names(s))}

    def slot(self, s, name):
        return self.L.emul_slot(s, name.encode())

    def class_name(self, s):
        return self.L.emul_class(s).decode()
