"""ctypes binding of oracle/_ref/libals_ref.so and libals_ref_b.so: the REFERENCE's own ALS functions, cut out of its
tree at build time and compiled against oracle/standin/ (oracle/make_ref.sh, oracle/ref_als_shim.cpp).

TEST INFRASTRUCTURE ONLY, like oracle.py.  variant("a") / variant("b") return a namespace with the functions of
oracle.py under the same names and signatures (nnls, predict, predict_mask, mse_test, c_nmf, c_ard_nmf, ...), so a test
hands the same arguments to the oracle and to the reference build.  This is done by executing oracle.py a second time
with its library handle replaced: every ora_X the wrappers call resolves to ref_X of the reference build, with the
oracle's argument types.  What the reference build does not hold (the synthetic generator, transpose, the hash helpers:
not reference functions) resolves to the oracle's library; anything else the reference build lacks raises.

  variant A (libals_ref.so)    stand-in reductions ascending, no contraction: the oracle's arithmetic
  variant B (libals_ref_b.so)  the same cut text, reductions descending, contraction on

Differences from oracle.py's returns, all because the reference returns less:
  * nnls()'s third value (sweep count) is -1;
  * the drivers' `iter` is the number of "%4d | %8.2e" lines the reference printed (verbose), and `tol` holds the
    PRINTED tolerances (three significant digits): compare with printed_tol();
  * c_ard_nmf*()'s n_iter is -1 (the `iter` vector is the reference's own).

available(name) reports absence instead of raising at import.
"""
import ctypes as C
import importlib.util
import os
import types

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"a": os.path.join(_HERE, "_ref", "libals_ref.so"), "b": os.path.join(_HERE, "_ref", "libals_ref_b.so")}

# not reference functions: helpers of the oracle that the wrappers (CSC.t(), synth_*) need
_ORACLE_HELPERS = ("ora_transpose", "ora_synth_count", "ora_synth_fill", "ora_synth_gene_count", "ora_synth_gene_fill",
                   "ora_synth_winit", "ora_rng_rand", "ora_rng_draw", "ora_rng_mask", "ora_log_normalize", "ora_max_threads")

_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)


def available(name="a"):
    return os.path.exists(LIBS[name])


class _Lib:
    """Stands where oracle.py expects its CDLL: ora_X -> ref_X of the reference build, typed as the oracle's ora_X."""

    def __init__(self, ref, ora_lib):
        self._ref, self._ora = ref, ora_lib

    def __getattr__(self, name):
        if name in _ORACLE_HELPERS:
            return getattr(self._ora, name)
        if not name.startswith("ora_"):
            raise AttributeError(name)
        try:
            f = getattr(self._ref, "ref_" + name[4:])
        except AttributeError:
            raise AttributeError("the reference build has no counterpart of %s" % name) from None
        proto = getattr(self._ora, name)
        f.restype, f.argtypes = proto.restype, proto.argtypes
        setattr(self, name, f)
        return f


_variants = {}


def variant(name="a"):
    if name in _variants:
        return _variants[name]
    if not available(name):
        raise FileNotFoundError("%s is not built (oracle/make_ref.sh needs the reference tree)" % LIBS[name])
    from oracle import oracle as ora
    ref = C.CDLL(LIBS[name])
    ref.ref_variant.restype = C.c_int
    assert ref.ref_variant() == (1 if name == "b" else 0)
    spec = importlib.util.spec_from_file_location("oracle._reference_%s" % name, os.path.join(_HERE, "oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod._lib = _Lib(ref, ora.lib())
    mod.CSC = ora.CSC           # one CSC class for both
    mod.transpose = ora.transpose
    _extend(mod, ref)
    mod.variant_name = name
    _variants[name] = mod
    return mod


def printed_tol(tol):
    """The tolerances as the reference prints them ("%8.2e"), for comparing a full-precision trace with a printed one."""
    return ["%8.2e" % float("%8.2e" % t) for t in np.asarray(tol, dtype=np.float64)]


def _p(a, t):
    return a.ctypes.data_as(t)


def _extend(mod, ref):
    """The entries without an ora_* counterpart (oracle.py composes them, or tests/ restates them in numpy)."""
    csc = [_f64p, _i32p, _i32p]
    ref.ref_rcpp_predict.restype = C.c_int
    ref.ref_rcpp_predict.argtypes = csc + [C.c_int32, C.c_int32, _f64p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int, _f64p]
    ref.ref_predict_dense.restype = None
    ref.ref_predict_dense.argtypes = [_f64p, C.c_int32, C.c_int32, _f64p, _f64p, C.c_int, C.c_double, C.c_double, C.c_int]
    ref.ref_c_gcnmf.restype = C.c_int
    ref.ref_c_gcnmf.argtypes = csc * 3 + [C.c_int32, C.c_int32, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, _f64p,
                                          C.c_int32, C.c_int32, _f64p, _f64p, _f64p, _f64p, _i32p]
    ref.ref_spatial_graph.restype = C.c_int64
    ref.ref_spatial_graph.argtypes = [_f64p, _f64p, C.c_int64, C.c_double, C.c_int64, _i32p, _i32p, _f64p]
    ref.ref_rowwise_compress_sparse.restype = C.c_int
    ref.ref_rowwise_compress_sparse.argtypes = csc + [C.c_int32, C.c_int32, C.c_int64, _f64p]
    ref.ref_rowwise_compress_dense.restype = C.c_int
    ref.ref_rowwise_compress_dense.argtypes = [_f64p, C.c_int32, C.c_int32, C.c_int64, _f64p]

    def ptrs(A):
        return _p(A.x, _f64p), _p(A.i, _i32p), _p(A.p, _i32p)

    def rcpp_predict(A, w, L1, L2, threads=0):
        """Rcpp_predict run as written (its own transposition rule).  w in R orientation; returns h (n, k)."""
        w = np.asarray(w, dtype=np.float64)
        wf = np.ascontiguousarray(w.T)
        h = np.empty((A.ncol, max(w.shape)))
        k = ref.ref_rcpp_predict(*ptrs(A), A.nrow, A.ncol, _p(wf, _f64p), w.shape[0], w.shape[1], L1, L2, threads, _p(h, _f64p))
        return h.ravel()[:A.ncol * k].reshape(A.ncol, k).copy()

    def predict_dense(A, F, X, L1=0.0, L2=0.0, threads=0):
        """predict on a dense matrix (rows x cols array); F (rows, k), X (cols, k) warm start."""
        A = np.asarray(A, dtype=np.float64)
        Af = np.ascontiguousarray(A.T)
        F = np.ascontiguousarray(F, dtype=np.float64)
        X = np.array(X, dtype=np.float64, order="C")
        ref.ref_predict_dense(_p(Af, _f64p), A.shape[0], A.shape[1], _p(F, _f64p), _p(X, _f64p), F.shape[1], L1, L2, threads)
        return X

    def c_gcnmf(A, At, G, tol, maxit, L1, L2, w, threads=0):
        """c_gcnmf.  w: 2-D array in R orientation (k x m, or m x k which the reference transposes when m != k).
        Returns w (m, k), d, h (n, k), iter, tol (printed)."""
        w = np.asarray(w, dtype=np.float64)
        wf = np.ascontiguousarray(w.T)
        m, n = A.nrow, A.ncol
        cap = max(w.shape)
        w_out, h, d = np.empty(m * cap), np.empty(n * cap), np.empty(cap)
        tr = np.zeros(max(int(maxit), 1))
        k = C.c_int32(0)
        it = ref.ref_c_gcnmf(*ptrs(A), *ptrs(At), *ptrs(G), m, n, tol, int(maxit), L1, L2, threads, _p(wf, _f64p), w.shape[0],
                             w.shape[1], _p(w_out, _f64p), _p(h, _f64p), _p(d, _f64p), _p(tr, _f64p), C.byref(k))
        k = k.value
        # w_out is m x k column-major == (k, m) C-order
        return dict(w=w_out[:m * k].reshape(k, m).T.copy(), d=d[:k].copy(), h=h[:n * k].reshape(n, k).copy(), iter=it,
                    tol=tr[:it].copy())

    def spatial_graph(c1, c2, max_dist, max_k=100):
        """(p, i, x) of the n x n graph, as tests/spatial_graph_restatement.brute returns them."""
        c1 = np.ascontiguousarray(c1, dtype=np.float64).ravel()
        c2 = np.ascontiguousarray(c2, dtype=np.float64).ravel()
        n = c1.size
        p = np.zeros(n + 1, dtype=np.int32)
        i = np.zeros(max(n * int(max_k), 1), dtype=np.int32)
        x = np.zeros(max(n * int(max_k), 1))
        nnz = ref.ref_spatial_graph(_p(c1, _f64p), _p(c2, _f64p), n, float(max_dist), int(max_k), _p(p, _i32p), _p(i, _i32p),
                                    _p(x, _f64p))
        return p, i[:nnz].copy(), x[:nnz].copy()

    def rowwise_compress_sparse(A, n):
        """floor(nrow / n) x ncol Fortran-ordered array, or None where the reference indexes outside a matrix."""
        out = np.zeros((A.nrow // n, A.ncol), order="F")
        bad = ref.ref_rowwise_compress_sparse(*ptrs(A), A.nrow, A.ncol, int(n), _p(out, _f64p))
        return None if bad else out

    def rowwise_compress_dense(A, n):
        A = np.asfortranarray(A, dtype=np.float64)
        out = np.zeros((A.shape[0] // n, A.shape[1]), order="F")
        bad = ref.ref_rowwise_compress_dense(_p(A, _f64p), A.shape[0], A.shape[1], int(n), _p(out, _f64p))
        return None if bad else out

    for f in (rcpp_predict, predict_dense, c_gcnmf, spatial_graph, rowwise_compress_sparse, rowwise_compress_dense):
        setattr(mod, f.__name__, f)
