"""The R .Call shim (singlet_amd/r/singlet_hip_shim.c, singlet_hip_graph_shim.c) executed under the emulated R C API of
tests/r_emul/, without a device: the emulator's own behaviour on hand-made objects (collection at every allocation, the
protect stack, non-local exits, scalar conversions), the registration table, and every refusal the two files raise before
they reach the library.  Each refusal must come back as an R error with the quoted text, leave the protect stack at its
depth at entry and touch no collected object.  The calls that reach the GPU are in test_gpu_r_shim.py.

One Rf_error site is not reached: "too many points for a dgCMatrix" of _singlet_spatial_graph needs a vector of 2^31
elements."""
import re

import numpy as np
import pytest

import r_shim_emul as R


@pytest.fixture()
def rs():
    s = R.Session()
    yield s
    s.close()


# ---- the emulator itself --------------------------------------------------------------------------------------------------
def test_torture_poisons_an_unprotected_vector_at_the_next_allocation(rs):
    L = rs.L
    v = L.emul_make_real(np.arange(3.0).ctypes.data_as(R._f64p), 3)   # not protected
    assert L.emul_alive(v) and np.array_equal(rs.values(v), [0.0, 1.0, 2.0])
    L.Rf_allocVector(R.INTSXP, 1)
    assert not L.emul_alive(v)
    got = rs.values(v)
    assert np.isnan(got).all() and np.all(got.view(np.uint64) == 0x7FF4DEADDEADDEAD)   # the signalling pattern


def test_torture_spares_protected_and_reachable_objects(rs):
    L = rs.L
    v = rs.real([1.5, 2.5])                                   # protected by the session
    obj = rs.s4("dgCMatrix")
    x = L.emul_make_real(np.ones(4).ctypes.data_as(R._f64p), 4)
    L.emul_set_slot(obj, b"x", x)                             # reachable through a slot of a protected object only
    lst = rs.rlist([R.nil()])
    inner = L.emul_make_int(np.arange(2, dtype=np.int32).ctypes.data_as(R._i32p), 2)
    L.SET_VECTOR_ELT(lst, 0, inner)                           # ... through a list element
    m = L.Rf_protect(L.Rf_allocMatrix(R.REALSXP, 2, 3))       # its dim attribute is reachable through it
    for _ in range(3):
        L.Rf_allocVector(R.REALSXP, 8)
    assert L.emul_alive(v) and L.emul_alive(x) and L.emul_alive(inner) and L.emul_alive(lst) and L.emul_alive(obj)
    assert np.array_equal(rs.values(v), [1.5, 2.5]) and np.array_equal(rs.values(rs.slot(obj, "x")), np.ones(4))
    assert rs.dim(m) == (2, 3) and L.Rf_isMatrix(m) and L.Rf_nrows(m) == 2 and L.Rf_ncols(m) == 3
    L.Rf_unprotect(1)                                         # m leaves the stack: the next allocation takes it
    L.Rf_allocVector(R.REALSXP, 1)
    assert not L.emul_alive(m) and L.emul_alive(v)


def test_torture_spares_a_vector_reachable_from_an_arguments_slot(rs):
    """During a call the arguments are roots although nothing protects them: an entry that allocates must not poison the
    x slot of its argument (here the arguments are taken off the protect stack first)."""
    L = rs.L
    A = rs.dgc([1.0, 2.0], [0, 1], [0, 1, 2], (2, 2))
    x = rs.slot(A, "x")
    n = rs.integer(3)
    L.Rf_unprotect(2)
    before = L.emul_object_count()
    r = rs.call("emul_selftest_toplevel", n, A, A)           # allocates its result
    assert r.kind == R.OK and L.emul_object_count() == before + 1
    assert L.emul_alive(A) and L.emul_alive(x) and np.array_equal(rs.values(x), [1.0, 2.0]) and L.emul_alive(n)
    assert r.events == []
    L.Rf_allocVector(R.REALSXP, 1)           # after the call nothing holds them
    assert not L.emul_alive(A) and not L.emul_alive(x) and not L.emul_alive(n)
    assert L.emul_alive(r.value)             # the last value stays reachable until the next call


def test_rf_error_returns_the_message_and_resets_the_protect_stack(rs):
    base = rs.L.emul_protect_depth()
    a = rs.integer(7)
    r = rs.call("emul_selftest_error", a, a, a)
    assert r.value is None and r.kind == R.ERROR and r.message == "self-test error 7: as asked"
    assert r.protect_delta_at_exit == 2      # the entry held two objects when it raised ...
    assert r.protect_delta == 0 and rs.L.emul_protect_depth() == base + 1   # ... and R unwound them
    assert r.ralloc_blocks == 0              # R_alloc memory ends with the call


def test_protect_imbalance_of_an_entry_is_visible(rs):
    r = rs.call("emul_selftest_leak", rs.logical(1), rs.logical(0), rs.logical(0))
    assert r.kind == R.OK and r.protect_delta == 1
    r = rs.call("emul_selftest_leak", rs.logical(0), rs.logical(0), rs.logical(0))
    assert r.kind == R.OK and r.protect_delta == 0


def test_toplevel_exec_is_false_only_when_an_interrupt_is_armed(rs):
    n = rs.integer(4)
    r = rs.call("emul_selftest_toplevel", n, n, n)
    assert r.kind == R.OK and list(rs.values(r.value)) == [1, 1, 1, 1] and r.polls == 4
    rs.L.emul_arm_interrupt(3)               # pending from the third poll on
    r = rs.call("emul_selftest_toplevel", n, n, n)
    assert r.kind == R.OK and list(rs.values(r.value)) == [1, 1, 0, 0] and r.polls == 4
    assert r.protect_delta == 0 and r.events == []
    rs.L.emul_arm_interrupt(0)
    r = rs.call("emul_selftest_toplevel", n, n, n)
    assert list(rs.values(r.value)) == [1, 1, 1, 1]


def test_scalar_conversions(rs):
    L = rs.L
    d100, i100, t = rs.real(100.0), rs.integer(100), rs.logical(1)
    assert L.Rf_asInteger(d100) == 100 and L.Rf_asInteger(i100) == 100 and L.Rf_asInteger(t) == 1   # maxit = 100 is a double in R
    assert L.Rf_asReal(d100) == 100.0 and L.Rf_asReal(i100) == 100.0 and L.Rf_asReal(t) == 1.0
    assert L.Rf_asLogical(d100) == 1 and L.Rf_asLogical(i100) == 1 and L.Rf_asLogical(t) == 1
    assert L.Rf_asLogical(rs.real(0.0)) == 0 and L.Rf_asLogical(rs.integer(0)) == 0
    assert L.Rf_asInteger(rs.real(2.9)) == 2 and L.Rf_asInteger(rs.real(-2.9)) == -2
    na = rs.integer(R.NA_INTEGER)
    assert np.isnan(L.Rf_asReal(na)) and L.Rf_asInteger(na) == R.NA_INTEGER and L.Rf_asLogical(na) == R.NA_INTEGER
    assert np.isnan(L.Rf_asReal(rs.logical(R.NA_INTEGER)))
    assert L.Rf_asInteger(rs.real(np.nan)) == R.NA_INTEGER and L.Rf_asInteger(rs.real(3e9)) == R.NA_INTEGER
    assert L.Rf_asReal(rs.real(2.0**32 + 5)) == 2.0**32 + 5
    assert np.isnan(L.Rf_asReal(rs.real([]))) and np.isnan(L.Rf_asReal(rs.string("a")))
    v = rs.real([1.0, 2.0, 3.0])             # a plain vector: no matrix, nrows = length, ncols = 1
    assert not L.Rf_isMatrix(v) and L.Rf_nrows(v) == 3 and L.Rf_ncols(v) == 1
    M = rs.matrix(np.arange(6.0).reshape(2, 3))
    assert L.Rf_isMatrix(M) and (L.Rf_nrows(M), L.Rf_ncols(M)) == (2, 3)
    assert np.array_equal(rs.values(M), [0, 3, 1, 4, 2, 5]) and np.array_equal(rs.as_matrix(M), np.arange(6.0).reshape(2, 3))
    A = rs.dgc([1.0], [0], [0, 1], (1, 1))
    assert L.R_has_slot(A, L.Rf_install(b"Dim")) and not L.R_has_slot(A, L.Rf_install(b"Dimnames"))
    assert rs.class_name(A) == "dgCMatrix" and rs.typeof(A) == R.S4SXP


def test_use_after_collection_is_recorded_for_an_offender(rs):
    a = rs.integer(0)
    r = rs.call("emul_selftest_use_after", a, a, a)
    assert r.kind == R.OK                    # nothing aborts: the offence is an event
    assert r.events == ["use after collection: REAL"]
    assert np.isnan(rs.values(r.value)[0])   # what the offender read was the poison


def test_an_r_error_outside_a_call_is_an_event_not_an_abort(rs):
    """The driver calls a few API functions directly; where one of them raises an R error there is no .Call to unwind to:
    the error is recorded and the function returns a harmless value."""
    L = rs.L
    A = rs.dgc([1.0], [0], [0, 1], (1, 1))
    L.emul_clear_events()
    assert L.Rf_nrows(A) == 0 and L.Rf_ncols(A) == 0          # "object is not a matrix"
    assert L.Rf_allocVector(R.REALSXP, -1) == R.nil()
    assert L.Rf_allocVector(99, 1) == R.nil()
    assert L.Rf_allocMatrix(R.REALSXP, -2, 3) == R.nil()
    assert L.SET_VECTOR_ELT(rs.rlist([]), 0, A) == A           # subscript out of bounds: nothing is written
    got = [L.emul_event(q).decode() for q in range(L.emul_event_count())]
    assert len(got) == 6 and all(g.startswith("R error outside a call: ") for g in got), got
    assert "object is not a matrix" in got[0] and "negative length" in got[2] and "not emulated" in got[3]
    assert "out of bounds" in got[5]
    L.emul_arm_interrupt(1)
    n = rs.integer(1)
    r = rs.call("emul_selftest_toplevel", n, n, n)             # and the session goes on working
    assert r.kind == R.OK and list(rs.values(r.value)) == [0]


# ---- registration -----------------------------------------------------------------------------------------------------------
ARITY = {"_singlet_weight_by_split": 3, "_singlet_c_nmf": 11, "_singlet_c_ard_nmf": 13, "_singlet_c_linked_nmf": 11,
         "_singlet_c_gcnmf": 10, "_singlet_c_nmf_dense": 11, "_singlet_c_nmf_sparse_list": 9,
         "_singlet_c_ard_nmf_sparse_list": 13, "_singlet_c_ard_nmf_dense": 13, "_singlet_c_project_model": 5,
         "_singlet_Rcpp_predict": 5, "_singlet_c_LKNN": 10, "_singlet_c_SNN": 3, "_singlet_spatial_graph": 5,
         "_singlet_rowwise_compress_sparse": 3, "_singlet_rowwise_compress_dense": 3}


def test_registration_table(rs):
    L = rs.L
    got = {L.emul_entry_name(q).decode(): L.emul_entry_arity(q) for q in range(L.emul_entry_count())}
    assert got == ARITY and len(got) == 16
    assert L.emul_dynamic_symbols() == 0     # R_useDynamicSymbols(dll, FALSE)
    src = open(R.os.path.join(R.HERE, "..", "singlet_amd", "r", "singlet_hip_shim.c")).read()
    assert got == {m.group(1): int(m.group(2)) for m in re.finditer(r'\{"(\w+)",\s*\(DL_FUNC\)&\1,\s*(\d+)\}', src)}


def test_a_call_with_a_wrong_argument_count_is_refused(rs):
    z = rs.real(0.0)
    for name, arity in ARITY.items():
        for n in (arity - 1, arity + 1):
            r = rs.call(name, *([z] * n))
            assert r.kind == R.REFUSED and r.value is None and str(arity) in r.message, (name, n)
    r = rs.call("_singlet_no_such_entry", z, z, z)
    assert r.kind == R.REFUSED and "not available" in r.message


# ---- the shim's refusals ----------------------------------------------------------------------------------------------------
M_, N_, K_ = 5, 7, 3


class Args:
    """Well-formed arguments of every entry on a 5 x 7 matrix, rank 3; a case replaces the one it breaks."""

    def __init__(self, rs):
        self.rs = rs
        rng = np.random.default_rng(0)
        D = rng.random((M_, N_)) + 0.1
        self.D = D
        self.A = self.dgc_of(D)
        self.At = self.dgc_of(D.T)
        self.G = self.dgc_of(np.eye(N_))
        self.w = rs.matrix(rng.random((K_, M_)))
        self.lh = rs.matrix(rng.random((K_, N_)))
        self.lw = rs.matrix(rng.random((K_, M_)))
        self.dense = rs.matrix(D)
        cuts = [0, 3, 4, N_]
        self.chunks = rs.rlist([self.dgc_of(D[:, a:b]) for a, b in zip(cuts, cuts[1:])])
        self.tchunks = rs.rlist([self.dgc_of(D.T[:, :2]), self.dgc_of(D.T[:, 2:])])
        self.tol, self.maxit, self.F, self.z, self.one = rs.real(0.0), rs.real(2.0), rs.logical(0), rs.real(0.0), rs.real(1.0)
        self.seed, self.invd, self.thr, self.trace = rs.real(7.0), rs.real(4.0), rs.real(1e9), rs.real(1.0)
        self.split = rs.integer(np.arange(N_) % 2)
        self.groups = rs.integer(2)
        self.cx, self.cy = rs.real(np.arange(N_, dtype=float)), rs.real(np.zeros(N_))
        self.emb = rs.matrix(rng.random((2, N_)))
        self.metric = rs.string("euclidean")
        self.T = rs.logical(1)

    def dgc_of(self, D):
        D = np.asarray(D, dtype=np.float64)
        cols = [np.nonzero(D[:, j])[0] for j in range(D.shape[1])]
        p = np.concatenate([[0], np.cumsum([c.size for c in cols])])
        i = np.concatenate(cols) if cols else np.zeros(0)
        x = np.concatenate([D[c, j] for j, c in enumerate(cols)]) if cols else np.zeros(0)
        return self.rs.dgc(x, i, p, D.shape)

    def of(self, entry, **kw):
        a = dict(vars(self))
        a.update(kw)
        g = a.get
        fit = [g("tol"), g("maxit"), g("F")]
        if entry == "c_nmf":
            return [g("A"), g("At")] + fit + [g("z"), g("z"), g("z"), g("z"), g("z"), g("w")]
        if entry == "c_nmf_dense":
            return [g("dense"), g("z")] + fit + [g("z"), g("z"), g("z"), g("z"), g("z"), g("w")]
        if entry == "c_linked_nmf":
            return [g("A"), g("At")] + fit + [g("z"), g("z"), g("z"), g("w"), g("lh"), g("lw")]
        if entry == "c_gcnmf":
            return [g("A"), g("At"), g("G")] + fit + [g("z"), g("z"), g("z"), g("w")]
        if entry == "c_nmf_sparse_list":
            return [g("chunks"), g("tchunks")] + fit + [g("z"), g("z"), g("z"), g("w")]
        tail = [g("z"), g("z"), g("z"), g("w"), g("seed"), g("invd"), g("thr"), g("trace")]
        if entry == "c_ard_nmf":
            return [g("A"), g("At")] + fit + tail
        if entry == "c_ard_nmf_dense":
            return [g("dense"), g("z")] + fit + tail
        if entry == "c_ard_nmf_sparse_list":
            return [g("chunks"), g("tchunks")] + fit + tail
        if entry in ("c_project_model", "Rcpp_predict"):
            return [g("A"), g("w"), g("z"), g("z"), g("z")]
        if entry == "weight_by_split":
            return [g("A"), g("split"), g("groups")]
        if entry in ("rowwise_compress_sparse", "rowwise_compress_dense"):
            return [g("A") if entry.endswith("sparse") else g("dense"), g("n", self.one), g("z")]
        if entry == "c_LKNN":
            return [g("emb"), g("cx"), g("cy"), g("one"), g("one"), g("metric"), g("T"), g("z"), g("F"), g("z")]
        if entry == "c_SNN":
            return [g("G"), g("z"), g("z")]
        if entry == "spatial_graph":
            return [g("cx"), g("cy"), g("one"), g("max_k", self.one), g("z")]
        raise KeyError(entry)


@pytest.fixture()
def args(rs):
    return Args(rs)


def refused(rs, args, entry, text, **kw):
    name = "_singlet_" + entry
    base = rs.L.emul_protect_depth()
    r = rs.call(name, *args.of(entry, **kw))
    assert r.kind == R.ERROR and r.value is None, (entry, kw.keys(), r.kind, r.message)
    assert text in r.message, (entry, r.message)
    assert r.protect_delta == 0 and rs.L.emul_protect_depth() == base
    assert r.events == [] and r.ralloc_blocks == 0
    return r


SPARSE_ENTRIES = ("c_nmf", "c_ard_nmf", "c_linked_nmf", "c_gcnmf", "c_project_model", "Rcpp_predict", "weight_by_split",
                  "rowwise_compress_sparse")
FIT_ENTRIES = ("c_nmf", "c_ard_nmf", "c_linked_nmf", "c_nmf_dense", "c_nmf_sparse_list", "c_ard_nmf_sparse_list", "c_ard_nmf_dense")


@pytest.mark.parametrize("entry", SPARSE_ENTRIES)
def test_refuses_a_dgcmatrix_without_a_slot_or_with_wrong_slot_types(rs, args, entry):
    x, i, p, dim = rs.real([1.0]), rs.integer([0]), rs.integer([0, 1] + [1] * (N_ - 1)), rs.integer([M_, N_])
    for missing in ("x", "i", "p", "Dim"):
        slots = {k: v for k, v in dict(x=x, i=i, p=p, Dim=dim).items() if k != missing}
        refused(rs, args, entry, "A: not a dgCMatrix (missing slot)", A=rs.s4("dgCMatrix", **slots))
    refused(rs, args, entry, "A: not a dgCMatrix (missing slot)", A=rs.matrix(args.D))   # no S4 object at all
    bad = [dict(x=rs.integer([1])), dict(i=rs.real([0.0])), dict(p=rs.real([0.0, 1.0])), dict(Dim=rs.real([5.0, 7.0])),
           dict(Dim=rs.integer([M_, N_, 1]))]
    for b in bad:
        slots = dict(x=x, i=i, p=p, Dim=dim)
        slots.update(b)
        refused(rs, args, entry, "A: not a dgCMatrix (slot types)", A=rs.s4("dgCMatrix", **slots))


@pytest.mark.parametrize("entry", SPARSE_ENTRIES)
def test_refuses_a_dgcmatrix_with_short_slots(rs, args, entry):
    """The library reads p[0..ncol] and p[ncol] entries of i and x from host memory whose lengths only the shim knows."""
    p_ok = [0, 2] + [2] * (N_ - 1)
    refused(rs, args, entry, "A: not a dgCMatrix (length(p) != ncol + 1)", A=rs.dgc([1.0, 2.0], [0, 1], p_ok[:-1], (M_, N_)))
    refused(rs, args, entry, "A: not a dgCMatrix (length(p) != ncol + 1)", A=rs.dgc([1.0, 2.0], [0, 1], p_ok + [2], (M_, N_)))
    refused(rs, args, entry, "A: not a dgCMatrix (length(p) != ncol + 1)", A=rs.dgc([], [], [], (M_, -1)))
    refused(rs, args, entry, "A: not a dgCMatrix (length(i) != length(x))", A=rs.dgc([1.0, 2.0], [0], p_ok, (M_, N_)))
    refused(rs, args, entry, "A: not a dgCMatrix (length(i) != length(x))", A=rs.dgc([1.0], [0, 1], p_ok, (M_, N_)))
    refused(rs, args, entry, "A: not a dgCMatrix (p[ncol] > length(x))", A=rs.dgc([1.0], [0], p_ok, (M_, N_)))


def test_refuses_short_slots_in_the_other_matrices_and_in_chunks(rs, args):
    p_ok = [0, 2] + [2] * (M_ - 1)
    short = rs.dgc([1.0], [0], p_ok, (N_, M_))
    refused(rs, args, "c_nmf", "At: not a dgCMatrix (p[ncol] > length(x))", At=short)
    refused(rs, args, "c_gcnmf", "G: not a dgCMatrix (length(p) != ncol + 1)", G=rs.dgc([1.0], [0], [0, 1], (N_, N_)))
    for entry in ("c_nmf_sparse_list", "c_ard_nmf_sparse_list"):
        good = args.dgc_of(args.D[:, :3])
        refused(rs, args, entry, "A: not a dgCMatrix (length(i) != length(x))",
                chunks=rs.rlist([good, rs.dgc([1.0, 2.0], [0], [0, 2, 2, 2, 2], (M_, 4))]))
        refused(rs, args, entry, "At: not a dgCMatrix (p[ncol] > length(x))", tchunks=rs.rlist([short]))
        refused(rs, args, entry, "A: not a dgCMatrix (missing slot)", chunks=rs.rlist([good, rs.real(1.0)]))


@pytest.mark.parametrize("entry", FIT_ENTRIES + ("c_gcnmf", "c_project_model", "Rcpp_predict"))
def test_refuses_a_w_that_is_no_numeric_matrix(rs, args, entry):
    refused(rs, args, entry, "w must be a numeric matrix", w=rs.real(np.ones(K_ * M_)))          # no dim
    refused(rs, args, entry, "w must be a numeric matrix", w=rs.int_matrix(np.ones((K_, M_))))   # integer


@pytest.mark.parametrize("entry", FIT_ENTRIES)
def test_refuses_a_w_whose_columns_are_not_the_rows_of_a(rs, args, entry):
    refused(rs, args, entry, "w must be k x nrow(A)", w=rs.matrix(np.ones((M_, K_))))    # the transposed orientation
    refused(rs, args, entry, "w must be k x nrow(A)", w=rs.matrix(np.ones((K_, M_ + 1))))


def test_refuses_links_that_are_not_matrices(rs, args):
    text = "link_h and link_w must be numeric matrices"
    refused(rs, args, "c_linked_nmf", text, lh=rs.real(np.ones(K_ * N_)))
    refused(rs, args, "c_linked_nmf", text, lw=rs.real(np.ones(K_ * M_)))
    refused(rs, args, "c_linked_nmf", text, lh=rs.int_matrix(np.ones((K_, N_))))
    refused(rs, args, "c_linked_nmf", text, lw=rs.int_matrix(np.ones((K_, M_))))


@pytest.mark.parametrize("entry", ["c_nmf_dense", "c_ard_nmf_dense", "rowwise_compress_dense"])
def test_refuses_a_dense_a_that_is_no_matrix(rs, args, entry):
    refused(rs, args, entry, "A must be a numeric matrix", dense=rs.real(np.ones(M_ * N_)))
    refused(rs, args, entry, "A must be a numeric matrix", dense=args.A)
    if entry != "rowwise_compress_dense":    # which takes an integer matrix
        refused(rs, args, entry, "A must be a numeric matrix", dense=rs.int_matrix(np.ones((M_, N_))))
    else:
        refused(rs, args, entry, "A must be a numeric matrix", dense=rs.rlist([]))


@pytest.mark.parametrize("entry", ["c_nmf_sparse_list", "c_ard_nmf_sparse_list"])
def test_refuses_bad_chunk_lists(rs, args, entry):
    refused(rs, args, entry, "A: not a non-empty list of dgCMatrix", chunks=rs.rlist([]))
    refused(rs, args, entry, "A: not a non-empty list of dgCMatrix", chunks=args.A)
    refused(rs, args, entry, "At: not a non-empty list of dgCMatrix", tchunks=rs.rlist([]))
    refused(rs, args, entry, "At: not a non-empty list of dgCMatrix", tchunks=rs.real(1.0))
    taller = args.dgc_of(np.ones((M_ + 1, 2)))
    refused(rs, args, entry, "A: chunks differ in their number of rows", chunks=rs.rlist([args.dgc_of(args.D[:, :5]), taller]))
    refused(rs, args, entry, "At: chunks differ in their number of rows",
            tchunks=rs.rlist([args.dgc_of(args.D.T[:, :2]), args.dgc_of(np.ones((N_ + 1, 3)))]))
    # the columns of A's chunks against nrow(At[[1]]): h is allocated from the second, written to the extent of the first
    r = refused(rs, args, entry, "the chunks of A hold 5 columns in all but the chunks of At have 7 rows",
                chunks=rs.rlist([args.dgc_of(args.D[:, :3]), args.dgc_of(args.D[:, 3:5])]))
    assert r.message == "the chunks of A hold 5 columns in all but the chunks of At have 7 rows"


def test_refuses_a_bad_split_by(rs, args):
    text = "split_by must be an integer vector with one entry per column of A"
    refused(rs, args, "weight_by_split", text, split=rs.real(np.zeros(N_)))
    refused(rs, args, "weight_by_split", text, split=rs.integer(np.zeros(N_ - 1)))
    refused(rs, args, "weight_by_split", text, split=rs.integer(np.zeros(N_ + 1)))


@pytest.mark.parametrize("entry", ["rowwise_compress_sparse", "rowwise_compress_dense"])
def test_refuses_a_bad_bin_size(rs, args, entry):
    text = "rowwise_compress: n must be a number >= 1 (the bin size)"
    for n in (rs.integer(R.NA_INTEGER), rs.real(np.nan), rs.real(0.0), rs.integer(0), rs.real(0.5), rs.real(-3.0)):
        refused(rs, args, entry, text, n=n)


def test_refuses_bad_lknn_arguments(rs, args):
    refused(rs, args, "c_LKNN", "m must be a numeric matrix", emb=rs.real(np.ones(N_)))
    refused(rs, args, "c_LKNN", "m must be a numeric matrix", emb=rs.int_matrix(np.ones((2, N_))))
    refused(rs, args, "c_LKNN", "coordinates must be numeric vectors", cx=rs.integer(np.arange(N_)))
    refused(rs, args, "c_LKNN", "coordinates must be numeric vectors", cy=rs.integer(np.arange(N_)))
    refused(rs, args, "c_LKNN", "metric must be a string", metric=rs.real(1.0))
    refused(rs, args, "c_LKNN", "metric must be a string", metric=rs.L.Rf_protect(rs.L.Rf_allocVector(R.STRSXP, 0)))
    refused(rs, args, "c_LKNN", "length of coordinate vectors must be equivalent", cy=rs.real(np.zeros(N_ - 1)))
    text = "number of columns in 'm' must be equal to number of coordinates"
    refused(rs, args, "c_LKNN", text, emb=rs.matrix(np.ones((2, N_ + 1))))
    refused(rs, args, "c_LKNN", text, emb=rs.matrix(np.ones((N_ + 1, N_ + 2))))
    refused(rs, args, "c_LKNN", text, cx=rs.real(np.zeros(N_ - 1)), cy=rs.real(np.zeros(N_ - 1)))


def test_refuses_bad_snn_arguments(rs, args):
    i, p, dim = rs.integer([0]), rs.integer([0, 1] + [1] * (N_ - 1)), rs.integer([N_, N_])
    for missing in ("i", "p", "Dim"):
        slots = {k: v for k, v in dict(i=i, p=p, Dim=dim).items() if k != missing}
        refused(rs, args, "c_SNN", "G: not a dgCMatrix (missing slot)", G=rs.s4("dgCMatrix", **slots))
    for b in (dict(i=rs.real([0.0])), dict(p=rs.real([0.0])), dict(Dim=rs.real([7.0, 7.0])), dict(Dim=rs.integer([N_]))):
        slots = dict(i=i, p=p, Dim=dim)
        slots.update(b)
        refused(rs, args, "c_SNN", "G: not a dgCMatrix (slot types)", G=rs.s4("dgCMatrix", **slots))
    refused(rs, args, "c_SNN", "G: not a dgCMatrix (length(p) != ncol + 1)", G=rs.s4("dgCMatrix", i=i, p=rs.integer([0, 1]), Dim=dim))
    refused(rs, args, "c_SNN", "G: not a dgCMatrix (length(p) != ncol + 1)",
            G=rs.s4("dgCMatrix", i=i, p=rs.integer([0, 1] + [1] * N_), Dim=dim))
    refused(rs, args, "c_SNN", "G: not a dgCMatrix (length(p) != ncol + 1)",
            G=rs.s4("dgCMatrix", i=i, p=rs.integer([]), Dim=rs.integer([N_, -1])))
    refused(rs, args, "c_SNN", "G: not a dgCMatrix (p[ncol] > length(i))",       # the library would read i[0..1]
            G=rs.s4("dgCMatrix", i=i, p=rs.integer([0, 2] + [2] * (N_ - 1)), Dim=dim))


def test_refuses_bad_spatial_graph_arguments(rs, args):
    text = "spatial_graph: max_k must be a non-negative number"
    for k in (rs.integer(R.NA_INTEGER), rs.real(np.nan), rs.real(-1.0), rs.integer(-5)):
        refused(rs, args, "spatial_graph", text, max_k=k)
    refused(rs, args, "spatial_graph", "spatial_graph: c1 and c2 differ in length", cy=rs.real(np.zeros(N_ - 1)))
    refused(rs, args, "spatial_graph", "spatial_graph: c1 and c2 differ in length", cx=rs.integer(np.arange(N_ + 1)))
    refused(rs, args, "spatial_graph", "c1 must be a numeric vector", cx=rs.string("a"))
    refused(rs, args, "spatial_graph", "c2 must be a numeric vector", cy=rs.logical([1] * N_))


def test_the_shared_object_is_a_build_product(monkeypatch):
    """Without it the tests fail with an instruction; they neither skip nor compile."""
    monkeypatch.setattr(R, "_lib", None)
    monkeypatch.setattr(R, "SO_PATH", R.os.path.join(R.HERE, "r_emul", "no_such_library.so"))
    with pytest.raises(RuntimeError, match=r"run build\(\)"):
        R.load()
