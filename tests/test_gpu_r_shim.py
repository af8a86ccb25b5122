"""The R .Call shim (singlet_amd/r/singlet_hip_shim.c, singlet_hip_graph_shim.c) executed on the GPU under the emulated R
C API of tests/r_emul/: all 16 registered entries, called as R calls them.

Every case builds its inputs twice from one numpy source -- as emulated R objects, and as the arguments of the Python mirror
(singlet_amd/api.py) -- and holds the shim's result, read back through R's layout,
  - bit for bit against the mirror's: both reach one C entry of one library with the same bytes, and the library's
    reductions are run-to-run deterministic.  Each case first calls the mirror twice and asserts that the two results are the
    same bits, so a difference between shim and mirror is the shim's (all 16 entries are reproducible in that sense: c_nmf,
    c_ard_nmf, c_linked_nmf, c_gcnmf, c_nmf_dense, c_nmf_sparse_list, c_ard_nmf_sparse_list, c_ard_nmf_dense,
    c_project_model, Rcpp_predict, weight_by_split, rowwise_compress_sparse, rowwise_compress_dense, c_LKNN, c_SNN,
    spatial_graph);
  - against the reference the existing GPU test of the same entry uses, with that test's tolerance and zero-pattern
    assertion: oracle.oracle at 1e-9 relative Frobenius error + same_zero_pattern (test_gpu_nmf.py: _check, TOL); the trace
    vectors as test_c_ard_nmf_parity; gcnmf_restatement at 1e-9 (test_gpu_gcnmf.py: _check); oracle.weight_by_split at 1e-14
    (test_gpu_ops.py: test_weight_by_split_one_shot); rowwise_compress_restatement, local_neighbors_restatement and
    spatial_graph_restatement bit for bit (the _same of test_gpu_rasterize.py, test_gpu_local_neighbors.py,
    test_gpu_spatial_graph.py).
Structure on every case: result type, dim, list names in the order the shim cites from the reference, integer `iter`,
protect balance 0, no use of a collected object.

Each test declares the entries it calls (@covers); the last test holds the union against the registration table, so an
entry registered later without a case fails here."""
import ctypes as C

import numpy as np
import pytest

import gcnmf_restatement as gr
import local_neighbors_restatement as lr
import r_shim_emul as R
import rowwise_compress_restatement as rr
import spatial_graph_restatement as sr
from conftest import rel_fro, same_zero_pattern, to_dgc

pytestmark = pytest.mark.gpu
TOL = 1e-9   # test_gpu_nmf.py / test_gpu_gcnmf.py
M, N, K = 37, 53, 5

COVERED = {}


def covers(*entries):
    def deco(fn):
        fn._covers = tuple("_singlet_" + e for e in entries)
        for e in fn._covers:
            COVERED.setdefault(e, []).append(fn.__name__)
        return fn
    return deco


class Shim:
    def __init__(self, rs, declared):
        self.rs, self.declared, self.called = rs, set(declared), set()

    def call(self, entry, *args, ok=True):
        name = "_singlet_" + entry
        assert name in self.declared, "%s is not declared by @covers" % name
        self.called.add(name)
        base = self.rs.L.emul_protect_depth()
        r = self.rs.call(name, *args)
        if ok:
            assert r.kind == R.OK, (r.kind, r.message)
            assert r.protect_delta == 0 and r.protect_delta_at_exit == 0 and self.rs.L.emul_protect_depth() == base
            assert r.events == [], r.events
            assert r.ralloc_blocks == 0
            assert self.rs.L.emul_alive(r.value)
        return r


@pytest.fixture()
def rs():
    s = R.Session()
    yield s
    s.close()


@pytest.fixture()
def shim(rs, request, sa):
    s = Shim(rs, getattr(request.function, "_covers", ()))
    failed = request.session.testsfailed
    yield s
    if request.session.testsfailed == failed:   # a test that passed called everything it declares
        assert s.called == s.declared, (s.called, s.declared)


@pytest.fixture(scope="module")
def data(ora):
    """One small problem, shared: 37 x 53, rank 5, a third of the entries stored."""
    A = ora.synth_csc(M, N, 3)
    w0 = ora.synth_winit(K, M)             # the oracle's form, m x k; R's w is its transpose, k x m
    assert w0.shape == (M, K)
    return {"A": A, "At": A.t(), "w0": w0, "wR": np.ascontiguousarray(w0.T), "D": A.to_dense()}


# ---- helpers: one numpy source, two sets of arguments ---------------------------------------------------------------------
def r_dgc(rs, A):
    return rs.dgc(A.x, A.i, A.p, (A.nrow, A.ncol))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def twice(fn):
    """the mirror's result, after checking that a second identical call gives the same bits"""
    a, b = fn(), fn()
    if isinstance(a, dict):
        for key in a:
            if isinstance(a[key], np.ndarray) and a[key].dtype.kind == "f":
                assert same_bits(a[key], b[key]), key
            else:
                assert np.array_equal(a[key], b[key]), key
    elif isinstance(a, np.ndarray):
        assert same_bits(a, b)
    else:
        assert np.array_equal(a.p, b.p) and np.array_equal(a.i, b.i) and same_bits(a.x, b.x)
    return a


def fit_list(rs, r, names, w_dim, h_dim):
    """The named list of a fit -> {name: array}, after the structure checks: a VECSXP with exactly these names in this order,
    w and h numeric matrices of the given dim, d a numeric vector of length k."""
    v = r.value
    assert rs.typeof(v) == R.VECSXP and rs.length(v) == len(names) and rs.names(v) == list(names)
    assert rs.dim(v) is None
    el = rs.as_dict(v)
    out = {}
    for key, dim in (("w", w_dim), ("h", h_dim)):
        if key in el:
            assert rs.typeof(el[key]) == R.REALSXP and rs.dim(el[key]) == dim, (key, rs.dim(el[key]))
            out[key] = rs.as_matrix(el[key])
    k = (h_dim or w_dim)[0]
    assert rs.typeof(el["d"]) == R.REALSXP and rs.dim(el["d"]) is None and rs.length(el["d"]) == k
    out["d"] = rs.values(el["d"])
    for key in ("test_mse", "iter", "tol", "score_overfit"):
        if key in el:
            assert rs.typeof(el[key]) == (R.INTSXP if key == "iter" else R.REALSXP) and rs.dim(el[key]) is None
            out[key] = rs.values(el[key])
    return out


def same_as_mirror(got, mirror):
    for key in got:
        assert same_bits(got[key], mirror[key]) if got[key].dtype.kind == "f" else np.array_equal(got[key], mirror[key]), key


def check_oracle(got, ref, keys=("w", "h", "d")):
    """test_gpu_nmf.py: _check -- got in R's orientation (w k x m, h k x n), ref (columns, k)"""
    for key in keys:
        g = got[key].T if got[key].ndim == 2 else got[key]
        assert rel_fro(g, ref[key]) < TOL, key
        if g.ndim == 2:
            assert same_zero_pattern(g, ref[key]), key


def check_ard_traces(got, ref):
    """test_gpu_nmf.py: test_c_ard_nmf_parity"""
    assert np.array_equal(got["iter"], ref["iter"])
    assert np.allclose(got["test_mse"], ref["test_mse"], rtol=1e-9, atol=0)
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-7, atol=0)
    assert np.allclose(got["score_overfit"], ref["score_overfit"], rtol=1e-6, atol=1e-12)


NMF_NAMES = ("w", "d", "h")
ARD_NAMES = ("w", "d", "h", "test_mse", "iter", "tol", "score_overfit")   # src/singlet.cpp:1144-1151


def body(text):
    """the lines of a verbose trace after its three header lines"""
    lines = text.splitlines()
    assert lines[0] == "" and set(lines[2]) == {"-"}, lines[:3]
    return lines[1], lines[3:]


# ---- c_nmf ------------------------------------------------------------------------------------------------------------------
@covers("c_nmf")
def test_c_nmf(sa, ora, rs, shim, data, capsys):
    A, At, w0 = data["A"], data["At"], data["w0"]
    wR = data["wR"]
    pen = (0.02, 0.005, 0.01, 0.003)   # L1_w, L1_h, L2_w, L2_h all different: a swapped penalty shows
    mirror = twice(lambda: sa.c_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 4, False, *pen, 0, wR))
    ref = ora.c_nmf(A, At, 0.0, 4, *pen, 0, w0)
    rA, rAt, rw = r_dgc(rs, A), r_dgc(rs, At), rs.matrix(wR)
    scal = [rs.real(v) for v in pen]
    results = []
    for maxit in (rs.real(4.0), rs.integer(4)):   # R hands maxit = 4 over as a double; 4L is an integer
        r = shim.call("c_nmf", rA, rAt, rs.real(0.0), maxit, rs.logical(0), *scal, rs.integer(0), rw)
        assert r.output == "" and r.polls >= 4
        got = fit_list(rs, r, NMF_NAMES, (K, M), (K, N))
        same_as_mirror(got, mirror)
        check_oracle(got, ref)
        results.append(got)
    same_as_mirror(results[0], results[1])
    swapped = sa.c_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 4, False, pen[1], pen[0], pen[3], pen[2], 0, wR)
    assert not same_bits(swapped["h"], mirror["h"])   # the penalties matter at this size
    # verbose = TRUE: the lines Rprintf wrote are the lines the mirror prints
    capsys.readouterr()
    sa.c_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 3, True, *pen, 0, wR)
    want_head, want = body(capsys.readouterr().out)
    r = shim.call("c_nmf", rA, rAt, rs.real(0.0), rs.real(3.0), rs.logical(1), *scal, rs.integer(0), rw)
    head, lines = body(r.output)
    assert head == want_head == "%4s | %8s " % ("iter", "tol")
    assert lines == want and len(lines) == 3 and lines[0].startswith("   1 | ")


# ---- c_ard_nmf and its two other front-ends ---------------------------------------------------------------------------------
SEED = 2**33 + 2**31 + 12345   # above 2^31 and 2^32 (exact as a double): a seed cut to 31 or 32 bits on its way gives another mask
INVD = 5   # not a power of two: the draw is hash % inv_density, and the low two bits of the hash do not depend on the seed's high bits


def ard_cases(sa, ora, rs, data):
    """entry -> (R arguments up to At, the mirror as a function of (maxit, verbose, trace), the oracle likewise, h columns)"""
    import scipy.sparse as sp
    A, At, w0 = data["A"], data["At"], data["w0"]
    wR = data["wR"]
    D = data["D"].copy()
    D[:, 9] = 0.0
    S, St = sp.csc_matrix(D), sp.csc_matrix(D.T)
    dS = sa.dgCMatrix(S.data, S.indices, S.indptr, (M, N))
    dSt = sa.dgCMatrix(St.data, St.indices, St.indptr, (N, M))
    cuts, tcuts = [0, 20, 21, N], [0, 30, M]
    chunks = [dS.col_slice(a, b) for a, b in zip(cuts, cuts[1:])]
    tchunks = [dSt.col_slice(a, b) for a, b in zip(tcuts, tcuts[1:])]
    oc = [ora.CSC(c.x, c.i, c.p, c.nrow, c.ncol) for c in chunks]
    otc = [ora.CSC(c.x, c.i, c.p, c.nrow, c.ncol) for c in tchunks]
    tail = (0.01, 0.0, 0, wR)
    return {
        "c_ard_nmf": (
            lambda: [r_dgc(rs, A), r_dgc(rs, At)],
            lambda maxit, verbose, trace: sa.c_ard_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, maxit, verbose, *tail, SEED, INVD, 1e9, trace),
            lambda maxit, trace: ora.c_ard_nmf(A, At, 0.0, maxit, 0.01, 0.0, 0, w0, SEED, INVD, 1e9, trace)),
        "c_ard_nmf_dense": (
            lambda: [rs.matrix(D), rs.real(0.0)],
            lambda maxit, verbose, trace: sa.c_ard_nmf_dense(D, None, 0.0, maxit, verbose, *tail, SEED, INVD, 1e9, trace),
            lambda maxit, trace: ora.c_ard_nmf_dense(D, 0.0, maxit, 0.01, 0.0, 0, w0, SEED, INVD, 1e9, trace)),
        "c_ard_nmf_sparse_list": (
            lambda: [rs.rlist([rs.dgc(c.x, c.i, c.p, (c.nrow, c.ncol)) for c in chunks]),
                     rs.rlist([rs.dgc(c.x, c.i, c.p, (c.nrow, c.ncol)) for c in tchunks])],
            lambda maxit, verbose, trace: sa.c_ard_nmf_sparse_list(chunks, tchunks, 0.0, maxit, verbose, *tail, SEED, INVD, 1e9, trace),
            lambda maxit, trace: ora.c_ard_nmf_sparse_list(oc, otc, 0.0, maxit, 0.01, 0.0, 0, w0, SEED, INVD, 1e9, trace)),
    }


def _ard(entry, sa, ora, rs, shim, data, capsys):
    head_args, mirror_fn, oracle_fn = ard_cases(sa, ora, rs, data)[entry]
    w0 = data["w0"]
    wR = data["wR"]
    mirror = twice(lambda: mirror_fn(5, False, 2))
    ref = oracle_fn(5, 2)
    first = head_args()
    # seed and inv_density as R gives them: doubles
    common = [rs.real(0.0), rs.real(5.0), rs.logical(0), rs.real(0.01), rs.real(0.0), rs.integer(0), rs.matrix(wR),
              rs.real(float(SEED)), rs.real(float(INVD)), rs.real(1e9), rs.real(2.0)]
    r = shim.call(entry, *first, *common)
    got = fit_list(rs, r, ARD_NAMES, (K, M), (K, N))
    n_trace = len(mirror["iter"])
    assert list(mirror["iter"]) == [0, 2, 4, 5] and all(len(got[key]) == n_trace for key in ("test_mse", "iter", "tol", "score_overfit"))
    same_as_mirror(got, mirror)
    check_oracle(got, ref)
    check_ard_traces(got, ref)
    # verbose: iterations 1 and 3 are traced (a score), iteration 2 prints "-" (trace_test_mse = 2, src/singlet.cpp:1116)
    capsys.readouterr()
    mirror_fn(3, True, 2)
    want_head, want = body(capsys.readouterr().out)
    common[1], common[2] = rs.real(3.0), rs.logical(1)
    r = shim.call(entry, *first, *common)
    head, lines = body(r.output)
    assert head == want_head == "%4s | %8s | %8s " % ("iter", "tol", "overfit")
    assert lines == want and len(lines) == 3
    assert lines[1].endswith("|        -") and "e" in lines[0].split("|")[2] and "e" in lines[2].split("|")[2]


@covers("c_ard_nmf")
def test_c_ard_nmf(sa, ora, rs, shim, data, capsys):
    _ard("c_ard_nmf", sa, ora, rs, shim, data, capsys)
    # the seed arrives whole: its low 32 or 31 bits alone select another test set
    A, At, wR = data["A"], data["At"], data["wR"]
    a = sa.c_ard_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 2, False, 0.01, 0.0, 0, wR, SEED, INVD, 1e9, 1)
    for cut in (SEED & 0xffffffff, SEED & 0x7fffffff):
        b = sa.c_ard_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 2, False, 0.01, 0.0, 0, wR, cut, INVD, 1e9, 1)
        assert not same_bits(a["test_mse"], b["test_mse"]), hex(cut)


@covers("c_ard_nmf_dense")
def test_c_ard_nmf_dense(sa, ora, rs, shim, data, capsys):
    _ard("c_ard_nmf_dense", sa, ora, rs, shim, data, capsys)


@covers("c_ard_nmf_sparse_list")
def test_c_ard_nmf_sparse_list(sa, ora, rs, shim, data, capsys):
    _ard("c_ard_nmf_sparse_list", sa, ora, rs, shim, data, capsys)


# ---- c_linked_nmf -----------------------------------------------------------------------------------------------------------
@covers("c_linked_nmf")
@pytest.mark.parametrize("which", ["both", "h_only", "w_only"])
def test_c_linked_nmf(sa, ora, rs, shim, data, which):
    """as test_gpu_nmf.py: test_c_linked_nmf -- a 1 x 1 link has a column count that does not match its side and is ignored"""
    A, At, w0 = data["A"], data["At"], data["w0"]
    wR = data["wR"]
    rng = np.random.default_rng(4)
    lh = (rng.random((K, N)) < 0.7) * (0.5 + rng.random((K, N)))
    lw = (rng.random((K, M)) < 0.8).astype(np.float64)
    off = np.ones((1, 1))
    link_h = lh if which in ("both", "h_only") else off
    link_w = lw if which in ("both", "w_only") else off
    mirror = twice(lambda: sa.c_linked_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 4, False, 0.01, 0.0, 0, wR, link_h, link_w))
    ref = ora.c_linked_nmf(A, At, 0.0, 4, 0.01, 0.0, 0, w0, link_h, link_w)
    r = shim.call("c_linked_nmf", r_dgc(rs, A), r_dgc(rs, At), rs.real(0.0), rs.real(4.0), rs.logical(0), rs.real(0.01),
                  rs.real(0.0), rs.integer(0), rs.matrix(wR), rs.matrix(link_h), rs.matrix(link_w))
    got = fit_list(rs, r, NMF_NAMES, (K, M), (K, N))
    same_as_mirror(got, mirror)
    check_oracle(got, ref)
    if which in ("both", "h_only"):
        assert np.all(got["h"][lh == 0] == 0)


# ---- c_nmf_dense, c_nmf_sparse_list -----------------------------------------------------------------------------------------
@covers("c_nmf_dense")
def test_c_nmf_dense(sa, ora, rs, shim, data):
    D, w0 = data["D"].copy(), data["w0"]
    wR = data["wR"]
    D[:, 11] = 0.0    # an all-zero column is still solved by the dense front-end
    pen = (0.02, 0.005, 0.01, 0.003)
    mirror = twice(lambda: sa.c_nmf_dense(D, None, 0.0, 4, False, *pen, 0, wR))
    ref = ora.c_nmf_dense(D, 0.0, 4, *pen, 0, w0)
    r = shim.call("c_nmf_dense", rs.matrix(D), rs.real(0.0), rs.real(0.0), rs.real(4.0), rs.logical(0), *[rs.real(v) for v in pen],
                  rs.integer(0), rs.matrix(wR))
    got = fit_list(rs, r, NMF_NAMES, (K, M), (K, N))
    same_as_mirror(got, mirror)
    check_oracle(got, ref)


@covers("c_nmf_sparse_list")
def test_c_nmf_sparse_list(sa, ora, rs, shim, data):
    A, At, w0 = data["A"], data["At"], data["w0"]
    wR = data["wR"]
    dA, dAt = to_dgc(sa, A), to_dgc(sa, At)
    cuts, tcuts = [0, 20, 21, N], [0, 1, 30, M]    # three chunks of unequal width, one a single column
    chunks = [dA.col_slice(a, b) for a, b in zip(cuts, cuts[1:])]
    tchunks = [dAt.col_slice(a, b) for a, b in zip(tcuts, tcuts[1:])]
    mirror = twice(lambda: sa.c_nmf_sparse_list(chunks, tchunks, 0.0, 4, False, 0.01, 0.002, 0, wR))
    oc = [ora.CSC(c.x, c.i, c.p, c.nrow, c.ncol) for c in chunks]
    otc = [ora.CSC(c.x, c.i, c.p, c.nrow, c.ncol) for c in tchunks]
    ref = ora.c_nmf_sparse_list(oc, otc, 0.0, 4, 0.01, 0.002, 0, w0)
    r = shim.call("c_nmf_sparse_list", rs.rlist([rs.dgc(c.x, c.i, c.p, (c.nrow, c.ncol)) for c in chunks]),
                  rs.rlist([rs.dgc(c.x, c.i, c.p, (c.nrow, c.ncol)) for c in tchunks]), rs.real(0.0), rs.real(4.0), rs.logical(0),
                  rs.real(0.01), rs.real(0.002), rs.integer(0), rs.matrix(wR))
    got = fit_list(rs, r, NMF_NAMES, (K, M), (K, N))
    same_as_mirror(got, mirror)
    check_oracle(got, ref)


# ---- c_project_model, Rcpp_predict ------------------------------------------------------------------------------------------
@covers("c_project_model")
@pytest.mark.parametrize("orient", ["k_by_m", "m_by_k", "square"])
def test_c_project_model(sa, ora, rs, shim, data, orient):
    """k = ncol(w) when nrow(w) == nrow(A), else nrow(w): the square w is taken as m x k, unlike Rcpp_predict"""
    A = data["A"] if orient != "square" else ora.synth_csc(6, N, 2)
    m = A.nrow
    k = K if orient != "square" else m
    w = np.random.default_rng(1).random((m, k))
    win = w.T.copy() if orient == "k_by_m" else w
    mirror = twice(lambda: sa.c_project_model(to_dgc(sa, A), win, 0.01, 0.002, 0))
    ref = ora.c_project_model(A, win, 0.01, 0.002)
    r = shim.call("c_project_model", r_dgc(rs, A), rs.matrix(win), rs.real(0.01), rs.real(0.002), rs.integer(0))
    got = fit_list(rs, r, ("h", "d"), None, (k, N))
    assert mirror["h"].shape == (k, N)
    same_as_mirror(got, mirror)
    check_oracle(got, ref, ("h", "d"))


@covers("Rcpp_predict")
@pytest.mark.parametrize("shape", [(300, 11), (11, 300), (40, 40)])
def test_rcpp_predict(sa, ora, rs, shim, shape):
    """the three shapes of test_gpu_nmf.py: test_rcpp_predict"""
    A = ora.synth_csc(max(shape), 410, 20)
    w = np.random.default_rng(2).random(shape)
    mirror = twice(lambda: sa.Rcpp_predict(to_dgc(sa, A), w, 0.01, 0.0, 0))
    ref = ora.rcpp_predict(A, w, 0.01, 0.0)
    r = shim.call("Rcpp_predict", r_dgc(rs, A), rs.matrix(w), rs.real(0.01), rs.real(0.0), rs.integer(0))
    k = min(shape) if shape[0] != shape[1] else shape[0]
    assert rs.typeof(r.value) == R.REALSXP and rs.dim(r.value) == (k, 410) and rs.names(r.value) == []
    got = rs.as_matrix(r.value)
    assert same_bits(got, mirror)
    assert rel_fro(got.T, ref) < TOL and same_zero_pattern(got.T, ref)


# ---- weight_by_split --------------------------------------------------------------------------------------------------------
@covers("weight_by_split")
def test_weight_by_split(sa, ora, rs, shim, data):
    A = data["A"]
    sb = np.random.default_rng(5).integers(0, 4, A.ncol).astype(np.int32)
    mirror = twice(lambda: sa.weight_by_split(to_dgc(sa, A), sb, 4))
    ref = ora.weight_by_split(A, sb, 4)
    rA = r_dgc(rs, A)
    x_before = rs.slot(rA, "x")
    r = shim.call("weight_by_split", rA, rs.integer(sb), rs.integer(4))
    assert r.value == rA                                  # the argument itself comes back ...
    assert rs.slot(rA, "x") == x_before                   # ... with the same x vector, rewritten in place
    x = rs.values(x_before)
    assert not np.array_equal(x, A.x) and same_bits(x, mirror.x)
    assert np.array_equal(rs.values(rs.slot(rA, "i")), A.i) and np.array_equal(rs.values(rs.slot(rA, "p")), A.p)
    assert rel_fro(x, ref.x) < 1e-14                      # test_gpu_ops.py: test_weight_by_split_one_shot


# ---- c_gcnmf ----------------------------------------------------------------------------------------------------------------
@covers("c_gcnmf")
@pytest.mark.parametrize("orient", ["k_by_m", "m_by_k"])
def test_c_gcnmf(sa, ora, rs, shim, data, orient):
    """w in both orientations (transposed iff nrow(w) == nrow(A) and w is not square); w comes back m x k"""
    A, At, w0 = data["A"], data["At"], data["w0"]
    wR = data["wR"]
    rng = np.random.default_rng(8)
    G = sa.spatial_graph(rng.random(N) * 6, rng.random(N) * 6, 1.5)
    assert G.nnz > N
    Gc = ora.CSC(G.x.copy(), G.i.astype(np.int32), G.p.astype(np.int32), N, N)
    win = wR if orient == "k_by_m" else w0
    mirror = twice(lambda: sa.c_gcnmf(to_dgc(sa, A), to_dgc(sa, At), G, 0.0, 3, False, 0.01, 0.002, 0, win))
    ref = gr.c_gcnmf(ora, A, At, Gc, 0.0, 3, 0.01, 0.002, w0)
    r = shim.call("c_gcnmf", r_dgc(rs, A), r_dgc(rs, At), rs.dgc(G.x, G.i, G.p, (N, N)), rs.real(0.0), rs.real(3.0), rs.logical(0),
                  rs.real(0.01), rs.real(0.002), rs.integer(0), rs.matrix(win))
    got = fit_list(rs, r, NMF_NAMES, (M, K), (K, N))
    same_as_mirror(got, mirror)
    for key in ("w", "h", "d"):                           # test_gpu_gcnmf.py: _check
        g = got[key].T if key == "h" else got[key]
        assert rel_fro(g, ref[key]) < TOL, (key, rel_fro(g, ref[key]))
        if g.ndim == 2:
            assert same_zero_pattern(g, ref[key]), key


# ---- rowwise_compress -------------------------------------------------------------------------------------------------------
def _raster_same(got, want):
    """test_gpu_rasterize.py: _same, on an array read back from R's layout"""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert rr.same_bits(got, want)


def _dense_dgc(rs, sa, D):
    mask = (D != 0) | np.isnan(D)
    cols = [np.nonzero(mask[:, j])[0] for j in range(D.shape[1])]
    p = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
    i = np.concatenate(cols).astype(np.int32)
    x = np.concatenate([D[c, j] for j, c in enumerate(cols)])
    return rs.dgc(x, i, p, D.shape), sa.dgCMatrix(x, i, p, D.shape)


@covers("rowwise_compress_sparse", "rowwise_compress_dense")
@pytest.mark.parametrize("n,rows", [(2.9, 18), (3, 12), (38, 0), (1e300, 0)])
def test_rowwise_compress(sa, rs, shim, data, n, rows):
    """n = 2.9 acts as 2; 37 rows are no multiple of 2 or 3; n > nrow gives a 0 x ncol matrix"""
    D = np.where(data["D"] != 0, np.round(data["D"] * 9) + 1, 0.0)
    want = rr.vectorised_dense(D, int(n)) if n <= M else np.zeros((0, N))
    assert want.shape == (rows, N)
    rA, dA = _dense_dgc(rs, sa, D)
    for entry, r_arg, mirror_fn in (("rowwise_compress_sparse", rA, lambda: sa.rowwise_compress_sparse(dA, n)),
                                    ("rowwise_compress_dense", rs.matrix(D), lambda: sa.rowwise_compress_dense(D, n))):
        mirror = twice(mirror_fn)
        r = shim.call(entry, r_arg, rs.real(n), rs.integer(0))
        assert rs.typeof(r.value) == R.REALSXP and rs.dim(r.value) == (rows, N) and rs.length(r.value) == rows * N
        got = rs.as_matrix(r.value)
        assert same_bits(got, mirror)
        _raster_same(got, want)


@covers("rowwise_compress_dense")
def test_rowwise_compress_dense_integer_matrix_with_na(sa, rs, shim, data):
    """an integer matrix is widened as Rcpp's NumericMatrix takes it: NA_integer_ becomes NaN, which poisons its bin's mean"""
    Di = np.where(data["D"] != 0, np.round(data["D"] * 9) + 1, 0).astype(np.int32)
    Di[4, 7] = R.NA_INTEGER
    Df = Di.astype(np.float64)
    Df[4, 7] = np.nan
    mirror = twice(lambda: sa.rowwise_compress_dense(Df, 3))
    r = shim.call("rowwise_compress_dense", rs.int_matrix(Di), rs.integer(3), rs.integer(0))
    assert rs.typeof(r.value) == R.REALSXP and rs.dim(r.value) == (12, N)
    got = rs.as_matrix(r.value)
    assert np.isnan(got[1, 7]) and np.isnan(got).sum() == 1
    assert same_bits(np.nan_to_num(got, nan=-1.0), np.nan_to_num(np.asarray(mirror), nan=-1.0))
    _raster_same(got, rr.vectorised_dense(Df, 3))


# ---- the spatial graphs -----------------------------------------------------------------------------------------------------
def graph_of(rs, r):
    """an S4 dgCMatrix -> (p, i, x), after the structure checks"""
    v = r.value
    assert rs.typeof(v) == R.S4SXP and rs.class_name(v) == "dgCMatrix" and rs.L.emul_slot_count(v) == 4
    i, p, x, dim = (rs.slot(v, s) for s in ("i", "p", "x", "Dim"))
    assert rs.typeof(i) == R.INTSXP and rs.typeof(p) == R.INTSXP and rs.typeof(x) == R.REALSXP and rs.typeof(dim) == R.INTSXP
    n = rs.length(p) - 1
    assert list(rs.values(dim)) == [n, n] and rs.length(i) == rs.length(x) == rs.values(p)[-1]
    return rs.values(p), rs.values(i), rs.values(x)


def nan_bits(x):
    """test_gpu_local_neighbors.py: _bits"""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = np.nan
    return x.view(np.uint64)


def graph_same(got, ref):
    """the _same of test_gpu_local_neighbors.py / test_gpu_spatial_graph.py on (p, i, x) triples"""
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(nan_bits(got[2]), nan_bits(ref[2]))


@covers("c_LKNN", "c_SNN")
@pytest.mark.parametrize("transposed", [False, True])
def test_c_lknn_and_c_snn(sa, rs, shim, capsys, transposed):
    rng = np.random.default_rng(3)
    x, y = lr.lattice(7)                     # 49 points
    n, D = x.size, 3
    emb = rng.random((D, n)) * (rng.random((D, n)) >= 0.3)
    m_arg = emb.T.copy() if transposed else emb      # cells x factors is transposed by the reference's rule
    capsys.readouterr()
    mirror = twice(lambda: sa.c_LKNN(m_arg, x, y, 6, 2.0, "jaccard", True, 0.1, True, 0))
    want_lines = capsys.readouterr().out.splitlines()[:3]
    ref = lr.lknn_brute(emb, x, y, 6, 2.0, "jaccard", True, 0.1)
    r = shim.call("c_LKNN", rs.matrix(m_arg), rs.real(x), rs.real(y), rs.real(6.0), rs.real(2.0), rs.string("jaccard"),
                  rs.logical(1), rs.real(0.1), rs.logical(1), rs.integer(0))
    got = graph_of(rs, r)
    graph_same(got, (mirror.p, mirror.i, mirror.x))
    graph_same(got, ref)
    lines = r.output.splitlines()
    assert lines == want_lines and lines[0] == "number of edges per node: 24" and lines[1] == "filtering %d edges" % (24 * n)
    assert lines[2] == "selected %d edges" % got[0][n] and got[0][n] > 0
    # c_SNN of that graph, with a non-zero threshold
    knn = sa.dgCMatrix(got[2], got[1], got[0], (n, n))
    mirror = twice(lambda: sa.c_SNN(knn, 1 / 15, 0))
    r = shim.call("c_SNN", rs.dgc(got[2], got[1], got[0], (n, n)), rs.real(1 / 15), rs.integer(0))
    assert r.output == ""
    snn = graph_of(rs, r)
    graph_same(snn, (mirror.p, mirror.i, mirror.x))
    graph_same(snn, lr.snn(knn.i, knn.p, n, n, 1 / 15))


@covers("c_SNN")
def test_c_snn_reads_no_x_slot(sa, rs, shim):
    """only the pattern is read: an object with i, p and Dim alone is enough; non-square: the result is ncol x ncol"""
    import scipy.sparse as sp
    Rm = sp.random(31, 23, density=0.15, format="csc", random_state=4)
    G = sa.dgCMatrix.from_scipy(Rm)
    mirror = twice(lambda: sa.c_SNN(G, 0.0, 0))
    r = shim.call("c_SNN", rs.s4("dgCMatrix", i=rs.integer(G.i), p=rs.integer(G.p), Dim=rs.integer([31, 23])), rs.real(0.0), rs.integer(0))
    snn = graph_of(rs, r)
    assert len(snn[0]) == 24
    graph_same(snn, (mirror.p, mirror.i, mirror.x))
    graph_same(snn, lr.snn(G.i, G.p, 31, 23, 0.0))


@covers("spatial_graph")
@pytest.mark.parametrize("case", ["doubles", "integers", "tiny_max_dist", "max_k_above_n", "max_k_2"])
def test_spatial_graph(sa, rs, shim, case):
    rng = np.random.default_rng(6)
    n = 41
    if case == "integers":
        xi, yi = rng.integers(0, 6, n).astype(np.int32), rng.integers(0, 6, n).astype(np.int32)
        x, y, rx, ry = xi.astype(np.float64), yi.astype(np.float64), rs.integer(xi), rs.integer(yi)
    else:
        x, y = rng.random(n) * 5, rng.random(n) * 5
        rx, ry = rs.real(x), rs.real(y)
    max_dist = 1e-300 if case == "tiny_max_dist" else 1.5
    max_k = {"max_k_above_n": 1e6, "max_k_2": 2.9}.get(case, 100.0)
    mirror = twice(lambda: sa.spatial_graph(x, y, max_dist, max_k))
    ref = sr.brute(x, y, max_dist, int(max_k))
    r = shim.call("spatial_graph", rx, ry, rs.real(max_dist), rs.real(max_k), rs.integer(0))
    got = graph_of(rs, r)
    graph_same(got, (mirror.p, mirror.i, mirror.x))
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])          # test_gpu_spatial_graph.py: _same
    assert np.array_equal(got[2].view(np.uint64), np.asarray(ref[2], dtype=np.float64).view(np.uint64))
    if case == "tiny_max_dist":              # a point is always within max_dist of itself: what is left is the diagonal
        assert np.array_equal(got[0], np.arange(n + 1)) and np.array_equal(got[1], np.arange(n)) and np.all(got[2] == 1.0)
    elif case == "max_k_2":
        assert np.diff(got[0]).max() == 2
    else:
        assert got[0][-1] > n


@covers("spatial_graph", "c_SNN")
def test_graphs_without_an_edge(sa, rs, shim):
    """The zero-edge branch of graph_result: i and x of length 0, the second library call made on the dummy pointers.
    spatial_graph keeps every point's own edge whatever max_dist is (its distance to itself is 0 < max_dist), so its only
    graph without an edge has no point; c_SNN of a pattern without an entry has none either (the diagonal is set for
    non-empty columns only)."""
    mirror = twice(lambda: sa.spatial_graph(np.zeros(0), np.zeros(0), 1.0, 100))
    r = shim.call("spatial_graph", rs.real([]), rs.real([]), rs.real(1.0), rs.real(100.0), rs.integer(0))
    got = graph_of(rs, r)
    assert list(got[0]) == [0] and got[1].size == 0 and got[2].size == 0
    graph_same(got, (mirror.p, mirror.i, mirror.x))
    empty = sa.dgCMatrix(np.zeros(0), np.zeros(0, np.int32), np.zeros(8, np.int32), (9, 7))
    mirror = twice(lambda: sa.c_SNN(empty, 0.0, 0))
    r = shim.call("c_SNN", rs.dgc([], [], np.zeros(8), (9, 7)), rs.real(0.0), rs.integer(0))
    got = graph_of(rs, r)
    assert list(got[0]) == [0] * 8 and got[1].size == 0 and got[2].size == 0
    graph_same(got, (mirror.p, mirror.i, mirror.x))
    graph_same(got, lr.snn(empty.i, empty.p, 9, 7, 0.0))


# ---- library errors, interrupts, unload ---------------------------------------------------------------------------------------
def _nmf_args(rs, A, At, wR, maxit):
    return [r_dgc(rs, A), r_dgc(rs, At), rs.real(0.0), rs.real(float(maxit)), rs.logical(0), rs.real(0.01), rs.real(0.01), rs.real(0.0),
            rs.real(0.0), rs.integer(0), rs.matrix(wR)]


@covers("c_nmf")
def test_a_library_error_becomes_an_r_error(sa, ora, rs, shim, data):
    """as test_gpu_degenerate.py: test_non_finite_input_is_refused expects from the C ABI"""
    A, At, w0 = data["A"], data["At"], data["w0"]
    wR = data["wR"]
    x = A.x.copy()
    x[7] = np.nan
    bad = ora.CSC(x, A.i, A.p, A.nrow, A.ncol)
    base = rs.L.emul_protect_depth()
    args = _nmf_args(rs, bad, At, wR, 3)
    depth = rs.L.emul_protect_depth()
    r = shim.call("c_nmf", *args, ok=False)
    assert r.kind == R.ERROR and r.value is None
    assert r.message.startswith("singlet HIP back end:") and "non-finite" in r.message
    assert r.protect_delta == 0 and rs.L.emul_protect_depth() == depth and r.protect_delta_at_exit == 3 and base < depth
    assert r.events == []
    mirror = sa.c_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 3, False, 0.01, 0.01, 0.0, 0.0, 0, wR)
    r = shim.call("c_nmf", *_nmf_args(rs, A, At, wR, 3))      # the next valid call of the process
    same_as_mirror(fit_list(rs, r, NMF_NAMES, (K, M), (K, N)), mirror)


@covers("spatial_graph", "c_LKNN", "c_SNN")
def test_a_library_error_inside_graph_result_becomes_an_r_error(sa, rs, shim):
    """graph_fail_if of singlet_hip_graph_shim.c: the library refuses inside graph_result's first call, where the protect
    stack holds p (and the widened c1, c2 of spatial_graph).  Each entry: an R error with the back end's prefix and the text
    the mirror's exception carries, the stack unwound, no collected object touched, and the next valid call equal to the
    mirror's."""
    x, y = lr.lattice(4)
    n = x.size
    emb = np.ones((2, n))
    xi = x.astype(np.int32)
    xi[3] = R.NA_INTEGER                     # widened to NaN by the shim, which sgl_spatial_graph refuses
    xf = x.copy()
    xf[3] = np.nan
    cases = [
        ("spatial_graph", lambda: [rs.integer(xi), rs.integer(y.astype(np.int32)), rs.real(1.5), rs.real(100.0), rs.integer(0)],
         lambda: sa.spatial_graph(xf, y, 1.5, 100), "coordinate 3 is not finite", 3),
        ("c_LKNN", lambda: [rs.matrix(emb), rs.real(x), rs.real(y), rs.real(5.0), rs.real(-1.0), rs.string("euclidean"), rs.logical(1),
                            rs.real(0.0), rs.logical(0), rs.integer(0)],
         lambda: sa.c_LKNN(emb, x, y, 5, -1.0, "euclidean", True, 0.0, False, 0), "radius", 1),
        ("c_SNN", lambda: [rs.dgc([1.0, 1.0], [1, 0], [0, 2], (2, 1)), rs.real(0.0), rs.integer(0)],
         lambda: sa.c_SNN(sa.dgCMatrix([1.0, 1.0], [1, 0], [0, 2], (2, 1)), 0.0, 0), "ascending", 1),
    ]
    for entry, r_args, mirror_fn, text, held in cases:
        with pytest.raises(sa.SingletHipError, match=text):
            mirror_fn()
        args = r_args()
        depth = rs.L.emul_protect_depth()
        r = shim.call(entry, *args, ok=False)
        assert r.kind == R.ERROR and r.value is None, (entry, r.kind)
        assert r.message.startswith("singlet HIP back end: ") and text in r.message, (entry, r.message)
        # what was held when the library refused: p in graph_result's first call (p, i and x in its second), c1 and c2
        assert r.protect_delta_at_exit in (held, held + 2), r.protect_delta_at_exit
        assert r.protect_delta == 0 and rs.L.emul_protect_depth() == depth
        assert r.events == [] and r.ralloc_blocks == 0 and r.output == ""
    # the next valid call of each
    mirror = sa.spatial_graph(x, y, 1.5, 100)
    got = graph_of(rs, shim.call("spatial_graph", rs.integer(x.astype(np.int32)), rs.real(y), rs.real(1.5), rs.real(100.0), rs.integer(0)))
    graph_same(got, (mirror.p, mirror.i, mirror.x))
    mirror = sa.c_LKNN(emb, x, y, 5, 1.0, "euclidean", True, 0.0, False, 0)
    got = graph_of(rs, shim.call("c_LKNN", rs.matrix(emb), rs.real(x), rs.real(y), rs.real(5.0), rs.real(1.0), rs.string("euclidean"),
                                 rs.logical(1), rs.real(0.0), rs.logical(0), rs.integer(0)))
    graph_same(got, (mirror.p, mirror.i, mirror.x))
    knn = sa.dgCMatrix(got[2], got[1], got[0], (n, n))
    mirror = sa.c_SNN(knn, 0.0, 0)
    snn = graph_of(rs, shim.call("c_SNN", rs.dgc(got[2], got[1], got[0], (n, n)), rs.real(0.0), rs.integer(0)))
    graph_same(snn, (mirror.p, mirror.i, mirror.x))


@covers("c_nmf", "c_ard_nmf")
def test_an_interrupt_ends_the_fit_as_r_does(sa, rs, shim, data):
    """An interrupt pending from the second poll on: the library stops at its polling point with SGL_EINTR (the path
    test_gpu_nmf.py: test_callbacks_log_poll_and_verbose takes from Python), the shim unprotects and calls Rf_onintr."""
    A, At, w0 = data["A"], data["At"], data["w0"]
    wR = data["wR"]
    ard_tail = [rs.real(7.0), rs.real(4.0), rs.real(1e9), rs.real(1.0)]
    for entry in ("c_nmf", "c_ard_nmf"):
        args = _nmf_args(rs, A, At, wR, 5000)
        if entry == "c_ard_nmf":
            args = args[:5] + [rs.real(0.01), rs.real(0.0), rs.integer(0), args[10]] + ard_tail
        depth = rs.L.emul_protect_depth()
        rs.L.emul_arm_interrupt(2)
        r = shim.call(entry, *args, ok=False)
        rs.L.emul_arm_interrupt(0)
        assert r.kind == R.INTERRUPT and r.value is None and r.message == "interrupted"
        assert r.protect_delta_at_exit == 0      # the shim unprotects before Rf_onintr
        assert r.protect_delta == 0 and rs.L.emul_protect_depth() == depth
        assert 2 <= r.polls < 50 and r.events == [] and r.ralloc_blocks == 0
    mirror = sa.c_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 3, False, 0.01, 0.01, 0.0, 0.0, 0, wR)
    r = shim.call("c_nmf", *_nmf_args(rs, A, At, wR, 3))
    same_as_mirror(fit_list(rs, r, NMF_NAMES, (K, M), (K, N)), mirror)
    mirror = sa.c_ard_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 2, False, 0.01, 0.0, 0, wR, 7, 4, 1e9, 1)
    args = _nmf_args(rs, A, At, wR, 2)
    r = shim.call("c_ard_nmf", *(args[:5] + [rs.real(0.01), rs.real(0.0), rs.integer(0), args[10]] + ard_tail))
    same_as_mirror(fit_list(rs, r, ARD_NAMES, (K, M), (K, N)), mirror)


def test_unload_releases_the_pool(sa, rs):
    """R_unload_singlet_hip_shim: the blocks the library keeps between calls go back to the driver"""
    L = sa._lib.load()
    with sa.Context(0) as c:                 # leaves a block of 64 MB or more in the pool
        c.synth(5000, 60000, 20)
    cached = C.c_int64()
    assert L.sgl_pool_info(C.byref(cached)) == 0 and cached.value > 0
    rs.L.R_unload_singlet_hip_shim(rs.L.emul_dll())
    assert L.sgl_pool_info(C.byref(cached)) == 0 and cached.value == 0


def test_every_registered_entry_has_a_case(rs):
    L = rs.L
    registered = {L.emul_entry_name(q).decode() for q in range(L.emul_entry_count())}
    assert len(registered) == 16
    assert registered == set(COVERED), (registered - set(COVERED), set(COVERED) - registered)
