"""Embedding neighbours on the GPU (sgl_knn / sgl_c_knn / sgl_knn_info, Context.knn, knn, find_neighbors) against the numpy
restatement of their rules (tests/embedding_knn_restatement.py).  Everything is np.array_equal on idx and dist: the rule is
exact, there is no tolerance and no share of cases left out."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import embedding_knn_restatement as rs
import local_neighbors_restatement as lnr
from conftest import to_dgc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL, ESTATE = -1, -6
INFO = ("instance", "segments", "queries_per_workgroup", "lists_global")


def _normal(rng, k, n):
    return rng.standard_normal((k, n))


def _nmf_like(rng, k, n):
    """Non-negative, many exact zeros, every row (factor) summing to 1 as scale() leaves h."""
    X = rng.random((k, n)) * (rng.random((k, n)) < 0.35)
    X[:, 0] += 1e-3
    return X / X.sum(axis=1, keepdims=True)


def _same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64, what
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[1], want[1]), (what, "dist")


# ------------------------------------------------------------------------------------------------------------ loop edges
# (n_dims, n_ref, n_query or None for the references themselves, K) -> (instance, segments, queries per workgroup, lists
# in global scratch).  Instances: 0 n_dims <= 8, 1 <= 16, 2 <= 32 (two queries per lane, 128 per workgroup), 3 <= 64 (one, 64),
# 4 above.  Lists in LDS up to K = 32.  Segments: with fewer than 1024 workgroups of queries, n_ref / max(1024, 4 K) of them.
CASES = {
    # instance 0: n_dims 1, 2, 8; one reference, one query; 63 / 64 / 65 and 127 / 128 / 129 queries; K = 1, 2, n_ref
    (1, 1, None, 1): (0, 1, 128, 0),
    (1, 65, None, 1): (0, 1, 128, 0),
    (2, 300, None, 2): (0, 1, 128, 0),
    (2, 64, 63, 64): (0, 1, 128, 1),
    (3, 63, 1, 20): (0, 1, 128, 0),
    (8, 129, 64, 20): (0, 1, 128, 0),
    (8, 300, 127, 33): (0, 1, 128, 1),
    # the segment edge on both sides (2047 / 2048 / 2049 references), and the largest sizes, at n_dims <= 4
    (3, 2047, 5, 20): (0, 1, 128, 0),
    (3, 2048, 5, 20): (0, 2, 128, 0),
    (3, 2049, 128, 32): (0, 2, 128, 0),
    (4, 2049, 129, 256): (0, 2, 128, 1),
    (3, 4097, None, 20): (0, 4, 128, 0),
    # instance 1: 9 and 16; the list boundary K = 32 / 33
    (9, 257, 65, 20): (1, 1, 128, 0),
    (16, 128, None, 32): (1, 1, 128, 0),
    (16, 130, None, 33): (1, 1, 128, 1),
    # instance 2: 17 and 32
    (17, 300, 65, 20): (2, 1, 128, 0),
    (32, 127, None, 127): (2, 1, 128, 1),
    (32, 129, 129, 2): (2, 1, 128, 0),
    # instance 3: 33, the flagship rank 50, 64
    (33, 300, 1, 20): (3, 1, 64, 0),
    (50, 1025, None, 20): (3, 1, 64, 0),
    (64, 300, 65, 33): (3, 1, 64, 1),
    (64, 63, 64, 32): (3, 1, 64, 0),
    # instance 4 (tiles of 8 references, dimensions four at a time): 65, 66, 67, 130; 7 / 8 / 9 references
    (65, 300, None, 20): (4, 1, 64, 0),
    (66, 7, 3, 7): (4, 1, 64, 0),
    (67, 8, 65, 1): (4, 1, 64, 0),
    (130, 9, None, 2): (4, 1, 64, 0),
    (130, 257, 63, 256): (4, 1, 64, 1),
    (132, 300, 64, 33): (4, 1, 64, 1),
}


def test_the_grid_reaches_every_instance_and_both_list_homes_and_more_than_one_segment():
    assert {(v[0], v[3]) for v in CASES.values()} == {(i, g) for i in range(5) for g in (0, 1)}
    assert {v[1] > 1 for v in CASES.values()} == {False, True}
    assert all(nr <= 300 for (nd, nr, _, _) in CASES if nd > 64) and all(nd <= 4 for (nd, nr, _, _) in CASES if nr > 1100)


@functools.lru_cache(maxsize=None)
def _case(nd, n_ref, nq, K, kind):
    rng = np.random.default_rng([nd, n_ref, nq or 0, K, len(kind)])
    make = _normal if kind == "normal" else _nmf_like
    R = make(rng, nd, n_ref)
    Q = None if nq is None else make(rng, nd, nq)
    if Q is not None and nq > 2:
        Q[:, 1] = R[:, n_ref // 2]         # a query that is a reference: s = +0.0
    want = rs.knn(R, Q, K)
    for a in (R, want[0], want[1]):
        a.setflags(write=False)
    return R, Q, want


# both kinds of operand at every shape; the largest one once
GRID = [(shape, kind) for shape in CASES for kind in ("normal", "nmf") if kind == "normal" or shape[1] <= 2100]


@pytest.mark.parametrize("shape,kind", GRID, ids=["d%d-r%d-q%s-K%d-%s" % (s + (k,)) for s, k in GRID])
def test_loop_edges_bit_for_bit(ctx, shape, kind):
    nd, n_ref, nq, K = shape
    R, Q, want = _case(nd, n_ref, nq, K, kind)
    got = ctx.knn(K, R, Q)
    info = ctx.knn_info()
    print(shape, kind, info)
    assert tuple(info[n] for n in INFO) == CASES[shape]
    _same(got, want, (shape, kind))


# ------------------------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("nd,n,K", [(2, 300, 5), (3, 400, 20), (3, 300, 40)])
def test_ties_go_to_the_lower_index(ctx, nd, n, K):
    """Coordinates from {0, 1, 2}: every sum is exact, most distances tie, and blocks of K + 1 and 2 K identical columns push
    cells out of their own lists."""
    rng = np.random.default_rng(nd * 1000 + K)
    R = rng.integers(0, 3, size=(nd, n)).astype(np.float64)
    R[:, 10:10 + K + 1] = R[:, [10]]
    R[:, 100:100 + 2 * K] = R[:, [100]]
    want = rs.knn(R, None, K)
    assert (want[0] != np.arange(n)[:, None]).all(axis=1).sum() >= K + 1     # cells that are not in their own lists
    _same(ctx.knn(K, R), want, "self")
    Q = rng.integers(0, 3, size=(nd, 70)).astype(np.float64)
    _same(ctx.knn(K, R, Q), rs.knn(R, Q, K), "queries")


# -------------------------------------------------------------------------------------------------------------- segments
def test_segments_merge_to_the_same_bits(ctx):
    rng = np.random.default_rng(21)
    R = rng.standard_normal((3, 50000))
    R[:, 40000:40030] = R[:, [7]]           # thirty copies of reference 7, segments apart: ties across the cut
    Q3 = np.stack([R[:, 7], rng.standard_normal(3), R[:, 49999] + 1e-9], axis=1)
    want = rs.knn(R, Q3, 20)
    few = ctx.knn(20, R, Q3)
    assert ctx.knn_info()["segments"] == 48
    _same(few, want, "3 queries, 48 segments")
    big = rng.standard_normal((3, 130945))   # 1024 workgroups of 128 queries: nothing to gain from a cut
    where = [5, 70000, 130944]
    big[:, where] = Q3
    many = ctx.knn(20, R, big)
    assert ctx.knn_info()["segments"] == 1
    _same((many[0][where], many[1][where]), want, "the same queries among 130945, one segment")
    one_less = ctx.knn(20, R, big[:, :130944])
    assert ctx.knn_info()["segments"] == 2
    assert np.array_equal(one_less[0], many[0][:130944]) and np.array_equal(one_less[1], many[1][:130944])


# ----------------------------------------------------------------------------------------------------------------- forms
def test_resident_host_and_one_shot_forms_agree(sa, ora):
    A = ora.synth_csc(40, 300, 6)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        c.fit_init(5)
        for _ in range(3):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        H = c.get_factors()[2]               # cells x k: the column-major image of the k x cells H
        want = rs.knn(H.T, None, 20)
        resident = c.knn(20)
        assert c.knn_info() == dict(instance=0, segments=1, queries_per_workgroup=128, lists_global=0)
        _same(resident, want, "R = NULL")
        _same(c.knn(20, H.T), want, "host R")
        _same(sa.knn(H.T, None, 20), want, "one-shot")
        _same(c.knn(20, None, H.T), want, "R = NULL, Q = H")
        _same(c.knn(20, H.T, H.T), want, "Q = R")
        _same(c.knn(20), resident, "twice")
        Q = np.random.default_rng(2).random((5, 33))
        _same(c.knn(7, None, Q, [3, 0]), rs.knn(H.T, Q, 7, [3, 0]), "resident references, host queries, dims")
        assert np.array_equal(c.get_factors()[2], H)


# ------------------------------------------------------------------------------------------------------------------ dims
@pytest.mark.parametrize("k,dims", [(12, [7, 2, 9]), (12, [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]), (70, list(range(69, 3, -1))), (70, [69])])
def test_dims_subset_and_permutation(ctx, sa, k, dims):
    rng = np.random.default_rng(k + len(dims))
    R, Q = rng.standard_normal((k, 200)), rng.standard_normal((k, 37))
    d = np.array(dims)
    want = rs.knn(R[d], Q[d], 9)             # on the host-gathered rows, in that order
    _same(ctx.knn(9, R, Q, d), want, "queries")
    assert ctx.knn_info()["instance"] == (0 if len(dims) <= 8 else 1 if len(dims) <= 16 else 4)
    _same(ctx.knn(9, R, None, d), rs.knn(R[d], None, 9), "self")
    _same(sa.knn(R, Q, 9, d), want, "one-shot")


# -------------------------------------------------------------------------------------------------------------- overflow
@pytest.mark.parametrize("nd", [2, 70])
def test_sums_that_overflow_rank_by_index(ctx, nd):
    rng = np.random.default_rng(9)
    R = rng.choice([-1e200, 1e200, 0.0, 1.0], size=(nd, 150))
    want = rs.knn(R, None, 25)
    assert np.isinf(want[1]).any() and not np.isnan(want[1]).any()
    got = ctx.knn(25, R)
    assert not np.isnan(got[1]).any()
    _same(got, want, "+-1e200")


# ------------------------------------------------------------------------------------------------------------ reads only
@pytest.mark.parametrize("case", ["plain", "links", "masked"])
def test_a_fit_continued_after_a_search_gives_the_same_bits(sa, ora, case):
    """A few iterations, a search on the resident H (and one with host operands), a few more: the factors, the tol values and
    the sweep totals of the uninterrupted run."""
    m, n, k = 120, 300, 12
    A = ora.synth_csc(m, n, 6)
    runs = {}
    for with_knn in (False, True):
        with sa.Context(0) as c:
            c.upload(to_dgc(sa, A))
            c.fit_init(k)
            if case == "links":
                table = (np.random.default_rng(1).random((k, 4)) < 0.7).astype(np.float64)
                c.set_links_grouped(table, (np.arange(n) % 4).astype(np.int32))
            c.sweeps_get(reset=True)
            trace = []
            for half in range(2):
                if case == "masked":
                    r = c.ard_run(0.0, 2, 0.01, 0.0, 42, 8, 1e300, 1)
                    trace.append((list(r["test_mse"]), list(r["tol"]), r["n_iter"]))
                else:
                    trace += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
                if with_knn and half == 0:
                    H = c.get_factors()[2]
                    _same(c.knn(20), rs.knn(H.T, None, 20), case)
                    c.knn(40, np.ones((70, 90)) * np.arange(90), None, [1, 5])
                    assert np.array_equal(c.get_factors()[2], H)
            runs[with_knn] = (c.get_factors(), trace, c.sweeps_get(reset=True))
    for x, y, name in zip(runs[True][0], runs[False][0], "wdh"):
        assert np.array_equal(x, y), (case, name)
    assert runs[True][1] == runs[False][1], case
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], (case, key)


# -------------------------------------------------------------------------------------------------------------- refusals
def _refused(sa, code, match, fn):
    with pytest.raises(sa.SingletHipError, match=match) as e:
        fn()
    assert e.value.code == code, (match, e.value.code)


def test_refusals_leave_the_context_usable(sa, ora):
    rng = np.random.default_rng(5)
    R, Q = rng.standard_normal((6, 40)), rng.standard_normal((6, 9))
    want = rs.knn(R, Q, 4)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    Rt = np.ascontiguousarray(R.T)
    with sa.Context(0) as c:
        def ok():
            _same(c.knn(4, R, Q), want, "after a refusal")

        def raw(k=6, n_ref=40, n_query=9, K=4):
            idx, dist = np.empty((9, 4), dtype=np.int32), np.empty((9, 4))
            sa._lib.check(c._L.sgl_knn(c._h, Rt.ctypes.data_as(f64p), k, n_ref, None, n_query, None, 0, K,
                                       idx.ctypes.data_as(i32p), dist.ctypes.data_as(f64p)))

        for fn, match in [
                (lambda: c.knn(0, R, Q), r"n_neighbors = 0 is outside \[1, min\(256, n_ref = 40\)\]"),
                (lambda: c.knn(257, R, Q), r"n_neighbors = 257 is outside"),
                (lambda: c.knn(41, R, Q), r"n_neighbors = 41 is outside \[1, min\(256, n_ref = 40\)\]"),
                (lambda: raw(k=0), r"k = 0 is outside \[1, 1024\]"),
                (lambda: c.knn(1, np.ones((1025, 2))), r"k = 1025 is outside \[1, 1024\]"),
                (lambda: raw(n_ref=0, K=1), r"n_ref = 0 is outside \[1, 2\^31\)"),
                (lambda: raw(n_ref=2**31), r"n_ref = 2147483648 is outside \[1, 2\^31\)"),
                (lambda: raw(n_query=-1), r"n_query = -1 is negative"),
                (lambda: c.knn(4, R, Q, []), r"n_dims = 0 is outside \[1, k = 6\]"),
                (lambda: c.knn(4, R, Q, [0, 1, 2, 3, 4, 5, 0]), r"n_dims = 7 is outside \[1, k = 6\]"),
                (lambda: c.knn(4, R, Q, [2, 6, 1]), r"dims\[1\] = 6 is outside \[0, k = 6\)"),
                (lambda: c.knn(4, R, Q, [2, 0, -1]), r"dims\[2\] = -1 is outside \[0, k = 6\)"),
                (lambda: c.knn(4, R, Q, [5, 3, 0, 3]), r"dims\[3\] = 3 repeats an earlier entry")]:
            _refused(sa, EINVAL, match, fn)
            ok()
        bad = R.copy()
        bad[4, 31] = np.inf
        bad[2, 5] = np.nan                   # the first one in column-major order
        bad[3, 5] = -np.inf
        _refused(sa, EINVAL, r"sgl_knn: R holds a non-finite value in column 5, row 2 ", lambda: c.knn(4, bad, Q))
        ok()
        badq = Q.copy()
        badq[5, 8] = -np.inf
        _refused(sa, EINVAL, r"sgl_knn: Q holds a non-finite value in column 8, row 5 ", lambda: c.knn(4, R, badq, [0, 1]))
        ok()
        # the resident form: no fit, then a fit whose H holds a NaN
        _refused(sa, ESTATE, "R is NULL and no fit is initialised", lambda: c.knn(4))
        ok()
        c.upload(to_dgc(sa, ora.synth_csc(30, 50, 4)))
        _refused(sa, ESTATE, "R is NULL and no fit is initialised", lambda: c.knn(4))
        c.fit_init(3)
        c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        H = c.get_factors()[2]
        _same(c.knn(4), rs.knn(H.T, None, 4), "resident")
        _refused(sa, EINVAL, r"dims\[0\] = 3 is outside \[0, k = 3\)", lambda: c.knn(4, dims=[3]))
        _refused(sa, EINVAL, r"n_neighbors = 51 is outside \[1, min\(256, n_ref = 50\)\]", lambda: c.knn(51))
        Hn = H.copy()
        Hn[17, 1] = np.nan
        c.set_factors(h=Hn)
        _refused(sa, EINVAL, r"sgl_knn: H holds a non-finite value in column 17, row 1 ", lambda: c.knn(4))
        c.set_factors(h=H)
        _same(c.knn(4), rs.knn(H.T, None, 4), "resident, after the refusal")
        # an all-reduce hook: the shard's H is not the embedding, whatever R is
        c.set_allreduce(lambda dev_ptr, count: None)
        _refused(sa, ESTATE, "all-reduce hook", lambda: c.knn(4))
        _refused(sa, ESTATE, "all-reduce hook", lambda: c.knn(4, R, Q))
        c.set_allreduce(None)
        _same(c.knn(4), rs.knn(H.T, None, 4), "hook cleared")
        ok()
        info = c.knn_info()
        _refused(sa, EINVAL, "n_neighbors = 0", lambda: c.knn(0, R, Q))
        assert c.knn_info() == info          # a refused call leaves the report as it was
    # the one-shot form: R must be given; the argument refusals come before a context is made
    _refused(sa, EINVAL, r"sgl_c_knn: n_neighbors = 41 is outside", lambda: sa.knn(R, Q, 41))
    _refused(sa, EINVAL, r"sgl_c_knn: dims\[1\] = 9 is outside \[0, k = 6\)", lambda: sa.knn(R, Q, 4, [0, 9]))
    _refused(sa, EINVAL, r"sgl_c_knn: R holds a non-finite value in column 5, row 2 ", lambda: sa.knn(bad, Q, 4))
    idx, dist = np.empty((9, 4), dtype=np.int32), np.empty((9, 4))
    L = sa._lib.load()
    assert L.sgl_c_knn(None, 6, 40, None, 0, None, 0, 4, idx.ctypes.data_as(i32p), dist.ctypes.data_as(f64p)) == EINVAL
    assert b"sgl_c_knn: R is NULL" in L.sgl_last_error()
    _same(sa.knn(R, Q, 4), want, "one-shot, after the refusals")


def test_a_team_member_refuses_and_the_team_goes_on(sa, ora):
    """Through a team of one: the rank's H is a shard's, whatever R is.  (The seconds are the communicator of the team.)"""
    rng = np.random.default_rng(5)
    R, Q = rng.standard_normal((6, 40)), rng.standard_normal((6, 9))
    with sa.Multi([0]) as M:
        M.upload(to_dgc(sa, ora.synth_csc(30, 50, 4)))
        M.fit_init(3)
        M.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)
        rc = M.rank_ctx(0)
        _refused(sa, ESTATE, "shard of a team", lambda: rc.knn(4))
        _refused(sa, ESTATE, "shard of a team", lambda: rc.knn(4, R, Q))
        M.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)   # the team goes on


def test_either_output_may_be_null(sa):
    rng = np.random.default_rng(6)
    R = rng.standard_normal((6, 40))
    want = rs.knn(R, None, 4)
    Rt = np.ascontiguousarray(R.T)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L = sa._lib.load()
    idx, dist = np.full((40, 4), -1, dtype=np.int32), np.full((40, 4), -1.0)
    sa._lib.check(L.sgl_c_knn(Rt.ctypes.data_as(f64p), 6, 40, None, 0, None, 0, 4, idx.ctypes.data_as(i32p), None))
    sa._lib.check(L.sgl_c_knn(Rt.ctypes.data_as(f64p), 6, 40, None, 0, None, 0, 4, None, dist.ctypes.data_as(f64p)))
    sa._lib.check(L.sgl_c_knn(Rt.ctypes.data_as(f64p), 6, 40, None, 0, None, 0, 4, None, None))
    _same((idx, dist), want, "one output at a time")
    q0 = sa.knn(R, np.ones((6, 0)), 4)      # no query: nothing to do
    assert q0[0].shape == (0, 4) and q0[1].shape == (0, 4)


# ------------------------------------------------------------------------------------------------------------ end to end
def _pbmc3k(sa):
    g = np.load(os.path.join(GOLD, "pbmc3k_counts.npz"))
    p, di, x = g["p"].astype(np.int64), g["di"].astype(np.int64), g["x"].astype(np.float64)
    cs = np.cumsum(di)
    i = cs - np.repeat(cs[p[:-1]] - di[p[:-1]], np.diff(p))      # undo the per-column delta coding
    return sa.dgCMatrix(x, i.astype(np.int32), p.astype(np.int32), (int(g["dim"][0]), int(g["dim"][1])))


def test_pbmc3k_from_counts_to_the_shared_neighbour_graph(sa):
    from singlet_amd import api
    A = _pbmc3k(sa)
    n, K = A.ncol, 20
    with sa.Context(0) as c:
        c.upload(A)
        c.log_normalize()
        model = sa.run_nmf(None, 10, tol=1e-4, maxit=8, verbose=False, seed=1, _fits=api._ResidentFits(None, ctx=c))
        assert model["h"].shape == (10, n)
        out = sa.find_neighbors(c, k_param=K)
        assert c.knn_info() == dict(instance=1, segments=min(n // 1024, 64), queries_per_workgroup=128, lists_global=0)
        H = c.get_factors()[2]
    want = rs.knn(H.T, None, K)
    _same((out["idx"], out["dist"]), want, "pbmc3k")
    nn, snn = out["nn"], out["snn"]
    assert nn.Dim == (n, n) and np.array_equal(nn.p, np.arange(n + 1) * K) and np.all(nn.x == 1.0)
    rows = nn.i.reshape(n, K)
    assert np.array_equal(rows, np.sort(want[0], axis=1)) and np.all(np.diff(rows, axis=1) > 0)
    assert np.all((rows == np.arange(n)[:, None]).sum(axis=1) == 1)          # every cell's own row
    p, i, x = lnr.snn(nn.i, nn.p, n, n, np.nextafter(1 / 15, -np.inf))
    assert np.array_equal(snn.p, p) and np.array_equal(snn.i, i) and np.array_equal(snn.x, x)
