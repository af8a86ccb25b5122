"""Cosine and correlation neighbours on the GPU (sgl_knn_metric / sgl_c_knn_metric / sgl_knn_metric_info; the metric keyword
of Context.knn, knn, find_neighbors, run_umap) against the numpy restatement of their rules (tests/knn_metric_restatement.py).
Everything is np.array_equal on idx and dist: the rule is exact, there is no tolerance and no share of cases left out."""
import ctypes as C
import functools

import numpy as np
import pytest

import embedding_knn_restatement as euclid
import knn_metric_restatement as rs
from conftest import to_dgc

pytestmark = pytest.mark.gpu
EINVAL = -1
BOTH = ("cosine", "correlation")
INFO = ("instance", "segments", "queries_per_workgroup", "lists_global")
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _normal(rng, k, n):
    return rng.standard_normal((k, n))


def _nmf_like(rng, k, n):
    """Non-negative, many exact zeros (whole zero columns at small k), every row (factor) summing to 1 as scale() leaves h."""
    X = rng.random((k, n)) * (rng.random((k, n)) < 0.35)
    X[:, 0] += 1e-3
    return X / X.sum(axis=1, keepdims=True)


def _same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64, what
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[1], want[1]), (what, "dist")
    assert not np.signbit(got[1]).any(), (what, "a negative zero")


def _search(c, K, R, Q, metric, dims=None):
    """(idx, dist) of c.knn and the report of the search."""
    got = c.knn(K, R, Q, dims, metric=metric)
    return got, c.knn_metric_info()


# ------------------------------------------------------------------------------------------------------------ loop edges
# (n_dims, n_ref, n_query or None for the references themselves, K) -> (instance, segments, queries per workgroup, lists in
# global scratch): the smallest shapes that turn each loop of the five scan instances with both list homes.
CASES = {
    (1, 65, None, 1): (0, 1, 128, 0),          # correlation: one dimension, every column without direction
    (2, 64, 63, 64): (0, 1, 128, 1),
    (8, 129, 64, 20): (0, 1, 128, 0),
    (3, 2049, 128, 32): (0, 2, 128, 0),        # the only one that runs as two segments
    (9, 257, 65, 20): (1, 1, 128, 0),
    (16, 130, None, 33): (1, 1, 128, 1),
    (17, 300, 65, 20): (2, 1, 128, 0),
    (32, 127, None, 127): (2, 1, 128, 1),
    (33, 300, 1, 20): (3, 1, 64, 0),
    (50, 1025, None, 20): (3, 1, 64, 0),
    (64, 300, 65, 33): (3, 1, 64, 1),
    (66, 7, 3, 7): (4, 1, 64, 0),
    (130, 9, None, 2): (4, 1, 64, 0),
    (130, 257, 63, 256): (4, 1, 64, 1),
    (132, 300, 64, 33): (4, 1, 64, 1),
}


def test_the_grid_reaches_every_instance_with_both_list_homes_and_two_segments():
    assert {(v[0], v[3]) for v in CASES.values()} == {(i, g) for i in range(5) for g in (0, 1)}
    assert [s for s, v in CASES.items() if v[1] > 1] == [(3, 2049, 128, 32)]


@functools.lru_cache(maxsize=None)
def _case(nd, n_ref, nq, K, kind, metric):
    rng = np.random.default_rng([nd, n_ref, nq or 0, K, len(kind)])
    make = _normal if kind == "normal" else _nmf_like
    R = make(rng, nd, n_ref)
    Q = None if nq is None else make(rng, nd, nq)
    if Q is not None and nq > 2:
        Q[:, 1] = R[:, n_ref // 2] * 4.0     # a query that is a reference times a power of two: key +0.0
    want = rs.knn(R, Q, K, metric=metric, with_count=True)
    for a in (R, want[0], want[1]):
        a.setflags(write=False)
    return R, Q, want


GRID = [(shape, kind, metric) for shape in CASES for kind in ("normal", "nmf") for metric in BOTH]


@pytest.mark.parametrize("shape,kind,metric", GRID, ids=["d%d-r%d-q%s-K%d-%s-%s" % (s + (k, m)) for s, k, m in GRID])
def test_loop_edges_bit_for_bit(ctx, shape, kind, metric):
    nd, n_ref, nq, K = shape
    R, Q, want = _case(nd, n_ref, nq, K, kind, metric)
    got, info = _search(ctx, K, R, Q, metric)
    print(shape, kind, metric, info)
    assert tuple(info[n] for n in INFO) == CASES[shape]
    assert info["metric"] == rs.METRICS[metric] and info["no_direction"] == want[2]
    if shape == (1, 65, None, 1) and metric == "correlation":
        assert want[2] == 65 and np.all(want[1] == 1.0) and np.array_equal(want[0], np.zeros((65, 1), dtype=np.int32))
    _same(got, want, (shape, kind, metric))


# --------------------------------------------------------------------------------------------------- ties and the snap
@pytest.mark.parametrize("metric", BOTH)
@pytest.mark.parametrize("nd,n,K", [(2, 300, 5), (3, 400, 20), (50, 300, 40), (70, 200, 33)])
def test_duplicates_and_power_of_two_copies_tie_at_zero_and_rank_by_index(ctx, metric, nd, n, K):
    """Blocks of K + 1 and 2 K columns that are one column times powers of two: all at key +0.0 from one another, ranked by
    index, and the later cells of a block pushed out of their own lists.  (nd = 2 under correlation has two directions only:
    nearly everything ties.)"""
    rng = np.random.default_rng(nd * 1000 + K + len(metric))
    R = rng.random((nd, n)) + 0.25
    R[:, 10:10 + K + 1] = R[:, [10]] * 2.0 ** rng.integers(-30, 31, K + 1)
    R[:, 100:100 + 2 * K] = R[:, [100]]
    R[:, 100 + K] *= 2.0 ** -500                                  # still far from underflow in the sum of squares: 2^-1000
    want = rs.knn(R, None, K, metric=metric, with_count=True)
    assert want[2] == 0
    for start, size in ((10, K + 1), (100, 2 * K)):
        block = np.arange(start, start + size)
        if not (nd == 2 and metric == "correlation"):
            assert np.array_equal(want[0][block], np.tile(block[:K], (size, 1)))
        assert np.all(want[1][block] == 0.0)
    assert (want[0] != np.arange(n)[:, None]).all(axis=1).sum() >= K + 1     # cells that are not in their own lists
    got, info = _search(ctx, K, R, None, metric)
    assert info["no_direction"] == 0
    _same(got, want, "self")
    Q = rng.random((nd, 70)) + 0.25
    Q[:, 3] = R[:, 10] * 8.0
    Q[:, 68] = R[:, 100] * 0.5
    wq = rs.knn(R, Q, K, metric=metric)
    assert np.all(wq[1][[3, 68]] == 0.0)
    _same(ctx.knn(K, R, Q, metric=metric), wq, "queries")


# --------------------------------------------------------------------------------------------------------- no direction
@pytest.mark.parametrize("metric", BOTH)
@pytest.mark.parametrize("nd", [3, 70])
def test_columns_without_direction_are_at_one_from_everything(ctx, metric, nd):
    rng = np.random.default_rng(nd)
    n, K = 150, 25
    R = rng.standard_normal((nd, n))
    R[:, 5:9] = 0.0                                               # all-zero columns
    R[:, 20:23] = 2.5                                             # constant columns: a direction under cosine, none under correlation
    R[:, 40:44] = rng.choice([-1e200, 1e200], size=(nd, 4))       # the sum of squares overflows
    R[0, 40], R[1, 40] = 1e200, -1e200                            # (not constant, so that correlation sees the overflow too)
    R[:, 60:63] = rng.choice([-1e-200, 1e-200], size=(nd, 3))     # ... and underflows to 0
    Q = rng.standard_normal((nd, 30))
    Q[:, 2] = 0.0
    Q[:, 7] = -1e200 * (1 + np.arange(nd) % 2)
    Q[:, 9] = 7.0
    for q, name in ((None, "self"), (Q, "queries")):
        want = rs.knn(R, q, K, metric=metric, with_count=True)
        flat = 3 if metric == "correlation" else 0
        assert want[2] == 11 + flat + (0 if q is None else 2 + (1 if metric == "correlation" else 0)), (name, want[2])
        assert not np.isnan(want[1]).any()
        lost = [5, 6, 7, 8, 40, 41, 42, 43, 60, 61, 62] if q is None else [2, 7]
        assert np.all(want[1][lost] == 1.0) and np.array_equal(want[0][lost], np.tile(np.arange(K, dtype=np.int32), (len(lost), 1)))
        got, info = _search(ctx, K, R, q, metric)
        assert info["no_direction"] == want[2], name
        assert not np.isnan(got[1]).any()
        _same(got, want, name)


# -------------------------------------------------------------------------------------------------------------- segments
@pytest.mark.parametrize("metric", BOTH)
def test_segments_merge_to_the_same_bits(ctx, metric):
    rng = np.random.default_rng(21)
    R = rng.standard_normal((3, 50000))
    R[:, 40000:40030] = R[:, [7]]           # thirty copies of reference 7, segments apart: ties at +0.0 across the cuts
    R[:, 20000:20005] = R[:, [7]] * 0.25
    Q3 = np.stack([R[:, 7] * 2.0, rng.standard_normal(3), R[:, 49999] + 1e-9], axis=1)
    want = rs.knn(R, Q3, 20, metric=metric)
    assert want[0][0].tolist() == [7] + list(range(20000, 20005)) + list(range(40000, 40014)) and np.all(want[1][0] == 0.0)
    got, info = _search(ctx, 20, R, Q3, metric)
    assert info["segments"] == 48 and info["instance"] == 0
    _same(got, want, "3 queries, 48 segments")


# ----------------------------------------------------------------------------------------------------------------- forms
@pytest.mark.parametrize("metric", BOTH)
def test_resident_host_and_one_shot_forms_agree(sa, ora, metric):
    A = ora.synth_csc(40, 300, 6)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        c.fit_init(5)
        for _ in range(3):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        H = c.get_factors()[2]               # cells x k: the column-major image of the k x cells H
        want = rs.knn(H.T, None, 20, metric=metric, with_count=True)
        resident = c.knn(20, metric=metric)
        assert c.knn_metric_info() == dict(instance=0, segments=1, queries_per_workgroup=128, lists_global=0,
                                           metric=rs.METRICS[metric], no_direction=want[2])
        _same(resident, want, "R = NULL")
        _same(c.knn(20, H.T, metric=metric), want, "host R")
        _same(sa.knn(H.T, None, 20, metric=metric), want, "one-shot")
        _same(c.knn(20, None, H.T, metric=metric), want, "R = NULL, Q = H")
        assert c.knn_metric_info()["no_direction"] == 2 * want[2]
        _same(c.knn(20, H.T, H.T, metric=metric), want, "Q = R")
        Q = np.random.default_rng(2).random((5, 33))
        _same(c.knn(7, None, Q, [3, 0], metric=metric), rs.knn(H.T, Q, 7, [3, 0], metric=metric), "resident references, host queries, dims")
        assert np.array_equal(c.get_factors()[2].view(np.uint64), H.view(np.uint64))     # H is bitwise unchanged
        c.knn(20)                            # a plain search: the report's metric and count go back to 0
        info = c.knn_metric_info()
        assert (info["metric"], info["no_direction"]) == (0, 0) and {n: info[n] for n in INFO} == c.knn_info()


@pytest.mark.parametrize("metric", BOTH)
@pytest.mark.parametrize("k,dims", [(12, [7, 2, 9]), (12, [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]), (70, list(range(69, 3, -1)))])
def test_dims_subset_and_permutation(ctx, sa, metric, k, dims):
    rng = np.random.default_rng(k + len(dims))
    R, Q = rng.standard_normal((k, 200)), rng.standard_normal((k, 37))
    d = np.array(dims)
    want = rs.knn(R[d], Q[d], 9, metric=metric)             # on the host-gathered rows, in that order
    got, info = _search(ctx, 9, R, Q, metric, d)
    _same(got, want, "queries")
    assert info["instance"] == (0 if len(dims) <= 8 else 1 if len(dims) <= 16 else 4)
    _same(ctx.knn(9, R, None, d, metric=metric), rs.knn(R[d], None, 9, metric=metric), "self")
    _same(sa.knn(R, Q, 9, d, metric=metric), want, "one-shot")


def test_a_plain_fit_continued_after_a_cosine_search_gives_the_same_bits(sa, ora):
    """A few iterations, a cosine search on the resident H (and one with host operands), a few more: the factors, the tol
    values and the sweep totals of the uninterrupted run."""
    m, n, k = 120, 300, 12
    A = ora.synth_csc(m, n, 6)
    runs = {}
    for with_knn in (False, True):
        with sa.Context(0) as c:
            c.upload(to_dgc(sa, A))
            c.fit_init(k)
            c.sweeps_get(reset=True)
            trace = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            if with_knn:
                H = c.get_factors()[2]
                _same(c.knn(20, metric="cosine"), rs.knn(H.T, None, 20, metric="cosine"), "mid-fit")
                c.knn(40, np.ones((70, 90)) * np.arange(90), None, [1, 5], metric="correlation")
                assert np.array_equal(c.get_factors()[2], H)
            trace += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            runs[with_knn] = (c.get_factors(), trace, c.sweeps_get(reset=True))
    for x, y, name in zip(runs[True][0], runs[False][0], "wdh"):
        assert np.array_equal(x, y), name
    assert runs[True][1] == runs[False][1]
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], key


# ------------------------------------------------------------------------------------- Euclidean through the new entries
def _raw(sa, c, Rt, Qt, k, K, metric, idx, dist):
    """sgl_knn_metric on c (None: sgl_c_knn_metric) with host operands Rt / Qt (column-major images) -> the return code."""
    L = sa._lib.load()
    args = (Rt.ctypes.data_as(f64p), k, Rt.shape[0], None if Qt is None else Qt.ctypes.data_as(f64p), Rt.shape[0] if Qt is None else Qt.shape[0],
            None, 0, K, metric, idx.ctypes.data_as(i32p), dist.ctypes.data_as(f64p))
    return L.sgl_c_knn_metric(*args) if c is None else L.sgl_knn_metric(c._h, *args)


@pytest.mark.parametrize("shape", [(8, 129, 64, 20), (9, 257, 65, 20), (17, 300, 65, 20), (64, 300, 65, 33), (132, 300, 64, 33)])
def test_metric_zero_through_the_new_entries_is_sgl_knn_bit_for_bit(sa, ctx, shape):
    nd, n_ref, nq, K = shape
    rng = np.random.default_rng(shape)
    R, Q = rng.standard_normal((nd, n_ref)), rng.standard_normal((nd, nq))
    plain = ctx.knn(K, R, Q)
    report = ctx.knn_info()
    _same(plain, euclid.knn(R, Q, K), "sgl_knn")
    Rt, Qt = np.ascontiguousarray(R.T), np.ascontiguousarray(Q.T)
    for c in (ctx, None):
        idx, dist = np.full((nq, K), -1, dtype=np.int32), np.full((nq, K), -1.0)
        sa._lib.check(_raw(sa, c, Rt, Qt, nd, K, 0, idx, dist))
        _same((idx, dist), plain, "metric = 0")
    info = ctx.knn_metric_info()
    assert {n: info[n] for n in INFO} == report and (info["metric"], info["no_direction"]) == (0, 0)


# -------------------------------------------------------------------------------------------------------------- refusals
def _refused(sa, code, match, fn):
    with pytest.raises(sa.SingletHipError, match=match) as e:
        fn()
    assert e.value.code == code, (match, e.value.code)


def test_refusals_leave_outputs_report_and_context_as_they_were(sa):
    rng = np.random.default_rng(5)
    R, Q = rng.standard_normal((6, 40)), rng.standard_normal((6, 9))
    Rt, Qt = np.ascontiguousarray(R.T), np.ascontiguousarray(Q.T)
    want = rs.knn(R, Q, 4, metric="cosine", with_count=True)
    with sa.Context(0) as c:
        _same(c.knn(4, R, Q, metric="cosine"), want, "before")
        info = c.knn_metric_info()
        assert info["metric"] == 1
        for who, cc in (("sgl_knn_metric", c), ("sgl_c_knn_metric", None)):
            for bad in (7, -1):
                idx, dist = np.full((9, 4), -7, dtype=np.int32), np.full((9, 4), -7.0)
                _refused(sa, EINVAL, r": %s: metric = %d is outside \[0, 2\]$" % (who, bad),
                         lambda: sa._lib.check(_raw(sa, cc, Rt, Qt, 6, 4, bad, idx, dist)))
                assert np.all(idx == -7) and np.all(dist == -7.0)          # the outputs are untouched
                assert c.knn_metric_info() == info                         # the report is as it was
                _same(c.knn(4, R, Q, metric="cosine"), want, "after a refusal")
            # the argument refusals of sgl_knn come first
            idx, dist = np.full((9, 4), -7, dtype=np.int32), np.full((9, 4), -7.0)
            _refused(sa, EINVAL, r": %s: n_neighbors = 0 is outside" % who, lambda: sa._lib.check(_raw(sa, cc, Rt, Qt, 6, 0, 7, idx, dist)))
        # a non-finite value: the message of sgl_knn, whatever the metric
        bad = R.copy()
        bad[4, 31] = np.inf
        bad[2, 5] = np.nan                   # the first one in column-major order
        badq = Q.copy()
        badq[5, 8] = -np.inf
        for metric in BOTH:
            _refused(sa, EINVAL, r"sgl_knn_metric: R holds a non-finite value in column 5, row 2 \(0-based; the first in column-major order\)",
                     lambda: c.knn(4, bad, Q, metric=metric))
            _refused(sa, EINVAL, r"sgl_knn_metric: Q holds a non-finite value in column 8, row 5 ", lambda: c.knn(4, R, badq, [0, 5], metric=metric))
            _refused(sa, EINVAL, r"sgl_c_knn_metric: R holds a non-finite value in column 5, row 2 ", lambda: sa.knn(bad, Q, 4, metric=metric))
            _refused(sa, EINVAL, r"sgl_knn_metric: dims\[1\] = 6 is outside \[0, k = 6\)", lambda: c.knn(4, R, Q, [2, 6], metric=metric))
            assert c.knn_metric_info() == info
        _same(c.knn(4, R, Q, metric="cosine"), want, "after the refusals")
    _same(sa.knn(R, Q, 4, metric="cosine"), want, "one-shot, after the refusals")


# ------------------------------------------------------------------------------------------------------------ downstream
def test_find_neighbors_with_cosine_is_knn_and_c_snn_composed_by_hand(sa):
    n, K = 400, 12
    X, _ = rs.rays(8, n)
    E = np.ascontiguousarray(X.T)                                          # cells x factors
    out = sa.find_neighbors(E, k_param=K, metric="cosine", return_dist=True)
    idx, dist = sa.knn(X, None, K, metric="cosine")
    _same((out["idx"], out["dist"]), (idx, dist), "find_neighbors")
    _same((idx, dist), rs.knn(X, None, K, metric="cosine"), "knn")
    order = np.argsort(idx, axis=1, kind="stable")
    nn = sa.dgCMatrix(np.take_along_axis(dist, order, axis=1).ravel(), np.take_along_axis(idx, order, axis=1).ravel(),
                      np.arange(n + 1, dtype=np.int64) * K, (n, n))
    assert np.array_equal(out["nn"].p, nn.p) and np.array_equal(out["nn"].i, nn.i) and np.array_equal(out["nn"].x, nn.x)
    snn = sa.c_SNN(nn, np.nextafter(1 / 15, -np.inf), 0)
    assert np.array_equal(out["snn"].p, snn.p) and np.array_equal(out["snn"].i, snn.i) and np.array_equal(out["snn"].x, snn.x)


def test_run_umap_with_cosine_is_the_three_steps_composed_by_hand(sa, ora):
    from singlet_amd import api
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    X, _ = rs.rays(10, 300)
    Y, G = sa.run_umap(X, n_neighbors=10, n_epochs=50, metric="cosine", return_graph=True)
    idx, dist = sa.knn(X, None, 10, metric="cosine")
    _same((idx, dist), rs.knn(X, None, 10, metric="cosine"), "knn")
    Gh = api.fuzzy_simplicial_set(idx, dist)
    a, b = api.find_ab_params(1.0, 0.3)
    Yh = api.umap_layout(Gh, api._umap_init(X, 2, "pca", 42), a, b, 50, 1.0, 5, 42)
    assert np.array_equal(G.p, Gh.p) and np.array_equal(G.i, Gh.i) and np.array_equal(bits(G.x), bits(Gh.x))
    assert Y.shape == (300, 2) and np.isfinite(Y).all() and np.array_equal(bits(Y), bits(Yh))
    Ge = sa.run_umap(X, n_neighbors=10, n_epochs=1, return_graph=True)[1]
    assert not np.array_equal(Ge.i, G.i)                                   # the default is still Euclidean: another graph
    # a Context and its array give the same result
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, ora.synth_csc(40, 300, 6)))
        c.fit_init(5)
        for _ in range(2):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        H = c.get_factors()[2]
        Yc, Gc = sa.run_umap(c, n_neighbors=10, n_epochs=20, metric="cosine", return_graph=True)
        Ya, Ga = sa.run_umap(np.ascontiguousarray(H.T), n_neighbors=10, n_epochs=20, metric="cosine", return_graph=True)
        assert np.array_equal(c.get_factors()[2], H)
        nc = sa.find_neighbors(c, k_param=10, metric="correlation")
        na = sa.find_neighbors(H, k_param=10, metric="correlation")
    assert np.array_equal(bits(Yc), bits(Ya)) and np.array_equal(Gc.i, Ga.i) and np.array_equal(bits(Gc.x), bits(Ga.x))
    _same((nc["idx"], nc["dist"]), (na["idx"], na["dist"]), "find_neighbors: context and array")
    assert np.array_equal(nc["snn"].i, na["snn"].i) and np.array_equal(nc["snn"].x, na["snn"].x)


def test_rays_on_the_device_are_the_restatement(ctx):
    """So the label purity on the device is the CPU test's: 1.0 for cosine and correlation, 0.33 for Euclidean."""
    X, label = rs.rays()
    for metric in ("cosine", "correlation", "euclidean"):
        want = rs.knn(X, None, 15, metric=metric)
        got = ctx.knn(15, X, metric=metric)
        _same(got, want, metric)
        p = rs.purity(got[0], label)
        print(metric, p)
        assert p >= 0.95 if metric != "euclidean" else p <= 0.5
