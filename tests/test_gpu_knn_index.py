"""The neighbour index kept on the GPU and the label / value transfer (sgl_knn_index_build / _search / _drop / _info /
_annotate / _map, sgl_op_knn_transfer; Context.knn_index_*, ReferenceIndex, transfer_labels, transfer_values, map_query).  A
search against the index is held to the one-shot calls and to their numpy restatements, the transfer to its restatement
(tests/knn_transfer_restatement.py).  Every comparison is np.array_equal: the rules are exact."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import knn_ivf_restatement as ivf
import knn_metric_restatement as km
import knn_transfer_restatement as tr
from conftest import to_dgc

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -6
METRICS = ("euclidean", "cosine", "correlation")
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("present", "method", "metric", "k", "n_dims", "n_ref", "n_lists", "train_cells", "shortest_list", "longest_list", "empty_lists",
          "bytes", "searches", "last_queries", "last_short_queries", "instance")


def _same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64, what
    assert got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[1], want[1]), (what, "dist")


def _instance(nd):
    return 0 if nd <= 8 else 1 if nd <= 16 else 2 if nd <= 32 else 3 if nd <= 64 else 4


def _refused(sa, code, match, fn):
    with pytest.raises(sa.SingletHipError, match=match) as e:
        fn()
    assert e.value.code == code, (match, e.value.code)


# ------------------------------------------------------------------------------- the search is the one-shot call, bit for bit
# (n_dims, n_ref, n_neighbors, n_lists, n_probe, n_iter): every scan instance family, both homes of the candidate lists
CASES = [(6, 400, 20, 20, 3, 10), (12, 300, 1, 7, 2, 4), (20, 500, 33, 64, 5, 3), (50, 257, 20, 9, 9, 2), (70, 260, 40, 8, 1, 2)]
QUERY_SETS = (1, 63, 65, 130, 0)


@functools.lru_cache(maxsize=None)
def _data(nd, n_ref):
    rng = np.random.default_rng([nd, n_ref])
    R = rng.random((nd, n_ref)) * (rng.random((nd, n_ref)) < 0.6) + 1e-3 * rng.random((nd, n_ref))
    R[:, 40:44] = R[:, [40]]                       # duplicates: ties that rank by index
    Q = rng.random((nd, sum(QUERY_SETS))) * (rng.random((nd, sum(QUERY_SETS))) < 0.6) + 1e-3
    Q[:, 5] = R[:, 41]                             # a query that is a reference
    R.setflags(write=False)
    Q.setflags(write=False)
    return R, Q


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", CASES, ids=["d%d-r%d-k%d-l%d-p%d-i%d" % c for c in CASES])
def test_search_is_the_one_shot_call_bit_for_bit(sa, case, metric):
    nd, n_ref, K, n_lists, n_probe, n_iter = case
    R, Q = _data(nd, n_ref)
    want_all = ivf.knn_ivf(R, Q, K, None, metric, n_lists, n_probe, n_iter)[:2]        # a query's result depends on that query alone
    with sa.Context(0) as c:
        c.knn_index_build(R, None, metric, "ivf", n_lists, n_iter)
        q0 = 0
        for served, nq in enumerate(QUERY_SETS, 1):
            Qs = Q[:, q0:q0 + nq]
            got = c.knn_index_search(Qs, K, n_probe)
            if nq:
                _same(got, sa.knn(R, Qs, K, None, metric, "ivf", n_lists, n_probe, n_iter), (case, metric, nq, "one-shot"))
                _same(got, (want_all[0][q0:q0 + nq], want_all[1][q0:q0 + nq]), (case, metric, nq, "restatement"))
            else:
                assert got[0].shape == (0, K) and got[1].shape == (0, K)
            info = c.knn_index_info()
            assert (info["searches"], info["last_queries"], info["instance"]) == (served, nq, _instance(nd))
            q0 += nq
        assert c.knn_ivf_info()["n_lists"] == 0 and c.knn_info()["segments"] == 0      # the one-shot reports stay as they were


def test_n_probe_changes_between_searches_and_all_lists_is_the_exact_call(sa):
    R, Q = _data(6, 400)
    Q = Q[:, :70]
    with sa.Context(0) as c:
        for metric in METRICS:
            c.knn_index_build(R, None, metric, "ivf", 20, 10)
            for n_probe in (3, 1, 20, 7, 3):
                got = c.knn_index_search(Q, 20, n_probe)
                _same(got, sa.knn(R, Q, 20, None, metric, "ivf", 20, n_probe, 10), (metric, n_probe))
                if n_probe == 20:
                    _same(got, sa.knn(R, Q, 20, None, metric), (metric, "exact"))
                    _same(got, km.knn(R, Q, 20, metric=metric), (metric, "exact restatement"))


def test_a_forced_query_batch_changes_no_bit(sa):
    R, Q = _data(20, 500)
    Q = Q[:, :130]
    with sa.ReferenceIndex(R.T, metric="cosine", n_lists=64, n_iter=3) as index:
        want = index.search(Q.T, 33, 5)
        for batch in (1, 7, 130):
            _same(index.search(Q.T, 33, 5, batch), want, batch)
        assert index.info()["searches"] == 4


# ------------------------------------------------------------------------------------------------------ the exact method
@pytest.mark.parametrize("metric", METRICS)
def test_method_exact_is_the_exact_one_shot_call(sa, metric):
    with sa.Context(0) as c:
        for nd, n_ref, K, nq in ((6, 400, 20, 130), (12, 300, 1, 63), (20, 500, 33, 65), (50, 257, 20, 130), (70, 260, 40, 65),
                                 (6, 2500, 20, 7)):
            R, Q = _data(nd, n_ref)
            Q = Q[:, :nq]
            c.knn_index_build(R, None, metric, "exact")
            got = c.knn_index_search(Q, K, n_probe=99, query_batch=-5)          # method 0 reads neither
            _same(got, sa.knn(R, Q, K, None, metric), (nd, n_ref, metric))
            info = c.knn_index_info()
            assert (info["method"], info["n_lists"], info["train_cells"], info["instance"]) == (0, 0, 0, _instance(nd))
            assert info["bytes"] == 8 * nd * n_ref
            if n_ref == 2500:
                _same(got, km.knn(R, Q, K, metric=metric), "segments, restatement")
                _same(c.knn(K, R, Q, metric=metric), got, "segments, on a context")
                assert c.knn_info()["segments"] == 2          # 7 queries: the references are cut into segments and merged


def test_dims_given_at_build_are_applied_to_the_queries(sa):
    R, Q = _data(12, 300)
    Q = Q[:, :65]
    dims = [7, 0, 11, 4]
    for metric in ("euclidean", "correlation"):
        for method, extra in (("ivf", ("ivf", 7, 3, 4)), ("exact", ())):
            with sa.Context(0) as c:
                c.knn_index_build(R, dims, metric, method, 7, 4)
                got = c.knn_index_search(Q, 9, 3)
                _same(got, sa.knn(R, Q, 9, dims, metric, *extra), (metric, method))
                info = c.knn_index_info()
                assert (info["k"], info["n_dims"]) == (12, 4)
    # 1-based at the R-facing level
    with sa.ReferenceIndex(R.T, dims=[8, 1, 12, 5], method="exact") as index:
        _same(index.search(Q.T, 9), sa.knn(R, Q, 9, dims), "ReferenceIndex")


# -------------------------------------------------------------------------------------------------------------- snapshot
def test_the_index_is_a_snapshot_of_the_resident_h_and_the_fit_goes_on_undisturbed(sa, ora):
    m, n, k = 120, 300, 12
    A = ora.synth_csc(m, n, 6)
    Q = np.random.default_rng(2).random((k, 40))
    runs = {}
    for with_index in (False, True):
        with sa.Context(0) as c:
            c.upload(to_dgc(sa, A))
            c.fit_init(k)
            c.sweeps_get(reset=True)
            trace = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            if with_index:
                H = c.get_factors()[2].copy()
                c.knn_index_build(None, None, "euclidean", "ivf", 10, 10)
                _same(c.knn_index_search(Q, 20, 3), sa.knn(H.T, Q, 20, None, "euclidean", "ivf", 10, 3, 10), "mid-fit")
                assert np.array_equal(c.get_factors()[2], H)
            trace += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            if with_index:
                assert not np.array_equal(c.get_factors()[2], H)
                _same(c.knn_index_search(Q, 20, 3), sa.knn(H.T, Q, 20, None, "euclidean", "ivf", 10, 3, 10), "after the fit moved on")
                _same(c.knn_index_search(Q, 20, 3), ivf.knn_ivf(H.T, Q, 20, None, "euclidean", 10, 3, 10)[:2], "restatement")
            runs[with_index] = (c.get_factors(), trace, c.sweeps_get(reset=True))
    for x, y, name in zip(runs[True][0], runs[False][0], "wdh"):
        assert np.array_equal(x, y), name
    assert runs[True][1] == runs[False][1]
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], key


# ------------------------------------------------------------------------------------------------------------ life cycle
def test_life_cycle_and_every_field_of_the_report(sa):
    R, Q = _data(6, 400)
    Q = Q[:, :9]
    R2, Q2 = _data(20, 500)
    with sa.Context(0) as c:
        assert c.knn_index_info() == dict.fromkeys(FIELDS, 0)
        none = r"the context holds no neighbour index \(call sgl_knn_index_build\)$"
        _refused(sa, ESTATE, "sgl_knn_index_search: " + none, lambda: c.knn_index_search(Q, 4, 1))
        _refused(sa, ESTATE, "sgl_knn_index_annotate: " + none, lambda: c.knn_index_annotate(np.zeros(400, dtype=np.int32)))
        _refused(sa, ESTATE, "sgl_knn_index_map: " + none, lambda: c.knn_index_map(Q, 4, 1))
        c.knn_index_drop()                                         # nothing to drop: SGL_OK
        c.knn_index_build(R, None, "cosine", "ivf", 20, 10)
        _, assign = c.op_ivf_train(20, R, None, "cosine", 10)
        counts = np.bincount(assign, minlength=20)
        want = dict(present=1, method=1, metric=1, k=6, n_dims=6, n_ref=400, n_lists=20, train_cells=400, shortest_list=int(counts.min()),
                    longest_list=int(counts.max()), empty_lists=int((counts == 0).sum()),
                    bytes=8 * 6 * 400 + 8 * 6 * 20 + 4 * 400 + 8 * 21, searches=0, last_queries=0, last_short_queries=0, instance=0)
        assert c.knn_index_info() == want
        idx, _ = c.knn_index_search(Q, 30, 1)                      # one probe, 30 neighbours: some lists are shorter
        want.update(searches=1, last_queries=9, last_short_queries=int((idx < 0).any(axis=1).sum()))
        assert c.knn_index_info() == want and want["last_short_queries"] == int((counts[ivf.nearest(
            ivf.train(ivf.operands(R, None, None, "cosine")[0], 20, 10)[0], ivf.operands(R, Q, None, "cosine")[1])[:, 0]] < 30).sum())
        c.knn_index_annotate(np.arange(400) % 5, 5, np.ones((2, 400)))
        want["bytes"] += 4 * 400 + 8 * 2 * 400
        assert c.knn_index_info() == want
        out = c.knn_index_map(Q, 4, 20)
        want.update(searches=2, last_short_queries=0)
        assert c.knn_index_info() == want and out["scores"].shape == (9, 5) and out["values"].shape == (9, 2)
        # a second build, with another n_dims, metric and method, replaces the first and its annotations
        c.knn_index_build(R2, None, "euclidean", "exact")
        assert c.knn_index_info() == dict(dict.fromkeys(FIELDS, 0), present=1, k=20, n_dims=20, n_ref=500, bytes=8 * 20 * 500, instance=2)
        _same(c.knn_index_search(Q2[:, :9], 5), sa.knn(R2, Q2[:, :9], 5), "the second index")
        _refused(sa, ESTATE, r"sgl_knn_index_map: pred_out, best_out or scores_out is asked for, but the index holds no labels", lambda: sa._lib.check(
            sa._lib.load().sgl_knn_index_map(c._h, np.ascontiguousarray(Q2[:, :9].T).ctypes.data_as(f64p), 9, 5, 0, 1, None, None,
                                             np.zeros(9, dtype=np.int32).ctypes.data_as(i32p), None, None, None)))
        _refused(sa, ESTATE, r"sgl_knn_index_map: values_out is asked for, but the index holds no values", lambda: sa._lib.check(
            sa._lib.load().sgl_knn_index_map(c._h, np.ascontiguousarray(Q2[:, :9].T).ctypes.data_as(f64p), 9, 5, 0, 1, None, None, None, None, None,
                                             np.zeros(9 * 2).ctypes.data_as(f64p))))
        c.knn_index_drop()
        assert c.knn_index_info() == dict.fromkeys(FIELDS, 0)
        _refused(sa, ESTATE, "sgl_knn_index_search: " + none, lambda: c.knn_index_search(Q, 4, 1))
        c.knn_index_drop()                                         # twice: SGL_OK


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_outputs_report_and_index_as_they_were(sa):
    R, Q = _data(6, 400)
    Q = Q[:, :9]
    Qt = np.ascontiguousarray(Q.T)
    L = sa._lib.load()
    labels = (np.arange(400) % 3).astype(np.int32)
    V = np.random.default_rng(0).random((2, 400))
    with sa.Context(0) as c:
        c.knn_index_build(R, None, "euclidean", "ivf", 20, 10)
        c.knn_index_annotate(labels, 3, V)
        want = c.knn_index_map(Q, 4, 3)
        info = c.knn_index_info()

        def search(nq, K, n_probe, batch, Qp=Qt.ctypes.data_as(f64p)):
            idx, dist = np.full((9, 4), -7, dtype=np.int32), np.full((9, 4), -7.0)
            rc = L.sgl_knn_index_search(c._h, Qp, nq, K, n_probe, batch, idx.ctypes.data_as(i32p), dist.ctypes.data_as(f64p))
            assert np.all(idx == -7) and np.all(dist == -7.0)
            return rc

        def mapped(K, n_probe, weighting):
            o = [np.full((9, 4), -7, dtype=np.int32), np.full((9, 4), -7.0), np.full(9, -7, dtype=np.int32), np.full(9, -7.0), np.full((9, 3), -7.0),
                 np.full((9, 2), -7.0)]
            rc = L.sgl_knn_index_map(c._h, Qt.ctypes.data_as(f64p), 9, K, n_probe, weighting, *(a.ctypes.data_as(i32p if a.dtype == np.int32 else f64p)
                                                                                                for a in o))
            assert all(np.all(a == -7) for a in o)
            return rc

        for fn, message in ((lambda: search(9, 4, 3, 0, None), r"sgl_knn_index_search: Q is NULL"),
                            (lambda: search(-1, 4, 3, 0), r"sgl_knn_index_search: n_query = -1 is negative"),
                            (lambda: search(9, 0, 3, 0), r"sgl_knn_index_search: n_neighbors = 0 is outside \[1, min\(256, n_ref = 400\)\]"),
                            (lambda: search(9, 257, 3, 0), r"sgl_knn_index_search: n_neighbors = 257 is outside \[1, min\(256, n_ref = 400\)\]"),
                            (lambda: search(9, 4, 0, 0), r"sgl_knn_index_search: n_probe = 0 is outside \[1, min\(n_lists = 20, 64\)\]"),
                            (lambda: search(9, 4, 21, 0), r"sgl_knn_index_search: n_probe = 21 is outside \[1, min\(n_lists = 20, 64\)\]"),
                            (lambda: search(9, 4, 3, -1), r"sgl_knn_index_search: query_batch = -1 is negative"),
                            (lambda: mapped(4, 3, 2), r"sgl_knn_index_map: weighting = 2 is outside \[0, 1\]"),
                            (lambda: mapped(4, 3, -1), r"sgl_knn_index_map: weighting = -1 is outside \[0, 1\]"),
                            (lambda: mapped(4, 21, 1), r"sgl_knn_index_map: n_probe = 21 is outside"),
                            (lambda: mapped(401, 3, 1), r"sgl_knn_index_map: n_neighbors = 401 is outside")):
            _refused(sa, EINVAL, message, lambda: sa._lib.check(fn()))
            assert c.knn_index_info() == info
        badq = Q.copy()
        badq[2, 7] = np.nan
        _refused(sa, EINVAL, r"sgl_knn_index_search: Q holds a non-finite value in column 7, row 2 \(0-based; the first in column-major order\)",
                 lambda: c.knn_index_search(badq, 4, 3))
        _refused(sa, EINVAL, r"sgl_knn_index_map: Q holds a non-finite value in column 7, row 2 ", lambda: c.knn_index_map(badq, 4, 3))
        # annotate
        for fn, message in ((lambda: c.knn_index_annotate(labels, 0), r"n_classes = 0 is outside \[1, 65536\]"),
                            (lambda: c.knn_index_annotate(labels, 65537), r"n_classes = 65537 is outside \[1, 65536\]"),
                            (lambda: c.knn_index_annotate(None, None, np.ones((1025, 400))), r"n_values = 1025 is outside \[1, 1024\]"),
                            (lambda: c.knn_index_annotate(labels, 2), r"labels\[2\] = 2 is outside \[-1, n_classes = 2\)"),
                            (lambda: c.knn_index_annotate(np.where(np.arange(400) == 77, -2, labels), 3), r"labels\[77\] = -2 is outside \[-1, n_classes = 3\)"),
                            (lambda: c.knn_index_annotate(None, None, np.where(np.arange(800).reshape(2, 400) == 431, np.inf, V)),
                             r"V holds a non-finite value in column 31, row 1 ")):
            _refused(sa, EINVAL, "sgl_knn_index_annotate: " + message, fn)
            assert c.knn_index_info() == info
        # build: sgl_knn_metric's and sgl_knn_ivf's refusals under its own name; the index that is there stays
        for fn, message in ((lambda: c.knn_index_build(R, [1, 6]), r"dims\[1\] = 6 is outside \[0, k = 6\)"),
                            (lambda: c.knn_index_build(R, None, "euclidean", "ivf", 401), r"n_lists = 401 is outside \[1, min\(n_ref = 400, 65536\)\]"),
                            (lambda: c.knn_index_build(R, None, "euclidean", "ivf", 20, 1001), r"n_iter = 1001 is outside \[0, 1000\]"),
                            (lambda: c.knn_index_build(np.where(np.arange(2400).reshape(6, 400) == 405, np.nan, R)),
                             r"R holds a non-finite value in column 5, row 1 "),
                            (lambda: sa._lib.check(L.sgl_knn_index_build(c._h, np.ascontiguousarray(R.T).ctypes.data_as(f64p), 6, 400, None, 0, 0, 2, 20, 10)),
                             r"method = 2 is outside \[0, 1\]"),
                            (lambda: sa._lib.check(L.sgl_knn_index_build(c._h, np.ascontiguousarray(R.T).ctypes.data_as(f64p), 6, 400, None, 0, 3, 0, 0, 0)),
                             r"metric = 3 is outside \[0, 2\]")):
            _refused(sa, EINVAL, "sgl_knn_index_build: " + message, fn)
            assert c.knn_index_info() == info
        _refused(sa, ESTATE, r"sgl_knn_index_build: R is NULL and no fit is initialised", lambda: sa._lib.check(
            L.sgl_knn_index_build(c._h, None, 6, 400, None, 0, 0, 1, 20, 10)))
        again = c.knn_index_map(Q, 4, 3)
        for key in ("idx", "dist", "predicted", "score", "scores", "values"):
            assert np.array_equal(again[key], want[key]), key
        # the operator
        idx, dist = want["idx"], want["dist"]
        for fn, message in ((lambda: sa._lib.check(L.sgl_op_knn_transfer(c._h, idx.ctypes.data_as(i32p), dist.ctypes.data_as(f64p), 4, 9, 400,
                                                                         labels.ctypes.data_as(i32p), 3, None, 0, 5, None, None, None, None)),
                             r"weighting = 5 is outside \[0, 1\]"),
                            (lambda: c.op_knn_transfer(idx, dist, 400, labels, 0), r"n_classes = 0 is outside"),
                            (lambda: c.op_knn_transfer(idx, dist, 400, None, None, np.ones((1025, 400))), r"n_values = 1025 is outside"),
                            (lambda: c.op_knn_transfer(idx, dist, 400, labels, 2), r"labels\[2\] = 2 is outside \[-1, n_classes = 2\)"),
                            (lambda: c.op_knn_transfer(idx, dist, 400, None, None, np.where(np.arange(800).reshape(2, 400) == 431, np.nan, V)),
                             r"V holds a non-finite value in column 31, row 1 "),
                            (lambda: c.op_knn_transfer(np.where(np.arange(36).reshape(9, 4) == 13, 400, idx), dist, 400, labels, 3),
                             r"idx holds 400 in column 3, slot 1 \(0-based\): outside \[-1, n_ref = 400\)"),
                            (lambda: c.op_knn_transfer(np.where(np.arange(36).reshape(9, 4) == 13, -2, idx), dist, 400, labels, 3),
                             r"idx holds -2 in column 3, slot 1"),
                            (lambda: c.op_knn_transfer(np.where(np.arange(36).reshape(9, 4) == 12, -1, idx), dist, 400, labels, 3),
                             r"idx holds the valid entry %d in column 3, slot 1 \(0-based\) behind a padding slot" % idx[3, 1]),
                            (lambda: c.op_knn_transfer(np.zeros((2, 257), dtype=np.int32), np.zeros((2, 257)), 400, labels, 3),
                             r"n_neighbors = 257 is outside \[1, 256\]")):
            _refused(sa, EINVAL, "sgl_op_knn_transfer: " + message, fn)
        # ... with sentinel-filled outputs left untouched
        o = [np.full(9, -7, dtype=np.int32), np.full(9, -7.0), np.full((9, 3), -7.0), np.full((9, 2), -7.0)]
        bad = np.ascontiguousarray(np.where(np.arange(36).reshape(9, 4) == 35, 400, idx), dtype=np.int32)
        Vt = np.ascontiguousarray(V.T)
        _refused(sa, EINVAL, r"sgl_op_knn_transfer: idx holds 400 in column 8, slot 3", lambda: sa._lib.check(L.sgl_op_knn_transfer(
            c._h, bad.ctypes.data_as(i32p), dist.ctypes.data_as(f64p), 4, 9, 400, labels.ctypes.data_as(i32p), 3, Vt.ctypes.data_as(f64p), 2, 1,
            o[0].ctypes.data_as(i32p), o[1].ctypes.data_as(f64p), o[2].ctypes.data_as(f64p), o[3].ctypes.data_as(f64p))))
        assert all(np.all(a == -7) for a in o)
        Vbad = Vt.copy()
        Vbad[399, 1] = np.inf
        _refused(sa, EINVAL, r"sgl_op_knn_transfer: V holds a non-finite value in column 399, row 1", lambda: sa._lib.check(L.sgl_op_knn_transfer(
            c._h, np.ascontiguousarray(idx).ctypes.data_as(i32p), dist.ctypes.data_as(f64p), 4, 9, 400, labels.ctypes.data_as(i32p), 3,
            Vbad.ctypes.data_as(f64p), 2, 1, o[0].ctypes.data_as(i32p), o[1].ctypes.data_as(f64p), o[2].ctypes.data_as(f64p), o[3].ctypes.data_as(f64p))))
        assert all(np.all(a == -7) for a in o)
        assert c.knn_index_info() == dict(info, searches=info["searches"] + 1)
        _same(c.knn_index_search(Q, 4, 3), (want["idx"], want["dist"]), "the index answers the next search with the same bits")


def test_a_context_with_an_allreduce_hook_is_refused(sa):
    R = np.random.default_rng(1).standard_normal((3, 30))
    with sa.Context(0) as c:
        c.set_allreduce(lambda dev_ptr, count: None)
        for method in ("ivf", "exact"):
            _refused(sa, ESTATE, r"sgl_knn_index_build: the context is a shard of a team or has an all-reduce hook", lambda: c.knn_index_build(R, method=method))
        assert c.knn_index_info()["present"] == 0
        c.set_allreduce(None)
        c.knn_index_build(R, n_lists=4)
        _same(c.knn_index_search(R[:, :5], 3, 4), c.knn(3, R, R[:, :5]), "hook cleared")


# ------------------------------------------------------------------------------- the transfer operator against the restatement
def _same_transfer(got, want, what):
    for key in ("predicted", "score", "scores", "values"):
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)
    if want["scores"] is not None:
        assert not np.signbit(got["scores"]).any() and not np.signbit(got["score"]).any(), what


def _lists(rng, nq, K, n_ref):
    """Neighbour lists as a search writes them: distinct cells, distances ascending with ties, trailing padding on some rows."""
    idx = np.stack([rng.permutation(n_ref)[:K] for _ in range(nq)]).astype(np.int32)
    dist = np.sort(np.round(rng.random((nq, K)) * 8) / 8 + (rng.random((nq, K)) < 0.5) * rng.random((nq, K)), axis=1)
    nv = np.where(rng.random(nq) < 0.3, rng.integers(0, K + 1, nq), K)
    pad = np.arange(K)[None, :] >= nv[:, None]
    idx[pad] = -1
    dist[pad] = np.inf
    return idx, dist


GRID = [(1, 1, 1, 1), (20, 2, 2, 63), (64, 64, 64, 64), (65, 65, 65, 65), (256, 130, 130, 1000), (20, 130, 1, 65), (64, 1, 130, 1)]


@pytest.mark.parametrize("weighting", ["uniform", "distance"])
@pytest.mark.parametrize("shape", GRID, ids=["k%d-c%d-v%d-q%d" % s for s in GRID])
def test_transfer_operator_is_the_restatement(ctx, shape, weighting):
    K, n_classes, n_values, nq = shape
    n_ref = 300
    rng = np.random.default_rng([K, n_classes, n_values, nq])
    idx, dist = _lists(rng, nq, K, n_ref)
    labels = rng.integers(-1, n_classes, n_ref).astype(np.int32)          # drawn independently of any geometry: mixed votes
    V = rng.standard_normal((n_values, n_ref))
    want = tr.transfer(idx, dist, labels, n_classes, V, weighting)
    _same_transfer(ctx.op_knn_transfer(idx, dist, n_ref, labels, n_classes, V, weighting), want, (shape, weighting))
    _same_transfer(ctx.op_knn_transfer(idx, dist, n_ref, labels, n_classes, None, weighting), dict(want, values=None), "labels alone")
    _same_transfer(ctx.op_knn_transfer(idx, dist, n_ref, None, None, V, weighting), dict(want, predicted=None, score=None, scores=None), "values alone")


def test_transfer_operator_on_hand_made_columns(ctx, sa):
    INF = np.inf
    labels = np.array([0, 1, 1, 2, -1, -1, 0, 2], dtype=np.int32)
    V = np.array([[10.0, 20.0, 40.0, 80.0, 1.0, 2.0, 3.0, 4.0], [1.0, 0.0, -1.0, 0.5, 0.25, 0.125, 8.0, -8.0]])
    idx = np.array([[-1, -1, -1, -1],          # all padding
                    [3, 6, -1, -1],            # trailing padding
                    [0, 1, 2, 3],              # all distances equal
                    [0, 1, 2, 3],              # zero distances
                    [0, 1, 2, 3],              # a +Inf last distance
                    [4, 5, 4, 5],              # unlabelled neighbours
                    [4, 5, 4, 3],              # the only labelled neighbour in the last slot
                    [3, 1, 2, 0],              # an exact two-class tie: classes 2 and 1 at 1/2 each
                    [7, -1, -1, -1]], dtype=np.int32)      # a single neighbour
    dist = np.array([[INF, INF, INF, INF], [1.0, 3.0, INF, INF], [2.5, 2.5, 2.5, 2.5], [0.0, 0.0, 0.0, 0.0], [0.0, 1.0, 2.0, INF],
                     [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 1.0, 2.0], [0.0, 1.0, 1.0, 2.0], [5.0, INF, INF, INF]])
    for weighting in ("distance", "uniform"):
        got = ctx.op_knn_transfer(idx, dist, 8, labels, 3, V, weighting)
        _same_transfer(got, tr.transfer(idx, dist, labels, 3, V, weighting), weighting)
        assert got["predicted"][0] == -1 and np.isnan(got["values"][0]).all() and not got["scores"][0].any()
        assert got["predicted"][5] == -1 and got["score"][5] == 0.0
        assert got["predicted"][8] == 2 and got["score"][8] == 1.0 and got["values"][8].tolist() == [4.0, -8.0]
    got = ctx.op_knn_transfer(idx, dist, 8, labels, 3, V, "distance")
    assert got["predicted"].tolist() == [-1, 2, 1, 1, 1, -1, -1, 1, 2]
    assert got["scores"][1].tolist() == [0.0, 0.0, 1.0] and got["values"][1].tolist() == [80.0, 0.5]       # weights 1, 0
    assert got["scores"][7].tolist() == [0.0, 0.5, 0.5] and got["score"][7] == 0.5                           # the lower class wins the tie
    assert got["scores"][4].tolist() == [0.25, 0.5, 0.25]                                                    # +Inf: everybody votes 1
    assert ctx.op_knn_transfer(idx, dist, 8, labels, 3, V, "uniform")["predicted"][6] == 2                   # there the last slot votes
    # the one-shot forms of the operator
    lab = sa.transfer_labels(idx, dist, labels, 3)
    assert set(lab) == {"predicted", "score", "scores"} and np.array_equal(lab["scores"], got["scores"])
    assert np.array_equal(sa.transfer_values(idx, dist, V.T), got["values"], equal_nan=True)


# --------------------------------------------------------------------------------------- map is search plus the operator
@pytest.mark.parametrize("method", ["ivf", "exact"])
def test_map_is_search_followed_by_the_operator(sa, method):
    R, Q = _data(20, 500)
    Q = Q[:, :130]
    Qt = np.ascontiguousarray(Q.T)
    rng = np.random.default_rng(4)
    labels = rng.integers(-1, 7, 500).astype(np.int32)
    V = rng.standard_normal((3, 500))
    L = sa._lib.load()
    with sa.Context(0) as c:
        c.knn_index_build(R, None, "cosine", method, 64, 3)
        c.knn_index_annotate(labels, 7, V)
        for weighting in ("distance", "uniform"):
            idx, dist = c.knn_index_search(Q, 33, 5)
            want = c.op_knn_transfer(idx, dist, 500, labels, 7, V, weighting)
            got = c.knn_index_map(Q, 33, 5, weighting)
            _same((got["idx"], got["dist"]), (idx, dist), (method, weighting))
            _same_transfer(got, want, (method, weighting))
            _same_transfer(got, tr.transfer(idx, dist, labels, 7, V, weighting), (method, weighting, "restatement"))
            # some outputs NULL
            pred, values = np.full(130, -7, dtype=np.int32), np.full((130, 3), -7.0)
            sa._lib.check(L.sgl_knn_index_map(c._h, Qt.ctypes.data_as(f64p), 130, 33, 5, tr.WEIGHTINGS[weighting], None, None, pred.ctypes.data_as(i32p),
                                              None, None, values.ctypes.data_as(f64p)))
            assert np.array_equal(pred, want["predicted"]) and np.array_equal(values, want["values"], equal_nan=True)
            best = np.full(130, -7.0)
            sa._lib.check(L.sgl_knn_index_map(c._h, Qt.ctypes.data_as(f64p), 130, 33, 5, tr.WEIGHTINGS[weighting], None, None, None, best.ctypes.data_as(f64p),
                                              None, None))
            assert np.array_equal(best, want["score"])
        # labels alone on a fresh index: no values come back
        c.knn_index_build(R, None, "cosine", method, 64, 3)
        c.knn_index_annotate(labels)
        out = c.knn_index_map(Q, 33, 5)
        assert out["values"] is None and out["scores"].shape == (130, 7)


# ------------------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _clustered():
    X, label = ivf.clustered(2000, 20, 12)
    return X[:, :1600], label[:1600].astype(np.int32), X[:, 1600:], label[1600:]


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("lists", [(12, 3), (40, 4)], ids=["l12-p3", "l40-p4"])
def test_label_transfer_end_to_end_on_the_clustered_fixture(sa, lists, metric):
    n_lists, n_probe = lists
    Rx, lab, Qx, truth = _clustered()
    idx, dist = ivf.knn_ivf(Rx, Qx, 20, None, metric, n_lists, n_probe, 10)[:2]
    V = np.random.default_rng(8).standard_normal((2, 1600))
    with sa.ReferenceIndex(Rx.T, lab, V.T, metric=metric, n_lists=n_lists) as index:
        for weighting in ("distance", "uniform"):
            want = tr.transfer(idx, dist, lab, 12, V, weighting)
            got = index.map(Qx.T, 20, n_probe, weighting)          # raises if a query comes back short
            _same((got["idx"], got["dist"]), (idx, dist), (lists, metric))
            _same_transfer(got, want, (lists, metric, weighting))
            assert not (got["idx"] < 0).any() and index.info()["last_short_queries"] == 0
            assert np.array_equal(got["predicted"], truth), (lists, metric, weighting, float((got["predicted"] == truth).mean()))


# -------------------------------------------------------------------------------------------------------------- map_query
def _pbmc3k(sa):
    g = np.load(os.path.join(GOLD, "pbmc3k_counts.npz"))
    p, di, x = g["p"].astype(np.int64), g["di"].astype(np.int64), g["x"].astype(np.float64)
    cs = np.cumsum(di)
    i = cs - np.repeat(cs[p[:-1]] - di[p[:-1]], np.diff(p))      # undo the per-column delta coding
    m = int(g["dim"][0])

    def cells(lo, hi):
        return sa.dgCMatrix(x[p[lo]:p[hi]], i[p[lo]:p[hi]].astype(np.int32), (p[lo:hi + 1] - p[lo]).astype(np.int32), (m, hi - lo))
    return cells


def test_map_query_is_project_model_followed_by_the_index_map(sa):
    cells = _pbmc3k(sa)
    ref, query = sa.PreprocessData(cells(0, 2000)), sa.PreprocessData(cells(2000, 2700))
    model = sa.run_nmf(ref, 10, tol=1e-4, maxit=8, verbose=False, seed=7)
    assert model["h"].shape == (10, 2000)
    labels = np.argmax(model["h"], axis=0).astype(np.int32)            # a stand-in for cluster labels: the strongest factor
    coords = np.random.default_rng(3).standard_normal((2000, 2))
    with sa.ReferenceIndex(model["h"].T, labels, coords, metric="cosine") as index:
        got = sa.map_query(query, model["w"], index, n_neighbors=20, n_probe=12)
        assert set(got) == {"h", "d", "idx", "dist", "predicted", "score", "scores", "values"}
        pm = sa.project_model(query, model["w"], 0.01, 0)
        by_hand = index.map(np.asarray(pm["h"]).T, 20, 12, "distance")
        assert np.array_equal(got["h"], pm["h"]) and np.array_equal(got["d"], pm["d"])
        for key in ("idx", "dist", "predicted", "score", "scores", "values"):
            assert np.array_equal(got[key], by_hand[key], equal_nan=True), key
        assert got["idx"].shape == (700, 20) and got["scores"].shape == (700, 10) and got["values"].shape == (700, 2)
        print("pbmc3k map_query: share of query cells whose transferred label is their own strongest factor",
              float((got["predicted"] == np.argmax(got["h"], axis=0)).mean()))
        native = sa.map_query(sa.native((query.x, query.i, query.p, (query.nrow, query.ncol), "csc")), model["w"], index, n_neighbors=20, n_probe=12)
        assert np.array_equal(native["h"], got["h"]) and np.array_equal(native["predicted"], got["predicted"])
