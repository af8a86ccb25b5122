"""The inverted-list neighbour search on the GPU (sgl_knn_ivf / sgl_c_knn_ivf / sgl_knn_ivf_info / sgl_op_ivf_train /
sgl_op_ivf_search; method = "ivf" of Context.knn, knn, find_neighbors, run_umap) against the numpy restatement of its rules
(tests/knn_ivf_restatement.py) and against the exact search.  Every comparison is np.array_equal: the rules are exact, there is
no tolerance and no share of cases left out."""
import ctypes as C
import functools

import numpy as np
import pytest

import embedding_knn_restatement as euclid
import knn_ivf_restatement as ivf
import knn_metric_restatement as km
from conftest import to_dgc

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -6
METRICS = ("euclidean", "cosine", "correlation")
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64, what
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[1], want[1]), (what, "dist")
    assert not np.signbit(got[1]).any(), (what, "a negative zero")


def _nmf_like(rng, k, n):
    """Non-negative with many exact zeros (whole zero columns at small k), as an H looks."""
    X = rng.random((k, n)) * (rng.random((k, n)) < 0.4)
    X[:, 0] += 1e-3
    return X


# ------------------------------------------------------------------------------------------------- the training operator
# (n_dims, n_ref, n_lists, n_iter, data)
TRAIN = [
    (5, 100, 1, 3, "nmf"),            # one list
    (3, 40, 40, 2, "normal"),         # a list per cell
    (4, 130, 3, 5, "nmf"),            # all cells train
    (6, 300, 2, 4, "normal"),         # a subsample: T = 128
    (4, 130, 3, 4, "two"),            # two distinct integer columns, three lists: list 1 stays empty through every step
    (4, 130, 3, 0, "dup"),            # no step; seeds 0 and 1 are equal columns: list 1 is empty
    (20, 193, 3, 0, "normal"),        # 64 n_lists + 1 cells, no step
    (70, 150, 5, 3, "normal"),        # the generic instance of the assignment pass
    (9, 600, 9, 3, "skew"),           # a list of more than 256 training cells: two chunks in the centroid's sum
]


@functools.lru_cache(maxsize=None)
def _train_data(nd, n_ref, kind):
    rng = np.random.default_rng([nd, n_ref, len(kind)])
    if kind == "normal":
        R = rng.standard_normal((nd, n_ref))
    elif kind == "two":
        R = np.where(np.arange(n_ref)[None, :] < n_ref // 2, rng.integers(0, 9, (nd, 1)), rng.integers(0, 9, (nd, 1))).astype(np.float64)
    elif kind == "skew":
        R = rng.standard_normal((nd, n_ref)) * 0.05 + 3.0
        R[:, ::7] = rng.standard_normal((nd, R[:, ::7].shape[1])) * 4.0
    else:
        R = _nmf_like(rng, nd, n_ref)
        R[:, 7] = 0.0                  # a zero column: without direction under cosine
        if kind == "dup":
            R[:, 43] = R[:, 0]
    R.setflags(write=False)
    return R


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", TRAIN, ids=["d%d-r%d-l%d-i%d-%s" % c for c in TRAIN])
def test_training_operator_bit_for_bit(ctx, case, metric):
    nd, n_ref, n_lists, n_iter, kind = case
    R = _train_data(nd, n_ref, kind)
    C_want, a_want = ivf.train(ivf.operands(R, None, None, metric)[0], n_lists, n_iter)
    C_got, a_got = ctx.op_ivf_train(n_lists, R, None, metric, n_iter)
    counts = np.bincount(a_want, minlength=n_lists)
    print(case, metric, "lists", counts.min(), counts.max(), "empty", int((counts == 0).sum()))
    assert a_got.dtype == np.int32 and np.array_equal(a_got, a_want)
    assert C_got.shape == (nd, n_lists) and np.array_equal(C_got, C_want)
    if kind in ("two", "dup") and metric == "euclidean":
        assert counts[1] == 0
    if kind == "skew" and metric == "euclidean":
        assert counts.max() > 256
    if (nd, n_ref, n_lists) == (6, 300, 2):
        assert ivf.train_count(n_ref, n_lists) == 128


def test_training_operator_with_dims_and_the_resident_h(sa, ora):
    A = ora.synth_csc(40, 300, 6)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        c.fit_init(5)
        for _ in range(3):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        H = c.get_factors()[2]
        for metric in METRICS:
            want = ivf.train(ivf.operands(H.T, None, [3, 0, 4], metric)[0], 6, 3)
            for got in (c.op_ivf_train(6, None, [3, 0, 4], metric, 3), c.op_ivf_train(6, H.T, [3, 0, 4], metric, 3)):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), metric
        assert np.array_equal(c.get_factors()[2].view(np.uint64), H.view(np.uint64))


# --------------------------------------------------------------------------------------------------- the search operator
# (n_dims, n_neighbors): all five instance families (n_dims up to 8, 16, 32, 64, above) with both homes of the candidate lists
# (LDS up to 32 neighbours, global scratch above)
SHAPES = [(1, 1), (1, 33), (8, 20), (8, 256), (9, 32), (9, 33), (16, 20), (16, 256), (17, 1), (17, 33), (32, 32), (32, 256),
          (33, 20), (33, 33), (50, 32), (50, 256), (64, 1), (64, 33), (66, 20), (66, 33), (130, 32), (130, 256)]
N_REF = 65 + 129 + 70    # a list of 65, a list of 129, the rest


def _instance(nd):
    return 0 if nd <= 8 else 1 if nd <= 16 else 2 if nd <= 32 else 3 if nd <= 64 else 4


def test_the_grid_reaches_every_instance_with_both_list_homes(ctx):
    assert {nd for nd, _ in SHAPES} == {1, 8, 9, 16, 17, 32, 33, 50, 64, 66, 130} and {K for _, K in SHAPES} == {1, 20, 32, 33, 256}
    reached = set()
    for nd, K in SHAPES:
        R = np.random.default_rng(nd).standard_normal((nd, N_REF))
        ctx.op_ivf_search(np.zeros((nd, 1)), np.zeros(N_REF, dtype=np.int32), 1, K, R, R[:, :2])
        info = ctx.knn_ivf_info()
        assert info["instance"] == _instance(nd) and (info["n_lists"], info["n_probe"], info["train_cells"]) == (1, 1, 0)
        assert (info["shortest_list"], info["longest_list"], info["empty_lists"], info["short_queries"]) == (N_REF, N_REF, 0, 0)
        reached.add((info["instance"], K > 32))
    assert reached == {(i, g) for i in range(5) for g in (False, True)}


def _assignments(rng, nd):
    """name -> (centroids nd x n_lists, assign, n_probe): hand-made, none of them what a training would produce."""
    out = {}
    out["one list"] = (rng.standard_normal((nd, 1)), np.zeros(N_REF, dtype=np.int32), 1)
    out["a member per list"] = (rng.standard_normal((nd, N_REF)), rng.permutation(N_REF).astype(np.int32), 40)
    a = rng.choice(np.array([0, 2, 5], dtype=np.int32), N_REF)
    out["empty lists among the probed"] = (rng.standard_normal((nd, 6)), a, 4)
    a = np.full(N_REF, 2, dtype=np.int32)
    a[rng.permutation(N_REF)[:65]] = 0
    a[np.flatnonzero(a == 2)[:129]] = 1
    out["65 and 129"] = (rng.standard_normal((nd, 3)), a, 3)     # every list probed by every query: 1, 63, 64, 65 pairs per list
    short = np.arange(N_REF, dtype=np.int32) % 90                    # lists of 2 or 3 members, 5 probed: at most 15 candidates
    out["short lists"] = (rng.standard_normal((nd, 90)), short, 5)
    return out


@functools.lru_cache(maxsize=None)
def _search_case(nd, metric):
    rng = np.random.default_rng([nd, len(metric)])
    R = _nmf_like(rng, nd, N_REF) if nd % 2 else rng.standard_normal((nd, N_REF))
    R[:, 100:104] = R[:, [100]]                # duplicates: ties inside a list and across lists
    Q = rng.standard_normal((nd, 65)) if nd % 2 == 0 else _nmf_like(rng, nd, 65)
    Q[:, 1] = R[:, 50] * 4.0
    Rs, Qs = ivf.operands(R, Q, None, metric)
    for a in (R, Q, Rs, Qs):
        a.setflags(write=False)
    return R, Q, Rs, Qs, _assignments(rng, nd)


GRID = [(s, m) for s in SHAPES for m in METRICS]


@pytest.mark.parametrize("shape,metric", GRID, ids=["d%d-K%d-%s" % (s + (m,)) for s, m in GRID])
def test_search_operator_under_hand_made_assignments(ctx, shape, metric):
    nd, K = shape
    R, Q, Rs, Qs, assignments = _search_case(nd, metric)
    for name, (cent, assign, n_probe) in assignments.items():
        counts = np.bincount(assign, minlength=cent.shape[1])
        for nq in ((1, 63, 64, 65) if name == "65 and 129" else (65,)):
            want = ivf.search(Rs, Qs[:, :nq], metric, cent, assign, n_probe, K)
            got = ctx.op_ivf_search(cent, assign, n_probe, K, R, Q[:, :nq], None, metric)
            info = ctx.knn_ivf_info()
            what = (shape, metric, name, nq)
            _same(got, want, what)
            short = int((want[0] < 0).any(axis=1).sum())
            assert info == dict(n_lists=cent.shape[1], n_probe=n_probe, train_cells=0, shortest_list=int(counts.min()),
                                longest_list=int(counts.max()), empty_lists=int((counts == 0).sum()), short_queries=short,
                                instance=_instance(nd)), what
            if name == "short lists" and K > 15:
                assert short == nq and np.all(got[0][:, 15:] == -1) and np.all(np.isinf(got[1][:, 15:])), what
            if name == "65 and 129":
                assert sorted(counts.tolist()) == [65, 70, 129]
        # forced batches of 1, 7 and all queries: the same arrays (want: the 65 queries of the last round)
        for batch in (1, 7, 65):
            _same(ctx.op_ivf_search(cent, assign, n_probe, K, R, Q, None, metric, query_batch=batch), want, (shape, metric, name, "batch", batch))
        # the references themselves as the queries, in automatic batches and in batches of 100
        want = ivf.search(Rs, Rs, metric, cent, assign, n_probe, K)
        for batch in (0, 100):
            _same(ctx.op_ivf_search(cent, assign, n_probe, K, R, None, None, metric, query_batch=batch), want, (shape, metric, name, "self", batch))


# ----------------------------------------------------------------------------------------------------------- the whole call
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nd,n_ref,nq,K,n_lists", [(8, 300, 65, 20, 17), (20, 500, 130, 33, 64), (50, 257, 64, 20, 9), (70, 200, 33, 40, 6)])
def test_every_list_probed_is_the_exact_search_bit_for_bit(ctx, sa, metric, nd, n_ref, nq, K, n_lists):
    rng = np.random.default_rng([nd, n_ref, K])
    R, Q = _nmf_like(rng, nd, n_ref), _nmf_like(rng, nd, nq)
    R[:, 30:30 + K + 2] = R[:, [30]]           # more duplicates than neighbours
    exact_self, exact_query = ctx.knn(K, R, None, metric=metric), ctx.knn(K, R, Q, metric=metric)
    report = ctx.knn_info()
    kw = dict(metric=metric, method="ivf", n_lists=n_lists, n_probe=n_lists)
    _same(ctx.knn(K, R, None, **kw), exact_self, "self")
    info = ctx.knn_ivf_info()
    assert (info["n_lists"], info["n_probe"], info["train_cells"], info["short_queries"]) == (n_lists, n_lists, min(n_ref, 64 * n_lists), 0)
    _same(ctx.knn(K, R, Q, **kw), exact_query, "queries")
    _same(sa.knn(R, Q, K, **kw), exact_query, "one-shot")
    _same(ctx.knn(K, R, Q, n_iter=0, **kw), exact_query, "no Lloyd step")
    assert ctx.knn_info() == report            # the exact search's report is its own


@pytest.mark.parametrize("metric", METRICS)
def test_the_resident_h_with_dims(sa, ora, metric):
    A = ora.synth_csc(40, 300, 6)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        c.fit_init(5)
        for _ in range(3):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        H = c.get_factors()[2]
        Q = np.random.default_rng(2).random((5, 33))
        for dims in (None, [3, 0, 4]):
            kw = dict(dims=dims, metric=metric)
            _same(c.knn(20, method="ivf", n_lists=12, n_probe=12, **kw), c.knn(20, **kw), "resident, every list")
            _same(c.knn(7, None, Q, method="ivf", n_lists=12, n_probe=12, **kw), c.knn(7, None, Q, **kw), "resident, host queries")
            want = ivf.knn_ivf(H.T, None, 20, dims, metric, 12, 3, 10)
            _same(c.knn(20, method="ivf", n_lists=12, n_probe=3, **kw), want[:2], "resident, 3 of 12 lists")
            _same(c.knn(20, H.T, method="ivf", n_lists=12, n_probe=3, **kw), want[:2], "host R")
        assert np.array_equal(c.get_factors()[2].view(np.uint64), H.view(np.uint64))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nd,n_ref,nq,K,n_lists,n_probe,n_iter", [(6, 400, 70, 20, 20, 3, 10), (33, 300, None, 33, 12, 2, 4), (70, 260, 40, 10, 8, 1, 2)])
def test_fewer_probes_than_lists_is_the_restatement(ctx, sa, metric, nd, n_ref, nq, K, n_lists, n_probe, n_iter):
    rng = np.random.default_rng([nd, n_ref, n_lists])
    R = _nmf_like(rng, nd, n_ref)
    Q = None if nq is None else _nmf_like(rng, nd, nq)
    want = ivf.knn_ivf(R, Q, K, None, metric, n_lists, n_probe, n_iter)
    kw = dict(metric=metric, method="ivf", n_lists=n_lists, n_probe=n_probe, n_iter=n_iter)
    _same(ctx.knn(K, R, Q, **kw), want[:2], "context")
    counts = np.bincount(want[3], minlength=n_lists)
    assert ctx.knn_ivf_info() == dict(n_lists=n_lists, n_probe=n_probe, train_cells=ivf.train_count(n_ref, n_lists), shortest_list=int(counts.min()),
                                      longest_list=int(counts.max()), empty_lists=int((counts == 0).sum()),
                                      short_queries=int((want[0] < 0).any(axis=1).sum()), instance=_instance(nd))
    _same(sa.knn(R, Q, K, **kw), want[:2], "one-shot")
    got_train = ctx.op_ivf_train(n_lists, R, None, metric, n_iter)
    assert np.array_equal(got_train[0], want[2]) and np.array_equal(got_train[1], want[3])
    _same(ctx.op_ivf_search(want[2], want[3], n_probe, K, R, Q, None, metric), want[:2], "the operators composed")


def test_recall_on_clustered_data(ctx, sa):
    """The fixture "clustered" (tests/knn_ivf_restatement.py: 12 sparse non-negative profiles, multiplicative gamma noise, 2000
    cells x 20 dimensions) at 45 lists and 8 probes: the GPU equals the restatement, whose recall@20 against the exact
    restatement is at least 0.95 (tests/test_knn_ivf_restatement.py holds that precondition on the CPU)."""
    X, _ = ivf.clustered()
    want = ivf.knn_ivf(X, None, 20, None, "euclidean", 45, 8, 10)
    got = ctx.knn(20, X, method="ivf", n_lists=45, n_probe=8)
    _same(got, want[:2], "clustered")
    exact = ctx.knn(20, X)
    _same(exact, euclid.knn(X, None, 20), "exact")
    r = sa.knn_recall(got[0], exact[0])
    print("recall@20, 45 lists, 8 probes:", r, ctx.knn_ivf_info())
    assert r >= 0.95 and r == pytest.approx(ivf.recall(want[0], exact[0]), abs=1e-12)
    _same(ctx.knn(20, X, method="ivf"), ivf.knn_ivf(X, None, 20, None, "euclidean", *sa.api.knn_ivf_shape(2000), 10)[:2], "the defaults")


# -------------------------------------------------------------------------------------------------------------- refusals
def _refused(sa, code, match, fn):
    with pytest.raises(sa.SingletHipError, match=match) as e:
        fn()
    assert e.value.code == code, (match, e.value.code)


def _raw(sa, c, Rt, Qt, k, K, metric, n_lists, n_probe, n_iter, idx, dist):
    """sgl_knn_ivf on c (None: sgl_c_knn_ivf) with host operands (column-major images) -> the return code."""
    L = sa._lib.load()
    args = (Rt.ctypes.data_as(f64p), k, Rt.shape[0], Qt.ctypes.data_as(f64p), Qt.shape[0], None, 0, K, metric, n_lists, n_probe, n_iter,
            idx.ctypes.data_as(i32p), dist.ctypes.data_as(f64p))
    return L.sgl_c_knn_ivf(*args) if c is None else L.sgl_knn_ivf(c._h, *args)


def test_refusals_leave_outputs_report_and_context_as_they_were(sa):
    rng = np.random.default_rng(5)
    R, Q = rng.standard_normal((6, 40)), rng.standard_normal((6, 9))
    Rt, Qt = np.ascontiguousarray(R.T), np.ascontiguousarray(Q.T)
    kw = dict(metric="cosine", method="ivf", n_lists=5, n_probe=2, n_iter=3)
    want = ivf.knn_ivf(R, Q, 4, None, "cosine", 5, 2, 3)[:2]
    with sa.Context(0) as c:
        assert c.knn_ivf_info() == dict.fromkeys(("n_lists", "n_probe", "train_cells", "shortest_list", "longest_list", "empty_lists",
                                                  "short_queries", "instance"), 0)            # all 0 before the first search
        _same(c.knn(4, R, Q, **kw), want, "before")
        info = c.knn_ivf_info()
        assert info["n_lists"] == 5 and info["train_cells"] == 40
        for who, cc in (("sgl_knn_ivf", c), ("sgl_c_knn_ivf", None)):
            #        K, metric, n_lists, n_probe, n_iter -> message; each call breaks the later rules too: the stated order decides
            for args, message in (((0, 7, 0, 0, -1), r"n_neighbors = 0 is outside \[1, min\(256, n_ref = 40\)\]"),        # sgl_knn's own first
                                  ((4, 7, 0, 0, -1), r"n_lists = 0 is outside \[1, min\(n_ref = 40, 65536\)\]"),
                                  ((4, 7, 41, 0, -1), r"n_lists = 41 is outside \[1, min\(n_ref = 40, 65536\)\]"),
                                  ((4, 7, 5, 0, -1), r"n_probe = 0 is outside \[1, min\(n_lists = 5, 64\)\]"),
                                  ((4, 7, 5, 6, -1), r"n_probe = 6 is outside \[1, min\(n_lists = 5, 64\)\]"),
                                  ((4, 7, 5, 2, -1), r"n_iter = -1 is outside \[0, 1000\]"),
                                  ((4, 7, 5, 2, 1001), r"n_iter = 1001 is outside \[0, 1000\]"),
                                  ((4, 7, 5, 2, 3), r"metric = 7 is outside \[0, 2\]"),
                                  ((4, -1, 5, 2, 3), r"metric = -1 is outside \[0, 2\]")):
                idx, dist = np.full((9, 4), -7, dtype=np.int32), np.full((9, 4), -7.0)
                _refused(sa, EINVAL, r": %s: %s$" % (who, message), lambda: sa._lib.check(_raw(sa, cc, Rt, Qt, 6, args[0], args[1], *args[2:], idx, dist)))
                assert np.all(idx == -7) and np.all(dist == -7.0)          # the outputs are untouched
                assert c.knn_ivf_info() == info                            # the report is as it was
            _same(c.knn(4, R, Q, **kw), want, "after the refusals of " + who)
        big = rng.standard_normal((2, 200))
        _refused(sa, EINVAL, r"n_probe = 65 is outside \[1, min\(n_lists = 100, 64\)\]", lambda: c.knn(4, big, method="ivf", n_lists=100, n_probe=65))
        # a non-finite value: the message of sgl_knn on the raw operands, whatever the metric
        bad = R.copy()
        bad[4, 31] = np.inf
        bad[2, 5] = np.nan
        badq = Q.copy()
        badq[5, 8] = -np.inf
        _refused(sa, EINVAL, r"sgl_knn_ivf: R holds a non-finite value in column 5, row 2 \(0-based; the first in column-major order\)",
                 lambda: c.knn(4, bad, Q, **kw))
        _refused(sa, EINVAL, r"sgl_knn_ivf: Q holds a non-finite value in column 8, row 5 ", lambda: c.knn(4, R, badq, [0, 5], **kw))
        _refused(sa, EINVAL, r"sgl_c_knn_ivf: R holds a non-finite value in column 5, row 2 ", lambda: sa.knn(bad, Q, 4, **kw))
        _refused(sa, EINVAL, r"sgl_knn_ivf: dims\[1\] = 6 is outside \[0, k = 6\)", lambda: c.knn(4, R, Q, [2, 6], **kw))
        # the operators
        cent, assign = c.op_ivf_train(5, R, None, "cosine", 3)
        _refused(sa, EINVAL, r"sgl_op_ivf_train: n_lists = 41 is outside", lambda: c.op_ivf_train(41, R))
        _refused(sa, EINVAL, r"sgl_op_ivf_train: n_iter = 1001 is outside", lambda: c.op_ivf_train(5, R, n_iter=1001))
        _refused(sa, EINVAL, r"sgl_op_ivf_train: R holds a non-finite value in column 5, row 2 ", lambda: c.op_ivf_train(5, bad))
        wrong = assign.copy()
        wrong[17], wrong[30] = 5, -1
        _refused(sa, EINVAL, r"sgl_op_ivf_search: assign\[17\] = 5 is outside \[0, n_lists = 5\)$", lambda: c.op_ivf_search(cent, wrong, 2, 4, R, Q, None, "cosine"))
        _refused(sa, EINVAL, r"sgl_op_ivf_search: n_probe = 6 is outside", lambda: c.op_ivf_search(cent, assign, 6, 4, R, Q, None, "cosine"))
        _refused(sa, EINVAL, r"sgl_op_ivf_search: query_batch = -1 is negative", lambda: c.op_ivf_search(cent, assign, 2, 4, R, Q, None, "cosine", -1))
        nan_cent = cent.copy()
        nan_cent[1, 3] = np.nan
        _refused(sa, EINVAL, r"sgl_op_ivf_search: centroids holds a non-finite value in column 3, row 1 ", lambda: c.op_ivf_search(nan_cent, assign, 2, 4, R, Q, None, "cosine"))
        assert c.knn_ivf_info() == info
        _same(c.op_ivf_search(cent, assign, 2, 4, R, Q, None, "cosine"), want, "the operators, after the refusals")
        # no fit: R = NULL is a matter of state, before the arguments
        _refused(sa, ESTATE, r"sgl_knn_ivf: R is NULL and no fit is initialised", lambda: sa._lib.check(
            sa._lib.load().sgl_knn_ivf(c._h, None, 6, 40, None, 40, None, 0, 0, 7, 0, 0, -1, None, None)))
        _same(c.knn(4, R, Q, **kw), want, "after everything")
    _same(sa.knn(R, Q, 4, **kw), want, "one-shot, after the refusals")


def test_a_context_with_an_allreduce_hook_is_refused(sa):
    R = np.random.default_rng(1).standard_normal((3, 30))
    with sa.Context(0) as c:
        c.set_allreduce(lambda dev_ptr, count: None)
        _refused(sa, ESTATE, r"sgl_knn_ivf: the context is a shard of a team or has an all-reduce hook", lambda: c.knn(3, R, method="ivf", n_lists=0))
        _refused(sa, ESTATE, r"sgl_op_ivf_train: the context is a shard of a team", lambda: c.op_ivf_train(0, R))
        _refused(sa, ESTATE, r"sgl_op_ivf_search: the context is a shard of a team", lambda: c.op_ivf_search(np.zeros((3, 1)), np.zeros(30, dtype=np.int32), 1, 3, R))
        c.set_allreduce(None)
        _same(c.knn(3, R, method="ivf", n_lists=4, n_probe=4), c.knn(3, R), "hook cleared")


def test_a_fit_continued_after_a_search_gives_the_same_bits(sa, ora):
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
                _same(c.knn(20, method="ivf", n_lists=10, n_probe=3), ivf.knn_ivf(H.T, None, 20, None, "euclidean", 10, 3, 10)[:2], "mid-fit")
                c.knn(40, np.ones((70, 90)) * np.arange(90), None, [1, 5], metric="correlation", method="ivf", n_lists=4, n_probe=4)
                assert np.array_equal(c.get_factors()[2], H)
            trace += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            runs[with_knn] = (c.get_factors(), trace, c.sweeps_get(reset=True))
    for x, y, name in zip(runs[True][0], runs[False][0], "wdh"):
        assert np.array_equal(x, y), name
    assert runs[True][1] == runs[False][1]
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], key


# ------------------------------------------------------------------------------------------------------------ downstream
def test_find_neighbors_and_run_umap_with_every_list_probed_are_the_exact_calls(sa):
    X, _ = km.rays(8, 400)
    for metric in ("euclidean", "cosine"):
        a = sa.find_neighbors(X.T, 12, metric=metric)
        b = sa.find_neighbors(X.T, 12, metric=metric, nn_method="ivf", n_lists=9, n_probe=9)
        assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["dist"], b["dist"])
        for g in ("nn", "snn"):
            assert np.array_equal(a[g].p, b[g].p) and np.array_equal(a[g].i, b[g].i) and np.array_equal(a[g].x, b[g].x)
    Ya = sa.run_umap(X, 10, n_epochs=20, seed=3)
    Yb = sa.run_umap(X, 10, n_epochs=20, seed=3, nn_method="ivf", n_lists=9, n_probe=9)
    assert np.array_equal(Ya, Yb)
    # one probe among a list per two cells cannot hold 12 neighbours: nothing short may reach the graphs
    with pytest.raises(ValueError, match="n_probe"):
        sa.find_neighbors(X.T, 12, nn_method="ivf", n_lists=200, n_probe=1)
    with pytest.raises(ValueError, match="n_probe"):
        sa.run_umap(X, 10, n_epochs=20, nn_method="ivf", n_lists=200, n_probe=1)
