"""The layout transform on the GPU (sgl_c_fuzzy_query, sgl_c_umap_transform, sgl_op_umap_transform_epochs,
sgl_knn_index_set_layout, sgl_knn_index_project) against the numpy restatement of its rules
(tests/umap_transform_restatement.py).  rho is held bit for bit, sigma and W to the ulps of the device's exp; from given
memberships the epochs with a = b = 1 are held bit for bit (no transcendental is left), one epoch at general b to the bound
of pow; the index form is held bit for bit to the search followed by the transform.  All shapes are small on purpose."""
import functools
import os

import numpy as np
import pytest

import umap_restatement as ur
import umap_transform_restatement as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
INF = np.inf
N_REF = 1000
QNAN_BITS = 0x7FF8000000000000
A_GEN, B_GEN = 1.5769434603113077, 0.8950608779109733      # find_ab_params(1.0, 0.1) to the digits shown

# The largest relative difference of sigma and of W between the device and the restatement over the membership fixtures
# below, measured on the MI355X (the test prints it): only the device's exp separates the two.  The tests allow 16 x this.
# The rule of this constant: it is never more than 1e-9.
FUZZY_REL_MEASURED = 2.9e-14    # W at n = 1000, K = 256: 2.860e-14; sigma at most 4.5e-16
# A membership below this has no relative precision left to hold (it nears the subnormals): such a W is compared absolutely,
# against the tolerance times this floor.
W_FLOOR = 1e-300


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def lists(seed, n, K, n_ref=N_REF):
    """n ascending lists of K distinct references each; no padding, no zeros."""
    rng = np.random.default_rng(seed)
    idx = np.argsort(rng.random((n, n_ref)), axis=1)[:, :K].astype(np.int32)
    dist = np.sort(rng.random((n, K)) * 3.0 + 0.01, axis=1)
    return idx, dist


def pad(idx, dist, q, keep):
    idx[q, keep:], dist[q, keep:] = -1, INF


# ------------------------------------------------------------------------------------------------------------- memberships
@functools.lru_cache(maxsize=None)
def membership_case(n, K):
    idx, dist = lists(100 * n + K, n, K)
    for q in range(0, n, 7):
        dist[q] = 0.0                                            # all-zero distances
    for q in range(3, n, 11):
        dist[q, :1 + q % K] = 0.0                                # some leading zeros
    for q, keep in ((1, K - 1), (2, 1), (4, 0)):                 # 1, K - 1 and K padding slots
        if q < n:
            pad(idx, dist, q, keep)
    if n == 1 and K > 1:
        pad(idx, dist, 0, K - 1)
    rho, sigma, W = tr.fuzzy_query(idx, dist)
    return idx, dist, rho, sigma, W


def rel(got, want, floor=0.0):
    """The largest |got - want| / max(|want|, floor) over the entries where that denominator is not 0."""
    den = np.maximum(np.abs(want), floor)
    m = den > 0
    return float((np.abs(got - want)[m] / den[m]).max()) if m.any() else 0.0


@pytest.mark.parametrize("K", [1, 2, 31, 256])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_memberships(sa, n, K):
    idx, dist, rho, sigma, W = membership_case(n, K)
    gW, grho, gsigma = sa.fuzzy_query(idx, dist, N_REF)
    assert np.array_equal(bits(grho), bits(rho))
    own = idx >= 0
    empty = ~own.any(axis=1)
    assert (bits(gW[~own]) == 0).all() and (bits(gsigma[empty]) == 0).all() and (bits(grho[empty]) == 0).all()
    assert ((gW == 1.0) & own).any(axis=1)[~empty].all(), "every non-empty list holds a membership of exactly 1.0"
    zero = (rho == 0) & ~empty
    assert (gW[zero][own[zero]] == 1.0).all()
    r_sigma, r_w = rel(gsigma, sigma), rel(gW, W, W_FLOOR)
    print("memberships n %d K %d: rel sigma %.3e, rel W %.3e" % (n, K, r_sigma, r_w))
    assert FUZZY_REL_MEASURED <= 1e-9
    assert r_sigma <= 16 * FUZZY_REL_MEASURED and r_w <= 16 * FUZZY_REL_MEASURED


# ------------------------------------------------------------------------------------------- epochs at a = b = 1, bit for bit
N_Q, N_EPOCHS, SEED = 701, 30, 77


@functools.lru_cache(maxsize=None)
def layout_ref(dim):
    Yref = np.random.default_rng(dim).normal(size=(N_REF, dim)) * 4.0
    Yref[::10] = Yref[0]                 # a hundred references in one place: samples that land on a query sitting there
    return Yref


@functools.lru_cache(maxsize=None)
def epoch_case(dim, K, neg_rate):
    """Lists with padding and an empty one, the restatement's memberships, starts of which some coincide with references,
    and the restatement's result: computed once and shared, never changed."""
    idx, dist = lists(1000 * dim + K, N_Q, K)
    dist[1] = 0.0                        # every slot at membership 1.0: all K slots fire in every epoch (K = 256, 255 samples:
    for q in (10, 19, 28):               # 1024 rounds of 64 terms per epoch); 41 .. 59 leading zeros: nearly full ballots
        dist[q, :min(K, 31 + q)] = 0.0
    for q in range(5, N_Q, 9):
        pad(idx, dist, q, q % K)         # short lists, the empty one among them (q % K == 0)
    pad(idx, dist, 0, 0)
    _, _, W = tr.fuzzy_query(idx, dist)
    Yref = layout_ref(dim)
    Y0 = tr.start(idx, W, Yref)
    own0 = idx[:, 0] >= 0
    for q in range(2, N_Q, 4):
        if own0[q]:
            Y0[q] = Yref[idx[q, 0]]      # on top of its nearest reference: the attractive term at d2 == 0
    for q in range(3, N_Q, 8):
        if own0[q]:
            Y0[q] = Yref[0]              # on top of the hundred
    for a in (idx, W, Yref, Y0):
        a.setflags(write=False)
    want = tr.epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 0.25, neg_rate, SEED)
    want.setflags(write=False)
    return idx, W, Yref, Y0, want


CASES = [(2, 1, 0, 1), (2, 15, 5, 1), (3, 64, 63, 3), (5, 65, 5, 5), (2, 256, 255, 1), (3, 256, 5, 3), (5, 15, 63, 5), (2, 65, 0, 1), (3, 1, 255, 3)]


@pytest.mark.parametrize("dim,K,neg_rate,instance", CASES)
def test_epochs_bit_for_bit(sa, dim, K, neg_rate, instance):
    idx, W, Yref, Y0, want = epoch_case(dim, K, neg_rate)
    got = sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS, 0.25, neg_rate, SEED)
    info = sa.umap_transform_info()
    own = idx >= 0
    assert info == dict(instance=instance, widest_list=int(own.sum(axis=1).max()), empty_queries=int((~own.any(axis=1)).sum()), launches=1), info
    assert info["empty_queries"] >= 1 and info["widest_list"] == K
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).any(axis=1).sum())
    assert (bits(got[~own.any(axis=1)]) == QNAN_BITS).all()
    moved = (bits(got) != bits(Y0)).any(axis=1)
    if K == 1 and neg_rate == 0:
        # one slot of membership 1.0 puts the start ON its reference, the attractive term at d2 == 0 is +0.0 and no sample
        # pushes: only the queries that were moved onto another place travel
        assert not moved[(bits(Y0) == bits(Yref[np.maximum(idx[:, 0], 0)])).all(axis=1)].any() and moved.any()
    else:
        assert moved[own.any(axis=1)].mean() > 0.9
    again = sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS, 0.25, neg_rate, SEED)
    assert np.array_equal(bits(again), bits(got)), "run twice, equal bits"
    if neg_rate:
        other = sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS, 0.25, neg_rate, SEED + 1)
        assert not np.array_equal(bits(other), bits(got)), "the seed matters"


@pytest.mark.parametrize("dim,K,neg_rate", [(2, 15, 5), (3, 65, 5), (5, 256, 5)])
def test_chaining_and_slices(sa, dim, K, neg_rate):
    idx, W, Yref, Y0, want = epoch_case(dim, K, neg_rate)
    kw = dict(alpha0=0.25, neg_rate=neg_rate, seed=SEED)
    mid = sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 1, 7, **kw)
    assert np.array_equal(bits(mid), bits(tr.epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 0.25, neg_rate, SEED, 0, 1, 7)))
    end = sa.op_umap_transform_epochs(idx, W, Yref, mid, 1.0, 1.0, N_EPOCHS, 8, N_EPOCHS, **kw)
    assert np.array_equal(bits(end), bits(want)), "epochs 1..7 then 8..30 equal 1..30 (the NaN of the empty query is passed on unread)"
    for lo, hi in ((0, 1), (64, 129), (300, N_Q)):
        part = sa.op_umap_transform_epochs(idx[lo:hi], W[lo:hi], Yref, Y0[lo:hi], 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS, query_offset=lo, **kw)
        assert np.array_equal(bits(part), bits(want[lo:hi])), (lo, hi)
    part = sa.op_umap_transform_epochs(idx[64:129], W[64:129], Yref, Y0[64:129], 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS, **kw)
    assert not np.array_equal(bits(part), bits(want[64:129])), "without its offset a slice draws other samples"


def test_the_cut_into_launches_does_not_change_the_result(sa, monkeypatch):
    """300 epochs are three launches (128 + 128 + 44); the stage operator cut anywhere gives the same bits, and so does the
    profiling switch that asks for launches of 7 epochs."""
    idx, W, Yref, Y0, _ = epoch_case(2, 15, 5)
    idx, W, Y0 = idx[:130], W[:130], Y0[:130]
    kw = dict(alpha0=0.25, neg_rate=2, seed=5)
    whole = sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, 300, 1, 300, **kw)
    assert sa.umap_transform_info()["launches"] == 3
    assert np.array_equal(bits(whole), bits(tr.epochs(idx, W, Yref, Y0, 1.0, 1.0, 300, 0.25, 2, 5)))
    y = Y0
    for lo, hi in ((1, 100), (101, 101), (102, 300)):
        y = sa.op_umap_transform_epochs(idx, W, Yref, y, 1.0, 1.0, 300, lo, hi, **kw)
    assert np.array_equal(bits(y), bits(whole))
    monkeypatch.setenv("SGL_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH", "7")
    cut = sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, 300, 1, 300, **kw)
    assert sa.umap_transform_info()["launches"] == 43 and np.array_equal(bits(cut), bits(whole))


# --------------------------------------------------------------------------------------------------- the whole transform
def test_whole_transform_slices_repeats_and_seed(sa):
    idx, dist = lists(9, 300, 15)
    pad(idx, dist, 7, 4)
    pad(idx, dist, 8, 0)
    Yref = layout_ref(2)
    Y0, Y = sa.umap_transform(idx, dist, Yref, A_GEN, B_GEN, 30, seed=3, return_init=True)
    info = sa.umap_transform_info()
    assert info == dict(instance=0, widest_list=15, empty_queries=1, launches=1)
    # the start and the epochs are the stage forms of the device's own memberships, bit for bit
    W, rho, sigma = sa.fuzzy_query(idx, dist, N_REF)
    assert np.array_equal(bits(Y0), bits(tr.start(idx, W, Yref)))
    assert np.array_equal(bits(Y), bits(sa.op_umap_transform_epochs(idx, W, Yref, Y0, A_GEN, B_GEN, 30, 1, 30, seed=3)))
    assert (bits(Y[8]) == QNAN_BITS).all() and (bits(Y0[8]) == QNAN_BITS).all() and np.isfinite(np.delete(Y, 8, axis=0)).all()
    # against the restatement: close (exp and pow separate them), not bit for bit
    r0, r = tr.transform(idx, dist, Yref, A_GEN, B_GEN, 30, seed=3)
    ok = np.arange(300) != 8
    assert np.allclose(Y0[ok], r0[ok], rtol=1e-9, atol=1e-9)
    print("whole transform vs restatement: median |dy| %.3e" % float(np.median(np.abs(Y[ok] - r[ok]))))
    assert np.array_equal(bits(sa.umap_transform(idx, dist, Yref, A_GEN, B_GEN, 30, seed=3)), bits(Y)), "run twice, equal bits"
    assert not np.array_equal(bits(sa.umap_transform(idx, dist, Yref, A_GEN, B_GEN, 30, seed=4)), bits(Y)), "the seed matters"
    for lo, hi in ((0, 64), (64, 65), (65, 300)):
        p0, p = sa.umap_transform(idx[lo:hi], dist[lo:hi], Yref, A_GEN, B_GEN, 30, seed=3, query_offset=lo, return_init=True)
        assert np.array_equal(bits(p0), bits(Y0[lo:hi])) and np.array_equal(bits(p), bits(Y[lo:hi]))
    from singlet_amd import api
    assert np.array_equal(bits(api.umap_transform(idx, dist, Yref, A_GEN, B_GEN, seed=3)),
                          bits(api.umap_transform(idx, dist, Yref, A_GEN, B_GEN, 100, seed=3))), "100 epochs up to 10 000 queries"


# --------------------------------------------------------------------------------------------------- one epoch at general b
@pytest.mark.parametrize("neg_rate", [0, 5])
@pytest.mark.parametrize("dim,instance", [(2, 0), (3, 2), (5, 4)])
def test_one_epoch_general_b_within_the_bound_of_pow(sa, dim, instance, neg_rate):
    """|y' - y'_restated| <= 32 eps alpha_t S_f + 2 eps |y| per component, S_f the sum of the absolute clipped terms of the
    query: the OpenCL bound of 16 ulp for pow dominates each term's few roundings, clip is continuous, and the branches are
    decided by exact quantities (the existing layout test's bound, for its stated reason)."""
    idx, W, Yref, Y0, _ = epoch_case(dim, 65, 5)
    live = (idx >= 0).any(axis=1)
    for t in (1, 7):
        want, S = tr.epochs(idx, W, Yref, Y0, A_GEN, B_GEN, 10, 1.0, neg_rate, 99, 0, t, t, with_bound=True)
        got = sa.op_umap_transform_epochs(idx, W, Yref, Y0, A_GEN, B_GEN, 10, t, t, 1.0, neg_rate, 99)
        assert sa.umap_transform_info()["instance"] == instance
        bound = 32 * EPS * ur.alpha_of(1.0, t, 10) * S + 2 * EPS * np.abs(Y0)
        err = np.abs(got - want)[live]
        print("epoch dim %d neg %d t %d: max err %.3e, max err / bound %.3f" % (dim, neg_rate, t, err.max(), (err / np.maximum(bound[live], 1e-300)).max()))
        assert (err <= bound[live]).all(), (dim, neg_rate, t, float((err - bound[live]).max()))
        still = ~(tr.firing(W, t) & (idx >= 0)).any(axis=1) & live
        assert np.array_equal(bits(got[still]), bits(Y0[still])), "a query without a firing slot keeps its bits"
        assert (bits(got[~live]) == QNAN_BITS).all()
    # memberships of at most 0.3 (the stage operator takes any W in [0, 1]): nothing fires in epoch 1; in epoch 5 the slots
    # at 0.3 rest (floor(1.5) == floor(1.2)) and those in [0.2, 0.25) fire, which about two queries in three hold
    low = np.asarray(W) * 0.3
    got = sa.op_umap_transform_epochs(idx, low, Yref, Y0, A_GEN, B_GEN, 10, 1, 1, 1.0, neg_rate, 99)
    assert np.array_equal(bits(got[live]), bits(Y0[live])), "a query without a firing slot keeps its bits"
    got = sa.op_umap_transform_epochs(idx, low, Yref, Y0, A_GEN, B_GEN, 10, 5, 5, 1.0, neg_rate, 99)
    fired = (tr.firing(low, 5) & (idx >= 0)).any(axis=1)
    assert fired[live].any() and not fired[live].all()
    assert np.array_equal(bits(got[live & ~fired]), bits(Y0[live & ~fired]))
    assert (bits(got[live & fired]) != bits(Y0[live & fired])).any(axis=1).mean() > 0.9


# ------------------------------------------------------------------------------------------------------------- index form
@pytest.fixture(scope="module")
def indexed():
    rng = np.random.default_rng(21)
    centres = rng.normal(size=(8, 5)) * 6.0
    R = centres[rng.integers(0, 8, N_REF)] + rng.normal(size=(N_REF, 5))
    Q = centres[rng.integers(0, 8, 150)] + rng.normal(size=(150, 5))
    Q[3] = R[10]
    return R, Q, layout_ref(2)


@pytest.mark.parametrize("method", ["exact", "ivf"])
def test_index_project_equals_search_then_transform(sa, indexed, method):
    R, Q, Yref = indexed
    with sa.Context(0) as c:
        with pytest.raises(sa.SingletHipError, match="holds no neighbour index") as e:
            c.knn_index_project(Q.T, A_GEN, B_GEN)
        assert e.value.code == -6
        c.knn_index_build(R.T, None, "euclidean", method, 100 if method == "ivf" else None)
        with pytest.raises(sa.SingletHipError, match="holds no layout") as e:
            c.knn_index_project(Q.T, A_GEN, B_GEN)
        assert e.value.code == -6
        bytes0 = c.knn_index_info()["bytes"]
        c.knn_index_set_layout(np.zeros((3, N_REF)))
        assert c.knn_index_info()["bytes"] == bytes0 + 8 * 3 * N_REF
        c.knn_index_set_layout(Yref.T)                       # a second call replaces the first
        assert c.knn_index_info()["bytes"] == bytes0 + 8 * 2 * N_REF
        n_probe = 1 if method == "ivf" else None
        idx, dist = c.knn_index_search(Q.T, 15, n_probe)
        Y0, Y = sa.umap_transform(idx, dist, Yref, A_GEN, B_GEN, 30, seed=3, return_init=True)
        short = int((idx < 0).any(axis=1).sum())
        for query_batch in (1, 64, 0):
            out = c.knn_index_project(Q.T, A_GEN, B_GEN, 15, n_probe, 30, seed=3, query_batch=query_batch)
            assert np.array_equal(out["idx"], idx) and np.array_equal(bits(out["dist"]), bits(dist))
            assert np.array_equal(bits(out["layout_init"]), bits(Y0)) and np.array_equal(bits(out["layout"]), bits(Y)), query_batch
            info = sa.umap_transform_info()
            assert info["instance"] == 0 and info["widest_list"] == 15 and info["empty_queries"] == int((idx < 0).all(axis=1).sum())
            assert info["launches"] == (150 if query_batch == 1 else 3 if query_batch == 64 else info["launches"])
            assert c.knn_index_info()["last_short_queries"] == short, "a query that comes back short is counted"
        if method == "ivf":
            assert short > 0, "one probe of a hundred lists of about ten cells leaves lists short of 15: the padding is transformed as it comes"
        assert c.knn_index_project(np.zeros((5, 0)), A_GEN, B_GEN)["layout"].shape[0] == 0
        with pytest.raises(sa.SingletHipError, match=r"n_epochs must lie in \[1, 2\^20\]"):
            c.knn_index_project(Q.T, A_GEN, B_GEN, 15, n_probe, 0)
        with pytest.raises(sa.SingletHipError, match="Yref holds a non-finite value"):
            c.knn_index_set_layout(np.full((2, N_REF), np.nan))
        assert c.knn_index_info()["bytes"] == bytes0 + 8 * 2 * N_REF, "a refused layout leaves the one before"
        c.knn_index_build(R.T, None, "euclidean", method, 100 if method == "ivf" else None)
        assert c.knn_index_info()["bytes"] == bytes0, "a rebuild drops the layout"
        with pytest.raises(sa.SingletHipError, match="holds no layout"):
            c.knn_index_project(Q.T, A_GEN, B_GEN)
        c.knn_index_drop()
        assert c.knn_index_info()["present"] == 0


# ---------------------------------------------------------------------------------------------- refusals and end to end
def test_refusals_leave_the_library_usable(sa):
    idx, W, Yref, Y0, want = epoch_case(2, 15, 5)
    bad = np.array(idx)
    bad[10, 3] = bad[10, 2]
    with pytest.raises(sa.SingletHipError, match="query 10 at slot 3: index repeated"):
        sa.op_umap_transform_epochs(bad, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS)
    with pytest.raises(sa.SingletHipError, match="1 <= t_first <= t_last <= n_epochs"):
        sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 5, 4)
    Yb = np.array(Y0)
    Yb[1, 1] = np.inf
    with pytest.raises(sa.SingletHipError, match="query 1, component 1"):
        sa.op_umap_transform_epochs(idx, W, Yref, Yb, 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS)
    got = sa.op_umap_transform_epochs(idx, W, Yref, Y0, 1.0, 1.0, N_EPOCHS, 1, N_EPOCHS, 0.25, 5, SEED)
    assert np.array_equal(bits(got), bits(want))


def test_map_query_with_layout_equals_the_separate_steps(sa, ora):
    """The 40 x 300 synthetic fit: map_query(layout=True) equals project_model, index.map and index.project; it reads the
    context only; without `layout` the dict is today's."""
    A = ora.synth_csc(40, 300, 5)
    rng = np.random.default_rng(2)
    w = rng.random((40, 6))
    dA = sa.dgCMatrix(A.x, A.i, A.p, (A.nrow, A.ncol))
    ref, qry = dA.col_slice(0, 220), dA.col_slice(220, 300)
    E = np.asarray(sa.project_model(ref, w)["h"]).T          # cells x factors
    Yref = rng.normal(size=(220, 2)) * 3.0
    labels = (np.arange(220) % 3).astype(np.int32)
    with sa.ReferenceIndex(E, labels=labels, method="exact", layout=Yref) as index:
        plain = sa.map_query(qry, w, index, n_neighbors=10)
        assert sorted(plain) == sorted(["h", "d", "idx", "dist", "predicted", "score", "scores", "values"])
        searches = index.info()["searches"]
        full = sa.map_query(qry, w, index, n_neighbors=10, layout=True, a=A_GEN, b=B_GEN, n_epochs=20, seed=8)
        assert sorted(full) == sorted(list(plain) + ["layout", "layout_init"])
        assert index.info()["searches"] == searches + 2
        for key in plain:
            if plain[key] is None:
                assert full[key] is None
            else:
                assert np.ascontiguousarray(plain[key]).tobytes() == np.ascontiguousarray(full[key]).tobytes(), key
        Y0, Y = sa.umap_transform(plain["idx"], plain["dist"], Yref, A_GEN, B_GEN, 20, seed=8, return_init=True)
        assert np.array_equal(bits(full["layout"]), bits(Y)) and np.array_equal(bits(full["layout_init"]), bits(Y0))
        pr = index.project(np.asarray(plain["h"]).T, A_GEN, B_GEN, 10, None, 20, seed=8)
        assert np.array_equal(bits(pr["layout"]), bits(Y))
        with pytest.raises(ValueError, match="needs the curve"):
            sa.map_query(qry, w, index, n_neighbors=10, layout=True)
    # the ProjectUMAP mirror on the same pieces: a model, the reference embedding, the query embedding
    model = sa.UmapModel(A_GEN, B_GEN, 10, "euclidean", None, Yref, 1.0, 5, 8)
    got = sa.project_umap(model, E, np.asarray(plain["h"]).T, n_epochs=20)
    assert np.array_equal(bits(got), bits(Y))


# ----------------------------------------------------------------------------------------------------------------- quality
@pytest.mark.parametrize("name", ["blobs", "weak"])
def test_quality_against_the_sequential_transform(sa, name):
    """The criterion of tests/test_umap_transform_restatement.py on the device: the rest laid out by umap_layout here (existing
    code), the held-out queries placed by umap_transform; for each of the seeds 0 .. 2 the score is at least the sequential
    transform's worst recorded seed minus its seed-to-seed range, and on the blobs every query's 10 nearest references in the
    layout carry its label."""
    g = os.path.join(ROOT, "tests", "golden")
    points = np.load(os.path.join(g, "umap_fixtures.npz"))
    c = tr.quality_case(points, np.load(os.path.join(g, "umap_transform_fixtures.npz")), name)
    K, layout_epochs, neg, _ = (int(v) for v in points["settings"])
    idx_r, dist_r = ur.knn_lists(c["R"], K)
    Yref = sa.umap_layout(sa.fuzzy_simplicial_set(idx_r, dist_r), ur.pca_start(c["R"], 2), c["a"], c["b"], layout_epochs, 1.0, neg, 42)
    floor = tr.quality_floor(c["S_seq"])
    for seed in range(3):
        Y = sa.umap_transform(c["idx"], c["dist"], Yref, c["a"], c["b"], c["n_epochs"], c["alpha0"], c["neg"], seed)
        S = tr.neighbour_share(c["R"], c["Q"], Yref, Y, c["share_k"])
        print("%s seed %d: share %.4f (start %.4f, sequential %.4f .. %.4f, floor %.4f)"
              % (name, seed, S, c["S_start"], c["S_seq"].min(), c["S_seq"].max(), floor))
        assert S >= floor, (name, seed, S, floor)
        if name == "blobs":
            assert tr.nearest_labels_agree(Yref, Y, c["labels_ref"], c["labels_query"], 10)
