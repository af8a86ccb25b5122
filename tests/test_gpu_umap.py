"""The layout stage on the GPU (sgl_c_fuzzy_graph, sgl_c_umap_layout, sgl_op_umap_epoch, sgl_umap_info, run_umap) against
the numpy restatement of its rules (tests/umap_restatement.py).  What is exact is held bit for bit: the pattern, the counts,
the symmetry and rho of the fuzzy graph, and the whole layout with b == 1, where no transcendental is left.  What goes
through the device's exp or pow is held to a bound worked out from the rules, stated at each test.  Every test names, through
sgl_umap_info, the kernel instance and the path it claims to have run."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import umap_restatement as ur

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
EPS = 2.0 ** -52
A_GEN, B_GEN = 1.577, 0.8951
MERGE_WIDTH = 512      # keys of a vertex (its K slots and its incoming entries) that the LDS merge takes

# The largest relative difference of sigma and of a weight between the device and the restatement, measured on the fixtures of
# this file on an MI355X: only the ulps of the device's exp separate the two.  The tests allow 16 times this value, and never
# more than 1e-9.
FUZZY_REL_MEASURED = 3.709e-15
FUZZY_REL_ALLOWED = min(16 * FUZZY_REL_MEASURED, 1e-9)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def dgc(sa, p, i, x):
    n = len(p) - 1
    return sa.dgCMatrix(np.asarray(x, dtype=np.float64), np.asarray(i, dtype=np.int32), np.asarray(p, dtype=np.int32), (n, n))


# ------------------------------------------------------------------------------------------------------------- fuzzy graph
def check_fuzzy(sa, idx, dist, what, fallback=None):
    want_p, want_i, want_x, want_rho, want_sigma = ur.fuzzy_graph(idx, dist)
    G, rho, sigma = sa.fuzzy_simplicial_set(idx, dist, return_sigmas=True)
    info = sa.umap_info()
    n = idx.shape[0]
    assert G.Dim == (n, n) and np.array_equal(G.p, want_p) and np.array_equal(G.i, want_i), (what, "pattern")
    assert not np.any(G.i == np.repeat(np.arange(n), np.diff(G.p))), (what, "diagonal")
    M = sp.csc_matrix((G.x, G.i, G.p), shape=(n, n))
    Mt = M.T.tocsc()
    Mt.sort_indices()
    assert np.array_equal(Mt.indptr, G.p) and np.array_equal(Mt.indices, G.i) and np.array_equal(bits(Mt.data), bits(G.x)), (what, "symmetry")
    assert np.array_equal(bits(rho), bits(want_rho)), (what, "rho")
    rel_s = float(np.max(np.abs(sigma - want_sigma) / want_sigma))
    rel_w = float(np.max(np.abs(G.x - want_x) / want_x)) if want_x.size else 0.0
    print("fuzzy %s: n = %d, K = %d, nnz = %d, rel sigma %.3e, rel w %.3e, fallback %d" % (what, n, idx.shape[1], G.nnz, rel_s, rel_w,
                                                                                         info["merge_fallback"]))
    assert rel_s <= FUZZY_REL_ALLOWED and rel_w <= FUZZY_REL_ALLOWED, (what, rel_s, rel_w)
    indeg = np.bincount(np.asarray(idx)[np.asarray(idx) != np.arange(n)[:, None]], minlength=n)
    assert info["merge_fallback"] == int((idx.shape[1] + indeg > MERGE_WIDTH).sum()), (what, info)
    if fallback is not None:
        assert info["merge_fallback"] == fallback, (what, info)
    return G


@pytest.mark.parametrize("n,K", [(2, 2), (65, 2), (65, 31), (1000, 2), (1000, 31), (1000, 256)])
def test_fuzzy_graph_sizes(sa, n, K):
    X = np.random.default_rng(n * 1000 + K).standard_normal((n, 4))
    idx, dist = ur.knn_lists(X, K)
    G = check_fuzzy(sa, idx, dist, "random", fallback=None if K == 256 else 0)   # K = 256: hundreds of lists pass the LDS merge
    assert K != 256 or sa.umap_info()["merge_fallback"] > 100
    if n == 1000 and K == 2:   # reciprocated and one-way edges are both there
        other = idx[:, 1]
        mutual = other[other] == np.arange(n)
        assert mutual.any() and (~mutual).any() and G.nnz == 2 * n - mutual.sum()


def test_fuzzy_graph_cells_outside_their_own_lists_and_the_global_mean_floor(sa):
    """K + 3 identical points: the later ones are not in their own lists (K identical columns precede them), and all their
    distances are zero, so rho = 0 and the floor of sigma is 1e-3 of the mean of ALL distances."""
    K = 7
    X = np.random.default_rng(5).standard_normal((300, 3))
    X[100:100 + K + 3] = X[100]
    idx, dist = ur.knn_lists(X, K)
    assert (idx != np.arange(300)[:, None]).all(axis=1).sum() == 3
    _, rho, sigma = sa.fuzzy_simplicial_set(idx, dist, return_sigmas=True)
    check_fuzzy(sa, idx, dist, "identical columns", fallback=0)
    gmean = ur.blocked_sum(dist) / (300 * K)
    assert (rho[100:100 + K + 3] == 0).all() and np.array_equal(bits(sigma[100:100 + K + 3]), bits(np.full(K + 3, 1e-3 * gmean)))


def test_fuzzy_graph_all_distances_zero(sa):
    idx, dist = ur.knn_lists(np.ones((65, 2)), 5)
    assert not dist.any()
    G = check_fuzzy(sa, idx, dist, "all zero", fallback=0)
    assert (G.x == 1.0).all()


def test_fuzzy_graph_hub_takes_the_fallback(sa):
    """A star of 700 points: every leaf's nearest point is the centre, whose merged list (K slots + 699 incoming entries)
    passes the 512 keys of the LDS merge."""
    rng = np.random.default_rng(11)
    leaves = rng.standard_normal((699, 200))
    X = np.concatenate([np.zeros((1, 200)), leaves / np.linalg.norm(leaves, axis=1, keepdims=True)])
    idx, dist = ur.knn_lists(X, 5)
    assert (idx[1:, 1] == 0).all()
    G = check_fuzzy(sa, idx, dist, "star", fallback=1)
    assert G.p[1] - G.p[0] == 699


def raw_fuzzy(idx, dist, n, K, with_slots=True):
    from singlet_amd import _lib
    L = _lib.load()
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    rows = max(idx.shape[0], 1)
    p, i, x = np.full(rows + 1, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32), np.full(64, -7.0)
    rho, sigma, nnz = np.full(rows, -7.0), np.full(rows, -7.0), C.c_int64(-7)
    rc = L.sgl_c_fuzzy_graph(_lib.ptr(idx, _lib.i32p), _lib.ptr(dist, _lib.f64p), n, K, _lib.ptr(p, _lib.i32p), C.byref(nnz),
                             _lib.ptr(i, _lib.i32p) if with_slots else None, _lib.ptr(x, _lib.f64p) if with_slots else None, 64,
                             _lib.ptr(rho, _lib.f64p), _lib.ptr(sigma, _lib.f64p))
    untouched = (p == -7).all() and (i == -7).all() and (x == -7).all() and (rho == -7).all() and (sigma == -7).all() and nnz.value == -7
    return rc, (L.sgl_last_error() or b"").decode(), untouched


def test_fuzzy_graph_refusals_leave_the_outputs_untouched(sa):
    idx, dist = ur.knn_lists(np.random.default_rng(3).standard_normal((6, 2)), 3)

    def changed(array, where, value):
        out = array.copy()
        out[where] = value
        return out
    cases = [
        (idx[:, :1], dist[:, :1], 6, 1, r"neighbours must lie in \[2, 256\]"),
        (np.zeros((6, 257)), np.zeros((6, 257)), 6, 257, r"neighbours must lie in \[2, 256\]"),
        (idx, dist, 0, 3, r"cells must lie in \[1, 2\^31\)"),
        (idx, dist, 2 ** 31, 3, r"cells must lie in \[1, 2\^31\)"),
        (np.zeros((1, 2)), np.zeros((1, 2)), 1, 2, "cell 0 at place 1: index repeated"),   # one cell cannot fill two places
        (changed(idx, (4, 2), 6), dist, 6, 3, r"cell 4 at place 2: index outside \[0, n\)"),
        (changed(idx, (4, 2), -1), dist, 6, 3, r"cell 4 at place 2: index outside \[0, n\)"),
        (changed(idx, (2, 1), idx[2, 0]), dist, 6, 3, "cell 2 at place 1: index repeated"),
        (idx, changed(dist, (5, 2), np.inf), 6, 3, "cell 5 at place 2: distance is not finite"),
        (idx, changed(dist, (5, 0), np.nan), 6, 3, "cell 5 at place 0: distance is not finite"),
        (idx, changed(dist, (0, 0), -1e-300), 6, 3, "cell 0 at place 0: distance is negative"),
        (idx, changed(dist, (3, 1), dist[3, 2] * 2), 6, 3, "cell 3 at place 2: distances not ascending"),
    ]
    import re
    for bad_idx, bad_dist, n, K, msg in cases:
        for with_slots in (False, True):
            rc, text, untouched = raw_fuzzy(bad_idx, bad_dist, n, K, with_slots)
            assert rc == EINVAL and re.search(msg, text) and untouched, (msg, rc, text, untouched)
    with pytest.raises(ValueError):
        ur.fuzzy_graph(np.zeros((1, 2), dtype=np.int64), np.zeros((1, 2)))
    rc, _, untouched = raw_fuzzy(idx, dist, 6, 3)      # and the library is usable afterwards
    assert rc == 0 and not untouched


# --------------------------------------------------------------------------------------------------------------- one epoch
LENGTHS = [0, 1, 63, 64, 65, 129, 600]


def epoch_graph(n=701, seed=0):
    """Columns of 0, 1, 63, 64, 65, 129 and 600 stored entries first (the step of 64 entries and its carry), then random
    short ones; column 8 all at the maximum weight (all fire in every epoch; a diagonal entry is among them), column 9 all
    below half of it (none fires in epoch 1), a stored diagonal entry in column 10.  n is no multiple of the wave size."""
    rng = np.random.default_rng(seed)
    lens = LENGTHS + [40] * 4 + rng.integers(0, 50, n - len(LENGTHS) - 4).tolist()
    p, i, x = [0], [], []
    for c, m in enumerate(lens):
        rows = np.sort(rng.choice(n, size=m, replace=False))
        if c == 10:
            rows = np.unique(np.append(rows, 10))
        w = rng.random(rows.size) * 0.999 + 0.001
        if c == 8:
            w[:] = 1.0
        if c == 9:
            w *= 0.4
        i += rows.tolist()
        x += w.tolist()
        p.append(len(i))
    p, i, x = np.array(p, dtype=np.int32), np.array(i, dtype=np.int32), np.array(x)
    x[p[6]] = 1.0                                                 # the exact maximum sits in the wide column too
    return p, i, x


@pytest.mark.parametrize("neg_rate", [0, 5])
@pytest.mark.parametrize("dim,instance", [(2, 0), (3, 2), (5, 4)])
def test_one_epoch_general_b_within_the_bound_of_pow(sa, dim, instance, neg_rate):
    """|y' - y'_restated| <= 32 eps alpha_t S_f + 2 eps |y| per component, S_f the sum of the absolute clipped terms of the
    vertex: the OpenCL bound of 16 ulp for pow dominates each term's few roundings, clip is continuous, and the branches are
    decided by exact quantities."""
    p, i, x = epoch_graph()
    n = len(p) - 1
    rng = np.random.default_rng(dim)
    Y = rng.standard_normal((n, dim)) * 3.0
    Y[::3] = Y[0]                                                 # coincident points: attractive and repulsive terms at d2 = 0
    G = dgc(sa, p, i, x)
    for t in (1, 7):
        want, S = ur.epoch(p, i, x, Y, A_GEN, B_GEN, 10, 1.0, neg_rate, 99, t, with_bound=True)
        got = sa.op_umap_epoch(G, Y, A_GEN, B_GEN, 10, t, 1.0, neg_rate, 99)
        info = sa.umap_info()
        assert (info["instance"], info["widest_column"], info["multi_chunk"]) == (instance, 600, 3), info
        bound = 32 * EPS * ur.alpha_of(1.0, t, 10) * S + 2 * EPS * np.abs(Y)
        err = np.abs(got - want)
        print("epoch dim %d neg %d t %d: max err %.3e, max err / bound %.3f" % (dim, neg_rate, t, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (dim, neg_rate, t, float((err - bound).max()))
        col = np.repeat(np.arange(n), np.diff(p))
        fires = ur.firing(x, x.max(), t) & (i != col)
        still = np.bincount(col[fires], minlength=n) == 0
        assert still[0] and still.sum() > 1 and (t != 1 or still[9]) and not still[8]
        assert np.array_equal(bits(got[still]), bits(Y[still])), "a vertex without a firing entry keeps its bits"
        assert (fires | (i == col))[p[8]:p[9]].all() and (i[p[8]:p[9]] == 8).any()       # all fire but its diagonal entry
        assert t == 1 or ((got != Y).any(axis=1) == (want != Y).any(axis=1)).all() and (~still).sum() > n // 2


# ------------------------------------------------------------------------------------------------- whole layout with b == 1
@pytest.fixture(scope="module")
def thousand():
    X = np.random.default_rng(8).standard_normal((1000, 5))
    idx, dist = ur.knn_lists(X, 10)
    p, i, x, _, _ = ur.fuzzy_graph(idx, dist)
    return p, i, x


@pytest.mark.parametrize("dim,instance", [(2, 1), (3, 3), (5, 5)])
def test_whole_layout_with_b_one_equals_the_restatement_bit_for_bit(sa, thousand, dim, instance):
    """With a = b = 1 no transcendental is left: 30 epochs at n = 1000 pin the firing rule, the hash, the orders of the sums
    and the buffer swap."""
    p, i, x = thousand
    Y0 = np.random.default_rng(dim).standard_normal((1000, dim)) * 5.0
    want = ur.layout(p, i, x, Y0, 1.0, 1.0, 30, 1.0, 5, 1234)
    G = dgc(sa, p, i, x)
    got = sa.umap_layout(G, Y0, 1.0, 1.0, 30, 1.0, 5, 1234)
    assert sa.umap_info()["instance"] == instance
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(sa.umap_layout(G, Y0, 1.0, 1.0, 30, 1.0, 5, 1234)), bits(got)), "twice"
    odd = sa.umap_layout(G, Y0, 1.0, 1.0, 3, 1.0, 5, 1234)       # an odd number of epochs ends in the other buffer
    assert np.array_equal(bits(odd), bits(ur.layout(p, i, x, Y0, 1.0, 1.0, 3, 1.0, 5, 1234)))
    assert not np.array_equal(sa.umap_layout(G, Y0, 1.0, 1.0, 30, 1.0, 5, 1235), got), "the seed matters"


def test_layout_refusals_and_the_empty_graph(sa, thousand):
    p, i, x = thousand
    G = dgc(sa, p, i, x)
    Y0 = np.random.default_rng(0).standard_normal((1000, 2))
    for kw, msg in ((dict(a=0.0), "a and b"), (dict(b=np.nan), "a and b"), (dict(n_epochs=0), "n_epochs"), (dict(n_epochs=2 ** 20 + 1), "n_epochs"),
                    (dict(alpha0=-1.0), "alpha0"), (dict(neg_rate=256), "neg_rate"), (dict(neg_rate=-1), "neg_rate")):
        args = dict(a=1.0, b=1.0, n_epochs=5, alpha0=1.0, neg_rate=5)
        args.update(kw)
        with pytest.raises(sa.SingletHipError, match=msg) as e:
            sa.umap_layout(G, Y0, args["a"], args["b"], args["n_epochs"], args["alpha0"], args["neg_rate"], 1)
        assert e.value.code == EINVAL
    with pytest.raises(sa.SingletHipError, match="dim must lie"):
        sa.umap_layout(G, np.zeros((1000, 9)), 1.0, 1.0, 5)
    with pytest.raises(sa.SingletHipError, match="not finite"):
        sa.umap_layout(G, np.where(np.arange(2000).reshape(1000, 2) == 77, np.inf, Y0), 1.0, 1.0, 5)
    with pytest.raises(sa.SingletHipError, match="epoch must lie"):
        sa.op_umap_epoch(G, Y0, 1.0, 1.0, 5, 6)
    bad = x.copy()
    bad[5] = -1.0
    with pytest.raises(sa.SingletHipError, match="weight is negative"):
        sa.umap_layout(dgc(sa, p, i, bad), Y0, 1.0, 1.0, 5)
    swapped = i.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(sa.SingletHipError, match="not strictly ascending"):
        sa.umap_layout(dgc(sa, p, swapped, x), Y0, 1.0, 1.0, 5)
    empty = dgc(sa, np.zeros(1001, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    assert np.array_equal(bits(sa.umap_layout(empty, Y0, 1.0, 1.0, 5)), bits(Y0))
    assert np.array_equal(bits(sa.umap_layout(dgc(sa, p, i, np.zeros_like(x)), Y0, 1.0, 1.0, 5)), bits(Y0))     # w_max == 0


# --------------------------------------------------------------------------------------------------------------- quality
@pytest.fixture(scope="module")
def fixtures():
    return np.load(os.path.join(GOLD, "umap_fixtures.npz"))


@pytest.mark.parametrize("name", ["blobs", "weak"])
def test_quality_on_the_device_against_the_sequential_optimiser(sa, fixtures, name):
    """For each of the seeds 0 .. 2 the gain in trustworthiness over the start is at least 0.95 of the gain of the sequential
    optimiser's worst seed; on the 6-blob set the 10-neighbour label purity is exactly 1."""
    z = fixtures
    K, epochs, neg, tk = (int(v) for v in z["settings"])
    a, b = z["ab"]
    X, Y0, labels = z[name + "_X"], z[name + "_Y0"], z[name + "_labels"]
    t_start, worst = float(z[name + "_T_start"]), float(z[name + "_T_seq"].min())
    G = sa.fuzzy_simplicial_set(z[name + "_idx"], z[name + "_dist"])
    assert G.p[-1] == ur.fuzzy_graph(z[name + "_idx"], z[name + "_dist"])[0][-1]
    for seed in range(3):
        Y = sa.umap_layout(G, Y0, a, b, epochs, 1.0, neg, seed)
        assert sa.umap_info()["instance"] == 0
        T = ur.trustworthiness(X, Y, tk)
        print("%s seed %d: T %.5f, start %.5f, sequential worst %.5f, share of its gain %.4f" % (name, seed, T, t_start, worst,
                                                                                               (T - t_start) / (worst - t_start)))
        assert T - t_start >= 0.95 * (worst - t_start), (name, seed, T)
        if name == "blobs":
            assert ur.label_purity(Y, labels, 10) == 1.0


def _fit(sa, ora, with_umap):
    from conftest import to_dgc
    A = ora.synth_csc(40, 300, 6)
    out = {}
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        c.fit_init(5)
        trace = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
        if with_umap:
            H = c.get_factors()[2]
            out["ctx"] = sa.run_umap(c, n_neighbors=10, n_epochs=20, return_graph=True)
            out["arr"] = sa.run_umap(np.ascontiguousarray(H.T), n_neighbors=10, n_epochs=20, return_graph=True)
            assert np.array_equal(c.get_factors()[2], H)
        trace += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
        out["fit"] = (c.get_factors(), trace)
    return out


def test_run_umap_on_a_context_equals_the_array_and_only_reads_the_fit(sa, ora):
    with_umap, plain = _fit(sa, ora, True), _fit(sa, ora, False)
    (Yc, Gc), (Ya, Ga) = with_umap["ctx"], with_umap["arr"]
    assert Yc.shape == (300, 2) and np.isfinite(Yc).all() and np.array_equal(bits(Yc), bits(Ya))
    assert np.array_equal(Gc.p, Ga.p) and np.array_equal(Gc.i, Ga.i) and np.array_equal(bits(Gc.x), bits(Ga.x))
    assert sa.umap_info()["instance"] == 0
    for got, want in zip(with_umap["fit"][0], plain["fit"][0]):
        assert np.array_equal(bits(got), bits(want)), "the fit continues bit-identically after run_umap in mid-fit"
    assert with_umap["fit"][1] == plain["fit"][1]
    rnd = sa.run_umap(np.random.default_rng(1).random((4, 120)), n_neighbors=8, n_components=3, n_epochs=10, init="random", seed=5)
    assert rnd.shape == (120, 3) and np.isfinite(rnd).all() and sa.umap_info()["instance"] == 2
