"""The layout stage (sgl_c_fuzzy_graph, sgl_c_umap_layout) without a device: the numpy restatement against hand-worked
cases and against a scalar evaluation of the rules, the hash against the oracle's, find_ab_params against scipy, the quality
criterion on the fixture (tests/golden/umap_fixtures.npz, whose sequential-optimiser figures were recorded by
tests/golden/make_umap_fixtures.py), the declarations of the four entries, the host logic of run_umap with the device calls
replaced by the restatement, and the library's own host logic (singlet_amd/csrc/umap_host.h) run as a stand-alone program
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import umap_restatement as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ the hash
def test_the_hash_is_the_oracles(ora):
    rng = np.random.default_rng(0)
    for _ in range(200):
        s, i, j = (int(v) for v in rng.integers(0, 2 ** 63, 3))
        assert int(ur.rand2(s, [i], [j])[0]) == ora.rng_rand(s, i, j)
    assert int(ur.rand2(2 ** 64 - 1, [2 ** 64 - 1], [2 ** 64 - 1])[0]) == ora.rng_rand(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)
    from singlet_amd import api
    i, j = rng.integers(0, 2 ** 40, 50).astype(np.uint64), rng.integers(0, 2 ** 20, 50).astype(np.uint64)
    assert np.array_equal(api._rand2(42, i, j), ur.rand2(42, i, j))


# ------------------------------------------------------------------------------------------------------------ fuzzy graph
def test_fuzzy_graph_of_three_cells_by_hand():
    """Cells 0 and 1 list each other, cell 2 lists 0 and 1 and nobody lists it.  K = 3, so log2(K) = 1.585 and every own
    list has two entries: the nearest has membership 1, the other exp(-(d - rho) / sigma) with
    1 + exp(-(d - rho) / sigma) = log2(3) at the root of the bisection."""
    idx = np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1]])
    dist = np.array([[0.0, 1.0, 3.0], [0.0, 1.0, 4.0], [0.0, 3.0, 4.0]])
    p, i, x, rho, sigma = ur.fuzzy_graph(idx, dist)
    assert rho.tolist() == [1.0, 1.0, 3.0]
    far = math.log2(3) - 1.0                                   # the membership of the farther entry
    for j, gap in enumerate((2.0, 3.0, 1.0)):
        assert sigma[j] == pytest.approx(-gap / math.log(far), rel=1e-13)
    assert p.tolist() == [0, 2, 4, 6] and i.tolist() == [1, 2, 0, 2, 0, 1]
    w01 = (1.0 + 1.0) - 1.0 * 1.0
    w02, w12 = x[1], x[3]
    assert x[0] == w01 == x[2]
    assert w02 == pytest.approx((far + 1.0) - far * 1.0, rel=1e-13) and w12 == pytest.approx((far + far) - far * far, rel=1e-13)
    assert bits(x[4]) == bits(w02) and bits(x[5]) == bits(w12)


@pytest.mark.parametrize("n,K", [(2, 2), (65, 31), (400, 15)])
def test_symmetrised_graph_equals_its_transpose(n, K):
    X = np.random.default_rng(n).standard_normal((n, 3))
    X[n // 2:n // 2 + 3] = X[n // 2]                           # zero distances
    p, i, x, rho, sigma = ur.fuzzy_graph(*ur.knn_lists(X, K))
    D = np.zeros((n, n))
    col = np.repeat(np.arange(n), np.diff(p))
    D[i, col] = x
    assert np.array_equal(D, D.T) and not np.diag(D).any() and (x > 0).all() and (x <= 1).all()
    assert (np.diff(p) >= K - 1).all() and (sigma > 0).all()
    for c in range(n):
        assert (np.diff(i[p[c]:p[c + 1]]) > 0).all()


def test_sigma_is_the_root_of_psum():
    idx, dist = ur.knn_lists(np.random.default_rng(1).standard_normal((200, 4)), 20)
    rho, sigma, P, own = ur.smooth_knn(idx, dist)
    assert np.allclose(P.sum(axis=1), math.log2(20), rtol=1e-12)
    assert (P[~own] == 0).all() and (P[own] > 0).all() and (P.max(axis=1) == 1.0).all()


def test_fuzzy_graph_refusals():
    idx, dist = ur.knn_lists(np.random.default_rng(3).standard_normal((6, 2)), 3)
    for bad_idx, bad_dist, what in ((idx[:, :1], dist[:, :1], "K"), (np.where(np.arange(18).reshape(6, 3) == 5, 6, idx), dist, "index range"),
                                    (np.where(np.arange(18).reshape(6, 3) == 4, idx[1, 0], idx), dist, "index repeated"),
                                    (idx, np.where(np.arange(18).reshape(6, 3) == 5, np.nan, dist), "not finite"),
                                    (idx, np.where(np.arange(18).reshape(6, 3) == 0, -1.0, dist), "negative"),
                                    (idx, dist[:, ::-1], "order")):
        with pytest.raises(ValueError, match=what):
            ur.fuzzy_graph(bad_idx, bad_dist)


def test_blocked_sum_is_sequential_up_to_a_block():
    v = np.random.default_rng(2).random(3000)
    s = 0.0
    for t in v[:1024]:
        s = s + t
    assert ur.blocked_sum(v[:1024]) == s
    parts = []
    for lo in range(0, 3000, 1024):
        q = 0.0
        for t in v[lo:lo + 1024]:
            q = q + t
        parts.append(q)
    assert ur.blocked_sum(v) == (0.0 + parts[0] + parts[1]) + parts[2]


# ------------------------------------------------------------------------------------------------------------------ layout
# 4 cells; column 0 stores rows 1, 2, 3 with 1, 1/2 and 1/4 of the maximum weight; column 1 stores row 0 with 3/4 of it and a
# diagonal entry at the maximum; columns 2 and 3 store row 0.
P4 = np.array([0, 3, 5, 6, 7])
I4 = np.array([1, 2, 3, 0, 1, 0, 0])
X4 = np.array([4.0, 2.0, 1.0, 3.0, 4.0, 2.0, 1.0])
FIRES4 = {1: [1, 0, 0, 0, 0, 0, 0], 2: [1, 1, 0, 1, 0, 1, 0], 3: [1, 0, 0, 1, 0, 0, 0], 4: [1, 1, 1, 1, 0, 1, 1], 5: [1, 0, 0, 0, 0, 0, 0]}


def scalar_epoch(p, i, x, Y, a, b, n_epochs, alpha0, neg_rate, seed, t, events):
    """The rules one entry and one component at a time, in plain Python floats."""
    n, dim = len(Y), len(Y[0])
    w_max = max(x)
    out = [list(row) for row in Y]

    def term(j, o, attractive):
        d = [Y[j][f] - Y[o][f] for f in range(dim)]
        d2 = 0.0
        for f in range(dim):
            d2 = d2 + d[f] * d[f]
        pw = d2 if b == 1.0 else math.pow(d2, b)
        if attractive:
            if not d2 > 0.0:
                events.add("attractive at d2 = 0")
                return [0.0] * dim
            c = ((-2.0 * a * b) * (pw / d2)) / (a * pw + 1.0)
        else:
            if o == j:
                events.add("sample hits its head")
                return [0.0] * dim
            if d2 == 0.0:
                events.add("repulsive at d2 = 0")
                return [4.0] * dim
            c = (2.0 * b) / ((0.001 + d2) * (a * pw + 1.0))
        return [min(max(c * d[f], -4.0), 4.0) for f in range(dim)]

    for j in range(n):
        delta, fired = [0.0] * dim, False
        for e in range(p[j], p[j + 1]):
            r = x[e] / w_max
            if i[e] == j or not math.floor(t * r) > math.floor((t - 1) * r):
                continue
            fired = True
            g = term(j, i[e], True)
            for s in range(neg_rate):
                u = int(ur.rand2(seed, [e], [256 * t + s])[0])
                m = ((u >> 32) * n) >> 32
                v = term(j, m, False)
                g = [g[f] + v[f] for f in range(dim)]
            delta = [delta[f] + g[f] for f in range(dim)]
        if fired:
            alpha = alpha0 * (1.0 - (t - 1) / n_epochs)
            out[j] = [Y[j][f] + alpha * delta[f] for f in range(dim)]
    return out


def test_firing_pattern_of_the_four_cell_graph_over_five_epochs():
    for t in range(1, 6):
        assert ur.firing(X4, 4.0, t).astype(int).tolist()[:4] + [0] + ur.firing(X4, 4.0, t).astype(int).tolist()[5:] == FIRES4[t], t
    assert ur.firing(X4, 4.0, 3)[4]                              # the diagonal entry would fire by its weight: it is skipped


def test_one_attractive_step_by_hand():
    """dim 1, a = b = 1, no negative samples: c = -2 / (1 + d2).  Epoch 2 of 5 (alpha = 0.8): vertex 0 at y = 0 is pulled by
    row 1 at y = 1 (d = -1, c = -1, term 1) and by row 2 at y = 3 (d = -3, c = -0.2, term 0.6); row 3 does not fire."""
    Y = np.array([[0.0], [1.0], [3.0], [-2.0]])
    out = ur.epoch(P4, I4, X4, Y, 1.0, 1.0, 5, 1.0, 0, 7, 2)
    c2 = (-2.0 * (9.0 / 9.0)) / (9.0 + 1.0)
    assert out[0, 0] == 0.0 + 0.8 * ((0.0 + 1.0) + c2 * -3.0)
    assert out[1, 0] == 1.0 + 0.8 * ((-2.0 / 2.0) * 1.0)        # its entry of weight 3/4 fires, its diagonal entry never
    assert out[2, 0] == 3.0 + 0.8 * (((-2.0 * (9.0 / 9.0)) / 10.0) * 3.0)
    assert bits(out[3]) == bits(Y[3])                            # nothing of column 3 fires in epoch 2
    far = ur.epoch(P4, I4, X4, np.array([[0.0], [100.0], [3.0], [-2.0]]), 1.0, 1.0, 5, 1.0, 0, 7, 1)
    assert far[0, 0] == 0.0 + 1.0 * ((-2.0 / 10001.0) * -100.0) and far[0, 0] < 4.0
    near = ur._terms(np.array([[0.0, 0.0]]), np.array([[0.1, -0.1]]), 1.0, 1.0, False)
    assert near.tolist() == [[-4.0, 4.0]]                        # c = 2 / ((0.001 + 0.02) * 1.02) = 93: c * d is clipped


def test_terms_at_d2_zero_and_a_sample_that_hits_its_head():
    y = np.array([[1.5, -2.0]])
    assert bits(ur._terms(y, y, 1.577, 0.8951, True)).tolist() == bits(np.zeros((1, 2))).tolist()
    assert ur._terms(y, y, 1.577, 0.8951, False, np.array([False])).tolist() == [[4.0, 4.0]]
    assert bits(ur._terms(y, y, 1.577, 0.8951, False, np.array([True]))).tolist() == bits(np.zeros((1, 2))).tolist()


@pytest.mark.parametrize("a,b", [(1.0, 1.0), (1.577, 0.8951)])
def test_epochs_equal_the_scalar_evaluation_of_the_rules(a, b):
    events = set()
    Y = np.array([[0.0, 0.5], [1.0, -1.0], [1.5, -1.0], [0.0, 0.5]])   # cells 0 and 3 coincide: seed 4 samples 3 for entry 0 in epoch 1
    for t in range(1, 6):
        want = scalar_epoch(P4.tolist(), I4.tolist(), X4.tolist(), Y.tolist(), a, b, 5, 1.0, 3, 4, t, events)
        got = ur.epoch(P4, I4, X4, Y, a, b, 5, 1.0, 3, 4, t)
        if b == 1.0:
            assert np.array_equal(bits(got), bits(np.array(want))), t
        else:
            assert np.allclose(got, np.array(want), rtol=1e-14, atol=0), t
        Y = got
    assert events >= {"sample hits its head", "repulsive at d2 = 0"}
    events.clear()
    scalar_epoch([0, 1, 2], [1, 0], [1.0, 1.0], [[1.0], [1.0]], a, b, 5, 1.0, 0, 1, 1, events)
    assert events == {"attractive at d2 = 0"}
    same = ur.epoch([0, 1, 2], [1, 0], [1.0, 1.0], np.array([[1.0], [1.0]]), a, b, 5, 1.0, 0, 1, 1)
    assert same.tolist() == [[1.0], [1.0]]


def test_layout_is_the_chain_of_its_epochs_and_an_empty_graph_returns_the_start():
    Y0 = np.array([[0.0, 0.5], [1.0, -1.0], [1.5, -1.0], [-2.0, 0.25]])
    Y = Y0
    for t in range(1, 6):
        Y = ur.epoch(P4, I4, X4, Y, 1.577, 0.8951, 5, 1.0, 2, 3, t)
    assert np.array_equal(bits(ur.layout(P4, I4, X4, Y0, 1.577, 0.8951, 5, 1.0, 2, 3)), bits(Y))
    assert np.array_equal(bits(ur.layout(P4, I4, np.zeros(7), Y0, 1.0, 1.0, 5)), bits(Y0))
    assert np.array_equal(bits(ur.layout([0, 0, 0, 0, 0], [], [], Y0, 1.0, 1.0, 5)), bits(Y0))


def test_trustworthiness_of_a_perfect_and_of_a_scrambled_layout():
    X = np.random.default_rng(4).standard_normal((120, 3))
    assert ur.trustworthiness(X, X[:, :3] * 2.0, 10) == 1.0
    assert ur.trustworthiness(X, np.random.default_rng(5).standard_normal((120, 2)), 10) < 0.7
    labels = np.arange(120) % 2
    assert ur.label_purity(np.stack([labels * 100.0 + X[:, 0], X[:, 1]], axis=1), labels, 10) == 1.0


# ----------------------------------------------------------------------------------------------------------- find_ab_params
def test_find_ab_params_reproduces_the_published_values():
    import singlet_amd as sa
    a, b = sa.find_ab_params(1.0, 0.1)
    assert round(a, 3) == 1.577 and round(b, 4) == 0.8951


@pytest.mark.parametrize("spread,min_dist", [(1.0, 0.3), (1.0, 0.1), (1.0, 0.001), (2.0, 0.5), (0.5, 0.0), (1.0, 0.99)])
def test_find_ab_params_against_scipy(spread, min_dist):
    from scipy.optimize import curve_fit
    import singlet_amd as sa
    x = np.linspace(0, spread * 3, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))
    want, _ = curve_fit(curve, x, y)
    got = sa.find_ab_params(spread, min_dist)
    ss = [float(np.sum((curve(x, *q) - y) ** 2)) for q in (got, want)]
    assert ss[0] <= ss[1] + 1e-12
    assert np.allclose(got, want, rtol=1e-3, atol=0)


# ------------------------------------------------------------------------------------------------------------------ quality
@pytest.fixture(scope="module")
def fixtures():
    return np.load(os.path.join(ROOT, "tests", "golden", "umap_fixtures.npz"))


@pytest.mark.parametrize("name", ["blobs", "weak"])
def test_quality_of_the_synchronous_scheme_against_the_sequential_optimiser(fixtures, name):
    """For each of the seeds 0 .. 4 the gain in trustworthiness over the start is at least 0.95 of the gain of the sequential
    optimiser's WORST seed (of ten); on the 6-blob set the 10-neighbour label purity is exactly 1."""
    z = fixtures
    K, epochs, neg, tk = (int(v) for v in z["settings"])
    a, b = z["ab"]
    X, Y0, labels = z[name + "_X"], z[name + "_Y0"], z[name + "_labels"]
    assert (X.shape[0], int(labels.max()) + 1, K, epochs, neg) == ({"blobs": 800, "weak": 1200}[name], {"blobs": 6, "weak": 20}[name], 15, 200, 5)
    idx, dist = ur.knn_lists(X, K)
    assert np.array_equal(idx, z[name + "_idx"]) and np.array_equal(bits(dist), bits(z[name + "_dist"]))
    assert np.allclose(ur.pca_start(X, 2), Y0, rtol=0, atol=1e-9)
    t_start, t_seq = float(z[name + "_T_start"]), z[name + "_T_seq"]
    assert t_seq.shape == (10,) and ur.trustworthiness(X, Y0, tk) == pytest.approx(t_start, abs=1e-12)
    p, i, x, _, _ = ur.fuzzy_graph(idx, dist)
    for seed in range(5):
        Y = ur.layout(p, i, x, Y0, a, b, epochs, 1.0, neg, seed)
        T = ur.trustworthiness(X, Y, tk)
        print("%s seed %d: T %.5f, share of the sequential optimiser's worst gain %.4f" % (name, seed, T, (T - t_start) / (t_seq.min() - t_start)))
        assert T - t_start >= 0.95 * (float(t_seq.min()) - t_start), (name, seed, T)
        if name == "blobs":
            assert ur.label_purity(Y, labels, 10) == 1.0


# ------------------------------------------------------------------------------------------ declarations and the build rule
def test_header_declares_the_entries_and_keeps_the_version():
    h = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("SGL_API int sgl_c_fuzzy_graph(const int32_t* idx, const double* dist, int64_t n, int32_t K, int32_t* p_out, "
            "int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap, double* rho_out, double* sigma_out);") in flat
    assert ("SGL_API int sgl_c_umap_layout(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* Y0, "
            "int32_t dim, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, double* Y);") in flat
    assert ("SGL_API int sgl_op_umap_epoch(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* Yin, "
            "int32_t dim, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, int32_t t, "
            "double* Y);") in flat
    assert "SGL_API int sgl_umap_info(int64_t out[4]);" in flat
    assert ("SGL_API int sgl_abi_version(void);   /* 2: native multi-GPU section, sgl_nmf_iterate, chunk-list / dense ARD entry "
            "points */") in h


def test_the_unit_is_compiled_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_umap.o" in objs
    assert re.search(r"^kernels_umap\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^kernels_umap\.o: umap_host\.h$", mk, flags=re.M)


def test_the_binding_declares_the_entries():
    from singlet_amd import _lib
    i32p, i64p, f64p = _lib.i32p, _lib.i64p, _lib.f64p
    tail = [C.c_int32, f64p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_uint64]
    assert _lib.SIGNATURES["sgl_c_fuzzy_graph"] == (C.c_int, [i32p, f64p, C.c_int64, C.c_int32, i32p, i64p, i32p, f64p, C.c_int64, f64p, f64p])
    assert _lib.SIGNATURES["sgl_c_umap_layout"] == (C.c_int, [f64p, i32p, i32p] + tail + [f64p])
    assert _lib.SIGNATURES["sgl_op_umap_epoch"] == (C.c_int, [f64p, i32p, i32p] + tail + [C.c_int32, f64p])
    assert _lib.SIGNATURES["sgl_umap_info"] == (C.c_int, [i64p])


def test_the_widths_in_the_header_text_are_the_builds():
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "umap_host.h")).read()
    width = int(re.search(r"^#define UMAP_MERGE_WIDTH (\d+)", host, flags=re.M).group(1))
    block = int(re.search(r"^#define UMAP_SUM_BLOCK (\d+)", host, flags=re.M).group(1))
    chunk = int(re.search(r"^#define UMAP_CHUNK (\d+)", host, flags=re.M).group(1))
    h = re.sub(r"\s+", " ", re.sub(r"\n \* ", "\n", open(os.path.join(ROOT, "include", "singlet_hip.h")).read()))
    assert "up to %d keys per vertex (the LDS merge)" % width in h and width & (width - 1) == 0 and width >= 64
    assert block == ur.BLOCK and "blocks of %d consecutive terms" % block in h
    assert chunk == 64 and "in steps of %d stored entries" % chunk in h


# ------------------------------------------------------------------------------------------------- run_umap on the host
@pytest.fixture
def host_umap(monkeypatch):
    """run_umap with the three device calls replaced by the restatement; seen = what they received."""
    import singlet_amd as sa
    from singlet_amd import api
    seen = {}

    def knn(reference, query=None, n_neighbors=20, dims=None):
        R = np.asarray(reference)
        seen.update(knn=(R.shape, n_neighbors, dims))
        return ur.knn_lists(R.T if dims is None else R[dims].T, n_neighbors)

    def fuzzy(idx, dist, return_sigmas=False):
        p, i, x, _, _ = ur.fuzzy_graph(idx, dist)
        return sa.dgCMatrix(x, i, p, (idx.shape[0], idx.shape[0]))

    def layout(G, Y0, a, b, n_epochs, alpha0=1.0, neg_rate=5, seed=42):
        seen.update(layout=(np.array(Y0), a, b, n_epochs, alpha0, neg_rate, seed))
        return ur.layout(G.p, G.i, G.x, Y0, a, b, min(n_epochs, 3), alpha0, neg_rate, seed)

    monkeypatch.setattr(api, "knn", knn)
    monkeypatch.setattr(api, "fuzzy_simplicial_set", fuzzy)
    monkeypatch.setattr(api, "umap_layout", layout)
    return sa, seen


def test_run_umap_host_logic(host_umap):
    sa, seen = host_umap
    E = np.random.default_rng(6).random((5, 90)) * np.array([[5.0], [3.0], [1.0], [1.0], [1.0]])
    Y, G = sa.run_umap(E, n_neighbors=12, return_graph=True)
    assert Y.shape == (90, 2) and G.Dim == (90, 90)
    Y0, a, b, n_epochs, alpha0, neg, seed = seen["layout"]
    assert seen["knn"] == ((5, 90), 12, None) and (n_epochs, alpha0, neg, seed) == (500, 1.0, 5, 42)
    assert (a, b) == sa.find_ab_params(1.0, 0.3)
    assert np.allclose(Y0, ur.pca_start(E.T, 2), rtol=0, atol=1e-9) and np.max(np.abs(Y0)) == pytest.approx(10.0, rel=1e-15)
    sa.run_umap(np.zeros((3, 10001)) + np.arange(10001), n_neighbors=2, n_components=1, init="random", seed=9, n_epochs=None)
    Y0 = seen["layout"][0]
    assert seen["layout"][3] == 200 and Y0.shape == (10001, 1) and (Y0 >= -10).all() and (Y0 < 10).all()
    u = ur.rand2(9, np.arange(10001, dtype=np.uint64), np.zeros(10001, dtype=np.uint64))
    assert np.array_equal(Y0[:, 0], (u >> np.uint64(11)).astype(np.float64) * (20.0 / 2.0 ** 53) - 10.0)
    given = np.random.default_rng(1).random((90, 3))
    sa.run_umap(E, n_neighbors=5, n_components=3, init=given, dims=[0, 2], learning_rate=0.5, negative_sample_rate=2, n_epochs=7, seed=3)
    assert np.array_equal(seen["layout"][0], given) and seen["layout"][3:] == (7, 0.5, 2, 3) and seen["knn"][2].tolist() == [0, 2]


def test_run_umap_refusals(host_umap):
    sa, _ = host_umap
    E = np.random.default_rng(6).random((3, 40))
    for kw, msg in ((dict(n_components=0), "n_components"), (dict(n_components=9), "n_components"), (dict(n_components=4), "at most 3 components"),
                    (dict(init="spectral"), "init must be"), (dict(init=np.zeros((40, 3))), "init array"), (dict(dims=[3]), "dims"),
                    (dict(dims=[]), "dims")):
        with pytest.raises(ValueError, match=msg):
            sa.run_umap(E, n_neighbors=5, **kw)
    with pytest.raises(ValueError, match="k x n"):
        sa.run_umap(np.zeros(7))
    with pytest.raises(ValueError):
        sa.find_ab_params(0.0, 0.1)


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_host_logic_under_address_and_undefined_sanitizers(tmp_path):
    """The refusals, the firing rule, the learning rate, the instance choice, the chunk plan, the merge split and the epoch
    loop hold no HIP call: they are compiled with a host compiler into a program of their own (tests/umap_host_main.cpp) with
    both sanitizers and run here, on the CPU."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "umap_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "umap_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("umap_host: ok"), (r.stdout, r.stderr)
