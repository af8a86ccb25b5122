"""The layout transform (sgl_c_fuzzy_query, sgl_c_umap_transform, sgl_op_umap_transform_epochs) without a device: the numpy
restatement against hand-worked lists, the 1.0-membership consequence, the independence of the queries (permutation, slices
with their query_offset), the chaining of epoch ranges, the declarations of the entries, the refusals (they happen on the
host before anything is launched, so they can be asked of the library here), and the library's own host logic
(singlet_amd/csrc/umap_transform_host.h) run as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import umap_restatement as ur
import umap_transform_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def random_lists(rng, n, K, n_ref, pad=True, zeros=True):
    """Ascending lists of distinct references; some queries end in padding, one is empty, some begin with zero distances."""
    idx = np.stack([rng.permutation(n_ref)[:K] for _ in range(n)]).astype(np.int32)
    dist = np.sort(rng.random((n, K)) * 3.0 + 0.01, axis=1)
    if zeros:
        for q in range(0, n, 5):
            dist[q, :rng.integers(1, K + 1)] = 0.0
    if pad:
        for q in range(1, n, 4):
            cut = int(rng.integers(0, K))
            idx[q, cut:], dist[q, cut:] = -1, INF
        idx[n // 2], dist[n // 2] = -1, INF
    return idx, dist


# ----------------------------------------------------------------------------------------------------- hand-worked lists
def test_memberships_by_hand():
    # K = 1: log2(1) = 0, psum = 1 > 0 at every step: hi = mid, mid halves 64 times from 1 -> 2^-64; sigma = max(2^-64, 1e-3 * 2)
    rho, sigma, W = tr.fuzzy_query([[3]], [[2.0]])
    assert rho[0] == 2.0 and sigma[0] == 1e-3 * 2.0 and W[0, 0] == 1.0
    # all-zero distances: rho = 0, every membership 1.0; psum = 3 > log2(3) always: mid = 2^-64, mean = 0
    rho, sigma, W = tr.fuzzy_query([[0, 1, 2]], [[0.0, 0.0, 0.0]])
    assert rho[0] == 0.0 and sigma[0] == 2.0 ** -64 and (W == 1.0).all()
    # one padded slot: the own list is (1.0, 3.0); rho = 1, the second membership exp(-2 / sigma); target log2(3)
    rho, sigma, W = tr.fuzzy_query([[5, 6, -1]], [[1.0, 3.0, INF]])
    assert rho[0] == 1.0 and W[0, 0] == 1.0 and W[0, 2] == 0.0 and bits(W[0, 2]) == 0
    s = -2.0 / math.log(math.log2(3) - 1.0)          # 1 + exp(-2 / s) = log2(3)
    assert sigma[0] == pytest.approx(s, rel=1e-12) and W[0, 1] == pytest.approx(math.log2(3) - 1.0, rel=1e-12)
    assert sigma[0] >= 1e-3 * 2.0
    # an empty list
    rho, sigma, W = tr.fuzzy_query([[-1, -1]], [[INF, INF]])
    assert bits(rho)[0] == 0 and bits(sigma)[0] == 0 and (bits(W) == 0).all()


def test_start_and_one_epoch_by_hand():
    Yref = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 4.0]])
    idx = np.array([[1, 2], [-1, -1]])
    W = np.array([[1.0, 0.5], [0.0, 0.0]])
    y0 = tr.start(idx, W, Yref)
    assert y0[0].tolist() == [(1.0 * 2.0 + 0.5 * 0.0) / 1.5, (0.0 + 0.5 * 4.0) / 1.5]
    assert (bits(y0[1]) == 0x7FF8000000000000).all()
    # epoch 1, no negatives, a = b = 1: only slot 0 fires (floor(1 * 1.0) > floor(0)); slot 1 (0.5) fires in epoch 2
    assert tr.firing(W[0], 1).tolist() == [True, False] and tr.firing(W[0], 2).tolist() == [True, True]
    y = tr.epochs(idx, W, Yref, y0, 1.0, 1.0, 10, alpha0=0.25, neg_rate=0, t_first=1, t_last=1)
    d = y0[0] - Yref[1]
    d2 = d[0] * d[0] + d[1] * d[1]
    c = (-2.0 * (d2 / d2)) / (1.0 * d2 + 1.0)
    g = np.fmin(np.fmax(c * d, -4.0), 4.0)
    assert np.array_equal(bits(y[0]), bits(y0[0] + 0.25 * (0.0 + g)))
    assert (bits(y[1]) == 0x7FF8000000000000).all()
    # a query on top of a reference: the attractive term at d2 == 0 is +0.0, a sample at d2 == 0 is +4.0 in every component
    one = np.array([[0]])
    yq = np.array([[0.0, 0.0]])
    out = tr.epochs(one, np.array([[1.0]]), Yref[:1], yq, 1.0, 1.0, 4, alpha0=1.0, neg_rate=2, t_first=1, t_last=1)
    assert out.tolist() == [[8.0, 8.0]]
    # no firing slot keeps the bits of y (-0.0 stays -0.0)
    out = tr.epochs(one, np.array([[0.25]]), Yref[:1], np.array([[-0.0, 1.0]]), 1.0, 1.0, 4, neg_rate=2, t_first=1, t_last=3)
    assert np.array_equal(bits(out), bits(np.array([[-0.0, 1.0]])))


@pytest.mark.parametrize("K", [1, 2, 15, 64])
def test_every_non_empty_list_holds_a_membership_of_exactly_one(K):
    rng = np.random.default_rng(K)
    idx, dist = random_lists(rng, 200, K, 500)
    tr.check_lists(idx, dist, 500)
    rho, sigma, W = tr.fuzzy_query(idx, dist)
    own = idx >= 0
    assert ((W == 1.0) & own).any(axis=1)[own.any(axis=1)].all()
    assert (W[own] >= 0).all() and (W[own] <= 1.0).all() and (bits(W[~own]) == 0).all()
    empty = ~own.any(axis=1)
    assert empty.any() and (bits(rho[empty]) == 0).all() and (bits(sigma[empty]) == 0).all()
    assert np.isfinite(sigma).all() and (sigma[~empty] > 0).all()


# ------------------------------------------------------------------------------------------------------------ independence
@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(11)
    n, K, n_ref = 90, 7, 300
    idx, dist = random_lists(rng, n, K, n_ref)
    Yref = rng.normal(size=(n_ref, 2)) * 5.0
    Y0, Y = tr.transform(idx, dist, Yref, 1.577, 0.895, 30, seed=3)
    return idx, dist, Yref, Y0, Y


def test_a_slice_with_its_offset_equals_the_rows_of_the_whole(case):
    idx, dist, Yref, Y0, Y = case
    for lo, hi in ((0, 90), (0, 1), (17, 60), (89, 90)):
        y0, y = tr.transform(idx[lo:hi], dist[lo:hi], Yref, 1.577, 0.895, 30, seed=3, query_offset=lo)
        assert np.array_equal(bits(y0), bits(Y0[lo:hi])) and np.array_equal(bits(y), bits(Y[lo:hi]))
    # without the offset the negative samples are others
    _, y = tr.transform(idx[17:60], dist[17:60], Yref, 1.577, 0.895, 30, seed=3)
    assert not np.array_equal(bits(y), bits(Y[17:60]))
    _, y = tr.transform(idx, dist, Yref, 1.577, 0.895, 30, seed=4)
    assert not np.array_equal(bits(y), bits(Y))


def test_permuting_the_queries_permutes_the_result(case):
    """A query's samples hang on its global index: one query at a time with its own offset, in any order."""
    idx, dist, Yref, Y0, Y = case
    for q in np.random.default_rng(0).permutation(90)[:25]:
        y0, y = tr.transform(idx[q:q + 1], dist[q:q + 1], Yref, 1.577, 0.895, 30, seed=3, query_offset=int(q))
        assert np.array_equal(bits(y0[0]), bits(Y0[q])) and np.array_equal(bits(y[0]), bits(Y[q]))
    # and with neg_rate = 0 nothing hangs on the index at all
    perm = np.random.default_rng(1).permutation(90)
    _, _, W = tr.fuzzy_query(idx, dist)
    a = tr.epochs(idx, W, Yref, Y0, 1.0, 1.0, 30, neg_rate=0)
    b = tr.epochs(idx[perm], W[perm], Yref, Y0[perm], 1.0, 1.0, 30, neg_rate=0)
    assert np.array_equal(bits(a[perm]), bits(b))


def test_chained_epoch_ranges_equal_the_whole(case):
    idx, dist, Yref, Y0, Y = case
    _, _, W = tr.fuzzy_query(idx, dist)
    kw = dict(a=1.577, b=0.895, n_epochs=30, seed=3)
    mid = tr.epochs(idx, W, Yref, Y0, t_first=1, t_last=7, **kw)
    end = tr.epochs(idx, W, Yref, mid, t_first=8, t_last=30, **kw)
    assert np.array_equal(bits(end), bits(Y)) and not np.array_equal(bits(mid), bits(Y))
    assert tr.launches(1, 30) == [(1, 30)] and tr.launches(1, 129) == [(1, 128), (129, 129)] and tr.launches(8, 8) == [(8, 8)]


def test_list_refusals_of_the_restatement():
    idx, dist = np.array([[4, 1, 7], [2, 9, -1]]), np.array([[0.0, 1.0, 1.0], [0.5, 0.75, INF]])
    tr.check_lists(idx, dist, 10)
    for (q, s, vi, vd), msg in ((((0, 2, 10, None), "index range")), ((0, 2, -2, None), "index range"), ((0, 2, 4, None), "repeated"),
                               ((0, 1, None, INF), "not finite"), ((1, 0, None, -0.5), "negative"), ((1, 1, None, 0.25), "order")):
        i, d = idx.copy(), dist.copy()
        if vi is not None:
            i[q, s] = vi
        if vd is not None:
            d[q, s] = vd
        with pytest.raises(ValueError, match=msg):
            tr.check_lists(i, d, 10)
    with pytest.raises(ValueError, match="behind padding"):
        tr.check_lists(np.array([[2, -1, 3]]), np.array([[0.5, INF, 1.0]]), 10)


# ----------------------------------------------------------------------------------------------------------------- quality
@pytest.fixture(scope="module")
def recorded():
    g = os.path.join(ROOT, "tests", "golden")
    return np.load(os.path.join(g, "umap_fixtures.npz")), np.load(os.path.join(g, "umap_transform_fixtures.npz"))


@pytest.mark.parametrize("name", ["blobs", "weak"])
def test_quality_of_the_rules_against_the_sequential_transform(recorded, name):
    """Every fourth point held out as a query, the rest laid out by the device's umap_layout (recorded).  The score -- the mean
    share of a query's 15 nearest references in the embedding that are among its 15 nearest in the layout -- of the rules, for
    each of the seeds 0 .. 2, is at least the sequential transform's worst seed (of ten) minus its own seed-to-seed range; on
    the 6-blob set every query's 10 nearest references in the layout carry its label."""
    c = tr.quality_case(*recorded, name)
    assert (c["K"], c["n_epochs"], c["neg"], c["share_k"], c["alpha0"]) == (15, 100, 5, 15, 0.25) and c["S_seq"].shape == (10,)
    assert c["Q"].shape[0] == {"blobs": 200, "weak": 300}[name] and c["Yref"].shape == (c["R"].shape[0], 2)
    D = ((c["Q"][:, None, :] - c["R"][None, :, :]) ** 2).sum(axis=2)
    assert (np.sort(D, axis=1)[:, 14] >= np.take_along_axis(D, c["idx"].astype(np.int64), axis=1).max(axis=1) - 1e-9).all(), "the lists are the nearest"
    tr.check_lists(c["idx"], c["dist"], c["R"].shape[0])
    _, _, W = tr.fuzzy_query(c["idx"], c["dist"])
    assert tr.neighbour_share(c["R"], c["Q"], c["Yref"], tr.start(c["idx"], W, c["Yref"]), 15) == pytest.approx(c["S_start"], abs=1e-12)
    floor = tr.quality_floor(c["S_seq"])
    assert floor > c["S_start"], "the yardstick improves on the start by more than its own noise"
    for seed in range(3):
        _, Y = tr.transform(c["idx"], c["dist"], c["Yref"], c["a"], c["b"], c["n_epochs"], c["alpha0"], c["neg"], seed)
        S = tr.neighbour_share(c["R"], c["Q"], c["Yref"], Y, 15)
        print("%s seed %d: share %.4f (start %.4f, sequential %.4f .. %.4f, floor %.4f)"
              % (name, seed, S, c["S_start"], c["S_seq"].min(), c["S_seq"].max(), floor))
        assert S >= floor, (name, seed, S, floor)
        if name == "blobs":
            assert tr.nearest_labels_agree(c["Yref"], Y, c["labels_ref"], c["labels_query"], 10)


# ------------------------------------------------------------------------------------------ declarations and the build rule
def test_header_declares_the_entries():
    h = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    for proto in (
            "SGL_API int sgl_c_fuzzy_query(const int32_t* idx, const double* dist, int64_t n_query, int32_t K, int64_t n_ref, double* W_out, "
            "double* rho_out, double* sigma_out);",
            "SGL_API int sgl_c_umap_transform(const int32_t* idx, const double* dist, int64_t n_query, int32_t K, const double* Yref, int32_t dim, "
            "int64_t n_ref, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, int64_t query_offset, "
            "double* Y0_out, double* Y_out);",
            "SGL_API int sgl_op_umap_transform_epochs(const int32_t* idx, const double* W, int64_t n_query, int32_t K, const double* Yref, "
            "int32_t dim, int64_t n_ref, const double* Yin, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, "
            "uint64_t seed, int64_t query_offset, int32_t t_first, int32_t t_last, double* Y_out);",
            "SGL_API int sgl_knn_index_set_layout(sgl_ctx* ctx, const double* Yref, int32_t dim);",
            "SGL_API int sgl_knn_index_project(sgl_ctx* ctx, const double* Q, int64_t n_query, int32_t n_neighbors, int32_t n_probe, "
            "int64_t query_batch, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, int32_t* idx_out, "
            "double* dist_out, double* Y0_out, double* Y_out);",
            "SGL_API int sgl_umap_transform_info(int64_t out[4]);",
            "SGL_API int sgl_umap_info(int64_t out[4]);"):
        assert proto in flat, proto
    assert h.index("Layout transform: query cells placed") > h.index("SGL_API int sgl_umap_info(int64_t out[4]);")
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "umap_transform_host.h")).read()
    per = int(re.search(r"^#define UMAP_TRANSFORM_EPOCHS_PER_LAUNCH (\d+)", host, flags=re.M).group(1))
    assert per == tr.EPOCHS_PER_LAUNCH and "launches of at most %d epochs" % per in re.sub(r"\s+", " ", re.sub(r"\n \* ", "\n", h))


def test_the_unit_is_compiled_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_umap_transform.o" in objs
    assert re.search(r"^kernels_umap_transform\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^kernels_umap_transform\.o: .*umap_transform_host\.h", mk, flags=re.M)
    src = open(os.path.join(ROOT, "singlet_amd", "csrc", "kernels_umap_transform.hip")).read()
    assert "atomicAdd((double" not in src and "unsafeAtomicAdd" not in src


def test_the_binding_declares_the_entries():
    from singlet_amd import _lib
    i32p, i64p, f64p = _lib.i32p, _lib.i64p, _lib.f64p
    rules = [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_uint64]
    S = _lib.SIGNATURES
    assert S["sgl_c_fuzzy_query"] == (C.c_int, [i32p, f64p, C.c_int64, C.c_int32, C.c_int64, f64p, f64p, f64p])
    assert S["sgl_c_umap_transform"] == (C.c_int, [i32p, f64p, C.c_int64, C.c_int32, f64p, C.c_int32, C.c_int64] + rules + [C.c_int64, f64p, f64p])
    assert S["sgl_op_umap_transform_epochs"] == (C.c_int, [i32p, f64p, C.c_int64, C.c_int32, f64p, C.c_int32, C.c_int64, f64p] + rules
                                                 + [C.c_int64, C.c_int32, C.c_int32, f64p])
    assert S["sgl_knn_index_set_layout"] == (C.c_int, [C.c_void_p, f64p, C.c_int32])
    assert S["sgl_knn_index_project"] == (C.c_int, [C.c_void_p, f64p, C.c_int64, C.c_int32, C.c_int32, C.c_int64] + rules + [i32p, f64p, f64p, f64p])
    assert S["sgl_umap_transform_info"] == (C.c_int, [i64p])


# -------------------------------------------------------------------------------------------------------------- refusals
def test_the_library_refuses_on_the_host_and_leaves_the_outputs_untouched(sa):
    """Every refusal happens before a device is touched, so the library answers here as it does on the GPU."""
    idx = np.array([[4, 1, 7], [2, 9, -1]], dtype=np.int32)
    dist = np.array([[0.0, 1.0, 1.0], [0.5, 0.75, INF]])
    Yref = np.arange(20.0).reshape(10, 2)
    ok = dict(a=1.0, b=1.0, n_epochs=30, alpha0=0.25, neg_rate=5, seed=1, query_offset=0)
    before = sa.umap_transform_info()

    def refused(msg, idx=idx, dist=dist, Yref=Yref, **kw):
        with pytest.raises(sa.SingletHipError, match=msg) as e:
            sa.umap_transform(idx, dist, Yref, **{**ok, **kw})
        assert e.value.code == -1

    refused(r"a and b must be finite and > 0", a=0.0)
    refused(r"a and b must be finite and > 0", b=np.nan)
    refused(r"n_epochs must lie in \[1, 2\^20\]", n_epochs=0)
    refused(r"n_epochs must lie in \[1, 2\^20\]", n_epochs=2 ** 20 + 1)
    refused(r"alpha0 must be finite and > 0", alpha0=np.inf)
    refused(r"neg_rate must lie in \[0, 255\]", neg_rate=256)
    refused(r"query_offset must be >= 0", query_offset=-1)
    refused(r"at most 2\^55", query_offset=2 ** 55 - 1)
    for (q, s, vi, vd), msg in (((0, 2, 10, None), r"query 0 at slot 2: index outside \[-1, n_ref\)"), ((0, 2, 4, None), "query 0 at slot 2: index repeated"),
                               ((0, 1, None, np.nan), "query 0 at slot 1: distance is not finite"), ((1, 0, None, -0.5), "query 1 at slot 0: distance is negative"),
                               ((1, 1, None, 0.25), "query 1 at slot 1: distances not ascending")):
        i, d = idx.copy(), dist.copy()
        if vi is not None:
            i[q, s] = vi
        if vd is not None:
            d[q, s] = vd
        refused(msg, idx=i, dist=d)
        with pytest.raises(sa.SingletHipError, match=msg):
            sa.fuzzy_query(i, d, 10)
    refused("query 0 at slot 2: a valid slot behind a padding slot", idx=np.array([[2, -1, 3]], dtype=np.int32), dist=np.array([[0.5, INF, 1.0]]))
    bad = Yref.copy()
    bad[3, 1] = np.inf
    refused(r"a reference position is not finite \(Yref, at position 7\)", Yref=bad)
    with pytest.raises(sa.SingletHipError, match=r"n_ref must lie in \[1, 2\^31\)"):
        sa.fuzzy_query(idx, dist, 0)
    with pytest.raises(ValueError, match=r"K in \[1, 256\]"):
        sa.umap_transform(np.zeros((1, 257), dtype=np.int32), np.zeros((1, 257)), Yref, 1.0, 1.0)
    with pytest.raises(ValueError, match=r"dim in \[1, 8\]"):
        sa.umap_transform(idx, dist, np.zeros((10, 9)), 1.0, 1.0)
    # the stage operator: the range of epochs, W, Yin
    W = np.array([[1.0, 0.5, 0.25], [1.0, 0.5, 0.0]])
    Yin = np.ones((2, 2))
    opk = dict(a=1.0, b=1.0, n_epochs=30, alpha0=0.25, neg_rate=5, seed=1)
    for t0, t1 in ((0, 3), (8, 7), (1, 31)):
        with pytest.raises(sa.SingletHipError, match="1 <= t_first <= t_last <= n_epochs"):
            sa.op_umap_transform_epochs(idx, W, Yref, Yin, t_first=t0, t_last=t1, **opk)
    Wb = W.copy()
    Wb[1, 1] = 1.5
    with pytest.raises(sa.SingletHipError, match=r"query 1 at slot 1: membership outside \[0, 1\]"):
        sa.op_umap_transform_epochs(idx, Wb, Yref, Yin, t_first=1, t_last=3, **opk)
    Yb = Yin.copy()
    Yb[1, 0] = np.nan
    with pytest.raises(sa.SingletHipError, match=r"a query position is not finite \(Yin, query 1, component 0\)"):
        sa.op_umap_transform_epochs(idx, W, Yref, Yb, t_first=1, t_last=3, **opk)
    # the C entry itself leaves its outputs untouched, and no query at all is SGL_OK with nothing written
    from singlet_amd import _lib
    L, f64p, i32p = _lib.load(), _lib.f64p, _lib.i32p
    Y0, Y = np.full((2, 2), 7.0), np.full((2, 2), 9.0)
    i = np.ascontiguousarray(idx)
    i[0, 2] = 4
    rc = L.sgl_c_umap_transform(_lib.ptr(i, i32p), _lib.ptr(dist, f64p), 2, 3, _lib.ptr(Yref, f64p), 2, 10, 1.0, 1.0, 30, 0.25, 5, 1, 0,
                                _lib.ptr(Y0, f64p), _lib.ptr(Y, f64p))
    assert rc == -1 and (Y0 == 7.0).all() and (Y == 9.0).all()
    rc = L.sgl_c_umap_transform(_lib.ptr(i, i32p), _lib.ptr(dist, f64p), 0, 3, _lib.ptr(Yref, f64p), 2, 10, 1.0, 1.0, 30, 0.25, 5, 1, 0,
                                _lib.ptr(Y0, f64p), _lib.ptr(Y, f64p))
    assert rc == 0 and (Y0 == 7.0).all() and (Y == 9.0).all()
    assert sa.umap_transform(idx[:0], dist[:0], Yref, 1.0, 1.0).shape == (0, 2)
    assert sa.umap_transform_info() == before    # a refused call leaves the report as it was


def test_python_defaults_follow_umap_learns_transform():
    from singlet_amd import api
    import inspect
    assert api._transform_epochs(10000, None) == 100 and api._transform_epochs(10001, None) == 30 and api._transform_epochs(5, 12) == 12
    sig = inspect.signature(api.umap_transform).parameters
    assert sig["alpha0"].default == 0.25 * inspect.signature(api.run_umap).parameters["learning_rate"].default
    assert sig["neg_rate"].default == 5 and sig["query_offset"].default == 0
    assert inspect.signature(api.run_umap).parameters["return_model"].default is False
    assert inspect.signature(api.map_query).parameters["layout"].default is False
    assert inspect.signature(api.ReferenceIndex.__init__).parameters["layout"].default is None


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_host_logic_under_address_and_undefined_sanitizers(tmp_path):
    """The refusals, the plan and the cut of the epochs into launches hold no HIP call: they are compiled with a host
    compiler into a program of their own (tests/umap_transform_host_main.cpp) with both sanitizers and run here, on the CPU."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "umap_transform_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "umap_transform_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("umap_transform_host: ok"), (r.stdout, r.stderr)
