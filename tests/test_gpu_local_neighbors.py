"""Spatial neighbour graphs on the GPU (sgl_c_lknn / sgl_c_snn, kernels_neighbors.hip) against the test-side restatement
(tests/local_neighbors_restatement.py): bit-exact graphs over metrics, radii, k, max_dist and input shapes; ties, NaN
distances, the segmented-sort path of crowded buckets, refusals, determinism; SNN on LKNN output, random, non-square and
hub graphs, its 2^31 refusal; the 10^6-cell lattice on a sample; the find_local_neighbors / rescale_spatial mirrors and an
end-to-end run_gcnmf on the SNN."""
import zlib

import numpy as np
import pytest

import local_neighbors_restatement as lr

pytestmark = pytest.mark.gpu
F = np.float32


def _bits(x):
    """bit patterns, every NaN as one value (the sign of a NaN is not part of the comparison)"""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = np.nan
    return x.view(np.uint64)


def _same(got, ref):
    p, i, x = ref
    assert got.Dim == (len(p) - 1, len(p) - 1)
    assert np.array_equal(got.p, p), np.nonzero(got.p != p)[0][:5]
    assert np.array_equal(got.i, i)
    assert np.array_equal(_bits(got.x), _bits(x)), np.nonzero(_bits(got.x) != _bits(x))[0][:5]


def _lknn(sa, m, x, y, k, r, metric, sim=True, md=0.0):
    return sa.c_LKNN(m, x, y, k, r, metric, sim, md, False, 0)


def _coords(kind, n, rng):
    if kind == "lattice":
        side = int(round(np.sqrt(n)))
        return lr.lattice(side)
    if kind == "offset":
        side = int(round(np.sqrt(n)))
        return lr.lattice(side, offset=1e6)
    if kind == "float":
        return rng.random(n) * 12, rng.random(n) * 12
    x, y = lr.lattice(int(round(np.sqrt(n // 2))))   # duplicates: every site twice
    return np.concatenate([x, x]), np.concatenate([y, y])


def _embedding(D, n, rng, zeros=0.3):
    return rng.random((D, n)) * (rng.random((D, n)) >= zeros)


EXACT = ("jaccard", "cosine", "euclidean", "manhattan", "hamming")


@pytest.mark.parametrize("metric", EXACT)
@pytest.mark.parametrize("kind,radius,k,md,D", [
    ("lattice", 1.0, 5, 0.0, 3),
    ("lattice", float(np.sqrt(F(2))), 20, 0.0, 10),
    ("lattice", 4.0, 20, 0.1, 10),
    ("lattice", 5.0, 100, 0.0, 1),        # 3-4-5 triangles sit on the boundary
    ("offset", 1.0, 5, 0.0, 3),           # float spacing at 10^6
    ("offset", 5.0, 20, 1e30, 3),
    ("float", 1.0, 5, 0.0, 50),
    ("float", 4.0, 1, 0.1, 3),
    ("dups", 0.0, 0, 0.0, 3),
    ("dups", 1.0, 5, 0.0, 257),
])
def test_lknn_bit_exact(sa, metric, kind, radius, k, md, D):
    rng = np.random.default_rng(zlib.crc32(repr((metric, kind, radius, k, D)).encode()))
    x, y = _coords(kind, 400, rng)
    m = _embedding(D, x.size, rng)
    try:
        ref = lr.lknn_brute(m, x, y, k, radius, metric, True, md)
    except lr.SlotOverflow:
        with pytest.raises(sa.SingletHipError, match="slots"):
            _lknn(sa, m, x, y, k, radius, metric, True, md)
        return
    _same(_lknn(sa, m, x, y, k, radius, metric, True, md), ref)


@pytest.mark.parametrize("metric", ("jaccard", "cosine"))
@pytest.mark.parametrize("transpose", (False, True))
def test_lknn_similarity_flag_and_orientation(sa, metric, transpose):
    rng = np.random.default_rng(3)
    x, y = lr.lattice(15)
    m = _embedding(6, x.size, rng)
    for sim in (True, False):
        ref = lr.lknn_brute(m, x, y, 5, 2.0, metric, sim, 0.0)
        _same(_lknn(sa, m.T if transpose else m, x, y, 5, 2.0, metric, sim), ref)


@pytest.mark.parametrize("radius,k,md", [(1.0, 5, 0.0), (2.0, 3, 1.5), (4.0, 20, 0.0)])
def test_lknn_kl_within_ulps(sa, radius, k, md):
    rng = np.random.default_rng(11)
    x, y = lr.lattice(20)
    m = rng.random((5, x.size)) + 0.05
    got = _lknn(sa, m, x, y, 10**6, radius, "kl", True, md)     # no selection: every candidate compared
    ref = lr.lknn_brute(m, x, y, 10**6, radius, "kl", True, md)
    assert np.array_equal(got.p, ref[0]) and np.array_equal(got.i, ref[1])
    assert np.all(np.abs(got.x - ref[2]) <= 8 * np.spacing(np.abs(ref[2]).astype(F)))
    # with selection: compare the columns whose k-th gap is wider than the tolerance
    got = _lknn(sa, m, x, y, k, radius, "kl", True, md)
    full = ref
    refk = lr.lknn_brute(m, x, y, k, radius, "kl", True, md)
    checked = 0
    for c in range(x.size):
        d = np.sort(full[2][full[0][c]:full[0][c + 1]])
        if d.size > k and d[k] - d[k - 1] <= 16 * np.spacing(F(abs(d[k]))):
            continue
        assert np.array_equal(got.i[got.p[c]:got.p[c + 1]], refk[1][refk[0][c]:refk[0][c + 1]])
        checked += 1
    assert checked > x.size // 2


def test_lknn_forced_ties_and_nan(sa):
    x, y = lr.lattice(12)
    m = np.zeros((3, x.size))
    m[:, ::3] = 1.0                      # many equal distances; every third point all-zero -> NaN under jaccard / cosine
    m[0, 1::3] = 2.0
    for metric in ("jaccard", "cosine", "euclidean"):
        for k in (1, 3, 5, 100):           # <= k candidates (exact) and > k (the documented rule)
            _same(_lknn(sa, m, x, y, k, 2.0, metric), lr.lknn_brute(m, x, y, k, 2.0, metric, True, 0.0))


def test_lknn_crowded_bucket_takes_the_segmented_sort(sa):
    rng = np.random.default_rng(5)
    n = 1500                               # every point in one bucket: 1500 candidates > the LDS cap of 512
    x, y = rng.random(n) * 3, rng.random(n) * 3
    m = _embedding(4, n, rng)
    for metric, k in (("euclidean", 7), ("jaccard", 20), ("hamming", 3)):
        ref = lr.lknn_grid(m, x, y, k, 30.0, metric, True, 0.0)
        _same(_lknn(sa, m, x, y, k, 30.0, metric), ref)
    # mixed: one dense clump among sparse points
    x2 = np.concatenate([rng.random(700) * 0.5, rng.random(300) * 40])
    y2 = np.concatenate([rng.random(700) * 0.5, rng.random(300) * 40])
    m2 = _embedding(4, 1000, rng)
    _same(_lknn(sa, m2, x2, y2, 5, 2.0, "cosine"), lr.lknn_grid(m2, x2, y2, 5, 2.0, "cosine", True, 0.0))


def test_lknn_refusals(sa):
    x, y = np.zeros(3), np.zeros(3)
    m = np.array([[1.0, 2.0, 3.0]])
    with pytest.raises(sa.SingletHipError, match="slots"):
        _lknn(sa, m, x, y, 5, 0.0, "euclidean")
    xs, ys = lr.lattice(4)
    ms = np.ones((2, 16))
    bad = ms.copy()
    bad[1, 3] = np.nan
    with pytest.raises(sa.SingletHipError, match="NaN or infinite"):
        _lknn(sa, bad, xs, ys, 5, 1.0, "euclidean")
    bx = xs.copy()
    bx[2] = np.inf
    with pytest.raises(sa.SingletHipError, match="not finite"):
        _lknn(sa, ms, bx, ys, 5, 1.0, "euclidean")
    for r in (-1.0, np.nan, np.inf):
        with pytest.raises(sa.SingletHipError, match="radius"):
            _lknn(sa, ms, xs, ys, 5, r, "euclidean")
    with pytest.raises(sa.SingletHipError, match="number of columns in 'm'"):
        _lknn(sa, np.ones((2, 15)), xs, ys, 5, 1.0, "euclidean")
    with pytest.raises(sa.SingletHipError, match="length of coordinate vectors"):
        _lknn(sa, ms, xs, ys[:-1], 5, 1.0, "euclidean")


def test_lknn_two_call_contract_and_determinism(sa):
    import ctypes as C
    from singlet_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(9)
    x, y = rng.random(3000) * 30, rng.random(3000) * 30
    m = np.asfortranarray(_embedding(8, 3000, rng))
    a = _lknn(sa, m, x, y, 20, 3.0, "jaccard")
    b = _lknn(sa, m, x, y, 20, 3.0, "jaccard")
    assert np.array_equal(a.p, b.p) and np.array_equal(a.i, b.i) and np.array_equal(_bits(a.x), _bits(b.x))
    p = np.empty(3001, np.int32)
    nnz = C.c_int64()
    i = np.empty(max(a.nnz - 1, 1), np.int32)
    xx = np.empty(max(a.nnz - 1, 1))
    rc = L.sgl_c_lknn(m.ctypes.data_as(_lib.f64p), 8, 3000, _lib.ptr(x, _lib.f64p), _lib.ptr(y, _lib.f64p), 3000, 20, 3.0,
                      b"jaccard", 1, 0.0, _lib.ptr(p, _lib.i32p), C.byref(nnz), _lib.ptr(i, _lib.i32p), _lib.ptr(xx, _lib.f64p),
                      a.nnz - 1)
    assert rc == -1 and nnz.value == a.nnz and np.array_equal(p, a.p)


# ------------------------------------------------------------------------------------------------------------------ SNN ---
def _snn_ref(G, ms):
    return lr.snn(G.i, G.p, G.nrow, G.ncol, ms)


def test_snn_on_lknn_output(sa):
    rng = np.random.default_rng(1)
    x, y = lr.lattice(30)
    m = _embedding(5, x.size, rng)
    knn = _lknn(sa, m, x, y, 10, 2.0, "jaccard", True, 0.1)
    for ms in (0.0, 1 / 15, 0.5, 1.0, 2.0):
        _same(sa.c_SNN(knn, ms, 0), _snn_ref(knn, ms))


@pytest.mark.parametrize("nrow,ncol,dens", [(200, 200, 0.03), (50, 300, 0.1), (400, 60, 0.05), (1000, 800, 0.002)])
def test_snn_random_and_non_square(sa, nrow, ncol, dens):
    import scipy.sparse as sp
    R = sp.random(nrow, ncol, density=dens, format="csc", random_state=nrow + ncol).tolil()
    R[:, [0, ncol // 2]] = 0                                  # empty columns included
    R = R.tocsc()
    R.eliminate_zeros()
    G = sa.dgCMatrix.from_scipy(R)
    assert G.p[1] == 0 and G.p[ncol // 2] == G.p[ncol // 2 + 1]
    for ms in (0.0, 0.2, 1.0):
        _same(sa.c_SNN(G, ms, 0), _snn_ref(G, ms))


def test_snn_hub_row(sa):
    import scipy.sparse as sp
    n = 5000
    R = sp.random(n, n, density=0.002, format="lil", random_state=4)
    R[7, :3000] = 1.0                      # one row in 3000 columns: gathered lists of 3000+ (> the LDS cap of 2048)
    G = sa.dgCMatrix.from_scipy(R.tocsc())
    for ms in (0.0, 0.3):
        _same(sa.c_SNN(G, ms, 0), _snn_ref(G, ms))


def test_snn_refuses_2e31_entries(sa):
    n = 50000                              # a hub in every column: 50000^2 = 2.5e9 entries
    G = sa.dgCMatrix(np.ones(n), np.zeros(n, np.int32), np.arange(n + 1, dtype=np.int32), (1, n))
    with pytest.raises(sa.SingletHipError, match="dgCMatrix"):
        sa.c_SNN(G, 0.0, 0)


def test_snn_refuses_an_invalid_pattern(sa):
    G = sa.dgCMatrix([1.0, 1.0], [1, 0], [0, 2], (2, 1))
    with pytest.raises(sa.SingletHipError, match="ascending"):
        sa.c_SNN(G, 0.0, 0)
    G = sa.dgCMatrix([1.0], [5], [0, 1], (2, 1))
    with pytest.raises(sa.SingletHipError, match="outside"):
        sa.c_SNN(G, 0.0, 0)


# ------------------------------------------------------------------------------------------------- full size, mirrors ---
def test_million_cell_lattice_on_a_sample(sa):
    rng = np.random.default_rng(2026)
    x, y = lr.lattice(1000)
    m = rng.random((50, x.size)) * (rng.random((50, x.size)) < 0.5)
    knn = _lknn(sa, m, x, y, 20, 4.0, "jaccard", True, 0.0)   # (max_dist 1/10 would prune every jaccard distance here)
    assert knn.nnz > 19 * x.size
    pts = rng.choice(x.size, 20000, replace=False)
    ref = lr.lknn_grid(m, x, y, 20, 4.0, "jaccard", True, 0.0, points=pts)
    for c, (i, xv) in ref.items():
        assert np.array_equal(knn.i[knn.p[c]:knn.p[c + 1]], i), c
        assert np.array_equal(_bits(knn.x[knn.p[c]:knn.p[c + 1]]), _bits(xv)), c
    knn.x = np.ones_like(knn.x)
    snn = sa.c_SNN(knn, 1 / 15, 0)
    assert snn.nnz > 2 * knn.nnz
    ref = lr.snn(knn.i, knn.p, knn.nrow, knn.ncol, 1 / 15, columns=pts)
    for c, (i, xv) in ref.items():
        assert np.array_equal(snn.i[snn.p[c]:snn.p[c + 1]], i), c
        assert np.array_equal(_bits(snn.x[snn.p[c]:snn.p[c + 1]]), _bits(xv)), c


def test_rescale_spatial_and_find_local_neighbors(sa):
    rng = np.random.default_rng(8)
    side = 20
    gx, gy = lr.lattice(side)
    coords = np.stack([gx * 0.0125 + 0.1, gy * 0.02 + 0.3], axis=1) / 0.7   # scaled, shifted, different per axis
    sp = sa.rescale_spatial(coords)
    assert np.array_equal(sp[:, 0], gx) and np.array_equal(sp[:, 1], gy)
    emb = rng.random((side * side, 8))            # cells x factors, as cell.embeddings
    out = sa.find_local_neighbors(emb, sp, k_param=6, spatial_radius=2, nn_metric="cosine", dims=[1, 2, 3, 5])
    h = emb.T[[0, 1, 2, 4], :]
    p, i, x = lr.lknn_brute(h, sp[:, 0], sp[:, 1], 6, 2, "cosine", True, 1 / 10)
    assert np.array_equal(out["knn"].p, p) and np.array_equal(out["knn"].i, i) and np.all(out["knn"].x == 1)
    _same(out["snn"], lr.snn(i, p, side * side, side * side, 1 / 15))
    out = sa.find_local_neighbors(emb, sp, k_param=6, spatial_radius=2, nn_metric="euclidean", return_dist=True, compute_snn=False)
    assert out["snn"] is None
    _same(out["knn"], lr.lknn_brute(emb.T, sp[:, 0], sp[:, 1], 6, 2, "euclidean", True, 1 / 10))
    for kw, msg in ((dict(nn_metric="bogus"), "nn.metric"), (dict(use_dist=True, nn_metric="kl"), "dissimilarity"),
                    (dict(prune_knn=1), "prune.knn"), (dict(prune_snn=1.5), "prune.snn"), (dict(spatial_radius=100), "radius"),
                    (dict(dims=[9]), "dims")):
        with pytest.raises(ValueError, match=msg):
            sa.find_local_neighbors(emb, sp, **kw)


def test_run_gcnmf_on_the_snn(sa):
    import scipy.sparse as sps
    rng = np.random.default_rng(12)
    side = 24
    gx, gy = lr.lattice(side)
    n = side * side
    A = sa.dgCMatrix.from_scipy(sps.random(300, n, density=0.1, format="csc", random_state=3,
                                           data_rvs=lambda s: rng.integers(1, 6, s).astype(float)))
    model = sa.run_nmf(A, 5, verbose=0, seed=1, maxit=5)
    emb = np.asarray(model["h"]).T
    g = sa.find_local_neighbors(emb, np.stack([gx, gy], axis=1), k_param=8, spatial_radius=2)
    fit = sa.run_gcnmf(A, g["snn"], 5, verbose=0, seed=1, maxit=5)
    assert fit["w"].shape == (300, 5) and fit["h"].shape == (5, n)
    assert np.all(np.isfinite(fit["h"])) and np.all(fit["d"] > 0)
