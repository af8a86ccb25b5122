"""spatial_graph on the GPU (sgl_spatial_graph, kernels_neighbors.hip) against the test-side restatement
(tests/spatial_graph_restatement.py), bit-exact on p, i and x: random points, lattices with exact ties at max_dist, awkward
coordinates, the selection by index (max_k binding, 0, above n, permuted labels), pairs a fused multiply-add would change,
the all-in-range case at 10^6 points, 10^6-point sets on sampled columns, refusals, determinism, and GCNMF on the graph."""
import ctypes as C
import time

import numpy as np
import pytest

import gcnmf_restatement as gr
import spatial_graph_restatement as sr
from conftest import rel_fro, same_zero_pattern, to_dgc

pytestmark = pytest.mark.gpu


def _same(got, ref):
    p, i, x = ref
    n = len(p) - 1
    assert got.Dim == (n, n)
    assert np.array_equal(got.p, p), np.nonzero(got.p != p)[0][:5]
    assert np.array_equal(got.i, i)
    assert np.array_equal(got.x.view(np.uint64), np.asarray(x, dtype=np.float64).view(np.uint64)), \
        np.nonzero(got.x != x)[0][:5]


def _same_columns(got, x, y, max_dist, max_k, cols):
    ref = sr.columns(x, y, max_dist, max_k, cols)
    for c, (r, w) in ref.items():
        a, b = got.p[c], got.p[c + 1]
        assert np.array_equal(got.i[a:b], r), c
        assert np.array_equal(got.x[a:b].view(np.uint64), w.view(np.uint64)), c


@pytest.mark.parametrize("n,max_dist,max_k", [
    (1, 0.5, 100), (2, 2.0, 100), (3, 0.7, 100), (10, 0.3, 100), (100, 0.1, 100), (1000, 0.05, 100), (5000, 0.02, 100),
    (5000, 0.1, 100), (2000, 2.0, 100), (700, 0.3, 1), (700, 0.3, 5), (3000, 0.08, 37)])
def test_uniform_random(sa, n, max_dist, max_k):
    rng = np.random.default_rng(n * 31 + max_k)
    x, y = rng.random(n), rng.random(n)
    _same(sa.spatial_graph(x, y, max_dist, max_k), sr.brute(x, y, max_dist, max_k))


@pytest.mark.parametrize("max_dist", [1.0, float(np.sqrt(2.0)), 1.5, 2.0, 3.0])
def test_lattice_ties(sa, max_dist):
    # max_dist = 1: the 4-neighbours (d == 1) are out; max_dist = fl(sqrt(2)): the diagonals (d == fl(sqrt(2))) are out
    x, y = sr.lattice(37)
    got = sa.spatial_graph(x, y, max_dist)
    _same(got, sr.brute(x, y, max_dist))
    inner = 18 * 37 + 18
    expect = {1.0: 1, float(np.sqrt(2.0)): 5, 1.5: 9, 2.0: 9, 3.0: 25}[max_dist]
    assert got.p[inner + 1] - got.p[inner] == expect


@pytest.mark.parametrize("kind", ["duplicates", "offset1e6", "offset1e12", "negative", "crowded"])
def test_awkward_coordinates(sa, kind):
    rng = np.random.default_rng(5)
    max_dist, max_k = 1.5, 100
    if kind == "duplicates":
        x, y = sr.lattice(25)
        x, y = np.concatenate([x, x, x[:100]]), np.concatenate([y, y, y[:100]])
    elif kind == "offset1e6":
        x, y = sr.lattice(30, offset=1e6)
        x = x + rng.random(x.size) * 0.5
    elif kind == "offset1e12":
        x, y = sr.lattice(30, offset=1e12)
    elif kind == "negative":
        x, y = -rng.random(2500) * 40, -rng.random(2500) * 40 - 1e3
    else:   # one bucket holds most points, with more than max_k of them in range of each other
        x = np.concatenate([rng.random(3000) * 0.3 + 5, rng.random(1500) * 40])
        y = np.concatenate([rng.random(3000) * 0.3 + 5, rng.random(1500) * 40])
        max_dist, max_k = 0.5, 150
    _same(sa.spatial_graph(x, y, max_dist, max_k), sr.brute(x, y, max_dist, max_k))


@pytest.mark.parametrize("max_k", [0, 1, 5, 100, 10**12])
def test_max_k(sa, max_k):
    rng = np.random.default_rng(11)
    x, y = rng.random(400) * 3, rng.random(400) * 3
    got = sa.spatial_graph(x, y, 1.0, max_k)
    _same(got, sr.brute(x, y, 1.0, max_k))
    if max_k == 0:
        assert got.i.size == 0 and np.all(got.p == 0)
    if max_k == 10**12:   # acts as n
        _same(got, sr.brute(x, y, 1.0, 400))


def test_all_in_range_small(sa):
    # max_dist above the extent: every point is a candidate of every other, and each column keeps rows 0 .. max_k - 1
    rng = np.random.default_rng(2)
    x, y = rng.random(3000), rng.random(3000)
    got = sa.spatial_graph(x, y, 10.0, 64)
    _same(got, sr.brute(x, y, 10.0, 64))
    assert np.array_equal(got.i.reshape(3000, 64), np.broadcast_to(np.arange(64), (3000, 64)))


def test_empty_and_single(sa):
    got = sa.spatial_graph(np.zeros(0), np.zeros(0), 1.0)
    assert got.Dim == (0, 0) and list(got.p) == [0] and got.i.size == 0
    got = sa.spatial_graph([3.5], [-2.0], 1.0)
    assert list(got.p) == [0, 1] and list(got.i) == [0]
    _same(got, sr.brute([3.5], [-2.0], 1.0))


@pytest.mark.parametrize("kind", ["lattice", "random"])
def test_permuted_labels(sa, kind):
    # the selection is by index: labels in no spatial order must give the reference's answer, not a spatially sorted one
    rng = np.random.default_rng(17)
    if kind == "lattice":
        x, y = sr.lattice(60)
        max_dist, max_k = 2.5, 9
    else:
        x, y = rng.random(3600) * 20, rng.random(3600) * 20
        max_dist, max_k = 1.2, 6
    perm = rng.permutation(x.size)
    x, y = x[perm], y[perm]
    _same(sa.spatial_graph(x, y, max_dist, max_k), sr.brute(x, y, max_dist, max_k))


def test_contraction_sensitive_pairs(sa):
    rng = np.random.default_rng(23)
    x, y = rng.random(3000), rng.random(3000)
    max_dist = 0.05
    ref = sr.brute(x, y, max_dist, 100)
    p, i, _ = ref
    cols = np.repeat(np.arange(3000), np.diff(p))
    pairs = [(int(c), int(r)) for c, r in zip(cols[:3000], i[:3000]) if c != r]
    fused = sr.fused_pairs(x, y, pairs)
    assert len(fused) >= 20, len(fused)   # the fixture has teeth: a fused dx*dx + dy*dy changes d of these kept pairs
    _same(sa.spatial_graph(x, y, max_dist, 100), ref)


def test_all_in_range_million(sa):
    n, max_k = 10**6, 100
    rng = np.random.default_rng(29)
    x, y = rng.random(n) * 50, rng.random(n) * 50
    sa.spatial_graph(x[:1000], y[:1000], 100.0, max_k)   # warm-up: code objects, the sort's first call
    t0 = time.perf_counter()
    got = sa.spatial_graph(x, y, 100.0, max_k)
    dt = time.perf_counter() - t0
    assert dt < 20.0, dt   # O(n max_k) thanks to the early stop; a collect-then-select scan would be O(n^2)
    assert got.p[-1] == n * max_k
    assert np.array_equal(got.p, np.arange(n + 1, dtype=np.int64) * max_k)
    assert np.array_equal(got.i.reshape(n, max_k), np.broadcast_to(np.arange(max_k, dtype=np.int32), (n, max_k)))
    _same_columns(got, x, y, 100.0, max_k, rng.choice(n, 12, replace=False))


@pytest.mark.parametrize("kind,max_dist,max_k", [("lattice", 1.5, 100), ("lattice_perm", 2.3, 12), ("random", 2.5, 100),
                                                  ("random", 2.5, 5)])
def test_million_point_sets(sa, kind, max_dist, max_k):
    rng = np.random.default_rng(31)
    if kind.startswith("lattice"):
        x, y = sr.lattice(1000)
        if kind == "lattice_perm":
            perm = rng.permutation(x.size)
            x, y = x[perm], y[perm]
    else:
        x, y = rng.random(10**6) * 1000, rng.random(10**6) * 1000
    got = sa.spatial_graph(x, y, max_dist, max_k)
    cols = np.concatenate([rng.choice(x.size, 300, replace=False), [0, 999, x.size - 1]])
    _same_columns(got, x, y, max_dist, max_k, cols)
    cl = sr.CellList(x, y, max_dist, max_k)
    assert all(got.p[c + 1] - got.p[c] == cl.count(c) for c in cols[:50])


def _raises(fn, text):
    from singlet_amd import SingletHipError
    with pytest.raises(SingletHipError, match=text):
        fn()


def test_refusals(sa):
    x, y = np.arange(10.0), np.zeros(10)
    _raises(lambda: sa.spatial_graph(x, y[:9], 1.0), "differ in length")
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[3] = bad
        _raises(lambda: sa.spatial_graph(xb, y, 1.0), "coordinate 3 is not finite")
        _raises(lambda: sa.spatial_graph(y, xb, 1.0), "coordinate 3 is not finite")
    for md in (0.0, -1.0, np.nan, np.inf, -np.inf):
        _raises(lambda: sa.spatial_graph(x, y, md), "finite and > 0")
    for md in (5e-324, 1e-310):   # 1 / max_dist overflows
        _raises(lambda: sa.spatial_graph(x, y, md), "is not finite")
    _raises(lambda: sa.spatial_graph(x, y, 1.0, -1), "negative")


def _raw(sa, x, y, n, max_dist, max_k, p, nnz, i=None, v=None, cap=0):
    from singlet_amd import _lib
    from singlet_amd._lib import f64p, i32p, ptr
    L = _lib.load()
    return L.sgl_spatial_graph(ptr(x, f64p), ptr(y, f64p), n, max_dist, max_k, ptr(p, i32p), C.byref(nnz),
                               None if i is None else ptr(i, i32p), None if v is None else ptr(v, f64p), cap)


def test_abi_contract(sa):
    rng = np.random.default_rng(37)
    x, y = rng.random(500), rng.random(500)
    p = np.zeros(501, dtype=np.int32)
    nnz = C.c_int64()
    assert _raw(sa, x, y, 500, 0.1, 100, p, nnz) == 0
    ref = sr.brute(x, y, 0.1, 100)
    assert np.array_equal(p, ref[0]) and nnz.value == ref[0][-1]
    i = np.zeros(nnz.value, dtype=np.int32)
    v = np.zeros(nnz.value)
    assert _raw(sa, x, y, 500, 0.1, 100, p, nnz, i, v, nnz.value - 1) == -1   # cap < nnz
    assert _raw(sa, x, y, 500, 0.1, 100, p, nnz, i, None, nnz.value) == -1    # i_out without x_out
    assert _raw(sa, x, y, -1, 0.1, 100, p, nnz) == -1
    assert _raw(sa, x, y, 500, 0.1, -3, p, nnz) == -1
    assert _raw(sa, x, y, 500, 0.1, 100, p, nnz, i, v, nnz.value) == 0
    assert np.array_equal(i, ref[1]) and np.array_equal(v.view(np.uint64), ref[2].view(np.uint64))


def test_refuses_2_31_entries(sa):
    # 46341^2 >= 2^31: every point is in range of every other and max_k = n
    n = 46341
    rng = np.random.default_rng(41)
    x, y = rng.random(n), rng.random(n)
    _raises(lambda: sa.spatial_graph(x, y, 10.0, n), "cannot hold")
    got = sa.spatial_graph(x[:2000], y[:2000], 10.0, 2000)   # the library is usable afterwards
    assert got.p[-1] == 2000 * 2000


def test_deterministic(sa):
    rng = np.random.default_rng(43)
    x, y = rng.random(40000) * 100, rng.random(40000) * 100
    a = sa.spatial_graph(x, y, 1.7, 30)
    b = sa.spatial_graph(x, y, 1.7, 30)
    assert np.array_equal(a.p, b.p) and np.array_equal(a.i, b.i)
    assert np.array_equal(a.x.view(np.uint64), b.x.view(np.uint64))


def test_integer_valued_input(sa):
    # integer arrays are taken as doubles (Rcpp's std::vector<double>)
    x, y = sr.lattice(20)
    got = sa.spatial_graph(x.astype(np.int32), y.astype(np.int64), 1.5, 100)
    _same(got, sr.brute(x, y, 1.5, 100))


def test_gcnmf_on_the_spatial_graph(sa, ora):
    side = 18
    n = side * side
    x, y = sr.lattice(side)
    G = sa.spatial_graph(x, y, 1.5)
    ref_G = gr.lattice_graph(ora, side)
    assert np.array_equal(G.p, ref_G.p) and np.array_equal(G.i, ref_G.i)
    # the helper divides by 1.5 where spatial_graph multiplies by fl(1 / 1.5): a few ulps apart
    assert np.allclose(G.x, ref_G.x, rtol=8 * np.finfo(np.float64).eps, atol=0)
    assert np.allclose(np.add.reduceat(G.x, G.p[:-1]), 1.0, rtol=1e-15)
    m, k, maxit = 210, 8, 4
    A = ora.synth_csc(m, n, 12)
    At = A.t()
    w0 = ora.synth_winit(k, m)
    Gc = ora.CSC(G.x.copy(), G.i.astype(np.int32), G.p.astype(np.int32), n, n)
    ref = gr.c_gcnmf(ora, A, At, Gc, 0.0, maxit, 0.01, 0.0, w0)
    got = sa.c_gcnmf(to_dgc(sa, A), to_dgc(sa, At), G, 0.0, maxit, False, 0.01, 0.0, 0, w0.T)
    for key in ("w", "h", "d"):
        g = got[key].T if key == "h" else got[key]
        assert rel_fro(g, ref[key]) < 1e-9, (key, rel_fro(g, ref[key]))
        if g.ndim == 2:
            assert same_zero_pattern(g, ref[key]), key
    fit = sa.run_gcnmf(to_dgc(sa, A), G, k, verbose=0, seed=1, maxit=3)
    assert fit["w"].shape == (m, k) and fit["h"].shape == (k, n)
    assert np.all(np.isfinite(fit["h"])) and np.all(fit["d"] > 0)
