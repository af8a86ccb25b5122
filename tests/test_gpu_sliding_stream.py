"""The sliding-window entry stream of the LDS-tiled accumulate (kernels_tiled.hip): the LDS tile is a ring of two row blocks,
each chunk finishes its block and runs ahead into the next.  The device's stored-entry count against the host model
(scripts/layout_emulate.py), bit equality with the plain kernel on matrices that stress the window, and the split ranges."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import rel_fro, to_dgc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("layout_emulate", os.path.join(ROOT, "scripts", "layout_emulate.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


L = _model()


def _csc_from_dense(D):
    p = np.concatenate([[0], np.cumsum((D != 0).sum(axis=0))]).astype(np.int32)
    r, c = np.nonzero(D.T)
    return D.T[r, c].astype(np.float64), c.astype(np.int32), p, D.shape[0], D.shape[1]


def _skewed_csc(ora, m, n, seed, sigma=1.3, mean=40.0):
    rng = np.random.default_rng(seed)
    want = np.minimum((rng.lognormal(np.log(mean), sigma, n)).astype(np.int64), m)
    want[rng.integers(0, n, 5)] = 0
    is_, p = [], [0]
    for c in range(n):
        r = np.sort(rng.choice(m, size=int(want[c]), replace=False))
        is_.append(r)
        p.append(p[-1] + r.size)
    i = np.concatenate(is_).astype(np.int32)
    return ora.CSC(rng.random(i.size) + 0.25, i, np.array(p, dtype=np.int32), m, n)


def _pbmc3k(ora):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    return ora.CSC(g["x"].astype(np.float64), i.astype(np.int32), p.astype(np.int32), int(dim[0]), int(dim[1]))


def _layout(sa, ora, A, k):
    c = sa.Context(0)
    try:
        c.upload(to_dgc(sa, A), to_dgc(sa, A.t()))
        c.fit_init(k, ora.synth_winit(k, A.nrow))
        return c.layout_get()
    finally:
        c.close()


@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("matrix", ["iid", "pbmc3k", "skewed"])
@pytest.mark.parametrize("full", [True, False])
def test_device_stream_size_equals_the_host_model(sa, ora, matrix, k, full, monkeypatch):
    """Stored entries of both orientations, quad (k = 10) and pair (k = 50) layout, LDS-sized and shortened tiles, the tile
    ranges the build chose: exactly the host model's count"""
    if full:
        monkeypatch.setenv("SGL_TILED_FULL_TILES", "1")
    A = {"iid": lambda: ora.synth_csc(2500, 3000, 10), "pbmc3k": lambda: _pbmc3k(ora),
         "skewed": lambda: _skewed_csc(ora, 1500, 700, 3)}[matrix]()
    lay = _layout(sa, ora, A, k)
    nsl = 4 if k <= 32 else 2
    At = A.t()
    for o, M in (("A", A), ("At", At)):
        got = lay[o]
        assert got["tiles"] == (M.nrow + got["tile_rows"] - 1) // got["tile_rows"]
        want = L.entries(M.p, M.i, M.nrow, k, nsl, got["tile_rows"], ranges=got["tile_ranges"])
        assert got["entries"] == want, (matrix, o, got, want)


def _window_stress(m, n, D, seed):
    """columns that stress the window of D-row blocks: dense over every block, entries in the last block only, pairs of equal
    count whose entries sit in different blocks (run-ahead), empty columns, a block without entries, a sparse background"""
    rng = np.random.default_rng(seed)
    X = np.where(rng.random((m, n)) < 0.03, rng.random((m, n)) + 0.1, 0.0)
    X[D:2 * D, :] = 0                                  # an empty block (row count not a multiple of D: m % D != 0)
    X[:, 40:70] = 0                                    # empty columns
    X[:, 0] = rng.random(m) + 0.1                      # dense across every window
    X[:, 1] = 0
    X[m - min(m % D or D, 150):, 1] = rng.random(min(m % D or D, 150)) + 0.1   # only in the last block
    X[:, 2] = 0
    X[(m // D - 1) * D - 100:(m // D - 1) * D, 2] = 1.5   # the end of the block before the last one
    for a, (r0, r1) in enumerate([(0, 150), (2 * D, 2 * D + 150), (3 * D + 10, 3 * D + 160)]):
        X[:, 80 + a] = 0
        X[r0:r1, 80 + a] = rng.random(r1 - r0) + 0.1      # equal counts (neighbours in the sorted order), different blocks
    return X


@pytest.mark.parametrize("k,layout", [(7, "quad"), (10, "quad"), (10, "pair"), (32, "quad"), (33, "pair"), (50, "pair"),
                                      (63, "pair"), (64, "pair")])
def test_window_stress_bit_equal_to_the_plain_kernel(sa, ora, k, layout, monkeypatch):
    monkeypatch.setenv("SGL_TILED_RANGES", "1")
    monkeypatch.setenv("SGL_TILED_FULL_TILES", "1")
    if layout == "pair":
        monkeypatch.setenv("SGL_TILED_NO_QUAD", "1")
    nsl = 4 if layout == "quad" else 2
    D = L.tile_rows(k, nsl) // 2
    m = 7 * D + 37
    X = _window_stress(m, 300, D, k)
    A = ora.CSC(*_csc_from_dense(X))
    At = A.t()
    rng = np.random.default_rng(k)
    W, H = rng.random((m, k)), rng.random((A.ncol, k))
    c = sa.Context(0)
    try:
        c.upload(to_dgc(sa, A), to_dgc(sa, At))
        for which, F, M in ((2, W, A), (3, H, At)):
            got = c.op_rhs(which, F)
            assert np.array_equal(got, c.op_rhs(which - 2, F)), "tiled and plain kernels add the same products in the same order"
            assert rel_fro(got, ora.rhs(M, F)) < 1e-14
        c.fit_init(k, ora.synth_winit(k, m))
        lay = c.layout_get()
    finally:
        c.close()
    assert lay["A"]["entries"] == L.entries(A.p, A.i, m, k, nsl, lay["A"]["tile_rows"])


@pytest.mark.parametrize("k", [70, 128])
def test_window_stress_rank_parts(sa, ora, k, monkeypatch):
    """Ranks above 64: quad passes over factor parts (strided rows of F) on the same stream"""
    monkeypatch.setenv("SGL_TILED_RANGES", "1")
    monkeypatch.setenv("SGL_TILED_FULL_TILES", "1")
    D = 632 // 2
    m = 5 * D + 11
    X = _window_stress(m, 260, D, k)
    A = ora.CSC(*_csc_from_dense(X))
    At = A.t()
    rng = np.random.default_rng(k)
    W, H = rng.random((m, k)), rng.random((A.ncol, k))
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A), to_dgc(sa, At))
        assert rel_fro(c.op_rhs(2, W), ora.rhs(A, W)) < 1e-14
        assert rel_fro(c.op_rhs(3, H), ora.rhs(At, H)) < 1e-14


@pytest.mark.parametrize("k,ranges", [(10, 2), (10, 5), (50, 3), (50, 4), (31, 2)])
def test_window_stress_forced_ranges(sa, ora, k, ranges, monkeypatch):
    """Tile ranges over blockIdx.y: the schedule never runs ahead across a range edge (each range its own slab)"""
    monkeypatch.setenv("SGL_TILED_RANGES", str(ranges))
    monkeypatch.setenv("SGL_TILED_FULL_TILES", "1")
    nsl = 4 if k <= 32 else 2
    D = L.tile_rows(k, nsl) // 2
    m = 11 * D + 5
    X = _window_stress(m, 400, D, 100 + k)
    A = ora.CSC(*_csc_from_dense(X))
    At = A.t()
    rng = np.random.default_rng(ranges)
    W, H = rng.random((m, k)), rng.random((A.ncol, k))
    c = sa.Context(0)
    try:
        c.upload(to_dgc(sa, A), to_dgc(sa, At))
        got = c.op_rhs(2, W), c.op_rhs(3, H)
        c.fit_init(k, ora.synth_winit(k, m))
        lay = c.layout_get()
    finally:
        c.close()
    assert lay["A"]["tile_ranges"] == ranges
    assert lay["A"]["entries"] == L.entries(A.p, A.i, m, k, nsl, lay["A"]["tile_rows"], ranges=ranges)
    assert rel_fro(got[0], ora.rhs(A, W)) < 1e-14 and rel_fro(got[1], ora.rhs(At, H)) < 1e-14


def test_padding_on_a_30000_row_iid_matrix(sa, ora, monkeypatch):
    """30 000 genes x 4000 cells at 5 % (config 3's column height), k = 50, the tile range whole as config 3's cell side runs
    it: at most 1.08 stored entries per non-zero (1.19 - 1.21 with runs padded in lock step per tile)"""
    monkeypatch.setenv("SGL_TILED_RANGES", "1")   # (a matrix this narrow is cut into 25 ranges, and the window stops at their edges)
    A = ora.synth_csc(30000, 4000, 20)
    lay = _layout(sa, ora, A, 50)
    assert lay["A"]["tile_rows"] == 408
    assert lay["A"]["entries"] / A.p[-1] <= 1.08, lay
