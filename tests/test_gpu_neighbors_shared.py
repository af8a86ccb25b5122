"""What sgl_c_lknn, sgl_c_snn and sgl_spatial_graph share in kernels_neighbors.hip -- the two-call CSC tail and the spatial cell
list -- checked for each of them: the raw two-call contract, empty and one-point inputs with hand-written results, and
point sets on one line, where the grid is a single bucket row or column and every neighbouring row / column of the boundary
table lies outside the grid or is empty."""
import ctypes as C
import functools

import numpy as np
import pytest

import local_neighbors_restatement as lr
import spatial_graph_restatement as sr

pytestmark = pytest.mark.gpu


def _bits(x):
    """bit patterns, every NaN as one value"""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = np.nan
    return x.view(np.uint64)


def _same(got, ref):
    p, i, x = ref
    assert np.array_equal(got.p, p), np.nonzero(got.p != p)[0][:5]
    assert np.array_equal(got.i, i)
    assert np.array_equal(_bits(got.x), _bits(x)), np.nonzero(_bits(got.x) != _bits(x))[0][:5]


# ------------------------------------------------------------------------------------------------- two-call contract ---
@functools.lru_cache(maxsize=None)
def _two_call_case(entry):
    """(n, reference (p, i, x), call(L, p, nnz, i, x, cap)) of one entry point; the inputs stay alive in the closure"""
    from singlet_amd._lib import f64p, i32p, ptr
    rng = np.random.default_rng(41)
    x, y = rng.random(500) * 12, rng.random(500) * 12
    if entry == "sgl_c_lknn":
        m = np.asfortranarray(rng.random((4, 500)) * (rng.random((4, 500)) >= 0.3))
        ref = lr.lknn_brute(m, x, y, 5, 2.0, "euclidean", True, 0.0)
        return 500, ref, lambda L, *out: L.sgl_c_lknn(m.ctypes.data_as(f64p), 4, 500, ptr(x, f64p), ptr(y, f64p), 500, 5, 2.0,
                                                      b"euclidean", 1, 0.0, *out)
    if entry == "sgl_c_snn":
        import scipy.sparse as sp
        R = sp.random(200, 200, density=0.03, format="csc", random_state=7)
        Gi, Gp = R.indices.astype(np.int32), R.indptr.astype(np.int32)
        ref = lr.snn(Gi, Gp, 200, 200, 0.1)
        return 200, ref, lambda L, *out: L.sgl_c_snn(ptr(Gi, i32p), ptr(Gp, i32p), 200, 200, 0.1, *out)
    ref = sr.brute(x, y, 1.5, 100)
    return 500, ref, lambda L, *out: L.sgl_spatial_graph(ptr(x, f64p), ptr(y, f64p), 500, 1.5, 100, *out)


@pytest.mark.parametrize("entry", ["sgl_c_lknn", "sgl_c_snn", "sgl_spatial_graph"])
def test_two_call_contract(sa, entry):
    from singlet_amd import _lib
    from singlet_amd._lib import f64p, i32p, ptr
    L = _lib.load()
    n, (rp, ri, rx), call = _two_call_case(entry)
    assert rp[-1] > n   # more than the diagonal / one neighbour per point: there is something to cut

    def fresh():
        return np.full(n + 1, -1, dtype=np.int32), C.c_int64(-1)

    p, nnz = fresh()
    assert call(L, ptr(p, i32p), C.byref(nnz), None, None, 0) == 0                      # count only
    assert np.array_equal(p, rp) and nnz.value == rp[-1]
    i, v = np.full(nnz.value, -1, dtype=np.int32), np.zeros(nnz.value)
    p, nnz = fresh()
    assert call(L, ptr(p, i32p), C.byref(nnz), ptr(i, i32p), ptr(v, f64p), rp[-1] - 1) == -1   # cap = nnz - 1
    assert b"capacity" in L.sgl_last_error()
    assert np.array_equal(p, rp) and nnz.value == rp[-1]                                # ... with p and nnz already filled
    p, nnz = fresh()
    assert call(L, ptr(p, i32p), C.byref(nnz), ptr(i, i32p), None, int(rp[-1])) == -1   # i_out without x_out
    assert call(L, ptr(p, i32p), C.byref(nnz), ptr(i, i32p), ptr(v, f64p), int(rp[-1])) == 0
    assert np.array_equal(p, rp) and nnz.value == rp[-1]
    assert np.array_equal(i, ri) and np.array_equal(_bits(v), _bits(rx))


# ---------------------------------------------------------------------------------------------- empty and one point ---
def test_lknn_empty_and_one_point(sa):
    g = sa.c_LKNN(np.zeros((4, 0)), np.zeros(0), np.zeros(0), 5, 1.0, "euclidean", True, 0.0, False, 0)
    assert g.Dim == (0, 0) and np.array_equal(g.p, [0]) and g.i.size == 0 and g.x.size == 0
    g = sa.c_LKNN(np.ones((4, 1)), np.array([3.0]), np.array([-2.0]), 5, 1.0, "euclidean", True, 0.0, False, 0)
    assert g.Dim == (1, 1) and np.array_equal(g.p, [0, 0]) and g.i.size == 0 and g.x.size == 0


def test_snn_empty_and_one_column(sa):
    g = sa.c_SNN(sa.dgCMatrix([], [], [0], (3, 0)), 0.0, 0)
    assert g.Dim == (0, 0) and np.array_equal(g.p, [0]) and g.i.size == 0 and g.x.size == 0
    g = sa.c_SNN(sa.dgCMatrix([1.0], [1], [0, 1], (3, 1)), 0.0, 0)
    assert g.Dim == (1, 1) and np.array_equal(g.p, [0, 1]) and np.array_equal(g.i, [0]) and np.array_equal(g.x, [1.0])


# ------------------------------------------------------------------------------- one bucket row, one bucket column ---
@functools.lru_cache(maxsize=None)
def _line():
    rng = np.random.default_rng(53)
    return rng.random(300) * 40, np.full(300, 7.25), rng.random((3, 300))


@pytest.mark.parametrize("along", ["row", "column"])
def test_lknn_points_on_a_line(sa, along):
    t, c, m = _line()
    x, y = (t, c) if along == "row" else (c, t)
    _same(sa.c_LKNN(m, x, y, 5, 2.0, "euclidean", True, 0.0, False, 0), lr.lknn_brute(m, x, y, 5, 2.0, "euclidean", True, 0.0))


@pytest.mark.parametrize("along", ["row", "column"])
def test_spatial_graph_points_on_a_line(sa, along):
    t, c, _ = _line()
    x, y = (t, c) if along == "row" else (c, t)
    _same(sa.spatial_graph(x, y, 1.5, 100), sr.brute(x, y, 1.5, 100))
