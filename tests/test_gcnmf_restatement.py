"""The test-side restatement of c_gcnmf (tests/gcnmf_restatement.py) checked on the CPU: it reduces to the oracle's c_nmf
on the identity graph, and it reproduces a case worked by hand."""
import numpy as np
import pytest

import gcnmf_restatement as gr


def _full_matrix(ora, m, n, inv_density):
    """synthetic matrix without empty rows or columns (so that c_nmf's empty-column skips never apply)"""
    A = ora.synth_csc(m, n, inv_density)
    D = A.to_dense()
    D[np.arange(m), np.arange(m) % n] += 1.0
    D[np.arange(n) % m, np.arange(n)] += 1.0
    import scipy.sparse as sp
    S = sp.csc_matrix(D)
    S.sort_indices()
    return ora.CSC(S.data, S.indices, S.indptr, m, n)


@pytest.mark.parametrize("k,L1,L2", [(1, 0.0, 0.0), (5, 0.01, 0.0), (12, 0.01, 0.01)])
def test_identity_graph_is_c_nmf(ora, k, L1, L2):
    A = _full_matrix(ora, 40, 55, 6)
    At = A.t()
    assert np.all(np.diff(A.p) > 0) and np.all(np.diff(At.p) > 0)
    w0 = ora.synth_winit(k, A.nrow)
    ref = ora.c_nmf(A, At, 0.0, 4, L1, L1, L2, L2, 0, w0)
    got = gr.c_gcnmf(ora, A, At, gr.identity_graph(ora, A.ncol), 0.0, 4, L1, L2, w0)
    for key in ("w", "h", "d"):
        assert np.abs(got[key] - ref[key]).max() <= 1e-13 * max(np.abs(ref[key]).max(), 1.0), key
    assert got["iter"] == ref["iter"] == 4


def test_pairwise_w_side_equals_rhs_of_convolved_h(ora):
    """The two forms of the W-side right-hand sides (l.1703-1706 pair by pair; rhs(At, H G)) agree."""
    A = ora.synth_csc(30, 45, 5)
    G = gr.random_directed_graph(ora, A.ncol, 4, seed=3)
    w0 = ora.synth_winit(6, A.nrow)
    a = gr.c_gcnmf(ora, A, A.t(), G, 0.0, 3, 0.01, 0.0, w0, pairwise=True)
    b = gr.c_gcnmf(ora, A, A.t(), G, 0.0, 3, 0.01, 0.0, w0, pairwise=False)
    for key in ("w", "h", "d"):
        assert np.allclose(a[key], b[key], rtol=1e-12, atol=1e-15), key


def test_hand_worked_three_cells_two_genes(ora):
    """A = [[1, 0, 2], [0, 3, 0]], G(r, c) = [[1, .5, 0], [0, 1, 0], [.5, 0, 1]] (asymmetric), k = 1, w = (1, 2),
    one iteration without penalties.  By hand:
      H side: a = 1 + 4 = 5, B = (1, 6, 2), Bc = B G = (1 + .5 * 2, .5 * 1 + 6, 2) = (2, 6.5, 2), h = Bc / 5 = (.4, 1.3, .4);
              scale: d = 2.1, h = (4, 13, 4) / 21.
      W side: H G = (4 + 2, 2 + 13, 4) / 21, b = (1 * 6 + 2 * 4, 3 * 15) / 21 = (14, 45) / 21, a = (16 + 169 + 16) / 441,
              nnls starts from the current w and adds b / a to it (the reference's nnls takes b as the right-hand side,
              not a residual): w = (1, 2) + (294, 945) / 201 = (495, 1347) / 201; scale: d = 1842 / 201,
              w = (495, 1347) / 1842."""
    A = ora.CSC([1.0, 3.0, 2.0], [0, 1, 0], [0, 1, 2, 3], 2, 3)
    G = ora.CSC([1.0, 0.5, 0.5, 1.0, 1.0], [0, 2, 0, 1, 2], [0, 2, 4, 5], 3, 3)
    got = gr.c_gcnmf(ora, A, A.t(), G, 0.0, 1, 0.0, 0.0, np.array([[1.0], [2.0]]))
    assert np.allclose(got["h"][:, 0], np.array([4.0, 13.0, 4.0]) / 21, rtol=1e-12, atol=0)
    assert np.allclose(got["w"][:, 0], np.array([495.0, 1347.0]) / 1842, rtol=1e-12, atol=0)
    assert np.allclose(got["d"], [1842.0 / 201], rtol=1e-12, atol=0)
    # the orientation matters: with G^T the H side reads Bc = (1 + .5 * 6, 6, .5 * 1 + 2) -- a different h
    other = gr.c_gcnmf(ora, A, A.t(), gr.transpose_graph(ora, G), 0.0, 1, 0.0, 0.0, np.array([[1.0], [2.0]]))
    assert not np.allclose(other["h"], got["h"])


def test_lattice_graph_shape(ora):
    G = gr.lattice_graph(ora, 4)
    assert G.nrow == G.ncol == 16
    assert G.nnz == 4 * 4 + 8 * 6 + 4 * 9   # corners, edges, interior
    cols = np.repeat(np.arange(16), np.diff(G.p))
    assert np.allclose(np.bincount(cols, weights=G.x), 1.0)
    for c in range(16):   # rows ascending within each column, self-loop present
        r = G.i[G.p[c]:G.p[c + 1]]
        assert np.all(np.diff(r) > 0) and c in r


def test_edge_length_graph_shape(ora):
    """what tests/test_gpu_graph_conv.py relies on: the lengths and overrides, sorted distinct rows, self-loops for single
    entries, rows 0 and n - 1, weights of whole eighths of both signs, 173 columns for the main pass and 147 hubs -- and
    that its exact test is exact: at k = 3 and k = 1024 the sequential float64 sum equals the int64 sum, below 2^31."""
    n = 320
    G = gr.edge_length_graph(ora, n)
    lens = np.diff(G.p)
    assert G.nrow == G.ncol == n and lens[0] == 129 and lens[n - 1] == n and lens[100] == 192 and lens[101] == 193
    assert set(gr.EDGE_LENGTHS) <= set(lens.tolist())
    assert (lens > 128).sum() == 147 and (lens <= 128).sum() == 173
    for c in range(n):
        r = G.i[G.p[c]:G.p[c + 1]]
        assert np.all(np.diff(r) > 0) and (lens[c] != 1 or r[0] == c)
    assert G.i.min() == 0 and G.i.max() == n - 1
    w8 = G.x * 8
    assert np.array_equal(w8, np.rint(w8)) and np.abs(w8).max() == 15 and np.abs(w8).min() == 1 and w8.min() < 0 < w8.max()
    N2 = gr.edge_length_graph(ora, n, weights=np.random.default_rng(29).standard_normal)
    assert np.array_equal(N2.p, G.p) and np.array_equal(N2.i, G.i) and not np.array_equal(N2.x, G.x)
    for k in (3, 1024):
        X = 1024.0 * np.arange(n)[:, None] + np.arange(k)[None, :] + 1.0
        ref8 = np.zeros((n, k), dtype=np.int64)
        for c in range(n):
            s = slice(G.p[c], G.p[c + 1])
            ref8[c] = (w8[s, None].astype(np.int64) * X[G.i[s]].astype(np.int64)).sum(axis=0)
        assert np.abs(ref8).max() < 2 ** 31
        assert np.array_equal(gr.convolve(G, X) * 8, ref8)


def test_knn_hub_graph_shape(ora):
    G = gr.knn_hub_graph(ora, 324, hubs=(0, 200, 201, 323), hub_len=129)
    lens = np.diff(G.p)
    assert np.array_equal(np.nonzero(lens != 20)[0], [0, 200, 201, 323]) and np.all(lens[[0, 200, 201, 323]] == 129)
    for c in range(324):
        assert np.all(np.diff(G.i[G.p[c]:G.p[c + 1]]) > 0)
    assert G.x.min() >= 0.1 and G.x.max() <= 1.0
