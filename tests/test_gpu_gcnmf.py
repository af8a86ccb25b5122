"""Graph-convolutional NMF (c_gcnmf, src/singlet.cpp:1668-1730) on the GPU against the test-side restatement
(tests/gcnmf_restatement.py), its identity with c_nmf on the identity graph, where it differs from c_nmf, hubs, the graph's
lifetime on a context, refusals, config 3 at full size and the Python mirror of RunGCNMF."""
import os

import numpy as np
import pytest

import gcnmf_restatement as gr
from conftest import rel_fro, same_zero_pattern, to_dgc

pytestmark = pytest.mark.gpu
TOL = 1e-9
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check(got, ref, keys=("w", "h", "d")):
    """got: the c_gcnmf list (w m x k, h k x n); ref: the restatement's (cols, k) arrays"""
    for key in keys:
        g = got[key]
        if key == "h":
            g = g.T
        assert rel_fro(g, ref[key]) < TOL, (key, rel_fro(g, ref[key]))
        if g.ndim == 2:
            assert same_zero_pattern(g, ref[key]), key


def _graph(ora, kind, n):
    if kind == "lattice":
        side = int(round(np.sqrt(n)))
        assert side * side == n
        return gr.lattice_graph(ora, side)
    if kind == "directed":
        return gr.random_directed_graph(ora, n, 5, seed=11)
    return gr.sparse_odd_graph(ora, n, seed=12)


def _dg(sa, G):
    return to_dgc(sa, G)


@pytest.mark.parametrize("k,L1,L2,kind,maxit", [
    (1, 0.0, 0.0, "lattice", 4), (5, 0.01, 0.0, "directed", 4), (16, 0.01, 0.01, "odd", 4), (30, 0.01, 0.0, "lattice", 3),
    (50, 0.0, 0.0, "directed", 3), (64, 0.01, 0.0, "odd", 3), (100, 0.01, 0.0, "lattice", 3), (130, 0.01, 0.0, "directed", 3),
    (200, 0.01, 0.01, "odd", 3), (7, 0.0, 0.01, "lattice", 5)])
def test_c_gcnmf_parity(sa, ora, k, L1, L2, kind, maxit):
    m, n = 210, 324
    A = ora.synth_csc(m, n, 12)
    At = A.t()
    G = _graph(ora, kind, n)
    w0 = ora.synth_winit(k, m)
    ref = gr.c_gcnmf(ora, A, At, G, 0.0, maxit, L1, L2, w0)
    got = sa.c_gcnmf(to_dgc(sa, A), to_dgc(sa, At), _dg(sa, G), 0.0, maxit, False, L1, L2, 0, w0.T)
    assert got["w"].shape == (m, k) and got["h"].shape == (k, n)
    _check(got, ref)
    assert got["iter"] == ref["iter"] == maxit
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-7, atol=1e-14)


KNN_HUBS = (0, 200, 201, 323)   # the first and the last column, two adjacent ones


@pytest.mark.parametrize("k", [2, 4, 31, 63, 127, 258])
def test_c_gcnmf_parity_knn_graph_with_hubs(sa, ora, k):
    """Columns of kNN length (20 entries: five rounds of the convolution's four-deep loop) and four hubs of 129 (segments of
    64 + 64 + 1), at the widths test_c_gcnmf_parity leaves out: 16-byte loads with 1 and 2 lanes per column (k = 2, 4), single
    loads with 32 and 64 lanes and with two passes (k = 31, 63, 127), four passes (k = 258).  tests/test_gpu_graph_conv.py
    holds the convolution itself to the exact sum at these widths; this is the fit through it."""
    m, n, maxit, L1, L2 = 210, 324, 3, 0.01, 0.0
    A = ora.synth_csc(m, n, 12)
    At = A.t()
    G = gr.knn_hub_graph(ora, n, hubs=KNN_HUBS, hub_len=129)
    w0 = ora.synth_winit(k, m)
    ref = gr.c_gcnmf(ora, A, At, G, 0.0, maxit, L1, L2, w0)
    got = sa.c_gcnmf(to_dgc(sa, A), to_dgc(sa, At), _dg(sa, G), 0.0, maxit, False, L1, L2, 0, w0.T)
    assert got["w"].shape == (m, k) and got["h"].shape == (k, n)
    _check(got, ref)
    assert got["iter"] == ref["iter"] == maxit
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-7, atol=1e-14)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("m,n,k", [(700, 800, 513), (1200, 1100, 1024)])
def test_c_gcnmf_parity_high_rank(sa, ora, m, n, k):
    """c_gcnmf above 512, sized as tests/test_gpu_high_rank.py::test_c_nmf_parity_high_rank sizes c_nmf so that every factor
    stays alive: the convolution's 16-pass instance of single loads (k = 513) and its 8-pass instance of 16-byte loads
    (k = 1024), main pass and hub segments, two iterations (the second convolves a non-zero h on the W side too)."""
    A = ora.synth_csc(m, n, 20)
    At = A.t()
    G = gr.knn_hub_graph(ora, n, hubs=(0, n // 2, n // 2 + 1, n - 1), hub_len=129)
    w0 = ora.synth_winit(k, m)
    ref = gr.c_gcnmf(ora, A, At, G, 0.0, 2, 0.0, 0.0, w0, pairwise=False)
    d = np.asarray(ref["d"])
    assert d.min() > 1e-8 * d.max() and d.min() > 1e-10, d.min()   # a dead factor would make the case test nothing
    got = sa.c_gcnmf(to_dgc(sa, A), to_dgc(sa, At), _dg(sa, G), 0.0, 2, False, 0.0, 0.0, 0, w0.T)
    _check(got, ref)
    assert got["iter"] == ref["iter"] == 2
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-7, atol=1e-14)


def test_graph_orientation_matters(sa, ora):
    """G and G^T of an asymmetric graph give different fits, each equal to its own restatement."""
    m, n, k = 150, 256, 9
    A = ora.synth_csc(m, n, 10)
    G = gr.random_directed_graph(ora, n, 4, seed=5)
    Gt = gr.transpose_graph(ora, G)
    w0 = ora.synth_winit(k, m)
    got = [sa.c_gcnmf(to_dgc(sa, A), None, _dg(sa, g), 0.0, 3, False, 0.01, 0.0, 0, w0) for g in (G, Gt)]   # w0 is m x k here
    ref = [gr.c_gcnmf(ora, A, A.t(), g, 0.0, 3, 0.01, 0.0, w0) for g in (G, Gt)]
    _check(got[0], ref[0])
    _check(got[1], ref[1])
    assert rel_fro(got[0]["h"], got[1]["h"]) > 1e-3


def _full_matrix(ora, m, n, inv_density):
    """synthetic matrix without empty rows or columns"""
    import scipy.sparse as sp
    A = ora.synth_csc(m, n, inv_density)
    S = sp.csc_matrix((A.x, A.i, A.p), shape=(m, n)).tolil()
    S[np.arange(m), np.arange(m) % n] = 1.0
    S[np.arange(n) % m, np.arange(n)] = 1.0
    S = S.tocsc()
    S.sort_indices()
    return ora.CSC(S.data, S.indices, S.indptr, m, n)


@pytest.mark.parametrize("plain_acc", [True, False])
@pytest.mark.parametrize("k", [6, 50, 130])
def test_identity_graph_is_bit_equal_to_c_nmf(sa, ora, monkeypatch, plain_acc, k):
    """1.0 * x + 0 is exact and every column is non-empty: c_gcnmf on the identity graph IS c_nmf (L1_w = L1_h), bit for
    bit, through the plain CSC accumulate and through the LDS-tiled one."""
    if plain_acc:
        monkeypatch.setenv("SGL_NO_TILED", "1")
    A = _full_matrix(ora, 400, 700, 15)
    assert np.all(np.diff(A.p) > 0) and np.all(np.diff(A.t().p) > 0)
    w0 = ora.synth_winit(k, A.nrow)
    I = gr.identity_graph(ora, A.ncol)
    a = sa.c_nmf(to_dgc(sa, A), None, 0.0, 4, False, 0.01, 0.01, 0.0, 0.0, 0, w0.T)
    g = sa.c_gcnmf(to_dgc(sa, A), None, _dg(sa, I), 0.0, 4, False, 0.01, 0.0, 0, w0.T)
    assert np.array_equal(a["w"].T, g["w"]) and np.array_equal(a["h"], g["h"]) and np.array_equal(a["d"], g["d"])
    assert np.array_equal(a["tol"], g["tol"])


@pytest.mark.parametrize("plain_acc", [True, False])
def test_empty_cell_and_empty_gene_are_solved(sa, ora, monkeypatch, plain_acc):
    """An empty cell column with non-empty neighbours gets a non-zero h (its right-hand side is its neighbours'); an
    empty gene is solved too (c_nmf would leave its warm start in place)."""
    if plain_acc:
        monkeypatch.setenv("SGL_NO_TILED", "1")
    import scipy.sparse as sp
    m, n, k = 160, 289, 8
    A = ora.synth_csc(m, n, 8)
    S = sp.csc_matrix((A.x, A.i, A.p), shape=(m, n)).tolil()
    S[:, 20] = 0.0
    S[7, :] = 0.0
    S = S.tocsc()
    S.eliminate_zeros()
    S.sort_indices()
    A = ora.CSC(S.data, S.indices, S.indptr, m, n)
    assert A.p[21] == A.p[20] and 7 not in A.i
    G = gr.lattice_graph(ora, 17)
    w0 = ora.synth_winit(k, m)
    ref = gr.c_gcnmf(ora, A, A.t(), G, 0.0, 3, 0.01, 0.0, w0)
    got = sa.c_gcnmf(to_dgc(sa, A), None, _dg(sa, G), 0.0, 3, False, 0.01, 0.0, 0, w0.T)
    _check(got, ref)
    assert np.any(got["h"][:, 20] > 0)
    plain = sa.c_nmf(to_dgc(sa, A), None, 0.0, 3, False, 0.01, 0.01, 0.0, 0.0, 0, w0.T)
    assert rel_fro(got["w"][7], ref["w"][7]) < TOL
    # b = 0 and L1 > 0 drive the solved gene to exactly 0; c_nmf skips it, so its warm start stays (scaled)
    assert np.all(got["w"][7] == 0) and np.all(ref["w"][7] == 0) and np.all(plain["w"].T[7] > 0)


def test_hub_column(sa, ora):
    """One column with 20 000 entries among columns of 0 - 3: the segment pass sums it; equal to the restatement.  The
    rhs_h phase (accumulate + convolution) with and without the hub is printed."""
    m, n, k = 60, 25000, 10
    A = ora.synth_csc(m, n, 10)
    G = gr.hub_graph(ora, n, hub=12345, hub_len=20000, seed=9)
    assert np.diff(G.p).max() == 20000 and np.sort(np.diff(G.p))[-2] <= 3
    w0 = ora.synth_winit(k, m)
    ref = gr.c_gcnmf(ora, A, A.t(), G, 0.0, 2, 0.01, 0.0, w0, pairwise=False)
    got = sa.c_gcnmf(to_dgc(sa, A), None, _dg(sa, G), 0.0, 2, False, 0.01, 0.0, 0, w0.T)
    _check(got, ref)
    # the same graph without the hub's entries
    keep = np.ones(G.nnz, dtype=bool)
    keep[G.p[12345]:G.p[12346]] = False
    cnt = np.diff(G.p).copy()
    cnt[12345] = 0
    G0 = ora.CSC(G.x[keep], G.i[keep], np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), n, n)
    times = {}
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        for name, g in (("hub", G), ("no_hub", G0)):
            c.fit_init(k, w0)
            c.set_graph(_dg(sa, g))
            c.timing_enable(True)
            c.nmf_run(0.0, 5, 0.01, 0.01, 0.0, 0.0)
            t = c.timing_get(reset=True)
            c.timing_enable(False)
            times[name] = t["rhs_h"][0] / max(t["rhs_h"][1], 1)
    print("\nrhs_h per call (accumulate + convolution), n = 25 000, k = 10: with a 20 000-entry hub %.4f ms, without %.4f ms"
          % (times["hub"], times["no_hub"]))


def test_graph_does_not_leak(sa, ora):
    m, n, k = 180, 256, 7
    A = ora.synth_csc(m, n, 10)
    G = gr.lattice_graph(ora, 16)
    w0 = ora.synth_winit(k, m)
    with sa.Context(0) as fresh:
        fresh.upload(to_dgc(sa, A))
        fresh.fit_init(k, w0)
        fresh.nmf_run(0.0, 3, 0.01, 0.01, 0.0, 0.0)
        base = fresh.get_factors()
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        c.fit_init(k, w0)
        c.set_graph(_dg(sa, G))
        c.nmf_run(0.0, 3, 0.01, 0.01, 0.0, 0.0)
        with_graph = c.get_factors()
        assert not np.array_equal(with_graph[2], base[2])
        c.fit_init(k, w0)          # drops the graph
        c.nmf_run(0.0, 3, 0.01, 0.01, 0.0, 0.0)
        after = c.get_factors()
        c.fit_init(k, w0)
        c.set_graph(_dg(sa, G))
        c.set_graph(None)          # clears it
        c.nmf_run(0.0, 3, 0.01, 0.01, 0.0, 0.0)
        cleared = c.get_factors()
    for x in (after, cleared):
        assert all(np.array_equal(u, v) for u, v in zip(x, base))


def test_refusals_leave_the_context_usable(sa, ora):
    m, n, k = 120, 196, 5
    A = ora.synth_csc(m, n, 10)
    G = gr.lattice_graph(ora, 14)
    w0 = ora.synth_winit(k, m)
    Err = sa.SingletHipError

    def refused(fn, words):
        with pytest.raises(Err) as e:
            fn()
        assert words in str(e.value), str(e.value)

    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        c.fit_init(k, w0)
        # wrong shape, unsorted rows, NaN
        refused(lambda: c.set_graph(_dg(sa, gr.lattice_graph(ora, 13))), "n x n")
        bad = _dg(sa, G)
        xi = bad.i.copy()
        xi[[0, 1]] = xi[[1, 0]]
        refused(lambda: c.set_graph(sa.dgCMatrix(bad.x, xi, bad.p, bad.Dim)), "ascending")
        xx = bad.x.copy()
        xx[5] = np.nan
        refused(lambda: c.set_graph(sa.dgCMatrix(xx, bad.i, bad.p, bad.Dim)), "non-finite")
        # all-reduce hook, either order
        c.set_allreduce(lambda p, cnt: None)
        refused(lambda: c.set_graph(_dg(sa, G)), "all-reduce")
        c.set_allreduce(None)
        c.set_graph(_dg(sa, G))
        refused(lambda: c.set_allreduce(lambda p, cnt: None), "graph")
        # masked (ARD) steps
        refused(lambda: c.step_h_masked(0.01, 0.0, 7, 10), "graph")
        refused(lambda: c.ard_run(0.0, 2, 0.01, 0.0, 7, 10, 0.05, 1), "graph")
        # links plus graph, either order
        refused(lambda: _set_links(sa, c, np.ones((2, n))), "graph")
        c.set_graph(None)
        _set_links(sa, c, np.ones((2, n)))
        refused(lambda: c.set_graph(_dg(sa, G)), "link")
        # still usable: a GCNMF fit on the same context equals the one-shot call
        c.fit_init(k, w0)
        c.set_graph(_dg(sa, G))
        c.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        W, d, H = c.get_factors()
    one = sa.c_gcnmf(to_dgc(sa, A), None, _dg(sa, G), 0.0, 2, False, 0.01, 0.0, 0, w0.T)
    assert np.array_equal(one["w"], W) and np.array_equal(one["h"], H.T) and np.array_equal(one["d"], d)
    # dense upload
    with sa.Context(0) as c:
        c.upload_dense(A.to_dense())
        c.fit_init(k, w0)
        refused(lambda: c.set_graph(_dg(sa, G)), "dense")
        c.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)
    # a team (ranks sharing device 0, as the config-4 team tests build it)
    with sa.Multi([0, 0]) as M:
        M.upload(to_dgc(sa, A))
        M.fit_init(k, w0)
        refused(lambda: M.rank_ctx(0).set_graph(_dg(sa, G)), "team")
        M.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)


def _set_links(sa, c, link_h):
    from singlet_amd._lib import check, f64p, ptr
    buf = np.ascontiguousarray(np.asarray(link_h, dtype=np.float64).T)
    check(c._L.sgl_set_links(c._h, ptr(buf, f64p), link_h.shape[0], link_h.shape[1], None, 0, 0))


@pytest.mark.timeout(1200)
def test_config3_full_size_one_iteration(sa, ora):
    """Config 3 (30 000 genes x 1 000 000 cells, k = 50) on the 1000 x 1000 lattice: one GCNMF iteration through the step
    API.  h of cell slices at the first, middle and last cells (straddling lattice rows) against the restatement of the
    H update (their columns and their neighbours' regenerated by ora.synth_csc(cell0=)); w of the heaviest and the
    lightest gene against the restatement of the W update fed the GPU's scaled H."""
    import scipy.sparse as sp
    genes, side, k, L1 = 30000, 1000, 50, 0.01
    cells = side * side
    G = gr.lattice_graph(ora, side)
    w0 = ora.synth_winit(k, genes)
    with sa.Context(0) as c:
        c.synth(genes, cells, 20)
        c.fit_init(k, w0)
        c.set_graph(_dg(sa, G))
        c.step_begin()
        c.step_h(L1, 0.0)
        _, _, H_unscaled = c.get_factors(w=False, d=False)
        c.step_scale_h()
        _, _, Hs = c.get_factors(w=False, d=False)
        c.step_w(L1, 0.0)
        W_unscaled, _, _ = c.get_factors(d=False, h=False)
        gene_nnz = c.col_counts(1)
    a = ora.aat(w0)
    for s0, s1 in ((0, 1500), (cells // 2 - 700, cells // 2 + 800), (cells - 1500, cells)):
        lo, hi = max(0, s0 - side - 1), min(cells, s1 + side + 1)
        B = ora.rhs(ora.synth_csc(genes, hi - lo, 20, cell0=lo), w0)
        ref = np.zeros((s1 - s0, k))
        for o, j in enumerate(range(s0, s1)):
            b = np.zeros(k)
            for q in range(G.p[j], G.p[j + 1]):
                b += G.x[q] * B[G.i[q] - lo]
            ref[o] = ora.nnls(a, b, np.zeros(k), L1, 0.0)[0]
        got = H_unscaled[s0:s1]
        assert rel_fro(got, ref) < TOL and same_zero_pattern(got, ref), (s0, rel_fro(got, ref))
    S = sp.csc_matrix((G.x, G.i, G.p), shape=(cells, cells))
    Hc = np.asarray(S.T @ Hs)          # (H G)(:, c) = sum_r G(r, c) H(:, r)
    ah = ora.aat(Hs)
    for g in (int(np.argmax(gene_nnz)), int(np.argmin(gene_nnz))):
        col = ora.synth_gene_columns([g], cells, 20)
        b = np.zeros(k)
        for q in range(col.p[0], col.p[1]):
            b += col.x[q] * Hc[col.i[q]]
        ref = ora.nnls(ah, b, w0[g], L1, 0.0)[0]
        assert rel_fro(W_unscaled[g], ref) < TOL and same_zero_pattern(W_unscaled[g], ref), g


def _pbmc3k(sa):
    g = np.load(os.path.join(GOLD, "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)
    for c in range(dim[1]):
        s, e = p[c], p[c + 1]
        i[s:e] = np.cumsum(i[s:e])
    return sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (dim[0], dim[1]))


def _knn_graph(sa, X, nn):
    """kNN over the rows of X (cells), column c = its nn nearest other cells with weight 1 / nn"""
    sq = (X * X).sum(1)
    D = sq[:, None] + sq[None, :] - 2 * X @ X.T
    np.fill_diagonal(D, np.inf)
    nbr = np.sort(np.argsort(D, axis=1)[:, :nn], axis=1)
    n = X.shape[0]
    p = np.arange(n + 1, dtype=np.int32) * nn
    return sa.dgCMatrix(np.full(n * nn, 1.0 / nn), nbr.reshape(-1).astype(np.int32), p, (n, n))


def test_run_gcnmf_pbmc3k(sa):
    counts = _pbmc3k(sa)
    norm = sa.PreprocessData(counts)
    Xc = norm.to_scipy().T.tocsr()
    proj = np.random.default_rng(0).standard_normal((counts.nrow, 20))
    G = _knn_graph(sa, np.asarray(Xc @ proj), 10)
    k = 10
    model = sa.run_gcnmf(counts, G, k, maxit=4, verbose=0, seed=3)
    assert model["w"].shape == (counts.nrow, k) and model["h"].shape == (k, counts.ncol) and model["d"].shape == (k,)
    assert model["factor_names"] == ["GCNMF_%d" % q for q in range(1, k + 1)]
    w_init = np.random.default_rng(3).random((counts.nrow, k)).T
    direct = sa.c_gcnmf(norm, None, G, 1e-5, 4, False, 0.01, 0.0, 0, w_init)
    assert np.array_equal(model["d"], direct["d"]) and np.array_equal(model["w"], direct["w"])
    assert np.array_equal(model["h"], direct["h"])
    assert np.all(np.isfinite(model["h"])) and np.any(model["h"] > 0)
