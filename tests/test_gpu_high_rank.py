"""Ranks above 128 up to the library's limit (SGL_MAX_K = 1024) against the CPU oracle, on every path: the operators
one by one, the one-shot entry points, and teams on one device.  The ranks sit at the edges where the generic
any-rank code changes shape:

  * 129, 256 / 257     -- leaving the MFMA kernels, the four-columns-per-wave solves, the 129 - 256 Gram
  * 375 / 376 / 377    -- mask_gram_kernel<33>'s dynamic LDS (1056 + 128 k bytes) crosses 48 KB at k = 376
  * 384 / 385          -- gram_valu_kernel's LDS (128 k bytes) crosses 48 KB after k = 384
  * 512 / 513          -- nnls_wave_kernel<8> -> <16>; 9 launches of the VALU Gram and more
  * 639 / 640 / 641    -- the wave solve's tenth and eleventh register rows (64 coordinates per row)
  * 1023 / 1024        -- the limit: 16 register rows, 16 Gram launches, 32 tiled passes of the masked right-hand sides

Same assertions and tolerances as the tests of the lower ranks (test_gpu_ops.py, test_gpu_nmf.py,
test_gpu_native_team.py); nothing is loosened for the high ranks."""
import numpy as np
import pytest

from conftest import rel_fro, same_zero_pattern, to_dgc

pytestmark = pytest.mark.gpu
TOL = 1e-9   # as test_gpu_nmf.py

EDGES = [129, 200, 256, 257, 300, 375, 376, 377, 384, 385, 512, 513, 639, 640, 641, 768, 1000, 1023, 1024]


def _check(got, ref, keys=("w", "h", "d")):
    for key in keys:
        g = got[key].T if got[key].ndim == 2 else got[key]
        assert rel_fro(g, ref[key]) < TOL, key
        if g.ndim == 2:
            assert same_zero_pattern(g, ref[key]), key


def _alive(d):
    """every factor of the oracle's fit alive: a dead one (d at the 1e-15 ridge) would make the case test nothing"""
    d = np.asarray(d)
    assert d.min() > 1e-8 * d.max() and d.min() > 1e-10, d.min()


def _mask_gram_oracle(ora, F, G, ncols, seed, inv_density, mask_t, col_off, row_off):
    """G - (AAt(F[idx_c]) + 1e-15 I) per column (src/singlet.cpp:458-463), idx_c from the oracle's mask; G None: the raw sum
    (as test_gpu_ops.py)."""
    nrow, k = F.shape
    if mask_t == 0:   # columns are cells, rows genes
        M = ora.rng_mask(seed, col_off, ncols, nrow + row_off, inv_density)[:, row_off:]
    else:             # columns are genes, rows cells
        M = ora.rng_mask(seed, row_off, nrow, ncols + col_off, inv_density)[:, col_off:].T
    out = np.empty((ncols, k, k))
    for c in range(ncols):
        Fs = F[M[c].astype(bool)]
        S = Fs.T @ Fs
        out[c] = S if G is None else G - (S + 1e-15 * np.eye(k))
    return out


# ------------------------------------------------------------------------------------------------------------ operators --

@pytest.mark.parametrize("cols", [90, 8193])
@pytest.mark.parametrize("k", EDGES)
def test_gram_high_rank(ctx, ora, k, cols):
    """VALU Gram (k > 256) in one to sixteen launches of 65 536 pairs, 16 k doubles of LDS per block (above 48 KB from
    k = 385); 8193 columns are 33 blocks: the partials span two 32-block segments of the fixed-order sum."""
    F = np.random.default_rng(k * 1000 + cols).random((cols, k))
    G = ctx.op_gram(F)
    E = ora.aat(F)
    assert rel_fro(G, E) < 1e-13
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("k,cols", [(16, 278523), (64, 278523), (65, 278523), (128, 278523), (129, 139259), (256, 139259)])
def test_gram_many_partial_blocks(ctx, ora, k, cols):
    """Column counts that reach the block caps of k_gram: 1024 blocks of 272 columns up to k = 128 (32 segments of the
    partial sum), 512 blocks on the 129 - 256 matrix-core kernel (16 segments); the last block is short."""
    F = np.random.default_rng(k * 7 + 1).random((cols, k))
    G = ctx.op_gram(F)
    E = ora.aat(F)
    assert rel_fro(G, E) < 1e-13
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("k", [257, 384, 511, 512, 513, 639, 640, 641, 768, 1023, 1024])
@pytest.mark.parametrize("L1,L2", [(0.0, 0.0), (0.01, 0.0), (0.01, 0.05)])
def test_nnls_high_rank(ctx, ora, k, L1, L2):
    """Shared-Gram solve above 256: one wave per column, nnls_wave_kernel<8> up to k = 512 and <16> above (coordinates
    64 r .. 64 r + 63 in register row r: rows 10 - 15 from k = 641); 96 columns are 24 workgroups of four waves."""
    rng = np.random.default_rng(k)
    ncols = 96
    F = rng.random((4 * k + 5, k))
    G = ora.aat(F)
    B = rng.normal(size=(ncols, k)) * 3 + 1.0
    X0 = np.abs(rng.normal(size=(ncols, k))) * (rng.random((ncols, k)) < 0.6) * 1e-3
    X, sweeps = ctx.op_nnls(G, B, X0, L1, L2)
    E = np.empty_like(X0)
    esw = 0
    for c in range(ncols):
        E[c], _, it = ora.nnls(G, B[c], X0[c], L1, L2)
        esw += it
    assert rel_fro(X, E) < 1e-10
    assert np.array_equal(X == 0, E == 0)
    assert sweeps == esw


@pytest.mark.parametrize("k", [513, 1024])
def test_rhs_high_rank_plain_and_tiled(ctx, ora, sa, k):
    """Right-hand sides at k = 513 / 1024 by the plain CSC kernel (which = 0 / 1) and the LDS-tiled one (2 / 3, factor parts
    of tiled_part_size rows), both orientations."""
    A = ora.synth_csc(700, 900, 12)
    At = A.t()
    ctx.upload(to_dgc(sa, A), to_dgc(sa, At))
    rng = np.random.default_rng(k)
    W = rng.random((A.nrow, k))
    H = rng.random((A.ncol, k))
    for which, F, M in ((0, W, A), (1, H, At), (2, W, A), (3, H, At)):
        assert rel_fro(ctx.op_rhs(which, F), ora.rhs(M, F)) < 1e-14, which


@pytest.mark.parametrize("k", [129, 200, 256, 257, 375, 376, 377, 512, 513, 1024])
@pytest.mark.parametrize("use_lists", [False, True])
def test_mask_gram_downdate_high_rank(ctx, ora, k, use_lists):
    """Per-column Gram downdates above 128 (mask_gram_kernel<20> / <33>, one launch per 8448 pairs of the triangle; the dynamic
    LDS crosses 48 KB at k = 376): the five settings of test_mask_gram_downdate -- both orientations with offsets, raw sums,
    every row drawn, almost none."""
    rng = np.random.default_rng(500 + k)
    nrow, ncols = 1500, 7
    F = rng.random((nrow, k)) + 0.1
    G = ora.aat(rng.random((3 * k + 2, k)))
    for mask_t, inv, co, ro, raw in ((0, 5, 11, 0, False), (1, 4, 0, 23, False), (0, 3, 5, 0, True), (1, 1, 0, 0, False), (0, 700, 3, 0, False)):
        got = ctx.op_mask_gram(F, None if raw else G, ncols, 77, inv, mask_t, co, ro, use_lists)
        exp = _mask_gram_oracle(ora, F, None if raw else G, ncols, 77, inv, mask_t, co, ro)
        scale = np.abs(exp).max() + 1.0
        assert np.abs(got - exp).max() / scale < 1e-12, (mask_t, inv, raw)
        assert np.array_equal(got, got.transpose(0, 2, 1))


@pytest.mark.parametrize("k", [129, 256, 257, 512, 513, 1024])
@pytest.mark.parametrize("use_lists", [True, False])
def test_mse_test_op_high_rank(sa, ora, k, use_lists, monkeypatch):
    """sgl_op_mse_test above 128 (mse_test_kernel<4>, and <16> above 256: up to 16 register rows), one shard and two shards
    with a cell offset, as test_mse_test_op."""
    if not use_lists:
        monkeypatch.setenv("SGL_MSE_NO_LIST", "1")
        monkeypatch.setenv("SGL_MASK_NO_LIST", "1")
    m, n, seed, inv = 333, 517, 99, 7
    A = ora.synth_csc(m, n, 9)
    rng = np.random.default_rng(k)
    W = np.abs(rng.standard_normal((m, k)))
    H = np.abs(rng.standard_normal((n, k))) * (rng.random((n, k)) < 0.8)
    d = 0.5 + rng.random(k)
    exp = ora.mse_test(A, W, d, H, seed, inv)

    def shard(lo, hi):
        sub = ora.CSC(A.x[A.p[lo]:A.p[hi]], A.i[A.p[lo]:A.p[hi]], A.p[lo:hi + 1] - A.p[lo], m, hi - lo)
        c = sa.Context(0)
        try:
            c.upload(to_dgc(sa, sub), None, cell_offset=lo, ncells_total=n)
            c.fit_init(k, W)
            c.set_factors(W, d, H[lo:hi])
            return c.op_mse_test(seed, inv)
        finally:
            c.close()

    one = shard(0, n)
    assert abs(one - exp) <= 1e-11 * abs(exp), (one, exp)
    two = shard(0, 200) + shard(200, n)
    assert abs(two - exp) <= 1e-11 * abs(exp), (two, exp)


@pytest.mark.parametrize("k,cols", [(k, c) for k in (1, 17, 64, 65, 128, 257, 1024) for c in (1234, 20000, 200000) if k * c <= 52_000_000])
def test_scale_high_rank(ctx, ora, k, cols):
    """scale(): row sums in 64-row passes (k_rowsum), the one-launch partial sum with the ridge inside while k x segments <= 1024,
    the two-stage sum + add_eps_kernel above (20 000 columns: 2 segments, so k = 1024; 200 000 columns: 13, so k >= 79).
    1e-14 to the exactly rounded sums (math.fsum); to the oracle 1e-14 plus the oracle's own distance from them -- its
    left-to-right sum of 200 000 terms is itself ~1.4e-14 off, so the oracle alone cannot hold a kernel to 1e-14 there."""
    import math
    F = np.random.default_rng(k * 31 + cols).random((cols, k))
    S, d = ctx.op_scale(F)
    ES, ed = ora.scale(F)
    Ft = np.ascontiguousarray(F.T)
    d_exact = np.array([math.fsum(r) for r in Ft]) + 1e-15
    S_exact = F / d_exact
    assert rel_fro(d, d_exact) < 1e-14 and rel_fro(S, S_exact) < 1e-14
    assert rel_fro(d, ed) < 1e-14 + rel_fro(ed, d_exact) and rel_fro(S, ES) < 1e-14 + rel_fro(ES, S_exact)


# ------------------------------------------------------------------------------------------------- one-shot entry points --

@pytest.mark.timeout(900)
@pytest.mark.parametrize("m,n,k", [(700, 800, 513), (1200, 1100, 1024)])
def test_c_nmf_parity_high_rank(sa, ora, m, n, k):
    """c_nmf above 512: VALU Gram in 5 / 16 launches, the wave solve's <16> instance, plain CSC right-hand sides."""
    A = ora.synth_csc(m, n, 20)
    At = A.t()
    w0 = ora.synth_winit(k, m)
    ref = ora.c_nmf(A, At, 0.0, 1, 0.0, 0.0, 0.0, 0.0, 0, w0)
    _alive(ref["d"])
    got = sa.c_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 1, False, 0.0, 0.0, 0.0, 0.0, 0, w0.T)
    _check(got, ref)
    assert got["iter"] == ref["iter"] == 1
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-8, atol=0)


def _ard_case(ora, k):
    # enough data for every factor to stay alive: at k = 1024 a factor's few non-zero cells of h must not all be masked for a
    # gene, or its per-gene Gram has a zero diagonal (NaN in the oracle as in the reference)
    m, n = (900, 1000) if k <= 400 else (1200, 1300) if k <= 600 else (1100, 3000)
    A = ora.synth_csc(m, n, 20)
    return A, A.t(), ora.synth_winit(k, m)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [300, 384, 513, 1024])
def test_c_ard_nmf_parity_high_rank(sa, ora, k):
    """Masked fit above 256: per-column Gram downdates by mask_gram_kernel<33> (above 48 KB of LDS from k = 376), the wave solve
    on per-column Grams (gstride != 0), masked right-hand sides in passes of the factor rows, mse_test_kernel<16>."""
    A, At, w0 = _ard_case(ora, k)
    ref = ora.c_ard_nmf(A, At, 0.0, 1, 0.01, 0.0, 0, w0, 77, 20, 1e-3, 1)
    _alive(ref["d"])
    got = sa.c_ard_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 1, False, 0.01, 0.0, 0, w0.T, 77, 20, 1e-3, 1)
    _check(got, ref)
    assert np.array_equal(got["iter"], ref["iter"])
    assert np.allclose(got["test_mse"], ref["test_mse"], rtol=1e-9, atol=0)
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-7, atol=0)
    assert np.allclose(got["score_overfit"], ref["score_overfit"], rtol=1e-6, atol=1e-12)


@pytest.mark.timeout(900)
def test_c_ard_nmf_high_rank_gram_chunks_are_bit_identical(sa, ora, monkeypatch):
    """The per-column Grams of the masked fit in chunks of 256 columns (SGL_GCOLS_MB=1: 4 chunks of the 1000 cells and of
    the 900 genes at k = 384) against one chunk: the same bits, and the oracle's fit."""
    k = 384
    A, At, w0 = _ard_case(ora, k)
    dA, dAt = to_dgc(sa, A), to_dgc(sa, At)
    monkeypatch.delenv("SGL_GCOLS_MB", raising=False)
    whole = sa.c_ard_nmf(dA, dAt, 0.0, 1, False, 0.01, 0.0, 0, w0.T, 77, 20, 1e-3, 1)
    monkeypatch.setenv("SGL_GCOLS_MB", "1")
    chunked = sa.c_ard_nmf(dA, dAt, 0.0, 1, False, 0.01, 0.0, 0, w0.T, 77, 20, 1e-3, 1)
    for key in ("w", "d", "h", "test_mse", "tol", "iter", "score_overfit"):
        assert np.array_equal(np.asarray(chunked[key]), np.asarray(whole[key])), key
    ref = ora.c_ard_nmf(A, At, 0.0, 1, 0.01, 0.0, 0, w0, 77, 20, 1e-3, 1)
    _check(chunked, ref)


@pytest.mark.parametrize("k", [257, 1024])
@pytest.mark.parametrize("orient", ["m_by_k", "k_by_m"])
def test_c_project_model_high_rank(sa, ora, orient, k):
    A = ora.synth_csc(1100, 2000, 20)     # (410 cells leave a factor of k = 1024 without a non-zero)
    w = np.random.default_rng(1).random((1100, k))
    win = w if orient == "m_by_k" else w.T.copy()
    ref = ora.c_project_model(A, win, 0.01, 0.0)
    _alive(ref["d"])
    got = sa.c_project_model(to_dgc(sa, A), win, 0.01, 0.0, 0)
    _check(got, ref, ("h", "d"))


@pytest.mark.parametrize("k", [257, 1024])
@pytest.mark.parametrize("transposed", [False, True])
def test_rcpp_predict_high_rank(sa, ora, k, transposed):
    A = ora.synth_csc(1100, 2000, 20)
    w = np.random.default_rng(2).random((1100, k))
    if transposed:
        w = w.T.copy()
    ref = ora.rcpp_predict(A, w, 0.01, 0.0)
    got = sa.Rcpp_predict(to_dgc(sa, A), w, 0.01, 0.0, 0)
    assert rel_fro(got.T, ref) < TOL and same_zero_pattern(got.T, ref)


# ------------------------------------------------------------------------------------------------------ teams on one device --

@pytest.mark.timeout(900)
@pytest.mark.parametrize("m,n,k,ranks", [(300, 900, 130, 2), (300, 900, 130, 3), (400, 700, 257, 2), (400, 700, 257, 3)])
def test_team_on_one_device_high_rank(sa, ora, m, n, k, ranks):
    """The plain team above 128 (gene-block solves on the wave kernels, the Gram all-reduced): the oracle's fit, and the one-shard
    fit to rounding, as test_team_on_one_device_matches_the_oracle_and_the_single_shard."""
    A = ora.synth_csc(m, n, 20)
    At = A.t()
    w0 = ora.synth_winit(k, m)
    ref = ora.c_nmf(A, At, 0.0, 2, 0.01, 0.01, 0.0, 0.0, 0, w0)
    _alive(ref["d"])
    one = sa.c_nmf(to_dgc(sa, A), None, 0.0, 2, False, 0.01, 0.01, 0.0, 0.0, 0, w0.T)
    with sa.Multi([0] * ranks) as M:
        M.upload(to_dgc(sa, A))
        M.fit_init(k, w0)
        it, tols = M.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        W, d, H = M.get_factors()
        for r in range(1, ranks):
            Wr, dr, _ = M.rank_ctx(r).get_factors(h=False)
            assert np.array_equal(Wr, W) and np.array_equal(dr, d)
    assert it == 2
    assert rel_fro(W, ref["w"]) < 1e-9 and rel_fro(H, ref["h"]) < 1e-9 and rel_fro(d, ref["d"]) < 1e-9
    assert same_zero_pattern(W, ref["w"]) and same_zero_pattern(H, ref["h"])
    assert rel_fro(W, one["w"].T) < 1e-11 and rel_fro(H, one["h"].T) < 1e-11
    assert np.allclose(tols, one["tol"], rtol=1e-9, atol=0)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("m,n,k,ranks", [(420, 640, 130, 2), (420, 640, 130, 3), (600, 700, 257, 2), (600, 700, 257, 3),
                                         (900, 1000, 384, 2), (900, 1000, 384, 3)])
def test_sharded_masked_path_high_rank(sa, ora, m, n, k, ranks):
    """The masked team above 128: VALU downdates of the W-update from the hash (no mask lists), the triangles of the per-gene
    downdates packed and reduce-scattered (tri_pack_kernel, mask_gram_finalize_tri_kernel), gene-block solves on per-column
    Grams; as test_sharded_masked_path_matches_the_oracle_and_the_single_shard."""
    A = ora.synth_csc(m, n, 10)
    At = A.t()
    w0 = ora.synth_winit(k, m)
    seed, inv = 977, 10
    ref = ora.c_ard_nmf(A, At, 0.0, 2, 0.01, 0.0, 0, w0, seed, inv, 1e9, 1)
    _alive(ref["d"])
    one = sa.c_ard_nmf(to_dgc(sa, A), None, 0.0, 2, False, 0.01, 0.0, 0, w0.T, seed, inv, 1e9, 1)
    with sa.Multi([0] * ranks) as M:
        M.upload(to_dgc(sa, A))
        M.fit_init(k, w0)
        r = M.ard_run(0.0, 2, 0.01, 0.0, seed, inv, 1e9, 1)
        W, d, H = M.get_factors()
    assert list(r["iter"]) == list(ref["iter"]) == [0, 1]
    assert rel_fro(r["test_mse"], ref["test_mse"]) < 1e-9 and rel_fro(r["tol"], ref["tol"]) < 1e-7
    assert rel_fro(W, ref["w"]) < 1e-9 and rel_fro(H, ref["h"]) < 1e-9 and rel_fro(d, ref["d"]) < 1e-9
    assert same_zero_pattern(W, ref["w"]) and same_zero_pattern(H, ref["h"])
    assert rel_fro(W, one["w"].T) < 1e-10 and rel_fro(H, one["h"].T) < 1e-10
    assert rel_fro(r["test_mse"], one["test_mse"]) < 1e-11
