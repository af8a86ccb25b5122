"""RasterizeRowwise on the GPU (kernels_raster.hip: sgl_c_rowwise_compress_sparse / _dense, sgl_rasterize_rowwise) against the
test-side restatement (tests/rowwise_compress_restatement.py), bit for bit: random shapes with empty and full columns and
integer counts, pbmc3k, the remainder rows, sparse = dense, n > nrow, refusals, NaN / Inf, determinism, the resident form
(after upload, after LogNormalize, under a fit, refused on teams / hooks / overflow), and two sizes past 2^31 elements."""
import os

import numpy as np
import pytest

import rowwise_compress_restatement as rr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NS = [1, 2, 3, 7, 10, 64, 1000]


def _dgc(sa, D, stored=None):
    """dgCMatrix of the dense D; `stored` (bool mask) names the stored entries (default: every non-zero)."""
    D = np.asarray(D, dtype=np.float64)
    mask = (D != 0) | np.isnan(D) if stored is None else stored
    nrow, ncol = D.shape
    cols = [np.nonzero(mask[:, j])[0] for j in range(ncol)]
    p = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
    i = np.concatenate(cols).astype(np.int32) if ncol else np.zeros(0, np.int32)
    x = np.concatenate([D[c, j] for j, c in enumerate(cols)]) if ncol else np.zeros(0)
    return sa.dgCMatrix(x, i, p, (nrow, ncol))


def _random(rng, nrow, ncol, density, counts=True):
    if counts:
        D = np.where(rng.random((nrow, ncol)) < density, rng.integers(1, 60, (nrow, ncol)), 0).astype(np.float64)
    else:
        D = np.where(rng.random((nrow, ncol)) < density, rng.standard_normal((nrow, ncol)) * 10.0 ** rng.integers(-4, 5, (nrow, ncol)), 0.0)
    if ncol >= 3:
        D[:, 0] = 0.0                                        # an empty column
        D[:, ncol // 2] = rng.integers(1, 9, nrow)           # a fully dense column
    return D


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.dtype == np.float64 and (got.flags.f_contiguous or got.size == 0)
    if not rr.same_bits(got, want):
        bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError("first differing (bin, column): %s" % bad[:5].tolist())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape,density,counts", [((1000, 37), 0.05, True), ((2001, 130), 0.3, False), ((5000, 9), 0.01, True)])
def test_one_shot_equals_the_restatement(sa, n, shape, density, counts):
    rng = np.random.default_rng(n * 7 + shape[0] + int(counts))
    D = _random(rng, *shape, density, counts)
    want = rr.vectorised_dense(D, n)
    if n <= shape[0] and shape[0] % n == 0:
        assert rr.same_bits(rr.literal_dense(D, n), want)
    gs = sa.rowwise_compress_sparse(_dgc(sa, D), n)
    gd = sa.rowwise_compress_dense(D, n)
    _same(gs, want)
    _same(gd, want)


def _pbmc3k(sa):
    g = np.load(os.path.join(GOLD, "pbmc3k_counts.npz"))
    p, di, x = g["p"].astype(np.int64), g["di"].astype(np.int64), g["x"].astype(np.float64)
    cs = np.cumsum(di)
    i = cs - np.repeat(cs[p[:-1]] - di[p[:-1]], np.diff(p))      # undo the per-column delta coding
    return sa.dgCMatrix(x, i.astype(np.int32), p.astype(np.int32), (int(g["dim"][0]), int(g["dim"][1])))


def test_pbmc3k(sa):
    A = _pbmc3k(sa)
    assert A.nrow == 13714 and A.nrow % 10 == 4
    want = rr.vectorised_sparse(A, 10)
    got = sa.rowwise_compress_sparse(A, 10)
    _same(got, want)
    _same(sa.rowwise_compress_dense(rr.densify(A), 10), want)
    B = sa.RasterizeRowwise(A)
    _same(np.asarray(B), want)


@pytest.mark.parametrize("n", [3, 7, 10, 64])
def test_remainder_rows_change_nothing(sa, n):
    rng = np.random.default_rng(n)
    nrow = 40 * n + n - 1 if n > 1 else 40
    D = _random(rng, nrow, 20, 0.2)
    want = rr.vectorised_dense(D[: (nrow // n) * n], n)
    _same(sa.rowwise_compress_dense(D, n), want)
    _same(sa.rowwise_compress_sparse(_dgc(sa, D), n), want)
    D2 = D.copy()
    D2[(nrow // n) * n:, :] = rng.standard_normal((nrow % n, 20)) * 1e300   # the remainder filled, NaN and Inf too
    D2[-1, :3] = [np.nan, np.inf, -np.inf]
    _same(sa.rowwise_compress_dense(D2, n), want)
    _same(sa.rowwise_compress_sparse(_dgc(sa, D2), n), want)


def test_sparse_equals_dense_with_signed_zeros_and_specials(sa):
    rng = np.random.default_rng(11)
    D = _random(rng, 300, 50, 0.3, counts=False)
    flat = D.reshape(-1, order="F")
    pos = rng.choice(flat.size, 200, replace=False)
    flat[pos] = np.tile([np.nan, np.inf, -np.inf, -0.0, 0.0], 40)
    D = flat.reshape(D.shape, order="F")
    stored = (D != 0) | np.isnan(D) | np.signbit(D)        # stored -0.0 entries
    for n in (1, 3, 10):
        want = rr.vectorised_dense(D, n)
        a, b = sa.rowwise_compress_sparse(_dgc(sa, D, stored), n), sa.rowwise_compress_dense(D, n)
        _same(a, want)
        _same(b, want)
        assert np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)])


def test_nan_and_inf_propagate_and_overflow_gives_inf(sa):
    D = np.zeros((6, 4))
    D[0, 0], D[1, 0] = np.inf, -np.inf          # +Inf and -Inf in one bin: NaN
    D[2, 1] = np.nan
    D[0, 2], D[1, 2] = 1.5e308, 1.5e308        # a finite overflow: Inf
    D[4, 3], D[5, 3] = -np.inf, 3.0
    for got in (sa.rowwise_compress_sparse(_dgc(sa, D), 2), sa.rowwise_compress_dense(D, 2)):
        assert np.isnan(got[0, 0]) and np.isnan(got[1, 1]) and got[0, 2] == np.inf and got[2, 3] == -np.inf
        assert got[1, 0] == 0.0 and got[2, 0] == 0.0
        _same(got, rr.vectorised_dense(D, 2))


def test_n_above_nrow_and_refusals(sa):
    D = np.arange(12.0).reshape(4, 3)
    A = _dgc(sa, D)
    for fn, M in ((sa.rowwise_compress_sparse, A), (sa.rowwise_compress_dense, D)):
        assert fn(M, 5).shape == (0, 3)
        for bad in (0, -1, -7.5, 0.5, float("nan")):
            with pytest.raises(sa.SingletHipError, match=r"n (=|is NA)"):
                fn(M, bad)
        assert fn(M, 2.9).shape == (2, 3)            # truncated toward zero, as Rcpp's as<size_t>
    with pytest.raises(ValueError, match="wrong sign"):
        sa.RasterizeRowwise(A, 5)
    for i, p in (([0, 7], [0, 2, 2, 2]),                 # a row outside [0, nrow)
                 ([2, 1], [0, 2, 2, 2])):                # rows not ascending within a column
        bad = sa.dgCMatrix.__new__(sa.dgCMatrix)         # past the Python-side checks, straight to the library's
        bad.x, bad.i, bad.p, bad.Dim, bad.Dimnames = np.array([1.0, 2.0]), np.array(i, np.int32), np.array(p, np.int32), (4, 3), (None, None)
        with pytest.raises(sa.SingletHipError, match="dgCMatrix"):
            sa.rowwise_compress_sparse(bad, 2)


def test_deterministic(sa):
    rng = np.random.default_rng(5)
    D = _random(rng, 3000, 200, 0.1, counts=False)
    A = _dgc(sa, D)
    a = sa.rowwise_compress_sparse(A, 7)
    for _ in range(3):
        assert np.array_equal(sa.rowwise_compress_sparse(A, 7).view(np.uint64), a.view(np.uint64))
        assert np.array_equal(sa.rowwise_compress_dense(D, 7).view(np.uint64), a.view(np.uint64))


def test_rasterize_rowwise_names(sa):
    rng = np.random.default_rng(2)
    D = _random(rng, 25, 4, 0.5)
    A = _dgc(sa, D)
    A = sa.dgCMatrix(A.x, A.i, A.p, A.Dim, (["g%d" % r for r in range(25)], ["c%d" % c for c in range(4)]))
    B = sa.RasterizeRowwise(A, 10)
    assert isinstance(B, np.ndarray) and B.shape == (2, 4) and B.flags.f_contiguous
    assert B.rownames == ["g0", "g10"] and B.colnames == ["c0", "c1", "c2", "c3"]   # rownames(A)[seq(1, 20, 10)]
    _same(np.asarray(B), rr.vectorised_dense(D, 10))
    Bd = sa.RasterizeRowwise(D, 10)                    # anything else: the dense entry
    assert Bd.rownames is None and Bd.colnames is None
    _same(np.asarray(Bd), rr.vectorised_dense(D, 10))


# ---- the resident form -------------------------------------------------------------------------------------------------
def _resident_dense(c):
    x, i, p = c.download(0)
    nr, nc, _ = c.dims()
    return rr.densify(type("M", (), {"x": x, "i": i, "p": p, "nrow": nr, "ncol": nc})())


@pytest.mark.parametrize("n", [1, 3, 10, 64])
def test_resident_equals_the_restatement(sa, n):
    rng = np.random.default_rng(100 + n)
    D = _random(rng, 1283, 300, 0.05)
    c = sa.Context(0)
    try:
        c.upload(_dgc(sa, D))
        c.rasterize_rowwise(n)
        want = rr.vectorised_dense(D, n)
        assert c.dims()[:2] == want.shape
        _same(np.asfortranarray(_resident_dense(c)), want)
        xt, it, pt = c.download(1)                       # the transpose, built on the device
        T = rr.densify(type("M", (), {"x": xt, "i": it, "p": pt, "nrow": want.shape[1], "ncol": want.shape[0]})())
        assert np.array_equal(T.view(np.uint64), np.ascontiguousarray(want.T).view(np.uint64))
        c.rasterize_rowwise(1)                           # again, on the rasterised matrix
        _same(np.asfortranarray(_resident_dense(c)), want)
    finally:
        c.close()


def test_resident_after_dense_upload_and_log_normalize(sa):
    rng = np.random.default_rng(9)
    D = _random(rng, 500, 120, 0.1)
    D[:, 0] = 1.0                                        # no empty column for LogNormalize
    c = sa.Context(0)
    try:
        c.upload_dense(D)
        c.rasterize_rowwise(10)
        _same(np.asfortranarray(_resident_dense(c)), rr.vectorised_dense(D, 10))
        c.upload(_dgc(sa, D))
        c.log_normalize(10000.0)
        c.rasterize_rowwise(10)
        want = np.asarray(sa.RasterizeRowwise(sa.PreprocessData(_dgc(sa, D)), 10))
        _same(np.asfortranarray(_resident_dense(c)), want)
    finally:
        c.close()


def test_fit_on_the_resident_rasterisation_equals_c_nmf_dense(sa):
    rng = np.random.default_rng(21)
    D = rng.integers(1, 20, (600, 400)).astype(np.float64) * (rng.random((600, 400)) < 0.3)
    R = rr.vectorised_dense(D, 10)
    assert (R.sum(axis=0) > 0).all() and (R.sum(axis=1) > 0).all()   # no empty row or column: the skip rule is moot
    k = 6
    w0 = rng.random((k, R.shape[0]))
    ref = sa.c_nmf_dense(R, None, 1e-12, 8, False, 0.01, 0.01, 0.0, 0.0, 0, w0)
    c = sa.Context(0)
    try:
        c.upload(_dgc(sa, D))
        c.rasterize_rowwise(10)
        c.fit_init(k, np.ascontiguousarray(w0.T))
        c.nmf_run(1e-12, 8, 0.01, 0.01, 0.0, 0.0)
        W, d, H = c.get_factors()
    finally:
        c.close()
    assert np.array_equal(W, ref["w"].T) and np.array_equal(d, ref["d"]) and np.array_equal(H, ref["h"].T)


def test_resident_refusals(sa):
    rng = np.random.default_rng(4)
    D = _random(rng, 100, 30, 0.2)
    A = _dgc(sa, D)
    c = sa.Context(0)
    try:
        with pytest.raises(sa.SingletHipError, match="no matrix"):
            c.rasterize_rowwise(2)
        c.upload(A)
        for bad in (0, -3, 101):
            with pytest.raises(sa.SingletHipError, match="n ="):
                c.rasterize_rowwise(bad)
        assert c.dims() == (100, 30, A.nnz)               # the matrix stays
        c.set_allreduce(lambda ptr, count: None)
        with pytest.raises(sa.SingletHipError, match="all-reduce"):
            c.rasterize_rowwise(2)
        assert c.dims() == (100, 30, A.nnz)
        c.set_allreduce(None)
        c.rasterize_rowwise(100)                          # n = nrow: one bin
        assert c.dims()[:2] == (1, 30)
        # a sum that overflows: refused like a non-finite dense upload, and no matrix stays resident
        big = np.zeros((4, 3))
        big[0, 1] = big[1, 1] = 1.5e308
        c.upload(_dgc(sa, big))
        with pytest.raises(sa.SingletHipError, match="non-finite"):
            c.rasterize_rowwise(2)
        with pytest.raises(sa.SingletHipError, match="no matrix"):
            c.download(0)
    finally:
        c.close()
    with sa.Multi([0, 0]) as M:
        M.upload(A)
        r0 = M.rank_ctx(0)
        before = r0.dims()
        with pytest.raises(sa.SingletHipError, match="team"):
            r0.rasterize_rowwise(2)
        assert r0.dims() == before


# ---- past 2^31 elements --------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_one_shot_result_past_2e31(sa):
    nrow, ncol, n = 100_000, 43_000, 2                     # 50 000 x 43 000 = 2.15e9 bins
    nb = nrow // n
    assert nb * ncol > 2**31
    rows = {0: [0, 1, 77, nrow - 2, nrow - 1], ncol - 1: [0, 1, 5000, nrow - 2, nrow - 1], ncol // 2: [3]}
    p = np.zeros(ncol + 1, dtype=np.int64)
    for col, r in rows.items():
        p[col + 1] = len(r)
    p = np.cumsum(p).astype(np.int32)
    i = np.concatenate([np.array(rows[c], np.int32) for c in sorted(rows)])
    x = np.arange(1.0, i.size + 1.0)
    A = sa.dgCMatrix(x, i, p, (nrow, ncol))
    got = sa.rowwise_compress_sparse(A, n)
    assert got.shape == (nb, ncol)
    want = {}
    q = 0
    for col in sorted(rows):
        for r in rows[col]:
            want[(r // n, col)] = want.get((r // n, col), 0.0) + x[q]
            q += 1
    for (b, col), s in want.items():
        assert got[b, col] == s / n, (b, col)
    nz = np.count_nonzero(got[:, [0, ncol // 2, ncol - 1]])
    assert nz == len(want)
    rng = np.random.default_rng(0)
    bs, cs = rng.integers(0, nb, 20000), rng.integers(0, ncol, 20000)
    keep = np.array([(b, c) not in want for b, c in zip(bs, cs)])
    assert not got[bs[keep], cs[keep]].any()
    assert got[nb - 1, ncol - 1] == (x[-2] + x[-1]) / n   # the last element, past 2^31


@pytest.mark.timeout(1800)
def test_resident_config3(sa, ora):
    GENES, CELLS, INV, n = 30_000, 1_000_000, 20, 10
    c = sa.Context(0)
    try:
        c.synth(GENES, CELLS, INV)
        c.rasterize_rowwise(n)
        nr, nc, nnz = c.dims()
        assert (nr, nc) == (GENES // n, CELLS) and nr * nc > 2**31
        x, i, p = c.download(0)
        assert c.col_counts(1).sum() == nnz              # the transpose holds the same entries
    finally:
        c.close()
    assert p[-1] == nnz
    for s0 in (0, 333_333, 715_700, CELLS - 256):          # slices before, across and past 2^31 dense elements (column 715 828)
        S = ora.synth_csc(GENES, 256, INV, cell0=s0)
        want = rr.vectorised_sparse(S, n)
        got = rr.densify(type("M", (), {"x": x[p[s0]:p[s0 + 256]], "i": i[p[s0]:p[s0 + 256]], "p": p[s0:s0 + 257] - p[s0],
                                        "nrow": nr, "ncol": 256})())
        _same(np.asfortranarray(got), want)
