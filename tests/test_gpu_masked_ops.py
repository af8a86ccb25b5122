"""One masked half-step (predict_mask on either side, then mse_test) stage by stage at operator level: the per-cell test
error of every mse_test kernel family (sgl_op_mse_test_cells), the masked right-hand sides of both paths
(sgl_op_rhs_masked) and the solve against per-column Grams in every family of its dispatch (sgl_op_nnls_percol), each
against a plain reference of the same operation on small matrices built to sit on the kernels' loop edges.  (The fourth
stage, the Gram downdate, is test_mask_gram_downdate in test_gpu_ops.py.)"""
import numpy as np
import pytest

from conftest import rel_fro, to_dgc
from test_gpu_ops import _csc_from_dense, _random_csc

pytestmark = pytest.mark.gpu

NEVER = (1 << 63) - 25   # larger than half the hash range and odd: the only multiple a 64-bit hash can equal is the divisor itself


# ---------------------------------------------------------------------------------------------- A. per-cell test error --
MSE_M = [63, 64, 65, 128, 129, 700]
MSE_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193)   # around every multiple of the 64-entry window, and m itself
MSE_INV = (1, 2, 7, 40, NEVER)
MSE_RANKS_HASH = [1, 63, 64, 65, 128, 129, 256, 257, 1024]       # mse_test_kernel<R>: R = 1, 2, 4, 16 at both ends
MSE_RANKS_LIST = [1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128]   # NJ = 1 .. 8 at both ends
MSE_SEED = 99
_mse_cache = {}


def _mse_matrix(ora, m):
    """Cells with 0, 1, 63 .. 65, 127 .. 129, 191 .. 193 and m entries (those that fit), each count three times: rows from 0
    upward, rows ending at m - 1, random rows; the first and the last cell empty."""
    rng = np.random.default_rng(7000 + m)
    counts = sorted({c for c in MSE_COUNTS if c <= m} | {m})
    cols = [np.zeros(0, dtype=np.int64)]
    for cnt in counts:
        cols += [np.arange(cnt), np.arange(m - cnt, m), np.sort(rng.choice(m, size=cnt, replace=False))]
    cols.append(np.zeros(0, dtype=np.int64))
    p = np.concatenate([[0], np.cumsum([c.size for c in cols])])
    i = np.concatenate(cols).astype(np.int32)
    return ora.CSC(rng.random(i.size) + 0.25, i, p, m, len(cols))


def _mse_case(ora, m, k):
    """(A, W, d, H, squared errors at every (cell, gene) in longdouble and in float64), once per (m, k)."""
    if (m, k) not in _mse_cache:
        A = _mse_matrix(ora, m)
        rng = np.random.default_rng(100 * m + k)
        W = np.abs(rng.standard_normal((m, k)))
        H = np.abs(rng.standard_normal((A.ncol, k))) * (rng.random((A.ncol, k)) < 0.8)
        d = 0.5 + rng.random(k)
        D = A.to_dense()
        Wd = (W * d).astype(np.longdouble)
        pred = np.stack([(Wd * H[c].astype(np.longdouble)).sum(axis=1) for c in range(A.ncol)])   # pred[c, g], no BLAS: longdouble throughout
        e2 = (pred - D.T.astype(np.longdouble)) ** 2
        e2_f64 = ((W * d) @ H.T - D).T ** 2
        _mse_cache[(m, k)] = (A, W, d, H, e2, e2_f64)
    return _mse_cache[(m, k)]


def _mse_reference(ora, case, inv, cell_offset):
    """Per-cell losses in longdouble; asserts on the way that plain float64 with the genes summed in reverse order stays
    within 1e-12 of them (relative to max(loss, mean loss)): the 1e-11 the kernels are held to is an order above what
    the number format and the order of the sum can explain."""
    A, e2, e2_f64 = case[0], case[4], case[5]
    M = ora.rng_mask(MSE_SEED, cell_offset, A.ncol, A.nrow, inv).astype(bool)
    ref = np.zeros(A.ncol, dtype=np.longdouble)
    alt = np.zeros(A.ncol)
    for c in range(A.ncol):
        if M[c].any():
            ref[c] = e2[c][M[c]].sum() / M[c].sum()
            s = 0.0
            for v in e2_f64[c][M[c]][::-1]:
                s += v
            alt[c] = s / M[c].sum()
    ref64 = ref.astype(np.float64)
    assert np.all(np.abs(alt - ref64) <= 1e-12 * np.maximum(ref64, ref64.mean())), (A.nrow, inv)
    return ref64, M


def _assert_losses(got, ref, M, what):
    print(what, "worst per-cell error / bound:", float(np.max(np.abs(got - ref) / np.maximum(np.maximum(ref, ref.mean()), 1e-300))) / 1e-11)
    assert np.all(np.abs(got - ref) <= 1e-11 * np.maximum(ref, ref.mean())), what
    assert np.all(got[~M.any(axis=1)] == 0.0), what   # cells without a drawn gene: exactly 0


def _mse_fit(ctx, sa, case, k, cell_offset, ncells_total):
    A, W, d, H = case[:4]
    ctx.upload(to_dgc(sa, A), None, cell_offset=cell_offset, ncells_total=ncells_total)
    ctx.fit_init(k, W)
    ctx.set_factors(W, d, H)


def _check_total(ctx, got, inv, ncells_total):
    tot = ctx.op_mse_test(MSE_SEED, inv)
    assert abs(got.sum() / ncells_total - tot) <= 1e-11 * abs(tot), (inv, got.sum() / ncells_total, tot)


@pytest.mark.parametrize("k", MSE_RANKS_HASH)
@pytest.mark.parametrize("m", MSE_M)
def test_mse_test_cells_hashing_kernel(ctx, sa, ora, m, k):
    """mse_test_kernel<R> cell by cell: its 64-entry window over a cell's non-zeros has to move (cells of more than 64
    entries, with the window's last entry on, before and after a chunk edge), next to chunks that draw nothing (inv_density 40:
    a sixth of the 64-gene chunks at m = 700) and under a mask that draws everything / nothing.  Reference: longdouble NumPy,
    `(W * d) @ H[c]` against the dense matrix over the genes ora.rng_mask draws; the same formula in float64 with the genes in
    reverse order is within 1e-12 of it on these inputs (asserted in _mse_reference), the kernels are held to 1e-11."""
    case = _mse_case(ora, m, k)
    n = case[0].ncol
    _mse_fit(ctx, sa, case, k, 0, n)
    for inv in MSE_INV:
        ref, M = _mse_reference(ora, case, inv, 0)
        got = ctx.op_mse_test_cells(MSE_SEED, inv, 0)
        _assert_losses(got, ref, M, ("hashing", m, k, inv))
        if inv == NEVER:
            assert not got.any()
        _check_total(ctx, got, inv, n)
    if k > 128:
        for variant in (1, 2):
            with pytest.raises(sa.SingletHipError):
                ctx.op_mse_test_cells(MSE_SEED, 7, variant)


@pytest.mark.parametrize("k", MSE_RANKS_LIST)
@pytest.mark.parametrize("m", MSE_M)
def test_mse_test_cells_list_kernels(ctx, sa, ora, m, k):
    """mse_test_list_kernel<NJ> (lists, the matrix value through the sliding window) and mask_vals_kernel +
    mse_test_vals_kernel<NJ> (values listed by bisection) at every NJ: both against the longdouble reference, the same
    bits as each other (kernels_mask.hip: same predictions, same four partial sums in the same order), and the hashing
    kernel of the same rank beside them."""
    case = _mse_case(ora, m, k)
    n = case[0].ncol
    _mse_fit(ctx, sa, case, k, 0, n)
    for inv in MSE_INV:
        ref, M = _mse_reference(ora, case, inv, 0)
        window = ctx.op_mse_test_cells(MSE_SEED, inv, 1)
        assert ctx.mask_pairs()[0] == M.sum()
        listed = ctx.op_mse_test_cells(MSE_SEED, inv, 2)
        _assert_losses(window, ref, M, ("list", m, k, inv))
        _assert_losses(listed, ref, M, ("vals", m, k, inv))
        assert np.array_equal(window, listed), (m, k, inv)
        assert np.array_equal(window, ctx.op_mse_test_cells(MSE_SEED, inv, 1)), "the window kernel, now that the values are listed"
        _assert_losses(ctx.op_mse_test_cells(MSE_SEED, inv, 0), ref, M, ("hashing", m, k, inv))
        _check_total(ctx, listed, inv, n)     # (the fit's own selection: the listed values by now)


@pytest.mark.parametrize("k", [33, 65, 129])
def test_mse_test_cells_of_a_shard_hash_the_global_cell(ctx, sa, ora, k):
    """A shard at cell_offset 1000 of 5000 cells: every family hashes / lists draw(cell + 1000, gene), and the total
    divides by 5000."""
    m = 700
    case = _mse_case(ora, m, k)
    _mse_fit(ctx, sa, case, k, 1000, 5000)
    ref0, _ = _mse_reference(ora, case, 7, 0)
    for inv in (7, 40):
        ref, M = _mse_reference(ora, case, inv, 1000)
        for variant in ((0, 1, 2) if k <= 128 else (0,)):
            got = ctx.op_mse_test_cells(MSE_SEED, inv, variant)
            _assert_losses(got, ref, M, (variant, k, inv))
            _check_total(ctx, got, inv, 5000)
    assert not np.allclose(ref0, _mse_reference(ora, case, 7, 1000)[0])   # the offset matters to the reference


@pytest.mark.parametrize("k", [3, 16, 50, 70, 128, 130])
def test_mse_test_op_after_a_masked_h_update_reads_the_lists(sa, ora, k):
    """sgl_op_mse_test as a fit calls it: k_mse_test takes the list kernels only when a masked H-update has listed the
    mask under the same key -- the operator alone hashes, so the use_lists rows of test_mse_test_op (test_gpu_ops.py) run
    the hashing kernel whatever they set.  Here the mask IS listed first (mask_pairs says so), on one shard and on two with
    a cell offset, against ora.mse_test (src/singlet.cpp:536-568) to the 1e-11 of that test.  Above k = 128 the lists
    never apply (test_mse_test_op_high_rank runs the hashing kernel in both of its rows): the step lists nothing."""
    m, n, seed, inv = 333, 517, 99, 7
    A = ora.synth_csc(m, n, 9)
    rng = np.random.default_rng(k)
    W = np.abs(rng.standard_normal((m, k)))
    H = np.abs(rng.standard_normal((n, k))) * (rng.random((n, k)) < 0.8)
    d = 0.5 + rng.random(k)
    exp = ora.mse_test(A, W, d, H, seed, inv)
    drawn = ora.rng_mask(seed, 0, n, m, inv)

    def shard(lo, hi):
        sub = ora.CSC(A.x[A.p[lo]:A.p[hi]], A.i[A.p[lo]:A.p[hi]], A.p[lo:hi + 1] - A.p[lo], m, hi - lo)
        c = sa.Context(0)
        try:
            c.upload(to_dgc(sa, sub), None, cell_offset=lo, ncells_total=n)
            c.fit_init(k, W)
            c.step_h_masked(0.0, 0.0, seed, inv)
            assert c.mask_pairs()[0] == (drawn[lo:hi].sum() if k <= 128 else 0)
            c.set_factors(W, d, H[lo:hi])
            first = c.op_mse_test(seed, inv)      # lists the matrix values
            assert c.op_mse_test(seed, inv) == first
            return first
        finally:
            c.close()

    one = shard(0, n)
    assert abs(one - exp) <= 1e-11 * abs(exp), (one, exp)
    two = shard(0, 200) + shard(200, n)
    assert abs(two - exp) <= 1e-11 * abs(exp), (two, exp)


# ------------------------------------------------------------------------------------------ B. masked right-hand sides --
RHS_STYLES = ["uniform", "heavy", "mostly_empty", "extremes"]
RHS_M, RHS_N = 650, 290
RHS_SEED, RHS_INV = 4242, 5
RHS_RANKS_PLAIN = [7, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 1024]   # acc_kernel<R, MASK>: R = 1, 2, 3, 4, 8, 16 at both ends
RHS_RANKS_TILED = [1, 2, 16, 33, 50, 64, 65, 128]
TILED_SWITCHES = ("SGL_TILED_SORT", "SGL_TILED_RANGES", "SGL_TILED_NO_QUAD", "SGL_TILED_FULL_TILES")
TILED_SETTINGS = [{}, {"SGL_TILED_SORT": "1"}, {"SGL_TILED_SORT": "0"}, {"SGL_TILED_RANGES": "3"}, {"SGL_TILED_NO_QUAD": "1"},
                  {"SGL_TILED_FULL_TILES": "1"}, {"SGL_TILED_RANGES": "1"}, {"SGL_TILED_RANGES": "1", "SGL_TILED_SORT": "0"}]
_rhs_cache = {}


def _rhs_matrix(ora, style):
    """A 650 x 290 matrix of the style (test_gpu_ops._random_csc) in which the cells 3 .. 7 and, for t(A), the genes
    10 .. 14 hold exactly 63, 64, 65, 66, 67 entries: the four-wide entry loop of acc_kernel ends with 3, 0, 1, 2, 3 single
    entries (64: none, and the next 64-entry batch is empty)."""
    if style not in _rhs_cache:
        rng = np.random.default_rng(RHS_STYLES.index(style) + 31)
        D = _random_csc(ora, rng, RHS_M, RHS_N, style).to_dense()
        cells, genes = np.arange(3, 8), np.arange(10, 15)
        other_cells = np.setdiff1d(np.arange(RHS_N), cells)
        other_genes = np.setdiff1d(np.arange(RHS_M), genes)
        D[genes, :] = 0.0
        D[:, cells] = 0.0
        for q in range(5):
            D[genes[q], rng.choice(other_cells, size=63 + q, replace=False)] = rng.random(63 + q) + 0.25
            D[rng.choice(other_genes, size=63 + q, replace=False), cells[q]] = rng.random(63 + q) + 0.25
        assert list((D[:, cells] != 0).sum(axis=0)) == [63, 64, 65, 66, 67] and list((D[genes] != 0).sum(axis=1)) == [63, 64, 65, 66, 67]
        A = ora.CSC(*_csc_from_dense(D))
        _rhs_cache[style] = (A, A.t(), D, {})
    return _rhs_cache[style]


def _rhs_masked_matrices(ora, style, cell_offset):
    """(A, t(A)) with the entries draw(cell + cell_offset, gene) removed, from the oracle's mask."""
    A, At, D, masked = _rhs_matrix(ora, style)
    if cell_offset not in masked:
        M = ora.rng_mask(RHS_SEED, cell_offset, RHS_N, RHS_M, RHS_INV).astype(bool)   # [cell, gene]
        Dm = np.where(M.T, 0.0, D)
        assert 0 < (Dm != 0).sum() < (D != 0).sum()
        masked[cell_offset] = (ora.CSC(*_csc_from_dense(Dm)), ora.CSC(*_csc_from_dense(Dm.T.copy())))
    return masked[cell_offset]


def _rhs_upload(ctx, sa, ora, style, cell_offset):
    A, At = _rhs_matrix(ora, style)[:2]
    ctx.upload(to_dgc(sa, A), to_dgc(sa, At), cell_offset=cell_offset, ncells_total=5000 if cell_offset else RHS_N)
    return _rhs_masked_matrices(ora, style, cell_offset)


@pytest.mark.parametrize("cell_offset", [0, 1000])
@pytest.mark.parametrize("style", RHS_STYLES)
def test_rhs_masked_plain_kernel(ctx, sa, ora, style, cell_offset):
    """acc_kernel<R, 1> (A: draw(column + cell_offset, row)) and <R, 2> (t(A): draw(row + cell_offset, column)) at every R
    against ora.rhs on the matrix without the drawn entries, to the 1e-14 of test_rhs_both_orientations; a mask that draws
    everything gives exact zeros, one that draws nothing the bits of the unmasked kernel."""
    masked = _rhs_upload(ctx, sa, ora, style, cell_offset)
    for k in RHS_RANKS_PLAIN:
        rng = np.random.default_rng(k)
        for which, rows in ((0, RHS_M), (1, RHS_N)):
            F = rng.random((rows, k))
            got = ctx.op_rhs_masked(which, F, RHS_SEED, RHS_INV)
            err = rel_fro(got, ora.rhs(masked[which], F))
            print("plain", style, cell_offset, k, which, "rel_fro", err)
            assert err < 1e-14, (k, which)
            assert not ctx.op_rhs_masked(which, F, RHS_SEED, 1).any(), (k, which)
            assert np.array_equal(ctx.op_rhs_masked(which, F, RHS_SEED, NEVER), ctx.op_rhs(which, F)), (k, which)


@pytest.mark.parametrize("cell_offset", [0, 1000])
@pytest.mark.parametrize("setting", TILED_SETTINGS, ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()) or "default")
@pytest.mark.parametrize("style", RHS_STYLES)
def test_rhs_masked_tiled_kernel(ctx, sa, ora, style, setting, cell_offset, monkeypatch):
    """The LDS-tiled kernel on the masked value array (tiled_fill_kernel with masked = 1: the hash must see the ORIGINAL
    column and row of an entry wherever the layout puts it): columns sorted by count or in matrix order, the tile range
    split in three or whole, the pair layout at every rank, LDS-sized tiles.  Same reference and bound as the plain kernel; where
    the unmasked tiled kernel gives the bits of the unmasked plain one (same products in the same order), so must the
    masked pair -- a zeroed entry adds +0 * F."""
    for name in TILED_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in setting.items():
        monkeypatch.setenv(name, value)
    masked = _rhs_upload(ctx, sa, ora, style, cell_offset)
    same_bits = 0
    for k in RHS_RANKS_TILED:
        rng = np.random.default_rng(k)
        for which, rows in ((2, RHS_M), (3, RHS_N)):
            F = rng.random((rows, k))
            got = ctx.op_rhs_masked(which, F, RHS_SEED, RHS_INV)
            err = rel_fro(got, ora.rhs(masked[which - 2], F))
            print("tiled", style, setting, cell_offset, k, which, "rel_fro", err)
            assert err < 1e-14, (k, which)
            assert not ctx.op_rhs_masked(which, F, RHS_SEED, 1).any(), (k, which)
            unmasked = ctx.op_rhs(which, F)
            assert np.array_equal(ctx.op_rhs_masked(which, F, RHS_SEED, NEVER), unmasked), (k, which)
            if np.array_equal(unmasked, ctx.op_rhs(which - 2, F)):
                same_bits += 1
                assert np.array_equal(got, ctx.op_rhs_masked(which - 2, F, RHS_SEED, RHS_INV)), (k, which)
    print("tiled", style, setting, "bit-equal to the plain kernel at", same_bits, "of", 2 * len(RHS_RANKS_TILED))
    if setting.get("SGL_TILED_RANGES") == "1":   # the whole tile range in one piece: one pass per rank up to 64, in the plain kernel's order
        assert same_bits >= 2 * sum(k <= 64 for k in RHS_RANKS_TILED)


def test_rhs_masked_refuses_what_it_cannot_run(ctx, sa, ora):
    _rhs_upload(ctx, sa, ora, "uniform", 0)
    F = np.ones((RHS_M, 4))
    for which in (0, 2):
        with pytest.raises(sa.SingletHipError):
            ctx.op_rhs_masked(which, F, RHS_SEED, 0)


def _masked_step(c, side, W, H, seed, inv):
    """One masked half-step from the factors (W, H): the new H (side 'h') or W (side 'w')."""
    c.set_factors(w=W, h=H)
    if side == "h":
        c.step_h_masked(0.01, 0.0, seed, inv)
        return c.get_factors()[2].copy()
    c.step_w_masked(0.01, 0.0, seed, inv)
    return c.get_factors()[0].copy()


@pytest.mark.parametrize("side", ["h", "w"])
@pytest.mark.parametrize("k", [20, 50])
def test_masked_value_array_follows_the_mask(sa, ora, k, side):
    """The fit keeps ONE masked value array per orientation, keyed by (seed, inv_density, mask_t): a half-step under mask a,
    then b, then a again -- and a again under another inv_density -- gives, each time, the bits of a fresh context that
    only ever saw that mask."""
    A, At = _rhs_matrix(ora, "uniform")[:2]
    rng = np.random.default_rng(k)
    W, H = rng.random((RHS_M, k)) + 0.1, rng.random((RHS_N, k)) + 0.1
    keys = [(11, 7), (12, 7), (11, 7), (11, 3), (11, 7)]

    def fresh():
        c = sa.Context(0)
        c.upload(to_dgc(sa, A), to_dgc(sa, At))
        c.fit_init(k, W)
        return c

    c = fresh()
    try:
        assert c.layout_get()["A" if side == "h" else "At"]["entries"] > 0    # the fit runs on entry streams
        seen = [_masked_step(c, side, W, H, *key) for key in keys]
    finally:
        c.close()
    alone = {}
    for key in set(keys):
        c = fresh()
        try:
            alone[key] = _masked_step(c, side, W, H, *key)
        finally:
            c.close()
    for key, got in zip(keys, seen):
        assert np.array_equal(got, alone[key]), key
    assert not np.array_equal(alone[(11, 7)], alone[(12, 7)]) and not np.array_equal(alone[(11, 7)], alone[(11, 3)])


@pytest.mark.parametrize("k", [7, 50, 100])
def test_masked_steps_on_the_plain_kernel_match_the_oracle(ctx, sa, ora, k, monkeypatch):
    """SGL_MASKED_RHS_PLAIN=1: the fit's masked right-hand sides hashed entry by entry (acc_kernel<R, MASK>) instead of read
    from the masked value array; both half-steps against ora.predict_mask to the 1e-9 of the fits, same zeros."""
    monkeypatch.setenv("SGL_MASKED_RHS_PLAIN", "1")
    A, At = _rhs_matrix(ora, "heavy")[:2]
    rng = np.random.default_rng(k)
    W, H = rng.random((RHS_M, k)) + 0.1, rng.random((RHS_N, k)) + 0.1
    ctx.upload(to_dgc(sa, A), to_dgc(sa, At))
    ctx.fit_init(k, W)
    got_h = _masked_step(ctx, "h", W, H, 77, 6)
    ref_h = ora.predict_mask(A, 77, 6, W, H, 0.01, 0.0)
    assert rel_fro(got_h, ref_h) < 1e-9 and np.array_equal(got_h == 0, ref_h == 0)
    got_w = _masked_step(ctx, "w", W, H, 77, 6)
    ref_w = ora.predict_mask(At, 77, 6, H, W, 0.01, 0.0, 0, True)
    assert rel_fro(got_w, ref_w) < 1e-9 and np.array_equal(got_w == 0, ref_w == 0)
    # columns without a non-zero are not solved: they keep their input
    empty = np.diff(A.p) == 0
    assert empty.any() and np.array_equal(got_h[empty], H[empty])


# --------------------------------------------------------------------------------------- C. per-column-Gram solve --
NNLS_SWITCHES = ("SGL_NNLS_QUAD_GLOBAL_FROM", "SGL_NNLS_QUAD_GLOBAL_MIN_COLS", "SGL_NNLS_NO_QUAD", "SGL_NNLS_NO_QUAD_GLOBAL",
                 "SGL_NNLS_NO_QUAD_BIG", "SGL_NNLS_QUAD_GLOBAL_112")
LDS, GLOBAL, LONG, WAVE = ({"SGL_NNLS_QUAD_GLOBAL_FROM": "1000"}, {"SGL_NNLS_QUAD_GLOBAL_FROM": "1"}, {"SGL_NNLS_QUAD_GLOBAL_MIN_COLS": "1"},
                           {"SGL_NNLS_NO_QUAD": "1", "SGL_NNLS_NO_QUAD_GLOBAL": "1"})
# (family, switches, ranks) as k_nnls_percol dispatches with a Gram per column
NNLS_FAMILIES = [
    ("lds_quads", {}, [1, 2, 15, 16, 17, 31, 32, 33, 46]),             # launch_nnls_quad<1 .. 3>: below 47 on a short launch
    ("lds_quads", LDS, [47, 48, 49, 50]),                              # <4>: as far as four triangles per wave fit LDS
    ("global_quads", GLOBAL, [1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112]),   # launch_nnls_quad_global<1 .. 7>
    ("global_quads", LONG, [113, 128]),                                # <8>: long launches only
    ("big_quads", {}, [129, 144, 145, 176, 177, 208]),                 # k_nnls_quad_global_big: NR = 9 .. 13
    ("big_quads", LONG, [209, 240, 241, 256]),                         # NR = 14 .. 16: long launches only
    ("wave", WAVE, [1, 64, 65, 128, 129, 256, 257, 512, 513, 1024]),   # nnls_wave_kernel<R> with a column stride, R = 1, 2, 3, 4, 8, 16
]
NNLS_CASES = [pytest.param(fam, env, k, id="%s-%d" % (fam, k)) for fam, env, ks in NNLS_FAMILIES for k in ks]
NNLS_PEN = [(0.0, 0.0), (0.01, 0.0), (0.01, 0.02)]
_nnls_cache = {}


def _nnls_ncols(k):
    # 203 columns: 51 quads, the last of three columns, more than one workgroup in every family.  Above k = 256 only the wave
    # kernel runs (one column per wave, four per workgroup): five columns are two workgroups, the second partly filled, and
    # 203 Grams of 1024 x 1024 would be 1.7 GB
    return 203 if k <= 256 else 5


def _nnls_case(ora, k):
    """Grams that differ loudly from column to column: G_c = s_c (G - AAt(F[idx_c]) - 1e-15 I) with idx_c the rows the
    oracle's mask draws for column c at inv_density 6 and s_c in [0.25, 4]; B and X0 as in test_nnls; the oracle's
    solution and sweep count of every column under each penalty (kept per rank; the Grams are made again)."""
    rng = np.random.default_rng(9000 + k)
    ncols = _nnls_ncols(k)
    F = rng.random((600, k)) + 0.1
    G = ora.aat(F)
    M = ora.rng_mask(5, 0, ncols, 600, 6).astype(bool)
    s = 0.25 * 16.0 ** rng.random(ncols)
    Gc = np.empty((ncols, k, k))
    for c in range(ncols):
        Fs = F[M[c]]
        Gc[c] = s[c] * (G - (Fs.T @ Fs + 1e-15 * np.eye(k)))
    B = rng.normal(size=(ncols, k)) * 3 + 1.0
    X0 = np.abs(rng.normal(size=(ncols, k))) * (rng.random((ncols, k)) < 0.6) * 1e-3
    if k not in _nnls_cache:
        ref = {}
        for L1, L2 in NNLS_PEN:
            E = np.empty_like(X0)
            its = np.zeros(ncols, dtype=np.int64)
            for c in range(ncols):
                E[c], _, its[c] = ora.nnls(Gc[c], B[c], X0[c], L1, L2)
            ref[(L1, L2)] = (E, its)
        _nnls_cache[k] = ref
    return Gc, B, X0, _nnls_cache[k]


def _skips(ncols):
    """col_nnz with zeros at the first column, the last one, a whole quad and one column inside a quad."""
    nz = np.arange(1, ncols + 1, dtype=np.int64)
    nz[[0, ncols - 1]] = 0
    if ncols > 24:
        nz[8:12] = 0
        nz[21] = 0
    return nz


def _nnls_env(monkeypatch, env):
    for name in NNLS_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("family,env,k", NNLS_CASES)
def test_nnls_percol(ctx, ora, family, env, k, monkeypatch):
    """k_nnls_percol with gstride = k * k, what every masked half-step solves with: each family of its dispatch, forced by
    the switches the dispatch reads, at both ends of every instance, over 1, 3, 4, 5 and 203 columns (partial quads, one
    quad, many workgroups) and with skipped columns.  Per column ora.nnls on that column's Gram, to the bounds of test_nnls:
    1e-10, the same zeros, the same sweep total; skipped columns keep the bits of their input and count no sweep.  A kernel
    that read a neighbouring column's Gram, right-hand side or skip flag for any lane fails here: the Grams differ by up to
    16 x from column to column.  LDS and global quads give the same bits where both can run (k <= 50)."""
    Gc, B, X0, ref = _nnls_case(ora, k)
    ncols = B.shape[0]
    nz = _skips(ncols)
    for L1, L2 in NNLS_PEN:
        E, its = ref[(L1, L2)]
        _nnls_env(monkeypatch, env)
        runs = [(n, None) for n in (1, 3, 4, 5) if n < ncols] + [(ncols, None), (ncols, nz), (5, _skips(5))]
        for n, skip in runs:
            X, sweeps = ctx.op_nnls_percol(Gc[:n], B[:n], X0[:n], skip, L1, L2)
            solved = np.ones(n, dtype=bool) if skip is None else skip != 0
            what = (family, k, L1, L2, n, skip is not None)
            err = rel_fro(X[solved], E[:n][solved])
            if n == ncols:
                print("nnls_percol", what, "rel_fro", err)
            assert err < 1e-10, what
            assert np.array_equal(X[solved] == 0, E[:n][solved] == 0), what
            assert np.array_equal(X[~solved], X0[:n][~solved]), what
            assert sweeps == its[:n][solved].sum(), what
            if family == "lds_quads":
                _nnls_env(monkeypatch, GLOBAL)
                X2, sweeps2 = ctx.op_nnls_percol(Gc[:n], B[:n], X0[:n], skip, L1, L2)
                _nnls_env(monkeypatch, env)
                assert np.array_equal(X, X2) and sweeps == sweeps2, what


def test_nnls_percol_refuses_bad_arguments(ctx, sa):
    G, B = np.ones((3, 2, 2)), np.ones((3, 2))
    with pytest.raises(ValueError):
        ctx.op_nnls_percol(G[:2], B, B)
    with pytest.raises(sa.SingletHipError):
        ctx.op_nnls_percol(np.ones((1, 1025, 1025)), np.ones((1, 1025)), np.ones((1, 1025)))
