"""sgl_subset: A <- A[rows, cols] on the resident matrix, and RunNMF, the driver that uses it.

The reference side is a plain-NumPy CSC with a column gather and a stable-sort transpose; the operator only moves data, so
both downloaded orientations are compared with it bit for bit (x as uint64), and a fit on a subset context must give the
bits of the same fit on a context that uploaded the host-side subset: same matrix image, same kernels.

The gather copies tiles of SGL_SUBSET_TILE consecutive OUTPUT entries (singlet_amd/csrc/kernels_subset.hip); T below is the
one copy of that constant on this side, and the tile-edge cases place column ends on, before and after multiples of it.
"""
import functools
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
T = 4096   # SGL_SUBSET_TILE of singlet_amd/csrc/kernels_subset.hip
SGL_EINVAL, SGL_ESTATE = -1, -6
NO_MATRIX = "no matrix resident"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------- plain CSC helper
class Csc:
    """dgCMatrix slots in NumPy, no library behind them (the reference side of this file)."""

    def __init__(self, x, i, p, nrow):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.i = np.ascontiguousarray(i, dtype=np.int32)
        self.p = np.ascontiguousarray(p, dtype=np.int64)
        self.nrow, self.ncol = int(nrow), int(self.p.shape[0] - 1)

    @property
    def nnz(self):
        return int(self.p[-1])

    def lens(self):
        return np.diff(self.p)

    def t(self):
        """Matrix::t of a valid matrix: a stable sort by row keeps the columns ascending inside every row."""
        o = np.argsort(self.i, kind="stable")
        tp = np.zeros(self.nrow + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.i, minlength=self.nrow), out=tp[1:])
        colof = np.repeat(np.arange(self.ncol, dtype=np.int32), self.lens())
        return Csc(self.x[o], colof[o], tp, self.ncol)

    def gather(self, sel):
        """Columns sel, in that order, each as it is stored."""
        sel = np.asarray(sel, dtype=np.int64)
        ln = self.lens()[sel]
        p = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        src = np.repeat(self.p[sel] - p[:-1], ln) + np.arange(int(p[-1]), dtype=np.int64)
        return Csc(self.x[src], self.i[src], p, self.nrow)

    def subset(self, rows=None, cols=None):
        M = self
        if cols is not None:
            M = M.gather(cols)
        if rows is not None:
            M = M.t().gather(rows).t()
        return M

    def dgc(self, sa, names=(None, None)):
        return sa.dgCMatrix(self.x, self.i, self.p.astype(np.int32), (self.nrow, self.ncol), names)


def from_dense(D):
    """The CSC image of a dense matrix as `D != 0` defines it."""
    keep = (D != 0).T
    p = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    return Csc(D.T[keep], np.nonzero(keep)[1], p, D.shape[0])


def from_rows(nrow, ncol, cols_per_row, rng):
    """nrow x ncol with row r stored at the columns cols_per_row[r] (ascending)."""
    r = np.concatenate([np.full(len(c), q, dtype=np.int32) for q, c in enumerate(cols_per_row)])
    c = np.concatenate([np.asarray(c, dtype=np.int64) for c in cols_per_row])
    o = np.lexsort((r, c))
    p = np.zeros(ncol + 1, dtype=np.int64)
    np.cumsum(np.bincount(c, minlength=ncol), out=p[1:])
    return Csc(0.5 + rng.random(r.size), r[o], p, nrow)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_csc(got, exp, what):
    x, i, p = got
    assert np.array_equal(p, exp.p), what + ": p"
    assert np.array_equal(i, exp.i), what + ": i"
    assert np.array_equal(bits(x), bits(exp.x)), what + ": x (bits)"


def assert_resident(c, exp, what):
    """dims, both orientations and the per-column counts of the resident matrix against the reference."""
    assert c.dims() == (exp.nrow, exp.ncol, exp.nnz), what + ": dims"
    assert_same_csc(c.download(0), exp, what + ": A")
    assert_same_csc(c.download(1), exp.t(), what + ": At")
    assert np.array_equal(c.col_counts(0), exp.lens()), what + ": counts per cell"
    assert np.array_equal(c.col_counts(1), exp.t().lens()), what + ": counts per gene"


# ---------------------------------------------------------------------------------------------------------- selections
EMPTY_ROWS, EMPTY_COLS = (5, 20), (7, 40)


@functools.lru_cache(maxsize=None)
def small():
    """37 x 53 at 30 % with two empty rows and two empty columns."""
    rng = np.random.default_rng(21)
    D = np.where(rng.random((37, 53)) < 0.3, 0.5 + rng.random((37, 53)), 0.0)
    D[list(EMPTY_ROWS), :] = 0.0
    D[:, list(EMPTY_COLS)] = 0.0
    return from_dense(D)


def selection(name, n, empties):
    if name == "identity":
        return np.arange(n)
    if name == "reversal":
        return np.arange(n)[::-1]
    if name == "permutation":
        return np.random.default_rng(22 + n).permutation(n)
    if name == "duplicates":
        return np.array([3, 1, 3, 3])
    if name == "single":
        return np.array([n - 2])
    return np.array(empties)   # "empty": only empty rows / columns, so the result stores nothing


SELECTIONS = ("identity", "reversal", "permutation", "duplicates", "single", "empty")


@gpu
@pytest.mark.parametrize("mode", ("rows", "cols", "both"))
@pytest.mark.parametrize("name", SELECTIONS)
def test_selection_matches_numpy_bit_for_bit(sa, ctx, name, mode):
    M = small()
    rows = selection(name, M.nrow, EMPTY_ROWS) if mode in ("rows", "both") else None
    cols = selection(name, M.ncol, EMPTY_COLS) if mode in ("cols", "both") else None
    exp = M.subset(rows, cols)
    ctx.upload(M.dgc(sa), None)
    ctx.subset(rows, cols)
    assert_resident(ctx, exp, "%s / %s" % (name, mode))
    if name == "empty":
        assert exp.nnz == 0
        with sa.Context(0) as c2:   # the same residency as uploading the host-side subset
            c2.upload(exp.dgc(sa), None)
            assert c2.dims() == ctx.dims()
            for which in (0, 1):
                assert_same_csc(ctx.download(which), Csc(*c2.download(which), exp.ncol if which else exp.nrow), "vs upload")


@gpu
def test_explicit_zeros_stay_stored(sa, ctx):
    M = small()
    x = M.x.copy()
    x[::7] = 0.0
    x[3::11] = -0.0
    M = Csc(x, M.i, M.p, M.nrow)
    rows, cols = np.array([3, 1, 3, 36, 0, 20]), np.random.default_rng(5).permutation(M.ncol)[:30]
    exp = M.subset(rows, cols)
    assert np.count_nonzero(exp.x == 0) > 5 and np.any(np.signbit(exp.x))
    ctx.upload(M.dgc(sa), None)
    ctx.subset(rows, cols)
    assert_resident(ctx, exp, "explicit zeros")


@gpu
def test_both_null_is_a_noop_that_drops_the_fit(sa, ctx):
    M = small()
    ctx.upload(M.dgc(sa), None)
    ctx.fit_init(3, None)
    ctx.subset(None, None)
    assert_resident(ctx, M, "no-op")
    with pytest.raises(sa.SingletHipError) as err:
        ctx.step_h(0.01, 0.0)
    assert err.value.code == SGL_ESTATE


# ----------------------------------------------------------------------------------------------------------- tile edges
# rows of a 6 x 13 000 matrix with exactly these many entries; the row gather copies them as columns of t(A) that end one
# short of a tile edge, exactly on it, one past it, fill exactly one tile, span four, and sit empty on an edge
EDGE_CASES = {
    "ends_before_on_after": ((T - 1, 1, T, 0, T + 1, 3 * T + 1), [0, 1, 2, 3, 4, 5]),
    "wave_laps_dups":       ((63, 64, 65, T, 0, 1), [3, 3, 0, 1, 2, 4, 5, 3, 2]),
    "four_tiles_first":     ((T, T, 64, 0, 3 * T + 1, T + 1), [4, 0, 3, 1, 5, 3, 2]),
    "whole_tiles_only":     ((T, 0, T, T, 0, 63), [1, 0, 4, 2, 3, 0]),
    "single_long":          ((1, 65, T - 1, T + 1, 3 * T + 1, 0), [4]),
}


@functools.lru_cache(maxsize=None)
def edge_matrix(counts):
    rng = np.random.default_rng(31)
    return from_rows(6, 13000, [np.sort(rng.choice(13000, n, replace=False)) for n in counts], rng)


def test_edge_cases_cover_the_counts():
    seen = {counts[r] for counts, sel in EDGE_CASES.values() for r in sel}
    assert seen >= {0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1}


@gpu
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_row_gather_at_tile_edges(sa, ctx, case):
    counts, rows = EDGE_CASES[case]
    M = edge_matrix(counts)
    assert tuple(M.t().lens()) == counts
    exp = M.subset(rows, None)
    ctx.upload(M.dgc(sa), None)
    ctx.subset(rows, None)
    assert_resident(ctx, exp, case)


@gpu
def test_row_and_column_gather_at_tile_edges(sa, ctx):
    counts, rows = EDGE_CASES["four_tiles_first"]
    M = edge_matrix(counts)
    cols = np.arange(M.ncol)[::-1][::2]
    exp = M.subset(rows, cols)
    ctx.upload(M.dgc(sa), None)
    ctx.subset(rows, cols)
    assert_resident(ctx, exp, "rows and cols")


@gpu
@pytest.mark.parametrize("with_rows", (False, True))
def test_tile_over_thousands_of_empty_columns(sa, ctx, with_rows):
    rng = np.random.default_rng(32)
    ncol = 9000
    p = np.zeros(ncol + 1, dtype=np.int64)
    for c in (0, 4500, 8999):
        p[c + 1:] += 1
    M = Csc(0.5 + rng.random(3), [4999, 0, 2500], p, 5000)
    rows = np.arange(5000) if with_rows else None
    cols = np.arange(ncol)[::-1]
    exp = M.subset(rows, cols)
    assert list(np.nonzero(exp.lens())[0]) == [0, 4499, 8999]
    ctx.upload(M.dgc(sa), None)
    ctx.subset(rows, cols)
    assert_resident(ctx, exp, "sparse columns")


# ---------------------------------------------------------------------------------------------------------------- state
@gpu
def test_subset_drops_the_fit_and_its_streams(sa):
    M = small()
    rows = np.array([30, 2, 2, 11, 8, 36, 1])
    with sa.Context(0) as c:
        c.upload(M.dgc(sa), None)
        c.fit_init(4, None)
        c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        assert c.layout_builds()[:2] == (1, 1)
        c.subset(rows, None)
        assert c.layout_builds()[:2] == (0, 0)          # the streams of the old matrix are gone
        with pytest.raises(sa.SingletHipError) as err:
            c.step_h(0.01, 0.0)
        assert err.value.code == SGL_ESTATE
        assert_resident(c, M.subset(rows, None), "after a fit")
        c.fit_init(4, None)
        assert c.layout_builds()[:2] == (1, 1)          # and the next fit writes those of the new one
        assert np.isfinite(c.nmf_iterate(0.01, 0.01, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------- fits on the subset
def fit_bits(c, k, w0):
    """A plain and a masked fit on the resident matrix, everything they return."""
    c.fit_init(k, w0)
    n_iter, tr = c.nmf_run(0.0, 3, 0.01, 0.01, 0.0, 0.0)
    out = [np.array([n_iter], dtype=np.float64), tr, *c.get_factors()]
    c.fit_init(k, w0)
    r = c.ard_run(0.0, 3, 0.01, 0.0, 7, 20, 1e9, 1)
    out += [r["test_mse"], r["tol"], r["score_overfit"], r["iter"].astype(np.float64), *c.get_factors()]
    return out


def assert_same_fits(got, exp):
    assert len(got) == len(exp)
    for q, (a, b) in enumerate(zip(got, exp)):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), "fit output %d differs" % q


@gpu
def test_fits_on_the_subset_equal_fits_on_the_uploaded_subset(sa):
    rng = np.random.default_rng(41)
    D = np.where(rng.random((300, 400)) < 0.05, 0.5 + rng.random((300, 400)), 0.0)
    M = from_dense(D)
    rows = rng.permutation(300)[:120]
    rows = np.concatenate([rows, rows[[3, 77]]])
    w0 = rng.random((rows.size, 5))
    with sa.Context(0) as c, sa.Context(0) as f:
        c.upload(M.dgc(sa), None)
        c.subset(rows, None)
        f.upload(M.subset(rows, None).dgc(sa), None)
        assert_same_fits(fit_bits(c, 5, w0), fit_bits(f, 5, w0))


@gpu
def test_dense_door(sa):
    rng = np.random.default_rng(42)
    D = np.where(rng.random((40, 30)) < 0.8, 0.5 + rng.random((40, 30)), 0.0)
    rows = np.array([7, 39, 0, 7, 12, 13, 14, 30, 2, 21, 22, 5])
    exp = from_dense(D).subset(rows, None)
    w0 = rng.random((rows.size, 4))
    G = from_dense(np.eye(30)).dgc(sa)
    with sa.Context(0) as c, sa.Context(0) as f:
        c.upload_dense(D)
        c.subset(rows, None)
        assert_resident(c, exp, "dense door")
        f.upload(exp.dgc(sa), None)
        assert_same_fits(fit_bits(c, 4, w0), fit_bits(f, 4, w0))
        c.fit_init(4, w0)
        with pytest.raises(sa.SingletHipError, match="dense"):   # still dense input: c_gcnmf takes a dgCMatrix
            c.set_graph(G)


@gpu
def test_chain_log_normalize_then_subset(sa, ctx):
    M = small()
    counts = Csc(np.ceil(M.x * 9), M.i, M.p, M.nrow)
    rows, cols = np.array([36, 4, 4, 19, 0]), np.random.default_rng(6).permutation(M.ncol)[:41]
    ctx.upload(counts.dgc(sa), None)
    ctx.log_normalize()
    full = Csc(*ctx.download(0), counts.nrow)
    ctx.subset(rows, cols)
    assert_resident(ctx, full.subset(rows, cols), "log_normalize -> subset")


# ------------------------------------------------------------------------------------------------------------- refusals
def refused(sa, c, call, code, text, before):
    with pytest.raises(sa.SingletHipError, match=text) as err:
        call()
    assert err.value.code == code
    if before is not None:
        assert_resident(c, before, "after the refusal")


@gpu
def test_bad_indices_and_empty_lists_are_refused_before_anything_is_freed(sa):
    M = small()
    with sa.Context(0) as c:
        c.upload(M.dgc(sa), None)
        c.fit_init(3, None)
        refused(sa, c, lambda: c.subset([0, 1, -1], None), SGL_EINVAL, r"rows\[2\] = -1", M)
        refused(sa, c, lambda: c.subset([M.nrow], [0]), SGL_EINVAL, r"rows\[0\] = 37", M)
        refused(sa, c, lambda: c.subset([0], [1, M.ncol]), SGL_EINVAL, r"cols\[1\] = 53", M)
        refused(sa, c, lambda: c.subset(np.zeros(0, dtype=np.int32), None), SGL_EINVAL, "rows", M)
        refused(sa, c, lambda: c.subset([1], np.zeros(0, dtype=np.int32)), SGL_EINVAL, "cols", M)
        assert np.isfinite(c.nmf_iterate(0.01, 0.01, 0.0, 0.0))   # the running fit is untouched too


@gpu
def test_shards_and_hooks_are_refused(sa):
    M = small()
    with sa.Context(0) as c:
        c.upload(M.dgc(sa), None)
        c.set_allreduce(lambda p, n: None)
        refused(sa, c, lambda: c.subset([0, 1], None), SGL_ESTATE, "all-reduce hook", M)
        c.set_allreduce(None)
        c.upload(M.dgc(sa), None, cell_offset=5, ncells_total=100)
        refused(sa, c, lambda: c.subset(None, [0, 1]), SGL_ESTATE, "shard", M)
    with sa.Context(0) as c:
        refused(sa, c, lambda: c.subset([0], None), SGL_ESTATE, NO_MATRIX, None)
        with pytest.raises(sa.SingletHipError, match=NO_MATRIX):
            c.download(0)


# --------------------------------------------------------------------------------------------------------------- RunNMF
@functools.lru_cache(maxsize=None)
def pbmc3k():
    g = np.load(os.path.join(GOLD, "pbmc3k_counts.npz"))
    p, di, x = g["p"].astype(np.int64), g["di"].astype(np.int64), g["x"].astype(np.float64)
    cs = np.cumsum(di)
    i = cs - np.repeat(cs[p[:-1]] - di[p[:-1]], np.diff(p))      # undo the per-column delta coding
    return Csc(x, i, p, int(g["dim"][0]))


@gpu
def test_run_nmf_driver_equals_the_hand_staged_pipeline(sa):
    M = pbmc3k()
    rng = np.random.default_rng(51)
    genes = ["g%05d" % q for q in range(M.nrow)]
    A = M.dgc(sa, (genes, None))
    pick = rng.permutation(M.nrow)[:500]
    features = [genes[q] for q in pick]
    labels = rng.choice(np.array(["ctrl", "stim", "wash"]), M.ncol)
    got = sa.RunNMF(A, k=5, features=features, split_by=labels, maxit=5, tol=0, seed=1, verbose=0)

    P = sa.PreprocessData(A)
    S = Csc(P.x, P.i, P.p, P.nrow).subset(pick, None).dgc(sa, (features, None))
    Wt = sa.weight_by_split(S, np.searchsorted(np.unique(labels), labels), 3)
    ref = sa.run_nmf(Wt, 5, tol=0, maxit=5, verbose=False, L1=0.01, L2=0, seed=1)
    assert got["w"].shape == (500, 5) and got["h"].shape == (5, M.ncol)
    for key in ("w", "d", "h"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    assert got["rownames_w"] == features and len(got["cv_data"]) == 0

    cv = sa.RunNMF(A, k=[3, 5], features=features, reps=1, maxit=3, seed=1, verbose=0)
    assert cv["cv_data"].columns() == ["k", "rep", "test_error", "iter", "tol"]
    assert set(cv["cv_data"].column("k")) == {3, 5} and cv["w"].shape[0] == 500 and cv["w"].shape[1] in (3, 5)
