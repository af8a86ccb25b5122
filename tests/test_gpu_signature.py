"""Signature scores on the device (sgl_signature_scores, its stage operators and the Python layer above them;
kernels_signature.hip) against the numpy restatement (signature_restatement.py).  The statistic is all integers and the
score one division and one subtraction: every comparison is array_equal, on every path (the two LDS instances, the long path
in one and in several batches) and whatever the set passes.  The matrices are the smallest at which each loop can turn
wrong; the restatement of a matrix is computed once and shared."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import signature_restatement as sr

pytestmark = pytest.mark.gpu

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = np.array([5.0, 3.0, 3.0, 1.0, 1.0, 1.0, 0.5, -0.5, -2.0, -2.0])   # a handful of levels: the runs are long
ZERO_SET = np.array([291, 293, 295, 297, 299])                               # genes the short cells of the edge matrix never store
_CACHE = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ matrices --
class Cells:
    """A matrix given cell by cell: (values, rows) with the rows ascending; stored zeros stay stored."""

    def __init__(self, m):
        self.m, self.x, self.i = m, [], []

    def add(self, x, rows):
        rows = np.asarray(rows, dtype=np.int64)
        x = np.asarray(x, dtype=np.float64)
        assert rows.shape == x.shape and (np.diff(rows) > 0).all() and (rows.size == 0 or rows[-1] < self.m)
        self.x.append(x)
        self.i.append(rows)
        return len(self.x) - 1

    def add_random(self, rng, L, values, zeros=0, avoid=None):
        """L non-zero values and `zeros` stored zeros of either sign on random rows (none of `avoid`)."""
        pool = np.arange(self.m) if avoid is None else np.setdiff1d(np.arange(self.m), avoid)
        rows = rng.choice(pool, size=L + zeros, replace=False)
        x = np.concatenate([values(rng, L), rng.choice([0.0, -0.0], size=zeros)])
        o = np.argsort(rows)
        return self.add(x[o], rows[o])

    def csc(self):
        p = np.concatenate([[0], np.cumsum([len(a) for a in self.x])]).astype(np.int64)
        return np.concatenate(self.x + [np.zeros(0)]), np.concatenate(self.i + [np.zeros(0, dtype=np.int64)]).astype(np.int32), p

    def dgc(self, sa):
        x, i, p = self.csc()
        return sa.dgCMatrix(x, i, p.astype(np.int32), (self.m, len(self.x)))

    def lens(self):
        return np.array([int(np.count_nonzero(a)) for a in self.x])


def levels(r, k):
    return r.choice(LEVELS, size=k)


def distinct(r, k):
    v = r.permutation(k).astype(np.float64) + 1.0
    v[r.random(k) < 0.3] *= -1.0
    return v


def edge_matrix():
    """64 cells of 300 genes whose stored non-zero entries number every loop edge of the gather, the sort and the walk."""
    if "edge" not in _CACHE:
        rng = np.random.default_rng(30)
        m = 300
        g = Cells(m)
        Ls = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
        for q in range(64):
            L = Ls[q % len(Ls)]
            g.add_random(rng, L, levels if q % 3 else distinct, zeros=min(int(rng.integers(0, 4)), m - L, 290 - L if L < 200 else m),
                         avoid=ZERO_SET if L < 200 else None)
        _CACHE["edge"] = g
    return _CACHE["edge"]


def reference_ranks(key, g, R):
    k = ("ranks", key, R)
    if k not in _CACHE:
        x, _, p = g.csc()
        _CACHE[k] = sr.matrix_cell_ranks(x, p, g.m, R)
    return _CACHE[k]


def reference_scores(key, g, sets, R):
    k = ("scores", key, R, len(sets))
    if k not in _CACHE:
        x, i, p = g.csc()
        _CACHE[k] = sr.scores(x, i, p, g.m, sets, R)
    return _CACHE[k]


def check_info(info, g, lds_cap=0, batch=0, n_sets=0, pass_sets=0):
    """sgl_signature_info reports the paths the restatement's plan gives."""
    small, large, long_ = sr.split_paths(g.lens(), lds_cap)
    cut = sr.batches(g.lens()[long_], batch) if long_.size else [0]
    want = {"lds_small": small.size, "lds_large": large.size, "long_cells": long_.size, "batches": len(cut) - 1,
            "passes": sr.passes(n_sets, pass_sets) if n_sets else 0, "lds_cap": sr.lds_cap(lds_cap), "batch_cap": sr.batch_cap(batch),
            "pass_sets": sr.pass_size(pass_sets) if n_sets else 0}
    assert info == want
    return want


# ---------------------------------------------------------------------------------------------------- the rank operator --
@pytest.mark.parametrize("lds_cap, batch", [(0, 0), (64, 0), (64, 200)], ids=["lds", "long", "long in batches"])
def test_cell_ranks_equal_the_restatement(sa, ctx, lds_cap, batch):
    g = edge_matrix()
    R = 100
    ctx.upload(g.dgc(sa))
    entry, zero2 = ctx.op_cell_ranks(R, lds_cap, batch)
    want_entry, want_zero2 = reference_ranks("edge", g, R)
    assert np.array_equal(zero2, want_zero2) and np.array_equal(entry, want_entry)
    info = check_info(ctx.signature_info(), g, lds_cap, batch)
    if lds_cap == 0:
        assert info["lds_small"] == 64 and info["long_cells"] == 0
    else:
        assert info["long_cells"] == int((g.lens() > 64).sum()) > 0 and info["lds_large"] == 0
        assert info["batches"] == 1 if batch == 0 else info["batches"] > 10
    if batch:   # cells that are a batch of their own among them
        assert (g.lens() > batch).sum() >= 4
    for R2 in (1, 300):   # max_rank at both ends of its range
        e2, z2 = ctx.op_cell_ranks(R2, lds_cap, batch)
        w = reference_ranks("edge", g, R2)
        assert np.array_equal(e2, w[0]) and np.array_equal(z2, w[1])


def caps_matrix():
    if "caps" not in _CACHE:
        rng = np.random.default_rng(31)
        g = Cells(sr.LDS_CAP + 70)
        for L in (sr.LDS_SMALL - 1, sr.LDS_SMALL, sr.LDS_SMALL + 1, sr.LDS_CAP - 1, sr.LDS_CAP, sr.LDS_CAP + 1):
            g.add_random(rng, L, levels if L % 2 else distinct, zeros=3)
        _CACHE["caps"] = g
    return _CACHE["caps"]


def test_at_the_real_caps(sa, ctx):
    g = caps_matrix()
    R = 1500
    rng = np.random.default_rng(32)
    sets = [rng.choice(g.m, size=k, replace=False) for k in (1, 10, 200, 1500)]
    ctx.upload(g.dgc(sa))
    entry, zero2 = ctx.op_cell_ranks(R)
    want = reference_ranks("caps", g, R)
    assert np.array_equal(entry, want[0]) and np.array_equal(zero2, want[1])
    info = check_info(ctx.signature_info(), g)
    assert (info["lds_small"], info["lds_large"], info["long_cells"], info["batches"]) == (2, 3, 1, 1)
    rank2, score = ctx.signature_scores(sets, R, return_rank2=True)
    w2, ws = reference_scores("caps", g, sets, R)
    assert np.array_equal(rank2, w2) and np.array_equal(score, ws)
    check_info(ctx.signature_info(), g, n_sets=4)


def test_runs_at_every_edge_of_the_long_path(sa, ctx):
    """m = 2200: a cell of 2100 equal values, runs that end at the sorted positions 1023, 1024 and 1025 (positive and
    negative), and one run that spans the whole cell, on the long path in one batch, in batches of one cell, and in LDS."""
    m = 2200
    rng = np.random.default_rng(33)
    g = Cells(m)
    rows = lambda L: np.sort(rng.choice(m, size=L, replace=False))
    g.add(np.full(2100, 2.5), rows(2100))
    for end in (1023, 1024, 1025):
        v = np.arange(2100, 0, -1).astype(np.float64)                            # descending: sorted position j holds 2100 - j
        v[990:end] = v[990]                                                      # the run [990, end)
        v[1500:2048] = v[1500]
        g.add(v[rng.permutation(2100)], rows(2100))
        g.add(-v[rng.permutation(2100)], rows(2100))                             # all negative: P = 0, the run mirrored
    g.add(np.full(m, -1.0), np.arange(m))                                        # one run that spans the whole cell, Z = 0
    g.add(np.full(m, 7.0), np.arange(m))
    n = len(g.x)
    sets = [np.arange(m), rng.choice(m, size=1500, replace=False), np.array([0]), rng.choice(m, size=40, replace=False)]
    ctx.upload(g.dgc(sa))
    x, i, p = g.csc()
    for R in (1500, m, 1024):
        want = sr.matrix_cell_ranks(x, p, m, R)
        use = [s for s in sets if len(s) <= R]
        w2, ws = sr.scores(x, i, p, m, use, R)
        for lds_cap, batch in ((64, 0), (64, 2100), (0, 0)):
            entry, zero2 = ctx.op_cell_ranks(R, lds_cap, batch)
            assert np.array_equal(entry, want[0]) and np.array_equal(zero2, want[1])
            rank2, score = ctx.op_signature_scores(use, R, lds_cap, batch)
            assert np.array_equal(rank2, w2) and np.array_equal(score, ws)
            info = check_info(ctx.signature_info(), g, lds_cap, batch, n_sets=len(use))
            assert info["long_cells"] == (n if lds_cap else 0) and info["lds_large"] == (0 if lds_cap else n)
            assert info["batches"] == (0 if not lds_cap else (n if batch else 1))


def test_cap_edges(sa, ctx):
    """Runs whose midrank is R - 0.5, R, R + 0.5 and R + 1; the zero block straddling R, wholly above and wholly below it;
    negatives behind it.  m = 40, R = 10."""
    m, R = 40, 10
    g = Cells(m)
    top = lambda k: list(np.arange(100.0, 100.0 - k, -1.0))
    g.add(top(8) + [1.0, 1.0] + [-1.0], np.arange(11))            # run [8, 10): midrank 9.5 = R - 0.5; zero block [10, 39) above R
    g.add(top(8) + [1.0, 1.0, 1.0] + [-1.0], np.arange(12))       # run [8, 11): midrank 10 = R: kept
    g.add(top(8) + [1.0] * 4 + [-1.0], np.arange(13))             # run [8, 12): midrank 10.5 = R + 0.5: capped
    g.add(top(8) + [1.0] * 5 + [-1.0, -1.0], np.arange(15))       # run [8, 13): midrank 11 = R + 1
    g.add(top(9) + [1.0], np.arange(10))                          # position 9: rank 10 = R, untied; the zero block starts at R
    g.add(top(3) + [-1.0, -2.0, -2.0], np.arange(6))              # zero block [3, 37): straddles R; the negatives behind it
    g.add(top(3) + [-1.0] * 34, np.arange(37))                    # zero block [3, 6): wholly below R; a negative run across R
    g.add(top(3) + [-3.0], [0, 5, 9, 39])                         # zero block [3, 39)
    g.add(top(4) + list(-np.arange(1.0, 36.0)), np.arange(39))    # zero block of ONE gene at position 4, below R
    g.add([0.0, -0.0, 4.0], [2, 3, 4])                            # stored zeros join the zero block
    g.add(top(20), np.arange(20, 40))                             # the zero block wholly above R, no negatives
    g.add(list(-np.arange(1.0, 41.0)), np.arange(40))             # P = 0, Z = 0
    sets = [np.arange(10), np.arange(8, 13), np.array([39]), np.arange(30, 40), np.arange(3, 9), np.array([2, 3, 4, 20])]
    x, i, p = g.csc()
    want = sr.matrix_cell_ranks(x, p, m, R)
    assert want[0][p[0] + 8] == 19 and want[0][p[1] + 8] == 20 and want[0][p[2] + 8] == 22 and want[0][p[3] + 8] == 22
    assert want[1][0] == 22 and want[1][6] == 2 * 3 + 3 + 1 and want[1][11] == 0
    w2, ws = sr.scores(x, i, p, m, sets, R)
    ctx.upload(g.dgc(sa))
    for lds_cap in (0, 1):
        entry, zero2 = ctx.op_cell_ranks(R, lds_cap)
        assert np.array_equal(entry, want[0]) and np.array_equal(zero2, want[1])
        rank2, score = ctx.op_signature_scores(sets, R, lds_cap)
        assert np.array_equal(rank2, w2) and np.array_equal(score, ws)
        check_info(ctx.signature_info(), g, lds_cap, n_sets=len(sets))
    assert ctx.signature_info()["long_cells"] == int((g.lens() > 1).sum()) == 11


# ----------------------------------------------------------------------------------------------------------------- sets --
def sets_for(n_sets, m, R):
    """Sets of every kind: all m genes (when R = m), n_s = R, sizes 1, the set wholly in the short cells' zero block; gene 7
    is in every set but that one and the all-genes set holds it anyway."""
    rng = np.random.default_rng(40 + n_sets)
    out = [np.arange(m) if R == m else rng.permutation(m)[:R]]
    kinds = (lambda: np.array([7]), lambda: ZERO_SET, lambda: np.concatenate([[7], np.setdiff1d(rng.permutation(m)[:R], [7])[:R - 1]]),
             lambda: np.concatenate([[7], np.setdiff1d(rng.choice(m, size=int(rng.integers(1, 30)), replace=False), [7])]))
    while len(out) < n_sets:
        out.append(kinds[len(out) % 4 if len(out) < 5 else 3]())
    return [np.asarray(s, dtype=np.int32) for s in out[:n_sets]]


@pytest.mark.parametrize("n_sets", [1, 2, 63, 64, 65, sr.PASS_SETS, sr.PASS_SETS + 1])
def test_sets_of_every_kind_and_number(sa, ctx, n_sets):
    g = edge_matrix()
    m = R = g.m
    sets = sets_for(n_sets, m, R)
    assert len(sets[0]) == m and (n_sets < 5 or (np.array_equal(sets[1], ZERO_SET) and len(sets[2]) == R and len(sets[4]) == 1))
    assert all(7 in s for j, s in enumerate(sets) if j != 1)   # a gene that is in every set but the zero block's
    if n_sets > 1:   # the set of the zero block is wholly in it for the short cells
        x, i, p = g.csc()
        assert any(not np.isin(i[p[c]:p[c + 1]], ZERO_SET).any() for c in range(len(g.x)))
    ctx.upload(g.dgc(sa))
    rank2, score = ctx.signature_scores(sets, R, return_rank2=True)
    w2, ws = reference_scores("edge", g, sets, R)
    assert np.array_equal(rank2, w2) and np.array_equal(score, ws)
    info = check_info(ctx.signature_info(), g, n_sets=n_sets)
    assert info["passes"] == (2 if n_sets > sr.PASS_SETS else 1)
    # the long path and small passes give the same bits
    r3, s3 = ctx.op_signature_scores(sets, R, 64, 200, 64 if n_sets > 2 else 1)
    assert np.array_equal(r3, w2) and np.array_equal(s3, ws)
    info = check_info(ctx.signature_info(), g, 64, 200, n_sets, 64 if n_sets > 2 else 1)
    assert info["passes"] == -(-n_sets // (64 if n_sets > 2 else 1))


# -------------------------------------------------------------------------------------------- forms, fits, dense upload --
def test_the_forms_give_identical_bits(sa, ctx):
    g = edge_matrix()
    A = g.dgc(sa)
    R = 120
    sets = sets_for(9, g.m, R)
    w2, ws = reference_scores("edge", g, sets, R)
    ctx.upload(A)
    a = ctx.signature_scores(sets, R, return_rank2=True)
    assert np.array_equal(a[0], w2) and np.array_equal(a[1], ws)
    forms = {"again": ctx.signature_scores(sets, R, return_rank2=True), "one-shot": sa.c_signature_scores(A, sets, R, return_rank2=True)}
    x, i, p = g.csc()
    S = sp.csc_matrix((x, i, p), shape=(g.m, len(g.x)))
    with sa.Context(0) as c:
        c.upload_dense(S.toarray())
        forms["dense"] = c.signature_scores(sets, R, return_rank2=True)
        assert c.signature_info()["lds_small"] == 64            # the CSC image that upload keeps
        c.upload_native(sa.native(S.astype(np.float32).tocsr()))
        forms["native"] = c.signature_scores(sets, R, return_rank2=True)
    for lds_cap, batch, pass_sets in ((64, 0, 0), (1, 200, 2), (128, 1, 1), (0, 0, 4), (5000, 1 << 40, 5000)):
        forms["knobs %d %d %d" % (lds_cap, batch, pass_sets)] = ctx.op_signature_scores(sets, R, lds_cap, batch, pass_sets)
    for name, f in forms.items():
        assert same_bits(f[0], a[0]) and same_bits(f[1], a[1]), name
    # either output may be NULL
    only_score = ctx.signature_scores(sets, R)
    assert same_bits(only_score, a[1])
    from singlet_amd._marshal import signature_sets
    sp_, sg = signature_sets(sets)
    r2 = np.zeros((len(g.x), len(sets)), dtype=np.uint64)
    L = sa._lib.load()
    rc = L.sgl_signature_scores(ctx._h, sp_.ctypes.data_as(C.POINTER(C.c_int64)), sg.ctypes.data_as(C.POINTER(C.c_int32)), len(sets), R,
                                r2.ctypes.data_as(C.POINTER(C.c_uint64)), None)
    assert rc == 0 and same_bits(r2.T, a[0])
    assert L.sgl_signature_scores(ctx._h, sp_.ctypes.data_as(C.POINTER(C.c_int64)), sg.ctypes.data_as(C.POINTER(C.c_int32)), len(sets), R, None, None) == 0


def _same(fa, fb, what):
    for x, y in zip(fa, fb):
        assert same_bits(x, y), what


def test_a_fit_continued_after_a_call_gives_the_same_bits(sa):
    m, n, k = 400, 3000, 8     # cells of about 100 entries
    sets = [np.arange(0, 30), np.arange(20, 300), np.array([399])]
    runs = {}
    for with_call in (False, True):
        with sa.Context(0) as c:
            c.synth(m, n, 4)
            c.fit_init(k)
            c.sweeps_get(reset=True)
            tols = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            if with_call:
                before = c.get_factors()
                x0 = c.download(0)
                a = c.signature_scores(sets, 300, return_rank2=True)
                b = c.op_signature_scores(sets, 300, lds_cap=64, max_batch_entries=1000, pass_sets=1)
                c.op_cell_ranks(300, 64)
                _same(a, b, "paths")
                _same(c.get_factors(), before, "factors")
                _same(c.download(0), x0, "matrix")
                assert a[1].shape == (3, n) and c.signature_info()["long_cells"] > 0
            tols += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            runs[with_call] = (c.get_factors(), tols, c.sweeps_get(reset=True))
    _same(runs[True][0], runs[False][0], "fit")
    assert runs[True][1] == runs[False][1]
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], key


# ----------------------------------------------------------------------------------------------------------- refusals --
def test_refusals_return_their_code_and_leave_the_context_usable(sa):
    g = edge_matrix()
    A = g.dgc(sa)
    m, R = g.m, 50
    sets = sets_for(5, m, R)
    w2, ws = reference_scores("edge", g, sets, R)

    def refused(c, match, fn):
        dims = c.dims()
        with pytest.raises(sa.SingletHipError, match=match) as e:
            fn()
        assert e.value.code == EINVAL and c.dims() == dims

    with sa.Context(0) as c:
        refused(c, "no matrix resident", lambda: c.signature_scores(sets, R))
        refused(c, "no matrix resident", lambda: c.op_cell_ranks(R))
        refused(c, "no matrix resident", lambda: c.op_signature_scores(sets, R))
        c.upload(A)
        refused(c, "n_sets = 0", lambda: c.signature_scores([], R))
        refused(c, "set 1 is empty", lambda: c.signature_scores([[1], [], [2]], R))
        refused(c, r"set_genes\[2\] = 300 is outside \[0, 300\)", lambda: c.signature_scores([[1, 2], [300]], R))
        refused(c, r"set_genes\[1\] = -1 is outside", lambda: c.signature_scores([[1, -1], [300]], R))
        refused(c, r"set_genes\[3\] = 5 occurs twice", lambda: c.signature_scores([[5], [5, 6, 5]], R))
        refused(c, "set 1 holds 51 genes, more than max_rank = 50", lambda: c.signature_scores([[5], np.arange(51)], R))
        refused(c, r"max_rank = 0 is outside \[1, 300\]", lambda: c.signature_scores(sets, 0))
        refused(c, r"max_rank = 301 is outside \[1, 300\]", lambda: c.signature_scores(sets, 301))
        refused(c, "max_rank = 301", lambda: c.op_cell_ranks(301))
        refused(c, "lds_cap = -1 is negative", lambda: c.op_cell_ranks(R, -1))
        refused(c, "max_batch_entries = -5 is negative", lambda: c.op_cell_ranks(R, 0, -5))
        refused(c, "lds_cap = -1 is negative", lambda: c.op_signature_scores(sets, R, -1))
        refused(c, "max_batch_entries = -2 is negative", lambda: c.op_signature_scores(sets, R, 0, -2))
        refused(c, "pass_sets = -3 is negative", lambda: c.op_signature_scores(sets, R, 0, 0, -3))
        # the first defect is named: the rank before the sets, a size before a gene
        refused(c, "max_rank = 0", lambda: c.signature_scores([[], [999]], 0))
        refused(c, "set 1 is empty", lambda: c.signature_scores([[999], []], R))
        L = sa._lib.load()
        assert L.sgl_signature_scores(c._h, None, None, 1, R, None, None) == EINVAL and b"NULL" in L.sgl_last_error()
        assert L.sgl_signature_info(c._h, None) == EINVAL
        bad_ptr = np.array([1, 2], dtype=np.int64)
        gene = np.zeros(2, dtype=np.int32)
        assert L.sgl_signature_scores(c._h, bad_ptr.ctypes.data_as(C.POINTER(C.c_int64)), gene.ctypes.data_as(C.POINTER(C.c_int32)), 1, R,
                                      None, None) == EINVAL and b"set_ptr[0] = 1" in L.sgl_last_error()
        rank2, score = c.signature_scores(sets, R, return_rank2=True)      # the context is usable
        assert np.array_equal(rank2, w2) and np.array_equal(score, ws)
    with sa.Multi([0, 0]) as M:
        M.upload(A)
        with pytest.raises(sa.SingletHipError, match="team") as e:
            M.rank_ctx(0).signature_scores(sets, R)
        assert e.value.code == EINVAL
        with pytest.raises(sa.SingletHipError, match="team") as e:
            M.rank_ctx(1).op_cell_ranks(R)
        assert e.value.code == EINVAL
    # the one-shot form refuses its arguments before anything is uploaded
    with pytest.raises(sa.SingletHipError, match=r"set_genes\[3\] = 5 occurs twice") as e:
        sa.c_signature_scores(A, [[5], [5, 6, 5]], R)
    assert e.value.code == EINVAL
    with pytest.raises(sa.SingletHipError, match="max_rank = 1500") as e:
        sa.c_signature_scores(A, sets)
    assert e.value.code == EINVAL


# -------------------------------------------------------------------------------------------------------------- pbmc3k --
def _pbmc3k(sa):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)          # row indices are stored as within-column deltas
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    return sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))


SIGNATURES = {"B": ["CD79A", "MS4A1", "CD79B"], "NK": ["GNLY", "NKG7", "GZMB"], "Platelet": ["PPBP", "PF4"], "DC": ["FCER1A", "CST3"],
              "T": ["CD3D", "CD3E", "CD2"], "Mono": ["LYZ", "CD14", "S100A9", "FCGR3A"]}
ANCHOR = {"B": {4}, "NK": {7}, "Platelet": {9}, "DC": {8}, "T": {1, 2, 5}, "Mono": {3, 6}}


def test_pbmc3k_anchor_and_normalisation(sa):
    """The cell types with the highest mean score per signature are those of the CPU probe (max_rank = 1500, cells without a
    type left out); only the argmax sets are asserted.  The scores of the counts equal those of the log-normalised matrix."""
    A = _pbmc3k(sa)
    names = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_names.npz"))
    genes, ct = names["genes"], names["cell_type"]
    with sa.Context(0) as c:
        c.upload(A)
        res = sa.score_signatures(c, SIGNATURES, gene_names=genes, max_rank=1500)
        info = c.signature_info()
        assert info["lds_small"] + info["lds_large"] == A.ncol and info["lds_large"] > 0 and info["long_cells"] == 0 and info["passes"] == 1
        assert res["names"] == list(SIGNATURES) and res["dropped"] == {} and res["scores"].shape == (A.ncol, 6)
        c.log_normalize()
        after = sa.score_signatures(c, SIGNATURES, gene_names=genes, max_rank=1500)
        assert same_bits(after["scores"], res["scores"])
    assert same_bits(sa.score_signatures(A, SIGNATURES, gene_names=genes)["scores"], res["scores"])   # the one-shot door
    for j, name in enumerate(res["names"]):
        mean = np.array([res["scores"][ct == t, j].mean() for t in range(1, 10)])
        k = len(ANCHOR[name])
        top = set((np.argsort(-mean)[:k] + 1).tolist())
        print(name, np.round(mean, 3).tolist())
        assert top == ANCHOR[name], (name, mean)
    # a negative set lowers the score and the result stays in [0, 1]
    neg = sa.score_signatures(A, {"T_not_B": ["CD3D", "CD3E", "CD2", "MS4A1-", "CD79A-"]}, gene_names=genes)["scores"][:, 0]
    assert neg.min() >= 0.0 and (neg <= res["scores"][:, 4]).all() and (neg < res["scores"][:, 4]).any()
