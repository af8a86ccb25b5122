"""The matrix ingest at its loop edges: the four upload doors, the validator, the dense image, the device transpose and
the two value transforms (log_normalize, weight_by_split), each at the sizes where its loops change path.

Every matrix reaches the hot-path kernels through sgl_upload_csc (with or without a caller's t(A)), sgl_upload_csc_list, the
A-only upload behind the one-shot entries, or sgl_upload_dense.  The hot path trusts what they let through: a row index that
slips past validate_csc_kernel is an out-of-bounds atomicAdd in the transpose's row histogram and an out-of-bounds factor
read in every accumulate.  So the refusals are checked where the kernels' loops turn -- entries 63 / 64 / 65 of a column
(the second lap of the wave; the pair (63, 64) is compared across two laps), a column past the first grid pass of
4096 x 4 waves, a value past the first grid pass of all_finite_kernel's 8192 x 256 threads -- and after every refusal the
context must be EMPTY (a refused upload leaves no matrix resident), checked in an order that fails on
`download` before any kernel could touch a refused matrix.

The transforms are held per element against a reference evaluated in np.longdouble from math.fsum column / group totals:

  log_normalize   |got - r| <= (len + 1 + L + 1) * 2^-53 * |r|,  r = log1p(x / S * scale), len the column's length:
                  len - 1 for a sum of positive terms in any order, 2 for the divide and the multiply (log1p does not
                  amplify a positive argument's relative error), L the share of the device's log1p, + 1 of slack.
                  L is MEASURED: the largest excess of err / (2^-53 |r|) over len + 1 across all cases of this file was
                  -1.151 on an MI355X -- negative: the device's log1p, the divide and the multiply together stayed
                  inside the len + 1 the sum and the two operations are given -- so, rounded up and plus one, the
                  assertion runs with L_LOG1P = ceil(-1.151) + 1 = 0, i.e. against (len + 2) * 2^-53 |r|.
  weight_by_split |got - r| <= (N_g + N_0 + 2) * 2^-53 * |r|,  r = x / (S_g / S_0), N the stored entries of a group:
                  N - 1 per positive sum in any order, one each for the two divides, 2 of slack.  Every operation is
                  correctly rounded, so nothing is measured.
"""
import functools
import math

import numpy as np
import pytest

from conftest import to_dgc

gpu = pytest.mark.gpu
U = 2.0 ** -53
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
L_LOG1P = 0          # ceil(measured L = -1.151) + 1, see the module docstring
NO_MATRIX = "no matrix resident"
CLASS_TEXT = {"range": "row index outside", "order": "not strictly ascending", "finite": "non-finite"}


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

    def copy(self):
        return Csc(self.x.copy(), self.i.copy(), self.p, self.nrow)

    def lens(self):
        return np.diff(self.p)

    def col_of_entry(self):
        return np.repeat(np.arange(self.ncol, dtype=np.int32), self.lens())

    def t(self):
        """Matrix::t of a VALID matrix: a stable sort by row keeps the columns ascending inside every row."""
        o = np.argsort(self.i, kind="stable")
        tp = np.zeros(self.nrow + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.i, minlength=self.nrow), out=tp[1:])
        return Csc(self.x[o], self.col_of_entry()[o], tp, self.ncol)

    def cols(self, c0, c1):
        s, e = int(self.p[c0]), int(self.p[c1])
        return Csc(self.x[s:e], self.i[s:e], self.p[c0:c1 + 1] - self.p[c0], self.nrow)

    def dgc(self, sa):
        return sa.dgCMatrix(self.x, self.i, self.p.astype(np.int32), (self.nrow, self.ncol))


def from_cols(nrow, rows_per_col, rng, lo=0.5, hi=20.0):
    p = np.concatenate([[0], np.cumsum([len(r) for r in rows_per_col])])
    i = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows_per_col]) if p[-1] else np.zeros(0, np.int32)
    return Csc(lo + (hi - lo) * rng.random(int(p[-1])), i, p, nrow)


def from_dense(D):
    """The CSC image of a dense matrix as `D != 0` defines it (-0.0 is dropped, a denormal kept)."""
    keep = (D != 0).T                                   # column-major walk
    p = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    return Csc(D.T[keep], np.nonzero(keep)[1], p, D.shape[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_csc(got, exp, what):
    x, i, p = got
    assert np.array_equal(p, exp.p), what + ": p"
    assert np.array_equal(i, exp.i), what + ": i"
    assert np.array_equal(bits(x), bits(exp.x)), what + ": x (bits)"


# ----------------------------------------------------------------------------------------------------------- refusals
@functools.lru_cache(maxsize=None)
def lanes_base():
    """200 rows, columns of 5, 130, 0, 7 and 3 entries: entry q of the 130-entry column is entry 5 + q of the matrix."""
    rng = np.random.default_rng(11)
    rows = [np.sort(rng.choice(200, n, replace=False)) for n in (5, 130, 0, 7, 3)]
    return from_cols(200, rows, rng)


@functools.lru_cache(maxsize=None)
def wide_base():
    """5 rows, 16384 + 5 columns of 2 or 3 entries: columns from 16384 on are the validator's second grid pass."""
    rng = np.random.default_rng(12)
    ncol = 16384 + 5
    n = 2 + (rng.random(ncol) < 0.5)
    rows = [np.sort(rng.choice(5, int(q), replace=False)) for q in n]
    return from_cols(5, rows, rng)


def position(name):
    """(valid base matrix, entry index of the defect)."""
    if name == "pass2":
        m = wide_base()
        return m, int(m.p[16384 + 2]) + 1
    m = lanes_base()
    return m, {"first": 0, "last": m.nnz - 1, "lap63": 5 + 63, "lap64": 5 + 64, "lap65": 5 + 65}[name]


POSITIONS = ("first", "last", "lap63", "lap64", "lap65", "pass2")
DEFECTS = {"eq_nrow": "range", "minus1": "range", "int_max": "range", "int_min": "range", "equal": "order", "descending": "order",
           "nan": "finite", "pinf": "finite", "ninf": "finite"}
DOORS = ("A", "At", "listA", "listAt")


def with_defect(m, e, name):
    m = m.copy()
    if DEFECTS[name] == "range":
        m.i[e] = {"eq_nrow": m.nrow, "minus1": -1, "int_max": I32_MAX, "int_min": I32_MIN}[name]
    elif DEFECTS[name] == "finite":
        m.x[e] = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}[name]
    else:   # the pair that ends at e, or that starts there when e opens its column
        c = int(np.searchsorted(m.p, e, side="right") - 1)
        assert m.p[c + 1] - m.p[c] >= 2
        a, b = (e, e + 1) if e == m.p[c] else (e - 1, e)
        if name == "equal":
            m.i[b] = m.i[a]
        else:
            m.i[a], m.i[b] = m.i[b], m.i[a]
    return m


def defect_classes(m):
    """What a correct validator reports, restated in NumPy."""
    out = set()
    if ((m.i < 0) | (m.i >= m.nrow)).any():
        out.add("range")
    inner = np.ones(m.nnz, dtype=bool)
    inner[m.p[:-1][m.lens() > 0]] = False               # the first entry of a column has no predecessor in it
    if (m.i[:-1][inner[1:]] >= m.i[1:][inner[1:]]).any():
        out.add("order")
    if not np.isfinite(m.x).all():
        out.add("finite")
    return out


def refusal_plan():
    """(door, position, defect): every defect at every position through one door, the doors dealt round-robin (a later
    chunk cannot hold entry 0 of the matrix)."""
    plan = []
    for pi, pos in enumerate(POSITIONS):
        for di, d in enumerate(DEFECTS):
            door = DOORS[(pi + di) % 4]
            if door == "listA" and pos == "first":
                door = "A"
            plan.append((door, pos, d))
    return plan


ONE_SHOT_PLAN = [(pos, d) for q, d in enumerate(DEFECTS) for pos in [POSITIONS[q % len(POSITIONS)]]]


def test_refusal_plan_covers_every_door_class_and_position():
    plan = refusal_plan()
    assert {(pos, d) for _, pos, d in plan} == {(pos, d) for pos in POSITIONS for d in DEFECTS}
    for door in DOORS:
        assert {DEFECTS[d] for dr, _, d in plan if dr == door} == {"range", "order", "finite"}, door
    assert {DEFECTS[d] for _, d in ONE_SHOT_PLAN} == {"range", "order", "finite"}
    for pos in POSITIONS:     # the defects land where the docstring says, and the restated validator sees them
        m, e = position(pos)
        c = int(np.searchsorted(m.p, e, side="right") - 1)
        assert 0 <= e < m.nnz and (pos != "pass2" or c >= 16384)
        assert (pos not in ("lap63", "lap64", "lap65")) or (m.p[c + 1] - m.p[c] == 130 and e - m.p[c] == int(pos[3:]))
        assert defect_classes(m) == set()
        for d, cls in DEFECTS.items():
            assert cls in defect_classes(with_defect(m, e, d))


def split_at_defect(m, e):
    """Two column chunks, the defect in the later one."""
    c = int(np.searchsorted(m.p, e, side="right") - 1)
    c = c if c > 0 else 1
    return [m.cols(0, c), m.cols(c, m.ncol)]


def upload_through(sa, c, door, bad, good):
    """`bad` is the matrix with the defect, `good` the same matrix without it."""
    if door == "A":
        c.upload(bad.dgc(sa), None)
    elif door == "At":      # A = t(good) is valid, the caller's t(A) carries the defect
        c.upload(good.t().dgc(sa), bad.dgc(sa))
    elif door == "listA":
        c.upload_list([q.dgc(sa) for q in split_at_defect(bad, defect_entry(bad, good))], None)
    elif door == "listAt":
        A = good.t()
        half = max(1, A.ncol // 2)
        c.upload_list([A.cols(0, half).dgc(sa), A.cols(half, A.ncol).dgc(sa)],
                      [q.dgc(sa) for q in split_at_defect(bad, defect_entry(bad, good))])
    else:
        raise AssertionError(door)


def defect_entry(bad, good):
    d = np.nonzero((bad.i != good.i) | (bits(bad.x) != bits(good.x)))[0]
    return int(d[-1])


def assert_names_classes(msg, classes):
    for cls, text in CLASS_TEXT.items():
        assert (text in msg) == (cls in classes), "%r should name exactly %s" % (msg, sorted(classes))


@pytest.fixture(scope="module")
def good_fit(sa, ora):
    """A valid matrix and the factors of two iterations on a fresh context."""
    A = ora.synth_csc(60, 50, 5)
    w0 = ora.synth_winit(4, 60)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A), None)
        c.fit_init(4, w0)
        c.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        ref = c.get_factors()
    return to_dgc(sa, A), w0, ref


def assert_empty_then_usable(sa, c, good_fit):
    """The order matters: against a library that keeps the refused matrix, `download` must be what fails -- before any
    kernel walks row indices that were just found out of range."""
    for which in (0, 1):
        with pytest.raises(sa.SingletHipError, match=NO_MATRIX):
            c.download(which)
    assert c.dims() == (0, 0, 0)
    for call in (lambda: c.fit_init(3, None), lambda: c.log_normalize(1e4),
                 lambda: c.weight_by_split(np.zeros(0, dtype=np.int32), 1), lambda: c.rasterize_rowwise(1)):
        with pytest.raises(sa.SingletHipError, match=NO_MATRIX):
            call()
    A, w0, ref = good_fit
    c.upload(A, None)
    c.fit_init(4, w0)
    c.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
    for a, b in zip(c.get_factors(), ref):
        assert np.array_equal(bits(a), bits(b))


@gpu
@pytest.mark.parametrize("door,pos,defect", refusal_plan(), ids=lambda v: str(v))
def test_refused_upload_names_the_defect_and_leaves_the_context_empty(sa, good_fit, door, pos, defect):
    good, e = position(pos)
    bad = with_defect(good, e, defect)
    with sa.Context(0) as c:
        c.upload(good_fit[0], None)          # something is resident before: the refusal must not leave IT there either
        with pytest.raises(sa.SingletHipError) as err:
            upload_through(sa, c, door, bad, good)
        assert_names_classes(str(err.value), defect_classes(bad))
        assert_empty_then_usable(sa, c, good_fit)


@gpu
@pytest.mark.parametrize("pos,defect", ONE_SHOT_PLAN, ids=lambda v: str(v))
def test_one_shot_a_only_door_refuses(sa, pos, defect):
    """sa.weight_by_split uploads through the A-only door (no transpose is built) on a context of its own."""
    good, e = position(pos)
    bad = with_defect(good, e, defect)
    sb = (np.arange(bad.ncol) % 2).astype(np.int32)
    with pytest.raises(sa.SingletHipError) as err:
        sa.weight_by_split(bad.dgc(sa), sb, 2)
    assert_names_classes(str(err.value), defect_classes(bad))


@gpu
@pytest.mark.parametrize("door", ["A", "At", "listA", "listAt"])
@pytest.mark.parametrize("pair", ["range+finite", "order+finite", "range+order"])
def test_two_defects_in_different_columns_name_both(sa, good_fit, door, pair):
    good = lanes_base()
    bad = good
    if "range" in pair:      # the LAST entry of column 0: no later entry of the column turns it into an order defect too
        bad = with_defect(bad, int(good.p[1]) - 1, "eq_nrow")
    if "order" in pair:
        bad = with_defect(bad, 5 + 64, "descending")
    if "finite" in pair:
        bad = with_defect(bad, int(good.p[3]) + 2, "nan")
    assert defect_classes(bad) == set(pair.split("+"))
    with sa.Context(0) as c:
        with pytest.raises(sa.SingletHipError) as err:
            upload_through(sa, c, door, bad, good)
        assert_names_classes(str(err.value), set(pair.split("+")))
        assert_empty_then_usable(sa, c, good_fit)


@gpu
@pytest.mark.parametrize("defect", ["eq_nrow", "descending", "nan"])
def test_team_upload_refused_on_one_rank_clears_every_rank(sa, ora, defect):
    """sgl_multi_upload_csc deals the cells out rank by rank: a defect in the LAST rank's block is met after the first rank
    has accepted its own.  No rank may keep a matrix, and the team must say so at fit_init."""
    A = ora.synth_csc(60, 50, 5)
    good = Csc(A.x, A.i, A.p, A.nrow)
    bad = with_defect(good, good.nnz - 1, defect)
    w0 = ora.synth_winit(4, 60)

    def run(M):
        M.upload(good.dgc(sa))
        M.fit_init(4, w0)
        M.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        return M.get_factors()

    with sa.Multi([0, 0]) as M:
        ref = run(M)
    with sa.Multi([0, 0]) as M:
        M.upload(good.dgc(sa))
        with pytest.raises(sa.SingletHipError) as err:
            M.upload(bad.dgc(sa))
        assert_names_classes(str(err.value), defect_classes(bad))
        for r in (1, 0):
            c = M.rank_ctx(r)
            for which in (0, 1):
                with pytest.raises(sa.SingletHipError, match=NO_MATRIX):
                    c.download(which)
            assert c.dims() == (0, 0, 0)
        with pytest.raises(sa.SingletHipError, match=NO_MATRIX):
            M.fit_init(4, w0)
        for a, b in zip(run(M), ref):
            assert np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def full_1500x1400():
    """Every entry stored: 2 100 000 values, past the 2 097 152 threads of all_finite_kernel's grid."""
    D = 0.5 + np.random.default_rng(13).random((1500, 1400))
    D.setflags(write=False)
    return D


@gpu
@pytest.mark.parametrize("door", ["sparse", "dense"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "pinf", "ninf"])
def test_non_finite_value_in_the_second_grid_pass_is_refused(sa, good_fit, door, value):
    D = full_1500x1400().copy()
    r, c_ = 1000, 1399
    assert c_ * 1500 + r >= 2097152
    D[r, c_] = value
    with sa.Context(0) as c:
        with pytest.raises(sa.SingletHipError) as err:
            if door == "dense":
                c.upload_dense(D)
            else:
                m = Csc(D.T.ravel(), np.tile(np.arange(1500, dtype=np.int32), 1400), np.arange(1401) * 1500, 1500)
                c.upload(m.dgc(sa), None)
        assert_names_classes(str(err.value), {"finite"})
        assert_empty_then_usable(sa, c, good_fit)


# ------------------------------------------------------------------------------------------------------ accepted edges
def accepted_cases():
    rng = np.random.default_rng(21)
    full = np.arange(40)
    out = {
        "nrow_1": from_cols(1, [[0], [], [0], [0], []], rng),
        "ncol_1": from_cols(9, [[1, 4, 8]], rng),
        "empty_first_middle_last": from_cols(7, [[], [0, 6], [], [], [3], []], rng),
        "full_column": from_cols(40, [[2], full, full, [39]], rng),
        "lengths_63_64_65_128_129": from_cols(130, [np.sort(rng.choice(130, n, replace=False)) for n in (63, 64, 65, 128, 129)], rng),
        # legal: the ascending test must not look across a column boundary
        "last_row_above_next_first": from_cols(10, [[5, 9], [0, 3], [9], [0], [8, 9], [0, 1]], rng),
    }
    m = from_cols(6, [[0, 2, 5], [1, 2], [4]], rng)
    m.x[:] = [-0.0, 5e-324, 1.0, -5e-324, 1e-310, -0.0]
    out["neg_zero_and_denormals"] = m
    return out


@gpu
@pytest.mark.parametrize("name", list(accepted_cases()))
def test_accepted_edges_round_trip_with_a_device_built_transpose(sa, ora, name):
    m = accepted_cases()[name]
    T = ora.transpose(ora.CSC(m.x, m.i, m.p, m.nrow, m.ncol))
    with sa.Context(0) as c:
        c.upload(m.dgc(sa), None)
        assert c.dims() == (m.nrow, m.ncol, m.nnz)
        assert_same_csc(c.download(0), m, "A")
        assert_same_csc(c.download(1), Csc(T.x, T.i, T.p, T.nrow), "t(A)")
        assert np.array_equal(c.col_counts(0), np.diff(m.p))
        assert np.array_equal(c.col_counts(1), np.diff(T.p))


@gpu
@pytest.mark.parametrize("door", ["A", "A+At", "list", "dense"])
def test_matrix_without_a_stored_entry(sa, ora, door):
    """Pinned as the library behaves: a matrix with no stored entry is accepted through every door, reads back empty in
    both orientations, goes through both transforms, and a fit on it ends where the oracle's ends (every column is empty
    on both sides: w stays the initial w, h = 0, d = 1) -- no HIP error anywhere."""
    nrow, ncol = 6, 5
    m = Csc(np.zeros(0), np.zeros(0, np.int32), np.zeros(ncol + 1, np.int64), nrow)
    w0 = ora.synth_winit(3, nrow)
    with sa.Context(0) as c:
        if door == "A":
            c.upload(m.dgc(sa), None)
        elif door == "A+At":
            c.upload(m.dgc(sa), m.t().dgc(sa))
        elif door == "list":
            c.upload_list([m.cols(0, 2).dgc(sa), m.cols(2, ncol).dgc(sa)], None)
        else:
            c.upload_dense(np.zeros((nrow, ncol)))
        assert c.dims() == (nrow, ncol, 0)
        assert_same_csc(c.download(0), m, "A")
        assert_same_csc(c.download(1), m.t(), "t(A)")
        assert not c.col_counts(0).any() and not c.col_counts(1).any()
        c.log_normalize(1e4)
        c.weight_by_split(np.array([0, 1, 1, 0, 2], dtype=np.int32), 3)
        assert c.dims() == (nrow, ncol, 0)
        c.fit_init(3, w0)
        c.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        W, d, H = c.get_factors()
    E = ora.CSC(m.x, m.i, m.p, nrow, ncol)
    ref = ora.c_nmf(E, E.t(), 0.0, 2, 0.01, 0.01, 0.0, 0.0, 0, w0)
    for got, exp, what in ((W, ref["w"], "w"), (d, ref["d"], "d"), (H, ref["h"], "h")):
        print("ingest-figure empty-matrix %s %s: got %s, oracle %s" % (door, what, np.unique(got), np.unique(exp)))
        assert np.array_equal(np.isnan(got), np.isnan(exp)), what
        fin = np.isfinite(exp)
        assert np.allclose(got[fin], exp[fin], rtol=1e-9, atol=0.0), what


# --------------------------------------------------------------------------------------------------------- dense image
def dense_patterns(nrow, ncol, rng):
    V = 0.5 + rng.random((nrow, ncol))
    r, c = np.indices((nrow, ncol))
    zero_cols = V.copy()
    zero_cols[:, [0, ncol // 2, ncol - 1]] = 0.0
    neg_zero = V.copy()
    neg_zero[(r * 3 + c) % 4 == 1] = -0.0
    den = np.where((r + 2 * c) % 3 == 0, 5e-324, np.where((r + c) % 3 == 1, -1e-310, 0.0))
    return {
        "all_nonzero": V,
        "all_zero": np.zeros((nrow, ncol)),
        "zero_columns_first_middle_last": zero_cols,
        "row_0_only": np.where(r == 0, V, 0.0),
        "last_row_only": np.where(r == nrow - 1, V, 0.0),
        "checkerboard_even": np.where((r + c) % 2 == 0, V, 0.0),     # either parity puts lane 63 behind 31 or 32 set lanes
        "checkerboard_odd": np.where((r + c) % 2 == 1, V, 0.0),
        "negative_zero_is_dropped": neg_zero,
        "denormals_are_kept": den,
    }


def check_dense_image(c, D, what):
    exp = from_dense(D)
    c.upload_dense(D)
    assert c.dims() == (D.shape[0], D.shape[1], exp.nnz), what
    assert_same_csc(c.download(0), exp, what + " A")
    assert_same_csc(c.download(1), exp.t(), what + " t(A)")
    assert np.array_equal(c.col_counts(0), exp.lens()), what


@gpu
@pytest.mark.parametrize("ncol", [1, 5])
@pytest.mark.parametrize("nrow", [1, 63, 64, 65, 127, 129])
def test_dense_image_at_the_wave_edges(sa, nrow, ncol):
    pats = dense_patterns(nrow, ncol, np.random.default_rng(31 * nrow + ncol))
    assert not np.signbit(from_dense(pats["negative_zero_is_dropped"]).x).any()
    assert from_dense(pats["denormals_are_kept"]).nnz == np.count_nonzero(pats["denormals_are_kept"])
    with sa.Context(0) as c:
        for name, D in pats.items():
            check_dense_image(c, D, "%s %dx%d" % (name, nrow, ncol))


@gpu
def test_dense_image_past_the_first_grid_pass(sa):
    """3 rows, 16384 + 3 columns: columns from 16384 on are the second pass of the count / fill grid (4096 x 4 waves)."""
    rng = np.random.default_rng(32)
    D = np.where(rng.random((3, 16384 + 3)) < 0.6, 0.5 + rng.random((3, 16384 + 3)), 0.0)
    D[:, 16384] = [0.0, 2.0, 0.0]
    D[:, 16385] = [1.0, 2.0, 3.0]
    D[:, 16386] = 0.0
    with sa.Context(0) as c:
        check_dense_image(c, D, "wide")


# ---------------------------------------------------------------------------------------------------- value transforms
TRANSFORM_MATRICES = ("lengths", "wide", "long")


@functools.lru_cache(maxsize=None)
def transform_matrix(name):
    """(A, t(A)) of one of the three matrices both transforms run on."""
    if name == "lengths":     # every column length where the wave's lap count changes, an empty column, a long one
        rng = np.random.default_rng(41)
        lens = (0, 1, 63, 64, 65, 128, 129, 1000, 129, 0, 64, 1, 1000, 65, 63, 128)
        m = from_cols(1000, [np.sort(rng.choice(1000, n, replace=False)) for n in lens], rng)
    elif name == "wide":      # 65536 + 7 columns: past the first pass of wave_blocks' 16384 x 4 waves and of expand_cols_kernel
        rng = np.random.default_rng(42)
        ncol = 65536 + 7
        keep = rng.random((ncol, 4)) < 0.6
        keep[65536:] = [[1, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1], [0, 1, 0, 0], [1, 0, 0, 1], [0, 0, 1, 0], [1, 1, 0, 1]]
        p = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
        m = Csc(0.5 + 19.5 * rng.random(int(p[-1])), np.nonzero(keep)[1], p, 4)
    else:                     # 4 500 000 stored entries: past the first pass of the by-row instance, row_hist_kernel and gather_kernel
        rng = np.random.default_rng(43)
        nrow, ncol = 3000, 1500
        m = Csc(0.5 + 19.5 * rng.random(nrow * ncol), np.tile(np.arange(nrow, dtype=np.int32), ncol), np.arange(ncol + 1) * nrow, nrow)
    t = m.t()
    for a in (m.x, m.i, m.p, t.x, t.i, t.p):
        a.setflags(write=False)
    return m, t


@functools.lru_cache(maxsize=None)
def log_normalize_reference(name, scale):
    """(r in np.longdouble, the column length of every entry)."""
    m, _ = transform_matrix(name)
    S = np.array([math.fsum(m.x[m.p[c]:m.p[c + 1]]) for c in range(m.ncol)])
    lens = m.lens()
    r = np.log1p(m.x.astype(np.longdouble) / np.repeat(S, lens).astype(np.longdouble) * np.longdouble(scale))
    return r, np.repeat(lens, lens)


def transposed_like(m, x):
    """x (in A's entry order) in t(A)'s entry order."""
    return x[np.argsort(m.i, kind="stable")]


def upload_for_transform(sa, c, name, door):
    m, t = transform_matrix(name)
    c.upload(m.dgc(sa), t.dgc(sa) if door == "given" else None)
    return m, t


@gpu
@pytest.mark.parametrize("door", ["given", "device"])
@pytest.mark.parametrize("name", TRANSFORM_MATRICES)
def test_log_normalize_per_element(sa, name, door):
    """See the module docstring for the bound.  Largest fractions of the bound (len + 1 + L_LOG1P + 1) * 2^-53 |r| on an
    MI355X: lengths 0.283, wide 0.283 (a one-entry column: 0.85 of 3), long 0.0011; the largest excess of the error over (len + 1) * 2^-53 |r|, which is
    what L measures, was -1.151 (lengths and wide; -2997.7 on the 3000-entry columns of long).  Both doors give the same bits."""
    scale = 1e4
    r, ln = log_normalize_reference(name, scale)
    with sa.Context(0) as c:
        m, t = upload_for_transform(sa, c, name, door)
        c.log_normalize(scale)
        x, i, p = c.download(0)
        xt, it, pt = c.download(1)
    assert np.array_equal(i, m.i) and np.array_equal(p, m.p) and np.array_equal(it, t.i) and np.array_equal(pt, t.p)
    assert np.array_equal(bits(xt), bits(transposed_like(m, x))), "At.x is not the transpose of A.x to the bit"
    q = (np.abs(x.astype(np.longdouble) - r) / (np.longdouble(U) * np.abs(r))).astype(np.float64)
    excess = float((q - (ln + 1)).max())
    frac = float((q / (ln + 1 + L_LOG1P + 1)).max())
    print("ingest-figure log_normalize %s %s: excess over len + 1 = %.3f, largest fraction of the bound = %.4f" % (name, door, excess, frac))
    bad = np.nonzero(q > ln + 1 + L_LOG1P + 1)[0]
    assert bad.size == 0, "entry %d (column length %d): error %.2f * 2^-53 |r|" % (bad[0], ln[bad[0]], q[bad[0]])


def weight_by_split_reference(m, sb, n_groups):
    """(r in np.longdouble, N_g + N_0 + 2 per entry, group of every entry)."""
    g = np.repeat(sb, m.lens())
    S = np.array([math.fsum(m.x[g == q]) for q in range(n_groups)]).astype(np.longdouble)
    N = np.bincount(g, minlength=n_groups)
    ratio = S / S[0]
    r = np.where(g == 0, m.x.astype(np.longdouble), m.x.astype(np.longdouble) / ratio[g])
    return r, N[g] + N[0] + 2, g


def split_labels(name, n_groups=4):
    m, _ = transform_matrix(name)
    return np.random.default_rng(51).integers(0, n_groups, m.ncol).astype(np.int32)


@gpu
@pytest.mark.parametrize("door", ["given", "device", "absent"])
@pytest.mark.parametrize("name", TRANSFORM_MATRICES)
def test_weight_by_split_per_element(sa, name, door):
    """Largest fractions of the bound (N_g + N_0 + 2) * 2^-53 |r| on an MI355X: lengths 0.0023 (an error of 2.60 * 2^-53 |r|),
    wide 0.00054 (42.8), long 0.0000024 (5.36), the same through all three doors: the column sums are trees and the group
    totals in-order sums of them, far inside a bound that holds for any order."""
    m, t = transform_matrix(name)
    sb = split_labels(name)
    r, nb, g = weight_by_split_reference(m, sb, 4)
    if door == "absent":      # the one-shot entry: A-only upload, no transpose anywhere
        out = sa.weight_by_split(m.dgc(sa), sb, 4)
        x, i, p = out.x, out.i, out.p
    else:
        with sa.Context(0) as c:
            upload_for_transform(sa, c, name, door)
            c.weight_by_split(sb, 4)
            x, i, p = c.download(0)
            xt, it, pt = c.download(1)
        assert np.array_equal(it, t.i) and np.array_equal(pt, t.p)
        assert np.array_equal(bits(xt), bits(transposed_like(m, x))), "At.x is not the transpose of A.x to the bit"
    assert np.array_equal(i, m.i) and np.array_equal(p, m.p)
    assert np.array_equal(bits(x[g == 0]), bits(m.x[g == 0])), "cells of group 0 must keep their bits"
    q = (np.abs(x.astype(np.longdouble) - r) / (np.longdouble(U) * np.abs(r))).astype(np.float64)
    print("ingest-figure weight_by_split %s %s: largest fraction of the bound = %.7f (largest error %.2f * 2^-53 |r|)"
          % (name, door, float((q / nb).max()), float(q.max())))
    bad = np.nonzero(q > nb)[0]
    assert bad.size == 0, "entry %d: error %.2f * 2^-53 |r|, bound %d" % (bad[0], q[bad[0]], nb[bad[0]])


@gpu
def test_weight_by_split_group_edges(sa, ora):
    m, t = transform_matrix("lengths")
    E = ora.CSC(m.x, m.i, m.p, m.nrow, m.ncol)
    sb = split_labels("lengths")
    with sa.Context(0) as c:
        def state():
            return [bits(a) if a.dtype == np.float64 else a for a in c.download(0) + c.download(1)]

        def reload():
            c.upload(m.dgc(sa), None)
            return state()

        before = reload()
        c.weight_by_split(np.zeros(m.ncol, dtype=np.int32), 1)          # one group: nothing to rescale
        assert all(np.array_equal(a, b) for a, b in zip(state(), before))
        # a label out of range (either side) is refused and leaves the matrix as it was
        for label in (4, -1, I32_MIN, I32_MAX):
            bad = sb.copy()
            bad[m.ncol - 1] = label
            with pytest.raises(sa.SingletHipError, match="out of range"):
                c.weight_by_split(bad, 4)
            assert all(np.array_equal(a, b) for a, b in zip(state(), before))
        # a group without cells (group 4 of 6, and the trailing group 5) changes nothing for the others
        c.weight_by_split(sb, 4)
        four = state()
        reload()
        c.weight_by_split(np.where(sb == 3, 5, sb).astype(np.int32), 6)   # the cells of group 3 now form group 5; 3 and 4 are empty
        assert all(np.array_equal(a, b) for a, b in zip(state(), four))
        # group 0 without cells: its total is 0, every ratio is x / 0 -- the oracle's own inf / NaN pattern
        reload()
        sb0 = (1 + sb % 2).astype(np.int32)
        c.weight_by_split(sb0, 3)
        x, _, _ = c.download(0)
        xt, _, _ = c.download(1)
        ref = ora.weight_by_split(E, sb0, 3)
        assert np.array_equal(x, ref.x, equal_nan=True)
        assert np.array_equal(bits(xt), bits(transposed_like(m, x)))
        # ... and with a column that has no entries alone in group 2: 0 / 0 is NaN, and nothing is there to divide by it
        reload()
        sb1 = np.where(m.lens() == 0, 2, 1).astype(np.int32)
        c.weight_by_split(sb1, 3)
        x, _, _ = c.download(0)
        assert np.array_equal(x, ora.weight_by_split(E, sb1, 3).x, equal_nan=True)
