"""The typed upload door (sgl_upload_typed, Context.upload_native, native()) on the GPU.

The expected side is always the existing door: sgl_upload_csc of the same matrix converted to double / int32, sorted and
(for gene-major arrays) transposed with NumPy on the host.  Both resident orientations are read back with download(0) /
download(1) and compared as tests/test_gpu_ingest.py compares them: p, i, and x by bits.  Sizes are the smallest at which
each loop can go wrong: the base of the ingest tests (200 rows, columns of 5, 130, 0, 7 and 3 entries), one column past
the validator's and the mark kernel's first pass of 4096 x 4 waves, one entry past the convert kernels' first pass of
8192 x 256 elements, the wave laps 63 / 64 / 65, and the LDS sort's capacity (read from the report) - 1, + 0, + 1 and x 3.
After every refusal the context must be empty: `download` must raise "no matrix resident" first.  DEVICE space goes
through torch tensors; the first such case of a process also pays torch's one-time device initialisation.
"""
import ctypes as C
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu
NO_MATRIX = "no matrix resident"
CLASS_TEXT = {"range": "row index outside", "order": "not strictly ascending", "finite": "non-finite", "inexact": "inexact"}
DUPLICATES = "duplicate entries are not summed"
F64, F32, I32, I64 = 0, 1, 2, 3
NP_OF = {F64: np.float64, F32: np.float32, I32: np.int32, I64: np.int64}
PASS_ELEMENTS = 8192 * 256          # one grid pass of a convert kernel
PASS_SLICES = 4096 * 4              # one grid pass of the validator and of the mark kernel


class Csc:
    """CSC slots in NumPy (x double, i int32, p int64): columns are the major slices."""

    def __init__(self, x, i, p, nrow):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.i = np.ascontiguousarray(i, dtype=np.int32)
        self.p = np.ascontiguousarray(p, dtype=np.int64)
        self.nrow, self.ncol = int(nrow), int(self.p.shape[0] - 1)

    @property
    def nnz(self):
        return int(self.p[-1])

    def col_of_entry(self):
        return np.repeat(np.arange(self.ncol, dtype=np.int32), np.diff(self.p))

    def sorted(self):
        """Every column's (index, value) pairs in ascending index: the canonical form of the same matrix."""
        o = np.lexsort((self.i, self.col_of_entry()))
        return Csc(self.x[o], self.i[o], self.p, self.nrow)

    def t(self):
        o = np.argsort(self.i, kind="stable")
        tp = np.zeros(self.nrow + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.i, minlength=self.nrow), out=tp[1:])
        return Csc(self.x[o], self.col_of_entry()[o], tp, self.ncol)

    def out_of_order_columns(self):
        """Lengths of the columns in which some index is below its predecessor."""
        bad = np.zeros(self.nnz, dtype=bool)
        bad[1:] = self.i[1:] < self.i[:-1]
        bad[self.p[:-1][np.diff(self.p) > 0]] = False
        cols = np.unique(self.col_of_entry()[bad])
        return np.diff(self.p)[cols]


def from_cols(nrow, rows_per_col, values):
    p = np.concatenate([[0], np.cumsum([len(r) for r in rows_per_col])])
    i = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows_per_col]) if p[-1] else np.zeros(0, np.int32)
    return Csc(values[:int(p[-1])], i, p, nrow)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_csc(got, exp, what):
    x, i, p = got
    assert np.array_equal(p, exp[2]), what + ": p"
    assert np.array_equal(i, exp[1]), what + ": i"
    assert np.array_equal(bits(x), bits(exp[0])), what + ": x (bits)"


def existing_door(sa, A):
    """(download(0), download(1)) after sgl_upload_csc of the canonical genes x cells matrix A."""
    with sa.Context(0) as c:
        c.upload(sa.dgCMatrix(A.x, A.i, A.p.astype(np.int32), (A.nrow, A.ncol)), None)
        return c.download(0), c.download(1)


def assert_state(c, exp, what):
    assert c.dims() == (exp[1][2].shape[0] - 1, exp[0][2].shape[0] - 1, exp[0][0].shape[0]), what
    assert_same_csc(c.download(0), exp[0], what + " A")
    assert_same_csc(c.download(1), exp[1], what + " t(A)")


def assert_empty(sa, c):
    for which in (0, 1):
        with pytest.raises(sa.SingletHipError, match=NO_MATRIX):
            c.download(which)
    assert c.dims() == (0, 0, 0)


def assert_names_classes(msg, classes):
    for cls, text in CLASS_TEXT.items():
        assert (text in msg) == (cls in classes), "%r should name exactly %s" % (msg, sorted(classes))


def to_space(a, space, misalign=False):
    """HOST: the NumPy array itself.  DEVICE: a torch tensor on cuda:0; misalign: one element past an aligned start, so
    the convert kernels take their one-element-per-thread form."""
    if space == "host":
        return a
    import torch
    if misalign:
        return torch.from_numpy(np.concatenate([a[:1], a])).to("cuda:0")[1:]
    return torch.from_numpy(a).to("cuda:0")


def typed(sa, M, major_is_genes, xt=F64, it=I32, pt=I32, space="host", misalign=False):
    """The NativeMatrix of the arrays of M (its columns are the major slices) in the given types."""
    arr = [to_space(np.ascontiguousarray(a, dtype=NP_OF[t]), space, misalign) for a, t in ((M.x, xt), (M.i, it), (M.p, pt))]
    if major_is_genes:      # the columns of M are genes: M is the CSC of t(A), the CSR of the genes x cells A
        return sa.native((arr[0], arr[1], arr[2], (M.ncol, M.nrow), "csr"))
    return sa.native((arr[0], arr[1], arr[2], (M.nrow, M.ncol), "csc"))


def raw_upload(sa, c, x, xt, i, it, p, pt, n_major, n_minor, mig, space=0, flags=1):
    from singlet_amd import _lib
    rep = np.zeros(8, dtype=np.int64)
    rc = _lib.load().sgl_upload_typed(c._h, C.c_void_p(x.ctypes.data), xt, C.c_void_p(i.ctypes.data), it, C.c_void_p(p.ctypes.data), pt,
                                      n_major, n_minor, mig, space, flags, 0, 0, _lib.ptr(rep, _lib.i64p))
    return rc, rep


# -------------------------------------------------------------------------------------------------------- the bases
@functools.lru_cache(maxsize=None)
def lanes_base():
    """200 rows, columns of 5, 130, 0, 7 and 3 entries; integer values 1 .. 20: exact in every value type."""
    rng = np.random.default_rng(11)
    rows = [np.sort(rng.choice(200, n, replace=False)) for n in (5, 130, 0, 7, 3)]
    return from_cols(200, rows, rng.integers(1, 21, 145).astype(np.float64))


@functools.lru_cache(maxsize=None)
def expected(sa, name):
    """name -> (the canonical genes x cells matrix, the existing door's resident state for it); computed once."""
    A = {"lanes": lanes_base, "one_entry_columns": one_entry_columns, "long_column": long_column, "sort": lambda: sort_case(sa)[0].sorted(),
         "wide_sort": lambda: wide_sort_case().sorted()}[name]()
    return A, existing_door(sa, A)


def expected_for(sa, name, mig):
    """With gene-major arrays the canonical matrix S is t(A): A = t(S), and the state is (A, S) instead of (S, t(S))."""
    S, st = expected(sa, name)
    if not mig:
        return st
    key = name + "/t"
    if key not in _T_CACHE:
        _T_CACHE[key] = existing_door(sa, S.t())
    return _T_CACHE[key]


_T_CACHE = {}


# -------------------------------------------------------------------------------------------- 1. every type combination
@gpu
@pytest.mark.parametrize("space", ["host", "device", "device_misaligned"])
@pytest.mark.parametrize("mig", [0, 1])
def test_every_type_combination_is_bit_for_bit_the_f64_door(sa, mig, space):
    M = lanes_base()
    exp = expected_for(sa, "lanes", mig)
    with sa.Context(0) as c:
        for xt in (F64, F32, I32, I64):
            for it in (I32, I64):
                for pt in (I32, I64):
                    N = typed(sa, M, mig, xt, it, pt, space.split("_")[0], space.endswith("misaligned"))
                    assert N.space == (0 if space == "host" else 1) and N.major_is_genes == mig
                    rep = c.upload_native(N)
                    what = "x %d idx %d ptr %d" % (xt, it, pt)
                    assert_state(c, exp, what)
                    size = {F64: 8, F32: 4, I32: 4, I64: 8}
                    assert rep == dict(nnz=145, sorted_lds=0, sorted_long=0, integral=1, lds_capacity=rep["lds_capacity"],
                                       bytes_copied=145 * (size[xt] + size[it]) + (M.ncol + 1) * size[pt]), what
                    assert rep["lds_capacity"] >= 256 and 2 * 8 * rep["lds_capacity"] <= 160 * 1024


@gpu
def test_cpu_tensor_travels_as_host_and_fractions_are_reported(sa):
    import torch
    M = lanes_base()
    half = Csc(M.x * 0.5, M.i, M.p, M.nrow)
    A, st = expected(sa, "lanes")
    N = sa.native((torch.from_numpy(half.x.astype(np.float32)), torch.from_numpy(M.i.astype(np.int64)), torch.from_numpy(M.p), (200, 5), "csc"))
    assert N.space == 0 and N.device is None
    with sa.Context(0) as c:
        rep = c.upload_native(N)
        assert rep["integral"] == 0
        x, i, p = c.download(0)
        assert np.array_equal(bits(x), bits(half.x)) and np.array_equal(i, st[0][1]) and np.array_equal(p, st[0][2])
        N.device = 1                   # as if the tensors lived on another GPU: refused before the call, nothing is touched
        N.space = 1
        with pytest.raises(ValueError, match="GPU"):
            c.upload_native(N)
        assert c.dims() == (200, 5, 145)
        zeros = Csc(np.where(np.arange(145) % 3 == 0, 0.0, M.x), M.i, M.p, M.nrow)   # explicit zeros stay stored
        c.upload_native(typed(sa, zeros, 0, F32))
        x, i, p = c.download(0)
        assert np.array_equal(bits(x), bits(zeros.x)) and c.dims() == (200, 5, 145)


# ------------------------------------------------------------------------------------------------------ 2. grid edges
@functools.lru_cache(maxsize=None)
def one_entry_columns():
    """16 385 columns of one entry each: the last column is the second pass of the validator's 4096 x 4 waves."""
    n = PASS_SLICES + 1
    return Csc(1.0 + np.arange(n) % 7, np.arange(n) % 5, np.arange(n + 1), 5)


@functools.lru_cache(maxsize=None)
def long_column():
    """One column of 2 097 153 entries: the last entry is one past the convert kernels' first pass."""
    n = PASS_ELEMENTS + 1
    return Csc(1.0 + np.arange(n) % 11, np.arange(n), [0, n], n)


@gpu
@pytest.mark.parametrize("space", ["host", "device", "device_misaligned"])
def test_one_entry_past_the_convert_kernels_first_pass(sa, space):
    """I64 -> F64 and I64 -> I32 both run at 2 097 153 entries; misaligned: the one-element form, whose first pass ends at
    the same entry."""
    M = long_column()
    exp = expected_for(sa, "long_column", 0)
    with sa.Context(0) as c:
        rep = c.upload_native(typed(sa, M, 0, I64, I64, I64, space.split("_")[0], space.endswith("misaligned")))
        assert rep["nnz"] == PASS_ELEMENTS + 1 and rep["integral"] == 1
        assert_state(c, exp, "long column")


@gpu
@pytest.mark.parametrize("mig", [0, 1])
def test_one_slice_past_the_validators_first_pass(sa, mig):
    M = one_entry_columns()
    with sa.Context(0) as c:
        c.upload_native(typed(sa, M, mig, F32, I64, I32))
        assert_state(c, expected_for(sa, "one_entry_columns", mig), "16385 slices")
        bad = Csc(M.x, M.i.copy(), M.p, M.nrow)
        bad.i[PASS_SLICES] = 5                                    # the defect sits in the second pass
        with pytest.raises(sa.SingletHipError) as err:
            c.upload_native(typed(sa, bad, mig, F32, I32, I32))
        assert_names_classes(str(err.value), {"range"})
        assert_empty(sa, c)


# ------------------------------------------------------------------------------------------------------------ 3. sort
@functools.lru_cache(maxsize=None)
def lds_capacity(sa):
    with sa.Context(0) as c:
        return c.upload_native(typed(sa, lanes_base(), 0))["lds_capacity"]


@functools.lru_cache(maxsize=None)
def sort_case(sa):
    """Columns of length 1, 2, 3, 63, 64, 65, 130, cap - 1, cap, cap + 1 and 3 cap, each three times: reversed, randomly
    permuted, and sorted (which must not be counted).  -> (the matrix, expected sorted_lds, expected sorted_long)."""
    cap = lds_capacity(sa)
    rng = np.random.default_rng(31)
    nrow = 3 * cap + 7
    cols = []
    for n in (1, 2, 3, 63, 64, 65, 130, cap - 1, cap, cap + 1, 3 * cap):
        rows = np.sort(rng.choice(nrow, n, replace=False))
        perm = rng.permutation(rows)
        if n > 1 and np.array_equal(perm, rows):
            perm = np.roll(rows, 1)
        cols += [rows[::-1], rows, perm]
    M = from_cols(nrow, cols, rng.integers(1, 1000, sum(len(r) for r in cols)).astype(np.float64))
    lens = M.out_of_order_columns()
    assert lens.size == 2 * 10, "every length but 1, reversed and permuted"
    return M, int((lens <= cap).sum()), int((lens > cap).sum())


@functools.lru_cache(maxsize=None)
def wide_sort_case():
    """16 384 + 3 columns of two entries; columns 7, 16 384 and 16 386 reversed: the mark kernel's second pass."""
    n = PASS_SLICES + 3
    i = np.tile(np.array([1, 4], dtype=np.int32), n)
    for c in (7, PASS_SLICES, PASS_SLICES + 2):
        i[2 * c:2 * c + 2] = [4, 1]
    return Csc(1.0 + np.arange(2 * n) % 13, i, 2 * np.arange(n + 1), 6)


@gpu
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("mig", [0, 1])
def test_out_of_order_slices_are_sorted_and_counted(sa, mig, space):
    M, n_lds, n_long = sort_case(sa)
    cap = lds_capacity(sa)
    assert n_lds == 2 * 8 and n_long == 2 * 2 and M.out_of_order_columns().max() == 3 * cap
    with sa.Context(0) as c:
        rep = c.upload_native(typed(sa, M, mig, F32, I64 if mig else I32, I64, space))
        assert (rep["sorted_lds"], rep["sorted_long"], rep["nnz"]) == (n_lds, n_long, M.nnz)
        assert_state(c, expected_for(sa, "sort", mig), "sorted upload")
        # the canonical form of the same matrix: one validator pass, nothing sorted
        rep = c.upload_native(typed(sa, M.sorted(), mig, F32, I32, I32, space))
        assert (rep["sorted_lds"], rep["sorted_long"]) == (0, 0)
        assert_state(c, expected_for(sa, "sort", mig), "canonical upload")
        # without SGL_UP_SORT the same arrays are refused as `order`
        with pytest.raises(sa.SingletHipError) as err:
            c.upload_native(typed(sa, M, mig, F32, I32, I64, space), sort=False)
        assert_names_classes(str(err.value), {"order"})
        assert DUPLICATES not in str(err.value)
        assert_empty(sa, c)


@gpu
@pytest.mark.parametrize("mig", [0, 1])
def test_out_of_order_slice_in_the_mark_kernels_second_pass(sa, mig):
    M = wide_sort_case()
    with sa.Context(0) as c:
        rep = c.upload_native(typed(sa, M, mig, I32, I32, I32))
        assert (rep["sorted_lds"], rep["sorted_long"]) == (3, 0)
        assert_state(c, expected_for(sa, "wide_sort", mig), "wide")


# ------------------------------------------------------------------------------------------------------- 4. refusals
def refused(sa, c, N, classes, exc=None, sort=True, text=None):
    """Something valid is resident first: the refusal must not leave IT there either."""
    c.upload_native(typed(sa, lanes_base(), 0))
    with pytest.raises(exc or sa.SingletHipError) as err:
        c.upload_native(N, sort=sort)
    if classes is not None:
        assert_names_classes(str(err.value), classes)
    if text:
        assert text in str(err.value), str(err.value)
    assert_empty(sa, c)


def lanes_with(i=None, x=None, p=None):
    M = lanes_base()
    return Csc(M.x if x is None else x, M.i if i is None else i, M.p if p is None else p, M.nrow)


@gpu
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("it", [I32, I64])
@pytest.mark.parametrize("value,entry", [(-1, 0), (200, 144), (-1, 5 + 64), (200, 5 + 65)])
def test_index_out_of_range_is_refused(sa, it, value, entry, space):
    i = lanes_base().i.copy()
    i[entry] = value
    with sa.Context(0) as c:
        # at the first and the last entry no neighbour makes it an order defect as well
        refused(sa, c, typed(sa, lanes_with(i=i), 0, F32, it, I32, space), {"range"} if entry in (0, 144) else None, text=CLASS_TEXT["range"])


@gpu
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("mig", [0, 1])
def test_a_64_bit_index_is_range_checked_before_it_is_narrowed(sa, mig, space):
    """2^32 + 3 with 200 rows is out of range: it must not become row 3 (which would be a valid, ascending index here)."""
    M = lanes_base() if not mig else lanes_base().t()

    def valid_with_3_at(e):
        j = M.i.copy()
        j[e] = 3
        return M.i[e] != 3 and Csc(M.x, j, M.p, M.nrow).out_of_order_columns().size == 0 and not (np.diff(j) == 0)[np.diff(M.col_of_entry()) == 0].any()

    e = next(q for q in range(M.nnz) if valid_with_3_at(q))      # the low 32 bits would pass every check here
    i = M.i.astype(np.int64)
    i[e] = 2 ** 32 + 3
    arr = [to_space(a, space) for a in (M.x.astype(np.float32), i, M.p)]
    N = sa.native((arr[0], arr[1], arr[2], (M.ncol, M.nrow), "csr") if mig else (arr[0], arr[1], arr[2], (M.nrow, M.ncol), "csc"))
    with sa.Context(0) as c:
        refused(sa, c, N, None, text=CLASS_TEXT["range"])


@gpu
@pytest.mark.parametrize("space", ["host", "device"])
def test_int64_values_beyond_2_to_53_are_refused_as_inexact(sa, space):
    M = lanes_base()
    with sa.Context(0) as c:
        for v, entry in ((2 ** 53 + 1, 0), (-(2 ** 53 + 1), 144), (2 ** 63 - 1, 70), (-2 ** 63, 71)):
            x = M.x.astype(np.int64)
            x[entry] = v
            arr = [to_space(a, space) for a in (x, M.i, M.p)]
            refused(sa, c, sa.native((arr[0], arr[1], arr[2], (200, 5), "csc")), {"inexact"})
        x = M.x.astype(np.int64)
        x[0], x[144] = 2 ** 53, -2 ** 53        # the edge itself is exact
        arr = [to_space(a, space) for a in (x, M.i, M.p)]
        rep = c.upload_native(sa.native((arr[0], arr[1], arr[2], (200, 5), "csc")))
        got = c.download(0)
        assert rep["integral"] == 1 and np.array_equal(bits(got[0]), bits(x.astype(np.float64)))
        assert got[0][0] == 2.0 ** 53 and got[0][144] == -2.0 ** 53


@gpu
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "pinf", "ninf"])
@pytest.mark.parametrize("xt", [F32, F64])
def test_non_finite_values_are_refused(sa, xt, value, space):
    with sa.Context(0) as c:
        for entry in (0, 144):
            x = lanes_base().x.copy()
            x[entry] = value
            refused(sa, c, typed(sa, lanes_with(x=x), 0, xt, I32, I32, space), {"finite"})
        M = long_column()                     # the last entry: past the first grid pass
        x = M.x.copy()
        x[PASS_ELEMENTS] = value
        refused(sa, c, typed(sa, Csc(x, M.i, M.p, M.nrow), 0, xt, I32, I64, space), {"finite"})


@gpu
@pytest.mark.parametrize("space", ["host", "device"])
def test_duplicate_indices_are_refused_sorted_or_not(sa, space):
    M = lanes_base()
    with sa.Context(0) as c:
        i = M.i.copy()
        i[5 + 64] = i[5 + 63]                                  # inside a sorted slice, across the wave's laps
        refused(sa, c, typed(sa, lanes_with(i=i), 0, F32, I32, I32, space), {"order"}, text=DUPLICATES)
        refused(sa, c, typed(sa, lanes_with(i=i), 0, F32, I64, I32, space), {"order"}, sort=False)
        i = M.i.copy()
        i[5:135] = i[5:135][::-1]                              # an unsorted slice ...
        i[5 + 10] = i[5 + 100]                                 # ... that holds one index twice
        refused(sa, c, typed(sa, lanes_with(i=i), 0, F32, I32, I64, space), {"order"}, text=DUPLICATES)


@gpu
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("pt", [I32, I64])
def test_invalid_offsets_are_refused(sa, pt, space):
    M = lanes_base()
    assert list(M.p) == [0, 5, 135, 135, 142, 145]
    with sa.Context(0) as c:
        for p in ([1, 5, 135, 135, 142, 145], [0, 5, 135, 134, 142, 145], [0, 5, 4, 135, 142, 145]):
            refused(sa, c, typed(sa, lanes_with(p=np.array(p)), 0, F32, I32, pt, space), set(), text="offset")
        for p in ([0, 5, 135, 135, 142, 144], [0, 5, 135, 135, 142, 146]):      # fewer / more entries than the arrays hold
            refused(sa, c, typed(sa, lanes_with(p=np.array(p)), 0, F32, I32, pt, space), None, exc=ValueError, text="145 entries")
        c.upload_native(typed(sa, M, 0, F32, I32, pt, space))                      # and the context is usable again
        assert_state(c, expected_for(sa, "lanes", 0), "after the refusals")


@gpu
def test_bad_arguments_are_einval_and_leave_the_context_empty(sa):
    M = lanes_base()
    x, i, p = M.x, M.i, M.p.astype(np.int32)
    good = (x, F64, i, I32, p, I32, 5, 200, 0)
    cases = {"x_type 4": (x, 4, i, I32, p, I32, 5, 200, 0), "x_type -1": (x, -1, i, I32, p, I32, 5, 200, 0),
             "idx_type F64": (x, F64, i, F64, p, I32, 5, 200, 0), "idx_type F32": (x, F64, i, F32, p, I32, 5, 200, 0),
             "ptr_type F32": (x, F64, i, I32, p, F32, 5, 200, 0), "ptr_type 7": (x, F64, i, I32, p, 7, 5, 200, 0),
             "major_is_genes 2": (x, F64, i, I32, p, I32, 5, 200, 2), "major_is_genes -1": (x, F64, i, I32, p, I32, 5, 200, -1),
             "n_minor 2^31": (x, F64, i, I32, p, I32, 5, 2 ** 31, 0), "n_minor 0": (x, F64, i, I32, p, I32, 5, 0, 0),
             "n_major 2^31": (x, F64, i, I32, p, I32, 2 ** 31, 200, 0), "n_major 0": (x, F64, i, I32, p, I32, 0, 200, 0)}
    with sa.Context(0) as c:
        for what, args in cases.items():
            assert raw_upload(sa, c, *good)[0] == 0 and c.dims() == (200, 5, 145)
            assert raw_upload(sa, c, *args)[0] == -1, what
            assert_empty(sa, c)
        for kw in (dict(space=2), dict(flags=2), dict(flags=0x80000001)):
            assert raw_upload(sa, c, *good)[0] == 0
            assert raw_upload(sa, c, *good, **kw)[0] == -1, kw
            assert_empty(sa, c)
        rc, rep = raw_upload(sa, c, *good)
        assert rc == 0 and list(rep[:4]) == [145, 0, 0, 1] and list(rep[6:]) == [0, 0]
        assert_state(c, expected_for(sa, "lanes", 0), "after the refusals")


# -------------------------------------------------------------------------------------------------------- 5. drivers
@functools.lru_cache(maxsize=None)
def counts_60x90():
    """A 60 genes x 90 cells count matrix in canonical CSC, every gene and cell non-empty."""
    rng = np.random.default_rng(51)
    D = rng.poisson(rng.gamma(1.0, 1.0, (60, 3)) @ rng.gamma(0.5, 1.0, (3, 90))).astype(np.float64)   # three planted factors
    D[np.arange(60), np.arange(60)] += 1
    D[np.arange(90) % 60, np.arange(90)] += 1
    keep = (D != 0).T
    return Csc(D.T[keep], np.nonzero(keep)[1], np.concatenate([[0], np.cumsum(keep.sum(axis=1))]), 60)


def driver_inputs(sa, form, scale=1.0):
    """(the NativeMatrix, the dgCMatrix of the host-converted matrix)."""
    A = counts_60x90()
    A = Csc(A.x * scale, A.i, A.p, A.nrow)
    dgc = sa.dgCMatrix(A.x, A.i, A.p.astype(np.int32), (60, 90))
    if form == "f32_csr_cells_by_genes":         # AnnData's X: the CSR of cells x genes is the CSC of A
        N = sa.native((A.x.astype(np.float32), A.i.astype(np.int32), A.p.astype(np.int32), (90, 60), "csr"), cells_by_genes=True)
        assert N.major_is_genes == 0
    else:                                        # int32 CSC of cells x genes = the CSC of t(A), indices shuffled per gene
        T = A.t()
        rng = np.random.default_rng(52)
        o = np.concatenate([T.p[g] + rng.permutation(int(T.p[g + 1] - T.p[g])) for g in range(T.ncol)])
        xt = np.int32 if scale == 1.0 else np.float32
        N = sa.native((T.x[o].astype(xt), T.i[o].astype(np.int64), T.p, (90, 60), "csc"), cells_by_genes=True)
        assert N.major_is_genes == 1 and Csc(T.x[o], T.i[o], T.p, T.nrow).out_of_order_columns().size > 30
    assert (N.nrow, N.ncol) == (60, 90)
    return N, dgc


def same_model(a, b, what):
    for key in ("w", "d", "h"):
        assert np.array_equal(a[key], b[key]), "%s: %s" % (what, key)
    if "cv_data" in a and "cv_data" in b:        # (run_nmf returns none)
        same_cv(a["cv_data"], b["cv_data"], what)


def same_cv(a, b, what):
    assert a.columns() == b.columns() and len(a) == len(b), what
    for col in a.columns():
        assert np.array_equal(np.array(a.column(col)), np.array(b.column(col)), equal_nan=True), "%s: cv_data %s" % (what, col)


FORMS = ["f32_csr_cells_by_genes", "i32_csc_cells_by_genes_unsorted"]


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_drivers_through_native_equal_the_dgcmatrix_route(sa, form):
    N, dgc = driver_inputs(sa, form)
    same_model(sa.run_nmf(N, 3, maxit=8, verbose=False, seed=7), sa.run_nmf(dgc, 3, maxit=8, verbose=False, seed=7), "run_nmf")
    # tol_overfit: the search must not stop at its first rank on 90 cells (it would have no rank left to choose from)
    kw = dict(k_max=6, maxit=8, verbose=0, seed=8, tol_overfit=1e9)
    same_model(sa.ard_nmf(N, **kw), sa.ard_nmf(dgc, **kw), "ard_nmf")
    kw = dict(n_replicates=2, maxit=8, verbose=0, seed=9)
    cv = sa.cross_validate_nmf(N, [2, 3], **kw)
    assert len(cv) > 0
    same_cv(cv, sa.cross_validate_nmf(dgc, [2, 3], **kw), "cross_validate_nmf")
    w = np.random.default_rng(10).random((60, 4))
    for wm in (w, w.T):
        a, b = sa.project_model(N, wm, L1=0.01), sa.project_model(dgc, wm, L1=0.01)
        assert np.array_equal(a["h"], b["h"]) and np.array_equal(a["d"], b["d"]), "project_model"
    rows, cols = [5, 3, 59, 3], np.arange(90) % 4 == 1
    a, b = sa.subset(N, rows, cols), sa.subset(dgc, rows, cols)
    assert a.Dim == b.Dim and np.array_equal(a.p, b.p) and np.array_equal(a.i, b.i) and np.array_equal(bits(a.x), bits(b.x)), "subset"


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_runnmf_through_native(sa, form):
    N, dgc = driver_inputs(sa, form)
    kw = dict(k=3, features=list(range(0, 60, 2)) + [1], split_by=np.arange(90) % 3, maxit=8, verbose=0, seed=12)
    same_model(sa.RunNMF(N, **kw), sa.RunNMF(dgc, **kw), "RunNMF")


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_runnmf_log_normalises_integral_input_only(sa, form):
    """The decision comes from the upload's report.  Integral counts: RunNMF is run_nmf on the log-normalised matrix.  The
    same matrix scaled by 0.5 has fractions: RunNMF is run_nmf on the matrix as it is."""
    kw = dict(tol=0, maxit=8, verbose=False, seed=13)         # (tol: the two drivers' defaults differ)
    N, dgc = driver_inputs(sa, form)
    got = sa.RunNMF(N, k=3, tol=0, maxit=8, verbose=0, seed=13)
    same_model(got, sa.run_nmf(sa.PreprocessData(dgc), 3, **kw), "integral: log-normalised")
    assert not np.array_equal(got["d"], sa.run_nmf(dgc, 3, **kw)["d"])
    N, dgc = driver_inputs(sa, form, scale=0.5)
    got = sa.RunNMF(N, k=3, tol=0, maxit=8, verbose=0, seed=13)
    same_model(got, sa.run_nmf(dgc, 3, **kw), "fractions: as it is")
    assert not np.array_equal(got["d"], sa.run_nmf(sa.PreprocessData(dgc), 3, **kw)["d"])
