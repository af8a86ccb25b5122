"""native() and the host half of sgl_upload_typed, without a device: the layout table, that nothing is copied, the dtype
and contiguity refusals, that neither SciPy nor torch is imported for NumPy tuples, the batch edges of the long sort path
around 2^31 entries, the declaration of the entry, and the host logic (singlet_amd/csrc/ingest_host.h) run as a
stand-alone program under AddressSanitizer and UBSan."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX = 2 ** 31 - 1


def arrays(n_major=4, nnz=6, xt=np.float32, it=np.int32, pt=np.int32):
    p = np.array([0, 2, 2, 5, 6][:n_major + 1], dtype=pt)
    return np.arange(1, nnz + 1).astype(xt), np.array([0, 2, 1, 3, 4, 0], dtype=it), p


class FakeScipy:
    """What native() reads of a SciPy object, and nothing more."""

    def __init__(self, fmt, shape, x, i, p):
        self.format, self.shape, self.data, self.indices, self.indptr = fmt, shape, x, i, p


# (format, cells_by_genes, shape as held) -> (major_is_genes, nrow = genes, ncol = cells, n_major, n_minor)
LAYOUT = [("csr", True, (4, 7), (0, 7, 4, 4, 7)),      # AnnData's X: cells x genes CSR
          ("csc", False, (7, 4), (0, 7, 4, 4, 7)),     # genes x cells CSC: this package's A
          ("csr", False, (4, 7), (1, 4, 7, 4, 7)),     # genes x cells CSR
          ("csc", True, (7, 4), (1, 4, 7, 4, 7))]      # cells x genes CSC


@pytest.mark.parametrize("fmt,cbg,shape,exp", LAYOUT)
@pytest.mark.parametrize("how", ["tuple", "duck"])
def test_layout_table(sa, fmt, cbg, shape, exp, how):
    x, i, p = arrays()
    N = sa.native((x, i, p, shape, fmt) if how == "tuple" else FakeScipy(fmt, shape, x, i, p), cells_by_genes=cbg)
    assert (N.major_is_genes, N.nrow, N.ncol, N.n_major, N.n_minor) == exp
    assert N.space == 0 and N.device is None and N.nnz == 6
    from singlet_amd.native import major_is_genes
    assert major_is_genes(fmt, cbg) == exp[0]
    with pytest.raises(ValueError, match="csr"):
        major_is_genes("coo", cbg)


def test_references_are_kept_and_nothing_is_copied(sa):
    x, i, p = arrays(xt=np.int64, it=np.int64, pt=np.int64)
    N = sa.native((x, i, p, (4, 7), "csr"), cells_by_genes=True, Dimnames=(list("abcdefg"), None))
    assert N.data is x and N.indices is i and N.indptr is p
    for a, b in zip((N.data, N.indices, N.indptr), (x, i, p)):
        assert np.shares_memory(a, b)
    assert N.addresses() == (x.ctypes.data, i.ctypes.data, p.ctypes.data)
    assert (N.x_type, N.idx_type, N.ptr_type) == (3, 3, 3)
    assert N.Dimnames[0] == list("abcdefg") and sa.native(N) is N
    x[0] = 77                                   # the object sees its owner's writes
    assert N.data[0] == 77


@pytest.mark.parametrize("xt,code", [(np.float64, 0), (np.float32, 1), (np.int32, 2), (np.int64, 3)])
def test_value_type_codes(sa, xt, code):
    x, i, p = arrays(xt=xt)
    assert sa.native((x, i, p, (4, 7), "csr")).x_type == code


@pytest.mark.parametrize("bad", [np.bool_, np.uint8, np.uint16, np.float16, np.int16, np.uint32, np.complex64])
def test_value_dtypes_that_are_refused_not_cast(sa, bad):
    x, i, p = arrays(xt=bad)
    with pytest.raises(TypeError, match=np.dtype(bad).name):
        sa.native((x, i, p, (4, 7), "csr"))


@pytest.mark.parametrize("which", ["indices", "indptr"])
@pytest.mark.parametrize("bad", [np.int16, np.uint32, np.uint64, np.float64])
def test_index_dtypes_that_are_refused(sa, which, bad):
    x, i, p = arrays(it=bad if which == "indices" else np.int32, pt=bad if which == "indptr" else np.int32)
    with pytest.raises(TypeError, match=which + ".*" + np.dtype(bad).name):
        sa.native((x, i, p, (4, 7), "csr"))


def test_contiguity_and_shape_refusals(sa):
    x, i, p = arrays()
    x2 = np.arange(12, dtype=np.float32)[::2]
    assert not x2.flags.c_contiguous
    with pytest.raises(ValueError, match="data.*contiguous"):
        sa.native((x2, i, p, (4, 7), "csr"))
    with pytest.raises(ValueError, match="indices.*contiguous"):
        sa.native((x, np.zeros(12, np.int32)[::2], p, (4, 7), "csr"))
    with pytest.raises(ValueError, match="one-dimensional"):
        sa.native((x.reshape(2, 3), i, p, (4, 7), "csr"))
    with pytest.raises(ValueError, match="byte order"):
        sa.native((x.astype(x.dtype.newbyteorder()), i, p, (4, 7), "csr"))
    with pytest.raises(ValueError, match="offsets"):
        sa.native((x, i, p, (5, 7), "csr"))            # 5 major slices need 6 offsets
    with pytest.raises(ValueError, match="entries"):
        sa.native((x[:5], i, p, (4, 7), "csr"))
    with pytest.raises(TypeError, match="list"):
        sa.native((list(x), i, p, (4, 7), "csr"))      # a list would have to be copied
    with pytest.raises(TypeError, match="expected"):
        sa.native(np.zeros((3, 3)))
    N = sa.native((x, i, np.array([0, 2, 2, 5, 7], dtype=np.int32), (4, 7), "csr"))
    with pytest.raises(ValueError, match=r"indptr\[4\] = 7"):
        N.check_entry_count()
    sa.native((x, i, p, (4, 7), "csr")).check_entry_count()


def test_numpy_tuples_import_neither_scipy_nor_torch():
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "import singlet_amd as sa\n"
            "N = sa.native((np.ones(2, np.float32), np.array([0, 1], np.int64), np.array([0, 1, 2], np.int64), (2, 3), 'csr'), True)\n"
            "assert (N.nrow, N.ncol, N.major_is_genes) == (3, 2, 0)\n"
            "bad = [m for m in sys.modules if m.split('.')[0] in ('scipy', 'torch')]\n"
            "assert not bad, bad\n"
            "print('clean')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stdout + r.stderr


def test_scipy_and_torch_objects_are_read_in_place(sa):
    sp = pytest.importorskip("scipy.sparse")
    torch = pytest.importorskip("torch")
    D = (np.arange(28).reshape(4, 7) % 3 == 0) * np.arange(1.0, 29.0).reshape(4, 7)
    for make, fmt in ((sp.csr_matrix, "csr"), (sp.csc_matrix, "csc"), (sp.csr_array, "csr"), (sp.csc_array, "csc")):
        M = make(D.astype(np.float32))
        N = sa.native(M, cells_by_genes=True)
        assert N.format == fmt and np.shares_memory(N.data, M.data) and np.shares_memory(N.indices, M.indices)
        assert np.shares_memory(N.indptr, M.indptr) and (N.nrow, N.ncol) == (7, 4)
        assert N.major_is_genes == (0 if fmt == "csr" else 1)
    T = torch.tensor(D, dtype=torch.float32).to_sparse_csr()
    N = sa.native(T, cells_by_genes=True)
    assert N.space == 0 and N.device is None, "a CPU tensor travels as HOST"
    assert (N.x_type, N.idx_type, N.ptr_type, N.major_is_genes, N.nrow, N.ncol) == (1, 3, 3, 0, 7, 4)
    assert N.addresses() == (T.values().data_ptr(), T.col_indices().data_ptr(), T.crow_indices().data_ptr())
    N = sa.native(torch.tensor(D).to_sparse_csc())
    assert (N.format, N.x_type, N.major_is_genes, N.nrow, N.ncol) == ("csc", 0, 0, 4, 7)
    with pytest.raises(TypeError, match="layout"):
        sa.native(torch.tensor(D).to_sparse_coo())
    with pytest.raises(TypeError, match="float16"):
        sa.native((torch.ones(2, dtype=torch.float16), torch.tensor([0, 1]), torch.tensor([0, 1, 2]), (2, 3), "csr"))
    with pytest.raises(ValueError, match="same place"):
        sa.native((np.ones(2), torch.tensor([0, 1]), torch.tensor([0, 1, 2]), (2, 3), "csr"))


# ----------------------------------------------------------------------------------------------------- batch edges
def batch_edges(sa, lens, cap=I32_MAX):
    import ctypes as C
    from singlet_amd import _lib
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    cut = np.full(lens.size + 1, -1, dtype=np.int64)
    runs = C.c_int64(-1)
    _lib.check(_lib.load().sgl_ingest_batch_edges(_lib.ptr(lens, _lib.i64p), lens.size, cap, _lib.ptr(cut, _lib.i64p), C.byref(runs)))
    return [int(v) for v in cut[:runs.value + 1]]


@pytest.mark.parametrize("total", [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1])
@pytest.mark.parametrize("lead", [1000, 2 ** 30, 2 ** 31 - 20])
def test_long_path_batches_stay_below_2_to_31_entries(sa, total, lead):
    """hipcub takes int counts, so a batch must hold at most 2^31 - 1 entries, every slice must be in exactly one batch,
    whole.  The last slice starts `lead` + 3 entries in and ends at `total`: at 2^31 and 2^31 + 1 entries it straddles the
    edge and must open a batch of its own; at 2^31 - 1 everything still fits one call."""
    lens = [3, lead, total - lead - 3]
    assert min(lens) > 0 and sum(lens) == total and lead + 3 < I32_MAX
    cut = batch_edges(sa, lens)
    assert cut[0] == 0 and cut[-1] == len(lens) and all(b > a for a, b in zip(cut, cut[1:]))
    sums = [sum(lens[a:b]) for a, b in zip(cut, cut[1:])]
    assert max(sums) <= I32_MAX and sum(sums) == total
    assert cut == ([0, 3] if total == I32_MAX else [0, 2, 3])


def test_batch_edges_small_cases(sa):
    assert batch_edges(sa, []) == [0]
    assert batch_edges(sa, [I32_MAX, I32_MAX, 1]) == [0, 1, 2, 3]
    assert batch_edges(sa, [0, 0, 4, 0, 1], cap=4) == [0, 4, 5]
    assert batch_edges(sa, [5, 9, 2], cap=4) == [0, 1, 2, 3]
    with pytest.raises(sa.SingletHipError):
        batch_edges(sa, [3, -1])
    with pytest.raises(sa.SingletHipError):
        batch_edges(sa, [3], cap=0)


# ------------------------------------------------------------------------------------------------------ declaration
def test_entry_is_declared_bound_and_exported(sa):
    import ctypes as C
    from singlet_amd import _lib
    h = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    m = re.search(r"SGL_API\s+int\s+sgl_upload_typed\s*\(([^;]*)\)\s*;", h)
    assert m, "sgl_upload_typed is not declared"
    params = [q.strip() for q in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 15 and params[0].startswith("sgl_ctx*") and params[-1].startswith("int64_t* report")
    for name, value in (("SGL_T_F64", "0"), ("SGL_T_F32", "1"), ("SGL_T_I32", "2"), ("SGL_T_I64", "3"), ("SGL_SPACE_HOST", "0"),
                        ("SGL_SPACE_DEVICE", "1"), ("SGL_UP_SORT", "1u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), h), name
    res, args = _lib.SIGNATURES["sgl_upload_typed"]
    assert res is C.c_int and len(args) == 15 and args[11] is C.c_uint32 and args[7] is C.c_int64 and args[14] is _lib.i64p
    assert hasattr(C.CDLL(_lib.LIB_PATH), "sgl_upload_typed")
    import importlib
    nat = importlib.import_module("singlet_amd.native")   # (the package attribute `native` is the function)
    assert (nat.SGL_T_F64, nat.SGL_T_F32, nat.SGL_T_I32, nat.SGL_T_I64, nat.SGL_SPACE_DEVICE, nat.SGL_UP_SORT) == (0, 1, 2, 3, 1, 1)
    assert hasattr(sa.Context, "upload_native") and sa.native is nat.native


# -------------------------------------------------------------------------------------------- the host logic, sanitized
def test_host_logic_under_address_and_undefined_sanitizers(tmp_path):
    """The offset checks, the layout mapping and the batch-edge arithmetic hold no HIP call: they are compiled with a host
    compiler into a program of their own (tests/ingest_host_main.cpp) with both sanitizers and run here, on the CPU."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ingest_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "ingest_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ingest_host: ok" in r.stdout, r.stdout + r.stderr
