"""RasterizeRowwise's natives at the boundaries, on the CPU: the R shim's two entries (singlet_amd/r/singlet_hip_shim.c)
compile against the prototype-only R API of tests/r_api_stub/, are registered with the reference's arity
(src/RcppExports.cpp:446-447, 3 args) and are rebound by backend.R with the wrappers' defaults (R/RcppExports.R:8-14);
the header, the Python binding and the built library all carry the three new entries."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("_singlet_rowwise_compress_sparse", "_singlet_rowwise_compress_dense")
ENTRIES = ("sgl_c_rowwise_compress_sparse", "sgl_c_rowwise_compress_dense", "sgl_rasterize_rowwise")


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_shim_compiles_against_the_abi():
    shim = _read("singlet_amd", "r", "singlet_hip_shim.c")
    assert "sgl_c_rowwise_compress_sparse(" in shim and "sgl_c_rowwise_compress_dense(" in shim
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "r_api_stub"),
                        os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_shim.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("sym", SYMS)
def test_registered_with_arity_3(sym):
    shim = _read("singlet_amd", "r", "singlet_hip_shim.c")
    assert re.search(r'\{"%s",\s*\(DL_FUNC\)&%s,\s*3\}' % (sym, sym), shim)
    m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % sym, shim, flags=re.M)
    assert m and len(m.group(1).split(",")) == 3


@pytest.mark.parametrize("sym", SYMS)
def test_backend_rebinds_with_the_defaults(sym):
    backend = _read("singlet_amd", "r", "backend.R")
    name = sym[len("_singlet_"):]
    m = re.search(r'rebind\("%s", function\(([^)]*)\)\s*\.Call\(dll\[\["%s"\]\],([^)]*)\)' % (name, sym), backend)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["A", "n", "threads"]
    assert [a.strip() for a in m.group(2).split(",")] == ["A", "n", "threads"]
    # the defaults of R/RcppExports.R:8-14 (n = 10L, threads = 0L), restored through formals() for both wrappers
    assert re.search(r'for \(rw in c\("rowwise_compress_sparse", "rowwise_compress_dense"\)\)', backend)
    assert "formals(fn)$n <- 10L" in backend and "formals(fn)$threads <- 0L" in backend


def test_header_binding_and_library_carry_the_entries(sa):
    from singlet_amd import _lib
    h = _read("include", "singlet_hip.h")
    L = ctypes.CDLL(_lib.LIB_PATH)
    for e in ENTRIES:
        assert re.search(r"SGL_API\s+int\s+%s\s*\(" % e, h), e
        assert e in _lib.SIGNATURES, e
        assert hasattr(L, e), e
    assert _lib.SIGNATURES["sgl_rasterize_rowwise"][1][1] is ctypes.c_int64
    assert hasattr(sa, "RasterizeRowwise") and hasattr(sa.Context, "rasterize_rowwise")


def test_bin_size_follows_rcpp(sa):
    from singlet_amd.api import _bin_size
    assert _bin_size(10, "t") == 10 and _bin_size(10.9, "t") == 10 and _bin_size(-2.5, "t") == -2
    assert _bin_size(1e300, "t") == 2**63 - 1
    with pytest.raises(sa.SingletHipError, match="NA"):
        _bin_size(float("nan"), "t")
