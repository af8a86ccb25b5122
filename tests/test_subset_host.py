"""The host side of subset(): how rows / cols become the int32 index lists sgl_subset takes, and that the entry is declared
and bound.  No device is needed: everything here runs before the library is called."""
import os
import re

import numpy as np
import pytest

from singlet_amd import _lib
from singlet_amd.api import _subset_index, _subset_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["g0", "g1", "g2", "g3", "g4"]


def test_integers_pass_through_as_contiguous_int32():
    idx = _subset_index(np.array([4, 0, 4, 2], dtype=np.int64)[::1], 5, None, "rows")
    assert idx.dtype == np.int32 and idx.flags.c_contiguous and idx.tolist() == [4, 0, 4, 2]
    assert _subset_index(None, 5, NAMES, "rows") is None


def test_boolean_mask_selects_in_axis_order():
    assert _subset_index(np.array([True, False, True, True, False]), 5, None, "rows").tolist() == [0, 2, 3]


def test_boolean_mask_of_the_wrong_length_raises():
    with pytest.raises(ValueError, match="mask"):
        _subset_index(np.array([True, False, True]), 5, None, "rows")


def test_names_resolve_to_indices():
    assert _subset_index(["g3", "g0", "g3"], 5, NAMES, "rows").tolist() == [3, 0, 3]
    assert _subset_index(np.array(["g4"]), 5, np.array(NAMES), "cols").tolist() == [4]
    assert _subset_index(["a"], 3, ["a", "b", "a"], "rows").tolist() == [0]   # the first match, as R's `[`


def test_unknown_name_raises():
    with pytest.raises(ValueError, match="'g9'"):
        _subset_index(["g1", "g9"], 5, NAMES, "rows")
    with pytest.raises(ValueError, match="no names"):
        _subset_index(["g1"], 5, None, "rows")


def test_negative_integer_raises():
    with pytest.raises(ValueError, match="negative"):
        _subset_index([0, -1], 5, None, "rows")


def test_out_of_range_empty_and_other_types_raise():
    with pytest.raises(ValueError, match="outside"):
        _subset_index([5], 5, None, "cols")
    with pytest.raises(ValueError, match="nothing"):
        _subset_index([], 5, None, "cols")
    with pytest.raises(ValueError, match="nothing"):
        _subset_index(np.zeros(5, dtype=bool), 5, None, "cols")
    with pytest.raises(ValueError):
        _subset_index([0.5, 1.0], 5, None, "cols")
    with pytest.raises(ValueError, match="one-dimensional"):
        _subset_index([[0, 1]], 5, None, "cols")


def test_dimnames_are_carried_through():
    idx = _subset_index(["g3", "g0", "g3"], 5, NAMES, "rows")
    assert _subset_names(NAMES, idx) == ["g3", "g0", "g3"]
    assert _subset_names(None, idx) is None and _subset_names(NAMES, None) is NAMES


def test_public_names_are_exported():
    import singlet_amd as sa
    assert callable(sa.subset) and callable(sa.RunNMF) and callable(sa.Context.subset)


def test_run_nmf_refuses_var_features_before_touching_the_device():
    import singlet_amd as sa
    A = sa.dgCMatrix([1.0], [0], [0, 1], (2, 1))
    with pytest.raises(ValueError, match="var.features"):
        sa.RunNMF(A, k=2, features="var.features")


def test_entry_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "singlet_hip.h")) as f:
        header = f.read()
    decl = re.search(r"SGL_API\s+int\s+sgl_subset\s*\(([^)]*)\)\s*;", header)
    assert decl, "sgl_subset is not declared in include/singlet_hip.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["sgl_ctx* ctx", "const int32_t* rows", "int64_t n_rows", "const int32_t* cols", "int64_t n_cols"]
    res, argtypes = _lib.SIGNATURES["sgl_subset"]
    import ctypes as C
    assert res is C.c_int and argtypes == [C.c_void_p, _lib.i32p, C.c_int64, _lib.i32p, C.c_int64]
