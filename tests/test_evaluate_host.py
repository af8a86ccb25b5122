"""Host side of the model evaluation (no device): the header, the ctypes table and the package agree on the three new
entries, and singlet_amd.evaluate refuses mismatched shapes before the library is touched."""
import os
import re

import numpy as np
import pytest

import singlet_amd as sa
from singlet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sgl_evaluate", "sgl_c_evaluate", "sgl_multi_evaluate")


def test_header_ctypes_table_and_package_agree_on_the_new_names():
    with open(os.path.join(ROOT, "include", "singlet_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"SGL_API\s+[\w\s\*]+?\b(sgl_\w+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "sgl_abi_version(void);   /* 2:" in header
    # the rules the header has to state
    text = header[header.index("Model error of the current factors"):header.index("SGL_API int sgl_c_evaluate")]
    for phrase in ("zeros included", "+0.0", "NaN and Inf", "chunks of 1024", "chunk order", "sgl_upload_dense", "SGL_ESTATE",
                   "sgl_multi_evaluate", "are ignored", "same bits"):
        assert phrase in text, phrase
    assert callable(sa.evaluate) and "evaluate" in sa.api.__doc__
    for cls in (sa.Context, sa.Multi):
        assert callable(getattr(cls, "evaluate")), cls


def test_the_new_unit_is_built():
    with open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")) as f:
        assert "kernels_eval.o" in f.read()
    assert os.path.exists(os.path.join(ROOT, "singlet_amd", "csrc", "kernels_eval.hip"))


def test_evaluate_refuses_mismatched_shapes_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched before the checks"))
    m, n, k = 6, 8, 3
    A = sa.dgCMatrix.from_dense(np.arange(m * n, dtype=np.float64).reshape(m, n) % 5)
    good = {"w": np.ones((m, k)), "d": np.ones(k), "h": np.ones((k, n))}
    for key, bad in (("w", np.ones((m + 1, k))), ("w", np.ones((m, k + 1))), ("h", np.ones((k, n + 1))), ("h", np.ones((k + 1, n))),
                     ("d", np.ones(k + 1)), ("w", np.ones(m)), ("h", np.ones(n))):
        with pytest.raises(ValueError, match="evaluate:"):
            sa.evaluate(A, dict(good, **{key: bad}))
    with pytest.raises(ValueError, match="rank 0"):
        sa.evaluate(A, {"w": np.ones((m, 0)), "d": np.ones(0), "h": np.ones((0, n))})
    with pytest.raises(KeyError):
        sa.evaluate(A, {"w": good["w"], "h": good["h"]})
