"""Host side of the linked-NMF workflow (no device): the share / link tables of R/RunLNMF.R:143-154, the argument checks of
run_linked_nmf and RunLNMF that fire before the library is touched, and the agreement of the header, the ctypes table and
the package on the new names."""
import os
import re

import numpy as np
import pytest

import singlet_amd as sa
from singlet_amd import _lib
from singlet_amd.api import _link_table, _share_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sgl_set_links_grouped", "sgl_group_means", "sgl_c_group_means", "sgl_multi_set_links_grouped", "sgl_multi_group_means")


def test_share_and_link_table_on_hand_made_means():
    means = np.array([[1.0, 1.0, 2.0],      # shares 0.75, 0.75, 1.5
                      [0.5, 0.0, 1.5],      # shares 0.75, 0, 2.25
                      [1.0, 2.0, 5.0],      # shares 0.375, 0.75, 1.875
                      [3.0, 3.0, 3.0]])     # shares 1, 1, 1
    share = _share_table(means)
    assert np.array_equal(share, [[0.75, 0.75, 1.5], [0.75, 0.0, 2.25], [0.375, 0.75, 1.875], [1.0, 1.0, 1.0]])
    # `<` is strict: a share exactly at the cut-off stays linked
    assert np.array_equal(_link_table(means, 0.75), [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]])
    assert np.array_equal(_link_table(means, 0.5), [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]])
    assert np.array_equal(_link_table(means, 0.375), [[1, 1, 1], [1, 0, 1], [1, 1, 1], [1, 1, 1]])
    assert np.array_equal(_link_table(means, 1.0), [[0, 0, 1], [0, 0, 1], [0, 0, 1], [1, 1, 1]])
    assert np.array_equal(_link_table(means, 0.0), np.ones((4, 3)))
    assert _link_table(means, 0.5).dtype == np.float64
    # one group: its share is 1 whatever the mean
    assert np.array_equal(_share_table(np.array([[2.0], [7.0]])), [[1.0], [1.0]])


def test_a_nan_share_row_names_its_factor():
    means = np.array([[1.0, 1.0], [0.0, 0.0], [2.0, 1.0]])
    share = _share_table(means)
    assert np.all(np.isnan(share[1])) and not np.any(np.isnan(share[[0, 2]]))
    with pytest.raises(ValueError, match=r"factor 1 \(0-based; factor 2 of the reference\)"):
        _link_table(means, 0.5)
    with pytest.raises(ValueError, match="factor 0 "):
        _link_table(np.array([[np.nan, 1.0], [1.0, 1.0]]), 0.5)
    with pytest.raises(ValueError):
        _share_table(np.zeros((3, 0)))


def _matrix(m=6, n=8):
    D = np.arange(m * n, dtype=np.float64).reshape(m, n) % 5
    return sa.dgCMatrix.from_dense(D)


def test_run_linked_nmf_checks_fire_in_the_reference_order(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched before the checks"))
    A, m, n, k = _matrix(), 6, 8, 3
    w = np.ones((m, k))
    lh, lw = np.ones((k, n)), np.ones((m, k))
    cases = [
        (dict(w=w), "both link_h and link_w cannot be NULL. Specify at least one linking matrix."),
        (dict(w=w, link_h=np.ones((k + 1, n))), "number of rows in 'link_h' must be equal to the nubmer of columns in 'w'"),
        (dict(w=w, link_h=np.ones((k, n + 1))), "number of columns in 'link_h' must be equal to the number of columns in 'A'"),
        (dict(w=w, link_w=np.ones((m, k + 1))), "number of columns in 'link_w' must be equal to the nubmer of columns in 'w'"),
        (dict(w=w, link_w=np.ones((m + 1, k))), "number of rows in 'link_w' must be equal to the number of rows in 'A'"),
        (dict(w=w, link_h=lh, L1=1), "L1 penalty must be strictly in the range (0, 1]"),
        (dict(w=np.ones((m + 1, k)), link_h=lh), "number of rows in 'w' must be equal to the number of rows in 'A'"),
        # the order: a bad link_h is reported before a bad link_w, a bad link before L1, L1 before nrow(w)
        (dict(w=w, link_h=np.ones((k + 1, n)), link_w=np.ones((m + 1, k))), "number of rows in 'link_h' must be equal to the nubmer of columns in 'w'"),
        (dict(w=np.ones((m + 1, k)), link_w=np.ones((m + 1, k)), L1=2.0), "number of rows in 'link_w' must be equal to the number of rows in 'A'"),
        (dict(w=np.ones((m + 1, k)), link_w=lw, L1=2.0), "L1 penalty must be strictly in the range (0, 1]"),
        (dict(w=np.ones((m + 1, k)), link_h=lh, L1=2.0), "L1 penalty must be strictly in the range (0, 1]"),
    ]
    for kwargs, msg in cases:
        with pytest.raises(ValueError) as e:
            sa.run_linked_nmf(A, verbose=False, **kwargs)
        assert str(e.value) == msg, kwargs.keys()


def test_RunLNMF_checks_fire_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched before the checks"))
    A, m, n, k = _matrix(), 6, 8, 3
    model = {"w": np.ones((m, k)), "h": np.ones((k, n))}
    sb = np.arange(n) % 2
    with pytest.raises(ValueError) as e:
        sa.RunLNMF(A, model, None)
    assert str(e.value) == "no value specified for 'split.by'"
    with pytest.raises(ValueError, match="one entry per ROW of A"):
        sa.RunLNMF(A, model, np.arange(m) % 2)
    with pytest.raises(ValueError) as e:
        sa.RunLNMF(A, model, sb[:-1])
    assert str(e.value) == "length of 'split.by' was not equal to one of the dimensions of the input matrix"
    for bad, msg in (
            ({"w": np.ones((m, k)), "h": np.ones((k + 1, n))}, "number of rows in 'link_h' must be equal to the nubmer of columns in 'w'"),
            ({"w": np.ones((m, k)), "h": np.ones((k, n + 1))}, "number of columns in 'link_h' must be equal to the number of columns in 'A'"),
            ({"w": np.ones((m + 1, k)), "h": np.ones((k, n))}, "number of rows in 'link_w' must be equal to the number of rows in 'A'")):
        with pytest.raises(ValueError) as e:
            sa.RunLNMF(A, bad, sb)
        assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        sa.RunLNMF(A, model, sb, L1=1.0)
    assert str(e.value) == "L1 penalty must be strictly in the range (0, 1]"


def test_header_ctypes_table_and_package_agree_on_the_new_names():
    with open(os.path.join(ROOT, "include", "singlet_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"SGL_API\s+[\w\s\*]+?\b(sgl_\w+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    # argument counts of the declarations and of the ctypes table
    for name in NEW_ENTRIES:
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "sgl_abi_version(void);   /* 2:" in header
    for name in ("group_means", "run_linked_nmf", "RunLNMF", "MetadataSummary", "GetSharedFactors", "GetUniqueFactors"):
        assert callable(getattr(sa, name)), name
    for cls, names in ((sa.Context, ("set_links", "set_links_grouped", "group_means")), (sa.Multi, ("set_links", "set_links_grouped", "group_means"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("run_linked_nmf", "RunLNMF", "MetadataSummary", "GetSharedFactors", "group_means"):
        assert name in sa.api.__doc__, name
