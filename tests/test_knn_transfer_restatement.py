"""The neighbour index and the label / value transfer without a device: the numpy restatement of the transfer rules
(tests/knn_transfer_restatement.py) on hand-computed cases, the declarations of the new entries and their bindings, the Python
refusals that need no device, and the host logic of singlet_amd/csrc/knn_transfer_host.h run as a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import knn_transfer_restatement as tr

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
INF = np.inf


# ------------------------------------------------------------------------------------------------- hand-computed cases
def test_dudani_weights_are_one_half_and_zero_on_equally_spaced_distances():
    w, valid = tr.weights([[4, 7, 9]], [[0.0, 1.0, 2.0]], "distance")
    assert w.tolist() == [[1.0, 0.5, 0.0]] and valid.all()
    w, _ = tr.weights([[4, 7, 9]], [[0.0, 1.0, 2.0]], "uniform")
    assert w.tolist() == [[1.0, 1.0, 1.0]]
    w, valid = tr.weights([[4, 7, 9, -1]], [[3.0, 4.0, 5.0, INF]], 1)       # the padding does not move d_last
    assert w[0, :3].tolist() == [1.0, 0.5, 0.0] and valid.tolist() == [[True, True, True, False]]


def test_a_tie_between_two_classes_goes_to_the_lower_class():
    labels = np.array([2, 1, 1, 0])
    out = tr.transfer([[0, 1, 2, 3]], [[0.0, 1.0, 1.0, 2.0]], labels, 3)      # weights 1, 1/2, 1/2, 0: s = (0, 1, 1), W = 2
    assert out["scores"].tolist() == [[0.0, 0.5, 0.5]]
    assert out["predicted"].tolist() == [1] and out["score"].tolist() == [0.5]
    out = tr.transfer([[0, 1, 2, 3]], [[0.0, 1.0, 1.0, 2.0]], labels, 3, weighting="uniform")   # s = (1, 2, 1), W = 4
    assert out["scores"].tolist() == [[0.25, 0.5, 0.25]] and out["predicted"].tolist() == [1]


def test_w_zero_all_padding_a_single_neighbour_and_equal_distances():
    V = np.array([[10.0, 20.0, 40.0, 80.0], [1.0, 0.0, -1.0, 0.5]])
    # the only labelled neighbour sits in the last slot, whose Dudani weight is 0: W == 0
    out = tr.transfer([[0, 1, 2]], [[0.0, 1.0, 2.0]], np.array([-1, -1, 3, 0]), 4, V)
    assert out["predicted"].tolist() == [-1] and out["score"].tolist() == [0.0] and not out["scores"].any()
    assert not np.signbit(out["scores"]).any()
    assert out["values"].tolist() == [[(10.0 + 0.5 * 20.0) / 1.5, 1.0 / 1.5]]
    # under uniform weights the same neighbour votes
    out = tr.transfer([[0, 1, 2]], [[0.0, 1.0, 2.0]], np.array([-1, -1, 3, 0]), 4, V, "uniform")
    assert out["predicted"].tolist() == [3] and out["score"].tolist() == [1.0]
    assert out["values"].tolist() == [[((10.0 + 20.0) + 40.0) / 3.0, 0.0]]
    # all padding
    out = tr.transfer([[-1, -1, -1]], [[INF, INF, INF]], np.array([0, 1, 1, 0]), 2, V)
    assert out["predicted"].tolist() == [-1] and out["score"].tolist() == [0.0] and out["scores"].tolist() == [[0.0, 0.0]]
    assert np.isnan(out["values"]).all()
    # a single neighbour, then padding: d_last == d_first, weight 1
    out = tr.transfer([[3, -1, -1]], [[5.0, INF, INF]], np.array([0, 1, 1, 0]), 2, V)
    assert out["predicted"].tolist() == [0] and out["score"].tolist() == [1.0] and out["values"].tolist() == [[80.0, 0.5]]
    # equal distances (zero distances among them): everybody votes 1
    for d in (2.0, 0.0):
        out = tr.transfer([[0, 1, 2]], [[d, d, d]], np.array([1, 1, 0, 0]), 2, V)
        assert out["scores"].tolist() == [[1.0 / 3.0, 2.0 / 3.0]] and out["predicted"].tolist() == [1]
        assert out["values"].tolist() == [[((10.0 + 20.0) + 40.0) / 3.0, ((1.0 + 0.0) + -1.0) / 3.0]]
    # a +Inf distance in the last VALID slot: not finite, everybody votes 1
    out = tr.transfer([[0, 1, 2]], [[0.0, 1.0, INF]], np.array([1, 1, 0, 0]), 2)
    assert out["scores"].tolist() == [[1.0 / 3.0, 2.0 / 3.0]]


def test_sums_run_in_rank_order():
    # 1 + 2^-53 + 2^-53 sequentially from +0.0 stays 1; any pairing of the small terms first would give 1 + 2^-52
    V = np.array([[1.0, 2.0 ** -53, 2.0 ** -53]])
    out = tr.transfer([[0, 1, 2]], [[1.0, 1.0, 1.0]], None, 0, V)
    assert out["values"][0, 0] == 1.0 / 3.0 and out["predicted"] is None
    out = tr.transfer([[1, 2, 0]], [[1.0, 1.0, 1.0]], None, 0, V)
    assert out["values"][0, 0] == (2.0 ** -52 + 1.0) / 3.0


# ------------------------------------------------------------------------------------------- declarations and binding
NEW = ("sgl_knn_index_build", "sgl_knn_index_search", "sgl_knn_index_drop", "sgl_knn_index_info", "sgl_knn_index_annotate",
       "sgl_knn_index_map", "sgl_op_knn_transfer")


def test_the_entries_are_declared_and_bound_alike(sa):
    from singlet_amd import _lib, _marshal
    f64p, i32p, i64p = _lib.f64p, _lib.i32p, _lib.i64p
    i32, i64, ctx = C.c_int32, C.c_int64, C.c_void_p
    assert _lib.SIGNATURES["sgl_knn_index_build"] == (C.c_int, [ctx, f64p, i32, i64, i32p, i32, i32, i32, i32, i32])
    assert _lib.SIGNATURES["sgl_knn_index_search"] == (C.c_int, [ctx, f64p, i64, i32, i32, i64, i32p, f64p])
    assert _lib.SIGNATURES["sgl_knn_index_drop"] == (C.c_int, [ctx])
    assert _lib.SIGNATURES["sgl_knn_index_info"] == (C.c_int, [ctx, i64p])
    assert _lib.SIGNATURES["sgl_knn_index_annotate"] == (C.c_int, [ctx, i32p, i32, f64p, i32])
    assert _lib.SIGNATURES["sgl_knn_index_map"] == (C.c_int, [ctx, f64p, i64, i32, i32, i32, i32p, f64p, i32p, f64p, f64p, f64p])
    assert _lib.SIGNATURES["sgl_op_knn_transfer"] == (C.c_int, [ctx, i32p, f64p, i32, i64, i64, i32p, i32, f64p, i32, i32, i32p, f64p, f64p, f64p])
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    assert "Neighbour index and transfer" in header and "int64_t out[16]" in header
    for name in NEW:
        m = re.search(r"SGL_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "knn_transfer_host.h")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower()          # the host header makes no HIP call
    assert int(re.search(r"#define KNN_TRANSFER_MAX_CLASSES (\d+)", host).group(1)) == 65536
    assert int(re.search(r"#define KNN_TRANSFER_MAX_VALUES (\d+)", host).group(1)) == 1024
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^kernels_knn_transfer\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M) and " kernels_knn_transfer.o " in mk
    assert len(_marshal.KNN_INDEX_FIELDS) == 16 and _marshal.KNN_WEIGHTINGS == tr.WEIGHTINGS
    for name in ("knn_index_build", "knn_index_search", "knn_index_annotate", "knn_index_map", "knn_index_drop", "knn_index_info",
                 "op_knn_transfer"):
        assert callable(getattr(sa.Context, name)), name
    for name in ("ReferenceIndex", "transfer_labels", "transfer_values", "map_query"):
        assert hasattr(sa, name), name
    for name in ("search", "map", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(sa.ReferenceIndex, name)), name


def test_the_python_defaults_are_the_stated_ones(sa):
    p = inspect.signature(sa.Context.knn_index_build).parameters
    assert [p[k].default for k in ("reference", "dims", "metric", "method", "n_lists", "n_iter")] == [None, None, "euclidean", "ivf", None, 10]
    p = inspect.signature(sa.Context.knn_index_search).parameters
    assert [p[k].default for k in ("n_neighbors", "n_probe", "query_batch")] == [20, None, 0]
    p = inspect.signature(sa.Context.knn_index_map).parameters
    assert [p[k].default for k in ("n_neighbors", "n_probe", "weighting")] == [20, None, "distance"]
    p = inspect.signature(sa.ReferenceIndex.__init__).parameters
    assert [p[k].default for k in ("labels", "values", "dims", "metric", "method", "n_lists", "n_iter")] == [None, None, None, "euclidean", "ivf",
                                                                                                          None, 10]
    p = inspect.signature(sa.map_query).parameters
    assert [p[k].default for k in ("L1", "L2", "n_neighbors", "n_probe", "weighting")] == [0.01, 0, 20, None, "distance"]
    assert inspect.signature(sa.transfer_labels).parameters["weighting"].default == "distance"
    assert inspect.signature(sa.transfer_values).parameters["weighting"].default == "distance"


def test_the_python_refusals_that_need_no_device(sa, monkeypatch):
    from singlet_amd import _lib, _marshal

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    E = np.ones((5, 2))
    with pytest.raises(ValueError, match="metric must be"):
        sa.ReferenceIndex(E, metric="manhattan")
    with pytest.raises(ValueError, match="method must be 'exact' or 'ivf'"):
        sa.ReferenceIndex(E, method="annoy")
    with pytest.raises(ValueError, match="cells x factors"):
        sa.ReferenceIndex(np.ones(5))
    with pytest.raises(ValueError, match="1-based"):
        sa.ReferenceIndex(E, dims=[0, 1])
    with pytest.raises(ValueError, match="labels must hold one class"):
        sa.transfer_labels(np.zeros((2, 3), dtype=np.int32), np.zeros((2, 3)), None)
    with pytest.raises(ValueError, match="cells x n_values"):
        sa.transfer_values(np.zeros((2, 3), dtype=np.int32), np.zeros((2, 3)), np.ones((2, 2, 2)))
    with pytest.raises(ValueError, match="index must be a ReferenceIndex"):
        sa.map_query(None, np.ones((3, 2)), object())
    with pytest.raises(ValueError, match="weighting must be 'uniform' or 'distance'"):
        _marshal.knn_weighting("inverse")
    with pytest.raises(ValueError, match="one shape"):
        _marshal.knn_lists_in(np.zeros((2, 3), dtype=np.int32), np.zeros((3, 2)))
    with pytest.raises(ValueError, match="32-bit reference indices"):
        _marshal.knn_lists_in(np.zeros((2, 3)), np.zeros((2, 3)))
    i, d, nq, K = _marshal.knn_lists_in(np.arange(6).reshape(2, 3), np.ones((2, 3), dtype=np.float32))
    assert i.dtype == np.int32 and d.dtype == np.float64 and (nq, K) == (2, 3) and i.flags.c_contiguous


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_host_logic_under_address_and_undefined_sanitizers(tmp_path):
    """knn_transfer_host.h holds no HIP call: it is compiled with a host compiler into a program of its own
    (tests/knn_transfer_host_main.cpp) with both sanitizers and run here, on the CPU, as its own process."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knn_transfer_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "knn_transfer_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "knn_transfer_host: ok" in r.stdout, r.stdout + r.stderr
