"""The inverted-list neighbour search (sgl_knn_ivf) without a device: the numpy restatement (tests/knn_ivf_restatement.py)
against the exact restatements and hand-worked cases, the declarations of the new entries and their bindings, the Python
defaults and refusals, the recall precondition of the fixture "clustered", and the host logic of
singlet_amd/csrc/knn_ivf_host.h run as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import embedding_knn_restatement as euclid
import knn_ivf_restatement as ivf
import knn_metric_restatement as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("euclidean", "cosine", "correlation")


# ------------------------------------------------------------------------------------------- n_probe == n_lists is exact
@pytest.mark.parametrize("metric", METRICS)
def test_all_lists_probed_is_the_exact_search(metric):
    rng = np.random.default_rng(5)
    R = rng.random((6, 150)) * (rng.random((6, 150)) < 0.6)
    R[:, 40:44] = R[:, [40]]          # duplicates: ties that rank by index, possibly across lists' edges
    Q = rng.random((6, 31))
    for Qx, L, K in ((None, 7, 9), (Q, 7, 9), (None, 1, 150), (Q, 150, 20)):
        idx, dist, _, assign = ivf.knn_ivf(R, Qx, K, None, metric, L, L, 3)
        want = km.knn(R, Qx, K, metric=metric)
        assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1]), (metric, L, K)
        assert assign.shape == (150,) and assign.min() >= 0 and assign.max() < L
    dims = [4, 0, 2]
    idx, dist, _, _ = ivf.knn_ivf(R, Q, 5, dims, metric, 6, 6, 2)
    want = km.knn(R, Q, 5, dims=dims, metric=metric)
    assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1])


# ------------------------------------------------------------------------------------------------------- training picks
@pytest.mark.parametrize("n_lists", [1, 3, 45])
def test_training_picks_around_sixty_four_cells_per_list(n_lists):
    for n_ref, T in ((64 * n_lists - 1, 64 * n_lists - 1), (64 * n_lists, 64 * n_lists), (64 * n_lists + 1, 64 * n_lists)):
        picks = ivf.train_picks(n_ref, n_lists)
        assert ivf.train_count(n_ref, n_lists) == T == picks.size
        assert picks[0] == 0 and picks[-1] < n_ref and np.all(np.diff(picks) >= 1)
        if n_ref <= 64 * n_lists:
            assert np.array_equal(picks, np.arange(n_ref))          # every cell trains
        else:
            assert np.array_equal(picks, (np.arange(T) * n_ref) // T) and picks[-1] == ((T - 1) * n_ref) // T
        seeds = ivf.seed_picks(T, n_lists)
        assert seeds[0] == 0 and np.all(np.diff(seeds) >= 1) and seeds[-1] < T
    assert ivf.train_picks(300, 2).size == 128 and ivf.train_picks(300, 2)[[1, 127]].tolist() == [2, 297]
    assert ivf.seed_picks(128, 2).tolist() == [0, 64] and ivf.seed_picks(130, 3).tolist() == [0, 43, 86]


def test_group_sum_is_the_stated_order_and_exact_on_integers():
    rng = np.random.default_rng(9)
    for nd in (1, 3, 20, 64, 66):
        for count in (1, 2, 63, 64, 65, 255, 256, 257, 700):
            M = rng.integers(-8, 9, (nd, count)).astype(np.float64)
            assert np.array_equal(ivf.group_sum(M), M.sum(axis=1)), (nd, count)
    # the order by hand at nd = 20 (FL = 32 lanes over the factors, S = 8 slots, one position each): the tree adds slot 3 to
    # slot 1 first (2^-53 + 2^-53 = 2^-52, exact) and slot 1 to slot 0 last, where a sequential sum loses both halves of an ulp
    M = np.zeros((20, 8))
    M[0, [0, 1, 3]] = [1.0, 2.0 ** -53, 2.0 ** -53]
    assert ivf.group_sum(M)[0] == 1.0 + 2.0 ** -52 and (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0
    assert np.all(ivf.group_sum(M)[1:] == 0.0)
    # and over two chunks: the chunk sums meet last
    M = np.zeros((20, 257))
    M[0, [0, 255, 256]] = [2.0 ** -53, 1.0, 2.0 ** -53]
    assert ivf.group_sum(M)[0] == 1.0   # (2^-53 + 1) rounds to 1 inside the first chunk, and 1 + 2^-53 again


def test_duplicate_seeds_leave_an_empty_list():
    rng = np.random.default_rng(11)
    R = rng.random((4, 130))
    R[:, 43] = R[:, 0]                # seeds of 3 lists over 130 cells: training cells 0, 43, 86
    C, assign = ivf.train(R, 3, 0)    # no step: centroids 0 and 1 are equal, and ties go to the lower centroid
    counts = np.bincount(assign, minlength=3)
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0 and counts.sum() == 130
    assert np.array_equal(C[:, 1], R[:, 43]) and np.array_equal(C[:, 0], C[:, 1])
    idx, dist = ivf.search(R, R, "euclidean", C, assign, 3, 10)
    want = euclid.knn(R, None, 10)
    assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1])
    # through every step: two distinct integer columns, three lists; the mean of copies of a small integer column is exact,
    # so centroid 0 stays equal to centroid 1, which never receives a cell and keeps its value
    R = np.where(np.arange(130)[None, :] < 65, np.array([[1.0], [2.0], [0.0], [5.0]]), np.array([[7.0], [0.0], [3.0], [1.0]]))
    C, assign = ivf.train(R, 3, 4)
    assert np.bincount(assign, minlength=3).tolist() == [65, 0, 65]
    assert np.array_equal(C, R[:, [0, 43, 86]])


def test_a_short_result_has_minus_one_and_inf_in_the_right_slots():
    R = np.array([[0.0, 1.0, 2.0, 10.0, 11.0, 20.0]])
    C = np.array([[1.0, 10.5, 20.0, 40.0]])
    assign = np.array([0, 0, 0, 1, 1, 2], dtype=np.int32)       # list 3 is empty
    Q = np.array([[0.9, 19.0, 100.0]])
    idx, dist = ivf.search(R, Q, "euclidean", C, assign, 1, 3)
    assert idx.tolist() == [[1, 0, 2], [5, -1, -1], [-1, -1, -1]]
    assert np.array_equal(dist, np.array([[np.sqrt((0.9 - 1.0) ** 2), np.sqrt(0.9 ** 2), np.sqrt((0.9 - 2.0) ** 2)], [1.0, np.inf, np.inf], [np.inf] * 3]))
    idx, dist = ivf.search(R, Q, "euclidean", C, assign, 2, 3)
    assert idx.tolist() == [[1, 0, 2], [5, 4, 3], [5, -1, -1]]
    assert ivf.recall(idx, [[1, 0, 2], [5, 4, 3], [5, 4, 3]]) == (1 + 1 + 1 / 3) / 3
    assert ivf.recall([[-1, -1]], [[0, 1]]) == 0.0 and ivf.recall([[1, 0]], [[0, 1]]) == 1.0


def test_recall_of_the_binding_is_the_restatement(sa):
    rng = np.random.default_rng(3)
    exact = np.array([rng.permutation(50)[:8] for _ in range(40)])
    approx = exact.copy()
    approx[::3, 5:] = -1
    approx[1::3, 0] = 49 - approx[1::3, 0]
    assert sa.knn_recall(approx, exact) == pytest.approx(ivf.recall(approx, exact), abs=1e-15)
    assert sa.knn_recall(exact[:, ::-1], exact) == 1.0
    with pytest.raises(ValueError):
        sa.knn_recall(exact[:3], exact)


# ------------------------------------------------------------------------------------------- the recall precondition
def test_the_clustered_fixture_meets_the_recall_precondition():
    """A condition on the inputs of tests/test_gpu_knn_ivf.py, where the GPU is held to the restatement exactly: on the
    fixture "clustered" (2000 cells, 20 dimensions) the restatement's own recall@20 at 45 lists and 8 probes is at least 0.95."""
    X, label = ivf.clustered()
    assert X.shape == (20, 2000) and X.min() > 0 and np.unique(label).size == 12
    exact = euclid.knn(X, None, 20)[0]
    idx, _, _, assign = ivf.knn_ivf(X, None, 20, None, "euclidean", 45, 8, 10)
    r = ivf.recall(idx, exact)
    print("recall@20 at 45 lists, 8 probes:", r, "list sizes", np.bincount(assign, minlength=45).min(), np.bincount(assign, minlength=45).max())
    assert r >= 0.95
    assert ivf.recall(ivf.knn_ivf(X, None, 20, None, "euclidean", 45, 1, 10)[0], exact) < r      # fewer probes lose neighbours


# ------------------------------------------------------------------------------------------- declarations and binding
def test_the_entries_are_declared_and_bound_alike(sa):
    from singlet_amd import _lib, _marshal
    f64p, i32p, i64p = _lib.f64p, _lib.i32p, _lib.i64p
    i32, i64 = C.c_int32, C.c_int64
    tail = [f64p, i32, i64, f64p, i64, i32p, i32, i32, i32, i32, i32, i32, i32p, f64p]
    assert _lib.SIGNATURES["sgl_knn_ivf"] == (C.c_int, [C.c_void_p] + tail)
    assert _lib.SIGNATURES["sgl_c_knn_ivf"] == (C.c_int, tail)
    assert _lib.SIGNATURES["sgl_knn_ivf_info"] == (C.c_int, [C.c_void_p, i64p])
    assert _lib.SIGNATURES["sgl_op_ivf_train"] == (C.c_int, [C.c_void_p, f64p, i32, i64, i32p, i32, i32, i32, i32, f64p, i32p])
    assert _lib.SIGNATURES["sgl_op_ivf_search"] == (C.c_int, [C.c_void_p, f64p, i32, i64, f64p, i64, i32p, i32, i32, i32, f64p, i32, i32p, i32,
                                                              i64, i32p, f64p])
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    assert "Approximate embedding neighbours" in header
    for name in ("sgl_knn_ivf", "sgl_c_knn_ivf", "sgl_knn_ivf_info", "sgl_op_ivf_train", "sgl_op_ivf_search"):
        m = re.search(r"SGL_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "knn_ivf_host.h")).read()
    assert int(re.search(r"#define KNN_IVF_DEFAULT_PROBES (\d+)", host).group(1)) == _marshal.KNN_IVF_DEFAULT_PROBES
    assert "hip" not in re.sub(r"//.*", "", host).lower()          # the host header makes no HIP call
    for name in ("knn_recall", "knn", "find_neighbors", "run_umap"):
        assert hasattr(sa, name)


def test_the_python_defaults_stay_exact_and_the_ivf_defaults_are_the_stated_ones(sa):
    from singlet_amd import _marshal
    for fn in (sa.knn, sa.Context.knn):
        p = inspect.signature(fn).parameters
        assert p["method"].default == "exact" and p["n_lists"].default is None and p["n_probe"].default is None and p["n_iter"].default == 10
    for fn in (sa.find_neighbors, sa.run_umap):
        p = inspect.signature(fn).parameters
        assert p["nn_method"].default == "exact" and p["n_lists"].default is None and p["n_probe"].default is None
    D = _marshal.KNN_IVF_DEFAULT_PROBES
    assert _marshal.knn_ivf_shape(2000) == (45, min(D, 45)) and _marshal.knn_ivf_shape(2025) == (45, min(D, 45))
    assert _marshal.knn_ivf_shape(2026)[0] == 46 and _marshal.knn_ivf_shape(1) == (1, 1) and _marshal.knn_ivf_shape(3) == (2, min(D, 2))
    assert _marshal.knn_ivf_shape(10 ** 6) == (1000, D) and _marshal.knn_ivf_shape(2 ** 31 - 1)[0] == 46341
    assert _marshal.knn_ivf_shape(10 ** 6, 7, None) == (7, min(D, 7)) and _marshal.knn_ivf_shape(100, 500, 99) == (500, 99)   # given: as it is
    with pytest.raises(ValueError, match="method must be 'exact' or 'ivf'"):
        sa.knn(np.ones((2, 5)), None, 2, method="annoy")
    with pytest.raises(ValueError, match="method must be 'exact' or 'ivf'"):
        sa.find_neighbors(np.ones((5, 2)), 2, nn_method="hnsw")


def test_the_calls_the_binding_makes(sa, monkeypatch):
    """Through a recording stand-in for the library: method "exact" issues the call it issued before; "ivf" issues sgl_c_knn_ivf
    with metric, n_lists, n_probe, n_iter between n_neighbors and the outputs; a short result stops find_neighbors and
    run_umap with a ValueError that names n_probe."""
    from singlet_amd import _lib, api
    calls = []

    class Lib:
        def __getattr__(self, name):
            def fn(*a):
                calls.append((name, a))
                if name == "sgl_c_knn_ivf":            # a result whose last slot is missing
                    idx = np.ctypeslib.as_array(a[-2], shape=(a[2] * a[7],))
                    dist = np.ctypeslib.as_array(a[-1], shape=(a[2] * a[7],))
                    idx[:] = np.tile(np.arange(a[7], dtype=np.int32), a[2])
                    dist[:] = 1.0
                    idx[a[7] - 1::a[7]] = -1
                    dist[a[7] - 1::a[7]] = np.inf
                return 0
            return fn
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    R = np.arange(12.0).reshape(2, 6)
    sa.knn(R, None, 3)
    assert calls[-1][0] == "sgl_c_knn" and len(calls[-1][1]) == 10
    sa.knn(R, None, 3, metric="cosine")
    assert calls[-1][0] == "sgl_c_knn_metric"
    idx, dist = sa.knn(R, None, 3, metric="cosine", method="ivf", n_lists=4, n_probe=2, n_iter=5)
    name, a = calls[-1]
    assert name == "sgl_c_knn_ivf" and len(a) == 14 and a[1:3] == (2, 6) and a[7:12] == (3, 1, 4, 2, 5)
    assert idx[:, -1].tolist() == [-1] * 6 and np.all(np.isinf(dist[:, -1]))
    sa.knn(R, None, 3, method="ivf")
    assert calls[-1][1][7:12] == (3, 0, 3, min(api.knn_ivf_shape(6)[1], 3), 10)
    for call in (lambda: sa.find_neighbors(R.T, 3, nn_method="ivf", n_lists=4, n_probe=1),
                 lambda: sa.run_umap(R, 3, n_epochs=1, init="random", nn_method="ivf", n_lists=4, n_probe=1)):
        n_before = len(calls)
        with pytest.raises(ValueError, match="n_probe"):
            call()
        assert [c[0] for c in calls[n_before:]] == ["sgl_c_knn_ivf"]          # nothing after the search was called


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_host_logic_under_address_and_undefined_sanitizers(tmp_path):
    """knn_ivf_host.h holds no HIP call: it is compiled with a host compiler into a program of its own
    (tests/knn_ivf_host_main.cpp) with both sanitizers and run here, on the CPU, as its own process."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knn_ivf_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "knn_ivf_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "knn_ivf_host: ok" in r.stdout, r.stdout + r.stderr
