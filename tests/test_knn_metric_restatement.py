"""Cosine and correlation neighbours (sgl_knn_metric) without a device: the numpy restatement (tests/knn_metric_restatement.py)
against hand-worked cases, the guarantee of the snap, the fixture "rays", scipy's cdist where scipy is installed; the
declarations of the three new entries and their bindings; through a recording stand-in for _lib.load, that the default metric
still issues sgl_knn / sgl_c_knn with their layout and any other the new entries; the Python refusal; and the metric's argument
rule of singlet_amd/csrc/knn_host.h run as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import embedding_knn_restatement as euclid
import knn_metric_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = ("cosine", "correlation")


def col_dots(UA, UB):
    """dot of column j of UA with column j of UB, by the rule (the diagonal of rs.raw_dots)."""
    acc = np.zeros(UA.shape[1])
    for f in range(UA.shape[0]):
        acc = acc + UA[f] * UB[f]
    return acc


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_cosine_by_hand():
    #                0    1    2     3    4    5    6    7
    R = np.array([[3.0, 4.0, 0.0, -4.0, 0.0, 3.0, 6.0, 4.0],
                  [0.0, 0.0, 4.0, 0.0, 0.0, 4.0, 8.0, -3.0]])
    U, nodir = rs.unit_columns(R, "cosine")
    assert U[:, 0].tolist() == [1.0, 0.0] and U[:, 3].tolist() == [-1.0, 0.0] and U[:, 5].tolist() == [3.0 / 5.0, 4.0 / 5.0]
    assert nodir.tolist() == [False] * 4 + [True] + [False] * 3 and U[:, 4].tolist() == [0.0, 0.0]
    assert np.array_equal(U[:, 5], U[:, 6])                     # a copy scaled by two: the same unit column, bit for bit
    key, count = rs.keys(R, None, "cosine")
    assert count == 1
    assert key[0, 1] == 0.0 and key[0, 0] == 0.0                # parallel, and itself
    assert key[0, 2] == 1.0 and key[2, 3] == 1.0                # orthogonal
    assert key[0, 3] == 2.0 and key[1, 3] == 2.0                # anti-parallel
    assert key[5, 7] == 1.0                                     # (3, 4) . (4, -3): the two products cancel exactly
    assert key[5, 5] == 0.0 and key[5, 6] == 0.0 and not np.signbit(key[5, 6])   # itself and its double
    assert np.all(key[4] == 1.0) and np.all(key[:, 4] == 1.0)   # the zero column: 1.0 to everything, itself included
    idx, dist = rs.knn(R, None, 3, metric="cosine")
    assert idx[0].tolist() == [0, 1, 7] and dist[0].tolist() == [0.0, 0.0, 1.0 - 4.0 / 5.0]
    assert idx[1].tolist() == [0, 1, 7]                                              # its twin 0 precedes the cell itself
    assert idx[6].tolist() == [5, 6, 2] and dist[6].tolist() == [0.0, 0.0, 1.0 - 4.0 / 5.0]
    assert idx[3].tolist() == [3, 2, 4] and dist[3].tolist() == [0.0, 1.0, 1.0]      # 2 and 4 tie at 1: the lower index first
    assert idx[4].tolist() == [0, 1, 2] and dist[4].tolist() == [1.0, 1.0, 1.0]      # no direction: everything ties, by index


def test_correlation_by_hand():
    #                0    1    2    3    4    5
    R = np.array([[0.0, 3.0, 0.0, 0.0, 4.0, 0.0],
                  [3.0, 0.0, 4.0, 0.0, 4.0, 0.0],
                  [0.0, 3.0, 0.0, 4.0, 4.0, 0.0],
                  [3.0, 0.0, 4.0, 4.0, 4.0, 0.0]])
    U, nodir = rs.unit_columns(R, "correlation")
    assert U[:, 0].tolist() == [-0.5, 0.5, -0.5, 0.5] and U[:, 1].tolist() == [0.5, -0.5, 0.5, -0.5]
    assert U[:, 2].tolist() == U[:, 0].tolist() and U[:, 3].tolist() == [-0.5, -0.5, 0.5, 0.5]
    assert nodir.tolist() == [False, False, False, False, True, True]                # the constant and the zero column
    assert np.all(U[:, 4] == 0.0) and np.all(U[:, 5] == 0.0)
    key, count = rs.keys(R, R[:, :2], "correlation")
    assert count == 2 and key.shape == (6, 2)                                        # R's two; the queries have a direction
    assert key[:, 0].tolist() == [0.0, 2.0, 0.0, 1.0, 1.0, 1.0]
    assert rs.keys(R, R, "correlation")[1] == 4
    # under cosine the constant column has a direction
    assert rs.unit_columns(R, "cosine")[1].tolist() == [False] * 5 + [True]
    # one dimension: every column is its own mean
    assert rs.unit_columns(np.array([[1.0, -2.0, 0.0]]), "correlation")[1].all()
    assert rs.unit_columns(np.array([[1.0, -2.0, 0.0]]), "cosine")[0].tolist() == [[1.0, -1.0, 0.0]]


def test_overflow_and_underflow_leave_no_direction_and_no_nan():
    R = np.array([[1e200, -1e200, 1e-200, 1.0, 0.0],
                  [1e200, 1e200, -1e-200, 2.0, 0.0],
                  [-1e200, 1e200, 1e-200, 4.0, 0.0]])
    for metric in BOTH:
        U, nodir = rs.unit_columns(R, metric)
        assert nodir.tolist() == [True, True, True, False, True], metric
        assert np.all(U[:, nodir] == 0.0) and not np.isnan(U).any()
        key, count = rs.keys(R, None, metric)
        assert count == 4 and not np.isnan(key).any()
        assert np.all(key[nodir] == 1.0) and np.all(key[:, nodir] == 1.0) and key[3, 3] == 0.0
    assert np.signbit(rs.unit_columns(R, "cosine")[0][2, 0])    # -1e200 / +Inf: a negative zero, as the rule says


def test_euclidean_is_the_existing_restatement():
    rng = np.random.default_rng(3)
    R, Q = rng.standard_normal((5, 40)), rng.standard_normal((5, 7))
    a, b = rs.knn(R, Q, 6, [4, 0, 2], metric="euclidean"), euclid.knn(R, Q, 6, [4, 0, 2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert rs.knn(R, Q, 6, metric="euclidean", with_count=True)[2] == 0
    c = rs.knn(R, Q, 6, [4, 0, 2], metric="cosine")
    d = rs.knn(R[[4, 0, 2]], Q[[4, 0, 2]], 6, metric="cosine")
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1]) and c[0].dtype == np.int32


# --------------------------------------------------------------------------------------------------------------- the snap
def _columns(kind, rng, nd, n):
    if kind == "uniform":
        return rng.random((nd, n))
    if kind == "nmf":
        return rng.random((nd, n)) * (rng.random((nd, n)) < 0.35)
    return rng.lognormal(0.0, 6.0, (nd, n))


@pytest.mark.parametrize("nd", [1, 2, 50, 1024])
@pytest.mark.parametrize("kind", ["uniform", "nmf", "lognormal"])
@pytest.mark.parametrize("metric", BOTH)
def test_the_snap_puts_equal_unit_columns_at_exactly_zero(metric, kind, nd):
    """|1 - dot| of a unit column with itself is the rounding of the rule: bounded by about (2 nd + 4) 2^-53, measured at
    most 22 ulp of 1 (cosine) and 182 (correlation), against the 4096 ulp = 2^-40 of the snap."""
    n = 200
    X = _columns(kind, np.random.default_rng([nd, len(kind), len(metric)]), nd, n)
    U, nodir = rs.unit_columns(X, metric)
    raw = np.abs(1.0 - col_dots(U, U))
    print(metric, kind, nd, "max |1 - dot| in ulp of 1:", raw[~nodir].max() / 2.0 ** -52 if (~nodir).any() else None)
    assert np.all(raw[~nodir] < rs.SNAP)
    if not (nd == 1 and metric == "correlation") and kind != "nmf":
        assert not nodir.any()
    if nd == 1 and metric == "correlation":
        assert nodir.all()
    want = np.where(nodir, 1.0, 0.0)
    for scale in (1.0, 2.0, 2.0 ** 37, 2.0 ** -37):
        V, nodir_v = rs.unit_columns(X * scale, metric)
        assert np.array_equal(V, U) and np.array_equal(nodir_v, nodir), scale     # bitwise-equal unit columns
        key = 1.0 - col_dots(U, V)
        key[key < rs.SNAP] = 0.0
        assert np.array_equal(key, want) and not np.signbit(key).any(), scale
    full, _ = rs.keys(X[:, :40], None, metric)
    assert np.array_equal(np.diag(full), want[:40])
    assert not np.isnan(full).any() and full.min() >= 0.0 and full.max() <= 2.0 + 2.0 ** -40


# ------------------------------------------------------------------------------------------------------------------ rays
def test_rays_cosine_finds_the_programme_where_euclidean_finds_the_magnitude():
    X, label = rs.rays()
    assert X.shape == (10, 600) and X.min() > 0 and X.max() / X.min() > 500
    got = {m: rs.purity(rs.knn(X, None, 15, metric=m)[0], label) for m in ("cosine", "correlation", "euclidean")}
    print(got)
    assert got["cosine"] >= 0.95 and got["correlation"] >= 0.95 and got["euclidean"] <= 0.5


# ----------------------------------------------------------------------------------------------------------------- scipy
@pytest.mark.parametrize("metric", BOTH)
def test_keys_agree_with_scipy_cdist(metric):
    dist = pytest.importorskip("scipy.spatial.distance")
    rng = np.random.default_rng(8)
    R, Q = _columns("nmf", rng, 12, 150), rng.standard_normal((12, 40))
    R[:, 5] = 0.0
    R[:, 9] = 2.5
    key, _ = rs.keys(R, Q, metric)
    zr, zq = rs.unit_columns(R, metric)[1], rs.unit_columns(Q, metric)[1]
    assert zr[5] and (metric == "cosine" or zr[9])
    ok = (~zr[:, None]) & (~zq[None, :]) & (key != 0.0)      # both columns have a direction, the key was not snapped
    want = dist.cdist(R.T, Q.T, metric)
    assert ok.sum() > 5000 and np.max(np.abs(key[ok] - want[ok])) <= 1e-12


# ------------------------------------------------------------------------------------------------- declarations, bindings
def test_header_declares_the_new_entries():
    h = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    tail = ("const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims, int32_t n_dims, "
            "int32_t n_neighbors, int32_t metric, int32_t* idx_out, double* dist_out);")
    assert "SGL_API int sgl_knn_metric(sgl_ctx* ctx, " + tail in flat
    assert "SGL_API int sgl_c_knn_metric(" + tail in flat
    assert "SGL_API int sgl_knn_metric_info(sgl_ctx* ctx, int64_t out[6]);" in flat
    assert "metric = 7 is outside [0, 2]" in flat and "key < 2^-40" in flat and "tests/knn_metric_restatement.py" in flat


def test_the_binding_declares_the_new_entries():
    from singlet_amd import _lib
    i32p, i64p, f64p = _lib.i32p, _lib.i64p, _lib.f64p
    tail = [f64p, C.c_int32, C.c_int64, f64p, C.c_int64, i32p, C.c_int32, C.c_int32, C.c_int32, i32p, f64p]
    assert _lib.SIGNATURES["sgl_knn_metric"] == (C.c_int, [C.c_void_p] + tail)
    assert _lib.SIGNATURES["sgl_c_knn_metric"] == (C.c_int, tail)
    assert _lib.SIGNATURES["sgl_knn_metric_info"] == (C.c_int, [C.c_void_p, i64p])


def test_the_host_rule_and_the_binding_name_the_same_codes():
    from singlet_amd import _marshal
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "knn_host.h")).read()
    for name, code in _marshal.KNN_METRICS.items():
        assert re.search(r"^#define KNN_METRIC_%s %d\b" % (name.upper(), code), host, flags=re.M), name
    assert _marshal.KNN_METRICS == rs.METRICS and re.search(r"^#define KNN_METRIC_MAX 2$", host, flags=re.M)


# ------------------------------------------------------------------------------------------------- the binding's calls
KNN_LAYOUT = "R k n_ref Q n_query dims n_dims n_neighbors idx dist".split()
METRIC_LAYOUT = "R k n_ref Q n_query dims n_dims n_neighbors metric idx dist".split()


class Recorder:
    """Stands in for the loaded library: every attribute is a function that records (name, args) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn

    def take(self, name, layout):
        """The arguments of the one call recorded since the last take, which went to `name`, by the names of layout."""
        from singlet_amd import _lib
        assert [n for n, _ in self.calls] == [name]
        args = self.calls.pop()[1]
        argtypes = _lib.SIGNATURES[name][1]
        assert len(args) == len(argtypes) == len(layout), name
        for t, a in zip(argtypes, args):
            t.from_param(a)   # raises when the argument does not fit the declared type
        return dict(zip(layout, args))


@pytest.fixture
def rec(monkeypatch):
    import singlet_amd as sa
    from singlet_amd import _lib
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(sa.Context, "dims", lambda self: (7, 11, 30))
    return r


def test_one_shot_default_issues_sgl_c_knn_and_a_metric_the_new_entry(rec):
    import singlet_amd as sa
    R, Q = np.asfortranarray(np.arange(33.0).reshape(3, 11)), np.ones((3, 4))
    for kw in ({}, {"metric": "euclidean"}):
        sa.knn(R, Q, 5, dims=[2, 0], **kw)
        got = rec.take("sgl_c_knn", KNN_LAYOUT)
        assert (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"]) == (3, 11, 4, 2, 5)
    for name, code in (("cosine", 1), ("correlation", 2)):
        idx, dist = sa.knn(R, Q, 5, dims=[2, 0], metric=name)
        got = rec.take("sgl_c_knn_metric", METRIC_LAYOUT)
        assert (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"], got["metric"]) == (3, 11, 4, 2, 5, code)
        assert type(got["metric"]) is int
        assert C.cast(got["R"], C.c_void_p).value == R.T.ctypes.data
        assert np.ctypeslib.as_array(got["dims"], (2,)).tolist() == [2, 0]
        assert idx.shape == dist.shape == (4, 5) and idx.dtype == np.int32 and dist.dtype == np.float64
        assert C.cast(got["idx"], C.c_void_p).value == idx.ctypes.data and C.cast(got["dist"], C.c_void_p).value == dist.ctypes.data
    sa.knn(R, metric="cosine")
    got = rec.take("sgl_c_knn_metric", METRIC_LAYOUT)
    assert got["Q"] is None and got["dims"] is None and (got["n_query"], got["n_dims"], got["n_neighbors"]) == (11, 0, 20)


def test_context_default_issues_sgl_knn_and_a_metric_the_new_entry(rec):
    import singlet_amd as sa
    c = sa.Context(0)
    rec.calls.clear()
    c.k = 6
    for kw in ({}, {"metric": "euclidean"}):
        c.knn(**kw)
        got = rec.take("sgl_knn", ["h"] + KNN_LAYOUT)
        assert got["R"] is None and (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"]) == (6, 11, 11, 0, 20)
    idx, dist = c.knn(metric="correlation")
    got = rec.take("sgl_knn_metric", ["h"] + METRIC_LAYOUT)
    assert got["R"] is None and got["Q"] is None and got["dims"] is None
    assert (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"], got["metric"]) == (6, 11, 11, 0, 20, 2)
    assert idx.shape == dist.shape == (11, 20)
    c.knn(3, np.ones((6, 9)), np.ones((6, 2)), np.array([5, 1, 0]), "cosine")      # metric is the last positional
    got = rec.take("sgl_knn_metric", ["h"] + METRIC_LAYOUT)
    assert (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"], got["metric"]) == (6, 9, 2, 3, 3, 1)
    info = c.knn_info()
    rec.take("sgl_knn_info", ["h", "out"])
    assert list(info) == ["instance", "segments", "queries_per_workgroup", "lists_global"]
    info = c.knn_metric_info()
    rec.take("sgl_knn_metric_info", ["h", "out"])
    assert list(info) == ["instance", "segments", "queries_per_workgroup", "lists_global", "metric", "no_direction"]
    assert set(info.values()) == {0}


def test_the_python_refusal_names_the_three_choices(rec):
    import singlet_amd as sa
    R = np.ones((3, 11))
    c = sa.Context(0)
    c.k = 6
    rec.calls.clear()
    for fn in (lambda m: sa.knn(R, metric=m), lambda m: c.knn(metric=m), lambda m: sa.find_neighbors(R.T, k_param=3, metric=m),
               lambda m: sa.find_neighbors(c, k_param=3, metric=m), lambda m: sa.run_umap(R, 3, metric=m)):
        for bad in ("manhattan", "Cosine", "", None, 1):
            with pytest.raises(ValueError, match="'euclidean', 'cosine' or 'correlation'"):
                fn(bad)
    assert rec.calls == []                                   # refused before the library is called


# ------------------------------------------------------------------------------------- find_neighbors, run_umap on the host
def test_the_composed_calls_hand_the_metric_on_and_the_default_calls_as_before(monkeypatch):
    import singlet_amd as sa
    from singlet_amd import api
    seen = []

    def knn(reference, query=None, n_neighbors=20, dims=None, **kw):
        seen.append(kw)
        return rs.knn(reference, query, n_neighbors, dims, kw.get("metric", "euclidean"))

    class Ctx(sa.Context):
        def __init__(self):
            self.k = 4

        def __del__(self):
            pass

        def dims(self):
            return (9, 60, 100)

        def get_factors(self, w=True, d=True, h=True):
            return None, None, E

        def knn(self, n_neighbors=20, reference=None, query=None, dims=None, **kw):
            seen.append(("ctx", kw))
            return rs.knn(E.T, None, n_neighbors, dims, kw.get("metric", "euclidean"))

    monkeypatch.setattr(api, "knn", knn)
    monkeypatch.setattr(api, "c_SNN", lambda G, prune, threads: "snn")
    monkeypatch.setattr(api, "fuzzy_simplicial_set", lambda idx, dist: (idx, dist))
    monkeypatch.setattr(api, "umap_layout", lambda G, Y0, *a: Y0)
    E = np.random.default_rng(11).random((60, 4))               # cells x factors
    out = sa.find_neighbors(E, k_param=8)
    assert seen.pop() == {}                                     # the default: the very call of before, no keyword
    want = rs.knn(E.T, None, 8, metric="cosine")
    out = sa.find_neighbors(E, k_param=8, metric="cosine", return_dist=True)
    assert seen.pop() == {"metric": "cosine"}
    assert np.array_equal(out["idx"], want[0]) and np.array_equal(out["dist"], want[1]) and out["snn"] == "snn"
    for j in range(60):
        rows = out["nn"].i[8 * j:8 * j + 8]
        assert rows.tolist() == sorted(want[0][j].tolist())
        assert out["nn"].x[8 * j:8 * j + 8].tolist() == [want[1][j][want[0][j].tolist().index(r)] for r in rows]
    c = Ctx()
    sa.find_neighbors(c, k_param=8)
    assert seen.pop() == ("ctx", {})
    sa.find_neighbors(c, k_param=8, metric="correlation")
    assert seen.pop() == ("ctx", {"metric": "correlation"})
    Y0 = np.zeros((60, 2))
    sa.run_umap(E.T, 5, init=Y0)
    assert seen.pop() == {}
    _, G = sa.run_umap(E.T, 5, init=Y0, metric="cosine", return_graph=True)
    assert seen.pop() == {"metric": "cosine"}
    want = rs.knn(E.T, None, 5, metric="cosine")
    assert np.array_equal(G[0], want[0]) and np.array_equal(G[1], want[1])
    sa.run_umap(c, 5, init=Y0)
    assert seen.pop() == ("ctx", {})
    sa.run_umap(c, 5, init=Y0, metric="correlation")
    assert seen.pop() == ("ctx", {"metric": "correlation"}) and seen == []
    assert "Seurat's RunUMAP defaults to metric = \"cosine\"" in sa.run_umap.__doc__


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_metric_rule_under_address_and_undefined_sanitizers(tmp_path):
    """The metric's argument rule holds no HIP call: it is compiled with a host compiler into a program of its own
    (tests/knn_metric_host_main.cpp) with both sanitizers and run here, on the CPU, as its own process."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knn_metric_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "knn_metric_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "knn_metric_host: ok" in r.stdout, r.stdout + r.stderr
