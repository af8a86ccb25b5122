"""Embedding neighbours (sgl_knn) without a device: the numpy restatement against hand-worked cases, the declaration of the
three entries and the build rule of their unit, the binding's argument layout through a recording stand-in for _lib.load,
the host logic of find_neighbors, and the library's own host logic (singlet_amd/csrc/knn_host.h) run as a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import embedding_knn_restatement as rs
import local_neighbors_restatement as lnr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_a_tie_goes_to_the_lower_index():
    R = np.array([[0.0, 1.0, -1.0, 2.0, -1.0]])
    idx, dist = rs.knn(R, None, 3)
    assert idx[0].tolist() == [0, 1, 2] and dist[0].tolist() == [0.0, 1.0, 1.0]     # 1, 2 and 4 tie at 1: 1 and 2 enter
    assert idx[3].tolist() == [3, 1, 0] and dist[3].tolist() == [0.0, 1.0, 2.0]
    assert idx[4].tolist() == [2, 4, 0]                                             # its twin 2 precedes the cell itself


def test_k_plus_one_duplicates_push_a_cell_out_of_its_own_list():
    R = np.array([[5.0, 5.0, 5.0, 5.0, 9.0], [1.0, 1.0, 1.0, 1.0, 0.0]])
    idx, dist = rs.knn(R, None, 3)
    for j in range(4):
        assert idx[j].tolist() == [0, 1, 2] and dist[j].tolist() == [0.0, 0.0, 0.0]
    assert 3 not in idx[3]
    assert idx[4, 0] == 4


def test_sums_that_overflow_tie_at_infinity_and_rank_by_index():
    R = np.array([[0.0, 1e200, -1e200, 1e200]])
    idx, dist = rs.knn(R, None, 4)
    assert idx[0].tolist() == [0, 1, 2, 3] and dist[0].tolist() == [0.0, INF, INF, INF]
    assert idx[1].tolist() == [1, 3, 0, 2] and dist[1].tolist() == [0.0, 0.0, INF, INF]
    assert not np.isnan(dist).any()


def test_two_sums_with_equal_roots_rank_by_the_sums():
    e = 2.0 ** -26
    R = np.array([[1.0, 1.0, 0.0], [e, 0.0, 0.0]])     # from cell 2: s = 1 + 2^-52 to cell 0, s = 1 to cell 1
    assert 1.0 + e * e > 1.0 and np.sqrt(1.0 + e * e) == 1.0
    idx, dist = rs.knn(R, None, 3)
    assert idx[2].tolist() == [2, 1, 0]                 # by the roots the two would tie and 0 would precede 1
    assert dist[2].tolist() == [0.0, 1.0, 1.0]


def test_dims_select_and_order_the_rows():
    rng = np.random.default_rng(3)
    R, Q = rng.standard_normal((5, 40)), rng.standard_normal((5, 7))
    d = [4, 0, 2]
    a = rs.knn(R, Q, 6, d)
    b = rs.knn(R[d], Q[d], 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].shape == (7, 6) and a[0].dtype == np.int32


# ------------------------------------------------------------------------------------------ declarations and the build rule
def test_header_declares_the_three_entries_and_keeps_the_version():
    h = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    tail = ("const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims, int32_t n_dims, "
            "int32_t n_neighbors, int32_t* idx_out, double* dist_out);")
    assert "SGL_API int sgl_knn(sgl_ctx* ctx, " + tail in flat
    assert "SGL_API int sgl_c_knn(" + tail in flat
    assert "SGL_API int sgl_knn_info(sgl_ctx* ctx, int64_t out[4]);" in flat
    assert ("SGL_API int sgl_abi_version(void);   /* 2: native multi-GPU section, sgl_nmf_iterate, chunk-list / dense ARD entry "
            "points */") in h


def test_the_unit_is_compiled_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_knn.o" in objs
    assert re.search(r"^kernels_knn\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^kernels_knn\.o: knn_host\.h$", mk, flags=re.M)


def test_the_binding_declares_the_three_entries():
    from singlet_amd import _lib
    i32p, i64p, f64p = _lib.i32p, _lib.i64p, _lib.f64p
    tail = [f64p, C.c_int32, C.c_int64, f64p, C.c_int64, i32p, C.c_int32, C.c_int32, i32p, f64p]
    assert _lib.SIGNATURES["sgl_knn"] == (C.c_int, [C.c_void_p] + tail)
    assert _lib.SIGNATURES["sgl_c_knn"] == (C.c_int, tail)
    assert _lib.SIGNATURES["sgl_knn_info"] == (C.c_int, [C.c_void_p, i64p])


# ------------------------------------------------------------------------------------------------- the binding's calls
KNN_LAYOUT = "R k n_ref Q n_query dims n_dims n_neighbors idx dist".split()


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
        from singlet_amd import _lib
        hits = [a for n, a in self.calls if n == name]
        assert len(hits) == 1, (name, [n for n, _ in self.calls])
        self.calls.clear()
        argtypes = _lib.SIGNATURES[name][1]
        assert len(hits[0]) == len(argtypes) == len(layout), name
        for q, (t, a) in enumerate(zip(argtypes, hits[0])):
            t.from_param(a)   # raises when the argument does not fit the declared type
        return dict(zip(layout, hits[0]))


def addr(p):
    return C.cast(p, C.c_void_p).value


@pytest.fixture
def rec(monkeypatch):
    import singlet_amd as sa
    from singlet_amd import _lib
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(sa.Context, "dims", lambda self: (7, 11, 30))
    return r


def test_one_shot_call_layout(rec):
    import singlet_amd as sa
    R = np.asfortranarray(np.arange(33.0).reshape(3, 11))     # k x n in R's orientation: its column-major image is R.T
    Q = np.ones((3, 4))
    idx, dist = sa.knn(R, Q, 5, dims=[2, 0])
    got = rec.take("sgl_c_knn", KNN_LAYOUT)
    assert (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"]) == (3, 11, 4, 2, 5)
    assert all(type(got[n]) is int for n in ("k", "n_ref", "n_query", "n_dims", "n_neighbors"))
    assert addr(got["R"]) == R.T.ctypes.data                  # no copy of a matrix that is already column-major
    assert np.ctypeslib.as_array(got["dims"], (2,)).tolist() == [2, 0]
    assert idx.shape == dist.shape == (4, 5) and idx.dtype == np.int32 and dist.dtype == np.float64
    assert addr(got["idx"]) == idx.ctypes.data and addr(got["dist"]) == dist.ctypes.data
    sa.knn(R)                                                 # the defaults: the references themselves, 20 neighbours, all rows
    got = rec.take("sgl_c_knn", KNN_LAYOUT)
    assert got["Q"] is None and got["dims"] is None and (got["n_query"], got["n_dims"], got["n_neighbors"]) == (11, 0, 20)
    with pytest.raises(ValueError):
        sa.knn(R, np.ones((2, 4)))
    with pytest.raises(ValueError):
        sa.knn(np.ones(5))
    with pytest.raises(ValueError):
        sa.knn(R, dims=[0.5])


def test_context_call_layout(rec):
    import singlet_amd as sa
    c = sa.Context(0)
    rec.calls.clear()
    c.k = 6
    idx, dist = c.knn()                                       # the resident H: NULL, with the fit's rank and cell count
    got = rec.take("sgl_knn", ["h"] + KNN_LAYOUT)
    assert got["R"] is None and got["Q"] is None and got["dims"] is None
    assert (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"]) == (6, 11, 11, 0, 20)
    assert idx.shape == dist.shape == (11, 20)
    R, Q = np.ones((6, 9)), np.ones((6, 2))
    idx, _ = c.knn(3, R, Q, np.array([5, 1, 0], dtype=np.int64))
    got = rec.take("sgl_knn", ["h"] + KNN_LAYOUT)
    assert got["R"] is not None and got["Q"] is not None
    assert (got["k"], got["n_ref"], got["n_query"], got["n_dims"], got["n_neighbors"]) == (6, 9, 2, 3, 3)
    assert idx.shape == (2, 3)
    c.knn(0)                                                  # out of range: one slot, the library refuses before it writes
    got = rec.take("sgl_knn", ["h"] + KNN_LAYOUT)
    assert got["n_neighbors"] == 0
    info = c.knn_info()
    got = rec.take("sgl_knn_info", ["h", "out"])
    assert list(info) == ["instance", "segments", "queries_per_workgroup", "lists_global"] and set(info.values()) == {0}


# ------------------------------------------------------------------------------------------- find_neighbors on the host
@pytest.fixture
def host_graph(monkeypatch):
    """find_neighbors with the two device calls replaced by their restatements; seen = the arguments they received."""
    import singlet_amd as sa
    from singlet_amd import api
    seen = {}

    def knn(reference, query=None, n_neighbors=20, dims=None):
        seen["knn"] = (np.array(reference), query, n_neighbors, None if dims is None else np.array(dims))
        return rs.knn(reference, query, n_neighbors, dims)

    def c_snn(G, min_similarity, threads):
        seen["snn"] = min_similarity
        p, i, x = lnr.snn(G.i, G.p, G.nrow, G.ncol, min_similarity)
        return sa.dgCMatrix(x, i, p, (G.ncol, G.ncol))

    monkeypatch.setattr(api, "knn", knn)
    monkeypatch.setattr(api, "c_SNN", c_snn)
    return sa, seen


def test_find_neighbors_host_logic(host_graph):
    sa, seen = host_graph
    rng = np.random.default_rng(11)
    E = rng.standard_normal((60, 5))                          # cells x factors
    out = sa.find_neighbors(E, k_param=8, dims=[5, 1, 3], return_dist=True)
    assert list(out) == ["nn", "snn", "idx", "dist"]
    ref, query, K, d0 = seen["knn"]
    assert np.array_equal(ref, E.T) and query is None and K == 8 and d0.tolist() == [4, 0, 2]   # 1-based in, 0-based out
    assert seen["snn"] == np.nextafter(1 / 15, -np.inf)
    idx, dist = rs.knn(E.T, None, 8, [4, 0, 2])
    assert np.array_equal(out["idx"], idx) and np.array_equal(out["dist"], dist)
    nn = out["nn"]
    assert nn.Dim == (60, 60) and nn.p.tolist() == list(range(0, 8 * 60 + 1, 8))
    for j in range(60):
        rows, x = nn.i[8 * j:8 * j + 8], nn.x[8 * j:8 * j + 8]
        assert rows.tolist() == sorted(idx[j].tolist()) and j in rows
        assert x.tolist() == [dist[j][idx[j].tolist().index(r)] for r in rows] and x[rows.tolist().index(j)] == 0.0
    plain = sa.find_neighbors(E, k_param=8, compute_snn=False)
    assert plain["snn"] is None and np.all(plain["nn"].x == 1.0) and seen["knn"][3] is None


def test_find_neighbors_refusals(host_graph):
    sa, _ = host_graph
    E = np.ones((10, 4))
    with pytest.raises(ValueError, match="cells x factors"):
        sa.find_neighbors(np.ones(10))
    with pytest.raises(ValueError, match="requested up to 5 dims but there are only 4"):
        sa.find_neighbors(E, k_param=3, dims=[1, 5])
    with pytest.raises(ValueError, match="1-based"):
        sa.find_neighbors(E, k_param=3, dims=[0, 1])
    with pytest.raises(ValueError, match="1-based"):
        sa.find_neighbors(E, k_param=3, dims=[1.5])
    with pytest.raises(ValueError, match="prune.snn"):
        sa.find_neighbors(E, k_param=3, prune_snn=1.0)


def test_the_next_double_below_prune_makes_the_strict_rule_seurats(host_graph):
    """K = 8: one shared neighbour gives exactly 1 / 15 = prune.  Seurat zeroes what is below prune and keeps equality; c_SNN
    keeps what is strictly above its threshold.  With nextafter(prune, -inf) as the threshold the two graphs are equal; with
    the plain prune they are not."""
    sa, _ = host_graph
    rng = np.random.default_rng(4)
    E = rng.standard_normal((80, 3))
    n, K, prune = 80, 8, 1 / 15
    out = sa.find_neighbors(E, k_param=K, prune_snn=prune)
    want = rs.seurat_snn(out["idx"], n, prune)
    assert np.count_nonzero(want == prune) > 0                # the boundary case occurs
    snn = out["snn"]
    got = np.zeros((n, n))
    got[snn.i, np.repeat(np.arange(n), np.diff(snn.p))] = snn.x
    assert np.array_equal(got, want) and np.all(np.diag(got) == 1.0)
    p, i, x = lnr.snn(out["nn"].i, out["nn"].p, n, n, prune)  # the plain threshold loses the entries at equality
    strict = np.zeros((n, n))
    strict[i, np.repeat(np.arange(n), np.diff(p))] = x
    assert not np.array_equal(strict, want) and np.all(strict[want == prune] == 0.0)


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_host_logic_under_address_and_undefined_sanitizers(tmp_path):
    """The argument rules, the dims check and the launch plan hold no HIP call: they are compiled with a host compiler into a
    program of their own (tests/knn_host_main.cpp) with both sanitizers and run here, on the CPU."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knn_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "knn_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "knn_host: ok" in r.stdout, r.stdout + r.stderr
