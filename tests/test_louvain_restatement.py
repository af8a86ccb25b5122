"""Clustering (sgl_c_louvain) without a device: the numpy restatement against hand-worked cases, against a dense
evaluation of the formula and against the quality criterion on the fixture graphs (tests/golden/louvain_graphs.npz, whose
networkx figures were recorded by tests/golden/make_louvain_graphs.py); the declarations of the three entries; the host
logic of find_clusters with the device call replaced by the restatement; and the library's own host logic
(singlet_amd/csrc/cluster_host.h) run as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import louvain_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def graph_of(A):
    """Dense symmetric matrix -> (p, i, x) with rows ascending."""
    A = np.asarray(A, dtype=np.float64)
    p, i, x = [0], [], []
    for c in range(A.shape[1]):
        r = np.flatnonzero(A[:, c])
        i += r.tolist()
        x += A[r, c].tolist()
        p.append(len(i))
    return lr.as_graph(p, i, x)


def dense_of(p, i, x):
    n = len(p) - 1
    A = np.zeros((n, n))
    A[i, np.repeat(np.arange(n), np.diff(p))] = x
    return A


def edges(n, pairs, w=1.0):
    A = np.zeros((n, n))
    for a, b in pairs:
        A[a, b] = A[b, a] = w
    return A


def lattice(w, h):
    pairs = [(y * w + x, y * w + x + 1) for y in range(h) for x in range(w - 1)]
    pairs += [(y * w + x, y * w + x + w) for y in range(h - 1) for x in range(w)]
    return edges(w * h, pairs)


@pytest.fixture(scope="module")
def fixtures():
    z = np.load(os.path.join(ROOT, "tests", "golden", "louvain_graphs.npz"))
    return {str(name): {k: z["%s_%s" % (name, k)] for k in ("p", "i", "x", "planted", "gammas", "nx_q")} for name in z["names"]}


@pytest.fixture(scope="module")
def runs(fixtures):
    """The restatement on every fixture and gamma, computed once: (name, gamma index) -> (result, trace)."""
    out = {}
    for name, f in fixtures.items():
        for a, gamma in enumerate(f["gammas"]):
            trace = []
            out[name, a] = (lr.louvain(f["p"], f["i"], f["x"], float(gamma), trace=trace), trace)
    return out


# ------------------------------------------------------------------------------------------------ the restatement by hand
TWO_TRIANGLES = edges(6, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)])


def test_two_triangles_first_sweep_by_hand():
    """k = 2 2 3 3 2 2, S = 14, all singletons.  0 prefers 1 (1 - 4/14 against 1 - 6/14 for 2) but two singletons move only
    downwards; 1 moves to 0; 2 ties between 0 and 1 (1 - 6/14) and takes the lower; 3 prefers 4 and stays; 4 prefers 5 and
    stays; 5 moves to 4."""
    p, i, x = graph_of(TWO_TRIANGLES)
    new, q0, q1, moved = lr.op_sweep(p, i, x, np.arange(6), 1.0)
    assert new.tolist() == [0, 0, 0, 3, 4, 4] and moved == 3
    assert q0 == pytest.approx(-(4 * 4 + 2 * 9) / 196.0, abs=1e-15)
    assert q1 == pytest.approx((6 / 14 - 0.25) + (0 - 9 / 196) + (2 / 14 - 16 / 196), abs=1e-15)


def test_two_triangles_are_found():
    p, i, x = graph_of(TWO_TRIANGLES)
    r = lr.louvain(p, i, x, 1.0)
    assert r["labels"].tolist() == [0, 0, 0, 1, 1, 1] and r["n_clusters"] == 2
    assert r["q_levels"][r["n_levels"] - 1] == pytest.approx(6 / 7 - 0.5, abs=1e-15)
    assert r["sweeps_levels"][r["n_levels"] - 1] == 0 and np.all(r["q_levels"][r["n_levels"]:] == 0.0)


def test_two_singletons_do_not_swap():
    p, i, x = graph_of(edges(2, [(0, 1)]))
    new, q0, q1, moved = lr.op_sweep(p, i, x, [0, 1], 1.0)
    assert new.tolist() == [0, 0] and moved == 1 and q0 == -0.5 and q1 == 0.0
    new, _, _, moved = lr.op_sweep(p, i, x, [1, 0], 1.0)       # the labels the other way round: now vertex 0 is the higher one
    assert new.tolist() == [0, 0] and moved == 1


def test_a_tie_in_gain_goes_to_the_lower_id():
    p, i, x = graph_of(edges(3, [(0, 2), (2, 1)]))            # the path 0 - 2 - 1: vertex 2 ties between 0 and 1
    new, _, _, moved = lr.op_sweep(p, i, x, [0, 1, 2], 1.0)
    assert new.tolist() == [0, 1, 0] and moved == 1


def test_an_isolated_vertex_never_moves():
    A = edges(5, [(0, 1), (1, 2)])
    A[4, 4] = 3.0                                              # vertex 3 has nothing, vertex 4 only a self-loop
    p, i, x = graph_of(A)
    for labels in ([0, 1, 2, 3, 4], [0, 0, 0, 0, 0], [4, 3, 2, 1, 0]):
        new, _, _, _ = lr.op_sweep(p, i, x, labels, 1.0)
        assert new[3] == labels[3] and new[4] == labels[4]
    r = lr.louvain(p, i, x, 1.0)
    assert r["labels"].tolist() == [0, 0, 0, 1, 2]             # by size, then by smallest member


def test_a_self_loop_counts_once_in_k():
    A = edges(3, [(0, 1), (1, 2)], 2.0)
    A[1, 1] = 0.5
    p, i, x = graph_of(A)
    k, S = lr.degrees(p, i, x)
    assert k == [2.0, 4.5, 2.0] and S == 8.5
    q, tot, size = lr.modularity(p, i, x, [0, 0, 2], 1.0, k, S)
    assert tot == [6.5, 0.0, 2.0] and size == [2, 0, 1]
    assert q == pytest.approx((2.0 + 2.0 + 0.5) / 8.5 - (6.5 / 8.5) ** 2 - (2.0 / 8.5) ** 2, abs=1e-15)


def test_the_guard_discards_a_sweep_that_lowers_q():
    """A 3 x 3 unweighted lattice: the second synchronous sweep of level 0 would lower Q (many gains tie); it is discarded,
    the level ends with the labels of the first sweep, and the next level starts from their Q."""
    p, i, x = graph_of(lattice(3, 3))
    trace = []
    r = lr.louvain(p, i, x, 1.0, trace=trace)
    level0 = [(what, q) for level, what, q in trace if level == 0]
    assert [what for what, _ in level0] == ["start", "kept", "discarded"]
    assert level0[2][1] < level0[1][1] and r["q_levels"][0] == level0[1][1] and r["sweeps_levels"][0] == 1
    first, _, q1, _ = lr.op_sweep(p, i, x, np.arange(9), 1.0)
    assert q1 == level0[1][1]
    _, _, q2, moved = lr.op_sweep(p, i, x, first, 1.0)
    assert moved > 0 and q2 == level0[2][1]
    assert [q for level, what, q in trace if (level, what) == (1, "start")][0] == pytest.approx(r["q_levels"][0], abs=1e-12)


def test_blocked_sum_is_sequential_up_to_one_block_and_blocked_above():
    rng = np.random.default_rng(5)
    v = rng.random(3000).tolist()
    assert lr.blocked_sum(v[:1024]) == lr.seq_sum(v[:1024])
    want = ((0.0 + lr.seq_sum(v[:1024])) + lr.seq_sum(v[1024:2048])) + lr.seq_sum(v[2048:])
    assert lr.blocked_sum(v) == want and lr.blocked_sum([]) == 0.0
    assert lr.blocked_sum(v[:2048]) == lr.seq_sum(v[:1024]) + lr.seq_sum(v[1024:2048])


def test_renumbering_by_size_then_smallest_member():
    lab, n = lr.renumber_by_size([5, 2, 2, 5, 0, 2, 7, 7])
    assert lab.tolist() == [1, 0, 0, 1, 3, 0, 2, 2] and n == 4 and lab.dtype == np.int32
    assert lr.renumber_by_size([])[1] == 0


# ----------------------------------------------------------------------------------------------- quality and invariants
def test_quality_criterion_on_every_fixture(fixtures, runs):
    """Q >= min_nx - (max_nx - min_nx) over networkx seeds 0 .. 9; where networkx always reaches the same Q, equality to
    1e-12."""
    assert sorted(fixtures) == ["cliques", "sbm", "snn_diag", "snn_noisy", "snn_weak20"]
    assert fixtures["snn_noisy"]["gammas"].tolist() == [0.5, 1.0, 2.0]
    for (name, a), (r, _) in runs.items():
        nxq = fixtures[name]["nx_q"][a]
        assert nxq.shape == (10,)
        q, lo, hi = r["q_levels"][r["n_levels"] - 1], nxq.min(), nxq.max()
        print(name, fixtures[name]["gammas"][a], "Q", q, "networkx", lo, hi, "clusters", r["n_clusters"])
        if hi - lo < 1e-12:
            assert abs(q - lo) <= 1e-12, (name, a, q, lo)
        else:
            assert q >= lo - (hi - lo), (name, a, q, lo, hi)


def test_planted_partitions_of_the_cliques_and_the_block_model_are_recovered(fixtures, runs):
    for name in ("cliques", "sbm"):
        r, _ = runs[name, 0]
        planted = fixtures[name]["planted"]
        assert r["n_clusters"] == np.unique(planted).size
        assert np.unique(np.stack([planted, r["labels"]]), axis=1).shape[1] == r["n_clusters"]   # a bijection of the labels


def test_q_is_monotone_over_sweeps_and_equal_across_an_aggregation(runs):
    for (name, a), (r, trace) in runs.items():
        assert r["n_levels"] >= 2
        last = None
        for level, what, q in trace:
            if what == "start":
                if level > 0:
                    assert abs(q - r["q_levels"][level - 1]) <= 1e-12, (name, level)
                last = q
            elif what == "kept":
                assert q > last, (name, level)
                last = q
            else:
                assert q <= last
        assert np.all(np.diff(r["q_levels"][:r["n_levels"]]) >= -1e-12)


def test_q_against_a_dense_evaluation(fixtures, runs):
    for name, a in (("cliques", 0), ("sbm", 0), ("snn_noisy", 0), ("snn_noisy", 2), ("snn_diag", 0)):
        f = fixtures[name]
        r, _ = runs[name, a]
        gamma = float(f["gammas"][a])
        p, i, x = lr.as_graph(f["p"], f["i"], f["x"])
        want = lr.dense_modularity(dense_of(p, i, x), r["labels"], gamma)
        assert lr.modularity(p, i, x, r["labels"], gamma)[0] == pytest.approx(want, abs=1e-12)
        assert r["q_levels"][r["n_levels"] - 1] == pytest.approx(want, abs=1e-12)


def test_labels_are_numbered_by_descending_size(runs):
    for r, _ in runs.values():
        count = np.bincount(r["labels"])
        assert count.size == r["n_clusters"] and np.all(count > 0) and np.all(np.diff(count) <= 0)


def test_aggregation_keeps_the_weight_and_the_column_major_order():
    p, i, x = graph_of(TWO_TRIANGLES)
    cmap, (cp, ci, cx) = lr.aggregate(p, i, x, [0, 0, 0, 3, 4, 4])
    assert cmap.tolist() == [0, -1, -1, 1, 2, -1]
    # communities {0, 1, 2}, {3}, {4, 5}: a self-loop carries twice the intra edges; {3} has none, so no entry is stored
    assert cp.tolist() == [0, 2, 4, 6] and ci.tolist() == [0, 1, 0, 2, 1, 2]
    assert cx.tolist() == [6.0, 1.0, 1.0, 2.0, 2.0, 2.0]
    assert dense_of(cp, ci, cx).sum() == TWO_TRIANGLES.sum()


# ------------------------------------------------------------------------------------------ declarations and the build rule
def test_header_declares_the_entries_and_keeps_the_version():
    h = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("SGL_API int sgl_c_louvain(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* resolutions, "
            "int32_t n_res, double tol, int32_t max_sweeps, int32_t max_levels, int32_t* labels, int32_t* n_clusters, "
            "int32_t* n_levels, double* q_levels, int32_t* sweeps_levels);") in flat
    assert ("SGL_API int sgl_op_louvain_sweep(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, "
            "const int32_t* labels_in, double resolution, int32_t* labels_out, double* q_in, double* q_out, int64_t* moved_out);") in flat
    assert "SGL_API int sgl_louvain_info(int64_t out[4]);" in flat
    assert ("SGL_API int sgl_abi_version(void);   /* 2: native multi-GPU section, sgl_nmf_iterate, chunk-list / dense ARD entry "
            "points */") in h


def test_the_unit_is_compiled_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_cluster.o" in objs
    assert re.search(r"^kernels_cluster\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^kernels_cluster\.o: cluster_host\.h$", mk, flags=re.M)


def test_the_binding_declares_the_entries():
    from singlet_amd import _lib
    i32p, i64p, f64p = _lib.i32p, _lib.i64p, _lib.f64p
    csc = [f64p, i32p, i32p]
    assert _lib.SIGNATURES["sgl_c_louvain"] == (C.c_int, csc + [C.c_int32, f64p, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                                                i32p, i32p, i32p, f64p, i32p])
    assert _lib.SIGNATURES["sgl_op_louvain_sweep"] == (C.c_int, csc + [C.c_int32, i32p, C.c_double, i32p, f64p, f64p, i64p])
    assert _lib.SIGNATURES["sgl_louvain_info"] == (C.c_int, [i64p])


def test_the_fast_path_width_in_the_header_text_is_the_builds():
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "cluster_host.h")).read()
    cap = int(re.search(r"^#define LOUVAIN_FAST_DEGREE (\d+)", host, flags=re.M).group(1))
    block = int(re.search(r"^#define LOUVAIN_SUM_BLOCK (\d+)", host, flags=re.M).group(1))
    h = re.sub(r"\s+", " ", re.sub(r"\n \* ", "\n", open(os.path.join(ROOT, "include", "singlet_hip.h")).read()))
    assert "columns of up to %d stored entries (the fast path)" % cap in h
    assert block == lr.BLOCK and "blocks of %d consecutive terms" % block in h
    assert cap & (cap - 1) == 0 and cap >= 64                 # the LDS sort needs a power of two


# ------------------------------------------------------------------------------------------- find_clusters on the host
@pytest.fixture
def host_clusters(monkeypatch):
    """find_clusters with the device call replaced by the restatement; seen = the graph and arguments it received."""
    import singlet_amd as sa
    from singlet_amd import api
    seen = {}

    def c_louvain(G, resolutions, tol=1e-7, max_sweeps=64, max_levels=32):
        seen.update(G=G, res=np.array(resolutions), tol=tol, max_sweeps=max_sweeps, max_levels=max_levels)
        rs = [lr.louvain(G.p, G.i, G.x, float(g), tol, max_sweeps, max_levels) for g in resolutions]
        return {"labels": np.stack([r["labels"] for r in rs]), "n_clusters": np.array([r["n_clusters"] for r in rs], dtype=np.int32),
                "n_levels": np.array([r["n_levels"] for r in rs], dtype=np.int32), "q_levels": np.stack([r["q_levels"] for r in rs]),
                "sweeps_levels": np.stack([r["sweeps_levels"] for r in rs])}

    monkeypatch.setattr(api, "c_louvain", c_louvain)
    return sa, seen


def test_find_clusters_host_logic(host_clusters):
    sa, seen = host_clusters
    A = TWO_TRIANGLES + np.eye(6)
    p, i, x = graph_of(A)
    G = sa.dgCMatrix(x, i, p, (6, 6))
    out = sa.find_clusters({"nn": None, "snn": G}, resolution=[0.5, 1.0])
    assert list(out) == ["clusters", "modularity", "n_clusters", "levels"]
    assert seen["G"].nnz == G.nnz - 6 and not np.any(seen["G"].i == np.repeat(np.arange(6), np.diff(seen["G"].p)))
    assert np.array_equal(dense_of(seen["G"].p.astype(np.int64), seen["G"].i, seen["G"].x), TWO_TRIANGLES)
    assert seen["res"].tolist() == [0.5, 1.0] and (seen["tol"], seen["max_sweeps"], seen["max_levels"]) == (1e-7, 64, 32)
    assert out["clusters"].shape == (6, 2) and out["clusters"].dtype == np.int32 and out["clusters"].flags["C_CONTIGUOUS"]
    assert out["clusters"][:, 1].tolist() == [0, 0, 0, 1, 1, 1] and out["n_clusters"].tolist()[1] == 2
    assert out["modularity"][1] == pytest.approx(6 / 7 - 0.5, abs=1e-15) and out["levels"].shape == (2,)
    import scipy.sparse as sp
    kept = sa.find_clusters(sp.csr_matrix(A), resolution=1.0, drop_diagonal=False, tol=0.0, max_sweeps=3, max_levels=2)
    assert seen["G"].nnz == G.nnz and seen["res"].tolist() == [1.0] and (seen["tol"], seen["max_sweeps"], seen["max_levels"]) == (0.0, 3, 2)
    assert kept["clusters"].shape == (6, 1)


def test_find_clusters_refusals(host_clusters):
    sa, _ = host_clusters
    p, i, x = graph_of(TWO_TRIANGLES)
    G = sa.dgCMatrix(x, i, p, (6, 6))
    with pytest.raises(ValueError, match="compute_snn"):
        sa.find_clusters({"nn": G, "snn": None})
    with pytest.raises(ValueError, match="square"):
        sa.find_clusters(sa.dgCMatrix([1.0], [0], [0, 1, 1], (3, 2)))
    for bad in (0.0, -1.0, np.inf, np.nan, [1.0, 0.0], []):
        with pytest.raises(ValueError, match="resolution"):
            sa.find_clusters(G, resolution=bad)
    with pytest.raises(TypeError):
        sa.find_clusters(np.ones((3, 3)))


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_host_logic_under_address_and_undefined_sanitizers(tmp_path):
    """The argument rules, the naming of a defect, the guard, the path split and the renumbering hold no HIP call: they are
    compiled with a host compiler into a program of their own (tests/cluster_host_main.cpp) with both sanitizers and run
    here, on the CPU."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cluster_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cluster_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "cluster_host: ok" in r.stdout, r.stdout + r.stderr
