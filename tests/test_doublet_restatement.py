"""The doublet scores without a device: the numpy restatement of the pair merge against a dense sum, the score formulas at
hand-computed points, the self-removal rule, the threshold, the binding, every Python-level refusal of score_doublets (all
raised before the first upload, so no device is touched), the host rules of singlet_amd/csrc/doublet_host.h as a stand-alone
program under the address and undefined-behaviour sanitizers, and the two conditions of the planted fixture that the device
test leans on."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import doublet_restatement as rs
import embedding_knn_restatement as euclid
from planted_doublets import N_DOUBLETS, N_GENES, N_SINGLETS, dense_to_csc, planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- the merge
def test_merge_restatement_against_a_dense_sum():
    rng = np.random.default_rng(1)
    D = rng.integers(-2, 3, size=(57, 23)).astype(np.float64) * (rng.random((57, 23)) < 0.4)
    D[:, 4] = 0.0                                                   # an empty column
    D[:, 5] = np.arange(1, 58)                                      # a full one
    x, i, p = dense_to_csc(D)
    pa = np.array([0, 4, 4, 5, 7, 7, 22, 5, 3], dtype=np.int32)
    pb = np.array([1, 4, 2, 5, 7, 8, 0, 4, 3], dtype=np.int32)
    sx, si, sp, shared = rs.pair_columns(x, i, p, pa, pb)
    assert sp.dtype == np.int64 and si.dtype == np.int32 and sp[0] == 0 and sp[-1] == sx.shape[0] == si.shape[0]
    want_shared = 0
    for s, (a, b) in enumerate(zip(pa, pb)):
        rows, vals = si[sp[s]:sp[s + 1]], sx[sp[s]:sp[s + 1]]
        stored = (D[:, a] != 0) | (D[:, b] != 0)                    # dense_to_csc stores the non-zeros: the union of both
        assert np.array_equal(rows, np.flatnonzero(stored)) and np.all(np.diff(rows) > 0)
        assert np.array_equal(vals, (D[:, a] + D[:, b])[stored])    # a cancelled sum stays, as the zero it rounds to
        want_shared += int(((D[:, a] != 0) & (D[:, b] != 0)).sum())
    assert shared == want_shared
    assert sp[2] - sp[1] == 0 and sp[4] - sp[3] == 57               # both empty; the full column with itself


def test_merge_keeps_an_explicit_zero_and_the_bits_of_a_lone_value():
    x = np.array([0.0, -0.0, 5.0, 1e308, 1e308])
    i = np.array([1, 3, 3, 0, 0], dtype=np.int32)
    p = np.array([0, 2, 3, 4, 5], dtype=np.int32)
    sx, si, sp, shared = rs.pair_columns(x, i, p, [0, 0, 2], [1, 0, 3])
    assert si.tolist() == [1, 3, 1, 3, 0] and sp.tolist() == [0, 2, 4, 5] and shared == 1 + 2 + 1
    assert sx[:2].tobytes() == np.array([0.0, 5.0]).tobytes()       # the explicit zero stays stored; -0.0 + 5.0
    assert sx[2:4].tobytes() == np.array([0.0, -0.0]).tobytes()     # 0 + 0 and -0 + -0: IEEE keeps the sign
    assert np.isinf(sx[4])                                          # the overflow the library refuses


def test_path_counts_split_at_the_cap():
    p = np.array([0, 0, 64, 128, 193])                              # lengths 0, 64, 64, 65
    pa, pb = [0, 1, 1, 2, 0], [0, 2, 3, 3, 3]
    assert rs.path_counts(p, pa, pb, 128) == (3, 2)
    assert rs.path_counts(p, pa, pb, 129) == (5, 0)
    assert rs.path_counts(p, pa, pb, 1) == (1, 4)


def test_parents_are_distinct_cells_and_match_the_api():
    import singlet_amd as sa
    for n_obs, n_sim, seed in ((2, 50, 0), (7, 1000, 3), (1200, 2400, 0)):
        a, b = rs.parents(n_obs, n_sim, seed)
        ga, gb = sa.doublet_parents(n_obs, n_sim, seed)
        assert a.dtype == ga.dtype == np.int32 and np.array_equal(a, ga) and np.array_equal(b, gb)
        assert np.all(a != b) and a.min() >= 0 and b.min() >= 0 and a.max() < n_obs and b.max() < n_obs
    with pytest.raises(ValueError):
        sa.doublet_parents(1, 5, 0)
    with pytest.raises(ValueError):
        sa.doublet_parents(5, 0, 0)


# ---------------------------------------------------------------------------------------------------------- the scores
def test_score_formulas_at_hand_computed_points():
    import singlet_amd as sa
    # r = 1, rho = 0.1, q = 1: two observed and two simulated cells, k_adj = 2, every other neighbour simulated gives
    # nd = 2 -> q = 3 / 4; nd = k_adj would need q = (k_adj + 1) / (k_adj + 2) < 1, so q = 1 is taken from the formula itself
    rho, r = 0.1, 1.0
    for q, want in ((1.0, 1.0), (0.5, 0.05 / (0.9 - 0.5 * 0.8))):
        Ld = q * rho / r / (1 - rho - q * (1 - rho - rho / r))
        assert abs(Ld - want) < 1e-15 * 8
    # nd = 0 gives q = 1 / (k_adj + 2): cell 0 sees only observed cells
    idx = np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1], [3, 4, 5], [4, 3, 5], [5, 3, 4]], dtype=np.int32)
    nd, Ld, se = rs.scores(idx, 3, 3)
    assert nd.tolist() == [0, 0, 0, 2, 2, 2]
    q0, q2 = 1 / 4, 3 / 4
    assert Ld[0] == q0 * 0.1 / 1.0 / (1 - 0.1 - q0 * (1 - 0.1 - 0.1 / 1.0))
    assert Ld[3] == q2 * 0.1 / 1.0 / (1 - 0.1 - q2 * (1 - 0.1 - 0.1 / 1.0))
    se_q = math.sqrt(q0 * (1 - q0) / 5)
    den = 1 - 0.1 - q0 * (1 - 0.1 - 0.1 / 1.0)
    assert se[0] == q0 * 0.1 / 1.0 / den ** 2 * math.sqrt((se_q / q0 * 0.9) ** 2 + (0.02 / 0.1 * (1 - q0)) ** 2)
    got = sa.doublet_scores(idx, 3, 3)
    assert np.array_equal(got["nd"], nd[:3]) and np.array_equal(got["sim_nd"], nd[3:])
    assert np.array_equal(got["score"], Ld[:3]) and np.array_equal(got["sim_score"], Ld[3:])
    assert np.array_equal(got["se"], se[:3]) and np.array_equal(got["sim_se"], se[3:])
    # r = 2: the ratio enters as n_sim / n_obs
    idx2 = np.array([[0, 2, 1], [1, 2, 0], [2, 0, 1]], dtype=np.int32)
    nd2, Ld2, _ = rs.scores(idx2, 1, 2)
    q = (nd2[0] + 1) / 4
    assert nd2.tolist() == [2, 1, 1] and Ld2[0] == q * 0.1 / 2.0 / (1 - 0.1 - q * (1 - 0.1 - 0.1 / 2.0))
    assert np.array_equal(sa.doublet_scores(idx2, 1, 2)["score"], Ld2[:1])


def test_self_removal_rule():
    import singlet_amd as sa
    assert rs.remaining_neighbours([4, 9, 7, 8], 4) == [9, 7, 8]    # self first
    assert rs.remaining_neighbours([9, 7, 4, 8], 4) == [9, 7, 8]    # self not first (a duplicate with a lower index precedes it)
    assert rs.remaining_neighbours([9, 7, 6, 8], 4) == [9, 7, 6]    # self absent: the last entry goes
    # 5 observed, 5 simulated cells; row 4 as above, the simulated neighbours are the indices >= 5
    idx = np.tile(np.arange(4, dtype=np.int32), (10, 1))
    idx[np.arange(4), 0], idx[np.arange(4), np.arange(4)] = idx[np.arange(4), np.arange(4)], idx[np.arange(4), 0]
    for row, want in (([4, 9, 7, 8], 3), ([9, 7, 4, 8], 3), ([9, 7, 6, 8], 3), ([9, 7, 6, 1], 3), ([1, 2, 3, 9], 0)):
        idx[4] = row
        nd = rs.scores(idx, 5, 5)[0]
        assert nd[4] == want, row
        assert sa.doublet_scores(idx, 5, 5)["nd"][4] == want, row
    with pytest.raises(ValueError):
        sa.doublet_scores(idx[:9], 5, 5)
    with pytest.raises(ValueError):
        sa.doublet_scores(idx, 5, 5, expected_rate=1.0)


# -------------------------------------------------------------------------------------------------------- the threshold
def two_humps():
    rng = np.random.default_rng(2)
    return np.clip(np.concatenate([rng.normal(0.15, 0.04, 3000), rng.normal(0.7, 0.08, 1500)]), 0.0, None)


def test_threshold_between_two_humps_and_refusal_on_one():
    import singlet_amd as sa
    s = two_humps()
    t = rs.threshold(s)
    assert 0.3 < t < 0.55                                           # the valley, far from either hump
    assert sa.doublet_threshold(s) == t                             # the vectorised form gives the restatement's bin
    assert rs.threshold(s, 50) == sa.doublet_threshold(s, 50)
    one = np.clip(np.random.default_rng(3).normal(0.4, 0.05, 4000), 0.0, None)
    with pytest.raises(ValueError):
        rs.threshold(one)
    with pytest.raises(ValueError, match="local maxima"):
        sa.doublet_threshold(one)
    for bad in ([], [0.0, 0.0], [0.1, float("nan")], [-0.1, 0.4]):
        with pytest.raises(ValueError):
            sa.doublet_threshold(bad)


# ---------------------------------------------------------------------------------------------------------- the binding
def test_the_three_symbols_are_declared_and_bound():
    from singlet_amd import _lib
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    assert _lib.SIGNATURES["sgl_simulate_doublets"] == (C.c_int, [C.c_void_p, C.c_void_p, i32p, i32p, C.c_int64])
    assert _lib.SIGNATURES["sgl_op_pair_columns"] == (C.c_int, [C.c_void_p, i32p, i32p, C.c_int64, C.c_int64, i64p, i32p, f64p])
    assert _lib.SIGNATURES["sgl_doublets_info"] == (C.c_int, [C.c_void_p, i64p])
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    for name in ("sgl_simulate_doublets", "sgl_op_pair_columns", "sgl_doublets_info"):
        assert "SGL_API int %s(" % name in header
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "doublet_host.h")).read()
    assert "#define DOUBLET_LDS_CAP 4096" in host and "LDS path when la + lb <= lds_cap" in header


def test_every_python_refusal_of_score_doublets_comes_before_an_upload(monkeypatch):
    import singlet_amd as sa
    from singlet_amd import context

    def no_context(*a, **kw):
        raise AssertionError("a context was created before the arguments were refused")
    monkeypatch.setattr(context, "Context", no_context)
    fx = planted()
    A = sa.dgCMatrix(fx["x"], fx["i"], fx["p"], fx["dense"].shape)
    w = np.ones((N_GENES, 4))
    ok = dict(w=w)
    cases = [("cells", dict(ok), sa.dgCMatrix(fx["x"][:fx["p"][1]], fx["i"][:fx["p"][1]], fx["p"][:2], (N_GENES, 1))),
             ("sim_ratio", dict(ok, sim_ratio=0), A), ("sim_ratio", dict(ok, sim_ratio=float("nan")), A),
             ("sim_ratio", dict(ok, sim_ratio="2"), A), ("simulated cells", dict(ok, sim_ratio=1e-6), A),
             ("n_neighbors", dict(ok, n_neighbors=0), A), ("n_neighbors", dict(ok, n_neighbors=2.5), A),
             ("sim_ratio = 2.0 and n_neighbors = 86", dict(ok, n_neighbors=86), A),         # 86 x 3 + 1 = 259; 85 x 3 + 1 = 256 still fits
             ("sim_ratio = 20 and n_neighbors = 17", dict(ok, sim_ratio=20), A),            # the default k = 17 at 1200 cells: 358
             ("expected_rate", dict(ok, expected_rate=0.0), A), ("expected_rate", dict(ok, expected_rate=1.0), A),
             ("stdev_rate", dict(ok, stdev_rate=-0.1), A), ("threshold", dict(ok, threshold=float("inf")), A),
             ("sim_batch", dict(ok, sim_batch=-1), A), ("sim_batch", dict(ok, sim_batch=1.5), A),
             ("scale_factor", dict(ok, scale_factor=0), A), ("L1", dict(ok, L1=1.0), A), ("L1", dict(ok, L2=-1.0), A),
             ("either features or nfeatures", dict(rank=4, features=[0, 1, 2, 3], nfeatures=4), A),
             ("nfeatures", dict(rank=4, nfeatures=0), A), ("nfeatures = 601", dict(rank=4, nfeatures=N_GENES + 1), A),
             ("either w", dict(), A), ("either w", dict(w=w, rank=4), A),
             ("share an edge", dict(w=np.ones((N_GENES - 1, 4))), A), ("share an edge", dict(w=w, features=[0, 1, 2]), A),
             ("non-finite", dict(w=np.full((N_GENES, 4), np.nan)), A), ("rank", dict(rank=0), A), ("rank", dict(rank=1025), A),
             ("maxit", dict(rank=4, maxit=0), A)]
    for fragment, kw, M in cases:
        with pytest.raises(ValueError, match=fragment.replace("+", r"\+")):
            sa.score_doublets(M, **kw)
    with pytest.raises(ValueError, match="metric"):
        sa.score_doublets(A, w=w, metric="manhattan")
    with pytest.raises(ValueError):
        sa.score_doublets(A, w=w, nn_method="annoy")
    with pytest.raises((ValueError, IndexError)):
        sa.score_doublets(A, w=np.ones((3, 4)), features=[0, 1, N_GENES])


# ------------------------------------------------------------------------------------------ the host logic, sanitized
def test_host_rules_under_address_and_undefined_sanitizers(tmp_path):
    """doublet_host.h holds no HIP call: it is compiled with a host compiler into a program of its own
    (tests/doublet_host_main.cpp) with both sanitizers and run here, on the CPU, as its own process."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "doublet_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "doublet_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "doublet_host: ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------- the planted fixture
def test_planted_fixture_is_what_it_says():
    fx = planted()
    assert fx["dense"].shape == (N_GENES, N_SINGLETS + N_DOUBLETS) and int(fx["is_doublet"].sum()) == N_DOUBLETS
    assert np.array_equal(fx["dense"], np.trunc(fx["dense"])) and fx["dense"].min() >= 0
    depth = fx["dense"].sum(axis=0)
    assert 1.6 < depth[fx["is_doublet"]].mean() / depth[~fx["is_doublet"]].mean() < 2.4
    assert planted() is fx


@pytest.mark.parametrize("sim_ratio", [1.0, 2.0])
def test_planted_fixture_meets_the_conditions_the_device_test_leans_on(ora, sim_ratio):
    """Rank 4, the oracle's fit and projection, the restated search.  The AUC of the true doublets among the observed scores
    must be at least 0.95, and a relative perturbation of 1e-9 of the joint embedding may change nd in at most 1 % of the
    cells.  Measured with this restatement: AUC 0.9982 at sim_ratio 1 and 0.9994 at sim_ratio 2; no count changed at either
    (a numpy prototype with a plain coordinate-descent fit had given 0.998 - 1.000 at ranks 4, 6 and 8)."""
    fx = planted()
    out = rs.planted_pipe(ora, sim_ratio)
    n_obs, k_adj = out["n_obs"], out["k_adj"]
    assert n_obs == 1200 and out["n_sim"] == int(round(sim_ratio * 1200)) and k_adj == int(round(17 * (1 + sim_ratio)))
    a = rs.auc(out["score"][:n_obs], fx["is_doublet"])
    print("planted fixture, sim_ratio %g: AUC %.4f" % (sim_ratio, a))
    assert a >= 0.95
    E = np.concatenate([out["h_obs"], out["h_sim"]], axis=0)
    Ep = E * (1.0 + 1e-9 * np.random.default_rng(11).uniform(-1.0, 1.0, size=E.shape))
    idx, _ = euclid.knn(Ep.T, None, k_adj + 1)
    nd = rs.scores(idx, n_obs, out["n_sim"])[0]
    changed = int((nd != out["nd"]).sum())
    print("planted fixture, sim_ratio %g: %d of %d counts changed under the perturbation" % (sim_ratio, changed, nd.shape[0]))
    assert changed <= 0.01 * nd.shape[0]
