"""The numpy restatement of the neighbourhood enrichment calls (nhood_restatement.py) against the dense definition in integers,
its permutations against the (key, index) rule written out, its statistics against numpy's float mean / std over the null
tensor and a direct restatement of p and Benjamini-Hochberg; the library's host code (sgl_nhood_stats; no device) against the
restatement bit for bit; the stand-alone host program under the sanitizers; the planted fixture, the calibration, the ABI
symbols and the refusals of the front-end."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import nhood_restatement as nh
from gsea_restatement import bh_plain, rand2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgl_nhood_enrichment", "sgl_c_nhood_enrichment", "sgl_nhood_stats", "sgl_op_nhood_permute", "sgl_op_nhood_tally", "sgl_nhood_info")
U64 = np.uint64
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def random_graph(n, seed, hub=0):
    """An asymmetric graph with repeated rows, unsorted rows, self-loops, empty columns (0, n - 1 and every 5th) and, with
    `hub`, one column of that many entries: (Gi, Gp) int32."""
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for j in range(n):
        if j in (0, n - 1) or j % 5 == 4:
            rows = np.zeros(0, dtype=np.int64)
        elif hub and j == 2:
            rows = rng.integers(0, n, hub)
        else:
            rows = rng.integers(0, n, int(rng.integers(1, 9)))      # with replacement: repeated rows, any order
            if j % 3 == 0:
                rows[0] = j                                         # a self-loop
            if j % 6 == 1 and rows.shape[0] > 1:
                rows[1] = rows[0]                                   # a repeated row for certain
        Gi.extend(rows.tolist())
        Gp.append(len(Gi))
    return np.array(Gi, dtype=np.int32), np.array(Gp, dtype=np.int32)


# --------------------------------------------------------------------------------------------------------- definition
@pytest.mark.parametrize("n,K,hub", [(1, 1, 0), (2, 2, 0), (7, 3, 0), (64, 5, 0), (65, 1, 0), (200, 4, 120), (333, 9, 700)])
@pytest.mark.parametrize("drop", [True, False])
def test_tally_equals_the_dense_definition(n, K, hub, drop):
    Gi, Gp = random_graph(n, 100 + n, hub)
    lab = np.random.default_rng(n).integers(0, K, n)
    if K > 2:
        lab[lab == K - 1] = 0                                       # a class without cells
    B = np.zeros((n, n), dtype=np.int64)                            # B[i, j] = how often row i is stored in column j
    np.add.at(B, (Gi.astype(np.int64), nh.columns(Gp)), 1)
    if drop:
        np.fill_diagonal(B, 0)
    O = (lab[:, None] == np.arange(K)[None, :]).astype(np.int64)    # one-hot, n x K
    want = O.T @ B.T @ O                                            # [a, b] = sum_ij O[j, a] B[i, j] O[i, b]
    got = nh.tally(Gi, Gp, lab, K, drop)
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    assert int(got.sum()) == int(B.sum())
    if K > 2:
        assert not got[K - 1].any() and not got[:, K - 1].any()


# ------------------------------------------------------------------------------------------------------- permutations
def test_permutations_keep_class_sizes_differ_and_follow_the_key_index_order():
    n, K, seed = 300, 5, 11
    lab = np.random.default_rng(1).integers(0, K, n)
    P = nh.permuted(lab, seed, 0, 20)
    sizes = np.bincount(lab, minlength=K)
    assert all(np.bincount(row, minlength=K).tolist() == sizes.tolist() for row in P)
    orders = [tuple(nh.order(seed, r, n).tolist()) for r in range(20)]
    assert len(set(orders)) == 20 and all(sorted(o) == list(range(n)) for o in orders)
    # the rule written out: cells ascending by (key, c), keys from the counter hash
    for r in (0, 7, 19):
        key = [int(rand2(seed, U64(r), U64(c))) for c in range(n)]
        assert list(orders[r]) == [c for _, c in sorted((key[c], c) for c in range(n))]
        assert P[r].tolist() == lab[list(orders[r])].tolist()
    assert nh.permuted(lab, seed, 7, 3).tolist() == P[7:10].tolist()            # r0 is the permutation's own index
    assert nh.permuted(lab, seed + 1, 0, 1).tolist() != P[:1].tolist()


# --------------------------------------------------------------------------------------------------------- statistics
def small_case():
    def make():
        Gi, Gp = random_graph(120, 5, 40)
        lab = np.random.default_rng(2).integers(0, 4, 120)
        lab[lab == 3] = 1                                           # class 3 empty: D == 0 on its pairs
        return Gi, Gp, lab, nh.enrichment(Gi, Gp, lab, 4, 150, 3, True)
    return cached("small", make)


def test_statistics_against_numpy_over_the_null_tensor():
    """z, mean and sd against numpy's float mean and std (ddof 0) over the null tensor at a relative 1e-12 where D > 0; D == 0
    gives NaN for z and 0 for sd; p and Benjamini-Hochberg against a direct restatement."""
    Gi, Gp, lab, out = small_case()
    N, Cobs, nperm = out["null"].astype(np.float64), out["counts"].astype(np.float64), 150
    mean, sd = N.mean(axis=0), N.std(axis=0)
    D = nperm * out["S2"] - out["S1"] ** 2
    pos = D > 0
    assert pos.sum() == 9 and (D[3] == 0).all() and (D[:, 3] == 0).all()
    assert np.allclose(out["mean"], mean, rtol=1e-12, atol=0)
    assert np.allclose(out["sd"][pos], sd[pos], rtol=1e-12, atol=0) and (out["sd"][~pos] == 0).all()
    assert np.allclose(out["zscore"][pos], (Cobs[pos] - mean[pos]) / sd[pos], rtol=1e-12, atol=0)
    assert np.isnan(out["zscore"][~pos]).all() and np.isfinite(out["zscore"][pos]).all()
    pe = (1.0 + (out["null"] >= out["counts"][None]).sum(axis=0)) / (1.0 + nperm)
    pd = (1.0 + (out["null"] <= out["counts"][None]).sum(axis=0)) / (1.0 + nperm)
    assert out["p_enriched"].tolist() == pe.tolist() and out["p_depleted"].tolist() == pd.tolist()
    assert (out["p_enriched"][~pos] == 1.0).all()
    for p, q in (("p_enriched", "p_adj_enriched"), ("p_depleted", "p_adj_depleted")):
        assert np.array_equal(out[q].T.reshape(-1), bh_plain(out[p].T.reshape(-1)))
        assert (out[q] >= out[p]).all() and (out[q] <= 1.0).all()


def big_integer_cases():
    """(nperm, C, S1, S2) whose D needs more than 64 and more than 53 bits, and D == 0, as Python integers."""
    cases = [(4, 3, 8, 18), (4, 5, 20, 100), (1, 7, 7, 49), (1000, 0, 0, 0)]
    rng = np.random.default_rng(9)
    for nperm, nnz in ((1000, 8_000_000), ((1 << 19) - 1, 1 << 22), (1 << 20, 1 << 21), (2, 2_000_000_001), (999_983, 1_999_993)):
        for spread in (1, 1000, nnz // 3):
            mx = min(nperm, 4096)
            vals = [int(v) for v in rng.integers(max(nnz - spread, 0), nnz + 1, mx)]
            reps = [nperm // mx + (1 if q < nperm % mx else 0) for q in range(mx)]
            S1 = sum(v * m for v, m in zip(vals, reps))
            S2 = sum(v * v * m for v, m in zip(vals, reps))
            assert S2 < 1 << 63
            cases.append((nperm, vals[0], S1, S2))
        cases.append((nperm, nnz, nperm * nnz, nperm * nnz * nnz))  # every C_r = nnz: D == 0 at the largest values
    return cases


def expected_stats(nperm, Cc, S1, S2):
    D = nperm * S2 - S1 * S1
    assert D >= 0
    root = math.sqrt(float(D))
    return (float(nperm * Cc - S1) / root if D else math.nan), float(S1) / float(nperm), root / float(nperm)


def test_library_stats_equal_the_restatement_bit_for_bit():
    import singlet_amd as sa
    Gi, Gp, lab, out = small_case()
    got = sa.nhood_stats(150, *(out[q] for q in ("counts", "S1", "S2", "n_ge", "n_le")))
    assert sorted(got) == sorted(("zscore", "mean", "sd", "p_enriched", "p_depleted", "p_adj_enriched", "p_adj_depleted"))
    for name, v in got.items():
        assert v.tobytes() == out[name].tobytes() or np.array_equal(v, out[name], equal_nan=True), name
    # 128-bit D: values computed here from Python integers
    for nperm, Cc, S1, S2 in big_integer_cases():
        one = np.ones((1, 1), dtype=np.int64)
        st = sa.nhood_stats(nperm, *(np.array([[v]], dtype=np.int64) for v in (Cc, S1, S2)), one, one)
        z, mean, sd = expected_stats(nperm, Cc, S1, S2)
        assert (np.isnan(st["zscore"][0, 0]) if math.isnan(z) else st["zscore"][0, 0] == z), (nperm, Cc, S1, S2)
        assert st["mean"][0, 0] == mean and st["sd"][0, 0] == sd, (nperm, Cc, S1, S2)
    with pytest.raises(sa.SingletHipError, match="not those of"):
        sa.nhood_stats(4, *(np.array([[v]], dtype=np.int64) for v in (3, 8, 15, 1, 1)))    # nperm * S2 < S1^2
    with pytest.raises(sa.SingletHipError, match="nperm"):
        sa.nhood_stats(0, *(np.zeros((2, 2), dtype=np.int64) for _ in range(5)))
    with pytest.raises(ValueError, match="K x K"):
        sa.nhood_stats(10, np.zeros((2, 3), dtype=np.int64), *(np.zeros((2, 2), dtype=np.int64) for _ in range(4)))


# ------------------------------------------------------------------------------------------------ the planted fixture
def planted_reference(seed):
    def make():
        Gi, Gp, lab = nh.planted()
        return Gi, Gp, lab, nh.enrichment(Gi, Gp, lab, 3, 200, seed, True)
    return cached(("planted", seed), make)


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_planted_fixture_meets_the_claims_on_the_restatement_alone(seed):
    Gi, Gp, lab, out = planted_reference(seed)
    assert lab.shape == (576,) and int(Gp[-1]) == 2 * (2 * 23 * 24 + 2 * 23 * 23) == int(np.sum(nh.PLANTED_COUNTS))
    nh.planted_claims(out, 200)
    z = out["zscore"]
    assert 14.0 <= z[0, 1] <= 14.8 and -28.8 <= z[0, 2] <= -26.7 and 29.1 <= z[2, 2] <= 32.0     # the ranges seen over seeds 0, 1, 7


# -------------------------------------------------------------------------------------------------------- calibration
CAL_SEEDS = (0, 1, 2, 3, 7)
CAL_MEASURED = 4.53
CAL_MARGIN = 1.5


def calibration_labels(seed, n):
    """Labels i.i.d. from the counter hash: the hash of (cell) under its own seed, reduced modulo a prime and then modulo 4
    (single bit fields of the hash are periodic in small cell indices; the remainder of a prime mixes all of them)."""
    x = rand2(0xC0FFEE + seed, np.full(n, 5, dtype=U64), np.arange(n, dtype=U64))
    return ((x % U64(1000003)) % U64(4)).astype(np.int32)


def test_calibration_on_hash_labels():
    """Labels that carry no spatial signal (i.i.d. from the hash) on the 24 x 24 grid, K = 4, nperm = 500: max |z| over the
    pairs, MEASURED on the CPU with this restatement over the seeds 0, 1, 2, 3, 7: 1.58, 2.98, 1.69, 0.74, 4.52 (CAL_MEASURED
    = 4.53 rounds the largest up).  The bound asserted is CAL_MARGIN = 1.5 times that measurement, 6.8: far below the 14 - 32 of the
    planted fixture, and what a later change of the null would have to stay under.  (The permutations are sorts of hash keys,
    not uniform draws -- DESIGN.md "Neighbourhood enrichment" -- so 4.5 at seed 7 is the hash labels meeting the hash null, not
    a Gaussian tail; labels from numpy's generator gave z with a standard deviation of 0.93 over 12 draws.)"""
    Gi, Gp = nh.grid_graph(24, 24)
    worst = []
    for seed in CAL_SEEDS:
        lab = calibration_labels(seed, 576)
        assert np.bincount(lab, minlength=4).min() > 100
        out = nh.enrichment(Gi, Gp, lab, 4, 500, seed, True)
        assert np.isfinite(out["zscore"]).all()
        worst.append(float(np.abs(out["zscore"]).max()))
    print("calibration: max |z| per seed", [round(w, 3) for w in worst])
    assert max(worst) <= CAL_MEASURED * CAL_MARGIN, worst
    assert max(worst) <= CAL_MEASURED, "the measurement in the docstring no longer holds: %r" % worst


# ------------------------------------------------------------------------------------------- the host logic, sanitized
def test_host_rules_under_address_and_undefined_sanitizers(tmp_path):
    """nhood_host.h holds no HIP call: it is compiled with a host compiler into a program of its own
    (tests/nhood_host_main.cpp) with both sanitizers and run here, on the CPU, as its own process; the statistics are held
    against values computed here from Python integers (a file of cases given as its argument)."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "nhood_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "nhood_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases = big_integer_cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for nperm, Cc, S1, S2 in cases:
            z, mean, sd = expected_stats(nperm, Cc, S1, S2)
            f.write("%d %d %d %d %s %s %s\n" % (nperm, Cc, S1, S2, "nan" if math.isnan(z) else z.hex(), mean.hex(), sd.hex()))
    assert any(nperm * S2 - S1 * S1 >= 1 << 64 for nperm, _, S1, S2 in cases) and any(nperm * S2 == S1 * S1 for nperm, _, S1, S2 in cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "nhood_host: ok" in r.stdout and "%d lines" % len(cases) in r.stdout, r.stdout + r.stderr


def test_the_plan_of_the_restatement_at_its_edges():
    want = {1: 16, 45: 16, 46: 8, 64: 8, 65: 4, 90: 4, 91: 2, 128: 2, 129: 1, 181: 1, 182: 0, 256: 0}
    assert {K: nh.pg_max(K) for K in want} == want
    assert nh.plan(9000, 46, 100) == {"path": 1, "perms_per_group": 8, "lds_bytes": 8 * 46 * 46 * 4, "batch": 100, "sort": 0}
    assert nh.plan(10**6, 20, 1000)["batch"] == 256 and nh.plan(10**6, 20, 1000)["sort"] == 1
    assert nh.plan(9000, 182, 100)["path"] == 2 and nh.plan(9000, 3, 100, path=2)["perms_per_group"] == 16


# --------------------------------------------------------------------------------------------------------------- ABI
def test_the_symbols_are_declared_and_bound():
    from singlet_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    for name in ENTRIES:
        assert "SGL_API int %s(" % name in header and name in _lib.SIGNATURES and hasattr(L, name)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert _lib.SIGNATURES["sgl_op_nhood_tally"] == (C.c_int, [C.c_void_p, i32p, i32p, C.c_int32, i32p, C.c_int32, C.c_int32, C.c_int, C.c_int32,
                                                               C.c_int32, i64p])
    assert _lib.SIGNATURES["sgl_op_nhood_permute"] == (C.c_int, [C.c_void_p, C.c_int32, i32p, C.c_uint64, C.c_int32, C.c_int32, i32p])
    assert _lib.SIGNATURES["sgl_nhood_info"] == (C.c_int, [C.c_void_p, i64p])
    assert "Neighbourhood enrichment" in header and "NO parity with squidpy" in header
    import singlet_amd as sa
    for name in ("nhood_enrichment", "interaction_matrix", "c_nhood_enrichment", "nhood_stats"):
        assert callable(getattr(sa, name))
    for name in ("nhood_enrichment", "op_nhood_permute", "op_nhood_tally", "nhood_info"):
        assert callable(getattr(sa.Context, name))


# ------------------------------------------------------------------------------------------------------ the front-end
def test_every_refusal_of_the_front_end_comes_before_an_upload(monkeypatch):
    import singlet_amd as sa
    from singlet_amd import api, context

    def no_device(*a, **k):
        raise AssertionError("a refusal must come before the first upload")
    monkeypatch.setattr(context.Context, "__init__", no_device)
    monkeypatch.setattr(api, "c_nhood_enrichment", no_device)
    monkeypatch.setattr(api, "spatial_graph", no_device)
    n = 30
    rng = np.random.default_rng(0)
    Gi, Gp = nh.grid_graph(6, 5)
    G = sa.dgCMatrix(np.ones(Gi.shape[0]), Gi, Gp, (n, n))
    xy = rng.random((n, 2))
    lab = rng.integers(0, 3, n)
    f = sa.nhood_enrichment
    empty = sa.dgCMatrix(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(n, dtype=np.int32), (n - 1, n - 1))
    for args, kw, msg in (((lab,), dict(), "exactly one"), ((lab,), dict(graph=G, coords=xy, max_dist=0.3), "exactly one"),
                          ((lab,), dict(graph=G, max_dist=0.3), "max_dist belongs"), ((lab,), dict(coords=xy), "positive max_dist"),
                          ((lab,), dict(coords=xy, max_dist=-1.0), "positive max_dist"), ((lab,), dict(coords=xy[:-1], max_dist=0.3), "n x 2"),
                          ((lab,), dict(graph=empty), "29 cells, the labels 30"),
                          ((lab,), dict(graph=sa.dgCMatrix(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(n + 1, dtype=np.int32), (n + 2, n))), "square"),
                          ((lab,), dict(graph={"snn": None}), "without an SNN graph"),
                          ((lab.astype(np.float64),), dict(graph=G), "integer class"), ((lab.reshape(5, 6),), dict(graph=G), "integer class"),
                          ((lab,), dict(graph=G, n_classes=2), r"labels\[\d+\] = 2 is outside \[0, 2\)"),
                          ((np.where(lab == 0, -1, lab),), dict(graph=G), r"= -1 is outside"),
                          ((lab,), dict(graph=G, n_classes=257), "between 1 and 256"), ((lab + 300,), dict(graph=G), "between 1 and 256"),
                          ((lab,), dict(graph=G, nperm=0), "nperm"), ((lab,), dict(graph=G, nperm=(1 << 20) + 1), "nperm"),
                          ((lab,), dict(graph=G, nperm=2.5), "nperm"), ((lab,), dict(graph=G, batch=-1), "batch"),
                          ((lab,), dict(graph=G, seed=-1), "seed"), ((lab,), dict(graph=G, seed=2**64), "seed")):
        with pytest.raises(ValueError, match=msg):
            f(*args, **kw)
    for args, kw, msg in (((lab, empty), {}, "29 cells"), ((lab.astype(np.float64), G), {}, "integer class"), ((lab, G), dict(n_classes=2), "outside")):
        with pytest.raises(ValueError, match=msg):
            sa.interaction_matrix(*args, **kw)
