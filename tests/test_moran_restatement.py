"""The numpy restatement of the spatial autocorrelation calls (moran_restatement.py) against the definitions computed directly on
the dense n x n weight matrix in long double, the library's host code (sgl_moran_graph_moments, sgl_moran_stats; no device)
against the restatement bit for bit, the stand-alone host program under the sanitizers, and the refusals of the front-end.

THE TOLERANCES were measured on the CPU on the fixtures below (cases()), not chosen:
  * C, the cross product: |C_restated - C_direct| / (sum |w_ij| |x_i - m| |x_j - m| + |m| sum |x_i t_i| + m^2 |S0|), the
    magnitude of the terms the reformulation C = P - m T + m^2 S0 adds and subtracts.  Worst value seen: MEASURED_C = 8.9e-16
    (8.806e-16 at n = 200, the dense gene 5 + U(0, 1) on the symmetric graph with empty columns); the bound is 4 x that,
    C_TOL = 3.6e-15.
  * M2, M4, S0, S1, S2 against the direct sums, relative: worst 8.2e-15 (M2 of the dense gene: the double mean against
    the long double one, amplified by m / sd) -> MOMENT_TOL = 3.3e-14 (4 x).
  * p against scipy.stats.norm (2 sf(|z|), sf(z), cdf(z) at the restated z), relative, down to p = 1e-300: worst 1.4e-13
    (at |z| = 37, where the rounding of z / sqrt 2 is amplified by z^2 = 1.4e3) -> P_TOL = 2.2e-12 (16 x, to cover other
    libm builds, as test_annotate_restatement.py does).
I itself inherits the conditioning of C / M2: it is compared where the test says how."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import sparse
from scipy import stats as sps

import moran_restatement as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4, 5, 64, 65, 200)
MEASURED_C, C_TOL = 8.9e-16, 3.6e-15
MOMENT_TOL = 3.3e-14
P_TOL = 2.2e-12
ENTRIES = ("sgl_moran", "sgl_c_moran", "sgl_moran_embedding", "sgl_c_moran_embedding", "sgl_moran_graph_moments", "sgl_moran_stats",
           "sgl_op_moran_cross", "sgl_moran_info")
_CACHE = {}


def graphs(n, rng):
    """name -> dense W: asymmetric; with a diagonal; with negative weights; symmetric with empty columns."""
    dens = min(0.9, 6.0 / n + 0.15)
    A = rng.random((n, n)) * (rng.random((n, n)) < dens)
    np.fill_diagonal(A, 0.0)
    D = A.copy()
    D[np.arange(n), np.arange(n)] = rng.random(n) + 0.5
    N = A * np.where(rng.random((n, n)) < 0.3, -1.0, 1.0)
    S = np.triu(A, 1)
    S = S + S.T
    S[:, ::3] = 0.0
    S[::3, :] = 0.0
    if not S.any():
        S[1, 2] = S[2, 1] = 1.0
    return {"asymmetric": A, "diagonal": D, "negative": N, "symmetric_empty_columns": S}


def genes(n, rng):
    """name -> dense vector (zeros are the entries not stored)."""
    sparse = rng.poisson(0.3, n).astype(np.float64)
    if not sparse.any():
        sparse[0] = 1.0
    if np.all(sparse == sparse[0]):
        sparse[0] += 1.0
    return {"sparse": sparse, "dense": 5.0 + rng.random(n), "signed": rng.normal(size=n) * (rng.random(n) < 0.6) + (np.arange(n) == 0),
            "log_normalised": np.log1p(rng.poisson(2.0, n) * 3.7)}


def cases():
    """[(n, graph name, gene name, W, x)] -- computed once, shared, never written to."""
    if "cases" not in _CACHE:
        out = []
        for n in SIZES:
            rng = np.random.default_rng(100 + n)
            Ws, xs = graphs(n, rng), genes(n, rng)
            out.extend((n, gn, xn, W, x) for gn, W in Ws.items() for xn, x in xs.items())
        _CACHE["cases"] = out
    return _CACHE["cases"]


def restated(W, x):
    n = W.shape[0]
    Gx, Gi, Gp = mo.csc_graph(W)
    S0, S1, S2, t = mo.graph_moments(Gx, Gi, Gp, n)
    cells = np.nonzero(x)[0]
    m, M2, M4, T, c = mo.gene_moments(x[cells], cells, n, t)
    P = mo.cross_term(x[cells], cells, Gx, Gi, Gp, n)
    mom = np.array([[m], [M2], [M4], [T], [P], [c]], dtype=np.float64)
    return (S0, S1, S2, t), mom


def rel(a, b):
    return float(abs(np.longdouble(a) - b) / abs(b)) if b != 0 else float(abs(a))


def test_restatement_against_the_dense_long_double_definitions():
    worst_c, worst_m, where = 0.0, 0.0, None
    for n, gn, xn, W, x in cases():
        (S0, S1, S2, t), mom = restated(W, x)
        ref = mo.direct(x, W)
        Cr = mo.cross_product(mom, S0)[0]
        ec = float(abs(np.longdouble(Cr) - ref["C"]) / ref["scale"])
        if ec > worst_c:
            worst_c, where = ec, (n, gn, xn)
        for got, want in ((S0, ref["S0"]), (S1, ref["S1"]), (S2, ref["S2"]), (mom[1, 0], ref["M2"]), (mom[2, 0], ref["M4"])):
            worst_m = max(worst_m, rel(got, want))
        assert np.allclose(t, np.asarray(ref["t"], dtype=np.float64), rtol=1e-14, atol=1e-14)
        assert rel(mom[0, 0], ref["mean"]) <= MOMENT_TOL
    print("worst |C - C_direct| / scale: %.3e at %r; worst moment: %.3e" % (worst_c, where, worst_m))
    assert worst_c <= C_TOL, (worst_c, where)
    assert worst_m <= MOMENT_TOL, worst_m


@pytest.mark.parametrize("variance", mo.VARIANCES)
def test_statistics_against_the_definitions(variance):
    """I, sd and z of the assembly against ape's formulas written out in long double on the DIRECT moments.  The restated
    statistics are fed the restated moments, so what is left of the difference is the conditioning of C: the comparison is
    made at the bound that C_TOL implies for each case, C_TOL * scale / |C| (+ the moments' share)."""
    for n, gn, xn, W, x in cases():
        (S0, S1, S2, _), mom = restated(W, x)
        st = mo.stats(n, S0, S1, S2, mom, variance)
        ref = mo.direct(x, W, variance)
        assert float(st["EI"][0]) == float(np.longdouble(-1.0) / (n - 1))
        if ref["C"] == 0 or not np.isfinite(float(ref["sd"])):
            continue   # (n = 4 can give a negative variance under randomisation: sd is NaN on both sides)
        cond = float(ref["scale"] / abs(ref["C"]))
        assert rel(st["I"][0], ref["I"]) <= C_TOL * cond + 4 * MOMENT_TOL, (n, gn, xn)
        # V is a difference of terms of its own; its error is bounded through its largest term
        V, Vr = float(st["sd"][0]) ** 2, float(ref["sd"]) ** 2
        big = max(abs(Vr), 1.0 / (n - 1) ** 2) * 1e3
        assert abs(V - Vr) <= 64 * MOMENT_TOL * big, (n, gn, xn, V, Vr)
    # a negative variance (possible at tiny n) and a constant gene are reported as NaN, not refused
    st = mo.stats(5, 8.0, 16.0, 60.0, np.array([[2.0], [0.0], [0.0], [24.0], [24.0], [5.0]]), variance)
    assert np.isnan(st["I"][0]) and np.isnan(st["z"][0]) and np.isnan(st["p"][0]) and np.isnan(st["p_adj"][0])


def test_p_against_scipy_norm():
    z = np.concatenate([np.linspace(-8, 8, 161), [-37.0, 37.0, 0.0, 1e-8, -1e-8, 12.5, -12.5, 30.0]])
    worst = 0.0
    for alt, ref in (("two.sided", lambda v: 2.0 * sps.norm.sf(abs(v))), ("greater", sps.norm.sf), ("less", sps.norm.cdf)):
        # moments that make I = v * 0.13 - 1 / 9 (mean 0, M2 = 1, n = S0: C = P = I); under normality with S1 = S2 = 0 the
        # sd is sqrt(3 / 99 - 1 / 81) = 0.134, so z runs over about +-37 and p down to 1e-300
        n, S0 = 10, 10.0
        for v in z:
            I = v * 0.13 + (-1.0 / 9.0)
            mom = np.array([[0.0], [1.0], [0.0], [0.0], [I], [n]])
            st = mo.stats(n, S0, 0.0, 0.0, mom, "normality", alt)
            zz = float(st["z"][0]) if np.isfinite(st["z"][0]) else None
            if zz is None:
                continue
            want = float(ref(zz))
            if want < 1e-300:
                continue
            worst = max(worst, abs(float(st["p"][0]) - want) / want)
    # the assembly's own z, on real cases
    for n, gn, xn, W, x in cases()[::7]:
        (S0, S1, S2, _), mom = restated(W, x)
        st = mo.stats(n, S0, S1, S2, mom)
        if np.isfinite(st["z"][0]) and st["p"][0] > 1e-300:
            worst = max(worst, abs(float(st["p"][0]) - 2.0 * sps.norm.sf(abs(float(st["z"][0])))) / float(2.0 * sps.norm.sf(abs(float(st["z"][0])))))
    print("worst relative difference of p against scipy.stats.norm: %.3e" % worst)
    assert worst <= P_TOL, worst


def test_benjamini_hochberg_and_the_ranking():
    p = np.array([0.04, np.nan, 0.01, 0.04, 0.5])
    I = np.array([0.2, np.nan, 0.1, 0.3, 0.9])
    assert mo.rank(p, I, np.arange(5)).tolist() == [2, 3, 0, 4, 1]           # p asc, I desc, NaN last
    import singlet_amd as sa
    assert sa.moran_rank(p, I, np.arange(5)).tolist() == [2, 3, 0, 4, 1]
    padj = mo.ar.bh(p)
    assert np.isnan(padj[1]) and np.allclose(padj[[0, 2, 3, 4]], [4 / 3 * 0.04, 0.04, 4 / 3 * 0.04, 0.5])


# ------------------------------------------------------------------------------------- the library's host code, no device
def test_library_graph_moments_and_stats_equal_the_restatement_bit_for_bit():
    import singlet_amd as sa
    for n, gn, xn, W, x in cases():
        Gx, Gi, Gp = mo.csc_graph(W)
        (S0, S1, S2, t), mom = restated(W, x)
        gm = sa.moran_graph_moments(sa.dgCMatrix(Gx, Gi, Gp, (n, n)))
        assert (gm["S0"], gm["S1"], gm["S2"]) == (S0, S1, S2), (n, gn)
        assert gm["t"].tobytes() == t.tobytes(), (n, gn)
        for variance in mo.VARIANCES:
            for alt in mo.ALTERNATIVES:
                got = sa.moran_stats(n, S0, S1, S2, mom, variance, alt)
                want = mo.stats(n, S0, S1, S2, mom, variance, alt)
                # C is not an output: I = (n / S0) * (C / M2) carries its bits
                for key in ("I", "EI", "sd", "z"):
                    assert got[key].tobytes() == np.asarray(want[key], dtype=np.float64).tobytes(), (n, gn, xn, variance, alt, key)
                ok = ~np.isnan(want["p"])
                assert np.array_equal(np.isnan(got["p"]), ~ok)
                assert np.allclose(got["p"][ok], want["p"][ok], rtol=P_TOL, atol=0)
                assert np.allclose(got["p_adj"][ok], want["p_adj"][ok], rtol=P_TOL, atol=0)


def test_library_stats_over_many_rows_with_a_constant_one():
    import singlet_amd as sa
    rng = np.random.default_rng(3)
    n, W = 65, graphs(65, rng)["negative"]
    Gx, Gi, Gp = mo.csc_graph(W)
    S0, S1, S2, t = mo.graph_moments(Gx, Gi, Gp, n)
    rows = []
    for q in range(12):
        x = np.full(n, 3.0) if q == 5 else rng.poisson(0.5 + q, n).astype(np.float64)
        cells = np.nonzero(x)[0]
        m, M2, M4, T, c = mo.gene_moments(x[cells], cells, n, t)
        rows.append((m, M2, M4, T, mo.cross_term(x[cells], cells, Gx, Gi, Gp, n), c))
    mom = np.array(rows).T
    got, want = sa.moran_stats(n, S0, S1, S2, mom), mo.stats(n, S0, S1, S2, mom)
    assert got["I"].tobytes() == want["I"].tobytes() and np.isnan(got["I"][5]) and np.isnan(got["p_adj"][5])
    ok = ~np.isnan(want["p"])
    assert ok.sum() == 11 and np.allclose(got["p_adj"][ok], want["p_adj"][ok], rtol=P_TOL, atol=0)


def test_library_host_refusals():
    import singlet_amd as sa
    Z = sa.dgCMatrix(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(6, dtype=np.int32), (5, 5))
    with pytest.raises(sa.SingletHipError, match="S0 = 0"):
        sa.moran_graph_moments(Z)
    bad = sa.dgCMatrix(np.array([1.0, np.inf]), np.array([0, 1], dtype=np.int32), np.array([0, 2, 2], dtype=np.int32), (2, 2))
    with pytest.raises(sa.SingletHipError, match="non-finite"):
        sa.moran_graph_moments(bad)
    with pytest.raises(ValueError, match="square"):
        sa.moran_graph_moments(sa.dgCMatrix(np.ones(1), np.zeros(1, dtype=np.int32), np.array([0, 1, 1], dtype=np.int32), (3, 2)))
    mom = np.ones((6, 2))
    with pytest.raises(sa.SingletHipError, match="at least 4"):
        sa.moran_stats(3, 1.0, 1.0, 1.0, mom)
    with pytest.raises(sa.SingletHipError, match="S0 is zero"):
        sa.moran_stats(10, 0.0, 1.0, 1.0, mom)
    with pytest.raises(ValueError, match="variance"):
        sa.moran_stats(10, 1.0, 1.0, 1.0, mom, variance="bootstrap")
    with pytest.raises(ValueError, match="alternative"):
        sa.moran_stats(10, 1.0, 1.0, 1.0, mom, alternative="both")
    with pytest.raises(ValueError, match="6 x rows"):
        sa.moran_stats(10, 1.0, 1.0, 1.0, np.ones((5, 2)))


def test_the_symbols_are_declared_and_bound():
    from singlet_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    for name in ENTRIES:
        assert "SGL_API int %s(" % name in header and name in _lib.SIGNATURES and hasattr(L, name)
    f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert _lib.SIGNATURES["sgl_op_moran_cross"] == (C.c_int, [C.c_void_p, f64p, i32p, i32p, C.c_int32, i32p, C.c_int64, C.c_int32, C.c_int64,
                                                               C.c_int64, f64p])
    assert _lib.SIGNATURES["sgl_moran_info"] == (C.c_int, [C.c_void_p, i64p])
    assert L.sgl_abi_version() == 2


# ------------------------------------------------------------------------------------------- the host logic, sanitized
def test_host_rules_under_address_and_undefined_sanitizers(tmp_path):
    """moran_host.h holds no HIP call: it is compiled with a host compiler into a program of its own
    (tests/moran_host_main.cpp) with both sanitizers and run here, on the CPU, as its own process."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "moran_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "moran_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "moran_host: ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------ the front-end
def test_every_refusal_of_the_front_end_comes_before_an_upload(monkeypatch):
    import singlet_amd as sa
    from singlet_amd import api, context

    def no_device(*a, **k):
        raise AssertionError("a refusal must come before the first upload")
    monkeypatch.setattr(context.Context, "__init__", no_device)
    monkeypatch.setattr(api, "c_moran", no_device)
    monkeypatch.setattr(api, "c_moran_embedding", no_device)
    monkeypatch.setattr(api, "spatial_graph", no_device)
    n, m = 30, 7
    rng = np.random.default_rng(0)
    A = sa.as_dgCMatrix(sparse.csc_matrix(rng.poisson(0.5, (m, n)).astype(np.float64)))
    Gx, Gi, Gp = mo.grid_graph(6, 5)
    G = sa.dgCMatrix(Gx, Gi, Gp, (n, n))
    xy = rng.random((n, 2))
    f = sa.find_spatially_variable_features
    for kw, msg in ((dict(), "exactly one"), (dict(graph=G, coords=xy, max_dist=0.3), "exactly one"),
                    (dict(graph=G, max_dist=0.3), "max_dist belongs"), (dict(coords=xy), "positive max_dist"),
                    (dict(coords=xy, max_dist=-1.0), "positive max_dist"), (dict(coords=xy[:-1], max_dist=0.3), "n x 2"),
                    (dict(coords=xy[:, :1], max_dist=0.3), "n x 2"),
                    (dict(graph=sa.dgCMatrix(Gx[:0], Gi[:0], np.zeros(n, dtype=np.int32), (n - 1, n - 1))), "29 cells, the data 30"),
                    (dict(graph=sa.dgCMatrix(Gx[:0], Gi[:0], np.zeros(n + 1, dtype=np.int32), (n + 2, n))), "square"),
                    (dict(graph=G, variance="bootstrap"), "variance"), (dict(graph=G, alternative="both"), "alternative"),
                    (dict(graph=G, nfeatures=0), "nfeatures"), (dict(graph=G, nfeatures=2.5), "nfeatures"),
                    (dict(graph=G, features=[0, 7]), "outside"), (dict(graph=G, features=[1, 1]), "twice"),
                    (dict(graph=G, features=[[1]]), "one-dimensional")):
        with pytest.raises(ValueError, match=msg):
            f(A, **kw)
    with pytest.raises(ValueError, match="at least 4"):
        f(sa.as_dgCMatrix(sparse.csc_matrix(np.ones((2, 3)))), graph=sa.dgCMatrix(np.ones(1), np.zeros(1, dtype=np.int32), np.array([0, 1, 1, 1], dtype=np.int32), (3, 3)))
    h = rng.random((3, n))
    for args, kw, msg in (((h[:, :-1], G), {}, "one column per cell"), ((h, G), dict(variance="x"), "variance"),
                          ((h, G), dict(alternative="x"), "alternative"), ((h[0], G), {}, "k x n")):
        with pytest.raises(ValueError, match=msg):
            sa.moran_factors(*args, **kw)


# --------------------------------------------------------------------------------------------- the planted fixture
def planted_tables():
    """(fixture, restated moments, restated statistics) of the planted tissue, computed once."""
    if "planted" not in _CACHE:
        D, (Gx, Gi, Gp), which = mo.planted_tissue()
        n = D.shape[1]
        S0, S1, S2, t = mo.graph_moments(Gx, Gi, Gp, n)
        mom = np.zeros((6, D.shape[0]))
        for g in range(D.shape[0]):
            cells = np.nonzero(D[g])[0]
            m, M2, M4, T, c = mo.gene_moments(D[g][cells], cells, n, t)
            mom[:, g] = (m, M2, M4, T, mo.cross_term(D[g][cells], cells, Gx, Gi, Gp, n), c)
        _CACHE["planted"] = (D, (Gx, Gi, Gp), which, (S0, S1, S2), mom, mo.stats(n, S0, S1, S2, mom))
    return _CACHE["planted"]


def planted_claims(st, which, m):
    """The claims of examples/spatial_variable_features.py on a table of statistics."""
    order = mo.rank(st["p"], st["I"], np.arange(m))
    shuffled = np.setdiff1d(np.arange(m), which)
    assert set(order[:which.shape[0]].tolist()) == set(which.tolist())                      # every planted gene above every shuffled one
    assert np.all(st["I"][which] > 0.3)
    assert np.all(np.abs(st["I"][shuffled] - st["EI"][shuffled]) < 4.0 * st["sd"][shuffled])


def test_planted_fixture_meets_the_claims_on_the_restatement_alone():
    D, _, which, _, _, st = planted_tables()
    assert D.shape == (300, 1600) and which.shape == (10,)
    planted_claims(st, which, D.shape[0])
