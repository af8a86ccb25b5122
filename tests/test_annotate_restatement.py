"""The restatement of the factor annotation (annotate_restatement.py) against independent yardsticks -- long-double sums and
np.linalg.lstsq on the explicit one-hot design --, the host logic of the library (singlet_amd/csrc/annotate_host.h) compiled
alone under the address and undefined-behaviour sanitizers and compared with the scipy restatement over a fixed grid, the
Python mirror's column checks and filters, and the host-side wiring (header, bindings, Context, Makefile).

THE TOLERANCES OF THE HOST COMPARISON were measured on the CPU, not chosen: the worst relative difference |lib - scipy| /
|scipy| over the grid of tests/annotate_host_main.cpp and tests/annotate_cases.py for each output, times 16 to cover other
libm builds (lods, a difference of logarithms that crosses zero, is measured against max(|scipy|, 1)).  Measured -> used:
    digamma           4.3e-13 -> 6.8e-12     (the grid point 1.46 next to the root at 1.4616, where psi is 1.6e-3)
    trigamma          2.3e-16 -> 3.7e-15
    trigamma_inverse  3.1e-15 -> 5.0e-14
    t_sf              1.6e-12 -> 2.6e-11     (P(T > t) down to 1.3e-300, at t = 37.04 and df = +Inf; the worst point is t = 3.5 at
                                              df = 5e4, where the continued fraction serves and its denominators cancel like df / t^2;
                                              from df = 1e5 on, up to the grid's 1e9, the large-df form stays below 3e-13)
    t_isf             2.5e-12 -> 4.0e-11     (as a round trip: scipy's sf of the library's quantile against p, down to p = 1e-300
                                              for df >= 30; scipy's own isf and sf give 1e100 and 0 for df = 1, p = 1e-200, where
                                              the quantile is 3.2e199: not a yardstick there, and left out of the grid)
    coefficients, stdev_unscaled, Amean, sigma, df_residual: 0 -> equal bits (IEEE operations in one order on both sides)
    s2_post           1.1e-15 -> 1.7e-14
    s2_prior, df_prior, df_total (scalars)  1.4e-14 -> 2.2e-13
    t                 5.8e-16 -> 9.3e-15
    p_raw             2.6e-13 -> 4.1e-12     (relative, down to 4.8e-225 in the grid's cases and 1.3e-300 in the function grid)
    p_adj             2.6e-13 -> 4.1e-12
    var_prior         9.2e-12 -> 1.5e-10     (a quotient of two quantiles, squared)
    lods              4.4e-12 -> 7.1e-11"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import special

import annotate_cases as ac
import annotate_restatement as ar
import markers_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgl_group_moments", "sgl_c_group_moments", "sgl_gene_group_moments", "sgl_annotate_hold", "sgl_annotate_stats", "sgl_annotate",
           "sgl_c_annotate", "sgl_annotate_genes")
U = 2.0 ** -53

FUNCTION_TOL = {"digamma": 6.8e-12, "trigamma": 3.7e-15, "trigamma_inverse": 5.0e-14, "t_sf": 2.6e-11, "t_isf": 4.0e-11}
STATS_TOL = {"coefficients": 0.0, "stdev_unscaled": 0.0, "Amean": 0.0, "sigma": 0.0, "s2_post": 1.7e-14, "scalars": 2.2e-13, "t": 9.3e-15,
             "p_raw": 4.1e-12, "p_adj": 4.1e-12, "var_prior": 1.5e-10, "lods": 7.1e-11}
STATS_OUTPUTS = tuple(STATS_TOL)


def rel_diff(a, b, floor=0.0):
    """|a - b| / max(|b|, floor); NaN must meet NaN and an infinity its like."""
    if math.isnan(a) or math.isnan(b):
        assert math.isnan(a) and math.isnan(b), (a, b)
        return 0.0
    if math.isinf(a) or math.isinf(b) or a == b:
        assert a == b, (a, b)
        return 0.0
    return abs(a - b) / max(abs(b), floor)


def reference_vector(st, name):
    """The restatement's output `name` laid out as the library prints it (column-major for the per-(row, group) arrays)."""
    if name == "scalars":
        return np.array([st["df_residual"], st["s2_prior"], st["df_prior"], st["df_total"]], dtype=np.float64)
    a = np.asarray(st[name], dtype=np.float64)
    return a.T.reshape(-1) if a.ndim == 2 else a.reshape(-1)


def worst_differences(got, st):
    """{output: worst relative difference} of the library's vectors `got` against the restatement's dict."""
    out = {}
    for name in STATS_OUTPUTS:
        a, b = np.asarray(got[name], dtype=np.float64).reshape(-1), reference_vector(st, name)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        out[name] = max([rel_diff(float(x), float(y), 1.0 if name == "lods" else 0.0) for x, y in zip(a, b)] or [0.0])
    return out


# ------------------------------------------------------------------------------------------------- the moments, restated
def _embedding(seed, k, n, G):
    rng = np.random.default_rng(seed)
    F = rng.gamma(2.0, 1.0, size=(k, n)) * (rng.random((k, n)) < 0.7)
    labels = rng.integers(-1, G, size=n)
    return F, labels


@pytest.mark.parametrize("k,n,G", [(1, 257, 2), (7, 1000, 5), (65, 700, 3), (12, 600, 200)])
def test_embedding_moments_equal_long_double_sums_within_the_stated_bound(k, n, G):
    F, labels = _embedding(k * 1000 + n + G, k, n, G)
    group_n, sums, rss = ar.group_moments(F, labels, G)
    Fl = F.astype(np.longdouble)
    ref_rss = np.zeros(k, dtype=np.longdouble)
    sq_mean_err = np.zeros(k)
    for g in range(G):
        cells = labels == g
        assert group_n[g] == cells.sum()
        if not cells.any():
            assert (sums[:, g] == 0).all() and not np.signbit(sums[:, g]).any()
            continue
        ref = Fl[:, cells].sum(axis=1)
        bound = group_n[g] * U * np.abs(F[:, cells]).sum(axis=1)
        assert (np.abs(sums[:, g] - ref) <= bound).all()
        d = Fl[:, cells] - (ref / group_n[g])[:, None]
        ref_rss += (d * d).sum(axis=1)
        sq_mean_err += group_n[g] * ((group_n[g] + 1) * U * np.abs(F[:, cells]).mean(axis=1)) ** 2
    N = int(group_n.sum())
    bound = (N + 3) * U * ref_rss.astype(np.float64) + 2 * np.sqrt(ref_rss.astype(np.float64)) * np.sqrt(sq_mean_err)
    assert (np.abs(rss - ref_rss) <= bound).all(), (np.abs(rss - ref_rss).max(), bound.min())


def _gene_case(seed, n, density, G):
    rng = np.random.default_rng(seed)
    cells = np.sort(rng.choice(n, size=int(round(density * n)), replace=False)).astype(np.int64)
    x = np.round(rng.normal(1.0, 2.0, size=cells.shape[0]), 2)
    x[rng.random(x.shape[0]) < 0.1] = 0.0          # stored zeros of both signs
    x[rng.random(x.shape[0]) < 0.05] = -0.0
    labels = rng.integers(-1, G, size=n)
    return x, cells, labels


@pytest.mark.parametrize("n,density,G", [(300, 0.3, 2), (9000, 0.95, 5), (2000, 0.5, 1)])
def test_gene_moments_equal_long_double_sums_and_skipping_empty_blocks_changes_no_bit(n, density, G):
    x, cells, labels = _gene_case(n + G, n, density, G)
    group_n, N = mr.group_counts(labels, G)
    _, nz = mr.entry_counts(x, cells, labels, G)
    sums = mr.group_sums(x, cells, labels, G, 0)
    rss = ar.gene_rss(x, cells, labels, G, group_n, nz, sums)
    assert rss == ar.gene_rss(x, cells, labels, G, group_n, nz, sums, skip_empty_blocks=True)
    assert np.array_equal(sums, mr.group_sums(x, cells, labels, G, 0, skip_empty_blocks=True))
    dense = np.zeros(n, dtype=np.longdouble)
    dense[cells] = x
    ref, sq_mean_err = np.longdouble(0), 0.0
    for c in range(G):
        v = dense[labels == c]
        if v.size:
            d = v - v.sum() / v.size
            ref += (d * d).sum()
            sq_mean_err += v.size * ((v.size + 1) * U * float(np.abs(v).mean())) ** 2
    segments = -(-x.shape[0] // ar.SEG)
    bound = (ar.SEG // ar.BLOCK + 7 + segments + 2 + G + 2) * U * float(ref) + 2 * math.sqrt(float(ref)) * math.sqrt(sq_mean_err)
    assert abs(rss - ref) <= bound, (rss, ref, bound)


@pytest.mark.parametrize("center", [True, False])
def test_coefficients_and_sigma_equal_least_squares_on_the_one_hot_design(center):
    k, n, G = 9, 700, 4
    F, labels = _embedding(77, k, n, G)
    labels[labels == 2] = 1                                   # an empty group
    group_n, sums, rss = ar.group_moments(F, labels, G)
    st = ar.annotate_stats(group_n, sums, rss, center=center)
    inc = labels >= 0
    live = np.nonzero(group_n > 0)[0]
    X = (labels[inc, None] == live[None, :]).astype(np.float64)      # the means model ~ 0 + column of the included cells
    Y = F[:, inc].T
    if center:
        Y = Y - Y.mean(axis=0, keepdims=True)
    beta, res, rank, _ = np.linalg.lstsq(X, Y, rcond=None)
    assert rank == live.shape[0] and st["df_residual"] == inc.sum() - rank
    # The header's bound is that of the restated sums alone; the yardstick has an error of its own (lstsq solves through an
    # SVD, of the order of cond(X) n u max|F| with cond(X) = sqrt(largest / smallest group) < 8 here), so the comparison
    # allows both: 64 n u max|F|, four orders below what a wrong formula (a centring left out, n for n - 1) would show.
    scale = np.abs(F).max()
    assert np.abs(st["coefficients"][:, live] - beta.T).max() <= 64 * n * U * scale
    assert np.isnan(st["coefficients"][:, 2]).all() and np.isnan(st["t"][:, 2]).all() and np.isnan(st["p_adj"][:, 2]).all()
    sigma = np.sqrt(((Y - X @ beta) ** 2).sum(axis=0) / st["df_residual"])
    assert np.abs(st["sigma"] - sigma).max() <= 64 * n * U * sigma.max()
    assert np.array_equal(st["stdev_unscaled"][live], 1.0 / np.sqrt(group_n[live].astype(np.float64)))


def test_planted_pairs_are_exactly_what_the_restated_table_keeps():
    import planted_annotation as pa
    F, labels, pairs = pa.planted()
    st = ar.annotate_stats(*ar.group_moments(F, labels, pa.G))
    rows = ar.model_results(st)
    strong = {(g, f) for g, f, fc, p in rows if p < 1e-6}
    assert strong == set(pairs), (strong, pairs)


# --------------------------------------------------------------------------------------------- the host logic, sanitized
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/annotate_host_main.cpp compiled with a host compiler and both sanitizers into a program of its own."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("annotate_host") / "annotate_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "annotate_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_special_functions_agree_with_scipy_over_the_grid(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.strip().endswith("annotate_host: ok"), r.stdout[-500:]
    worst = dict.fromkeys(FUNCTION_TOL, 0.0)
    seen = dict.fromkeys(FUNCTION_TOL, 0)
    smallest_tail = 1.0
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] not in FUNCTION_TOL:
            continue
        v = [float(q) for q in w[1:]]
        if w[0] == "digamma":
            d = rel_diff(v[1], float(special.digamma(v[0])))
        elif w[0] == "trigamma":
            d = rel_diff(v[1], float(special.polygamma(1, v[0])))
        elif w[0] == "trigamma_inverse":
            d = rel_diff(v[1], ar.trigamma_inverse(v[0]))
        elif w[0] == "t_sf":
            ref = float(ar.t_sf(v[0], v[1]))
            d = rel_diff(v[2], ref)
            if ref > 0:
                smallest_tail = min(smallest_tail, ref)
        else:   # t_isf: the round trip through scipy's survival function
            d = rel_diff(float(ar.t_sf(v[2], v[1])), v[0])
        worst[w[0]] = max(worst[w[0]], d)
        seen[w[0]] += 1
    print("worst relative differences:", worst, "smallest tail compared:", smallest_tail)
    assert min(seen.values()) >= 15 and 1e-300 <= smallest_tail < 1e-299      # p holds its tolerance relatively down to 1e-300
    for name, tol in FUNCTION_TOL.items():
        assert worst[name] <= tol, (name, worst[name], tol)


def test_statistics_agree_with_the_scipy_restatement_over_the_grid(host_program, tmp_path):
    cases = ac.stats_cases()
    assert {c["rows"] for c in cases} >= {1, 2, 15, 3000}
    path = str(tmp_path / "cases.txt")
    ac.write_cases(path, cases)
    r = subprocess.run([host_program, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert ("cases %d" % len(cases)) in r.stdout
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if len(w) == 4:
            got.setdefault(int(w[0]), {}).setdefault(w[1], []).append(float(w[3]))
    worst = dict.fromkeys(STATS_OUTPUTS, 0.0)
    df_seen, prior_seen, smallest_p = set(), set(), 1.0
    for ci, c in enumerate(cases):
        st = ar.annotate_stats(c["group_n"], c["sum"], c["rss"], c["center"], c["scale"], c["proportion"], c["tail"])
        for name, d in worst_differences(got[ci], st).items():
            worst[name] = max(worst[name], d)
        df_seen.add(st["df_residual"])
        prior_seen.add("nan" if math.isnan(st["df_prior"]) else "inf" if math.isinf(st["df_prior"]) else "zero" if st["df_prior"] == 0 else "finite")
        if not np.isnan(st["p_raw"]).all():
            smallest_p = min(smallest_p, float(np.nanmin(st["p_raw"])))
    print("worst relative differences:", worst, "smallest p:", smallest_p)
    assert {0.0, 1.0, 1e6} <= df_seen and prior_seen == {"nan", "inf", "zero", "finite"} and smallest_p < 1e-200
    for name, tol in STATS_TOL.items():
        assert worst[name] <= tol, (name, worst[name], tol)


# ------------------------------------------------------------------------------------------------------ the Python mirror
def _meta():
    n = 12
    return {
        "type": np.array(["a", "b", None, "a", "c", "b", "a", "c", "b", "a", "c", "b"], dtype=object),   # an NA level
        "batch": np.array([2, 2, 5, 5, 9, 9, 2, 5, 9, 2, 5, 9]),                                           # integer-coded
        "one": np.array(["x"] * n),                                                                        # one level
        "score": np.linspace(0.0, 1.0, n),                                                                 # not a factor
        "many": np.arange(n),                                                                              # n levels
    }


def test_check_columns_keeps_factor_columns_and_reports_only_when_asked(sa, capsys):
    meta = _meta()
    assert sa.check_columns(meta) == ["type", "batch", "many"]
    assert capsys.readouterr().out == ""                                   # columns = None: silent (R/checkColumns.R:10)
    assert sa.check_columns(meta, ["type", "one", "score", "absent"]) == ["type"]
    out = capsys.readouterr().out
    assert "Some columns are not factors, or have only one level, or have more than max.levels levels." in out
    assert "Skipping `one`, `score`, `absent`." in out
    assert sa.check_columns(meta, max_levels=11) == ["type", "batch"]       # 12 levels > 11
    wide = {"c201": np.arange(402) % 201, "c200": np.arange(402) % 200}
    assert sa.check_columns(wide) == ["c200"]                               # 201 levels are too many at the default 200


def test_get_designs_codes_levels_in_sorted_order_and_missing_values_as_minus_one(sa):
    d = sa.get_designs(_meta(), ["type", "batch"])
    labels, levels = d["type"]
    assert levels == ["a", "b", "c"] and labels.dtype == np.int32
    assert labels.tolist() == [0, 1, -1, 0, 2, 1, 0, 2, 1, 0, 2, 1]
    labels, levels = d["batch"]
    assert levels == [2, 5, 9] and labels.tolist() == [0, 0, 1, 1, 2, 2, 0, 1, 2, 0, 1, 2]


def test_pandas_metadata_is_read_like_a_dict(sa):
    pd = pytest.importorskip("pandas")
    df = pd.DataFrame({"type": pd.Categorical(["b", "a", None, "b"], categories=["b", "a", "z"]), "x": [0.5, 1.5, 2.5, 3.5]})
    assert sa.check_columns(df) == ["type"]
    labels, levels = sa.get_designs(df)["type"]
    assert levels == ["b", "a", "z"] and labels.tolist() == [0, 1, -1, 0]   # the categories' order, an unused level kept


def _fit_from_moments(sa, seed=5):
    import planted_annotation as pa
    F, labels, _ = pa.planted()
    group_n, sums, rss = ar.group_moments(F, labels, pa.G)
    fit = sa.annotate_stats(group_n, sums, rss, tail="std")   # the library's host code: no device involved
    fit["p_value"] = fit.pop("p_raw")
    fit["_p_adj_std"] = fit.pop("p_adj")                      # as get_model_fit leaves it: the two-sided table is not formed twice
    return fit, (group_n, sums, rss)


@pytest.mark.parametrize("tail", ["pos", "neg", "std"])
@pytest.mark.parametrize("noneg", [True, False])
def test_get_model_results_filters_as_the_reference_does(sa, tail, noneg):
    fit, moments = _fit_from_moments(sa)
    st = ar.annotate_stats(*moments, tail=tail)
    want = ar.model_results(st, noneg=noneg)
    got = sa.get_model_results(fit, noneg=noneg, tail=tail, names=(["g0", "g1", "g2", "g3"], None))
    assert got["group"].tolist() == [w[0] for w in want] and got["factor"].tolist() == [w[1] for w in want]
    assert got["group_names"] == ["g%d" % w[0] for w in want]
    for a, w in zip(got["fc"], want):
        assert rel_diff(float(a), float(w[2]), 1.0) <= STATS_TOL["lods"]
    for a, w in zip(got["p"], want):
        assert rel_diff(float(a), float(w[3])) <= STATS_TOL["p_adj"]
    if noneg:
        assert (got["fc"] > 0).all()
    else:
        assert got["fc"].shape[0] == st["lods"].size


def test_an_invalid_tail_raises_with_the_reference_message(sa):
    fit, _ = _fit_from_moments(sa)
    with pytest.raises(ValueError, match="Invalid tail selection. Choose 'pos','neg', or 'std'"):
        sa.get_model_results(fit, tail="both")
    with pytest.raises(ValueError, match="Invalid tail selection"):
        sa.AnnotateNMF({"h": np.ones((2, 4))}, {"c": [0, 1, 0, 1]}, tail="two")


def test_the_library_statistics_equal_the_restatement_through_the_binding(sa):
    for c in ac.stats_cases():
        got = sa.annotate_stats(c["group_n"], c["sum"], c["rss"], c["center"], c["scale"], c["proportion"], c["tail"])
        got["scalars"] = [got["df_residual"], got["s2_prior"], got["df_prior"], got["df_total"]]
        vec = {k: (np.asarray(got[k]).T.reshape(-1) if np.asarray(got[k]).ndim == 2 else np.asarray(got[k])) for k in STATS_OUTPUTS}
        st = ar.annotate_stats(c["group_n"], c["sum"], c["rss"], c["center"], c["scale"], c["proportion"], c["tail"])
        for name, d in worst_differences(vec, st).items():
            assert d <= STATS_TOL[name], (c["name"], name, d)


def test_stats_refusals_name_the_argument(sa):
    from singlet_amd import SingletHipError
    gn, s, rss = np.array([3, 4]), np.ones((2, 2)), np.ones(2)
    with pytest.raises(SingletHipError, match=r"proportion = 1.5 is outside \(0, 1\)"):
        sa.annotate_stats(gn, s, rss, proportion=1.5)
    with pytest.raises(SingletHipError, match=r"group_n\[1\] = -4 is negative"):
        sa.annotate_stats(np.array([3, -4]), s, rss)
    with pytest.raises(ValueError, match="rows x G"):
        sa.annotate_stats(gn, np.ones((2, 3)), rss)
    with pytest.raises(SingletHipError, match=r"n_groups = 1025"):
        sa.annotate_stats(np.ones(1025, dtype=np.int64), np.ones((2, 1025)), rss)


# --------------------------------------------------------------------------------------------------------------- the wiring
def test_the_entries_are_declared_bound_and_exported(sa):
    from singlet_amd import _lib
    f64p, i32p, i64p = _lib.f64p, _lib.i32p, _lib.i64p
    i32, i64, ctx, outs = C.c_int32, C.c_int64, C.c_void_p, [_lib.f64p] * 11
    assert _lib.SIGNATURES["sgl_group_moments"] == (C.c_int, [ctx, f64p, i32, i64, i32p, i32, i64p, f64p, f64p])
    assert _lib.SIGNATURES["sgl_c_group_moments"] == (C.c_int, [f64p, i32, i64, i32p, i32, i64p, f64p, f64p])
    assert _lib.SIGNATURES["sgl_gene_group_moments"] == (C.c_int, [ctx, i32p, i32, i64p, i64p, f64p, f64p])
    assert _lib.SIGNATURES["sgl_annotate_hold"] == (C.c_int, [ctx, f64p, i32, i64])
    assert _lib.SIGNATURES["sgl_annotate_stats"] == (C.c_int, [i64, i32, i64p, f64p, f64p, C.c_int, C.c_int, C.c_double, C.c_int] + outs)
    assert _lib.SIGNATURES["sgl_annotate"] == (C.c_int, [ctx, f64p, i32, i64, i32p, i32, C.c_int, C.c_int, C.c_double, C.c_int, i64p, f64p, f64p] + outs)
    assert _lib.SIGNATURES["sgl_c_annotate"] == (C.c_int, [f64p, i32, i64, i32p, i32, C.c_int, C.c_int, C.c_double, C.c_int, i64p, f64p, f64p] + outs)
    assert _lib.SIGNATURES["sgl_annotate_genes"] == (C.c_int, [ctx, i32p, i32, C.c_int, C.c_int, C.c_double, C.c_int, i64p, i64p, f64p, f64p] + outs)
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    assert "Factor annotation" in header and "Smyth (2004" in header and "robust = TRUE" in header
    for name in ENTRIES:
        m = re.search(r"SGL_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    for name in ("group_moments", "gene_group_moments", "annotate", "annotate_genes", "hold_embedding"):
        assert callable(getattr(sa.Context, name)), name
    for name in ("check_columns", "get_designs", "get_model_fit", "get_model_results", "AnnotateNMF", "annotate_stats", "c_annotate", "c_group_moments"):
        assert callable(getattr(sa, name)), name
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "annotate_host.h")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower()          # the host header makes no HIP call
    assert int(re.search(r"#define ANNOTATE_SEG (\d+)", host).group(1)) == ar.SEG == mr.SEG
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^kernels_annotate\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M) and " kernels_annotate.o" in mk


def test_the_refusal_order_of_the_arguments():
    lab = np.array([0, -1, 2, 3, -2])
    assert ar.check_args(None, 5, 3, 1) == ("null", -1, 0)
    assert ar.check_args(lab, 5, 0, 1)[0] == "groups" and ar.check_args(lab, 5, 1025, 1)[0] == "groups"
    assert ar.check_args(lab, 5, 3, 0)[0] == "k" and ar.check_args(lab, 5, 3, 1025)[0] == "k"
    assert ar.check_args(lab, 5, 3, 1) == ("label", 3, 3) and ar.check_args(lab, 5, 4, 1) == ("label", 4, -2)
    assert ar.check_args(lab, 4, 4, 1) is None
