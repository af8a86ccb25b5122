"""The numpy restatement of sgl_variable_features (variable_features_restatement.py) against hand-worked cases, the
conditions the device tests rely on (found here, where no device is needed), and the host-side wiring: RunNMF's argument
refusals, the Makefile's object list and flag, the header's six entries and their bindings.

The worked 3 x 4 matrix (genes x cells), n = 4:

    g0 = [1, 0, 3, 0]   stored 1 and 3: S = 4, mean = 1, c = 2
                        variance about 1: (1 - 1)^2 + (3 - 1)^2 = 4, plus the 2 zeros at (0 - 1)^2 = 2: 6 / 3 = 2
                        standardised with sd = 2, vmax = 0.75: z = 0 and 1 -> 0.75 (the clip changes exactly this entry):
                        0 + 0.5625, plus 2 zeros at z0 = -0.5, not clipped: 2 * 0.25: 1.0625 / 3
                        (unclipped it would be 1.5 / 3)
    g1 = [2, 2, 2, 2]   constant: mean 2, variance 0; sd = 0 gives +0.0
    g2 = [0, 0, 0, 0]   nothing stored: mean 0, count 0, variance 0; with sd = 1: 0
"""
import os
import re

import numpy as np
import pytest

import variable_features_restatement as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgl_variable_features", "sgl_c_variable_features", "sgl_op_gene_mean", "sgl_op_gene_var", "sgl_op_gene_var_std",
           "sgl_op_loess_direct")
COMPOSITE_CASES = vr.COMPOSITE_CASES


def _worked():
    D = np.array([[1.0, 0, 3, 0], [2, 2, 2, 2], [0, 0, 0, 0]])
    x, i, p = vr.csc_of_dense(D)
    return vr.gene_side(x, i, p, 3) + (4,)


def test_the_worked_matrix_in_every_arithmetic():
    x, p, n = _worked()
    mean, count = vr.mean_f64(x, p, n)
    assert mean.tolist() == [1.0, 2.0, 0.0] and count.tolist() == [2, 4, 0]
    assert vr.mean_exact(x, p, n).tolist() == [1.0, 2.0, 0.0]
    assert vr.mean_ld(x, p, n).astype(float).tolist() == [1.0, 2.0, 0.0]
    for fn in (vr.var_f64, vr.var_exact, vr.var_ld):
        assert np.asarray(fn(x, p, n, mean), dtype=float).tolist() == [2.0, 0.0, 0.0], fn.__name__
    sd = np.array([2.0, 0.0, 1.0])
    for fn in (vr.var_std_f64, vr.var_std_exact):
        assert fn(x, p, n, mean, sd, 0.75).tolist() == [1.0625 / 3, 0.0, 0.0], fn.__name__
        assert fn(x, p, n, mean, sd, 1.0).tolist() == [1.5 / 3, 0.0, 0.0], fn.__name__   # z = 1 is not above vmax = 1
    assert abs(float(vr.var_std_ld(x, p, n, mean, sd, 0.75)[0]) - 1.0625 / 3) < 1e-16
    assert not np.signbit(vr.var_std_f64(x, p, n, mean, sd, 0.75)).any()


def test_an_explicit_zero_counts_as_stored_and_changes_no_value():
    x, i, p = vr.csc_of_triplets([0, 0, 1], [1, 2, 0], [0.0, 4.0, 0.0], 2, 4)
    gx, gp = vr.gene_side(x, i, p, 2)
    mean, count = vr.mean_f64(gx, gp, 4)
    assert count.tolist() == [2, 1] and mean.tolist() == [1.0, 0.0]
    # variance of [0, 0, 4, 0] about 1: 9 + 3 = 12, / 3, whether the zero is stored or not
    assert vr.var_f64(gx, gp, 4, mean).tolist() == [4.0, 0.0]
    assert vr.var_exact(gx, gp, 4, mean).tolist() == [4.0, 0.0]


def test_stated_order_equals_exact_arithmetic_where_every_sum_is_exact():
    for n in (64, 128):
        x, i, p, nrow, names = vr.exact_gate_matrix(n)
        gx, gp = vr.gene_side(x, i, p, nrow)
        mean, count = vr.mean_f64(gx, gp, n)
        assert np.array_equal(mean, vr.mean_exact(gx, gp, n))
        assert count[names.index("explicit zero")] == 1 and mean[names.index("explicit zero")] == 0.0
        assert count[names.index("c=%d" % n)] == n and count[names.index("c=0")] == 0
        assert np.array_equal(vr.var_f64(gx, gp, n, mean), vr.var_exact(gx, gp, n, mean))
        sd = 2.0 ** ((np.arange(nrow) % 3) - 1.0)
        sd[names.index("c=1")] = 0.0
        assert np.array_equal(vr.var_std_f64(gx, gp, n, mean, sd, 2.0), vr.var_std_exact(gx, gp, n, mean, sd, 2.0))
        g = names.index("clip")
        z = (gx[gp[g]:gp[g + 1]] - mean[g]) / sd[g]
        assert (z > 2.0).any() and (z <= 2.0).any(), "the clip binds on some entries of its gene and not on others"


def test_segments_are_added_in_order():
    t = np.arange(1.0, 2 * vr.SEG + 2)
    assert vr.gene_sum(t) == t.sum()          # integers: exact in any order
    rng = np.random.default_rng(0)
    t = rng.random(2 * vr.SEG + 1)
    want = (vr.lane_sum(t[:vr.SEG])[0] + vr.lane_sum(t[vr.SEG:2 * vr.SEG])[0]) + t[2 * vr.SEG]
    assert vr.gene_sum(t) == want
    assert vr.gene_sum(t[:0]) == 0.0 and not np.signbit(vr.gene_sum(t[:0]))
    # lanes: 65 terms -- lane 0 holds t0 + t64, then the butterfly
    t = rng.random(65)
    v = t[:64].copy()
    v[0] = v[0] + t[64]
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ off]
    assert vr.lane_sum(t)[0] == v[0]
    src = open(os.path.join(ROOT, "singlet_amd", "csrc", "kernels_hvg.hip")).read()
    assert re.search(r"#define HVG_SEG %d\b" % vr.SEG, src), "the kernel's segment length is the restated one"


# -------------------------------------------------------------------------------------------------------------- trend --
def test_window_ties_go_to_the_lowest_start_and_the_bandwidth_is_the_farthest_member():
    x = np.array([0.0, 1, 2, 3, 4])
    assert vr.loess_window(x, 2, 3) == (1, 1.0)      # starts 0, 1, 2 reach 2, 1, 2
    assert vr.loess_window(x, 0, 3) == (0, 2.0) and vr.loess_window(x, 4, 3) == (2, 2.0)
    assert vr.loess_window(np.array([0.0, 1, 2, 3]), 1, 2) == (0, 1.0)   # starts 0 and 1 both reach 1: the lowest
    assert vr.loess_window(x, 3, 5) == (0, 3.0) and vr.loess_window(x, 3, 1) == (3, 0.0)


def test_hmax_zero_weighs_every_member_one_and_fits_a_constant():
    x = np.array([0.0, 0, 0, 1, 2, 3])
    y = np.array([1.0, 2, 6, 0, 0, 0])
    for fn in (vr.loess_f64, vr.loess_ld):
        assert float(fn(x, y, 3)[0]) == 3.0          # window [0, 0, 0]: the mean of 1, 2, 6
    assert vr.loess_f64(x, y, 1).tolist() == y.tolist()


def test_the_degree_follows_the_distinct_values_of_positive_weight():
    # window [0, 1] of point 1 (tie to the lowest start): hmax = 1, the member at 0 weighs (1 - 1)^3 = 0 -> a constant: y[1]
    x, y = np.array([0.0, 1, 2, 3]), np.array([5.0, 7, 1, 2])
    assert vr.loess_f64(x, y, 2)[1] == 7.0
    # [0, 0, 1, 1, 3] around x = 1 with q = 5: hmax = 2, the member at 3 weighs nothing, two values carry a straight line
    x, y = np.array([0.0, 0, 1, 1, 3]), np.array([1.0, 3, 4, 6, 100])
    u = x - 1.0
    w = (1 - (np.abs(u) / 2.0) ** 3) ** 3
    assert w[4] == 0.0 and vr.trend_windows(x, 5)[2] == (3, 2)
    line = np.polyfit(u[:4], y[:4], 1, w=np.sqrt(w[:4]))[1]
    for fn in (vr.loess_f64, vr.loess_ld):
        assert abs(float(fn(x, y, 5)[2]) - line) < 1e-13
    assert abs(line - 5.0) < 1e-13     # the line through (-1, 2) and (0, 5), the weighted means of the two values
    # three values of positive weight: the weighted parabola, against numpy's least squares
    x = np.array([0.0, 0.5, 0.75, 1.5, 2.0, 4.0])
    y = np.array([1.0, 0.2, 3.0, -1.0, 2.0, 8.0])
    s0, hmax = vr.loess_window(x, 2, 5)
    u = x[s0:s0 + 5] - x[2]
    w = (1 - (np.abs(u) / hmax) ** 3) ** 3
    keep = w > 0
    para = np.polyfit(u[keep], y[s0:s0 + 5][keep], 2, w=np.sqrt(w[keep]))[2]
    for fn in (vr.loess_f64, vr.loess_ld):
        assert abs(float(fn(x, y, 5)[2]) - para) < 1e-12
    # a straight line is reproduced at every degree above 0
    x = np.sort(np.random.default_rng(2).uniform(0, 1, 40))
    assert np.max(np.abs(vr.loess_f64(x, 2 * x + 1, 12) - (2 * x + 1))) < 1e-12


@pytest.mark.parametrize("span", vr.TREND_SPANS)
@pytest.mark.parametrize("m", vr.TREND_SIZES)
def test_trend_inputs_meet_their_conditions(m, span):
    """The inputs of the device's trend test: the runs of equal x give windows of one value and of exactly two, every
    degree occurs, and the float64 restatement alone stays within a quarter of the tolerance the device gets (16 times the
    larger of its deviations from the longdouble trend in the stated lanes and in numpy's pairwise order)."""
    x, y = vr.trend_inputs(m)
    q = vr.window_length(m, span)
    assert 1 <= q <= m and np.all(np.diff(x) >= 0)
    if m >= 3:
        assert np.sum(x == x[0]) == m // 3
    tol, ld, dev_lanes, dev_pair = vr.trend_tolerance(x, y, q)
    print("trend-figure m=%d span=%g q=%d: float64 - longdouble: lanes %.3g, pairwise %.3g; tolerance %.3g" % (m, span, q, dev_lanes, dev_pair, tol))
    assert np.all(np.isfinite(ld.astype(float)))
    assert dev_lanes <= tol / 4
    if m >= 50 and span == 0.3:
        wins = vr.trend_windows(x, q)
        assert any(d == 1 for d, _ in wins), "a window that is one value"
        assert any(d == 2 for d, _ in wins), "a window of exactly two values"
        assert {deg for _, deg in wins} == {1, 2, 3}, "degrees 0, 1 and 2 all occur"


# ---------------------------------------------------------------------------------------------------------- composite --
def test_the_ranking_breaks_ties_by_the_lower_gene_index():
    D = vr.count_matrix(40, 128, 3)
    D[31] = D[9]          # two identical gene rows
    x, i, p = vr.csc_of_dense(D)
    gx, gp = vr.gene_side(x, i, p, 40)
    r = vr.variable_features(gx, gp, 128, 40)
    std, rank = r["variance_standardized"], r["rank"].tolist()
    assert std[9] == std[31] and rank.index(9) + 1 == rank.index(31)
    assert sorted(rank) == list(range(40)) and np.all(np.diff(std[r["rank"]]) <= 0)
    assert r["variance_expected"][3] == 0.0 and std[3] == 0.0       # an all-zero gene: constant, sd = 0
    assert r["variance"][38] == 0.0 and std[38] == 0.0              # a constant gene of 2s
    given = vr.variable_features(gx, gp, 128, 5, expected_var=np.full(40, 4.0))
    assert np.array_equal(given["variance_expected"], np.full(40, 4.0)) and given["trend"] is None and given["features"].shape == (5,)


@pytest.mark.parametrize("m,n,seed,nfeatures", COMPOSITE_CASES)
def test_composite_cases_have_no_near_tie_among_the_ranked(m, n, seed, nfeatures):
    """The condition of the device's composite test: every adjacent pair among the first nfeatures + 1 ranked standardised
    variances differs by more than 1e-9 relative, so a device within its bounds ranks them alike."""
    x, i, p = vr.csc_of_dense(vr.count_matrix(m, n, seed))
    gx, gp = vr.gene_side(x, i, p, m)
    r = vr.variable_features(gx, gp, n, nfeatures)
    gaps = vr.rank_gaps(r["variance_standardized"], r["rank"], nfeatures)
    print("composite-figure %d x %d seed %d: least relative gap among the first %d: %.3g" % (m, n, seed, nfeatures + 1, gaps.min()))
    assert gaps.min() > 1e-9
    assert (r["variance"] > 0).sum() >= m - 8 and r["variance_standardized"][r["rank"][0]] > 2.0


# -------------------------------------------------------------------------------------------------------------- wiring --
def test_run_nmf_refuses_its_arguments_before_any_upload():
    import singlet_amd as sa
    A = sa.dgCMatrix.from_dense(np.arange(12.0).reshape(3, 4))
    with pytest.raises(ValueError, match="either features or nfeatures"):
        sa.RunNMF(A, k=2, features=[0, 1], nfeatures=2)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="nfeatures must be a whole number"):
            sa.RunNMF(A, k=2, nfeatures=bad)
    with pytest.raises(ValueError, match="pass them as names or indices"):
        sa.RunNMF(A, k=2, features="var.features")
    assert "find_variable_features" in dir(sa)
    with pytest.raises(ValueError, match="one entry per gene"):
        sa.find_variable_features(A, 2, expected_var=np.ones(5))


def test_the_makefile_builds_the_unit_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_hvg.o" in objs
    assert re.search(r"^kernels_hvg\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)


def test_the_header_declares_the_six_entries_and_the_binding_matches():
    from singlet_amd import _lib
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"SGL_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "sgl_abi_version(void);   /* 2:" in header
    assert "NOT R's default loess(surface = \"interpolate\")" in header
