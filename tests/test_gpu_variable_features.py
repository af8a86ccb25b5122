"""Variable features on the device (sgl_variable_features and its four stage operators, kernels_hvg.hip) against the numpy
restatement (variable_features_restatement.py): exact where every sum is exact, bit for bit in the stated order on real
values, within the first-order rounding bound of the longdouble restatement, the trend within a tolerance measured on its
own inputs, the composite's list equal in order, the forms bit-identical, a fit in progress untouched, the refusals, and
RunNMF(nfeatures=)."""
import ctypes as C

import numpy as np
import pytest

import variable_features_restatement as vr

pytestmark = pytest.mark.gpu

U = vr.U
LD = vr.LD
EINVAL, ESTATE = -1, -6


def _dgc(sa, x, i, p, nrow, ncol, names=None):
    return sa.dgCMatrix(x, i, p, (nrow, ncol), (names, None)) if names is not None else sa.dgCMatrix(x, i, p, (nrow, ncol))


def _pow2_sd(nrow, zero_at):
    sd = 2.0 ** ((np.arange(nrow) % 3) - 1.0)
    sd[zero_at] = 0.0
    return sd


# --------------------------------------------------------------------------------------------------------- exact gate --
@pytest.mark.parametrize("n", [64, 128, 1024])
def test_exact_gate_counts_with_a_power_of_two_of_cells(sa, ctx, n):
    """Counts 0..7 and n a power of two: mean = S / n, every x - mu, its square and every partial sum are exact, so the
    three operators equal the exactly rounded restatement with ==, whatever the order.  sd and vmax are powers of two."""
    x, i, p, nrow, names = vr.exact_gate_matrix(n)
    gx, gp = vr.gene_side(x, i, p, nrow)
    ctx.upload(_dgc(sa, x, i, p, nrow, n))
    assert ctx.dims() == (nrow, n, x.shape[0])          # the explicit zeros are stored
    mean, count = ctx.op_gene_mean()
    assert np.array_equal(count, np.diff(gp))
    for c in [q for q in vr.EXACT_COUNTS if q < n] + [n]:
        assert count[names.index("c=%d" % c)] == c
    assert count[names.index("explicit zero")] == 1 and mean[names.index("explicit zero")] == 0.0
    assert np.array_equal(mean, vr.mean_exact(gx, gp, n)) and not np.signbit(mean).any()
    var = ctx.op_gene_var(mean)
    assert np.array_equal(var, vr.var_exact(gx, gp, n, mean))
    assert var[names.index("c=0")] == 0.0 and var[names.index("explicit zero")] == 0.0
    sd = _pow2_sd(nrow, names.index("c=1"))
    g = names.index("clip")
    z = (gx[gp[g]:gp[g + 1]] - mean[g]) / sd[g]
    assert (z > 2.0).any() and (z <= 2.0).any()
    std = ctx.op_gene_var_std(mean, sd, 2.0)
    assert np.array_equal(std, vr.var_std_exact(gx, gp, n, mean, sd, 2.0))
    assert std[names.index("c=1")] == 0.0 and not np.signbit(std).any()
    # not clipped at all: another value, exact as well
    assert np.array_equal(ctx.op_gene_var_std(mean, sd, 1024.0), vr.var_std_exact(gx, gp, n, mean, sd, 1024.0))
    assert np.array_equal(ctx.op_gene_mean()[0], mean)  # two calls, the same bits


def test_exact_gate_genes_around_the_segment_length(sa, ctx):
    """8 genes x (2 segments + 1) cells with c_g = segment - 1, segment, segment + 1 and 2 segments + 1.  The number of cells
    is no power of two: the mean is one division of an exact sum, and the variances are taken about a dyadic mu."""
    x, i, p, nrow, n = vr.segment_matrix()
    gx, gp = vr.gene_side(x, i, p, nrow)
    assert np.diff(gp)[:4].tolist() == [vr.SEG - 1, vr.SEG, vr.SEG + 1, 2 * vr.SEG + 1] and n == 2 * vr.SEG + 1
    ctx.upload(_dgc(sa, x, i, p, nrow, n))
    mean, count = ctx.op_gene_mean()
    assert np.array_equal(count, np.diff(gp)) and np.array_equal(mean, vr.mean_exact(gx, gp, n))
    mu = np.round(mean * 8.0) / 8.0
    assert np.array_equal(ctx.op_gene_var(mu), vr.var_exact(gx, gp, n, mu))
    sd = _pow2_sd(nrow, 5)
    assert np.array_equal(ctx.op_gene_var_std(mu, sd, 2.0), vr.var_std_exact(gx, gp, n, mu, sd, 2.0))


# ------------------------------------------------------------------------------------- stated order, rounding bound --
_REAL = {}


def _real(ctx, shape):
    """LogNormalized synth (means not dyadic), the three operators on it and the float64 / longdouble restatements, once."""
    if shape not in _REAL:
        m, n, inv = shape
        ctx.synth(m, n, inv)
        ctx.log_normalize()
        gx, _, gp = ctx.download(1)     # t(A): one column per gene
        mean, count = ctx.op_gene_mean()
        var = ctx.op_gene_var(mean)
        sd = np.sqrt(var) * 0.75
        sd[1] = 0.0
        vmax = float(np.median((gx[gp[0]:gp[1]] - mean[0]) / sd[0]))   # the clip binds on about half of gene 0's entries
        std = ctx.op_gene_var_std(mean, sd, vmax)
        _REAL[shape] = dict(gx=gx, gp=gp, n=n, mean=mean, count=count, var=var, sd=sd, std=std, vmax=vmax,
                            again=(ctx.op_gene_mean()[0], ctx.op_gene_var(mean), ctx.op_gene_var_std(mean, sd, vmax)))
    return _REAL[shape]


# 20 000 cells at one stored value in two: genes of about 10 000 entries, two segments each
REAL_SHAPES = [(257, 700, 20), (120, 20000, 2)]


@pytest.mark.parametrize("shape", REAL_SHAPES)
def test_real_values_equal_the_stated_order_bit_for_bit(ctx, shape):
    r = _real(ctx, shape)
    gx, gp, n = r["gx"], r["gp"], r["n"]
    if shape[1] > vr.SEG:
        assert np.diff(gp).max() > vr.SEG
    mean, count = vr.mean_f64(gx, gp, n)
    assert np.array_equal(r["count"], count)
    assert np.array_equal(r["mean"], mean)
    assert np.array_equal(r["var"], vr.var_f64(gx, gp, n, r["mean"]))
    z = (gx[gp[0]:gp[1]] - r["mean"][0]) / r["sd"][0]
    assert (z > r["vmax"]).any() and (z <= r["vmax"]).any()
    assert np.array_equal(r["std"], vr.var_std_f64(gx, gp, n, r["mean"], r["sd"], r["vmax"]))
    for got, first in zip(r["again"], (r["mean"], r["var"], r["std"])):
        assert np.array_equal(got, first)


@pytest.mark.parametrize("shape", REAL_SHAPES)
def test_real_values_stay_within_the_first_order_rounding_bound(ctx, shape):
    """Against the longdouble restatement: the mean within (c_g + 2) 2^-53 relative, either variance within
    (3 c_g + 8) 2^-53.  The terms are not negative; each carries at most three roundings before the sum (five units in the
    squared standardised term, which 3 c_g covers from c_g = 1 on) and one per addition; first order, no measured number."""
    r = _real(ctx, shape)
    gx, gp, n, c = r["gx"], r["gp"], r["n"], r["count"].astype(LD)
    for name, got, ld, bound in (("mean", r["mean"], vr.mean_ld(gx, gp, n), (c + 2) * U),
                                 ("var", r["var"], vr.var_ld(gx, gp, n, r["mean"]), (3 * c + 8) * U),
                                 ("std", r["std"], vr.var_std_ld(gx, gp, n, r["mean"], r["sd"], r["vmax"]), (3 * c + 8) * U)):
        err = np.abs(got.astype(LD) - ld)
        with np.errstate(invalid="ignore", divide="ignore"):
            print("hvg-figure %s %r: worst error / bound = %.3g" % (name, shape, float(np.nanmax(err / (bound * np.abs(ld))))))
        assert np.all(err <= bound * np.abs(ld)), name


# -------------------------------------------------------------------------------------------------------------- trend --
@pytest.mark.parametrize("span", vr.TREND_SPANS)
@pytest.mark.parametrize("m", vr.TREND_SIZES)
def test_trend_is_within_sixteen_times_the_float64_restatements_own_deviation(ctx, m, span):
    """Reference: the longdouble restatement.  Tolerance: 16 times the larger of the float64 restatement's largest
    deviations from it on these same inputs, in the stated lanes and in numpy's pairwise order; the factor covers a
    different but equally valid solve of the 3 x 3 system.  Measured (absolute, y of order 1; lanes / pairwise):
    m = 1, 2: 0 / 0; 3: 1.1e-16 / 1.1e-16; 4: 2.2e-16 (span 0.3), 4.4e-13 (span 1: four points, two of weight near zero);
    50: 1.5e-15 / 1.8e-15 (0.3), 1.5e-14 / 3.0e-14 (1); 257: 3.1e-15 / 3.5e-15 (0.3), 1.2e-13 / 1.2e-13 (1); 2000: 3.8e-14 / 3.8e-14 (0.3),
    4.7e-13 / 3.4e-13 (1) -- so the largest tolerance is 7.6e-12.  On the MI355X the device gave the float64 restatement's own bits in all
    fourteen cases."""
    x, y = vr.trend_inputs(m)
    q = vr.window_length(m, span)
    tol, ld, dev_lanes, dev_pair = vr.trend_tolerance(x, y, q)
    got = ctx.op_loess_direct(x, y, q)
    err = float(np.max(np.abs(got.astype(LD) - ld)))
    print("trend-figure m=%d span=%g: device - longdouble %.3g, float64 lanes %.3g, pairwise %.3g, tolerance %.3g; equal bits: %s"
          % (m, span, err, dev_lanes, dev_pair, tol, np.array_equal(got, vr.loess_f64(x, y, q))))
    assert err <= tol
    assert np.array_equal(ctx.op_loess_direct(x, y, q), got)


# ---------------------------------------------------------------------------------------------------------- composite --
_COMP = {}


def _composite(sa, ctx, case):
    if case not in _COMP:
        m, n, seed, nf = case
        D = vr.count_matrix(m, n, seed)
        x, i, p = vr.csc_of_dense(D)
        gx, gp = vr.gene_side(x, i, p, m)
        A = _dgc(sa, x, i, p, m, n, ["g%d" % g for g in range(m)])
        ctx.upload(A)
        _COMP[case] = dict(A=A, csc=(x, i, p), out=ctx.variable_features(nf), ref=vr.variable_features(gx, gp, n, nf), gx=gx, gp=gp)
    return _COMP[case]


def _composed_tolerances(ref):
    """Relative tolerances of the device's info against the float64 restatement, from the stage bounds:
      mean      2 (c + 2) u: both lie within (c + 2) u of the exact mean;
      variance  2 (3 c + 8) u likewise (about each side's own mean: the variance is stationary in mu there);
      fitted    both trends lie within the trend tolerance (16 times the restatement's own deviation, measured on these very
                inputs) of the longdouble trend: twice that, plus 8 u (1 + max |x| + max |y|) for the two log10 each side
                takes with its own library, a unit in the last place apart at most;
      expected  10^fitted: expm1(ln 10 * d_fitted) + 4 u;
      standardised  every term scales with 1 / expected (a clipped term with nothing): the expected's tolerance, plus 2 u
                for the square root, plus 2 (3 c + 8) u."""
    c = ref["count"].astype(np.float64)
    lx, ly, q = ref["trend"]
    d_fit = 2 * vr.trend_tolerance(lx, ly, q)[0] + 8 * U * (1 + np.abs(lx).max() + np.abs(ly).max())
    t_exp = float(np.expm1(np.log(10.0) * d_fit)) + 4 * U
    return {"mean": 2 * (c + 2) * U, "variance": 2 * (3 * c + 8) * U, "variance_expected": t_exp,
            "variance_standardized": t_exp + 2 * U + 2 * (3 * c + 8) * U}


@pytest.mark.parametrize("case", vr.COMPOSITE_CASES)
def test_composite_matches_the_restatement_and_ranks_alike(sa, ctx, case):
    m, n, seed, nf = case
    r = _composite(sa, ctx, case)
    out, ref = r["out"], r["ref"]
    gaps = vr.rank_gaps(ref["variance_standardized"], ref["rank"], nf)
    assert gaps.min() > 1e-9, "the condition of this comparison (tests/test_variable_features_restatement.py finds the seeds)"
    tol = _composed_tolerances(ref)
    assert np.max(tol["variance_standardized"]) < 0.5e-9, "the bounds cannot swap two of the ranked"
    for key, t in tol.items():
        err = np.abs(out[key] - ref[key])
        with np.errstate(invalid="ignore", divide="ignore"):
            print("composite-figure %r %s: worst error / tolerance %.3g" % (case, key, float(np.nanmax(err / (t * np.abs(ref[key]))))))
        assert np.all(err <= t * np.abs(ref[key])), key
    assert out["features"].dtype == np.int32 and out["features"].shape == (nf,)
    assert np.array_equal(out["features"], ref["features"])
    assert out["variance_expected"][3] == 0.0 and out["variance_standardized"][3] == 0.0       # the all-zero gene
    assert out["variance"][m - 2] == 0.0 and out["variance_standardized"][m - 2] == 0.0       # the constant gene


def test_composite_with_expected_variances_given_skips_the_trend(sa, ctx):
    case = vr.COMPOSITE_CASES[0]
    m, n, seed, nf = case
    r = _composite(sa, ctx, case)
    ctx.upload(r["A"])
    ev = np.linspace(0.5, 9.0, m)
    ev[7] = 0.0
    out = ctx.variable_features(nf, expected_var=ev, vmax=5.0)
    assert np.array_equal(out["variance_expected"], ev)
    ref = vr.variable_features(r["gx"], r["gp"], n, nf, vmax=5.0, expected_var=ev)
    # mean, variance and, with sd = sqrt(expected) one square root of the same double, the standardised variance: the stated order
    for key in ("mean", "variance", "variance_standardized"):
        assert np.array_equal(out[key], ref[key]), key
    assert np.array_equal(out["features"], ref["features"]) and out["variance_standardized"][7] == 0.0


def test_nfeatures_at_or_above_nrow_ranks_every_gene_and_a_planted_tie_goes_to_the_lower_index(sa, ctx):
    m, n = 60, 256
    D = vr.count_matrix(m, n, 11)
    D[41] = D[17]                    # two identical gene rows: the one exception to the gap condition
    x, i, p = vr.csc_of_dense(D)
    gx, gp = vr.gene_side(x, i, p, m)
    ctx.upload(_dgc(sa, x, i, p, m, n))
    ref = vr.variable_features(gx, gp, n, m)
    for nf in (m, m + 1, 100000):
        out = ctx.variable_features(nf)
        assert out["features"].shape == (m,) and sorted(out["features"].tolist()) == list(range(m))
    std = out["variance_standardized"]
    assert std[17] == std[41] and std[17] > 0
    order = out["features"].tolist()
    assert order.index(17) + 1 == order.index(41)
    assert np.all(np.diff(std[out["features"]]) <= 0)
    gaps = vr.rank_gaps(ref["variance_standardized"], ref["rank"], m - 4)   # the last three are the constant genes
    assert np.sum(gaps <= 1e-9) == 1 and np.array_equal(out["features"][:m - 3], ref["features"][:m - 3])


@pytest.mark.parametrize("case", vr.COMPOSITE_CASES)
def test_resident_one_shot_and_native_forms_give_the_same_bits(sa, ctx, case):
    m, n, seed, nf = case
    r = _composite(sa, ctx, case)
    x, i, p = r["csc"]
    forms = {"one-shot": sa.find_variable_features(r["A"], nf),
             "native float32, cells x genes": sa.find_variable_features(sa.native((x.astype(np.float32), i, p, (n, m), "csr"), cells_by_genes=True), nf)}
    with sa.Context(0) as c:
        c.upload_dense(vr.count_matrix(m, n, seed))
        forms["after a dense upload"] = c.variable_features(nf)
    ctx.upload(r["A"])
    forms["a second call"] = ctx.variable_features(nf)
    for name, got in forms.items():
        for key, want in r["out"].items():
            assert np.array_equal(got[key], want), (name, key)
    assert forms["one-shot"]["names"] == ["g%d" % g for g in r["out"]["features"]]
    assert "names" not in forms["a second call"]


# -------------------------------------------------------------------------------------------------------------- state --
def _same(a, b, what):
    for x, y, name in zip(a, b, ("w", "d", "h")):
        assert np.array_equal(x, y), (what, name)


@pytest.mark.parametrize("case", ["k50-packed", "links"])
def test_a_fit_continued_after_a_selection_gives_the_same_bits(sa, case, monkeypatch):
    """Two iterations, a selection (and its operators), two more: w, d, h, tol and the sweep totals of four straight.  k = 50 on
    70 000 cells runs the H-side solve packed by the previous solve's sweep counts."""
    if case == "k50-packed":
        monkeypatch.setenv("SGL_NNLS_REPACK_MIN_COLS", "32768")
        m, n, k = 200, 70000, 50
    else:
        m, n, k = 120, 300, 12
    runs = {}
    for with_call in (False, True):
        with sa.Context(0) as c:
            c.synth(m, n, 20)
            c.fit_init(k)
            if case == "links":
                table = (np.random.default_rng(1).random((k, 4)) < 0.7).astype(np.float64)
                c.set_links_grouped(table, (np.arange(n) % 4).astype(np.int32))
            c.sweeps_get(reset=True)
            tols = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            if with_call:
                before = c.get_factors()
                out = c.variable_features(20)
                mean, _ = c.op_gene_mean()
                c.op_gene_var_std(mean, np.sqrt(c.op_gene_var(mean)), 10.0)
                _same(c.get_factors(), before, case)
                assert out["features"].shape == (20,) and np.array_equal(out["mean"], mean)
            tols += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            runs[with_call] = (c.get_factors(), tols, c.sweeps_get(reset=True))
    _same(runs[True][0], runs[False][0], case)
    assert runs[True][1] == runs[False][1], case
    for key in ("h_sweeps", "w_sweeps"):    # (the wave-level count differs between identical runs: tests/test_gpu_evaluate.py)
        assert runs[True][2][key] == runs[False][2][key], (case, key)


def test_a_masked_fit_is_untouched_by_selections_around_it(sa):
    runs = {}
    for with_call in (False, True):
        with sa.Context(0) as c:
            c.synth(200, 500, 10)
            c.fit_init(10)
            trace = []
            for _ in range(2):
                if with_call:
                    c.variable_features(30)
                r = c.ard_run(0.0, 2, 0.01, 0.0, 42, 8, 1e300, 1)
                trace.append((list(r["test_mse"]), list(r["tol"]), r["n_iter"]))
            if with_call:
                c.variable_features(30)
            runs[with_call] = (c.get_factors(), trace)
    _same(runs[True][0], runs[False][0], "masked")
    assert runs[True][1] == runs[False][1]


# ----------------------------------------------------------------------------------------------------------- refusals --
def test_refusals_return_their_code_and_leave_the_context_usable(sa):
    m, n = 40, 96
    D = vr.count_matrix(m, n, 2)
    A = sa.dgCMatrix.from_dense(D)
    x, i, p = vr.csc_of_dense(D)
    ref = vr.variable_features(*vr.gene_side(x, i, p, m), n, 10)

    def refused(c, code, match, **kw):
        dims = c.dims()
        with pytest.raises(sa.SingletHipError, match=match) as e:
            c.variable_features(**kw)
        assert e.value.code == code and str(e.value).strip() != ""
        assert c.dims() == dims

    with sa.Context(0) as c:
        refused(c, ESTATE, "no matrix resident", nfeatures=10)
        for op in (c.op_gene_mean, lambda: c.op_loess_direct(np.array([1.0, 0.0]), np.zeros(2), 2)):
            with pytest.raises(sa.SingletHipError) as e:
                op()
            assert e.value.code in (ESTATE, EINVAL)
        c.upload(A)
        refused(c, EINVAL, "nfeatures", nfeatures=0)
        refused(c, EINVAL, "nfeatures", nfeatures=-2)
        for span in (0.0, -0.3, 1.0000001, float("nan"), float("inf")):
            refused(c, EINVAL, "span", nfeatures=10, span=span)
        for bad in (-1.0, float("nan"), float("inf")):
            ev = np.ones(m)
            ev[5] = bad
            refused(c, EINVAL, r"expected_var\[5\]", nfeatures=10, expected_var=ev)
        c.set_allreduce(lambda dev_ptr, count: None)
        refused(c, ESTATE, "all-reduce hook", nfeatures=10)
        c.set_allreduce(None)
        # the trend's own refusals
        for xs, q in ((np.array([0.0, 2.0, 1.0]), 2), (np.arange(3.0), 0), (np.arange(3.0), 4), (np.array([0.0, np.nan, 1.0]), 2)):
            with pytest.raises(sa.SingletHipError, match="sgl_op_loess_direct") as e:
                c.op_loess_direct(xs, np.zeros(3), q)
            assert e.value.code == EINVAL
        out = c.variable_features(10)
        assert np.array_equal(out["features"], ref["features"]) and c.dims() == (m, n, A.nnz)
        # a gene of positive variance whose mean is not positive is named
        neg = D.copy()
        neg[13, :4] = [3.0, -3.0, 2.0, -2.0]
        neg[13, 4:] = 0.0
        c.upload(sa.dgCMatrix.from_dense(neg))
        refused(c, EINVAL, "gene 13", nfeatures=10)
        refused(c, EINVAL, "gene 13", nfeatures=10, expected_var=np.ones(m))   # whoever supplies the expected variances
        # one cell: no variance
        c.upload(sa.dgCMatrix.from_dense(D[:, :1]))
        refused(c, EINVAL, "ncol", nfeatures=10)
        # a shard
        c.upload(A, None, cell_offset=n, ncells_total=3 * n)
        refused(c, ESTATE, "shard", nfeatures=10)
        assert c.op_gene_mean()[0].shape == (m,)    # the stage operators run on whatever is resident
        c.upload(A)
        assert np.array_equal(c.variable_features(10)["features"], ref["features"])
    with sa.Multi([0, 0]) as M:
        M.upload(A)
        with pytest.raises(sa.SingletHipError, match="team") as e:
            M.rank_ctx(0).variable_features(10)
        assert e.value.code == ESTATE
    # the one-shot form refuses its arguments before anything is uploaded
    L = sa._lib.load()
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    feats, n_out = np.zeros(10, dtype=np.int32), C.c_int32()
    pp = lambda a, t=f64p: a.ctypes.data_as(t)   # noqa: E731

    def one_shot(nf, span, feats_p=pp(feats, i32p)):
        return L.sgl_c_variable_features(pp(A.x), pp(A.i, i32p), pp(A.p, i32p), m, n, nf, span, 0.0, None, feats_p, C.byref(n_out), None)

    assert one_shot(0, 0.3) == EINVAL and b"nfeatures" in L.sgl_last_error()
    assert one_shot(10, 1.5) == EINVAL and b"span" in L.sgl_last_error()
    assert one_shot(10, 0.3, None) == EINVAL
    assert one_shot(10, 0.3) == 0 and n_out.value == 10 and np.array_equal(feats, ref["features"])


# ------------------------------------------------------------------------------------------------------------- RunNMF --
def test_run_nmf_with_nfeatures_equals_run_nmf_on_the_selected_features(sa):
    m, n = 400, 500
    D = vr.count_matrix(m, n, 21)
    names = ["gene%d" % g for g in range(m)]
    x, i, p = vr.csc_of_dense(D)
    A = _dgc(sa, x, i, p, m, n, names)
    sel = sa.find_variable_features(A, 60)
    assert sel["features"].shape == (60,) and sel["names"] == [names[g] for g in sel["features"]]
    a = sa.RunNMF(A, k=4, nfeatures=60, seed=1, verbose=0)
    b = sa.RunNMF(A, k=4, features=sel["features"], seed=1, verbose=0)
    for key in ("w", "d", "h"):
        assert np.array_equal(a[key], b[key]), key
    assert a["w"].shape == (60, 4) and a["rownames_w"] == sel["names"] == b["rownames_w"]
    assert a["var_features"] == sel["names"] and "var_features" not in b
    # without row names: indices
    bare = sa.RunNMF(_dgc(sa, x, i, p, m, n), k=4, nfeatures=60, seed=1, verbose=0)
    assert np.array_equal(bare["var_features"], sel["features"]) and np.array_equal(bare["w"], a["w"])
    # refusals: not counts (after the upload's decision), and features next to nfeatures
    with pytest.raises(ValueError, match="variable features are selected on counts"):
        sa.RunNMF(_dgc(sa, x * 0.5, i, p, m, n), k=4, nfeatures=60, seed=1, verbose=0)
    with pytest.raises(ValueError, match="variable features are selected on counts"):
        sa.RunNMF(sa.native(((x * 0.5).astype(np.float32), i, p, (n, m), "csr"), cells_by_genes=True), k=4, nfeatures=60, seed=1, verbose=0)
    with pytest.raises(ValueError, match="either features or nfeatures"):
        sa.RunNMF(A, k=4, features=sel["features"], nfeatures=60, seed=1, verbose=0)
