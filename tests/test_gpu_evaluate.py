"""Model error on the device (sgl_evaluate / sgl_c_evaluate / sgl_multi_evaluate, kernels_eval.hip): bit-exact on integer
inputs at every rank where the accumulate, the Gram or the epilogue changes its kernel; within the first-order bound of
the three sums on real fits; the forms agree bit for bit; a fit continued after an evaluation is untouched; the team adds
up to the single context; the refusals leave the context usable."""
import ctypes as C

import numpy as np
import pytest

import evaluate_restatement as er
from conftest import to_dgc

pytestmark = pytest.mark.gpu

U = er.U
EINVAL, ESTATE = -1, -6
# every edge of the dispatch: the epilogue (lanes 64 | 65, G in LDS up to 128), the tiled accumulate (quads to 32, pairs to 64,
# three parts to 96, parts of 32 above), the plain accumulate's registers (64 k: 192 | 193, 256 | 257, 512 | 513), the Gram
# (16-row tiles, matrix cores for 129 - 256, generic above), the library's limit
RANKS = [1, 2, 16, 17, 31, 32, 33, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 512, 513, 1024]
REAL_SHAPES = [(300, 1000, 8, 20), (257, 700, 50, 20), (130, 900, 70, 4), (64, 65, 1, 3), (500, 640, 130, 20), (300, 400, 256, 20)]


# ------------------------------------------------------------------------------------------------------------ helpers --
def _int_matrix(rng, m, n):
    """Values 0..7, about a quarter stored; two empty columns, two empty rows, one column of a single entry."""
    D = (rng.integers(1, 8, (m, n)) * (rng.random((m, n)) < 0.25)).astype(np.float64)
    if n > 8:
        D[:, 3] = 0.0
        D[:, n - 1] = 0.0
        D[:, 7] = 0.0
        D[11 % m, 7] = 5.0
    if m > 8:
        D[5, :] = 0.0
        D[m - 1, :] = 0.0
    return D


def _int_factors(rng, m, n, k):
    """w m x k and h k x n in 0..3, d in 1..2, as doubles: every product and partial sum is an integer far below 2^53."""
    return (rng.integers(0, 4, (m, k)).astype(np.float64), rng.integers(1, 3, k).astype(np.float64),
            rng.integers(0, 4, (k, n)).astype(np.float64))


def _resident(sa, c, D, w, d, h, dense=False):
    if dense:
        c.upload_dense(D)
    else:
        c.upload(sa.dgCMatrix.from_dense(D))
    c.fit_init(w.shape[1])
    c.set_factors(w, d, np.ascontiguousarray(h.T))
    return c.evaluate(True, True)


def _assert_exact(out, D, w, d, h, what):
    cell, gene, sse = er.losses_int64(D, w, d, h)
    m, n = D.shape
    assert out["cell_loss"].shape == (n,) and out["gene_loss"].shape == (m,), what
    assert np.array_equal(out["cell_loss"], cell.astype(np.float64)), what
    assert np.array_equal(out["gene_loss"], gene.astype(np.float64)), what
    assert not np.signbit(out["cell_loss"]).any() and not np.signbit(out["gene_loss"]).any(), what
    assert out["sse"] == float(sse), what
    assert out["mse"] == float(sse) / (float(m) * float(n)), what


_REAL = {}


def _real_fit(ora, ctx, shape):
    """Four iterations of a device fit on ora.synth_csc, its evaluation and the long-double restatement, once per shape."""
    if shape not in _REAL:
        m, n, k, inv = shape
        A = ora.synth_csc(m, n, inv)
        ctx.upload(to_dgc_cached(A))
        ctx.fit_init(k)
        ctx.nmf_run(0.0, 4, 0.01, 0.01, 0.0, 0.0)
        W, d, H = ctx.get_factors()
        out = ctx.evaluate(True, True)
        again = ctx.evaluate(True, True)
        D = er.dense_of(A)
        _REAL[shape] = dict(A=A, D=D, w=W, d=d, h=np.ascontiguousarray(H.T), out=out, again=again,
                            ld=er.losses_longdouble(D, W, d, H.T))
    return _REAL[shape]


def to_dgc_cached(A):
    import singlet_amd as sa
    return to_dgc(sa, A)


def _gammas(D, k, extra=0):
    m, n = D.shape
    return (er.gamma(int((D != 0).sum(axis=0).max()), m, k, extra), er.gamma(int((D != 0).sum(axis=1).max()), n, k, extra))


def _assert_within(out, ld, D, k, factor, what):
    """|dev - exact| <= factor gamma A_j per cell and per gene; sse against the sum of the bounds plus its own summation."""
    g_cell, g_gene = _gammas(D, k)
    ec = np.abs(out["cell_loss"].astype(np.longdouble) - ld["cell"])
    eg = np.abs(out["gene_loss"].astype(np.longdouble) - ld["gene"])
    with np.errstate(invalid="ignore"):   # 0 / 0: a column with nothing stored under factors that are zero there
        print("evaluate-figure %s: worst cell err / (gamma A) = %.3g, gene = %.3g" %
              (what, float(np.nanmax(ec / (g_cell * ld["cell_abs"]))), float(np.nanmax(eg / (g_gene * ld["gene_abs"])))))
    assert np.all(ec <= factor * g_cell * ld["cell_abs"]), what
    assert np.all(eg <= factor * g_gene * ld["gene_abs"]), what


# ----------------------------------------------------------------------------------------------------- exact integers --
@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("m,n", [(70, 300), (257, 65)])
def test_integer_inputs_are_exact_at_every_kernel_edge(sa, ctx, m, n, k):
    """Every product and partial sum is an integer below 2^53, so any summation order and any contraction gives the exact
    result: cell_loss, gene_loss and sse equal the int64 restatement with ==, mse the Python float division."""
    rng = np.random.default_rng(1000 * m + k)
    D = _int_matrix(rng, m, n)
    w, d, h = _int_factors(rng, m, n, k)
    out = _resident(sa, ctx, D, w, d, h)
    _assert_exact(out, D, w, d, h, "m=%d n=%d k=%d" % (m, n, k))
    # one side at a time and none: the same numbers, the skipped side absent
    only_cell, only_gene, none = ctx.evaluate(True, False), ctx.evaluate(False, True), ctx.evaluate()
    assert np.array_equal(only_cell["cell_loss"], out["cell_loss"]) and "gene_loss" not in only_cell
    assert np.array_equal(only_gene["gene_loss"], out["gene_loss"]) and "cell_loss" not in only_gene
    assert sorted(none) == ["mse", "sse"] and none["sse"] == out["sse"] == only_gene["sse"] and none["mse"] == out["mse"]


@pytest.mark.parametrize("k", [1, 5, 50, 130])
def test_degenerate_matrices_are_exact(sa, ctx, k):
    """n = 1; one gene; a matrix with no stored entry at all (the losses are the quadratic form alone); more cells than one
    chunk of the reduction and one block of the epilogue."""
    rng = np.random.default_rng(77 + k)
    for m, n, empty in ((70, 1, False), (1, 40, False), (70, 300, True), (9, 2500, False)):
        D = np.zeros((m, n)) if empty else _int_matrix(rng, m, n)
        w, d, h = _int_factors(rng, m, n, k)
        out = _resident(sa, ctx, D, w, d, h)
        _assert_exact(out, D, w, d, h, "m=%d n=%d k=%d empty=%s" % (m, n, k, empty))
        if empty:
            rec = (w * d[None, :]) @ h
            assert np.array_equal(out["cell_loss"], (rec * rec).sum(axis=0))


@pytest.mark.parametrize("k,dense", [(3, False), (3, True), (70, False), (130, False)])
def test_exact_fit_block_model_gives_plus_zero_and_one_raised_entry_gives_one(sa, ctx, k, dense):
    """Gene block f x cell block f holds w_f d_f h_f, nothing is stored elsewhere: every loss is exactly +0.0.  One stored
    entry raised by 1: that cell and that gene give exactly 1.0, everything else +0.0, sse = 1."""
    rng = np.random.default_rng(9 + k)
    m, n = 2 * k + 64, 3 * k + 200
    gb, cb = np.sort(rng.integers(0, k, m)), np.sort(rng.integers(0, k, n))
    gb[:k], cb[:k] = np.arange(k), np.arange(k)     # no block is empty
    gb, cb = np.sort(gb), np.sort(cb)
    w, h = np.zeros((m, k)), np.zeros((k, n))
    w[np.arange(m), gb] = rng.integers(1, 4, m)
    h[cb, np.arange(n)] = rng.integers(1, 4, n)
    d = rng.integers(1, 3, k).astype(np.float64)
    D = (w * d[None, :]) @ h
    out = _resident(sa, ctx, D, w, d, h, dense)
    for key in ("cell_loss", "gene_loss"):
        assert np.all(out[key] == 0.0) and not np.signbit(out[key]).any(), key
    assert out["sse"] == 0.0 and out["mse"] == 0.0 and not np.signbit(out["sse"])
    i0, j0 = np.flatnonzero(gb == cb[n // 2])[0], n // 2
    assert D[i0, j0] > 0
    D[i0, j0] += 1.0
    out = _resident(sa, ctx, D, w, d, h, dense)
    want_c, want_g = np.zeros(n), np.zeros(m)
    want_c[j0], want_g[i0] = 1.0, 1.0
    assert np.array_equal(out["cell_loss"], want_c) and np.array_equal(out["gene_loss"], want_g)
    assert out["sse"] == 1.0 and out["mse"] == 1.0 / (float(m) * float(n))


def test_nan_and_inf_propagate_and_negative_cancellation_is_clamped(sa, ctx):
    rng = np.random.default_rng(4)
    m, n, k = 40, 90, 6
    D = _int_matrix(rng, m, n)
    w, d, h = _int_factors(rng, m, n, k)
    h[2, 10] = np.nan
    w[7, 1] = np.inf
    out = _resident(sa, ctx, D, w, d, h)
    assert np.isnan(out["cell_loss"][10]) and np.isnan(out["sse"]) and np.isnan(out["mse"])
    assert not np.isfinite(out["gene_loss"][7])
    # a near-exact real fit: whatever cancellation leaves, no loss is negative or -0.0
    w, h = rng.random((m, k)), rng.random((k, n))
    d = 1.0 + rng.random(k)
    D = (w * d[None, :]) @ h
    out = _resident(sa, ctx, D, w, d, h, dense=True)
    for key in ("cell_loss", "gene_loss"):
        assert np.all(out[key] >= 0.0) and not np.signbit(out[key]).any(), key


# --------------------------------------------------------------------------------------------------- real-valued fits --
@pytest.mark.parametrize("shape", REAL_SHAPES)
def test_real_fits_stay_within_the_first_order_bound(ora, ctx, shape):
    """|dev - exact| <= 4 gamma A_j with gamma = (max column nnz + m + k^2 + 4) 2^-53 (n for m on the gene side) and A_j the sum
    of the absolute values of the identity's terms: gamma A_j is the first-order bound of the three sums including the
    rounding of b and G, the 4 covers the order differences between kernel families.  mse against the oracle's full-matrix
    mse_test with m + n more roundings inside gamma for the oracle's own sequential sums."""
    m, n, k, inv = shape
    r = _real_fit(ora, ctx, shape)
    out, ld, D = r["out"], r["ld"], r["D"]
    _assert_within(out, ld, D, k, 4, "shape %r" % (shape,))
    g_mse = _gammas(D, k, extra=m + n)[0]
    ref = ora.mse_test(r["A"], r["w"], r["d"], np.ascontiguousarray(r["h"].T), 1, 1)
    bound = 4 * g_mse * ld["cell_abs"].sum() / (np.longdouble(m) * n)
    print("evaluate-figure shape %r: mse %.17g oracle %.17g, |diff| / bound = %.3g" % (shape, out["mse"], ref, float(abs(out["mse"] - ref) / bound)))
    assert abs(np.longdouble(out["mse"]) - np.longdouble(ref)) <= bound
    assert out["mse"] == out["sse"] / (float(m) * float(n))
    # two calls in a row: the same bits
    for key in ("cell_loss", "gene_loss"):
        assert np.array_equal(out[key], r["again"][key]), key
    assert out["sse"] == r["again"]["sse"] and out["mse"] == r["again"]["mse"]
    # the two sides sum the same residuals in different orders: each within its bound of the exact sum, plus the roundings
    # of the two summations themselves ((m + n) 2^-53 sse covers the chunk tree, the chunk order and numpy's pairwise sum)
    g_cell, g_gene = _gammas(D, k)
    slack = 4 * g_cell * ld["cell_abs"].sum() + 4 * g_gene * ld["gene_abs"].sum() + (m + n) * U * ld["sse"]
    assert abs(np.longdouble(out["gene_loss"].sum()) - np.longdouble(out["sse"])) <= slack


# --------------------------------------------------------------------------------------------------------- forms agree --
@pytest.mark.parametrize("shape", [(257, 700, 50, 20), (500, 640, 130, 20), (64, 65, 1, 3)])
def test_resident_one_shot_and_python_forms_agree_bit_for_bit(sa, ora, ctx, shape):
    m, n, k, inv = shape
    r = _real_fit(ora, ctx, shape)
    A, model = r["A"], {"w": r["w"], "d": r["d"], "h": r["h"]}
    dgc = to_dgc(sa, A)
    forms = {"dgCMatrix": sa.evaluate(dgc, model, True, True),
             "native": sa.evaluate(sa.native((A.x, A.i, A.p, (m, n), "csc")), model, True, True)}
    # the C one-shot entry itself
    f64p = C.POINTER(C.c_double)
    i32p = C.POINTER(C.c_int32)
    L = sa._lib.load()
    sse, mse, cl, gl = np.zeros(1), np.zeros(1), np.empty(n), np.empty(m)
    wk, hk, dk = np.ascontiguousarray(r["w"]), np.ascontiguousarray(r["h"].T), np.ascontiguousarray(r["d"])
    p = lambda a, t=f64p: a.ctypes.data_as(t)   # noqa: E731
    assert L.sgl_c_evaluate(p(A.x), p(A.i, i32p), p(A.p, i32p), m, n, p(wk), p(dk), p(hk), k, p(sse), p(mse), p(cl), p(gl)) == 0
    forms["sgl_c_evaluate"] = {"sse": sse[0], "mse": mse[0], "cell_loss": cl, "gene_loss": gl}
    # a fresh context fed the factors by set_factors
    with sa.Context(0) as c:
        c.upload(dgc, to_dgc(sa, A.t()))
        c.fit_init(k)
        c.set_factors(wk, dk, hk)
        forms["fresh context"] = c.evaluate(True, True)
    for name, got in forms.items():
        for key in ("cell_loss", "gene_loss"):
            assert np.array_equal(got[key], r["out"][key]), (name, key)
        assert got["sse"] == r["out"]["sse"] and got["mse"] == r["out"]["mse"], name


# ------------------------------------------------------------------------------------------------------- fit untouched --
def _state(c):
    W, d, H = c.get_factors()
    return W, d, H


def _same_state(a, b, what):
    for x, y, name in zip(a, b, ("w", "d", "h")):
        assert np.array_equal(x, y), (what, name)


@pytest.mark.parametrize("case", ["k50-packed", "k130", "links", "graph"])
def test_a_fit_continued_after_an_evaluation_gives_the_same_bits(sa, ora, case, monkeypatch):
    """Two iterations, an evaluation of both sides, two more: w, d, h, tol and the sweep totals of four straight.  k = 50 on
    70 000 cells runs the H-side solve packed by the previous solve's sweep counts (and re-packed between passes); with
    grouped links and with a graph set the loss is still that of the plain reconstruction."""
    rng = np.random.default_rng(12)
    if case == "k50-packed":
        monkeypatch.setenv("SGL_NNLS_REPACK_MIN_COLS", "32768")
        m, n, k, A = 200, 70000, 50, None
    elif case == "k130":
        m, n, k = 257, 700, 130
        A = ora.synth_csc(m, n, 20)
    else:
        m, n, k = 120, 300, 12
        A = ora.synth_csc(m, n, 6)

    def prepare(c):
        if A is None:
            c.synth(m, n, 20)
        else:
            c.upload(to_dgc(sa, A))
        c.fit_init(k)
        if case == "links":
            G = 4
            table = (np.random.default_rng(1).random((k, G)) < 0.7).astype(np.float64)
            c.set_links_grouped(table, (np.arange(n) % G).astype(np.int32))
        elif case == "graph":
            ring = np.zeros((n, n))
            idx = np.arange(n)
            ring[idx, idx] = 0.5
            ring[(idx + 1) % n, idx] = 0.25
            ring[(idx - 1) % n, idx] = 0.25
            c.set_graph(sa.dgCMatrix.from_dense(ring))
        c.sweeps_get(reset=True)

    runs = {}
    for with_eval in (False, True):
        with sa.Context(0) as c:
            prepare(c)
            tols = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            if with_eval:
                before = _state(c)
                out = c.evaluate(True, True)
                _same_state(_state(c), before, case)
            tols += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            runs[with_eval] = (_state(c), tols, c.sweeps_get(reset=True))
    _same_state(runs[True][0], runs[False][0], case)
    assert runs[True][1] == runs[False][1], case
    # the sweeps every column needed (the wave-level count follows the order in which the re-packing passes' lists were
    # appended to, which differs from run to run: tests/test_gpu_nmf.py compares the same two totals)
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], (case, key)
    if A is not None:   # the loss after two iterations is the plain reconstruction's, links or graph or not
        W, d, H = before
        D = er.dense_of(A)
        _assert_within(out, er.losses_longdouble(D, W, d, H.T), D, k, 4, case)
    assert np.isfinite(out["sse"]) and out["sse"] > 0


@pytest.mark.parametrize("k", [10, 50])
def test_a_masked_fit_is_untouched_by_evaluations_around_it(sa, ora, k):
    """sgl_ard_run twice in a row, with and without evaluations before, between and after: the same factors and traces."""
    A = ora.synth_csc(200, 500, 10)
    runs = {}
    for with_eval in (False, True):
        with sa.Context(0) as c:
            c.upload(to_dgc(sa, A))
            c.fit_init(k)
            trace = []
            for _ in range(2):
                if with_eval:
                    c.evaluate(True, True)
                r = c.ard_run(0.0, 2, 0.01, 0.0, 42, 8, 1e300, 1)
                trace.append((list(r["test_mse"]), list(r["tol"]), r["n_iter"]))
            if with_eval:
                out = c.evaluate(True, True)
                W, d, H = c.get_factors()
                D = er.dense_of(A)
                _assert_within(out, er.losses_longdouble(D, W, d, H.T), D, k, 4, "masked k=%d" % k)
            runs[with_eval] = (_state(c), trace)
    _same_state(runs[True][0], runs[False][0], "masked")
    assert runs[True][1] == runs[False][1]


# ---------------------------------------------------------------------------------------------------------------- team --
def _team_set_factors(M, w, d, h):
    lo = 0
    for r in range(M.n):
        c = M.rank_ctx(r)
        nloc = c.dims()[1]
        c.set_factors(w, d, np.ascontiguousarray(h[:, lo:lo + nloc].T))
        lo += nloc
    assert lo == h.shape[1]


@pytest.mark.parametrize("m,n,k,ranks", [(300, 1000, 8, 2), (300, 1000, 8, 3), (300, 1000, 8, 8), (96, 400, 5, 7)])
def test_team_is_exact_on_integers_and_within_twice_the_bound_on_a_fit(sa, ora, ctx, m, n, k, ranks):
    rng = np.random.default_rng(ranks)
    D = _int_matrix(rng, m, n)
    w, d, h = _int_factors(rng, m, n, k)
    single = _resident(sa, ctx, D, w, d, h)
    A = ora.synth_csc(m, n, 20)
    with sa.Multi([0] * ranks) as M:
        M.upload(sa.dgCMatrix.from_dense(D))
        M.fit_init(k)
        _team_set_factors(M, w, d, h)
        out = M.evaluate(True, True)
        _assert_exact(out, D, w, d, h, "team of %d" % ranks)     # cell_loss in global cell order
        for key in ("cell_loss", "gene_loss"):
            assert np.array_equal(out[key], single[key]), key
        assert out["sse"] == single["sse"] and out["mse"] == single["mse"]
        assert sorted(M.evaluate()) == ["mse", "sse"]
        # a rank's own context refuses: its losses are not the matrix's
        rc = M.rank_ctx(0)
        with pytest.raises(sa.SingletHipError, match="sgl_multi_evaluate") as e:
            rc.evaluate()
        assert e.value.code == ESTATE
        # a real fit on the team
        M.upload(to_dgc(sa, A))
        M.fit_init(k)
        M.nmf_run(0.0, 4, 0.01, 0.01, 0.0, 0.0)
        W, dd, H = M.get_factors()
        out = M.evaluate(True, True)
        again = M.evaluate(True, True)
    Dr = er.dense_of(A)
    ld = er.losses_longdouble(Dr, W, dd, H.T)
    _assert_within(out, ld, Dr, k, 8, "team of %d, real fit" % ranks)
    g_cell = _gammas(Dr, k)[0]
    assert abs(np.longdouble(out["sse"]) - ld["sse"]) <= 8 * g_cell * ld["cell_abs"].sum() + (n + ranks) * U * ld["sse"]
    assert out["mse"] == out["sse"] / (float(m) * float(n))
    for key in ("cell_loss", "gene_loss"):
        assert np.array_equal(out[key], again[key])
    assert out["sse"] == again["sse"]


# ----------------------------------------------------------------------------------------------------------- refusals --
def test_refusals_leave_the_context_usable(sa):
    rng = np.random.default_rng(3)
    m, n, k = 30, 50, 4
    D = _int_matrix(rng, m, n)
    w, d, h = _int_factors(rng, m, n, k)
    with sa.Context(0) as c:
        with pytest.raises(sa.SingletHipError, match="no matrix resident") as e:
            c.evaluate()
        assert e.value.code == ESTATE
        c.upload(sa.dgCMatrix.from_dense(D))
        with pytest.raises(sa.SingletHipError, match="no fit initialised") as e:
            c.evaluate(True, True)
        assert e.value.code == ESTATE
        c.fit_init(k)
        c.set_factors(w, d, np.ascontiguousarray(h.T))
        c.set_allreduce(lambda dev_ptr, count: None)
        with pytest.raises(sa.SingletHipError, match="all-reduce hook") as e:
            c.evaluate()
        assert e.value.code == ESTATE
        c.set_allreduce(None)
        _assert_exact(c.evaluate(True, True), D, w, d, h, "after the refusals")
        # a new upload drops the fit
        c.upload(sa.dgCMatrix.from_dense(D))
        with pytest.raises(sa.SingletHipError, match="no fit initialised"):
            c.evaluate()
    with sa.Multi([0, 0]) as M:
        with pytest.raises(sa.SingletHipError) as e:
            M.evaluate()
        assert e.value.code == ESTATE
        M.upload(sa.dgCMatrix.from_dense(D))
        with pytest.raises(sa.SingletHipError, match="no fit initialised") as e:
            M.evaluate()
        assert e.value.code == ESTATE


def test_one_shot_form_refuses_bad_ranks_and_null_factors(sa):
    rng = np.random.default_rng(8)
    m, n, k = 30, 50, 4
    D = _int_matrix(rng, m, n)
    A = sa.dgCMatrix.from_dense(D)
    w, d, h = _int_factors(rng, m, n, k)
    wk, hk = np.ascontiguousarray(w), np.ascontiguousarray(h.T)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L = sa._lib.load()
    p = lambda a, t=f64p: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    sse = np.zeros(1)

    def call(w_, d_, h_, k_):
        return L.sgl_c_evaluate(p(A.x), p(A.i, i32p), p(A.p, i32p), m, n, p(w_), p(d_), p(h_), k_, p(sse), None, None, None)

    assert call(wk, d, hk, 0) == EINVAL and b"rank" in L.sgl_last_error()
    assert call(wk, d, hk, 1025) == EINVAL
    assert call(wk, d, hk, -3) == EINVAL
    for args in ((None, d, hk), (wk, None, hk), (wk, d, None)):
        assert call(*args, k) == EINVAL and b"NULL factor" in L.sgl_last_error()
    assert call(wk, d, hk, k) == 0 and sse[0] == float(er.losses_int64(D, w, d, h)[2])
    # an invalid matrix is refused as by the upload (row index out of range)
    bad = A.i.copy()
    bad[0] = m
    assert L.sgl_c_evaluate(p(A.x), p(bad, i32p), p(A.p, i32p), m, n, p(wk), p(d), p(hk), k, p(sse), None, None, None) == EINVAL


@pytest.mark.parametrize("fill", [0.2, 0.9])
def test_after_a_dense_upload_the_call_works_over_the_csc_image(sa, ctx, fill):
    """The header's statement for sgl_upload_dense: the evaluation runs over the CSC image kept next to the dense matrix,
    below and above the half-full threshold of the GEMM right-hand sides; same bits as after the sparse upload."""
    rng = np.random.default_rng(21)
    m, n, k = 70, 300, 9
    D = (rng.integers(1, 8, (m, n)) * (rng.random((m, n)) < fill)).astype(np.float64)
    w, d, h = _int_factors(rng, m, n, k)
    out = _resident(sa, ctx, D, w, d, h, dense=True)
    _assert_exact(out, D, w, d, h, "dense upload, fill %g" % fill)
    wr, hr = rng.random((m, k)), rng.random((k, n))
    a = _resident(sa, ctx, D, wr, d, hr, dense=True)
    b = _resident(sa, ctx, D, wr, d, hr, dense=False)
    for key in ("cell_loss", "gene_loss"):
        assert np.array_equal(a[key], b[key]), key
    assert a["sse"] == b["sse"]
