"""The product, through its C ABI, against a BUILD OF THE REFERENCE'S OWN STATEMENTS -- not through the oracle.

oracle/make_ref.sh cuts the ALS functions out of the reference tree at build time and compiles them against
oracle/standin/ (DESIGN.md "Oracle status"); the two libraries travel with oracle/_ref/.  Where they are present each
case is run live on variant A; otherwise the outputs that tests/golden/make_als_ref.py stored (tests/golden/als_ref.npz)
stand in.  The cases are those of tests/als_ref_cases.py that the fixture admits (the reference build against its own
second variant: every integer / structural output equal, every floating-point output within 1e-12).

Bounds: integer and structural outputs (iter vectors, iteration counts, NaN / Inf / zero patterns, the graph's pattern)
exactly; floating-point outputs at the project's parity bar, 1e-9 relative Frobenius.  The reference prints its
tolerance trace with three digits and returns no other: the product's trace is compared with the printed one to one
unit of the third digit.
"""
import os

import numpy as np
import pytest

import als_ref_cases as rc
from conftest import to_dgc
from oracle import reference

pytestmark = pytest.mark.gpu
PARITY = 1e-9       # DESIGN.md "Parity bar"

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "als_ref.npz")
_admitted = set(np.load(GOLD)["admitted"].tolist())
CASES = [c for c in rc.cases() if rc.case_id(c) in _admitted]

SEEN = {}           # entry -> [cases, largest distance, largest stored spread]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _fit(r, w_is_k_by_m=True):
    out = dict(w=r["w"].T if w_is_k_by_m else r["w"], d=r["d"], h=r["h"].T)
    if "test_mse" in r:
        out.update(test_mse=r["test_mse"], iter=np.asarray(r["iter"], dtype=np.int64), tol=r["tol"], score_overfit=r["score_overfit"])
    else:
        out["n_iter"] = np.array([r["iter"]], dtype=np.int64)
        out["tol_printed"] = np.asarray(r["tol"], dtype=np.float64)      # full precision: compared with the printed digits
    return out


def product(case, sa, ctx, ora):
    """The case on the GPU: {output name: array} in the layout of als_ref_cases.run."""
    entry, name, p = case
    if entry == "nnls":
        F, B, X0 = rc.nnls_inputs(p["k"])
        X, _ = ctx.op_nnls(ctx.op_gram(F), B, X0, p["L1"], p["L2"])
        return dict(x=X)
    if entry == "scale_cor":
        F, y = rc.scale_cor_inputs(p)
        S, d = ctx.op_scale(F)
        return dict(s=S, d=d, cor=np.array([ctx.op_cor(F.ravel(), y.ravel())]))
    if entry == "aat":
        return dict(g=ctx.op_gram(np.random.default_rng(2).random((p["cols"], p["k"]))))
    if entry in ("predict", "predict_mask", "predict_mask_degenerate"):
        if entry == "predict_mask_degenerate":
            A, M, F = rc.degenerate_inputs(ora, p)
            X0, L1, L2 = np.zeros((M.ncol, p["k"])), 0.01, 0.0
        else:
            M, F, X0 = rc.predict_inputs(ora, p)
            A, L1, L2 = (M.t() if p["mask_t"] else M), p["L1"], p["L2"]
        ctx.upload(to_dgc(sa, A), to_dgc(sa, A.t()))
        k = p["k"]
        masked = entry != "predict"
        if not p["mask_t"]:                       # H side: w is the operand, h the warm start
            ctx.fit_init(k, F)
            ctx.set_factors(h=X0)
            ctx.step_h_masked(L1, L2, 99, 8) if masked else ctx.step_h(L1, L2)
            return dict(x=ctx.get_factors()[2])
        ctx.fit_init(k, X0)                       # W side: h is the operand, w the warm start
        ctx.set_factors(w=X0, h=F)
        ctx.step_w_masked(L1, L2, 99, 8) if masked else ctx.step_w(L1, L2)
        return dict(x=ctx.get_factors()[0])
    if entry == "mse_test":
        A, w, d, h = rc.mse_inputs(ora, p)
        ctx.upload(to_dgc(sa, A), to_dgc(sa, A.t()))
        ctx.fit_init(p["k"], w)
        ctx.set_factors(w=w, d=d, h=h)
        return dict(mse=np.array([ctx.op_mse_test(31, p["inv_density"])]))
    I = rc.inputs(ora, case)
    dg = lambda M: to_dgc(sa, M)      # noqa: E731
    if entry == "c_nmf":
        return _fit(sa.c_nmf(dg(I["A"]), dg(I["At"]), p["tol"], p["maxit"], False, p["L1w"], p["L1h"], p["L2w"], p["L2h"], 0, I["w0"].T))
    if entry == "c_nmf_dense":
        return _fit(sa.c_nmf_dense(I["D"], None, 0.0, p["maxit"], False, 0.01, 0.01, 0.0, 0.0, 0, I["w0"].T))
    if entry == "c_nmf_sparse_list":
        return _fit(sa.c_nmf_sparse_list([dg(c) for c in I["A_"]], [dg(c) for c in I["At_"]], 0.0, p["maxit"], False, 0.01, 0.0, 0, I["w0"].T))
    if entry == "c_linked_nmf":
        return _fit(sa.c_linked_nmf(dg(I["A"]), dg(I["At"]), 0.0, p["maxit"], False, p["L1"], p["L2"], 0, I["w0"].T, I["link_h"], I["link_w"]))
    if entry == "c_project_model":
        r = sa.c_project_model(dg(I["A"]), I["w"], p["L1"], p["L2"], 0)
        return dict(h=r["h"].T, d=r["d"])
    if entry == "rcpp_predict":
        return dict(h=sa.Rcpp_predict(dg(I["A"]), I["w"], p["L1"], p["L2"], 0).T)
    if entry == "c_ard_nmf":
        return _fit(sa.c_ard_nmf(dg(I["A"]), dg(I["At"]), p["tol"], p["maxit"], False, p["L1"], p["L2"], 0, I["w0"].T, p["seed"],
                                 p["inv_density"], p["thr"], p["trace"]))
    if entry == "c_ard_nmf_dense":
        return _fit(sa.c_ard_nmf_dense(I["D"], None, 0.0, p["maxit"], False, 0.01, 0.0, 0, I["w0"].T, 31, 10, 1e-3, p["trace"]))
    if entry == "c_ard_nmf_sparse_list":
        return _fit(sa.c_ard_nmf_sparse_list([dg(c) for c in I["A_"]], [dg(c) for c in I["At_"]], 0.0, p["maxit"], False, 0.01, 0.0, 0,
                                             I["w0"].T, 31, 10, 1e-3, p["trace"]))
    if entry == "c_gcnmf":
        return _fit(sa.c_gcnmf(dg(I["A"]), dg(I["At"]), dg(I["G"]), 0.0, p["maxit"], False, p["L1"], p["L2"], 0, I["w"]), w_is_k_by_m=False)
    if entry == "spatial_graph":
        G = sa.spatial_graph(I["x"], I["y"], p["max_dist"], p["max_k"])
        return dict(p=np.asarray(G.p, dtype=np.int64), i=np.asarray(G.i, dtype=np.int64), x=np.asarray(G.x, dtype=np.float64))
    if entry == "rowwise_sparse":       # RasterizeRowwise on a dgCMatrix: the sparse native
        return dict(res=np.ascontiguousarray(np.asarray(sa.RasterizeRowwise(dg(I["A"]), p["n"]))))
    if entry == "rowwise_dense":        # ... on anything else: the dense native
        return dict(res=np.ascontiguousarray(np.asarray(sa.RasterizeRowwise(I["D"], p["n"]))))
    raise KeyError(entry)


PRODUCT_ENTRIES = set(c[0] for c in CASES) - {"nnls_quirks", "predict_dense"}   # two-coordinate hand cases and the dense predict
#                                                                                 have no operator of their own in the C ABI


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in PRODUCT_ENTRIES], ids=rc.case_id)
def test_product_against_the_reference_build(sa, ctx, ora, gold, case):
    cid = rc.case_id(case)
    got = product(case, sa, ctx, ora)
    live = rc.run(case, reference.variant("a"), ora) if reference.available("a") else None
    worst = 0.0
    for key, a in got.items():
        if live is not None:
            b = live[key]
            if rc.is_exact(key):
                dist, same = 0.0, np.asarray(a).shape == np.asarray(b).shape and np.array_equal(a, b)
            else:
                dist, same = rc.rel(a, b), rc.same_structure(a, b, key)
        else:
            dist, same = rc.against_stored(cid, key, a, gold)
        if key == "tol_printed":
            # three printed digits: one unit of the third is at most 1 % of the value
            b = live[key] if live is not None else gold["%s/%s" % (cid, key)]
            assert a.shape == b.shape and np.all(np.abs(a - b) <= 0.0101 * np.abs(b)), (cid, a, b)
            continue
        print("%-40s %-14s %.3e%s" % (cid, key, dist, "" if same else "  STRUCTURE DIFFERS"))
        assert same, "%s %s: integer / NaN / Inf / zero structure differs from the reference build" % (cid, key)
        if not rc.is_exact(key):
            assert dist <= PARITY, "%s %s: %.3e from the reference build" % (cid, key, dist)
            worst = max(worst, dist)
    spread = max([float(v) for k, v in gold.items() if k.startswith(cid + "/") and k.endswith("@spread")] or [0.0])
    s = SEEN.setdefault(case[0], [0, 0.0, 0.0])
    s[0], s[1], s[2] = s[0] + 1, max(s[1], worst), max(s[2], spread)


def test_report_per_entry_point():
    """Not a check of its own: prints, per entry point, the number of cases, the largest distance to the reference build
    and the largest stored spread (run with -s to see it)."""
    print("\n%-26s %5s %12s %12s" % ("entry", "cases", "max distance", "max spread"))
    for entry in sorted(SEEN):
        n, dist, spread = SEEN[entry]
        print("%-26s %5d %12.2e %12.2e" % (entry, n, dist, spread))
