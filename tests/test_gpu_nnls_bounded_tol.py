"""The bounded-tol lane solve (kernels_nnls_asm_bounded.hip) on the device: bit-identical to the exact generated kernels
(SGL_NNLS_EXACT_TOL=1) -- X and the sweep totals -- whatever the band: the default delta, where a tainted column is a rarity;
SGL_NNLS_TOL_BAND=0.5, where every column that stops by its tol on the way through the band is solved again by the exact
kernel, from the first pass or from a later one; and a band in between, where some are."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BANDS = (None, "0.1", "0.5")      # default delta; some columns taint; (nearly) all do
NCOLS = (1, 63, 64, 65, 197)


def _setenv(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _redo_counts(capfd):
    """the redo-list lengths the solves since the last call reported (SGL_NNLS_TRACE_REDO=1)"""
    return [int(a) for a in re.findall(r"nnls redo: (\d+) of", capfd.readouterr().err)]


@pytest.mark.parametrize("k", [6, 20, 49, 50])
def test_operator_solve_is_bit_identical_in_every_band(ctx, k, monkeypatch, capfd):
    """sgl_op_nnls at ragged column counts, one pass and re-packed passes (several passes even at 197 columns: a re-pack threshold
    of 64 columns, so that tainted columns come from later passes too), cold and warm starts, L1 on and off."""
    rng = np.random.default_rng(5200 + k)
    F = rng.random((3 * k + 5, k))
    G = F.T @ F + 1e-15 * np.eye(k)
    monkeypatch.setenv("SGL_NNLS_TRACE_REDO", "1")
    redo = {b: 0 for b in BANDS}
    for ncols in NCOLS:
        L1 = 0.02 if ncols % 2 else 0.0
        B = rng.normal(size=(ncols, k)) * 3 + 1.0
        B *= np.exp(rng.normal(size=(ncols, 1)) * 2)
        X0 = np.abs(rng.normal(size=(ncols, k))) * (rng.random((ncols, k)) < 0.5) * 1e-3
        for repack in (None, "64"):
            _setenv(monkeypatch, "SGL_NNLS_REPACK_MIN_COLS", repack)
            monkeypatch.setenv("SGL_NNLS_EXACT_TOL", "1")
            monkeypatch.delenv("SGL_NNLS_TOL_BAND", raising=False)
            X, s = ctx.op_nnls(G, B, X0, L1, 0.0)
            assert _redo_counts(capfd) == []          # the exact kernels keep no redo list
            monkeypatch.delenv("SGL_NNLS_EXACT_TOL")
            for band in BANDS:
                _setenv(monkeypatch, "SGL_NNLS_TOL_BAND", band)
                Xb, sb = ctx.op_nnls(G, B, X0, L1, 0.0)
                n = _redo_counts(capfd)
                assert len(n) == 1 and 0 <= n[0] <= ncols, (n, ncols)
                redo[band] += n[0]
                assert np.array_equal(X, Xb) and s == sb, (ncols, repack, band, n)
    print("k = %d: redo-list lengths summed over the cases, by band:" % k, redo)
    # a wider band contains the narrower one: a column tainted in the narrower is tainted (no later) in the wider
    assert redo[None] <= redo["0.1"] <= redo["0.5"] and redo["0.5"] > 0


@pytest.mark.parametrize("k,m,n", [(6, 63, 197), (20, 197, 65), (49, 64, 197), (50, 197, 64)])
def test_fit_is_bit_identical_in_every_band(sa, k, m, n, monkeypatch, capfd):
    """The H side and the W side of a resident fit (sgl_nnls_shared with the fit's own scratch; the four-columns-per-wave solve of
    short launches switched off so that the lane solve runs): factors, tols and both sides' sweep totals after three iterations."""
    monkeypatch.setenv("SGL_NNLS_QUAD_SHARED_MAX_COLS", "0")
    monkeypatch.setenv("SGL_NNLS_TRACE_REDO", "1")

    def fit():
        with sa.Context(0) as c:
            c.synth(m, n, 5)
            c.fit_init(k)
            c.sweeps_get(reset=True)
            tols = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(3)]
            sw = c.sweeps_get(reset=True)
            return c.get_factors(), tols, (sw["h_sweeps"], sw["w_sweeps"])

    for repack in (None, "64"):
        _setenv(monkeypatch, "SGL_NNLS_REPACK_MIN_COLS", repack)
        monkeypatch.setenv("SGL_NNLS_EXACT_TOL", "1")
        monkeypatch.delenv("SGL_NNLS_TOL_BAND", raising=False)
        (W, D, H), tols, sw = fit()
        assert _redo_counts(capfd) == []
        monkeypatch.delenv("SGL_NNLS_EXACT_TOL")
        for band in BANDS:
            _setenv(monkeypatch, "SGL_NNLS_TOL_BAND", band)
            (Wb, Db, Hb), tolsb, swb = fit()
            nred = _redo_counts(capfd)
            assert len(nred) == 6, nred                # three H-side and three W-side solves went the bounded way
            assert np.array_equal(W, Wb) and np.array_equal(D, Db) and np.array_equal(H, Hb), (repack, band, nred)
            assert tols == tolsb and sw == swb, (repack, band, nred)
            if band == "0.5":
                assert sum(nred) > 0
