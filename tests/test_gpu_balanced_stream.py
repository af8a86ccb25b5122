"""The balanced entry stream on the device (kernels_tiled.hip: tiled_count_kernel): the eight wave blocks of a workgroup level
their chunks of a stage by run-ahead.  The device's stored-entry count against the host model (scripts/layout_emulate.py)
with the balance and with SGL_TILED_NO_BALANCE=1 (the rule before), and bit equality of the sums: the balance moves entries
between the stages of a column, never their order."""
import numpy as np
import pytest

from conftest import rel_fro, to_dgc
from test_gpu_sliding_stream import L, _csc_from_dense, _pbmc3k, _skewed_csc, _window_stress

pytestmark = pytest.mark.gpu


def _set_balance(monkeypatch, balance):
    if balance:
        monkeypatch.delenv("SGL_TILED_NO_BALANCE", raising=False)
    else:
        monkeypatch.setenv("SGL_TILED_NO_BALANCE", "1")


@pytest.fixture(scope="module")
def matrices(ora):
    made = {}

    def get(name):
        if name not in made:
            A = {"iid": lambda: ora.synth_csc(2500, 3000, 10), "pbmc3k": lambda: _pbmc3k(ora),
                 "skewed": lambda: _skewed_csc(ora, 1500, 700, 3)}[name]()
            made[name] = (A, A.t())
        return made[name]
    return get


@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("matrix", ["iid", "pbmc3k", "skewed"])
def test_device_stream_equals_the_host_model_with_and_without_balance(sa, ora, matrices, matrix, k, monkeypatch):
    """Stored entries of both orientations, quad (k = 10) and pair (k = 50) layout, the tile rows and ranges the build chose:
    exactly the host model's count under either rule.  One context: the second fit_init must rebuild the streams, the
    switch is part of what keeps a stream valid."""
    A, At = matrices(matrix)
    nsl = 4 if k <= 32 else 2
    c = sa.Context(0)
    try:
        c.upload(to_dgc(sa, A), to_dgc(sa, At))
        lay = {}
        for balance in (True, False):
            _set_balance(monkeypatch, balance)
            c.fit_init(k, ora.synth_winit(k, A.nrow))
            lay[balance] = c.layout_get()
    finally:
        c.close()
    for balance in (True, False):
        for o, M in (("A", A), ("At", At)):
            got = lay[balance][o]
            want = L.entries(M.p, M.i, M.nrow, k, nsl, got["tile_rows"], ranges=got["tile_ranges"], balance=balance)
            assert got["entries"] == want, (matrix, o, balance, got, want)


@pytest.mark.parametrize("ranges", [1, 3])
@pytest.mark.parametrize("k", [10, 33, 50, 64, 70])
def test_balanced_window_stress_bit_equal(sa, ora, k, ranges, monkeypatch):
    """1100 columns: three workgroups of pairs (two of quads), the last one partial; 7 D + 37 rows.  The tiled kernel on the
    balanced stream, on the stream of the rule before, and -- the range whole -- the plain kernel add the same products in
    the same order.  (Three ranges add three partial sums per column: equal to the plain kernel up to rounding only, as in
    test_window_stress_forced_ranges; the two streams still agree bit for bit.)  k = 70: three quad passes over rank parts."""
    monkeypatch.setenv("SGL_TILED_RANGES", str(ranges))
    monkeypatch.setenv("SGL_TILED_FULL_TILES", "1")
    nsl = 4 if (k <= 32 or k > 64) else 2
    D = L.tile_rows(k, nsl) // 2
    m = 7 * D + 37
    X = _window_stress(m, 1100, D, k)
    A = ora.CSC(*_csc_from_dense(X))
    At = A.t()
    rng = np.random.default_rng(k)
    W, H = rng.random((m, k)), rng.random((A.ncol, k))
    kpart = k if k <= 64 else 24          # the part size of the streams at k = 70
    c = sa.Context(0)
    try:
        c.upload(to_dgc(sa, A), to_dgc(sa, At))
        got, lay = {}, {}
        for balance in (True, False):
            _set_balance(monkeypatch, balance)
            got[balance] = c.op_rhs(2, W), c.op_rhs(3, H)
            c.fit_init(k, ora.synth_winit(k, m))
            lay[balance] = c.layout_get()
        plain = c.op_rhs(0, W), c.op_rhs(1, H)
    finally:
        c.close()
    for o, (side, M) in enumerate((("A", A), ("At", At))):
        for balance in (True, False):
            g = lay[balance][side]
            assert g["tile_ranges"] == min(ranges, g["tiles"])       # (the 1100 rows of the transpose are two or three tiles)
            assert g["entries"] == L.entries(M.p, M.i, M.nrow, kpart, nsl, g["tile_rows"], ranges=ranges, balance=balance)
        # (the totals may coincide -- the balance moves groups between the stages -- so the model says whether the streams differ)
        cnts = [L.stream_counts(M.p, M.i, M.nrow, lay[True][side]["tile_rows"], nsl, ranges=ranges, balance=bal) for bal in (True, False)]
        assert not np.array_equal(*cnts), "the two rules build the same stream here: nothing compared"
        assert np.array_equal(got[True][o], got[False][o]), "balanced and unbalanced streams add the same products in the same order"
        if ranges == 1:
            assert np.array_equal(got[True][o], plain[o]), "tiled and plain kernels add the same products in the same order"
        else:
            assert rel_fro(got[True][o], plain[o]) < 1e-14


def test_fit_tol_bits_equal_with_and_without_balance(sa, monkeypatch):
    """Two iterations of a 3000 x 4000 fit at k = 50 on the balanced streams and on those of the rule before: the same tol bits"""
    tols, entries = {}, {}
    for balance in (True, False):
        _set_balance(monkeypatch, balance)
        with sa.Context(0) as c:
            c.synth(3000, 4000, 20)
            c.fit_init(50, None)
            tols[balance] = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            entries[balance] = c.layout_get()["A"]["entries"]
    assert entries[True] > 0 and entries[True] != entries[False]     # the fits ran on entry streams, and on different ones
    assert np.array(tols[True]).tobytes() == np.array(tols[False]).tobytes(), tols
    assert np.all(np.isfinite(tols[True]))
