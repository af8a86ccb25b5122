"""The graph convolution of graph-convolutional NMF (graph_conv_kernel, singlet_amd/csrc/kernels_graph.hip) on its own,
through sgl_op_graph_conv: every instance the dispatch can reach, on column lengths at every edge of the kernel's loops
(gcnmf_restatement.edge_length_graph: the four-deep main loop and its tail, 128 | 129 entries, hubs of 64 + 64 + 1 and of
whole multiples of the segment length, adjacent hubs, hubs in the first and the last column, weights of both signs).

The operator runs k_graph_conv as sgl_step_h / sgl_step_w do, on the DevGraph sgl_set_graph made: every rank below runs
the main pass (SEGS = false) on the 173 columns of at most 128 entries and the segment pass (SEGS = true) plus the hub
combine on the 147 longer ones.  Which rank runs which instance (VEC = 2 for even k, 1 for odd k; ne = k / VEC elements
per column; LPC lanes per column; NP passes of 64 lanes):

    VEC = 2 (even k)                         VEC = 1 (odd k)
    k = 2            LPC  1  NP 1            k = 1            LPC  1  NP  1
    k = 4            LPC  2  NP 1            k = 3            LPC  4  NP  1
    k = 6, 8         LPC  4  NP 1            k = 5, 7         LPC  8  NP  1
    k = 10, 16       LPC  8  NP 1            k = 9, 15        LPC 16  NP  1
    k = 18, 32       LPC 16  NP 1            k = 17, 31       LPC 32  NP  1
    k = 34, 64       LPC 32  NP 1            k = 33, 63       LPC 64  NP  1
    k = 66, 128      LPC 64  NP 1            k = 65, 127      LPC 64  NP  2
    k = 130, 256     LPC 64  NP 2            k = 129, 255     LPC 64  NP  4
    k = 258, 512     LPC 64  NP 4            k = 257, 511     LPC 64  NP  8
    k = 514, 1024    LPC 64  NP 8            k = 513, 1023    LPC 64  NP 16

Each instance is run at its smallest and its largest rank (the largest leaves no idle lane, the smallest the most), 20
instances, each with SEGS false and true.  The HALO instances need a team: tests/test_gpu_gcnmf_team.py.
"""
import numpy as np
import pytest

import gcnmf_restatement as gr
from conftest import to_dgc

pytestmark = pytest.mark.gpu

N = 320
EVEN = [2, 4, 6, 8, 10, 16, 18, 32, 34, 64, 66, 128, 130, 256, 258, 512, 514, 1024]
ODD = [1, 3, 5, 7, 9, 15, 17, 31, 33, 63, 65, 127, 129, 255, 257, 511, 513, 1023]
_CACHE = {}


def _matrix(ora):
    """the resident matrix: its values play no part, its 320 cells size the graph"""
    if "A" not in _CACHE:
        _CACHE["A"] = ora.synth_csc(40, N, 10)
    return _CACHE["A"]


def _exact_graph(ora):
    if "exact" not in _CACHE:
        _CACHE["exact"] = gr.edge_length_graph(ora, N)
    return _CACHE["exact"]


def _normal_graph(ora):
    if "normal" not in _CACHE:
        _CACHE["normal"] = gr.edge_length_graph(ora, N, weights=np.random.default_rng(29).standard_normal)
    return _CACHE["normal"]


def _ready(sa, ora, ctx, k, G):
    """fit of rank k on the resident matrix with G set: what sgl_op_graph_conv needs"""
    A = _matrix(ora)
    ctx.upload(to_dgc(sa, A))
    ctx.fit_init(k, ora.synth_winit(k, A.nrow))
    ctx.set_graph(to_dgc(sa, G))


def _conv(ctx, X):
    """op_graph_conv into a buffer of NaN: an element the kernels do not write cannot pass"""
    Y = np.full(X.shape, np.nan)
    assert ctx.op_graph_conv(X, out=Y) is Y
    return Y


def _exact_x(k):
    return (1024.0 * np.arange(N)[:, None] + np.arange(k)[None, :] + 1.0)


def _exact_reference(G, k):
    """8 * Y in int64: weights are whole eighths, X whole numbers"""
    Xi = 1024 * np.arange(N, dtype=np.int64)[:, None] + np.arange(k, dtype=np.int64)[None, :] + 1
    w8 = np.rint(G.x * 8).astype(np.int64)
    assert np.array_equal(w8 / 8.0, G.x) and np.abs(w8).max() == 15 and w8.min() < 0 < w8.max()
    ref8 = np.zeros((N, k), dtype=np.int64)
    for c in range(N):
        s = slice(G.p[c], G.p[c + 1])
        ref8[c] = (w8[s, None] * Xi[G.i[s]]).sum(axis=0)
    assert np.abs(ref8).max() < 2 ** 31   # every partial sum of |terms| is below 2^31 eighths too: exact in any order
    return ref8


@pytest.mark.parametrize("k", EVEN + ODD)
def test_graph_conv_exact(sa, ora, ctx, k):
    """X[r, f] = 1024 r + f + 1 and weights of whole eighths: every product and every partial sum is exact in float64
    (below 2^31 eighths), so the result is the same number in any order, fused or not, segmented or not -- and every
    (row, factor) carries its own value, so a mis-indexed gather, a dropped tail entry, a doubled or dropped segment or an
    element that is not written changes the result.  Equal to the int64 sum, element by element."""
    G = _exact_graph(ora)
    _ready(sa, ora, ctx, k, G)
    Y = _conv(ctx, _exact_x(k))
    ref = _exact_reference(G, k) / 8.0
    bad = np.argwhere(~(Y == ref))
    assert bad.size == 0, "k = %d: %d elements differ, first at (column %d, factor %d): got %r, expected %r (column of %d entries)" % (
        k, len(bad), bad[0][0], bad[0][1], Y[tuple(bad[0])], ref[tuple(bad[0])], np.diff(G.p)[bad[0][0]])
    assert np.array_equal(Y, ref)


@pytest.mark.parametrize("k", EVEN + ODD)
def test_graph_conv_rounding_bound(sa, ora, ctx, k):
    """standard_normal weights on the same structure, X = standard_normal * exp(uniform(-8, 8)): mixed signs, seven decades
    of scale.  Against the sum in long double, per element |Y - ref| <= (d + 2) 2^-53 sum |v| |x|, d the column's entry
    count.  That is the bound of a length-d dot product summed in ANY order: no term passes through more than d roundings
    (its product and at most d - 1 additions; an addition onto an exact zero does not round, fusing removes the product's),
    so the error is within gamma_d = d u / (1 - d u) of sum |v| |x|, u = 2^-53.  The sequential fused loop is one such
    order; a hub's 64-entry partials added in segment order is another.  The + 2 covers 1 / (1 - d u) and the long double
    reference's own error (d 2^-64 of the same sum).  Derived, not measured.  A second call returns the same bits."""
    G = _normal_graph(ora)
    rng = np.random.default_rng(1000 + k)
    X = rng.standard_normal((N, k)) * np.exp(rng.uniform(-8.0, 8.0, (N, k)))
    _ready(sa, ora, ctx, k, G)
    Y = _conv(ctx, X)
    ld = np.longdouble
    ref = np.zeros((N, k), dtype=ld)
    mag = np.zeros((N, k), dtype=ld)
    Xl, vl = X.astype(ld), G.x.astype(ld)
    for c in range(N):
        s = slice(G.p[c], G.p[c + 1])
        if s.stop > s.start:
            terms = vl[s, None] * Xl[G.i[s]]
            ref[c] = np.add.reduce(terms, axis=0)
            mag[c] = np.add.reduce(np.abs(terms), axis=0)
    d = np.diff(G.p).astype(ld)[:, None]
    bound = (d + 2) * ld(2.0) ** -53 * mag
    err = np.abs(Y.astype(ld) - ref)
    assert np.all(np.isfinite(Y))
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print("\nk = %d: largest |Y - ref| / bound = %.3f" % (k, ratio))
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, "k = %d: %d elements beyond the bound, first at (column %d, factor %d): error %.3e, bound %.3e" % (
        k, len(bad), bad[0][0], bad[0][1], float(err[tuple(bad[0])]), float(bound[tuple(bad[0])]))
    assert np.array_equal(_conv(ctx, X), Y)


@pytest.mark.parametrize("k", [7, 50, 129, 514])
def test_graph_conv_unit_self_loops_reproduce_x(sa, ora, ctx, k):
    """1.0 * x + 0 is exact: on the identity graph Y is X, bit for bit (the kernel's header comment promises it)."""
    rng = np.random.default_rng(k)
    X = rng.standard_normal((N, k)) * np.exp(rng.uniform(-8.0, 8.0, (N, k)))
    _ready(sa, ora, ctx, k, gr.identity_graph(ora, N))
    assert np.array_equal(_conv(ctx, X), X)


def test_op_refusals(sa, ora):
    """No fit, no graph, a k that is not the fit's, and a team rank's context are errors with a message; the context works
    afterwards, and the operator leaves the fit's factors alone."""
    k = 6
    A, G = _matrix(ora), _exact_graph(ora)
    w0 = ora.synth_winit(k, A.nrow)
    X = _exact_x(k)
    Err = sa.SingletHipError

    def refused(fn, words):
        with pytest.raises(Err) as e:
            fn()
        assert words in str(e.value), str(e.value)

    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A))
        refused(lambda: c.op_graph_conv(X), "no fit")
        c.fit_init(k, w0)
        refused(lambda: c.op_graph_conv(X), "no cell graph")
        c.set_graph(to_dgc(sa, G))
        refused(lambda: c.op_graph_conv(_exact_x(k + 1)), "rank %d" % k)
        refused(lambda: c.op_graph_conv(_exact_x(k - 1)), "rank %d" % k)
        with pytest.raises(ValueError):
            c.op_graph_conv(X[:-1])
        before = c.get_factors()
        Y = _conv(c, X)
        assert np.array_equal(Y, _exact_reference(G, k) / 8.0)
        assert all(np.array_equal(u, v) for u, v in zip(before, c.get_factors()))
        # the graph's own buffer is not used either: a fit after the call is the fit without it
        c.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        after = c.get_factors()
        c.fit_init(k, w0)
        c.set_graph(to_dgc(sa, G))
        c.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        assert all(np.array_equal(u, v) for u, v in zip(after, c.get_factors()))
    with sa.Multi([0, 0]) as M:
        M.upload(to_dgc(sa, A))
        M.fit_init(k, w0)
        M.set_graph(to_dgc(sa, G))
        r0 = M.rank_ctx(0)
        refused(lambda: r0.op_graph_conv(_exact_x(k)[:r0.dims()[1]]), "team")
        M.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)
