"""The iteration's one pass over H for scale and Gram (k_scale_gram) and the parallel scan of the NNLS packing order.

Inside sgl_iterate_shard the plain fit scales H and forms the Gram of the scaled H in ONE kernel, and hands that Gram from
the scale step to the W step; the public step entries (step_scale_h, step_w) keep the separate kernels.  The fused pass
makes the same divisions and the same MFMAs in the same order as the two kernels it replaces, so the two arms are compared
BYTE FOR BYTE -- W, d, H and every tol -- with no tolerance:

  1. nmf_iterate against step_begin / step_h / step_scale_h / step_w / step_scale_w, three iterations, genes = 300, over
     cells (fewer columns than a wave's four, than a block's sixteen, a ragged last step, several blocks with a short last
     one) x k (every tile count NT = 1 .. 4 and its row padding); k = 80 and 130 take the unfused path; one case with an
     all-reduce hook (the local Gram goes through the second all-reduce), one on a caller's stream;
  2. c_nmf against the CPU oracle at two of those shapes, at the tolerance of tests/test_gpu_nmf.py;
  3. the packing order of the H-side solve (from 65 536 columns on): factors and sweep totals of two iterations against
     the same fit with SGL_NNLS_NO_PACK=1, which a child process runs (one child for all sizes).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import to_dgc
from test_gpu_nmf import TOL, _check

pytestmark = pytest.mark.gpu
GENES = 300
L1 = 0.01
CELLS = (1, 3, 15, 16, 17, 255, 257, 4099)
RANKS = (1, 2, 15, 16, 17, 32, 33, 48, 49, 50, 63, 64)
PACK_CELLS = (65536, 65537, 70001, 200000)
PACK_K = 10


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def pair(sa):
    """Two contexts: the iteration and the step API."""
    a, b = sa.Context(0), sa.Context(0)
    yield a, b
    a.close()
    b.close()


def start(c, cells, k):
    c.synth(GENES, cells, 20)
    c.fit_init(k)


def by_iterate(c, n=3):
    return [c.nmf_iterate(L1, L1, 0.0, 0.0) for _ in range(n)]


def by_steps(c, n=3):
    tols = []
    for _ in range(n):
        c.step_begin()
        c.step_h(L1, 0.0)
        c.step_scale_h()
        c.step_w(L1, 0.0)
        tols.append(c.step_scale_w())
    return tols


def assert_same_bits(a, b, tols_a, tols_b):
    for name, x, y in zip("WdH", a.get_factors(), b.get_factors()):
        assert x.shape == y.shape and bits(x) == bits(y), name
    assert bits(tols_a) == bits(tols_b), (tols_a, tols_b)


@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("cells", CELLS)
def test_iteration_is_the_step_api_bit_for_bit(pair, cells, k):
    a, b = pair
    start(a, cells, k)
    start(b, cells, k)
    assert_same_bits(a, b, by_iterate(a), by_steps(b))


@pytest.mark.parametrize("k", [80, 130])
def test_ranks_above_64_take_the_separate_kernels(pair, k):
    a, b = pair
    start(a, 4099, k)
    start(b, 4099, k)
    assert_same_bits(a, b, by_iterate(a), by_steps(b))


def test_with_an_allreduce_hook(pair):
    """One rank: the identity is the all-reduce.  The fused pass comes after the all-reduce of d, its local Gram goes
    behind the right-hand sides before the second one."""
    a, b = pair
    calls = []
    try:
        a.set_allreduce(lambda dev_ptr, count: calls.append(count))
        b.set_allreduce(lambda dev_ptr, count: None)
        start(a, 4099, 50)
        start(b, 4099, 50)
        assert_same_bits(a, b, by_iterate(a), by_steps(b))
        # d, then right-hand sides and Gram together, every iteration (and the gene counts once)
        assert [n for n in calls if n != GENES] == [50, 50 * GENES + 50 * 50] * 3
    finally:
        a.set_allreduce(None)
        b.set_allreduce(None)


def test_on_a_callers_stream(pair):
    a, b = pair
    hip = ctypes.CDLL("libamdhip64.so")
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        a.set_stream(s.value)
        b.set_stream(s.value)
        start(a, 4099, 50)
        start(b, 4099, 50)
        assert_same_bits(a, b, by_iterate(a), by_steps(b))
    finally:
        a.set_stream(None)
        b.set_stream(None)
        assert hip.hipStreamDestroy(s) == 0


@pytest.mark.parametrize("n,k", [(257, 33), (4099, 50)])
def test_c_nmf_against_the_oracle(sa, ora, n, k):
    A = ora.synth_csc(GENES, n, 20)
    At = A.t()
    w0 = ora.synth_winit(k, GENES)
    ref = ora.c_nmf(A, At, 0.0, 3, L1, L1, 0.0, 0.0, 0, w0)
    got = sa.c_nmf(to_dgc(sa, A), to_dgc(sa, At), 0.0, 3, False, L1, L1, 0.0, 0.0, 0, w0.T)
    assert TOL == 1e-9
    _check(got, ref)
    assert got["iter"] == ref["iter"] == 3
    assert np.allclose(got["tol"], ref["tol"], rtol=1e-8, atol=0)


# ------------------------------------------------------------------------------------------------------ the pack scan --
def pack_fit(c, cells):
    """Two iterations at k = 10: the second H solve takes its columns in the order the scan laid out."""
    c.synth(GENES, cells, 20)
    c.fit_init(PACK_K)
    c.sweeps_get(reset=True)
    tols = by_iterate(c, 2)
    sw = c.sweeps_get(reset=True)
    W, d, H = c.get_factors()
    return dict(W=W, d=d, H=H, tol=np.array(tols), sweeps=np.array([sw["h_sweeps"], sw["w_sweeps"]], dtype=np.int64))


@pytest.fixture(scope="module")
def unpacked(sa, tmp_path_factory):
    """The same fits with SGL_NNLS_NO_PACK=1, from a child process (this file as a script)."""
    out = str(tmp_path_factory.mktemp("nopack") / "nopack.npz")
    env = dict(os.environ, SGL_NNLS_NO_PACK="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=600)
    with np.load(out) as z:
        return {key: z[key] for key in z.files}


@pytest.mark.parametrize("cells", PACK_CELLS)
def test_pack_scan_leaves_the_fit_bit_identical(pair, unpacked, cells):
    assert "SGL_NNLS_NO_PACK" not in os.environ
    got = pack_fit(pair[0], cells)
    for key in ("W", "d", "H", "tol"):
        assert bits(got[key]) == bits(unpacked["%s_%d" % (key, cells)]), key
    assert np.array_equal(got["sweeps"], unpacked["sweeps_%d" % cells])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import singlet_amd

    assert os.environ.get("SGL_NNLS_NO_PACK") == "1"
    ctx = singlet_amd.Context(0)
    res = {}
    for n_cells in PACK_CELLS:
        for key, val in pack_fit(ctx, n_cells).items():
            res["%s_%d" % (key, n_cells)] = val
    ctx.close()
    np.savez(sys.argv[1], **res)
