"""The decision rule of the bounded-tol NNLS (kernels_nnls_asm_bounded.hip, gen_nnls_lane.py), without a GPU.

The bounded sweep's running tol S lies within a relative delta of the exact kernel's T.  The kernel runs the exact, correctly
rounded stop test `tol / k > 1e-8` on lo = S (1 - delta) and hi = S (1 + delta), both formed by one FMA: where the two agree that
must be the exact kernel's decision on T, whatever S is inside its band; where they differ the column is solved again exactly."""
import numpy as np
import pytest

from test_generated_asm_on_cpu import _fma, _load


def two_sided(S, k, dlt):
    """(lo says go, hi says go) as the kernel body computes them: S (1 -+ delta) by one FMA each, then the correctly rounded
    quotient by k (sgl_div_normal: an IEEE division for these operands) against 1e-8"""
    lo, hi = _fma(-S, dlt, S), _fma(S, dlt, S)
    return lo / float(k) > 1e-8, hi / float(k) > 1e-8


@pytest.mark.parametrize("k", [5, 6, 19, 20, 49, 50])
def test_agreeing_ends_decide_like_the_exact_test(k):
    gen = _load("gen_nnls_lane")
    dlt = gen.band((k + 1) // 2 * 2)
    rng = np.random.default_rng(4100 + k)
    thr = 1e-8 * k
    n, agree, taint = 60000, 0, 0
    # T within a few delta of the threshold (both sides, and a share at the doubles next to it), S anywhere in T's band
    T = thr * (1.0 + dlt * rng.uniform(-4.0, 4.0, n))
    near = np.nextafter(thr, np.where(rng.random(64) < 0.5, 0.0, 1.0))
    for _ in range(3):
        near = np.concatenate([near, np.nextafter(near, 0.0), np.nextafter(near, 1.0)])
    T[:near.size] = near
    # the proven relation is |S - T| <= delta / 2 * T; the rule is held to the whole band in which lo < T < hi holds, |S - T| < delta * T / (1 + delta)
    # (S (1 - delta) < T < S (1 + delta) in exact arithmetic), less the FMA's half ulp at its edges
    u = rng.uniform(-1.0, 1.0, n)
    u[: n // 8] = np.sign(u[: n // 8])           # the edges of the band themselves
    S = T * (1.0 + u * dlt * (1.0 - 2.0 ** -20) / (1.0 + dlt))
    for t, s in zip(T, S):
        glo, ghi = two_sided(float(s), k, dlt)
        exact = float(t) / float(k) > 1e-8
        if glo == ghi:
            agree += 1
            assert glo == exact, (t, s, glo, ghi, exact)
        else:
            taint += 1
            assert ghi and not glo
    assert agree > 0 and taint > 0      # both outcomes occur this close to the threshold


def test_far_from_the_threshold_nothing_taints():
    gen = _load("gen_nnls_lane")
    k = 50
    dlt = gen.band(k)
    for S in (0.0, 1e-300, 1e-9 * k, 1e-8 * k * (1 - 3 * dlt), 1e-8 * k * (1 + 3 * dlt), 1e-3, 1.0, 7.5, 1e300):
        glo, ghi = two_sided(S, k, dlt)
        assert glo == ghi == (S / float(k) > 1e-8), S
    assert two_sided(1.0, k, 0.5) == (True, True)   # a fresh column (tol = 1) starts even in the widest band the tests use


def test_band_is_the_derived_bound():
    gen = _load("gen_nnls_lane")
    for KP in (2, 6, 20, 50):
        assert gen.band(KP) == 2.0 * (2.0 ** -26 + (KP + 4) * 2.0 ** -52)
        assert gen.band(KP) < 3.1e-8
