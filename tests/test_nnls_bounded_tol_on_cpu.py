"""The bounded-tol sweep of gen_nnls_lane.py (Sweep(KP, bounded=True)) executed WITHOUT a GPU, by the interpreter of
test_generated_asm_on_cpu.py with a v_rcp_f64 that is as inexact as the hardware's may be: every result perturbed by a relative
error of up to eps_r = 2^-13 (all up, all down, random).  A Python loop plays the kernel body around the sweep -- the two-sided
stop test of test_nnls_bounded_tol_rule.py, the gates, L1G, tol.  Columns the rule decides must match the oracle's nnls like the
exact sweep does (same sweep counts, same zero pattern, 1e-9); columns it cannot decide are tainted, which is all this level has
to show of them (the kernel then solves them again exactly: tests/test_gpu_nnls_bounded_tol.py)."""
import numpy as np
import pytest

from test_generated_asm_on_cpu import Machine, _check, _load, _padded, _problem
from test_nnls_bounded_tol_rule import two_sided

EPS_R = 2.0 ** -13


class InexactRcpMachine(Machine):
    """v_rcp_f64 returns (1 / x) (1 + e), |e| <= eps_r: mode '+', '-' or 'random'"""

    def __init__(self, lanes, lds, ops, mode, seed):
        super().__init__(lanes, lds, ops)
        self.mode = mode
        self.rng = np.random.default_rng(seed)

    def run(self, ins):
        op, _, rest = ins.partition(" ")
        if op != "v_rcp_f64":
            return super().run(ins)
        a = [t.strip() for t in rest.split(",")]
        for lane in self.lanes:
            e = {"+": EPS_R, "-": -EPS_R}.get(self.mode)
            if e is None:
                e = float(self.rng.uniform(-EPS_R, EPS_R))
            self.wr64(self.vreg(a[0]), lane, (1.0 / self.src64(a[1], lane)) * (1.0 + e))


def _gradual_problem(k, ncols, seed, L1):
    """Columns whose tol falls by a factor of 2 per sweep, exactly: the Gram is block diagonal, 2 x 2 blocks [[1, a], [a, 1]] with
    a^2 = 1 / 2 (and a single 1 for the last coordinate of an odd k), b = G x* + L1 diag(G) with x* in [0.5, 1.5], x0 = 0.  The
    penalised solution is x* (the step b_i / G_ii - L1 vanishes there), and a sweep is a Gauss-Seidel step of each block:
    x1 <- x1* - a e2, x2 <- x2* + a^2 e2 with e2 = x2 - x2*, so e2 shrinks by a^2 per sweep from (1 - a^2) x2* - x2* < 0 on: every
    iterate is positive (no clamp, no reset of tol), the steps and with them tol = sum |step / x| are geometric with ratio a^2 up
    to the drift of the denominators, which is of the size of e2 / x* -- below 1e-6 once tol is near the threshold 1e-8 k."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(0.5)
    G = np.eye(k)
    for j in range(0, k - 1, 2):
        G[j, j + 1] = G[j + 1, j] = a
    xs = rng.uniform(0.5, 1.5, size=(ncols, k))
    return G, xs @ G + L1 * np.diag(G), np.zeros((ncols, k))


def _run_bounded(ora, k, L1, mode, dlt=None, ncols=3, problem=_problem):
    gen = _load("gen_nnls_lane")
    KP = (k + 1) // 2 * 2
    s = gen.Sweep(KP, bounded=True)
    sweep = list(s.build())
    dlt = gen.band(KP) if dlt is None else dlt
    NGP = s.NGP
    G, B, X0 = problem(k, ncols, 700 + k, L1)
    Gp, rd = _padded(G, k, KP)
    row = 16 * NGP
    lds = np.zeros(KP * row + 2 * KP)
    for i in range(KP):
        for l in range(16):
            for mm in range(s.NG):
                j = l + 16 * mm
                lds[i * row + l * NGP + mm] = Gp[i, j] if j < KP else 0.0
    lds[KP * row::2] = np.diag(Gp)
    lds[KP * row + 1::2] = rd
    lanes = list(range(ncols))
    gl = np.array([(lane & 15) * NGP * 8 for lane in range(64)], dtype=np.uint32)
    m = InexactRcpMachine(lanes, lds.tobytes(), {"gl": gl, "dl": KP * row * 8, "l1": L1, "eps": 1e-15, "one_hi": 0x3ff00000}, mode, 31 * k)
    for lane in lanes:
        for j in range(k):
            m.wr64(s.b(j), lane, B[lane, j])
            m.wr64(s.x(j), lane, X0[lane, j])
        m.wr64(s.TOL, lane, 1.0)
    it = {c: 0 for c in lanes}
    tainted = set()
    for _ in range(101):
        go = {}
        for c in lanes:
            glo, ghi = two_sided(m.rd64(s.TOL, c), k, dlt)
            if c not in tainted and it[c] < 100 and glo != ghi:
                tainted.add(c)
            go[c] = glo and ghi and it[c] < 100 and c not in tainted
        if not any(go.values()):
            break
        for c in lanes:
            if go[c]:
                m.wr64(s.TOL, c, 0.0)
            m.wr64(s.GM, c, 1.0 if go[c] else 0.0)
            m.wr64(s.L1G, c, L1 * (1.0 if go[c] else 0.0))
        for ins in sweep:
            m.run(ins)
        for c in lanes:
            it[c] += 1 if go[c] else 0
    res = {c: (np.array([m.rd64(s.x(j), c) for j in range(k)]), it[c]) for c in lanes if c not in tainted}
    return res, tainted, (G, B, X0)


@pytest.mark.parametrize("mode", ["+", "-", "random"])
@pytest.mark.parametrize("k,L1", [(5, 0.0), (6, 0.02), (19, 0.0), (50, 0.02)])
def test_bounded_sweep_solves_like_the_oracle(ora, k, L1, mode):
    ncols = 3 if k < 40 else 2
    res, tainted, (G, B, X0) = _run_bounded(ora, k, L1, mode, ncols=ncols)
    assert len(res) + len(tainted) == ncols
    print("k = %d, rcp %s: %d of %d columns tainted" % (k, mode, len(tainted), ncols))   # (the default band is a few 1e-8 wide)
    _check(res, ora, G, B, X0, L1, 0.0)


@pytest.mark.parametrize("L1", [0.0, 0.02])
@pytest.mark.parametrize("k", [5, 6, 19, 50])
def test_widest_band_taints_every_column(ora, k, L1):
    """With delta = 0.5 the stop test is undecided for S in (1e-8 k / 1.5, 1e-8 k / 0.5], a band whose ends are a factor of 3
    apart.  A column taints there unless one sweep takes its tol across the whole band -- so the statement "every column taints"
    is one about columns that approach the threshold gradually, and it is checked on columns that do so by construction
    (_gradual_problem: tol halves with every sweep, 2 < 3, so some stop test must find S inside the band; about 27 sweeps, far
    from the limit of 100).  Columns that reach their fixed point in a sweep or two end on S = 0 exactly, which is the exact
    tol as well: they are decided without a redo, rightly (the test below)."""
    ncols = 3 if k < 40 else 2
    res, tainted, _ = _run_bounded(ora, k, L1, "random", dlt=0.5, ncols=ncols, problem=_gradual_problem)
    assert not res and len(tainted) == ncols


@pytest.mark.parametrize("k,L1", [(5, 0.0), (6, 0.02)])
def test_widest_band_decides_a_column_only_where_the_exact_kernel_agrees(ora, k, L1):
    """The same band on the general columns of the first test: whatever is NOT tainted in a band this wide was decided by the
    rule at every stop test, and must be the oracle's solution with the oracle's sweep count all the same.  (At these small ranks
    some columns sit at their fixed point after a few sweeps -- tol = 0 exactly in either kernel -- and jump over the band.)"""
    res, tainted, (G, B, X0) = _run_bounded(ora, k, L1, "random", dlt=0.5, ncols=3)
    assert len(res) + len(tainted) == 3
    _check(res, ora, G, B, X0, L1, 0.0)


def _fp64_chain(sweep):
    """the FP64-rate instructions of a sweep that are not row-update FMAs"""
    return [i for i in sweep if i.startswith(("v_mul_f64", "v_add_f64", "v_fma_f64", "v_rcp_f64", "v_min_f64", "v_cmp_"))]


@pytest.mark.parametrize("KP", [6, 20, 50])
def test_bounded_coordinate_is_six_instructions_shorter(KP):
    gen = _load("gen_nnls_lane")
    exact, bounded = list(gen.Sweep(KP).build()), list(gen.Sweep(KP, bounded=True).build())
    count = lambda L: sum(1 for i in L if not i.startswith(("s_waitcnt", "s_nop")))
    assert count(bounded) < count(exact)
    assert len(_fp64_chain(exact)) - len(_fp64_chain(bounded)) == 6 * KP    # one Newton step, remainder, correction; the L2 term, the gate
    assert sum(i.startswith("v_fmac_f64_dpp") for i in bounded) == KP * KP
    # the same registers: the plan of the exact sweep, no register beyond it
    se, sb = gen.Sweep(KP), gen.Sweep(KP, bounded=True)
    assert (se.V_T, se.TOP, se.WAVES) == (sb.V_T, sb.TOP, sb.WAVES)
    assert sb.L1G + 1 < sb.V_D and len({sb.A, sb.E2, sb.ND[0], sb.ND[1], sb.DEN, sb.R, sb.L1G, sb.Q, sb.TOL, sb.GM}) == 10
