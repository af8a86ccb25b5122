"""The rules of sgl_variable_features (include/singlet_hip.h) restated in numpy, operation by operation; no device.

The gene side of a matrix is (x, p, n): the stored values of t(A) gene after gene (ascending cell inside a gene), the
m + 1 offsets, and the number of cells.  c_g = p[g + 1] - p[g], explicit zeros included.

THE SUMMATION ORDER, as the header states it.  A gene's terms, in stored order, are cut into segments of SEG = 8192;
inside a segment lane l of 64 adds the terms l, l + 64, ... in that order from +0.0, the 64 lane sums are added by a
butterfly (v += v[lane ^ 32], then 16, 8, 4, 2, 1); the segment sums are added in segment order from +0.0.  The moment
sums of the trend use the same lanes and butterfly over the whole window (no segments).

Three arithmetics of the three gene stages: float64 in that order (*_f64: bit-comparable with the device), exact
(*_exact: fractions.Fraction, rounded once at the end) and np.longdouble (*_ld); the trend in float64 -- in the stated
lanes or with numpy's pairwise sums -- and in longdouble; the composite in float64.  The window, the bandwidth's
positivity test and the degree of the longdouble trend follow the float64 rule (they are comparisons the rule defines
on doubles); its arithmetic is longdouble throughout.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SEG = 8192
LANES = 64
LD = np.longdouble
_BUTTERFLY = [np.arange(LANES) ^ off for off in (32, 16, 8, 4, 2, 1)]


# ------------------------------------------------------------------------------------------------------------- layout --
def gene_side(x, i, p, nrow):
    """(x, p) of t(A) from the CSC image (x, i, p) of A: a stable sort by row keeps the cells ascending inside a gene."""
    x, i = np.asarray(x, dtype=np.float64), np.asarray(i)
    order = np.argsort(i, kind="stable")
    counts = np.bincount(i, minlength=nrow).astype(np.int64)
    return x[order], np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def csc_of_triplets(genes, cells, values, nrow, ncol):
    """CSC image (x, i, p) of the entries given (explicit zeros stay stored); one entry per (gene, cell)."""
    genes, cells, values = np.asarray(genes), np.asarray(cells), np.asarray(values, dtype=np.float64)
    order = np.lexsort((genes, cells))
    p = np.concatenate(([0], np.cumsum(np.bincount(cells, minlength=ncol)))).astype(np.int32)
    return values[order], genes[order].astype(np.int32), p


def _rows(x, p):
    return [x[p[g]:p[g + 1]] for g in range(len(p) - 1)]


# ------------------------------------------------------------------------------------------------------ stated order --
def lane_sum(t):
    """Sum of the terms t (n,) or (k, n) of one segment or window in the stated lanes: lane l adds the terms l, l + 64, ...
    in that order from +0.0, then the butterfly.  (A lane that runs out adds nothing; here it adds +0.0, which changes no
    sum that started at +0.0.)"""
    t = np.atleast_2d(np.asarray(t, dtype=np.float64))
    k, n = t.shape
    rounds = -(-n // LANES)
    pad = np.zeros((k, rounds * LANES))
    pad[:, :n] = t
    pad = pad.reshape(k, rounds, LANES)
    acc = np.zeros((k, LANES))
    for r in range(rounds):
        acc = acc + pad[:, r, :]
    for ix in _BUTTERFLY:
        acc = acc + acc[:, ix]
    return acc[:, 0]


def gene_sum(t):
    """The stated sum of one gene's terms: segments of SEG through lane_sum, added in segment order from +0.0."""
    s = np.float64(0.0)
    for a in range(0, t.shape[0], SEG):
        s = s + lane_sum(t[a:a + SEG])[0]
    return s


# ------------------------------------------------------------------------------------------------------------ float64 --
def mean_f64(x, p, n):
    rows = _rows(x, p)
    with np.errstate(all="ignore"):
        mean = np.array([gene_sum(r) / np.float64(n) for r in rows], dtype=np.float64).reshape(-1)
    return mean, np.diff(p).astype(np.int64)


def var_f64(x, p, n, mu):
    out = np.empty(len(p) - 1)
    with np.errstate(all="ignore"):
        for g, r in enumerate(_rows(x, p)):
            m = np.float64(mu[g])
            d = r - m
            q = gene_sum(d * d)
            z = np.float64(n - r.shape[0]) * (m * m)
            out[g] = (q + z) / np.float64(n - 1)
    return out


def var_std_f64(x, p, n, mu, sd, vmax):
    out = np.empty(len(p) - 1)
    vmax = np.float64(vmax)
    with np.errstate(all="ignore"):
        for g, r in enumerate(_rows(x, p)):
            m, s = np.float64(mu[g]), np.float64(sd[g])
            if s == 0.0:
                out[g] = 0.0
                continue
            z = (r - m) / s
            z = np.where(z > vmax, vmax, z)
            q = gene_sum(z * z)
            z0 = (np.float64(0.0) - m) / s
            out[g] = (q + np.float64(n - r.shape[0]) * (z0 * z0)) / np.float64(n - 1)
    return out


# -------------------------------------------------------------------------------------------------------------- exact --
def _F(v):
    return Fraction(float(v))


def mean_exact(x, p, n):
    return np.array([float(sum((_F(v) for v in r), Fraction(0)) / n) for r in _rows(x, p)])


def var_exact(x, p, n, mu):
    out = []
    for g, r in enumerate(_rows(x, p)):
        m = _F(mu[g])
        q = sum(((_F(v) - m) ** 2 for v in r), Fraction(0))
        out.append(float((q + (n - len(r)) * m * m) / (n - 1)))
    return np.array(out)


def var_std_exact(x, p, n, mu, sd, vmax):
    out, vm = [], _F(vmax)
    for g, r in enumerate(_rows(x, p)):
        m, s = _F(mu[g]), _F(sd[g])
        if s == 0:
            out.append(0.0)
            continue
        q = sum((min((_F(v) - m) / s, vm) ** 2 for v in r), Fraction(0))
        z0 = (0 - m) / s
        out.append(float((q + (n - len(r)) * z0 * z0) / (n - 1)))
    return np.array(out)


# --------------------------------------------------------------------------------------------------------- longdouble --
def mean_ld(x, p, n):
    return np.array([np.sum(r.astype(LD)) / LD(n) for r in _rows(x, p)], dtype=LD)


def var_ld(x, p, n, mu):
    out = np.empty(len(p) - 1, dtype=LD)
    for g, r in enumerate(_rows(x, p)):
        m = LD(mu[g])
        d = r.astype(LD) - m
        out[g] = (np.sum(d * d) + LD(n - r.shape[0]) * (m * m)) / LD(n - 1)
    return out


def var_std_ld(x, p, n, mu, sd, vmax):
    out = np.empty(len(p) - 1, dtype=LD)
    for g, r in enumerate(_rows(x, p)):
        m, s = LD(mu[g]), LD(sd[g])
        if s == 0:
            out[g] = 0
            continue
        z = np.minimum((r.astype(LD) - m) / s, LD(vmax))
        z0 = (LD(0) - m) / s
        out[g] = (np.sum(z * z) + LD(n - r.shape[0]) * (z0 * z0)) / LD(n - 1)
    return out


# -------------------------------------------------------------------------------------------------------------- trend --
def loess_window(x, i, q):
    """(start, hmax) of the window of point i: the q consecutive sorted positions containing i whose farthest member is
    nearest, ties to the lowest start (np.argmin returns the first minimum); float64, as the rule is defined."""
    n = x.shape[0]
    s = np.arange(max(0, i - q + 1), min(i, n - q) + 1)
    f = np.maximum(x[i] - x[s], x[s + q - 1] - x[i])
    k = int(np.argmin(f))
    return int(s[k]), np.float64(f[k])


def _degree(xw, xi, hmax):
    """Distinct x among the members of positive weight (hmax == 0 or |x - x_i| < hmax), at most 3."""
    pos = np.ones(xw.shape[0], dtype=bool) if hmax == 0.0 else np.abs(xw - xi) < hmax
    fresh = pos.copy()
    fresh[1:] &= (xw[1:] != xw[:-1]) | ~pos[:-1]
    return min(int(fresh.sum()), 3)


def _solve(S0, S1, S2, S3, S4, T0, T1, T2, distinct):
    if distinct >= 3:
        A = S2 * S4 - S3 * S3
        num = (T0 * A - S1 * (T1 * S4 - S3 * T2)) + S2 * (T1 * S3 - S2 * T2)
        den = (S0 * A - S1 * (S1 * S4 - S3 * S2)) + S2 * (S1 * S3 - S2 * S2)
        return num / den
    if distinct == 2:
        return (S2 * T0 - S1 * T1) / (S0 * S2 - S1 * S1)
    return T0 / S0


def loess_f64(x, y, q, order="lanes"):
    """The direct trend in float64; order "lanes": the stated lanes and butterfly, "pairwise": numpy's sum."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.empty(x.shape[0])
    for i in range(x.shape[0]):
        s0, hmax = loess_window(x, i, q)
        xw, yw = x[s0:s0 + q], y[s0:s0 + q]
        u = xw - x[i]
        if hmax != 0.0:
            r = np.abs(u) / hmax
            c = 1.0 - (r * r) * r
            w = (c * c) * c
        else:
            w = np.ones(q)
        wu = w * u
        wu2 = wu * u
        wu3 = wu2 * u
        wu4 = wu3 * u
        terms = np.stack([w, wu, wu2, wu3, wu4, w * yw, wu * yw, wu2 * yw])
        sums = lane_sum(terms) if order == "lanes" else np.array([np.sum(t) for t in terms])
        with np.errstate(all="ignore"):
            out[i] = _solve(*sums, _degree(xw, x[i], hmax))
    return out


def loess_ld(x, y, q):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.empty(x.shape[0], dtype=LD)
    for i in range(x.shape[0]):
        s0, hmax = loess_window(x, i, q)
        distinct = _degree(x[s0:s0 + q], x[i], hmax)
        xw, yw, xi = x[s0:s0 + q].astype(LD), y[s0:s0 + q].astype(LD), LD(x[i])
        u = xw - xi
        h = max(xi - xw[0], xw[-1] - xi)
        if hmax != 0.0:
            r = np.abs(u) / h
            c = 1 - r * r * r
            w = c * c * c
        else:
            w = np.ones(q, dtype=LD)
        sums = [np.sum(t) for t in (w, w * u, w * u * u, w * u ** 3, w * u ** 4, w * yw, w * u * yw, w * u * u * yw)]
        out[i] = _solve(*sums, distinct)
    return out


def trend_tolerance(x, y, q, factor=16):
    """The tolerance of a device trend against loess_ld on these inputs: `factor` times the larger of the float64
    restatement's largest deviations from it in the stated lanes and in numpy's pairwise order.  Returns (tolerance,
    longdouble trend, deviation in the stated lanes, deviation pairwise)."""
    ld = loess_ld(x, y, q)
    dev = [float(np.max(np.abs(loess_f64(x, y, q, o).astype(LD) - ld))) for o in ("lanes", "pairwise")]
    return factor * max(dev), ld, dev[0], dev[1]


# ---------------------------------------------------------------------------------------------------------- composite --
def window_length(m_live, span):
    return max(min(m_live, 3), int(np.floor(span * m_live)))


def variable_features(x, p, n, nfeatures, span=0.3, vmax=None, expected_var=None):
    m = len(p) - 1
    mean, count = mean_f64(x, p, n)
    var = var_f64(x, p, n, mean)
    live = np.flatnonzero(var > 0)
    trend = None
    if expected_var is not None:
        expd = np.asarray(expected_var, dtype=np.float64).copy()
    else:
        expd = np.zeros(m)
        if live.size:
            lx, ly = np.log10(mean[live]), np.log10(var[live])
            order = np.lexsort((live, lx))
            q = window_length(live.size, span)
            fit = loess_f64(lx[order], ly[order], q)
            expd[live[order]] = np.power(10.0, fit)
            trend = (lx[order], ly[order], q)
    sd = np.sqrt(expd)
    vm = np.sqrt(np.float64(n)) if vmax is None or not vmax > 0 else np.float64(vmax)
    std = var_std_f64(x, p, n, mean, sd, vm)
    key = np.where(np.isnan(std), -np.inf, std)
    rank = np.argsort(-key, kind="stable")   # descending, ties to the lower gene index
    return {"features": rank[:min(nfeatures, m)].astype(np.int32), "mean": mean, "count": count, "variance": var,
            "variance_expected": expd, "variance_standardized": std, "sd": sd, "vmax": vm, "rank": rank, "trend": trend}


def rank_gaps(std, rank, nfeatures):
    """Relative differences of the adjacent pairs among the first nfeatures + 1 ranked standardised variances."""
    v = std[rank[:nfeatures + 1]]
    return (v[:-1] - v[1:]) / np.abs(v[:-1])


# -------------------------------------------------------------------------------------------------------------- inputs --
EXACT_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


def exact_gate_matrix(n, seed=0):
    """Counts 0..7 over n cells (n a power of two), as triplets: genes of c_g = 0, 1, 63, ... (those below n) and n, one
    gene whose only entry is an explicit zero, one gene for the clip (values 1, 2 and 7), 12 genes with about a quarter
    stored.  Returns (x, i, p, nrow, names): names[g] says what gene g is there for."""
    rng = np.random.default_rng(seed + n)
    genes, cells, vals, names = [], [], [], []

    def add(where, v, name):
        g = len(names)
        names.append(name)
        genes.extend([g] * len(where))
        cells.extend(int(c) for c in where)
        vals.extend(float(q) for q in v)

    for c in [q for q in EXACT_COUNTS if q < n] + [n]:
        where = np.sort(rng.choice(n, c, replace=False))
        add(where, rng.integers(1, 8, c), "c=%d" % c)
    add([n // 3], [0.0], "explicit zero")
    where = np.sort(rng.choice(n, n // 4, replace=False))
    add(where, rng.choice([1, 2, 7], n // 4), "clip")
    for r in range(12):
        where = np.flatnonzero(rng.random(n) < 0.25)
        add(where, rng.integers(0, 8, where.size), "random %d" % r)   # (a drawn 0 is another explicit zero)
    nrow = len(names)
    x, i, p = csc_of_triplets(genes, cells, vals, nrow, n)
    return x, i, p, nrow, names


def segment_matrix(seed=0):
    """8 genes x (2 SEG + 1) cells of counts 1..7: c_g = SEG - 1, SEG, SEG + 1, 2 SEG + 1 and four sparse genes."""
    n = 2 * SEG + 1
    rng = np.random.default_rng(seed + 77)
    genes, cells, vals = [], [], []
    for g, c in enumerate((SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 0, 3, 100, 700)):
        where = np.sort(rng.choice(n, c, replace=False))
        genes.extend([g] * c)
        cells.extend(int(q) for q in where)
        vals.extend(float(q) for q in rng.integers(1, 8, c))
    x, i, p = csc_of_triplets(genes, cells, vals, 8, n)
    return x, i, p, 8, n


TREND_SIZES = (1, 2, 3, 4, 50, 257, 2000)
TREND_SPANS = (0.3, 1.0)


def trend_inputs(m):
    """Sorted x with runs of equal values and a smooth y with noise: a third of the points share the smallest x (as the
    genes seen once all do) -- from 50 points on that run fills whole windows at span 0.3 (windows that are one value) --
    and a second run of q - 1 points a little above it, whose windows reach into the first run or past its own end
    (windows of exactly two values; members at the bandwidth itself, which weigh nothing); the last q - 1 points hold
    two values only, which leaves their windows two values of positive weight."""
    rng = np.random.default_rng(1000 + m)
    x = np.sort(rng.uniform(-3.0, 1.0, m))
    x[:m // 3] = x[0] if m else 0.0
    if m >= 50:
        q = window_length(m, 0.3)
        x[m // 3:m // 3 + q - 1] = x[0] + 1e-3
        # the last q - 1 points are two values, so their windows take in the point before them, which alone is farthest:
        # two values of positive weight, a straight line
        a = x[m - q] + 0.3
        x[m - q + 1:m - q + 4] = a
        x[m - q + 4:] = a + 0.01
        assert np.all(np.diff(x) >= 0)
    y = 0.3 * x * x + 1.2 * x + 0.5 + 0.1 * rng.standard_normal(m)
    return x, y


def trend_windows(x, q):
    """Per point: (distinct x in the window, distinct x of positive weight capped at 3) -- what the not-gpu test counts."""
    out = []
    for i in range(x.shape[0]):
        s0, hmax = loess_window(x, i, q)
        xw = x[s0:s0 + q]
        out.append((int(np.unique(xw).size), _degree(xw, x[i], hmax)))
    return out


def count_matrix(m, n, seed, planted=0.3):
    """Integer counts, genes x cells, as a dense array: negative-binomial-like genes over a wide range of means, three in ten
    of them over-dispersed (the planted set, more than any nfeatures the tests ask for), a few constant and a few all-zero genes."""
    rng = np.random.default_rng(seed)
    mu = np.exp(rng.uniform(np.log(0.2), np.log(20.0), m))
    disp = np.where(rng.random(m) < planted, rng.uniform(2.0, 8.0, m), rng.uniform(0.05, 0.3, m))
    lam = mu[:, None] * rng.gamma(1.0 / disp[:, None], disp[:, None], (m, n))
    D = rng.poisson(lam).astype(np.float64)
    D[3, :] = 0.0
    D[m - 2, :] = 2.0
    D[m // 2, :] = 0.0
    return D


# the composite cases of the device test: (genes, cells, seed, nfeatures); the seeds were found with the not-gpu test, which
# holds them to the condition that no two of the first nfeatures + 1 ranked values lie within 1e-9 of each other
COMPOSITE_CASES = [(300, 1024, 5, 50), (2000, 700, 1, 200)]


def csc_of_dense(D):
    genes, cells = np.nonzero(D)
    return csc_of_triplets(genes, cells, D[genes, cells], D.shape[0], D.shape[1])
