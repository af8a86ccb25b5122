"""A dense numpy restatement of the co-occurrence rules of include/singlet_hip.h, "Co-occurrence by distance": the all-pairs
d2 by the stated expression, np.searchsorted on the squared thresholds, np.add.at; both statistics; the plan's arithmetic.  numpy
rounds every elementwise operation on its own (no contraction), which is the stated d2."""
import math

import numpy as np

TILE = 256
LDS_BYTES = 128 << 10
STAGE_BYTES = 6144
MAX_WG = 1024
WG_TARGET = 2048
MAX_SPLIT = 64
EXTENT_BLOCKS = 64
FLUSH_PAIRS = (1 << 32) - 1
MAX_K = 256
MAX_T = 64
PI = float.fromhex("0x1.921fb54442d18p+1")


def thr2_of(r):
    r = np.asarray(r, dtype=np.float64)
    return r * r


def d2_block(c1, c2, rows):
    """d2[i, j] for i in rows, every j: fl(fl(dx dx) + fl(dy dy)), dx = fl(c1[i] - c1[j])."""
    with np.errstate(over="ignore"):
        dx = c1[rows, None] - c1[None, :]
        dy = c2[rows, None] - c2[None, :]
        return dx * dx + dy * dy


def tally(c1, c2, lab, K, r, block=2048):
    """N[a, b, t], int64: the ordered pairs (i, j), i != j, with thr2[t] < d2 <= thr2[t + 1]."""
    c1, c2, lab = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64), np.asarray(lab, dtype=np.int64)
    th = thr2_of(r)
    T, n = th.shape[0] - 1, c1.shape[0]
    N = np.zeros((K, K, T), dtype=np.int64)
    for i0 in range(0, n, block):
        rows = np.arange(i0, min(i0 + block, n))
        d2 = d2_block(c1, c2, rows)
        t = np.searchsorted(th, d2, side="left") - 1            # the first threshold not below d2, minus one: thr2[t] < d2 <= thr2[t + 1]
        ok = (t >= 0) & (t < T) & (rows[:, None] != np.arange(n)[None, :])
        ii, jj = np.nonzero(ok)
        np.add.at(N, (lab[rows[ii]], lab[jj], t[ii, jj]), 1)
    return N


def tally_loops(c1, c2, lab, K, r):
    """The same table by a plain triple loop over Python floats (IEEE doubles, one rounding per operation)."""
    th = [float(v) * float(v) for v in r]
    T, n = len(th) - 1, len(c1)
    N = np.zeros((K, K, T), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            dx, dy = float(c1[i]) - float(c1[j]), float(c2[i]) - float(c2[j])
            d2 = dx * dx + dy * dy
            for t in range(T):
                if th[t] < d2 <= th[t + 1]:
                    N[int(lab[i]), int(lab[j]), t] += 1
    return N


def tally_offsets(ix, iy, c1, c2, lab, K, r, reach=1):
    """The table of points that sit one per node (ix, iy) of an integer lattice, when only nodes at most `reach` apart in each
    axis can hold a pair within r[T] (the caller's to guarantee): the stated d2 on those candidate pairs alone."""
    th = thr2_of(r)
    T = th.shape[0] - 1
    lab = np.asarray(lab, dtype=np.int64)
    w, h = int(ix.max()) + 1, int(iy.max()) + 1
    node = np.full((w + 2 * reach, h + 2 * reach), -1, dtype=np.int64)
    node[ix + reach, iy + reach] = np.arange(ix.shape[0])
    N = np.zeros((K, K, T), dtype=np.int64)
    for ox in range(-reach, reach + 1):
        for oy in range(-reach, reach + 1):
            if ox == 0 and oy == 0:
                continue
            j = node[ix + reach + ox, iy + reach + oy]
            i = np.nonzero(j >= 0)[0]
            j = j[i]
            dx, dy = c1[i] - c1[j], c2[i] - c2[j]
            d2 = dx * dx + dy * dy
            t = np.searchsorted(th, d2, side="left") - 1
            ok = (t >= 0) & (t < T)
            np.add.at(N, (lab[i[ok]], lab[j[ok]], t[ok]), 1)
    return N


def stats(N, cumulative=False):
    """ratio[a, b, t] = ((double)N / (double)row[a]) / ((double)row[b] / (double)tot); NaN when row[a] or row[b] is 0."""
    N = np.cumsum(N, axis=2) if cumulative else np.asarray(N)
    K, _, T = N.shape
    out = np.full((K, K, T), np.nan)
    for t in range(T):
        row = N[:, :, t].sum(axis=1)
        tot = int(row.sum())
        for a in range(K):
            for b in range(K):
                if row[a] and row[b]:
                    out[a, b, t] = (float(int(N[a, b, t])) / float(int(row[a]))) / (float(int(row[b])) / float(tot))
    return out


def ripley(N, group_n, area):
    """(Kfun, L), K x T: Kfun = (area * (double)Ncum[a, a, t]) / (double)(n_a (n_a - 1)), L = sqrt(Kfun / pi); NaN for n_a < 2."""
    K, _, T = N.shape
    Kf, L = np.full((K, T), np.nan), np.full((K, T), np.nan)
    for a in range(K):
        cum, na = 0, int(group_n[a])
        for t in range(T):
            cum += int(N[a, a, t])
            if na >= 2:
                Kf[a, t] = (float(area) * float(cum)) / float(na * (na - 1))
                L[a, t] = math.sqrt(Kf[a, t] / PI)
    return Kf, L


def lds_fits(K, T):
    return T * K * K * 4 + STAGE_BYTES <= LDS_BYTES


def plan(n, K, T, grid_run, bin_path=0, flush_pairs=0):
    path = 2 if bin_path == 2 or not lds_fits(K, T) else 1
    tiles = -(-n // TILE)
    per = -(-tiles // MAX_WG)
    wgs = -(-tiles // per)
    split = min(-(-WG_TARGET // wgs), MAX_SPLIT, tiles) if grid_run == 1 else 1
    return {"bin_path": path, "lds_bytes": STAGE_BYTES + (T * K * K * 4 if path == 1 else 0), "tiles": tiles, "tiles_per_wg": per,
            "workgroups": wgs * split, "flush_pairs": flush_pairs or FLUSH_PAIRS}


def grid(c1, c2, reach, grid_mode=0):
    """(mode run, W, H) of the plan."""
    with np.errstate(over="ignore"):
        ex, ey = float(c1.max() - c1.min()), float(c2.max() - c2.min())
    ext = max(ex, ey)
    if grid_mode == 1 or not ext < math.inf:
        return 1, 1, 1
    side = max(max(reach, 2.0 ** -510) * (1.0 + 2.0 ** -10), ext * 2.0 ** -30)
    W, H = int(math.floor(ex / side)) + 2, int(math.floor(ey / side)) + 2
    if grid_mode == 0 and W <= 3 and H <= 3:
        return 1, 1, 1
    return 2, W, H


def default_interval(c1, c2, count):
    return np.linspace(0.0, 0.5 * float(np.hypot(c1.max() - c1.min(), c2.max() - c2.min())), count + 1)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def planted(seed, clumps=10, per=25, uniform=2000, spread=0.012):
    """Classes 0 and 1 share `clumps` Gaussian clumps in the unit square (per points of each class per clump); class 2 is uniform
    and dense enough to hold most close pairs, so the shared clumps stand out in the first interval."""
    rng = np.random.default_rng(1000 + seed)
    centres = rng.random((clumps, 2)) * 0.8 + 0.1
    pts, lab = [], []
    for cl in (0, 1):
        for c in centres:
            pts.append(c + spread * rng.standard_normal((per, 2)))
            lab.append(np.full(per, cl))
    pts.append(rng.random((uniform, 2)))
    lab.append(np.full(uniform, 2))
    xy, lab = np.concatenate(pts), np.concatenate(lab).astype(np.int32)
    order = rng.permutation(xy.shape[0])
    return xy[order], lab[order]


def poisson(seed, n=1500, K=2):
    rng = np.random.default_rng(2000 + seed)
    return rng.random((n, 2)), rng.integers(0, K, n).astype(np.int32)
