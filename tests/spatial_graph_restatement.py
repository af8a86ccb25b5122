"""Test-side restatement of the reference's spatial_graph (src/singlet.cpp:1365-1414) in numpy float64, with this build's
rules (include/singlet_hip.h, sgl_spatial_graph): for each point i, scan j = 0, 1, ... in index order, keep j when
d = sqrt(dx*dx + dy*dy) < max_dist (strict) until max_k are kept, weight (max_dist - d) * (1 / max_dist), divide the column
by its sum taken sequentially in ascending row order.  numpy elementwise operations round each operation once (no
contraction), like the reference built for x86-64 without FMA.

Two forms: `brute` scans every j (n up to a few thousand); `columns` restates sampled columns of a large set through a
cell list of side 2 max_dist (conservative by a wide margin), whose candidates are then scanned in index order."""
from fractions import Fraction

import numpy as np


def _column(x, y, i, cand, max_dist, scale, max_k):
    """rows (ascending) and normalised weights of column i, given every candidate j that can lie within max_dist of i,
    in ascending index order"""
    dx = x[i] - x[cand]
    dy = y[i] - y[cand]
    d = np.sqrt(dx * dx + dy * dy)
    keep = np.nonzero(d < max_dist)[0][:max_k]
    w = (max_dist - d[keep]) * scale
    s = np.cumsum(w)[-1] if w.size else 0.0   # sequential, ascending rows
    v = w / s
    nz = v != 0   # the reference keeps the slots whose value is != 0 (all of them, under this build's refusals)
    return cand[keep][nz].astype(np.int32), v[nz]


def _check(x, y, max_dist, max_k):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    assert x.size == y.size and np.all(np.isfinite(x)) and np.all(np.isfinite(y))
    max_dist = float(max_dist)
    scale = 1.0 / max_dist
    assert max_dist > 0 and np.isfinite(max_dist) and np.isfinite(scale) and max_k >= 0
    return x, y, max_dist, scale, int(min(max_k, x.size))


def brute(x, y, max_dist, max_k=100):
    """(p, i, x) of the whole n x n graph"""
    x, y, max_dist, scale, K = _check(x, y, max_dist, max_k)
    n = x.size
    p = np.zeros(n + 1, dtype=np.int32)
    rows, vals = [], []
    every = np.arange(n, dtype=np.int64)
    for i in range(n if K > 0 else 0):
        r, v = _column(x, y, i, every, max_dist, scale, K)
        rows.append(r)
        vals.append(v)
        p[i + 1] = p[i] + r.size
    if K == 0:
        return p, np.zeros(0, np.int32), np.zeros(0)
    return p, np.concatenate(rows), np.concatenate(vals)


class CellList:
    """Cells of side 2 max_dist: a pair within max_dist lies in adjacent cells with a wide margin."""

    def __init__(self, x, y, max_dist, max_k=100):
        self.x, self.y, self.max_dist, self.scale, self.K = _check(x, y, max_dist, max_k)
        side = 2.0 * self.max_dist
        self.cx = np.floor((self.x - self.x.min()) / side).astype(np.int64) if self.x.size else np.zeros(0, np.int64)
        self.cy = np.floor((self.y - self.y.min()) / side).astype(np.int64) if self.y.size else np.zeros(0, np.int64)
        self.M = int(self.cy.max()) + 3 if self.cy.size else 3
        key = (self.cx + 1) * self.M + (self.cy + 1)
        self.order = np.argsort(key, kind="stable")   # each cell's members in ascending index
        self.skey = key[self.order]

    def column(self, i):
        """rows and normalised weights of column i"""
        if self.K == 0:
            return np.zeros(0, np.int32), np.zeros(0)
        parts = []
        for ddx in (-1, 0, 1):
            for ddy in (-1, 0, 1):
                k = (self.cx[i] + 1 + ddx) * self.M + (self.cy[i] + 1 + ddy)
                lo, hi = np.searchsorted(self.skey, [k, k + 1])
                parts.append(self.order[lo:hi])
        cand = np.sort(np.concatenate(parts))
        return _column(self.x, self.y, i, cand, self.max_dist, self.scale, self.K)

    def count(self, i):
        return self.column(i)[0].size


def columns(x, y, max_dist, max_k, cols):
    """{i: (rows, weights)} of the sampled columns"""
    cl = CellList(x, y, max_dist, max_k)
    return {int(i): cl.column(int(i)) for i in cols}


def fused_pairs(x, y, pairs):
    """the pairs (i, j) whose d changes when dx*dx + dy*dy is evaluated with one fused multiply-add (either operand order),
    the FMA emulated exactly with fractions"""
    out = []
    for i, j in pairs:
        dx = float(np.float64(x[i]) - np.float64(x[j]))
        dy = float(np.float64(y[i]) - np.float64(y[j]))
        plain = np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy))
        for a, b in ((dx, dy), (dy, dx)):
            fused = float(Fraction(a) * Fraction(a) + Fraction(float(np.float64(b) * np.float64(b))))
            if np.sqrt(np.float64(fused)) != plain:
                out.append((i, j))
                break
    return out


def lattice(side, offset=0.0):
    """side x side unit lattice, point y * side + x"""
    y, x = np.divmod(np.arange(side * side, dtype=np.int64), side)
    return x.astype(np.float64) + offset, y.astype(np.float64) + offset
