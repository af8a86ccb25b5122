"""Test-side numpy restatement of c_LKNN (src/singlet.cpp:1491-1603) and c_SNN (:1606-1665), rule for rule as
include/singlet_hip.h states them for sgl_c_lknn / sgl_c_snn.

  - float32 throughout: m, coordinates, radius and max_dist rounded once; the distance functions (l.1426-1478) accumulate
    in dimension order, one rounded float32 operation at a time across a vector of candidate pairs (never np.sum, which
    sums pairwise, and never a fused multiply-add);
  - selection: the k smallest by (distance, index), NaN after every number; then index order;
  - zeros (+-0) dropped after the selection (l.1572-1588);
  - a point keeping more than ceil((2 radius + 1)^2) - 1 neighbours is an overflow of the reference's slots (l.1496).

Two forms of LKNN: `lknn_brute` tests every pair (O(n^2), small n); `lknn_grid` finds the candidates through a cell list and
can restate a sample of the points of a large set.  Both run the same per-point rule (`_point`).
"""
import math

import numpy as np

F = np.float32
METRICS = ("jaccard", "cosine", "euclidean", "manhattan", "hamming", "kl")


class SlotOverflow(Exception):
    pass


def as_float_inputs(m, coord_x, coord_y):
    """The reference's argument conversion: Eigen float copies, m transposed iff m.cols != m.rows && m.rows == n (l.1492).
    Returns (mf D x n float32, cx, cy)."""
    m = np.asarray(m, dtype=np.float64)
    cx = np.asarray(coord_x, dtype=np.float64).astype(F)
    cy = np.asarray(coord_y, dtype=np.float64).astype(F)
    n = cx.size
    if m.shape[1] != m.shape[0] and m.shape[0] == n:
        m = m.T
    assert m.shape[1] == n
    return np.ascontiguousarray(m.astype(F)), cx, cy


def n_max_edges(radius):
    base = F(F(F(radius) * F(2)) + F(1))
    return math.ceil(float(base) * float(base)) - 1


def distances(P, Q, metric, similarity):
    """P, Q: D x c float32 (the point repeated, the candidates).  One float32 rounding per operation, dimension order."""
    D, c = Q.shape
    with np.errstate(all="ignore"):
        if metric in ("jaccard", "cosine"):
            pq, pp, qq = np.zeros(c, F), np.zeros(c, F), np.zeros(c, F)
            for d in range(D):
                a, b = P[d], Q[d]
                pq = pq + a * b
                pp = pp + a * a
                qq = qq + b * b
            if metric == "jaccard":
                r = F(1) - pq / ((pp + qq) - pq)
            else:
                r = F(1) - pq / (np.sqrt(pp) * np.sqrt(qq))
            if not similarity:
                r = F(1) - r
            return r.astype(F)
        if metric == "manhattan":
            s = np.zeros(c, F)
            for d in range(D):
                s = s + np.abs(P[d] - Q[d])
            return np.sqrt(s)
        if metric == "hamming":
            s = np.zeros(c, F)
            for d in range(D):
                s = s + np.where(P[d] != Q[d], F(1), F(0))
            return s
        if metric == "kl":
            pdivq, psum = np.zeros(c, F), np.zeros(c, F)
            for d in range(D):
                q = Q[d]
                pdivq = np.where(q != 0, pdivq + P[d] / np.where(q != 0, q, F(1)), pdivq)
                psum = psum + P[d]
            return (psum * np.log(pdivq.astype(np.float64)).astype(F)).astype(F)
        s = np.zeros(c, F)
        for d in range(D):
            t = P[d] - Q[d]
            s = s + t * t
        return np.sqrt(s)


def order_key(d):
    """(distance) -> uint32 key of the ranking: -0 == +0, NaN above +inf."""
    d = np.asarray(d, dtype=F).copy()
    d[d == 0] = F(0)
    u = d.view(np.uint32).copy()
    u[np.isnan(d)] = np.uint32(0x7fc00000)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _point(p1, cand, mf, cx, cy, k, radius, metric, similarity, max_dist):
    """cand: candidate indices in ascending order (any superset of the points inside the radius).  Returns (rows, x) of
    column p1 before the zero drop."""
    cand = cand[cand != p1]
    with np.errstate(all="ignore"):
        dx = cx[p1] - cx[cand]
        dy = cy[p1] - cy[cand]
        inside = np.sqrt(dx * dx + dy * dy) <= radius
    j = cand[inside]
    d = distances(np.repeat(mf[:, p1:p1 + 1], j.size, axis=1), mf[:, j], metric, similarity)
    if max_dist != 0:
        keep = ~(d > max_dist)
        j, d = j[keep], d[keep]
    if j.size > k:
        sel = np.lexsort((j, order_key(d)))[:k]
        sel = sel[np.argsort(j[sel], kind="stable")]
        j, d = j[sel], d[sel]
    return j, d


def _assemble(cols, n, nme):
    p = [0]
    rows, xs = [], []
    for j, d in cols:
        if j.size > nme:
            raise SlotOverflow("a point keeps %d neighbours, more than %d slots" % (j.size, nme))
        nz = d != 0
        rows.append(j[nz])
        xs.append(d[nz].astype(np.float64))
        p.append(p[-1] + int(nz.sum()))
    i = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    x = np.concatenate(xs) if xs else np.zeros(0)
    return np.asarray(p, dtype=np.int64), i, x


def lknn_brute(m, coord_x, coord_y, k, radius, metric, similarity, max_dist):
    """(p, i, x) of the n x n graph, every pair tested."""
    mf, cx, cy = as_float_inputs(m, coord_x, coord_y)
    radius, max_dist = F(radius), F(max_dist)
    n = cx.size
    allc = np.arange(n)
    cols = [_point(p1, allc, mf, cx, cy, k, radius, metric, similarity, max_dist) for p1 in range(n)]
    return _assemble(cols, n, n_max_edges(radius))


def _buckets(cx, cy, radius):
    xmin, ymin = float(cx.min()), float(cy.min())
    ext = max(float(cx.max()) - xmin, float(cy.max()) - ymin)
    side = max(max(float(radius), 2.0 ** -62) * (1 + 2.0 ** -10), ext * 2.0 ** -30)
    bx = np.floor((cx.astype(np.float64) - xmin) / side).astype(np.int64)
    by = np.floor((cy.astype(np.float64) - ymin) / side).astype(np.int64)
    return bx, by


def lknn_grid(m, coord_x, coord_y, k, radius, metric, similarity, max_dist, points=None):
    """Cell-list form.  points=None: the whole graph as (p, i, x); else {point: (rows, x)} for those points (after the zero
    drop; the slot check is applied to them only)."""
    mf, cx, cy = as_float_inputs(m, coord_x, coord_y)
    radius, max_dist = F(radius), F(max_dist)
    n = cx.size
    bx, by = _buckets(cx, cy, radius)
    W = int(bx.max()) + 3
    key = by * W + bx
    order = np.argsort(key, kind="stable")
    skey = key[order]
    nme = n_max_edges(radius)

    def column(p1):
        parts = []
        for yy in (by[p1] - 1, by[p1], by[p1] + 1):
            lo = np.searchsorted(skey, yy * W + max(bx[p1] - 1, 0), "left")
            hi = np.searchsorted(skey, yy * W + bx[p1] + 2, "left")
            parts.append(order[lo:hi])
        cand = np.sort(np.concatenate(parts))
        return _point(p1, cand, mf, cx, cy, k, radius, metric, similarity, max_dist)

    if points is None:
        return _assemble([column(p1) for p1 in range(n)], n, nme)
    out = {}
    for p1 in points:
        j, d = column(int(p1))
        if j.size > nme:
            raise SlotOverflow("a point keeps %d neighbours, more than %d slots" % (j.size, nme))
        nz = d != 0
        out[int(p1)] = (j[nz].astype(np.int32), d[nz].astype(np.float64))
    return out


def snn(Gi, Gp, nrow, ncol, min_similarity, columns=None):
    """c_SNN on G's pattern.  columns=None: (p, i, x) of the ncol x ncol graph; else {column: (rows, x)}."""
    import scipy.sparse as sp
    Gi = np.asarray(Gi, dtype=np.int64)
    Gp = np.asarray(Gp, dtype=np.int64)
    nnz = np.diff(Gp)
    B = sp.csc_matrix((np.ones(Gi.size, dtype=np.int64), Gi, Gp), shape=(nrow, ncol))
    cols = np.arange(ncol) if columns is None else np.asarray(columns)
    inter = (B.T.tocsr() @ B[:, cols]).tocsc()   # ncol x len(cols): |rows(j) & rows(i)|
    inter.sort_indices()
    out = {}
    for q, i in enumerate(cols):
        s, e = inter.indptr[q], inter.indptr[q + 1]
        j, c = inter.indices[s:e].astype(np.int64), inter.data[s:e].astype(np.int64)
        if nnz[i] == 0:
            out[int(i)] = (np.zeros(0, np.int32), np.zeros(0))
            continue
        sim = c.astype(np.float64) / (nnz[i] + nnz[j] - c).astype(np.float64)
        keep = (c > 0) & ((sim > min_similarity) | (j == i))
        x = np.where(j == i, 1.0, sim)
        out[int(i)] = (j[keep].astype(np.int32), x[keep])
    if columns is not None:
        return out
    p = np.zeros(ncol + 1, dtype=np.int64)
    for i in range(ncol):
        p[i + 1] = p[i] + out[i][0].size
    i_ = np.concatenate([out[i][0] for i in range(ncol)]) if ncol else np.zeros(0, np.int32)
    x_ = np.concatenate([out[i][1] for i in range(ncol)]) if ncol else np.zeros(0)
    return p, i_.astype(np.int32), x_


def lattice(side, offset=0.0):
    """side x side integer lattice as RescaleSpatial makes it: point y * side + x at (x, y) (+ offset)."""
    y, x = np.divmod(np.arange(side * side, dtype=np.int64), side)
    return x.astype(np.float64) + offset, y.astype(np.float64) + offset
