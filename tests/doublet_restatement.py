"""The rules of sgl_simulate_doublets and of the doublet scores (include/singlet_hip.h, "Simulated doublets"; DESIGN.md "Doublet
scores") restated in numpy, without a device: the pair merge, the parents, the scores, the threshold, and the whole pipe on
the host -- the oracle's normalisation and projection (oracle.log_normalize, oracle.scale, oracle.predict) and the search of
tests/embedding_knn_restatement.py.

The merge: the stored rows of S[:, s] are the sorted union of the parents' stored rows; a row stored in one parent carries
that value's bits, a row stored in both x_a + x_b, one numpy addition of two doubles (IEEE, commutative).  The scores and the
threshold are written as plain loops over cells and bins, on purpose not in the vectorised form of singlet_amd.api."""
import math

import numpy as np


def pair_columns(x, i, p, parent_a, parent_b):
    """(xo, io, po, shared): the CSC slots of S (po int64) and the rows stored in both parents, summed over the pairs."""
    xs, rows, po = [], [], [0]
    shared = 0
    for a, b in zip(np.asarray(parent_a).tolist(), np.asarray(parent_b).tolist()):
        ia, xa = i[p[a]:p[a + 1]], x[p[a]:p[a + 1]]
        ib, xb = i[p[b]:p[b + 1]], x[p[b]:p[b + 1]]
        u = np.union1d(ia, ib)
        out = np.empty(u.shape[0])
        in_a = np.zeros(u.shape[0], dtype=bool)
        qa, qb = np.searchsorted(u, ia), np.searchsorted(u, ib)
        out[qa] = xa
        in_a[qa] = True
        both = in_a[qb]
        out[qb[~both]] = xb[~both]
        with np.errstate(over="ignore"):
            out[qb[both]] = out[qb[both]] + xb[both]
        shared += int(both.sum())
        xs.append(out)
        rows.append(u.astype(np.int32))
        po.append(po[-1] + u.shape[0])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return cat(xs, np.float64), cat(rows, np.int32), np.asarray(po, dtype=np.int64), shared


def path_counts(p, parent_a, parent_b, cap):
    """(pairs on the LDS path, pairs on the long path): a pair is staged in LDS when la + lb <= cap."""
    ln = np.diff(np.asarray(p, dtype=np.int64))
    joint = ln[np.asarray(parent_a)] + ln[np.asarray(parent_b)]
    return int((joint <= cap).sum()), int((joint > cap).sum())


def parents(n_obs, n_sim, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n_obs, size=n_sim)
    b = (a + 1 + rng.integers(0, n_obs - 1, size=n_sim)) % n_obs
    return a.astype(np.int32), b.astype(np.int32)


def remaining_neighbours(row, own):
    """A cell's list without itself: its own index removed wherever it stands, else the last entry removed."""
    row = [int(v) for v in row]
    if own in row:
        row.remove(own)
    else:
        row.pop()
    return row


def scores(idx, n_obs, n_sim, expected_rate=0.1, stdev_rate=0.02):
    """(nd, Ld, se_Ld) over all n_obs + n_sim cells, the observed first."""
    n, k_adj = idx.shape[0], idx.shape[1] - 1
    rho, r = expected_rate, n_sim / n_obs
    nd, Ld, se = np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n)
    for j in range(n):
        nd[j] = sum(1 for v in remaining_neighbours(idx[j], j) if v >= n_obs)
        q = (nd[j] + 1) / (k_adj + 2)
        den = 1 - rho - q * (1 - rho - rho / r)
        Ld[j] = q * rho / r / den
        se_q = math.sqrt(q * (1 - q) / (k_adj + 3))
        se[j] = q * rho / r / den ** 2 * math.sqrt((se_q / q * (1 - rho)) ** 2 + (stdev_rate / rho * (1 - q)) ** 2)
    return nd, Ld, se


def threshold(sim_scores, bins=100):
    """The centre of the lowest bin between the two local maxima of the smoothed histogram; ValueError without two maxima."""
    top = float(np.max(sim_scores))
    h = np.histogram(sim_scores, bins=bins, range=(0.0, top))[0].astype(np.float64).tolist()   # (numpy's own bin edges decide)

    def maxima(h):
        ext = [0.0] + h + [0.0]
        return [b for b in range(bins) if ext[b + 1] > ext[b] and ext[b + 1] >= ext[b + 2]]
    peaks, rounds = maxima(h), 0
    while len(peaks) > 2 and rounds < 10000:
        ext = [0.0] + h + [0.0]
        h = [(ext[b] + ext[b + 1] + ext[b + 2]) / 3.0 for b in range(bins)]
        peaks, rounds = maxima(h), rounds + 1
    if len(peaks) != 2:
        raise ValueError("%d local maxima" % len(peaks))
    lo = min(range(peaks[0] + 1, peaks[1]), key=lambda b: (h[b], b))
    return (lo + 0.5) * top / bins


def auc(score, positive):
    """The probability that a positive cell outscores a negative one, ties counted half (midranks)."""
    score, positive = np.asarray(score, dtype=np.float64), np.asarray(positive, dtype=bool)
    order = np.argsort(score, kind="stable")
    s = score[order]
    rank = np.empty(s.shape[0])
    start = 0
    for stop in range(1, s.shape[0] + 1):
        if stop == s.shape[0] or s[stop] != s[start]:
            rank[start:stop] = 0.5 * (start + stop - 1) + 1.0
            start = stop
    r = np.empty_like(rank)
    r[order] = rank
    n1, n0 = int(positive.sum()), int((~positive).sum())
    return float((r[positive].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


def k_adjusted(n_obs, n_sim, n_neighbors=None):
    k = int(round(0.5 * math.sqrt(n_obs))) if n_neighbors is None else int(n_neighbors)
    return k, int(round(k * (1 + n_sim / float(n_obs))))


def embed(ora, x, i, p, nrow, w_scaled, rows=None, L1=0.01, L2=0.0, scale_factor=1e4):
    """H (cells x k) of the counts (x, i, p): oracle.log_normalize, the rows `rows` (ascending order kept as given), and the
    H-update of a projection on the scaled model (oracle.predict from H = 0), without the row scaling."""
    A = ora.log_normalize(ora.CSC(x, i, np.asarray(p, dtype=np.int32), nrow, len(p) - 1), scale_factor)
    if rows is not None:
        D = A.to_dense()[np.asarray(rows)]
        from planted_doublets import dense_to_csc
        A = ora.CSC(*dense_to_csc(D), D.shape[0], D.shape[1])
    return ora.predict(A, w_scaled, np.zeros((A.ncol, w_scaled.shape[1])), L1, L2)


_CACHE = {}


def planted_model(ora, rank=4, seed=7, maxit=30):
    """w (genes x rank) of the oracle's fit of the normalised planted fixture from a uniform start; computed once."""
    key = ("w", rank, seed, maxit)
    if key not in _CACHE:
        from planted_doublets import planted
        fx = planted()
        A = ora.log_normalize(ora.CSC(fx["x"], fx["i"], fx["p"], fx["dense"].shape[0], fx["dense"].shape[1]))
        w0 = np.random.default_rng(seed).random((A.nrow, rank))
        w = ora.c_nmf(A, A.t(), 1e-4, maxit, 0.01, 0.01, 0.0, 0.0, 0, w0)["w"]
        w.setflags(write=False)
        _CACHE[key] = w
    return _CACHE[key]


def planted_pipe(ora, sim_ratio, rank=4):
    """pipe() on the planted fixture with planted_model(rank); computed once per (sim_ratio, rank), never written to."""
    key = ("pipe", float(sim_ratio), rank)
    if key not in _CACHE:
        import embedding_knn_restatement as euclid
        from planted_doublets import planted
        fx = planted()
        _CACHE[key] = pipe(ora, euclid.knn, fx["x"], fx["i"], fx["p"], fx["dense"].shape[0], planted_model(ora, rank), sim_ratio=sim_ratio)
    return _CACHE[key]


def pipe(ora, knn, x, i, p, nrow, w, sim_ratio=2.0, n_neighbors=None, expected_rate=0.1, stdev_rate=0.02, seed=0, rows=None,
         L1=0.01, L2=0.0, scale_factor=1e4, perturb=None, extra=1):
    """The whole pipe on the host.  w: genes x k.  perturb: a function applied to the joint embedding before the search.
    Returns the merged S, the embeddings, the neighbour lists with `extra` more neighbours than the scores read (their
    squared distances tell how close a list's cut was), nd / Ld / se, and the parents."""
    n_obs = len(p) - 1
    n_sim = int(round(sim_ratio * n_obs))
    pa, pb = parents(n_obs, n_sim, seed)
    sx, si, sp, shared = pair_columns(x, i, p, pa, pb)
    ws, _ = ora.scale(np.ascontiguousarray(w, dtype=np.float64))
    h_obs = embed(ora, x, i, p, nrow, ws, rows, L1, L2, scale_factor)
    h_sim = embed(ora, sx, si, sp, nrow, ws, rows, L1, L2, scale_factor)
    E = np.concatenate([h_obs, h_sim], axis=0)
    if perturb is not None:
        E = perturb(E)
    k, k_adj = k_adjusted(n_obs, n_sim, n_neighbors)
    idx, dist = knn(E.T, None, k_adj + 1 + extra)
    nd, Ld, se = scores(idx[:, :k_adj + 1], n_obs, n_sim, expected_rate, stdev_rate)
    return {"S": (sx, si, sp), "shared": shared, "h_obs": h_obs, "h_sim": h_sim, "idx": idx, "dist": dist, "k_adj": k_adj, "nd": nd,
            "score": Ld, "se": se, "parent_a": pa, "parent_b": pb, "n_obs": n_obs, "n_sim": n_sim}
