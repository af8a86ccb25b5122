"""The rules of the layout stage (include/singlet_hip.h, "Layout") restated in numpy, vectorised per epoch: the fuzzy
neighbour graph, one synchronous epoch, the whole layout, and trustworthiness.  Every sum runs in the stated order -- a loop
over the positions of the order, vectorised across the cells -- and every product and addition is its own rounding (numpy
does not contract).  The GPU tests hold the library to these functions; the CPU tests hold these functions to hand-worked
cases and to the quality criterion.  Nothing here is the code under test.

Also here, as the quality yardstick ONLY: a sequential optimiser in umap-learn's edge order, with per-edge "next sample"
arrays and head and tail both moving (plain Python floats; slow).

A graph is (p, i, x): the three arrays of an n x n dgCMatrix, rows ascending within a column."""
import math

import numpy as np

BLOCK = 1024
U64 = np.uint64


def rand2(state, i, j):
    """The library's counter hash on uint64 arrays: bit for bit oracle.rng_rand."""
    with np.errstate(over="ignore"):
        i = np.array(i, dtype=U64)
        j = np.array(j, dtype=U64)
        i ^= i << U64(19)
        i ^= i >> U64(7)
        i ^= i << U64(36)
        x = U64(int(state) & (2**64 - 1)) + i
        x ^= x << U64(38)
        x ^= x >> U64(13)
        x ^= x << U64(23)
        j ^= j >> U64(7)
        j ^= j << U64(23)
        j ^= j >> U64(8)
        x = x + j
        x ^= x >> U64(7)
        x ^= x << U64(53)
        x ^= x >> U64(4)
    return x


def blocked_sum(v):
    """Blocks of BLOCK consecutive terms, each sequential from +0.0; then the block sums, sequentially from +0.0."""
    v = np.asarray(v, dtype=np.float64).ravel()
    nb = (v.size + BLOCK - 1) // BLOCK
    pad = np.zeros(nb * BLOCK)            # (+0.0 after the last term of the last block changes no sum that began at +0.0)
    pad[:v.size] = v
    blocks = pad.reshape(nb, BLOCK)
    s = np.zeros(nb)
    for t in range(BLOCK):
        s = s + blocks[:, t]
    total = 0.0
    for b in range(nb):
        total = total + float(s[b])
    return total


# ------------------------------------------------------------------------------------------------------------ fuzzy graph
def check_lists(idx, dist):
    """The refusals of sgl_c_fuzzy_graph: ValueError with the defect's name."""
    idx, dist = np.asarray(idx), np.asarray(dist, dtype=np.float64)
    n, K = idx.shape
    if not 2 <= K <= 256:
        raise ValueError("K")
    if not 1 <= n < 2**31:
        raise ValueError("n")
    if (idx < 0).any() or (idx >= n).any():
        raise ValueError("index range")
    srt = np.sort(idx, axis=1)
    if (srt[:, 1:] == srt[:, :-1]).any():
        raise ValueError("index repeated")
    if not np.isfinite(dist).all():
        raise ValueError("not finite")
    if (dist < 0).any():
        raise ValueError("negative")
    if (dist[:, 1:] < dist[:, :-1]).any():
        raise ValueError("order")


def smooth_knn(idx, dist):
    """-> rho, sigma, P (n x K memberships, +0.0 in the cell's own slot), own (n x K mask)."""
    idx = np.asarray(idx, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    n, K = idx.shape
    own = idx != np.arange(n)[:, None]
    pos = own & (dist > 0)
    rho = np.where(pos.any(axis=1), np.min(np.where(pos, dist, np.inf), axis=1), 0.0)   # the lists ascend: the first one
    s = np.zeros(n)
    for q in range(K):
        s = s + np.where(own[:, q], dist[:, q], 0.0)
    gmean = blocked_sum(dist) / float(n * K)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(rho > 0, s / own.sum(axis=1), gmean)
    target = math.log2(K)
    t = dist - rho[:, None]
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for _ in range(64):
            ps = np.zeros(n)
            for q in range(K):
                term = np.where(t[:, q] > 0, np.exp(-t[:, q] / mid), 1.0)
                ps = ps + np.where(own[:, q], term, 0.0)
            up = ps > target
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
            mid = np.where(up | np.isfinite(hi), (lo + hi) / 2.0, 2.0 * mid)
        sigma = np.fmax(mid, 1e-3 * mean)
        P = np.where(own, np.where(t > 0, np.exp(-t / sigma[:, None]), 1.0), 0.0)
    return rho, sigma, P, own


def fuzzy_graph(idx, dist):
    """-> (p, i, x, rho, sigma): w_ij = (p_ij + p_ji) - p_ij * p_ji, an absent direction +0.0; zeros dropped."""
    check_lists(idx, dist)
    idx = np.asarray(idx, dtype=np.int64)
    n, K = idx.shape
    rho, sigma, P, own = smooth_knn(idx, dist)
    src = np.repeat(np.arange(n), K)[own.ravel()]
    dst = idx.ravel()[own.ravel()]
    val = P.ravel()[own.ravel()]
    # column c, row r: `po` the membership of r in c's list, `pi` the membership of c in r's list
    col = np.concatenate([src, dst])
    row = np.concatenate([dst, src])
    po = np.concatenate([val, np.zeros(val.size)])
    pi = np.concatenate([np.zeros(val.size), val])
    key = col * n + row
    uk, inv = np.unique(key, return_inverse=True)
    a, b = np.zeros(uk.size), np.zeros(uk.size)
    np.add.at(a, inv, po)     # at most one non-zero term per sum: exact
    np.add.at(b, inv, pi)
    w = (a + b) - a * b
    keep = w != 0
    uk, w = uk[keep], w[keep]
    p = np.concatenate([[0], np.cumsum(np.bincount(uk // n, minlength=n))]).astype(np.int64)
    return p, (uk % n).astype(np.int64), w, rho, sigma


# ------------------------------------------------------------------------------------------------------------------ layout
def _terms(yj, yo, a, b, attractive, same=None):
    """The clipped terms (m x dim) of heads yj against points yo; same: the mask of samples that hit their head."""
    d = yj - yo
    d2 = np.zeros(d.shape[0])
    for f in range(d.shape[1]):
        d2 = d2 + d[:, f] * d[:, f]
    with np.errstate(all="ignore"):
        pw = d2 if b == 1.0 else np.power(d2, b)
        if attractive:
            c = ((-2.0 * a * b) * (pw / d2)) / (a * pw + 1.0)
        else:
            c = (2.0 * b) / ((0.001 + d2) * (a * pw + 1.0))
        out = np.fmin(np.fmax(c[:, None] * d, -4.0), 4.0)
    if attractive:
        out[~(d2 > 0)] = 0.0
    else:
        out[d2 == 0] = 4.0
        if same is not None:
            out[same] = 0.0
    return out


def firing(x, w_max, t):
    r = np.asarray(x, dtype=np.float64) / w_max
    return np.floor(float(t) * r) > np.floor(float(t - 1) * r)


def alpha_of(alpha0, t, n_epochs):
    return alpha0 * (1.0 - float(t - 1) / float(n_epochs))


def epoch(p, i, x, Y, a, b, n_epochs, alpha0, neg_rate, seed, t, with_bound=False):
    """The ONE epoch t (1-based) from the positions Y (n x dim) -> the new positions; with_bound also S (n x dim), the sum of
    the absolute clipped terms of every vertex."""
    p, i, x = np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(x, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n, dim = Y.shape
    S = np.zeros((n, dim))
    w_max = float(x.max()) if x.size else 0.0
    if not w_max > 0:
        return (Y.copy(), S) if with_bound else Y.copy()
    col = np.repeat(np.arange(n), np.diff(p))
    e = np.flatnonzero(firing(x, w_max, t) & (i != col))
    head = col[e]
    g = _terms(Y[head], Y[i[e]], a, b, True)
    absg = np.abs(g)
    for s in range(neg_rate):
        u = rand2(seed, e.astype(U64), np.full(e.size, 256 * t + s, dtype=U64))
        m = (((u >> U64(32)) * U64(n)) >> U64(32)).astype(np.int64)
        term = _terms(Y[head], Y[m], a, b, False, m == head)
        g = g + term
        absg = absg + np.abs(term)
    # delta_j: the sequential sum of g_e over the firing entries of column j in stored order, from +0.0
    first = np.searchsorted(head, head, side="left")
    rank = np.arange(e.size) - first
    delta = np.zeros((n, dim))
    for r in range(int(rank.max()) + 1 if e.size else 0):
        sel = rank == r
        delta[head[sel]] = delta[head[sel]] + g[sel]
        S[head[sel]] += absg[sel]
    moved = np.zeros(n, dtype=bool)
    moved[head] = True
    step = alpha_of(alpha0, t, n_epochs) * delta
    out = np.where(moved[:, None], Y + step, Y)
    return (out, S) if with_bound else out


def layout(p, i, x, Y0, a, b, n_epochs, alpha0=1.0, neg_rate=5, seed=42):
    Y = np.array(Y0, dtype=np.float64)
    for t in range(1, n_epochs + 1):
        Y = epoch(p, i, x, Y, a, b, n_epochs, alpha0, neg_rate, seed, t)
    return Y


# ----------------------------------------------------------------------------------------------------------------- quality
def _sqdist(X):
    s = (X * X).sum(axis=1)
    D = s[:, None] + s[None, :] - 2.0 * (X @ X.T)
    np.fill_diagonal(D, -np.inf)    # the point itself ranks first and is left out below
    return D


def trustworthiness(X, Y, k):
    """Venna & Kaski's trustworthiness of the layout Y (n x dim) of the points X (n x D) at k neighbours."""
    n = X.shape[0]
    ox = np.argsort(_sqdist(X), axis=1, kind="stable")[:, 1:]
    rank_x = np.empty((n, n), dtype=np.int64)
    rank_x[np.arange(n)[:, None], ox] = np.arange(1, n)[None, :]
    ny = np.argsort(_sqdist(Y), axis=1, kind="stable")[:, 1:k + 1]
    r = rank_x[np.arange(n)[:, None], ny]
    return 1.0 - 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)) * float(np.maximum(r - k, 0).sum())


def label_purity(Y, labels, k):
    """The share of the k nearest layout neighbours of a point that carry its label, over all points."""
    ny = np.argsort(_sqdist(Y), axis=1, kind="stable")[:, 1:k + 1]
    return float((labels[ny] == labels[:, None]).mean())


def knn_lists(X, K):
    """Exact k-NN lists (idx, dist) by (squared distance, index), the point itself included, as sgl_knn ranks them."""
    n = X.shape[0]
    D = np.zeros((n, n))
    for f in range(X.shape[1]):
        t = X[:, None, f] - X[None, :, f]
        D = D + t * t
    idx = np.argsort(D, axis=1, kind="stable")[:, :K]
    return idx.astype(np.int32), np.sqrt(np.take_along_axis(D, idx, axis=1))


def pca_start(X, dim):
    """The top components of the centred points, signed so that each one's largest-magnitude loading is positive, scaled to
    max |y| = 10."""
    Xc = X - X.mean(axis=0, keepdims=True)
    lam, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, np.argsort(-lam, kind="stable")[:dim]]
    top = np.argmax(np.abs(V), axis=0)
    V = V * np.where(V[top, np.arange(dim)] < 0, -1.0, 1.0)
    Y = Xc @ V
    return Y * (10.0 / np.max(np.abs(Y)))


def sequential_layout(p, i, x, Y0, a, b, n_epochs, alpha0=1.0, neg_rate=5, seed=0):
    """The yardstick: umap-learn's optimize_layout_euclidean, one edge after the other in stored order, head AND tail moving,
    per-edge epoch_of_next_sample arrays, a seeded generator for the negative samples.  Plain Python floats."""
    p, i, x = np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(x, dtype=np.float64)
    n, dim = np.asarray(Y0).shape
    col = np.repeat(np.arange(n), np.diff(p))
    w_max = float(x.max())
    keep = (x >= w_max / float(n_epochs)) & (i != col)
    head, tail = col[keep].tolist(), i[keep].tolist()
    eps = (w_max / x[keep]).tolist()
    eps_neg = [v / neg_rate for v in eps] if neg_rate else None
    nxt, nxt_neg = list(eps), list(eps_neg) if neg_rate else None
    Y = [list(map(float, row)) for row in np.asarray(Y0)]
    rng = np.random.default_rng(seed)
    alpha = alpha0
    rd = range(dim)
    for ep in range(n_epochs):
        draws = rng.integers(0, n, size=len(head) * max(neg_rate, 1) // 2 + 64).tolist()
        nd = 0
        for q in range(len(head)):
            if nxt[q] > ep:
                continue
            cur, oth = Y[head[q]], Y[tail[q]]
            d2 = 0.0
            for f in rd:
                d2 += (cur[f] - oth[f]) ** 2
            gc = (-2.0 * a * b * math.pow(d2, b - 1.0)) / (a * math.pow(d2, b) + 1.0) if d2 > 0.0 else 0.0
            for f in rd:
                gd = min(4.0, max(-4.0, gc * (cur[f] - oth[f])))
                cur[f] += gd * alpha
                oth[f] -= gd * alpha
            nxt[q] += eps[q]
            if not neg_rate:
                continue
            n_neg = int((ep - nxt_neg[q]) / eps_neg[q])
            for _ in range(n_neg):
                if nd == len(draws):
                    draws, nd = rng.integers(0, n, size=len(draws)).tolist(), 0
                k = draws[nd]
                nd += 1
                oth = Y[k]
                d2 = 0.0
                for f in rd:
                    d2 += (cur[f] - oth[f]) ** 2
                if d2 > 0.0:
                    gc = (2.0 * b) / ((0.001 + d2) * (a * math.pow(d2, b) + 1.0))
                elif head[q] == k:
                    continue
                else:
                    gc = 0.0
                for f in rd:
                    gd = min(4.0, max(-4.0, gc * (cur[f] - oth[f]))) if gc > 0.0 else 4.0
                    cur[f] += gd * alpha
            nxt_neg[q] += n_neg * eps_neg[q]
        alpha = alpha0 * (1.0 - float(ep + 1) / float(n_epochs))
    return np.array(Y)
