"""The rules of the layout transform (include/singlet_hip.h, "Layout transform") restated in numpy, vectorised across the
queries: the memberships of a query's neighbour list against the reference, the start, the epochs, the whole transform.
Every sum runs in the stated order -- a loop over the positions of the order -- and every product, quotient and addition is
its own rounding (numpy does not contract).  The GPU tests hold the library to these functions; the CPU tests hold these
functions to hand-worked lists and to the independence properties.  Nothing here is the code under test.

Lists are (idx, dist), n_query x K (row q the list of query q in rank order, as the searches return them), padding -1 / +Inf
behind the valid slots.  Positions are n x dim.

Also here, as the quality yardstick ONLY: a sequential transform in umap-learn's manner (per-slot "next sample" arrays, a
seeded generator, only the head moving, the same memberships; plain Python floats)."""
import math

import numpy as np

import umap_restatement as ur

U64 = np.uint64
QNAN = np.uint64(0x7FF8000000000000).view(np.float64)
EPOCHS_PER_LAUNCH = 128


def check_lists(idx, dist, n_ref):
    """The refusals of the lists: ValueError with the defect's name."""
    idx, dist = np.asarray(idx), np.asarray(dist, dtype=np.float64)
    n, K = idx.shape
    if not 1 <= K <= 256:
        raise ValueError("K")
    if not 1 <= n_ref < 2**31:
        raise ValueError("n_ref")
    if (idx < -1).any() or (idx >= n_ref).any():
        raise ValueError("index range")
    valid = idx >= 0
    if (valid[:, 1:] & ~valid[:, :-1]).any():
        raise ValueError("valid behind padding")
    srt = np.sort(np.where(valid, idx, -1 - np.arange(K)[None, :]), axis=1)
    if (srt[:, 1:] == srt[:, :-1]).any():
        raise ValueError("index repeated")
    d = np.where(valid, dist, 0.0)
    if not np.isfinite(d).all():
        raise ValueError("not finite")
    if (d < 0).any():
        raise ValueError("negative")
    if (valid[:, 1:] & (dist[:, 1:] < dist[:, :-1])).any():
        raise ValueError("order")


def fuzzy_query(idx, dist):
    """-> rho, sigma (n), W (n x K memberships, +0.0 in the padding slots)."""
    idx = np.asarray(idx, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    n, K = idx.shape
    own = idx >= 0
    d = np.where(own, dist, 0.0)
    pos = own & (d > 0)
    rho = np.where(pos.any(axis=1), np.min(np.where(pos, d, np.inf), axis=1), 0.0)   # the lists ascend: the first one
    s = np.zeros(n)
    for q in range(K):
        s = s + np.where(own[:, q], d[:, q], 0.0)       # (+0.0 for a padding slot changes no sum that began at +0.0)
    cnt = own.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, s / cnt, 0.0)
    target = math.log2(K)
    t = d - rho[:, None]
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
        W = np.where(own, np.where(t > 0, np.exp(-t / sigma[:, None]), 1.0), 0.0)
    empty = cnt == 0
    rho = np.where(empty, 0.0, rho)
    sigma = np.where(empty, 0.0, sigma)
    return rho, sigma, W


def start(idx, W, Yref):
    """y0_f = (sum_s w_s * Yref[idx_s, f]) / (sum_s w_s), both sums in slot order from +0.0; a quiet NaN without a valid slot."""
    idx = np.asarray(idx, dtype=np.int64)
    W = np.asarray(W, dtype=np.float64)
    Yref = np.asarray(Yref, dtype=np.float64)
    n, K = idx.shape
    own = idx >= 0
    num, den = np.zeros((n, Yref.shape[1])), np.zeros(n)
    for s in range(K):
        o = own[:, s]
        w = W[o, s]
        num[o] = num[o] + w[:, None] * Yref[idx[o, s]]
        den[o] = den[o] + w
    with np.errstate(invalid="ignore", divide="ignore"):
        y0 = num / den[:, None]
    y0[~own.any(axis=1)] = QNAN
    return y0


def firing(W, t):
    W = np.asarray(W, dtype=np.float64)
    return np.floor(float(t) * W) > np.floor(float(t - 1) * W)


def epochs(idx, W, Yref, Yin, a, b, n_epochs, alpha0=0.25, neg_rate=5, seed=42, query_offset=0, t_first=1, t_last=None,
           with_bound=False):
    """The epochs t_first .. t_last (1-based) of the queries from the positions Yin -> the new positions; with_bound also S
    (n x dim), the sum of the absolute clipped terms of every query over the LAST epoch of the range."""
    idx = np.asarray(idx, dtype=np.int64)
    W = np.asarray(W, dtype=np.float64)
    Yref = np.asarray(Yref, dtype=np.float64)
    Y = np.array(Yin, dtype=np.float64)
    n, K = idx.shape
    n_ref, dim = Yref.shape
    own = idx >= 0
    empty = ~own.any(axis=1)
    t_last = n_epochs if t_last is None else t_last
    S = np.zeros((n, dim))
    for t in range(t_first, t_last + 1):
        S = np.zeros((n, dim))
        head, slot = np.nonzero(own & firing(W, t))          # row-major: queries ascending, slots ascending within a query
        if head.size == 0:
            continue
        g = ur._terms(Y[head], Yref[idx[head, slot]], a, b, True)
        absg = np.abs(g)
        if neg_rate:
            # all samples of the epoch at once (firing slots x neg_rate); the terms are then added in the order of the samples
            ctr = (U64(256) * (U64(query_offset) + head.astype(U64)) + slot.astype(U64))
            u = ur.rand2(seed, ctr[:, None], (U64(256 * t) + np.arange(neg_rate, dtype=U64))[None, :])
            m = (((u >> U64(32)) * U64(n_ref)) >> U64(32)).astype(np.int64)
            terms = ur._terms(np.repeat(Y[head], neg_rate, axis=0), Yref[m.ravel()], a, b, False).reshape(head.size, neg_rate, dim)
            for i in range(neg_rate):
                g = g + terms[:, i]
                absg = absg + np.abs(terms[:, i])
        first = np.searchsorted(head, head, side="left")
        rank = np.arange(head.size) - first
        delta = np.zeros((n, dim))
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            delta[head[sel]] = delta[head[sel]] + g[sel]
            S[head[sel]] += absg[sel]
        moved = np.zeros(n, dtype=bool)
        moved[head] = True
        step = ur.alpha_of(alpha0, t, n_epochs) * delta
        Y = np.where(moved[:, None], Y + step, Y)
    Y[empty] = QNAN
    return (Y, S) if with_bound else Y


def transform(idx, dist, Yref, a, b, n_epochs, alpha0=0.25, neg_rate=5, seed=42, query_offset=0):
    """-> (Y0, Y): the start and the positions after n_epochs epochs."""
    check_lists(idx, dist, np.asarray(Yref).shape[0])
    _, _, W = fuzzy_query(idx, dist)
    Y0 = start(idx, W, Yref)
    return Y0, epochs(idx, W, Yref, Y0, a, b, n_epochs, alpha0, neg_rate, seed, query_offset)


def launches(t_first, t_last, per_launch=EPOCHS_PER_LAUNCH):
    """The host plan's cut of the epochs into launches: [(first, last), ...]."""
    return [(t, min(t + per_launch - 1, t_last)) for t in range(t_first, t_last + 1, per_launch)]


# ----------------------------------------------------------------------------------------------------------------- quality
def neighbour_share(E_ref, E_query, Y_ref, Y_query, k=15):
    """The mean share of a query's k nearest references in the embedding that are among its k nearest in the layout."""
    def nearest(R, Q):
        D = np.zeros((Q.shape[0], R.shape[0]))
        for f in range(R.shape[1]):
            t = Q[:, None, f] - R[None, :, f]
            D = D + t * t
        return np.argsort(D, axis=1, kind="stable")[:, :k]
    ne, ny = nearest(E_ref, E_query), nearest(Y_ref, Y_query)
    return float(np.mean([np.intersect1d(ne[q], ny[q]).size / float(k) for q in range(ne.shape[0])]))


def sequential_transform(idx, W, Yref, Y0, a, b, n_epochs, alpha0=0.25, neg_rate=5, seed=0):
    """The yardstick: umap-learn's optimize_layout_euclidean with move_other = False, one slot after the other in list order,
    per-slot epoch_of_next_sample arrays, a seeded generator for the negative samples; only the query moves."""
    idx = np.asarray(idx, dtype=np.int64)
    W = np.asarray(W, dtype=np.float64)
    n, K = idx.shape
    n_ref, dim = np.asarray(Yref).shape
    keep = (idx >= 0) & (W >= 1.0 / float(n_epochs))         # the list's maximum is 1.0
    head, slot = np.nonzero(keep)
    tail = idx[head, slot].tolist()
    eps = (1.0 / W[head, slot]).tolist()
    head = head.tolist()
    eps_neg = [v / neg_rate for v in eps] if neg_rate else None
    nxt, nxt_neg = list(eps), list(eps_neg) if neg_rate else None
    Y = [list(map(float, row)) for row in np.asarray(Y0)]
    R = [list(map(float, row)) for row in np.asarray(Yref)]
    rng = np.random.default_rng(seed)
    alpha = alpha0
    rd = range(dim)
    for ep in range(n_epochs):
        draws = rng.integers(0, n_ref, size=len(head) * max(neg_rate, 1) // 2 + 64).tolist()
        nd = 0
        for q in range(len(head)):
            if nxt[q] > ep:
                continue
            cur, oth = Y[head[q]], R[tail[q]]
            d2 = 0.0
            for f in rd:
                d2 += (cur[f] - oth[f]) ** 2
            gc = (-2.0 * a * b * math.pow(d2, b - 1.0)) / (a * math.pow(d2, b) + 1.0) if d2 > 0.0 else 0.0
            for f in rd:
                cur[f] += min(4.0, max(-4.0, gc * (cur[f] - oth[f]))) * alpha
            nxt[q] += eps[q]
            if not neg_rate:
                continue
            n_neg = int((ep - nxt_neg[q]) / eps_neg[q])
            for _ in range(n_neg):
                if nd == len(draws):
                    draws, nd = rng.integers(0, n_ref, size=len(draws)).tolist(), 0
                oth = R[draws[nd]]
                nd += 1
                d2 = 0.0
                for f in rd:
                    d2 += (cur[f] - oth[f]) ** 2
                gc = (2.0 * b) / ((0.001 + d2) * (a * math.pow(d2, b) + 1.0)) if d2 > 0.0 else 0.0
                for f in rd:
                    cur[f] += (min(4.0, max(-4.0, gc * (cur[f] - oth[f]))) if gc > 0.0 else 4.0) * alpha
            nxt_neg[q] += n_neg * eps_neg[q]
        alpha = alpha0 * (1.0 - float(ep + 1) / float(n_epochs))
    return np.array(Y)


def nearest_labels_agree(Y_ref, Y_query, labels_ref, labels_query, k=10):
    """Does every query carry the label of each of its k nearest references in the layout?"""
    D = np.zeros((Y_query.shape[0], Y_ref.shape[0]))
    for f in range(Y_ref.shape[1]):
        t = Y_query[:, None, f] - Y_ref[None, :, f]
        D = D + t * t
    near = np.argsort(D, axis=1, kind="stable")[:, :k]
    return bool((labels_ref[near] == labels_query[:, None]).all())


def quality_case(points, recorded, name):
    """The held-out split of one data set of tests/golden/umap_fixtures.npz (`points`) with what
    tests/golden/umap_transform_fixtures.npz (`recorded`) holds for it."""
    X, labels, query = points[name + "_X"], points[name + "_labels"], recorded[name + "_query"]
    K, n_epochs, neg, share_k = (int(v) for v in recorded["settings"])
    a, b = (float(v) for v in recorded["ab"])
    return dict(R=X[~query], Q=X[query], labels_ref=labels[~query], labels_query=labels[query], idx=recorded[name + "_idx"],
                dist=recorded[name + "_dist"], Yref=recorded[name + "_Yref"], S_start=float(recorded[name + "_S_start"]),
                S_seq=recorded[name + "_S_seq"], K=K, n_epochs=n_epochs, neg=neg, share_k=share_k, a=a, b=b,
                alpha0=float(recorded["alpha0"]))


def quality_floor(S_seq):
    """The yardstick's worst seed minus its own seed-to-seed range (best minus worst)."""
    return float(S_seq.min()) - (float(S_seq.max()) - float(S_seq.min()))
