"""The rules of sgl_c_louvain (include/singlet_hip.h, "Clustering") restated in plain Python and numpy: every sum in the
stated order, every product and addition its own rounding (Python floats are IEEE doubles and nothing here contracts).
The GPU tests hold the library to these functions bit for bit; the CPU tests hold these functions to hand-worked cases and
to the quality criterion.  Nothing here is fast, and nothing here is the code under test.

A graph is (p, i, x): the three arrays of an n x n dgCMatrix, rows ascending within a column."""
import numpy as np

BLOCK = 1024          # the sums over members, communities and coarse entries: sequential inside blocks of BLOCK terms
MAX_LEVELS = 32


def seq_sum(vals):
    """+0.0, then the terms in order."""
    s = 0.0
    for v in vals:
        s = s + v
    return s


def blocked_sum(vals):
    """Blocks of BLOCK consecutive terms, each summed sequentially from +0.0; then the block sums, sequentially from +0.0."""
    total, s, cnt = 0.0, 0.0, 0
    for v in vals:
        s = s + v
        cnt += 1
        if cnt == BLOCK:
            total, s, cnt = total + s, 0.0, 0
    if cnt:
        total = total + s
    return total


def as_graph(p, i, x):
    return np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(x, dtype=np.float64)


def degrees(p, i, x):
    """k_v = the sequential sum of column v (diagonal included), and S = the blocked sum of k over v ascending."""
    n = len(p) - 1
    xs = x.tolist()
    k = [seq_sum(xs[p[v]:p[v + 1]]) for v in range(n)]
    return k, blocked_sum(k)


def modularity(p, i, x, labels, gamma, k=None, S=None):
    """-> Q, tot, size.  own_v = the sequential sum, in ascending row, of the entries of column v whose row lies in v's
    community (the diagonal is one of them); tot_c / in_c = the blocked sums of k_v / own_v over the members of c in
    ascending v; term_c = in_c / S - (gamma * (tot_c / S)) * (tot_c / S), +0.0 for an id without members; Q = the blocked sum
    of term_c over the ids 0 .. n-1."""
    n = len(p) - 1
    if k is None:
        k, S = degrees(p, i, x)
    L = [int(c) for c in labels]
    xs, rows = x.tolist(), i.tolist()
    own = [seq_sum(xs[e] for e in range(p[v], p[v + 1]) if L[rows[e]] == L[v]) for v in range(n)]
    members = {}
    for v in range(n):
        members.setdefault(L[v], []).append(v)
    tot, size, term = [0.0] * n, [0] * n, [0.0] * n
    for c, mem in members.items():
        tot[c] = blocked_sum(k[v] for v in mem)
        inn = blocked_sum(own[v] for v in mem)
        size[c] = len(mem)
        b = tot[c] / S
        term[c] = inn / S - (gamma * b) * b
    return blocked_sum(term), tot, size


def sweep(p, i, x, labels, gamma, k, S, tot, size):
    """One synchronous sweep -> new labels, number of moved vertices."""
    n = len(p) - 1
    L = [int(c) for c in labels]
    xs, rows = x.tolist(), i.tolist()
    new, moved = list(L), 0
    for v in range(n):
        o, w = L[v], {}
        for e in range(p[v], p[v + 1]):
            j = rows[e]
            if j != v:
                w[L[j]] = w.get(L[j], 0.0) + xs[e]      # ascending j within every community
        if not w:
            continue                                     # no off-diagonal neighbour: never moves
        w.setdefault(o, 0.0)
        gk = gamma * k[v]
        best, gbest, go = -1, 0.0, 0.0
        for c in sorted(w):
            g = w[c] - (gk * ((tot[c] - k[v]) if c == o else tot[c])) / S
            if c == o:
                go = g
            if best < 0 or g > gbest:                    # ascending c: a tie stays with the lower id
                best, gbest = c, g
        if best != o and gbest > go and not (size[o] == 1 and size[best] == 1 and best > o):
            new[v] = best
            moved += 1
    return new, moved


def op_sweep(p, i, x, labels, gamma):
    """sgl_op_louvain_sweep: -> labels_out, Q of labels, Q of labels_out, moved.  No guard decision."""
    p, i, x = as_graph(p, i, x)
    k, S = degrees(p, i, x)
    q0, tot, size = modularity(p, i, x, labels, gamma, k, S)
    new, moved = sweep(p, i, x, labels, gamma, k, S, tot, size)
    q1 = modularity(p, i, x, new, gamma, k, S)[0]
    return np.array(new, dtype=np.int32), q0, q1, moved


def aggregate(p, i, x, labels):
    """-> cmap (old id -> new id, -1 for an id without members), the coarse graph (p, i, x).  The surviving ids are
    renumbered in ascending order; A'_cd = the blocked sum of A_uv over u in c, v in d in column-major order of the fine
    entries."""
    n = len(p) - 1
    L = np.asarray(labels, dtype=np.int64)
    ids = np.unique(L)
    cmap = np.full(n, -1, dtype=np.int64)
    cmap[ids] = np.arange(ids.size)
    nc = ids.size
    col = np.repeat(np.arange(n), np.diff(p))
    key = cmap[L[col]] * nc + cmap[L[i]]
    order = np.argsort(key, kind="stable")
    sk, sx = key[order], x[order].tolist()
    heads = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1]))) if sk.size else np.zeros(0, dtype=np.int64)
    ends = np.concatenate((heads[1:], [sk.size])).astype(np.int64)
    cx = np.array([blocked_sum(sx[a:b]) for a, b in zip(heads.tolist(), ends.tolist())], dtype=np.float64)
    gk = sk[heads] if sk.size else sk
    ci = (gk % nc).astype(np.int64)
    cp = np.searchsorted(gk // nc, np.arange(nc + 1), side="left").astype(np.int64)
    return cmap, (cp, ci, cx)


def renumber_by_size(assign):
    """Clusters numbered by descending size, ties by smallest member; 0 is the largest."""
    a = np.asarray(assign, dtype=np.int64)
    if a.size == 0:
        return np.zeros(0, dtype=np.int32), 0
    ids, first, count = np.unique(a, return_index=True, return_counts=True)
    order = np.lexsort((first, -count))
    rank = np.empty(ids.size, dtype=np.int64)
    rank[order] = np.arange(ids.size)
    lut = np.zeros(int(a.max()) + 1, dtype=np.int64)
    lut[ids] = rank
    return lut[a].astype(np.int32), int(ids.size)


def louvain(p, i, x, gamma=1.0, tol=1e-7, max_sweeps=64, max_levels=32, trace=None):
    """sgl_c_louvain for one resolution -> {"labels", "n_clusters", "n_levels", "q_levels", "sweeps_levels"}.
    trace: a list that receives (level, "start" | "kept" | "discarded", Q) in order."""
    p, i, x = as_graph(p, i, x)
    n = len(p) - 1
    out = {"labels": np.zeros(n, dtype=np.int32), "n_clusters": 0, "n_levels": 0,
           "q_levels": np.zeros(MAX_LEVELS), "sweeps_levels": np.zeros(MAX_LEVELS, dtype=np.int32)}
    if n == 0:
        return out
    assign = np.arange(n, dtype=np.int64)
    for level in range(max_levels):
        nl = len(p) - 1
        k, S = degrees(p, i, x)
        L = list(range(nl))
        Q, tot, size = modularity(p, i, x, L, gamma, k, S)
        if trace is not None:
            trace.append((level, "start", Q))
        kept = 0
        for _ in range(max_sweeps):
            new, moved = sweep(p, i, x, L, gamma, k, S, tot, size)
            if moved == 0:
                break                                    # Q' == Q: nothing to keep
            Q2, tot2, size2 = modularity(p, i, x, new, gamma, k, S)
            if Q2 <= Q:
                if trace is not None:
                    trace.append((level, "discarded", Q2))
                break
            gain, L, Q, tot, size = Q2 - Q, new, Q2, tot2, size2
            kept += 1
            if trace is not None:
                trace.append((level, "kept", Q))
            if gain <= tol:
                break
        out["q_levels"][level] = Q
        out["sweeps_levels"][level] = kept
        out["n_levels"] = level + 1
        if kept == 0:
            break
        cmap, coarse = aggregate(p, i, x, L)
        assign = cmap[np.asarray(L, dtype=np.int64)[assign]]
        if level + 1 < max_levels:
            p, i, x = coarse
    out["labels"], out["n_clusters"] = renumber_by_size(assign)
    return out


def dense_modularity(A, labels, gamma):
    """The formula evaluated the O(n^2) way, in numpy's own summation order (a check of the formula, not of the bits)."""
    A = np.asarray(A, dtype=np.float64)
    L = np.asarray(labels)
    k = A.sum(axis=0)
    S = k.sum()
    q = 0.0
    for c in np.unique(L):
        m = L == c
        q += A[np.ix_(m, m)].sum() / S - gamma * (k[m].sum() / S) ** 2
    return q
