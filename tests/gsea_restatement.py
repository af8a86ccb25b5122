"""The rules of the gene set enrichment test (include/singlet_hip.h, "Gene set enrichment") restated in numpy, operation by
operation: TEST INFRASTRUCTURE ONLY.  Every floating-point operation is a numpy ufunc on doubles (no fused multiply-add),
in the stated order, so a correct kernel gives the same bits.

Layouts follow the library: w is m x k (w[:, f] a factor), the sets are set_ptr[P + 1] / set_genes[], results are P x k."""
import numpy as np

U64 = np.uint64
BLOCK = 64            # hits per block of the prefix sums
LDS_CAP = 4096        # genes of a set the library takes
MAX_NPERM = 1 << 20
MAX_K = 1024
SCORE_TYPES = {"pos": 0, "neg": 1, "std": 2}


def rand2(state, i, j):
    """The library's counter hash on uint64 arrays (broadcast)."""
    with np.errstate(over="ignore"):
        i = np.array(i, dtype=U64)
        j = np.array(j, dtype=U64)
        i ^= i << U64(19)
        i ^= i >> U64(7)
        i ^= i << U64(36)
        x = U64(state) + i
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


def ranking(wf):
    """(pos, aw) of one factor: pos[g] = the 0-based position of gene g under (w descending, gene ascending); aw[p] = |w| of the
    gene at position p."""
    wf = np.asarray(wf, dtype=np.float64)
    order = np.argsort(-wf, kind="stable")      # -0.0 == 0.0: the zeros are one tie run, kept in gene order
    pos = np.empty(wf.shape[0], dtype=np.int64)
    pos[order] = np.arange(wf.shape[0])
    return pos, np.abs(wf[order])


def prefix_sums(a):
    """cum of n rows of s hit weights each (n x s) in the stated order: blocks of 64, the Kogge-Stone ladder, the carry."""
    a = np.asarray(a, dtype=np.float64)
    n, s = a.shape
    nb = (s + BLOCK - 1) // BLOCK
    v = np.zeros((n, nb * BLOCK))
    v[:, :s] = a
    v = v.reshape(n, nb, BLOCK)
    d = 1
    while d < BLOCK:
        nxt = v.copy()
        nxt[:, :, d:] = v[:, :, d:] + v[:, :, :-d]
        v = nxt
        d <<= 1
    cum = np.empty_like(v)
    carry = np.zeros(n)
    for b in range(nb):
        cum[:, b, :] = carry[:, None] + v[:, b, :]
        carry = carry + v[:, b, BLOCK - 1]
    return cum.reshape(n, nb * BLOCK)[:, :s]


def scores(positions, aw, m):
    """(ES_pos, ES_neg) of n sets of s hits each: positions (n x s) ascending along a row, aw the factor's rank-ordered |w|."""
    p = np.asarray(positions, dtype=np.int64)
    n, s = p.shape
    a = aw[p]
    cum = prefix_sums(a)
    NR = cum[:, s - 1]
    i = np.arange(s, dtype=np.int64)
    zero = NR == 0.0
    safe = np.where(zero, 1.0, NR)[:, None]
    hit = np.where(zero[:, None], ((i + 1).astype(np.float64) / np.float64(s))[None, :], cum / safe)
    step = np.where(zero[:, None], np.float64(1.0) / np.float64(s), a / safe)
    top = hit - (p - i[None, :]).astype(np.float64) / np.float64(m - s)
    bottom = top - step
    return top.max(axis=1), bottom.min(axis=1)


def std_score(ep, en):
    ep, en = np.asarray(ep, dtype=np.float64), np.asarray(en, dtype=np.float64)
    a = np.abs(en)
    return np.where(ep > a, ep, np.where(ep < a, en, 0.0))


def pick(score_type, ep, en):
    return ep if score_type == 0 else (en if score_type == 1 else std_score(ep, en))


def observed(w, set_ptr, set_genes):
    """The observed scores of every set in every factor: three P x k arrays (pos, neg, std)."""
    w = np.asarray(w, dtype=np.float64)
    m, k = w.shape
    set_ptr = np.asarray(set_ptr, dtype=np.int64)
    set_genes = np.asarray(set_genes, dtype=np.int64)
    P = set_ptr.shape[0] - 1
    size = np.diff(set_ptr)
    ep, en = np.empty((P, k)), np.empty((P, k))
    for f in range(k):
        pos, aw = ranking(w[:, f])
        for s in np.unique(size):
            js = np.nonzero(size == s)[0]
            rows = np.stack([np.sort(pos[set_genes[set_ptr[j]:set_ptr[j + 1]]]) for j in js])
            ep[js, f], en[js, f] = scores(rows, aw, m)
    return ep, en, std_score(ep, en)


def null_sample(seed, r0, r1, m, s_max):
    """sample[r - r0, t] = the gene at place t of permutation r's order by (key, gene), t < s_max: the full sort's prefix."""
    out = np.empty((r1 - r0, s_max), dtype=np.int64)
    g = np.arange(m, dtype=U64)
    for r in range(r0, r1):
        key = rand2(seed, np.full(m, r, dtype=U64), g)
        out[r - r0] = np.lexsort((np.arange(m), key))[:s_max]
    return out


def null_scores(w, sizes, score_type, seed, r0, r1, sample=None):
    """null[f, si, r - r0] of the sizes (ascending) for the permutations [r0, r1)."""
    w = np.asarray(w, dtype=np.float64)
    m, k = w.shape
    sizes = [int(s) for s in sizes]
    if sample is None:
        sample = null_sample(seed, r0, r1, m, sizes[-1])
    out = np.empty((k, len(sizes), r1 - r0))
    for f in range(k):
        pos, aw = ranking(w[:, f])
        for si, s in enumerate(sizes):
            ep, en = scores(np.sort(pos[sample[:, :s]], axis=1), aw, m)
            out[f, si] = pick(score_type, ep, en)
    return out


def bh(p):
    """Benjamini-Hochberg over the values that are not NaN, as the header states it."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    idx = np.nonzero(~np.isnan(p))[0]
    n = idx.size
    if n == 0:
        return out
    o = idx[np.lexsort((idx, p[idx]))]
    v = (np.float64(n) / np.arange(1, n + 1, dtype=np.float64)) * p[o]
    run = np.minimum.accumulate(v[::-1])[::-1]
    out[o] = np.minimum(run, 1.0)
    return out


def running_sum(v):
    """The elements added one by one from +0.0."""
    s = np.float64(0.0)
    for x in v.tolist():
        s = s + np.float64(x)
    return s


def gsea(w, set_ptr, set_genes, score_type=0, nperm=1000, seed=0):
    """The whole test: a dict of P x k arrays es, nes, pval, padj, n_ge, n_le, n_side, with set_size (P) and null (k x sizes x nperm)."""
    w = np.asarray(w, dtype=np.float64)
    m, k = w.shape
    set_ptr = np.asarray(set_ptr, dtype=np.int64)
    P = set_ptr.shape[0] - 1
    size = np.diff(set_ptr)
    sizes = np.unique(size)
    size_idx = np.searchsorted(sizes, size)
    es = observed(w, set_ptr, set_genes)[score_type]
    null = null_scores(w, sizes, score_type, seed, 0, nperm)
    out = {k_: np.zeros((P, k), dtype=np.int64) for k_ in ("n_ge", "n_le", "n_side")}
    out.update({k_: np.full((P, k), np.nan) for k_ in ("nes", "pval", "padj")})
    out.update(es=es, set_size=size, null=null, sizes=sizes)
    for f in range(k):
        for si in range(sizes.shape[0]):
            v = null[f, si]
            up, dn = v[v >= 0.0], v[v <= 0.0]
            sums = (running_sum(up), running_sum(dn))
            for j in np.nonzero(size_idx == si)[0]:
                e = es[j, f]
                ge, le = int((v >= e).sum()), int((v <= e).sum())
                upper = score_type == 0 or (score_type == 2 and e >= 0.0)
                side = up.size if upper else dn.size
                hits = ge if upper else le
                out["n_ge"][j, f], out["n_le"][j, f], out["n_side"][j, f] = ge, le, side
                out["pval"][j, f] = np.float64(1 + hits) / np.float64(1 + (side if score_type == 2 else nperm))
                if side > 0:
                    mean = sums[0 if upper else 1] / np.float64(side)
                    if mean != 0.0:
                        out["nes"][j, f] = e / abs(mean)
        out["padj"][:, f] = bh(out["pval"][:, f])
    return out


# ---------------------------------------------------------------------------------------------- independent yardsticks
def textbook_es(wf, genes):
    """(max, min) of the running sum of the textbook walk over ALL m genes in ranking order: + |w| / NR on a hit, - 1 / (m - s) on
    a miss, the minimum taken before a hit's step as well (0 at the start); with NR == 0 every hit steps 1 / s."""
    wf = np.asarray(wf, dtype=np.float64)
    m = wf.shape[0]
    order = np.argsort(-wf, kind="stable")
    member = np.zeros(m, dtype=bool)
    member[np.asarray(genes)] = True
    s = int(member.sum())
    NR = float(np.abs(wf[member]).sum())
    run, hi, lo = 0.0, -np.inf, np.inf
    for g in order.tolist():
        if member[g]:
            lo = min(lo, run)
            run += (abs(wf[g]) / NR) if NR > 0.0 else 1.0 / s
            hi = max(hi, run)
        else:
            run -= 1.0 / (m - s)
    return hi, lo


def bh_plain(p):
    """The O(P^2) definition: padj_j = min(1, min over j' with p_j' >= p_j of p_j' n / rank(j')), rank = the number of p <= p_j'."""
    p = np.asarray(p, dtype=np.float64)
    ok = ~np.isnan(p)
    n = int(ok.sum())
    out = np.full(p.shape, np.nan)
    for j in np.nonzero(ok)[0]:
        best = 1.0
        for q in np.nonzero(ok)[0]:
            if p[q] >= p[j]:
                best = min(best, p[q] * n / int((p[ok] <= p[q]).sum()))
        out[j] = best
    return out
