"""The rules of sgl_markers (include/singlet_hip.h, "Marker genes") restated operation by operation in numpy: the entry
classes, the doubled midranks and the tie term of a gene (integers), the group sums in their stated order (segments of
8192, blocks of 64, the butterfly, ascending additions from +0.0) and the derived statistics.  A gene is given as its
stored entries in stored order: the values x and the cells they sit in.  Nothing here is tuned to the device's output."""
import math

import numpy as np

SEG = 8192
BLOCK = 64
MAX_CELLS = 1 << 21
MAX_GROUPS = 1024


def group_counts(labels, G):
    """(group_n, N): the cells of every cluster and the included cells."""
    labels = np.asarray(labels)
    group_n = np.bincount(labels[labels >= 0], minlength=G).astype(np.int64)
    return group_n, int(group_n.sum())


def entry_counts(x, cells, labels, G):
    """(pos, nz) of one gene, G values each: the stored x > 0 and the stored x != 0 per cluster, included cells only."""
    l = np.asarray(labels)[cells]
    pos = np.bincount(l[(l >= 0) & (x > 0)], minlength=G).astype(np.int64)
    nz = np.bincount(l[(l >= 0) & (x != 0)], minlength=G).astype(np.int64)
    return pos, nz


def ranks(x, cells, labels, G):
    """(rank2 (G, int64), tie (Python int)) of one gene."""
    labels = np.asarray(labels)
    group_n, N = group_counts(labels, G)
    l = labels[cells]
    take = (l >= 0) & (x != 0)          # a stored zero of either sign joins the implicit zeros
    v, l = x[take], l[take]
    order = np.argsort(v, kind="stable")
    v, l = v[order], l[order]
    L = v.shape[0]
    Z = N - L                           # the zero block
    neg = int(np.sum(v < 0))
    rank2 = np.zeros(G, dtype=np.int64)
    tie = 0
    if L:
        head = np.ones(L, dtype=bool)
        head[1:] = v[1:] != v[:-1]
        starts = np.nonzero(head)[0]
        ends = np.append(starts[1:], L)
        run = np.cumsum(head) - 1
        shift = np.where(v > 0, Z, 0)   # the positives sit above the zero block
        a = starts[run] + shift
        b = ends[run] + shift
        np.add.at(rank2, l, (a + b + 1).astype(np.int64))
        for t in (ends - starts).tolist():
            tie += t * t * t - t
    nz = np.bincount(l, minlength=G).astype(np.int64)
    rank2 += (group_n - nz) * (2 * neg + Z + 1)   # the zero block [neg, neg + Z) is one run
    tie += Z * Z * Z - Z
    return rank2, tie


def _butterfly(V):
    """Rows of 64 lane values -> the butterfly sum every lane ends with (lane ^ 32, 16, 8, 4, 2, 1); column 0 is taken."""
    lane = np.arange(BLOCK)
    for off in (32, 16, 8, 4, 2, 1):
        V = V + V[:, lane ^ off]
    return V[:, 0]


def group_sums(x, cells, labels, G, transform, skip_empty_blocks=False):
    """sum (G doubles) of one gene in the stated order.  skip_empty_blocks: blocks without a member of c are left out of the
    additions (allowed: the bits are the same, which tests/test_markers_restatement.py holds)."""
    l = np.asarray(labels)[cells]
    f = np.expm1(x) if transform else np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    nb = (n + BLOCK - 1) // BLOCK
    F = np.zeros(nb * BLOCK)
    Lb = np.full(nb * BLOCK, -1, dtype=np.int64)   # a lane past the end holds no member
    F[:n], Lb[:n] = f, l
    F, Lb = F.reshape(nb, BLOCK), Lb.reshape(nb, BLOCK)
    per_seg = SEG // BLOCK
    out = np.zeros(G)
    for c in range(G):
        member = Lb == c
        if not member.any():   # every partial is +0.0, and so is their sum
            continue
        part = _butterfly(np.where(member, F, 0.0))
        present = member.any(axis=1)
        total = 0.0
        for s0 in range(0, nb, per_seg):
            seg = 0.0
            for blk in range(s0, min(s0 + per_seg, nb)):
                if skip_empty_blocks and not present[blk]:
                    continue
                seg = seg + part[blk]
            total = total + seg
        out[c] = total
    return out


def group_sums_reference(x, cells, labels, G, transform):
    """The same sums in long double, any order: (reference (G long doubles), the entries summed per cluster)."""
    l = np.asarray(labels)[cells]
    f = np.expm1(x.astype(np.longdouble)) if transform else x.astype(np.longdouble)
    return (np.array([f[l == c].sum(dtype=np.longdouble) for c in range(G)], dtype=np.longdouble),
            np.array([int(np.sum(l == c)) for c in range(G)], dtype=np.int64))


def derive(group_n, pos, sums, rank2, tie, pseudocount):
    """The derived statistics of one gene against every cluster: dict of G-vectors pct_in, pct_out, log2fc, z, p."""
    G = len(group_n)
    N = int(np.sum(group_n))
    out = {}
    dN = np.float64(N)
    n1 = np.asarray(group_n, dtype=np.int64)           # every line below is the same operation for all clusters c at once
    n2 = N - n1
    d1, d2 = n1.astype(np.float64), n2.astype(np.float64)
    pos = np.asarray(pos, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["pct_in"] = pos.astype(np.float64) / d1
        out["pct_out"] = (int(pos.sum()) - pos).astype(np.float64) / d2
        s_out = np.zeros(G)                            # S_out of c: the sums of c' != c added in ascending c' from +0.0
        for o in range(G):
            others = np.arange(G) != o
            s_out[others] = s_out[others] + sums[o]
        mean_in, mean_out = sums / d1, s_out / d2
        out["log2fc"] = np.log2(mean_in + np.float64(pseudocount)) - np.log2(mean_out + np.float64(pseudocount))
        U2 = np.asarray(rank2, dtype=np.int64) - n1 * (n1 + 1)
        D = U2 - n1 * n2
        var = (d1 * d2 / np.float64(12.0)) * ((dN + np.float64(1.0)) - np.float64(np.uint64(tie)) / (dN * (dN - np.float64(1.0))))
        ok = (n1 != 0) & (n2 != 0) & (var > 0)
        a = np.abs(D).astype(np.float64) / np.float64(2.0) - np.float64(0.5)
        a = np.where(a < 0, np.float64(0.0), a)
        zz = a / np.sqrt(var)
        out["z"] = np.where(ok, np.where(D < 0, -zz, zz), np.nan)
        arg = zz * np.float64(0.7071067811865476)      # M_SQRT1_2
        out["p"] = np.array([math.erfc(float(v)) if good else math.nan for v, good in zip(arg, ok)])
    return out


def check_args(labels, ncol, G, transform, pseudocount):
    """None when sgl_markers accepts the arguments, else (what, position, value) of the first refusal in the library's order."""
    if labels is None:
        return ("null", -1, 0)
    if G < 1 or G > MAX_GROUPS:
        return ("groups", -1, 0)
    if transform not in (0, 1):
        return ("transform", -1, 0)
    if not (pseudocount >= 0.0) or not (pseudocount < math.inf):
        return ("pseudocount", -1, 0)
    if ncol < 0 or ncol > MAX_CELLS:
        return ("cells", -1, 0)
    for j in range(ncol):
        if labels[j] < -1 or labels[j] >= G:
            return ("label", j, int(labels[j]))
    return None


def gene_entries(Tx, Ti, Tp, g):
    """(x, cells) of gene g from the CSC arrays of t(A) (one column per gene)."""
    return np.asarray(Tx[Tp[g]:Tp[g + 1]], dtype=np.float64), np.asarray(Ti[Tp[g]:Tp[g + 1]], dtype=np.int64)


def markers(Tx, Ti, Tp, labels, G, transform=1, pseudocount=1.0):
    """Everything sgl_markers returns, m x G (tie: m, as uint64), from the CSC arrays of t(A)."""
    m = len(Tp) - 1
    group_n, _ = group_counts(labels, G)
    out = {k: np.zeros((m, G), dtype=np.int64) for k in ("pos", "nz", "rank2")}
    out.update({k: np.zeros((m, G)) for k in ("sum", "pct_in", "pct_out", "log2fc", "z", "p")})
    out["tie"] = np.zeros(m, dtype=np.uint64)
    out["group_n"] = group_n
    for g in range(m):
        x, cells = gene_entries(Tx, Ti, Tp, g)
        out["pos"][g], out["nz"][g] = entry_counts(x, cells, labels, G)
        out["rank2"][g], tie = ranks(x, cells, labels, G)
        out["tie"][g] = np.uint64(tie)
        out["sum"][g] = group_sums(x, cells, labels, G, transform, skip_empty_blocks=True)
        d = derive(group_n, out["pos"][g], out["sum"][g], out["rank2"][g], tie, pseudocount)
        for k, v in d.items():
            out[k][g] = v
    return out
