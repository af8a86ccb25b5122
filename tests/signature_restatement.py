"""The rules of sgl_signature_scores (include/singlet_hip.h, "Signature scores") restated in numpy: the descending order within a
cell with its closed zero block and shifted negatives, the doubled midranks and their cap, the rank sums of the sets, the
score, and the host plan (the argument rules, the gene -> sets table, the paths, the batches, the set passes).  All integer
arithmetic up to the score; the GPU tests compare with array_equal.  Nothing here imports the library."""
import numpy as np

LDS_SMALL = 1024
LDS_CAP = 4096
PASS_SETS = 1024
BATCH_ENTRIES = 1 << 27


def cap_rank(r2, R):
    """r2' = r2 when r2 <= 2 R, else 2 R + 2 (uint64 arrays or ints)."""
    r2 = np.asarray(r2, dtype=np.uint64)
    return np.where(r2 <= np.uint64(2 * R), r2, np.uint64(2 * R + 2))


def cell_ranks(x, m, R):
    """The stored entries x (any order, zeros of either sign among them) of one cell of m genes.  Returns (r2' per stored
    entry as uint64, z2: the zero block's value or 0 when Z = 0, z2 whatever Z, P, N)."""
    x = np.asarray(x, dtype=np.float64)
    pos, neg = x > 0, x < 0
    P, N = int(pos.sum()), int(neg.sum())
    Z = m - P - N
    z2 = int(cap_rank(2 * P + Z + 1, R))
    out = np.full(x.shape[0], z2, dtype=np.uint64)
    for mask, first, shift in ((pos, 0, 0), (neg, P, Z)):
        v = x[mask]
        if v.size == 0:
            continue
        # descending: position of a value = the number of values of this sign above it; the positives start at 0, the
        # negatives behind the P positives (and the zero block, the shift)
        u, inv, cnt = np.unique(-v, return_inverse=True, return_counts=True)   # ascending -v = descending v
        start = np.concatenate(([0], np.cumsum(cnt)[:-1])) + first
        a = start[inv]
        b = a + cnt[inv]
        out[mask] = cap_rank((a + b + 1 + 2 * shift).astype(np.uint64), R)
    return out, (z2 if Z > 0 else 0), z2, P, N


def matrix_cell_ranks(Ax, Ap, m, R):
    """sgl_op_cell_ranks of a CSC matrix: (rank2_entry in storage order, zero2 per cell)."""
    n = len(Ap) - 1
    entry = np.zeros(len(Ax), dtype=np.uint64)
    zero2 = np.zeros(n, dtype=np.uint64)
    for c in range(n):
        lo, hi = int(Ap[c]), int(Ap[c + 1])
        entry[lo:hi], zero2[c], _, _, _ = cell_ranks(Ax[lo:hi], m, R)
    return entry, zero2


def score_of(rank2, n_s, R):
    """score = 1.0 - (double)(rank2 - n_s (n_s + 1)) / (2.0 * n_s * R), elementwise."""
    rank2 = np.asarray(rank2, dtype=np.uint64)
    n_s = np.asarray(n_s, dtype=np.uint64)
    num = (rank2 - n_s * (n_s + np.uint64(1))).astype(np.float64)
    return 1.0 - num / (2.0 * n_s.astype(np.float64) * float(R))


def scores(Ax, Ai, Ap, m, sets, R):
    """(rank2 uint64, score float64), each n_sets x ncol, of a CSC matrix."""
    n = len(Ap) - 1
    S = len(sets)
    rank2 = np.zeros((S, n), dtype=np.uint64)
    sizes = np.array([len(s) for s in sets], dtype=np.uint64)
    Ai = np.asarray(Ai)
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in sets])
    first = np.concatenate(([0], np.cumsum(sizes.astype(np.int64))[:-1]))   # (no set is empty)
    for c in range(n):
        lo, hi = int(Ap[c]), int(Ap[c + 1])
        r, _, z2, _, _ = cell_ranks(Ax[lo:hi], m, R)
        dense = np.full(m, z2, dtype=np.uint64)     # every gene's r2': the zero block's unless it is stored
        dense[Ai[lo:hi]] = r
        rank2[:, c] = np.add.reduceat(dense[flat], first)
    return rank2, score_of(rank2, sizes[:, None], R)


def dense_rank2(col, R):
    """The doubled capped midranks of one dense cell from scipy's rankdata(-col, "average"): the independent form."""
    from scipy.stats import rankdata
    r = rankdata(-np.asarray(col, dtype=np.float64), method="average")
    r2 = np.rint(2.0 * r).astype(np.uint64)
    return cap_rank(r2, R)


# ------------------------------------------------------------------------------------------ the host plan
def check_args(set_ptr, set_genes, n_sets, m, max_rank, lds_cap=0, max_batch_entries=0, pass_sets=0):
    """None, or the first defect as (kind, at, val), in the library's order."""
    if set_ptr is None or set_genes is None:
        return ("null", -1, 0)
    if n_sets < 1:
        return ("sets", -1, n_sets)
    if max_rank < 1 or max_rank > m:
        return ("rank", -1, max_rank)
    for at, v in enumerate((lds_cap, max_batch_entries, pass_sets)):
        if v < 0:
            return ("knob", at, v)
    if set_ptr[0] != 0:
        return ("ptr", 0, int(set_ptr[0]))
    for j in range(n_sets):
        s = int(set_ptr[j + 1]) - int(set_ptr[j])
        if s < 0:
            return ("ptr", j + 1, int(set_ptr[j + 1]))
        if s == 0:
            return ("empty", j, 0)
        if s > max_rank:
            return ("size", j, s)
    for j in range(n_sets):
        seen = set()
        for q in range(int(set_ptr[j]), int(set_ptr[j + 1])):
            g = int(set_genes[q])
            if g < 0 or g >= m:
                return ("gene", q, g)
            if g in seen:
                return ("twice", q, g)
            seen.add(g)
    return None


def gene_table(sets, m):
    """(gene_ptr int64 m + 1, gene_sets int32): the sets that hold every gene, ascending."""
    per = [[] for _ in range(m)]
    for j, s in enumerate(sets):
        for g in s:
            per[int(g)].append(j)
    ptr = np.zeros(m + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(p) for p in per])
    flat = np.array([j for p in per for j in p], dtype=np.int32)
    return ptr, flat


def lds_cap(knob):
    return knob if 0 < knob < LDS_CAP else LDS_CAP


def pass_size(knob):
    return knob if 0 < knob < PASS_SETS else PASS_SETS


def passes(n_sets, knob):
    return -(-n_sets // pass_size(knob))


def split_paths(lens, knob):
    """(small, large, long) cell lists under the lds_cap knob."""
    cap = lds_cap(knob)
    small = min(cap, LDS_SMALL)
    lens = np.asarray(lens)
    idx = np.arange(lens.shape[0])
    return idx[lens <= small], idx[(lens > small) & (lens <= cap)], idx[lens > cap]


def batch_cap(knob):
    return min(knob if knob > 0 else BATCH_ENTRIES, 2**31 - 1)


def batches(lens, knob):
    """The greedy rule: whole cells in order, a batch at most the cap; a cell above the cap alone.  Returns the cut list."""
    cap = batch_cap(knob)
    cut, s, n = [0], 0, len(lens)
    while s < n:
        tot, e = int(lens[s]), s + 1
        while e < n and int(lens[e]) <= cap - tot:
            tot += int(lens[e])
            e += 1
        cut.append(e)
        s = e
    return cut
