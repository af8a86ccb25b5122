"""The rules of the neighbourhood enrichment test (include/singlet_hip.h, "Neighbourhood enrichment") restated in numpy and
Python integers: TEST INFRASTRUCTURE ONLY.  Everything up to the statistics is an integer, so a correct kernel gives the same
values; the statistics use Python's exact integers and ONE correctly rounded conversion (float(int) rounds to nearest even),
one sqrt and one division each.

Layouts follow the Python layer: tables are K x K with [a, b] = centre class a (the column's cell), neighbour class b (the
row's cell); the null tensor is nperm x K x K."""
import math

import numpy as np

from gsea_restatement import bh, rand2

U64 = np.uint64
MAX_K = 256
MAX_NPERM = 1 << 20
MAX_PG = 16
LDS_TILE_BYTES = 128 << 10
SEG = 4096
SORT_SWITCH = 32768
BATCH_BYTES = 256 << 20


def columns(Gp):
    """The column of every stored entry."""
    Gp = np.asarray(Gp, dtype=np.int64)
    return np.repeat(np.arange(Gp.shape[0] - 1, dtype=np.int64), np.diff(Gp))


def tally(Gi, Gp, lab, K, drop_diagonal=True):
    """C[a, b] = the number of counted stored entries (row i, column j) with lab[j] == a and lab[i] == b; int64."""
    Gi, lab = np.asarray(Gi, dtype=np.int64), np.asarray(lab, dtype=np.int64)
    col = columns(Gp)
    keep = Gi != col if drop_diagonal else np.ones(Gi.shape[0], dtype=bool)
    flat = np.bincount(lab[col[keep]] * K + lab[Gi[keep]], minlength=K * K)
    return flat.reshape(K, K).astype(np.int64)


def order(seed, r, n):
    """The cells ascending by (key(r, c), c)."""
    key = rand2(seed, np.full(n, r, dtype=U64), np.arange(n, dtype=U64))
    return np.lexsort((np.arange(n), key))


def permuted(lab, seed, r0, nb):
    """lab_r of the permutations [r0, r0 + nb): nb x n."""
    lab = np.asarray(lab)
    return np.stack([lab[order(seed, r, lab.shape[0])] for r in range(r0, r0 + nb)])


def null(Gi, Gp, lab, K, nperm, seed, drop_diagonal=True):
    """C_r of every permutation: nperm x K x K."""
    return np.stack([tally(Gi, Gp, row, K, drop_diagonal) for row in permuted(lab, seed, 0, nperm)])


def tallies(C, N):
    """{"counts", "S1", "S2", "n_ge", "n_le"} of the observed counts C and the null tensor N, in Python integers held as int64."""
    N = np.asarray(N, dtype=np.int64)
    return {"counts": np.asarray(C, dtype=np.int64), "S1": N.sum(axis=0), "S2": (N * N).sum(axis=0), "n_ge": (N >= C[None]).sum(axis=0).astype(np.int64),
            "n_le": (N <= C[None]).sum(axis=0).astype(np.int64)}


def stats(nperm, counts, S1, S2, n_ge, n_le):
    """The statistics from the integer tallies, pair by pair in exact integers."""
    K = counts.shape[0]
    out = {name: np.zeros((K, K)) for name in ("zscore", "mean", "sd", "p_enriched", "p_depleted")}
    for a in range(K):
        for b in range(K):
            c, s1, s2 = int(counts[a, b]), int(S1[a, b]), int(S2[a, b])
            D = nperm * s2 - s1 * s1
            root = math.sqrt(float(D))
            out["mean"][a, b] = float(s1) / float(nperm)
            out["sd"][a, b] = root / float(nperm)
            out["zscore"][a, b] = float(nperm * c - s1) / root if D != 0 else math.nan
            out["p_enriched"][a, b] = float(1 + int(n_ge[a, b])) / float(1 + nperm)
            out["p_depleted"][a, b] = float(1 + int(n_le[a, b])) / float(1 + nperm)
    # Benjamini-Hochberg over the K^2 pairs in the library's order of the pairs: a + K b ascending
    for p, q in (("p_enriched", "p_adj_enriched"), ("p_depleted", "p_adj_depleted")):
        out[q] = bh(out[p].T.reshape(-1)).reshape(K, K).T
    return out


def enrichment(Gi, Gp, lab, K, nperm, seed, drop_diagonal=True):
    """The whole call: the tallies, the null tensor and the statistics."""
    C = tally(Gi, Gp, lab, K, drop_diagonal)
    N = null(Gi, Gp, lab, K, nperm, seed, drop_diagonal)
    t = tallies(C, N)
    out = dict(t, null=N)
    out.update(stats(nperm, **t))
    return out


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def pg_max(K):
    for pg in (16, 8, 4, 2, 1):
        if pg * K * K * 4 <= LDS_TILE_BYTES:
            return pg
    return 0


def plan(n, K, nperm, batch=0, path=0, pg=0, sort_switch=0):
    """{"path", "perms_per_group", "lds_bytes", "batch", "sort"} as nhood_host.h plans it."""
    cap = pg_max(K)
    p = 2 if path == 2 or cap == 0 else 1
    g = pg if pg else (cap if p == 1 else MAX_PG)
    if batch == 0:
        batch = max(BATCH_BYTES // (n + 8 * K * K) // MAX_PG * MAX_PG, MAX_PG)
    return {"path": p, "perms_per_group": g, "lds_bytes": g * K * K * 4 if p == 1 else 0, "batch": min(batch, nperm),
            "sort": int(n > (sort_switch or SORT_SWITCH))}


# ---- fixtures shared by the CPU and the GPU tests ---------------------------------------------------------------------------------
def grid_graph(side_x, side_y):
    """The 8-neighbour graph of a side_x x side_y grid (cell = x + side_x * y), rows ascending: (Gi, Gp)."""
    n = side_x * side_y
    x, y = np.arange(n) % side_x, np.arange(n) // side_x
    rows, cols = [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            ok = (x + dx >= 0) & (x + dx < side_x) & (y + dy >= 0) & (y + dy < side_y)
            cols.append(np.nonzero(ok)[0])
            rows.append((x + dx + side_x * (y + dy))[ok])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    o = np.lexsort((rows, cols))
    Gp = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=n))))
    return rows[o].astype(np.int32), Gp.astype(np.int32)


def planted(side=24):
    """The planted fixture: a side x side grid, 8-neighbour graph, label 2 where x >= side / 2 and (x + y) % 2 elsewhere."""
    n = side * side
    x, y = np.arange(n) % side, np.arange(n) // side
    lab = np.where(x >= side // 2, 2, (x + y) % 2).astype(np.int32)
    Gi, Gp = grid_graph(side, side)
    return Gi, Gp, lab


PLANTED_COUNTS = [[506, 540, 35], [540, 506, 35], [35, 35, 2092]]


def planted_claims(out, nperm=200):
    """What the planted fixture must show, on the restatement and on the device alike: the checkerboard classes 0 and 1 are
    neighbours far more often than chance, both avoid the block of class 2, which keeps to itself."""
    assert np.asarray(out["counts"]).tolist() == PLANTED_COUNTS
    z = out["zscore"]
    assert z[0, 1] >= 8 and z[0, 2] <= -15 and z[2, 2] >= 15, z
    assert out["n_ge"][0, 2] == nperm and out["n_ge"][0, 1] == 0 and out["n_ge"][2, 2] == 0
