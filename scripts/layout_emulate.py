#!/usr/bin/env python3
"""Host model of the entry-stream layout (kernels_tiled.hip: tiled_count_kernel) -- the sliding-window schedule, stored entries
per non-zero for a CSC matrix.  `stream_counts` returns the same group counts the device writes (balance=True: the device
default, the eight wave blocks of a workgroup level their chunks of a stage; balance=False: SGL_TILED_NO_BALANCE=1, the
rule before it); `entries` their total in stored entries, which is what sgl_layout_get reports.  Usage: layout_emulate.py [pbmc3k | iid M N INV] k"""
import sys
import os
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 160 * 1024 - 512


def tile_rows(k, nsl):
    """LDS-sized tile rows of the build (before the small-matrix shortening)"""
    KS = 32 if nsl == 4 else (k + 1) & ~1
    return min(LDS_BYTES // (KS * 8) // 8 * 8, 984)


def sorted_perm(p):
    """column order of the stream: descending non-zero count, ties in matrix order"""
    return np.argsort(-np.diff(np.asarray(p, dtype=np.int64)), kind="stable")


def block_ranges(T, nb, nr):
    """row-block ranges [b0, b1) of the nr tile ranges (floor / ceil of T / nr tiles each, two blocks per tile)"""
    return [(2 * (y * T // nr), min(2 * ((y + 1) * T // nr), nb)) for y in range(nr)]


def level_spread(f, E):
    """Run-ahead groups of the balance rule: spread E groups level over units that can take f[..., p] of them.  t = the largest
    level with sum(min(f, t)) <= E; unit p gets min(f_p, t), what is left goes one each to the highest-numbered units with
    f_p > t.  Where sum(f) <= E every unit gets f_p.  f: (waves, 32), E: (waves,)"""
    ts = np.arange(256, dtype=np.int64)
    S = np.minimum(f[:, None, :], ts[None, :, None]).sum(axis=2)          # S[w, t], non-decreasing in t
    t = (S <= E[:, None]).sum(axis=1) - 1
    add = np.minimum(f, t[:, None])
    left = E - add.sum(axis=1)
    hot = f > t[:, None]
    above = np.cumsum(hot[:, ::-1], axis=1)[:, ::-1] - hot                # hot units numbered higher than p
    return add + (hot & (above < left[:, None]))


def stream_counts(p, i, nrow, TR, nsl, ranges=1, order="sorted", tail_wg0=-1, tail_R=1, trace=None, balance=True):
    """Group counts cnt[wb, b, pair] of the sliding-window stream (b = row block of D = TR / 2 rows = the stage).

    In stage b the LDS holds blocks b and b + 1 of the range; every column finishes its entries in block b and may run ahead
    into block b + 1.  Per pair: n = the larger number of entries left in block b over its nsl columns, rounded up to
    groups of four; every column takes min(n, entries left in the window) real entries, pads for the rest.
    balance (the device default; False = SGL_TILED_NO_BALANCE=1, the rule before it): the eight wave blocks of a workgroup
    meet at a barrier after every stage, so the stage lasts as long as its longest chunk.  target = the largest of their
    chunks of must groups, in whole sets; a wave block short of it takes the difference as run-ahead, but only groups that
    hold real entries for every present column of the unit (f = floor(least window entries left / 4) - must), spread level
    over the units (level_spread).  A wave block that cannot reach the target stays short.
    The chunk (wave block, stage) is then rounded up to whole 64-slot sets by extra groups on the last pairs, each taking
    as many as its columns still have run-ahead entries for; what is left goes on pair 31 as pads.
    trace: a list that receives (col, first entry, entries, b) for every run of real entries."""
    p = np.asarray(p, dtype=np.int64)
    i = np.asarray(i, dtype=np.int64)
    ncol = p.size - 1
    D = TR // 2
    T = (nrow + TR - 1) // TR
    nb = (nrow + D - 1) // D
    CW = 32 * nsl
    nwb = (ncol + CW - 1) // CW
    gps = 16 // nsl
    perm = sorted_perm(p) if order == "sorted" else np.arange(ncol)
    # seg[b, c] = first entry of column c at or below row b * D
    col_of = np.repeat(np.arange(ncol), np.diff(p))
    per = np.zeros((nb + 1, ncol + 1), dtype=np.int64)
    np.add.at(per, (i // D + 1, col_of), 1)
    seg = p[:-1][None, :] + np.cumsum(per, axis=0)[:, :ncol]
    # slot (wb, pair, h) -> column (-1: none); seg of an absent column is 0 everywhere
    slot = np.full(nwb * CW, -1, dtype=np.int64)
    slot[:ncol] = perm
    slot = slot.reshape(nwb, 32, nsl)
    present = slot >= 0
    sc = np.where(present, slot, 0)
    cnt = np.zeros((nwb, nb, 32), dtype=np.int64)
    for wg in range((nwb + 7) // 8):            # a workgroup: eight consecutive wave blocks (fewer in the last one)
        w0, w1 = 8 * wg, min(8 * wg + 8, nwb)
        nr = tail_R if (tail_R > 1 and tail_wg0 >= 0 and wg >= tail_wg0) else ranges
        nr = max(1, min(nr, T))
        cols, pres = sc[w0:w1], present[w0:w1]
        for b0, b1 in block_ranges(T, nb, nr):
            if b0 >= b1:
                continue
            pos = np.where(pres, seg[b0][cols], 0)
            for b in range(b0, b1):
                hi = min(b + 2, b1)
                end_b = np.where(pres, seg[b + 1][cols], 0)
                end_w = np.where(pres, seg[hi][cols], 0)
                g = (np.max(end_b - pos, axis=2) + 3) // 4
                if balance:
                    tot = g.sum(axis=1)
                    target = gps * np.max((tot + gps - 1) // gps)
                    fmin = np.min(np.where(pres, end_w - pos, np.iinfo(np.int64).max), axis=2) // 4
                    f = np.where(pres.any(axis=2), np.maximum(fmin - g, 0), 0)
                    g = g + level_spread(f, target - tot)
                cap = (np.max(end_w - pos, axis=2) + 3) // 4 - g
                for w in range(w1 - w0):
                    rem = (-int(g[w].sum())) % gps
                    for q in range(31, -1, -1):
                        if rem == 0:
                            break
                        e = min(int(cap[w, q]), rem)
                        g[w, q] += e
                        rem -= e
                    g[w, 31] += rem
                take = np.minimum(4 * g[:, :, None], end_w - pos)
                if trace is not None:
                    for w, q, h in zip(*np.nonzero(pres & (take > 0))):
                        trace.append((int(cols[w, q, h]), int(pos[w, q, h]), int(take[w, q, h]), b))
                pos = pos + take
                cnt[w0:w1, b] = g
            assert np.array_equal(pos[pres], seg[b1][cols][pres]), "a column left entries behind"
    assert cnt.max(initial=0) <= 255, "a unit's groups must fit the byte of cnt"
    return cnt


def entries(p, i, nrow, k, nsl=2, TR=None, **kw):
    """stored entries of the stream (all column slots, pads included)"""
    TR = TR or tile_rows(k, nsl)
    return int(stream_counts(p, i, nrow, TR, nsl, **kw).sum()) * 4 * nsl


def lockstep_entries(p, i, nrow, TR, nsl, order="sorted"):
    """the previous rule for comparison: runs padded to equal length per tile of TR rows, chunks of (wave block, tile)"""
    p = np.asarray(p, dtype=np.int64)
    ncol = p.size - 1
    T = (nrow + TR - 1) // TR
    col_of = np.repeat(np.arange(ncol), np.diff(p))
    c = np.zeros((ncol, T), dtype=np.int64)
    np.add.at(c, (col_of, np.asarray(i) // TR), 1)
    perm = sorted_perm(p) if order == "sorted" else np.arange(ncol)
    CW = 32 * nsl
    nwb = (ncol + CW - 1) // CW
    pad = np.zeros((nwb * CW, T), dtype=np.int64)
    pad[:ncol] = c[perm]
    g = (pad.reshape(nwb, 32, nsl, T).max(axis=2) + 3) // 4
    tot = g.sum(axis=1)
    tot += (-tot) % (16 // nsl)
    return int(tot.sum()) * 4 * nsl


def transpose(p, i, nrow):
    p = np.asarray(p, dtype=np.int64)
    col_of = np.repeat(np.arange(p.size - 1), np.diff(p))
    o = np.argsort(i, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nrow))]).astype(np.int64), col_of[o]


def main():
    a = sys.argv[1:]
    if a[0] == "pbmc3k":
        z = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
        p, dim = z["p"].astype(np.int64), z["dim"]
        i = z["di"].astype(np.int64)          # row indices are delta-coded per column in the fixture
        for c in range(int(dim[1])):
            i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
        nrow, ncol = int(dim[0]), int(dim[1])
        k = int(a[1])
    else:
        m, n, inv, k = int(a[1]), int(a[2]), int(a[3]), int(a[4])
        rng = np.random.default_rng(0)
        D = rng.random((m, n)) < 1.0 / inv
        i = np.nonzero(D.T)[1].astype(np.int64)
        p = np.concatenate([[0], np.cumsum(D.sum(axis=0))]).astype(np.int64)
        nrow, ncol = m, n
    nnz = int(p[-1])
    tp, ti = transpose(p, i, nrow)
    for nsl in ((4, 2) if k <= 32 else (2,)):
        TR = tile_rows(k, nsl)
        for name, (pp, ii, nr) in {"H side (columns = cells)": (p, i, nrow), "W side (columns = genes)": (tp, ti, ncol)}.items():
            old = lockstep_entries(pp, ii, nr, TR, nsl)
            new = entries(pp, ii, nr, k, nsl, TR)
            print("%-26s k=%-3d nsl=%d TR=%-3d entries/nnz: lock-step tiles %.3f, sliding window %.3f" % (name, k, nsl, TR, old / nnz, new / nnz))


if __name__ == "__main__":
    main()
