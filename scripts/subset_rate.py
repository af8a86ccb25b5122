#!/usr/bin/env python3
"""Time sgl_subset (kernels_subset.hip) against the route it replaces.  Writes one JSON line to profiles/subset_rate.json
(and prints it).

On sgl_synth_csc 30 000 x 200 000 at 5 % (3.0e8 entries) two selections are timed, each once after a small warm-up:
2 000 random genes (`rows`: a column gather of t(A), then the transpose back to A) and 20 000 random cells (`cols`: a
column gather of A, then the transpose to t(A)).  Per selection:
  (a) gather_ms     the gather (lengths, scan, copy) between the context's hipEvents (booked under the "scale" phase);
  (b) transpose_ms  the device transpose that follows (the library's own wall clock around the synchronised call);
  (c) subset_ms     the whole sgl_subset call, wall clock (validation loop, frees, (a), (b), the column counts);
  (d) replaced_ms   download -> NumPy subset -> upload on a second context (the upload transposes and validates again),
                    with its three parts.
gather_bytes is the HBM model of (a): every kept entry read once and written once (12 B each way), plus the offsets read
and written and the index list; gather_GB_per_s = gather_bytes / (a)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "subset_rate.json")
GENES, CELLS = 30000, 200000


def host_subset(sa, x, i, p, nrow, rows, cols):
    """A[rows, ] or A[, cols] of the downloaded slots in NumPy (the selections here are ascending, so a row subset is a filter)."""
    if cols is not None:
        ln = np.diff(p)[cols]
        pn = np.concatenate([[0], np.cumsum(ln)])
        src = np.repeat(p[cols] - pn[:-1], ln) + np.arange(int(pn[-1]), dtype=np.int64)
        return sa.dgCMatrix(x[src], i[src], pn.astype(np.int32), (nrow, cols.size))
    new = np.full(nrow, -1, dtype=np.int32)
    new[rows] = np.arange(rows.size, dtype=np.int32)
    ni = new[i]
    keep = ni >= 0
    pn = np.concatenate([[0], np.cumsum(keep)])[p]
    return sa.dgCMatrix(x[keep], ni[keep], pn.astype(np.int32), (rows.size, p.size - 1))


def one(sa, name, rows, cols):
    c = sa.Context(0)
    try:
        c.synth(GENES, CELLS, 20)
        nnz_in = c.dims()[2]
        c.timing_enable(True)
        c.timing_get(reset=True)
        tr0 = sa.call_times()["transpose_s"]
        t = time.perf_counter()
        c.subset(rows, cols)
        subset_ms = 1e3 * (time.perf_counter() - t)
        gather_ms = c.timing_get(reset=True)["scale"][0]
        transpose_ms = 1e3 * (sa.call_times()["transpose_s"] - tr0)
        nrow, ncol, nnz_out = c.dims()
        got = c.download(0)
        # the route this replaces, from a resident matrix again
        c.synth(GENES, CELLS, 20)
        t0 = time.perf_counter()
        x, i, p = c.download(0)
        t1 = time.perf_counter()
        S = host_subset(sa, x, i, p, GENES, rows, cols)
        t2 = time.perf_counter()
        c.upload(S, None)
        t3 = time.perf_counter()
        ref = c.download(0)
        same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, ref))
    finally:
        c.close()
    n_sel = rows.size if rows is not None else cols.size
    gather_bytes = 24.0 * nnz_out + 16.0 * n_sel + 8.0 * (n_sel + 1) + 4.0 * n_sel
    return {"selection": name, "n_selected": int(n_sel), "nnz_in": int(nnz_in), "nnz_out": int(nnz_out), "shape_out": [nrow, ncol],
            "gather_ms": gather_ms, "transpose_ms": transpose_ms, "subset_ms": subset_ms,
            "replaced_ms": 1e3 * (t3 - t0), "replaced_download_ms": 1e3 * (t1 - t0), "replaced_numpy_ms": 1e3 * (t2 - t1),
            "replaced_upload_ms": 1e3 * (t3 - t2), "replaced_bytes_over_the_link": 12.0 * nnz_in + 12.0 * nnz_out,
            "gather_bytes": gather_bytes, "gather_GB_per_s": gather_bytes / (gather_ms * 1e6) if gather_ms > 0 else None,
            "same_bits_as_replaced_route": bool(same)}


def main():
    import singlet_amd as sa
    rng = np.random.default_rng(7)
    with sa.Context(0) as w:   # warm-up: module load, the sort's first use
        w.synth(2000, 3000, 20)
        w.subset(np.arange(0, 2000, 3), np.arange(0, 3000, 2))
    res = {"matrix": [GENES, CELLS], "inv_density": 20,
           "genes_2000": one(sa, "rows", np.sort(rng.choice(GENES, 2000, replace=False)), None),
           "cells_20000": one(sa, "cols", None, np.sort(rng.choice(CELLS, 20000, replace=False)))}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
