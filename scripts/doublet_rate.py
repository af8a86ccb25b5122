#!/usr/bin/env python3
"""Time sgl_simulate_doublets (kernels_doublet.hip) against its bandwidth bound and against the pure copy of the same size.
Writes one JSON line to profiles/doublet_rate.json (and prints it).

On sgl_synth_csc 30 000 x 1 000 000 at 5 % (1.5e9 entries), parents from doublet_parents(seed 0):
  (a) n_sim = 10^6 in one call, and the same parents in four calls of 250 000: per call
        merge_ms      the three passes (lengths, scan, fill) between the context's hipEvents ("scale" phase of dst),
        transpose_ms  the device transpose of S that follows (the library's own wall clock around the synchronised call),
        call_ms       the whole sgl_simulate_doublets call, wall clock;
  (b) the yardstick a pure copy sets: sgl_subset's column gather of the SAME columns (cols = parent_a then parent_b, 2 x 10^6
      columns, so the gather writes the parents' entries, which the merge reads), its gather_ms between the same hipEvents.
merge_bytes is the HBM model of the merge: both parents read once (12 B an entry) and S written once (12 B an entry), plus
the offsets and the lists; the length pass reads the parents' indices once more (4 B an entry), which the model leaves out.
NOT measured: skewed column lengths (the synthetic columns are all near 1 500 entries), the long path at scale (every pair
here fits the LDS cap), other caps."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "doublet_rate.json")
GENES, CELLS, N_SIM, BATCH = 30000, 1000000, 1000000, 250000


def simulate(sa, src, dst, pa, pb):
    dst.timing_get(reset=True)
    tr0 = sa.call_times()["transpose_s"]
    t = time.perf_counter()
    src.simulate_doublets(dst, pa, pb)
    call_ms = 1e3 * (time.perf_counter() - t)
    info = dst.doublets_info()
    merge_ms = dst.timing_get(reset=True)["scale"][0]
    parents_entries = info["entries"] + info["shared_rows"]
    nbytes = 12.0 * parents_entries + 12.0 * info["entries"] + 8.0 * 4 * pa.size + 8.0 * (pa.size + 1) + 8.0 * pa.size
    return {"n_sim": int(pa.size), "merge_ms": merge_ms, "transpose_ms": 1e3 * (sa.call_times()["transpose_s"] - tr0), "call_ms": call_ms,
            "merge_bytes": nbytes, "merge_GB_per_s": nbytes / (merge_ms * 1e6) if merge_ms > 0 else None, **info}


def main():
    import singlet_amd as sa
    genes, cells, n_sim, batch = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (GENES, CELLS, N_SIM, BATCH)
    with sa.Context(0) as w, sa.Context(0) as d:   # warm-up: module load, the sort's first use
        w.synth(2000, 3000, 20)
        w.simulate_doublets(d, *sa.doublet_parents(3000, 4000, 0))
        w.subset(cols=np.arange(0, 3000, 2))
    pa, pb = sa.doublet_parents(cells, n_sim, 0)
    res = {"matrix": [genes, cells], "inv_density": 20}
    with sa.Context(0) as src, sa.Context(0) as dst:
        src.synth(genes, cells, 20)
        res["nnz"] = src.dims()[2]
        dst.timing_enable(True)
        res["one_batch"] = simulate(sa, src, dst, pa, pb)
        res["batches"] = [simulate(sa, src, dst, pa[s:s + batch], pb[s:s + batch]) for s in range(0, n_sim, batch)]
    with sa.Context(0) as c:
        c.synth(genes, cells, 20)
        c.timing_enable(True)
        c.timing_get(reset=True)
        t = time.perf_counter()
        c.subset(cols=np.concatenate([pa, pb]))
        subset_ms = 1e3 * (time.perf_counter() - t)
        gather_ms = c.timing_get(reset=True)["scale"][0]
        nnz_out = c.dims()[2]
    gbytes = 24.0 * nnz_out + 28.0 * 2 * n_sim
    res["subset_gather"] = {"columns": 2 * int(n_sim), "nnz_out": int(nnz_out), "gather_ms": gather_ms, "subset_ms": subset_ms,
                            "gather_bytes": gbytes, "gather_GB_per_s": gbytes / (gather_ms * 1e6) if gather_ms > 0 else None}
    one = res["one_batch"]
    res["merge_ms_over_gather_ms"] = one["merge_ms"] / gather_ms if gather_ms > 0 else None
    res["merge_rate_over_gather_rate"] = (one["merge_GB_per_s"] / res["subset_gather"]["gather_GB_per_s"]
                                          if gather_ms > 0 and one["merge_ms"] > 0 else None)
    res["batches_merge_ms_sum"] = sum(b["merge_ms"] for b in res["batches"])
    res["not_measured"] = ["skewed column lengths", "the long path at scale", "nn_method='ivf' at 3e6 joint cells"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
