#!/usr/bin/env python3
"""Time the ligand-receptor calls (kernels_ligrec.hip) in one session, medians of 3 after a warm-up.  Writes one JSON line to
profiles/ligrec_rate.json (and prints it).

Workload: the synthetic matrix of bench.py's generator, 30 000 genes x 1 000 000 cells at 5 %, 1 000 interacting genes (every
30th), 2 000 pairs drawn among them, nperm = 1 000, at K = 20 and K = 64 (labels = cell index mod K).
Per K:
  call_ms            the whole sgl_ligrec on the resident matrix, wall clock (labels, sums, tally, downloads);
  sums_ms            the "scale" phase of sgl_op_ligrec_sums over 64 given label vectors (gather, sums kernel, segment reduction);
  entry_vector_adds_per_s = stored entries of the listed genes x 64 / sums_ms: the rate of the sums kernel;
  global_path_ms     the same 64 vectors with the bins in global scratch (path = 2).
Comparisons:
  marker_sums        one sgl_op_marker_sums (transform identity) on the matrix subset to the listed genes (sgl_subset), the
                     "scale" phase of one call, times nperm: the path without this feature;
  host_restatement_s tests/ligrec_restatement.py on 3 label vectors over the listed genes on the host, scaled to nperm.
NOT measured: skewed gene lengths (the generator's genes are all near 50 000 entries), K near 256, the global path at scale
beyond the 64 vectors above, hardware counters of the sums kernel.

  python scripts/ligrec_rate.py [genes] [cells] [listed genes] [nperm]     defaults: 30000 1000000 1000 1000"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "ligrec_rate.json")


def med(v):
    return float(np.median(v))


def scale_ms(c, call, repeats=3):
    call()                                                                # first use
    ms = []
    for _ in range(repeats):
        c.timing_get(reset=True)
        call()
        ms.append(c.timing_get(reset=True)["scale"][0])
    return med(ms)


def main():
    import singlet_amd as sa
    import ligrec_restatement as lr
    from nhood_restatement import permuted
    arg = [int(v) for v in sys.argv[1:]]
    m, n, G, nperm = (arg + [30000, 1000000, 1000, 1000][len(arg):])[:4]
    P = 2 * G
    genes = (np.arange(G, dtype=np.int32) * (m // G)).astype(np.int32)
    rng = np.random.default_rng(0)
    lig, rec = rng.integers(0, G, P).astype(np.int32), rng.integers(0, G, P).astype(np.int32)
    res = {"device": "MI355X", "medians_of": 3, "genes": m, "cells": n, "listed_genes": G, "pairs": P, "nperm": nperm}
    with sa.Context(0) as c:
        c.synth(m, n, 20)
        c.timing_enable(True)
        per_gene = c.col_counts(1)[genes]
        entries = int(per_gene.sum())
        res.update(stored_entries=int(c.dims()[2]), listed_entries=entries, longest_listed_gene=int(per_gene.max()), segments=lr.segments(per_gene))
        for K in (20, 64):
            lab = (np.arange(n) % K).astype(np.int32)
            c.ligrec(lab, genes, lig, rec, K, nperm=64, seed=1)              # first use
            calls = []
            for _ in range(3):
                t = time.perf_counter()
                out = c.ligrec(lab, genes, lig, rec, K, nperm=nperm, seed=0)
                calls.append(1e3 * (time.perf_counter() - t))
            info = c.ligrec_info()
            labs = c.op_nhood_permute(lab, seed=0, r0=0, nb=64)
            sums = scale_ms(c, lambda: c.op_ligrec_sums(labs, K, genes))
            glob = scale_ms(c, lambda: c.op_ligrec_sums(labs, K, genes, path=2))
            one = {"K": K, "info": info, "call_ms": med(calls), "sums_ms": sums, "global_path_ms": glob, "label_vectors_timed": 64,
                   "entry_vector_adds_per_s": entries * 64.0 / (sums * 1e-3), "entry_vector_adds_per_s_global": entries * 64.0 / (glob * 1e-3),
                   "n_ge_at_floor": int((out["n_ge"] == 0).sum())}
            if K == 20:
                keep = {"lab": lab, "labs3": labs[:3], "sums3": c.op_ligrec_sums(labs[:3], K, genes)}
                assert np.array_equal(labs[:3], permuted(lab, 0, 0, 3))
            res["K%d" % K] = one
        # the path without this feature: one marker pass over the subset matrix per label vector
        c.subset(rows=genes)
        lab = keep["lab"]
        ms = scale_ms(c, lambda: c.op_marker_sums(lab, 20, "identity"))
        res["marker_sums"] = {"K": 20, "one_call_ms": ms, "scaled_to_nperm_ms": ms * nperm}
        x, cells, p = c.download(1)                                        # the gene-side image of the subset: genes in listed order
    t = time.perf_counter()
    ref = lr.sums(x, cells.astype(np.int64), p, np.arange(G), keep["labs3"], 20)
    host = time.perf_counter() - t
    res["host_restatement_s"] = {"label_vectors_timed": 3, "s": host, "scaled_to_nperm_s": host * nperm / 3}
    res["equal_to_restatement"] = bool(ref.tobytes() == np.ascontiguousarray(keep["sums3"]).tobytes())
    res["K20"]["speedup_over_marker_sums"] = res["marker_sums"]["scaled_to_nperm_ms"] / res["K20"]["call_ms"]
    res["not_measured"] = ["skewed gene lengths", "K near 256", "the global path at scale", "hardware counters of the sums kernel"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
