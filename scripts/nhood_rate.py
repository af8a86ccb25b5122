#!/usr/bin/env python3
"""Time the neighbourhood enrichment calls (kernels_nhood.hip) in one session, medians of 3 after a warm-up.  Writes one JSON
line to profiles/nhood_rate.json (and prints it).

Workloads:
  grid_k20   10^6 cells on the 8-neighbour graph of a 1000 x 1000 grid, 20 classes in blocks of 250 x 200 cells, nperm = 1000;
  grid_k64   the same graph, 64 classes in blocks of 125 x 125 cells (8 permutations per group);
  snn        the SNN graph (find_neighbors, 20 neighbours) of a clustered 200 000 x 50 embedding, the 20 planted clusters as
             classes, nperm = 1000: a graph with hub columns.
Per workload:
  stage_ms          the library's own events around every stage of every batch (sgl_c_nhood_enrichment's stage_ms): keys + sort
                    + gather, tallies, reduction;
  call_ms           the whole one-shot call, wall clock (context, graph upload, column search, download, statistics);
  edge_visits       counted stored entries x nperm;  edge_visits_per_s = edge_visits / the tally stage;
  label_loads       2 x stored entries x groups: one load of PG bytes for the centre cell and one for the neighbour per entry and
                    group (16-byte loads at PG = 16);  label_loads_per_s = label_loads / the tally stage.  The yardstick beside it
                    is sgl_moran's cross term, 2.0e10 8-byte lookups/s (profiles/moran_rate.json): a comparison, not a gate;
  host_restatement_s  tests/nhood_restatement.py (numpy: lexsort, gather, bincount) on 3 permutations on the host, scaled to
                    nperm.
pg_1_vs_16: on the grid at K = 20, the tally operator (gather + tally kernels, the "scale" phase of sgl_op_nhood_tally) over the
same 64 given label vectors with perms_per_group = 1 and 16: what the interleaving buys.
NOT measured: hubs at scale beyond the SNN graph's, K near 256 on the global path, degrees other than 8 and the SNN graph's,
wave-level aggregation of equal bins (not built), hardware counters of the tally kernel."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "nhood_rate.json")
NPERM = 1000


def med(v):
    return float(np.median(v))


def workload(sa, nh, G, lab, K, nperm, host_perms=3):
    import math
    nnz = int(G.p[-1])
    col = np.repeat(np.arange(G.ncol, dtype=np.int64), np.diff(G.p))
    counted = int((G.i != col).sum())
    sa.c_nhood_enrichment(G, lab, K, nperm=16, seed=1)                       # first use
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        out = sa.c_nhood_enrichment(G, lab, K, nperm=nperm, seed=0, timing=True)
        runs.append((1e3 * (time.perf_counter() - t), out["stage_ms"].copy()))
    info = out["info"]
    stage = [med([r[1][q] for r in runs]) for q in range(3)]
    groups = sum(math.ceil(min(info["batch"], nperm - b0) / info["perms_per_group"]) for b0 in range(0, nperm, info["batch"]))
    res = {"cells": int(G.ncol), "stored_entries": nnz, "counted_entries": counted, "max_degree": int(np.diff(G.p).max()), "K": K, "nperm": nperm,
           "info": info, "stage_ms": {"keys_sort_gather": stage[0], "tallies": stage[1], "reduction": stage[2]}, "call_ms": med([r[0] for r in runs]),
           "edge_visits": float(counted) * nperm, "label_loads": 2.0 * nnz * groups, "label_load_bytes": info["perms_per_group"]}
    res["edge_visits_per_s"] = res["edge_visits"] / (stage[1] * 1e-3)
    res["label_loads_per_s"] = res["label_loads"] / (stage[1] * 1e-3)
    t = time.perf_counter()
    ref = nh.enrichment(G.i, G.p, lab, K, host_perms, 0, True)
    host = time.perf_counter() - t
    small = sa.c_nhood_enrichment(G, lab, K, nperm=host_perms, seed=0, return_null=True)
    res["host_restatement_s"] = {"permutations_timed": host_perms, "s": host, "scaled_to_nperm_s": host * nperm / host_perms}
    res["equal_to_restatement"] = bool(np.array_equal(small["null"], ref["null"]) and np.array_equal(small["counts"], ref["counts"]))
    res["z_max_abs"] = float(np.nanmax(np.abs(out["zscore"])))
    return res


def pg_sweep(sa, G, lab, K):
    with sa.Context(0) as c:
        labs = c.op_nhood_permute(lab, seed=0, r0=0, nb=64)
        c.timing_enable(True)
        c.op_nhood_tally(G, labs[:16], K)                                    # first use
        out = {}
        for pg in (1, 16):
            ms = []
            for _ in range(3):
                c.timing_get(reset=True)
                c.op_nhood_tally(G, labs, K, perms_per_group=pg)
                ms.append(c.timing_get(reset=True)["scale"][0])
            out["pg_%d_ms" % pg] = med(ms)
    out["label_vectors"] = 64
    out["ratio"] = out["pg_1_ms"] / out["pg_16_ms"]
    return out


def main():
    import singlet_amd as sa
    import nhood_restatement as nh
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    nperm = int(sys.argv[2]) if len(sys.argv) > 2 else NPERM
    n_snn = int(sys.argv[3]) if len(sys.argv) > 3 else 200_000
    n = side * side
    x, y = np.arange(n) % side, np.arange(n) // side
    Gi, Gp = nh.grid_graph(side, side)
    G = sa.dgCMatrix(np.ones(Gi.shape[0]), Gi, Gp, (n, n))
    res = {"device": "MI355X", "medians_of": 3}
    lab20 = ((x * 4 // side) * 5 + (y * 5 // side)).astype(np.int32)
    res["grid_k20"] = workload(sa, nh, G, lab20, 20, nperm)
    lab64 = ((x * 8 // side) * 8 + (y * 8 // side)).astype(np.int32)
    res["grid_k64"] = workload(sa, nh, G, lab64, 64, nperm)
    res["pg_1_vs_16"] = pg_sweep(sa, G, lab20, 20)
    rng = np.random.default_rng(0)
    cl = rng.integers(0, 20, n_snn).astype(np.int32)
    emb = rng.normal(size=(20, 50))[cl] * 4.0 + rng.normal(size=(n_snn, 50))
    t = time.perf_counter()
    nb = sa.find_neighbors(emb, k_param=20)
    res["snn"] = dict(workload(sa, nh, sa.as_dgCMatrix(nb["snn"]), cl, 20, nperm), find_neighbors_s=time.perf_counter() - t)
    res["moran_lookups_per_s_yardstick"] = json.loads(open(os.path.join(ROOT, "profiles", "moran_rate.json")).read())["main"]["lookups_per_s"]
    res["not_measured"] = ["hubs at scale beyond the SNN graph's", "K near 256 on the global path", "other degrees", "wave-level aggregation of equal bins (not built)",
                           "hardware counters of the tally kernel"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
