#!/usr/bin/env python3
"""Time the spatial autocorrelation calls (kernels_moran.hip) in one session, medians of 3.  Writes one JSON line to
profiles/moran_rate.json (and prints it).

Main workload: sgl_synth_csc 30 000 x 1 000 000 at 5 % (1.5e9 entries) with the spatial_graph of a 1000 x 1000 unit grid at
max_dist 1.5 (the eight surrounding cells, diagonal dropped: mean degree about 8).
  mean_ms      sgl_op_gene_mean's pass over the same entries (the bandwidth yardstick), between the context's hipEvents;
  cross_ms     the kernels of sgl_op_moran_cross over all genes (the "scale" phase of that call): scatter, lookups, clearing;
  moments_ms   the "scale" phase of sgl_moran minus cross_ms and mean_ms: the Q2 / Q4 / T pass and its finish;
  call_ms      the whole sgl_moran call, wall clock (graph check, graph moments and segment tables on the host, uploads);
  lookups      stored entries x the degree of their cell's column = table reads; lookups_per_s = lookups / cross_ms;
  table_bytes_moved  the model of the table path: 2 x 8 B written per entry (set, clear) + 8 B read per lookup + 12 B per
               entry read three times + 12 B of G per lookup.
  host_restatement_s  tests/moran_restatement.py on 3 genes of the same length on the host, scaled to all genes.
Small shape: 13 714 x 3 000 at 5 % on a 60 x 50 grid (pbmc3k scale): every gene takes the search path.
Table batch: the first 512 genes of the main workload with table_batch 1, 8, 64, 512.
Embedding: a random H 50 x 10^6 over the same graph: the kernels ("scale" phase) and the whole call with its 400 MB upload.
NOT measured: SNN graphs with hubs, degrees above 32, the search path at scale (at 10^6 cells and 5 % every gene has 50 000
entries and takes the table), the graph kept resident between calls."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "moran_rate.json")
GENES, SIDE = 30000, 1000


def med(v):
    return float(np.median(v))


def grid_graph(sa, side_x, side_y):
    n = side_x * side_y
    xy = np.stack([np.arange(n) % side_x, np.arange(n) // side_x], axis=1).astype(np.float64)
    t = time.perf_counter()
    G = sa.spatial_graph(xy[:, 0], xy[:, 1], 1.5, 100)
    graph_s = time.perf_counter() - t
    from singlet_amd.api import _without_diagonal
    return _without_diagonal(G), graph_s


def scale_ms(c, call):
    c.timing_get(reset=True)
    t = time.perf_counter()
    out = call()
    wall = 1e3 * (time.perf_counter() - t)
    return c.timing_get(reset=True)["scale"][0], wall, out


def gene_workload(sa, genes, side_x, side_y, batches=()):
    n = side_x * side_y
    G, graph_s = grid_graph(sa, side_x, side_y)
    deg = np.diff(G.p)
    res = {"matrix": [genes, n], "graph_nnz": int(G.p[-1]), "mean_degree": float(deg.mean()), "spatial_graph_s": graph_s}
    with sa.Context(0) as c:
        c.synth(genes, n, 20)
        res["nnz"] = c.dims()[2]
        c.timing_enable(True)
        c.op_gene_mean()
        c.op_moran_cross(G, genes=np.arange(8))                          # first use
        mean = [scale_ms(c, c.op_gene_mean)[0] for _ in range(3)]
        cross = [scale_ms(c, lambda: c.op_moran_cross(G))[0] for _ in range(3)]
        info = c.moran_info()
        whole = [scale_ms(c, lambda: c.moran(G))[:2] for _ in range(3)]
        # lookups: per cell its entries x its column's degree
        per_cell = c.col_counts(0)
        lookups = float(np.dot(per_cell.astype(np.float64), deg.astype(np.float64)))
        res.update(mean_ms=med(mean), cross_ms=med(cross), moments_ms=med([w[0] for w in whole]) - med(cross) - med(mean),
                   kernels_ms=med([w[0] for w in whole]), call_ms=med([w[1] for w in whole]), lookups=lookups,
                   lookups_per_s=lookups / (med(cross) * 1e-3), info=info)
        if info["table_genes"]:
            res["table_bytes_moved"] = 16.0 * res["nnz"] + 8.0 * lookups + 36.0 * res["nnz"] + 12.0 * lookups
            res["table_GB_per_s"] = res["table_bytes_moved"] / (med(cross) * 1e6)
        res["table_batch"] = []
        for b in batches:
            ms = [scale_ms(c, lambda: c.op_moran_cross(G, genes=np.arange(512), path=2, table_batch=b))[0] for _ in range(3)]
            res["table_batch"].append({"genes": 512, "table_batch": b, "cross_ms": med(ms), "batches": c.moran_info()["batches"]})
    return res, G


def host_restatement(sa, G, n, entries, genes_total):
    import moran_restatement as mo
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    tt = sa.moran_graph_moments(G)["t"]                                  # (the library's host code: the restated loop is pure Python)
    moments_s = time.perf_counter() - t0
    times = []
    for _ in range(3):
        cells = np.sort(rng.choice(n, size=entries, replace=False))
        x = 1.0 + rng.poisson(1.5, entries)
        t0 = time.perf_counter()
        mo.gene_moments(x, cells, n, tt)
        mo.cross_term(x, cells, G.x, G.i, G.p, n)
        times.append(time.perf_counter() - t0)
    return {"entries_per_gene": entries, "s_per_gene": med(times), "scaled_to_all_genes_s": med(times) * genes_total,
            "library_graph_moments_s": moments_s}


def embedding(sa, G, k, n):
    rng = np.random.default_rng(1)
    H = rng.random((k, n))
    with sa.Context(0) as c:
        c.timing_enable(True)
        c.moran_embedding(G, H[:, :n])                                   # first use
        runs = [scale_ms(c, lambda: c.moran_embedding(G, H))[:2] for _ in range(3)]
        c.hold_embedding(H)
        held = [scale_ms(c, lambda: c.moran_embedding(G))[:2] for _ in range(3)]
    return {"shape": [k, n], "kernels_ms": med([r[0] for r in runs]), "call_ms_with_upload": med([r[1] for r in runs]),
            "call_ms_held": med([r[1] for r in held])}


def main():
    import singlet_amd as sa
    genes, side = (int(v) for v in sys.argv[1:3]) if len(sys.argv) >= 3 else (GENES, SIDE)
    with sa.Context(0) as w:                                              # warm-up: module load
        w.synth(2000, 3000, 20)
        Gw, _ = grid_graph(sa, 60, 50)
        w.moran(Gw)
    res = {}
    res["main"], G = gene_workload(sa, genes, side, side, batches=(1, 8, 64, 512))
    n = side * side
    res["host_restatement"] = host_restatement(sa, G, n, max(res["main"]["nnz"] // genes, 1), genes)
    res["embedding"] = embedding(sa, G, 50, n)
    res["small"], _ = gene_workload(sa, 13714, 60, 50)
    res["not_measured"] = ["SNN graphs with hubs", "degrees above 32", "the search path at scale", "a graph kept resident between calls"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
