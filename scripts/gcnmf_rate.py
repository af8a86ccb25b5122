#!/usr/bin/env python3
"""Time graph-convolutional NMF against plain NMF on config 3's synthetic matrix (30 000 x 1 000 000, k = 50) with a
1000 x 1000 lattice graph (tests/gcnmf_restatement.py lattice_graph: 3 x 3 neighbourhoods, 9 x 10^6 entries), on one
resident context: ms per iteration and hipEvent phases of the c_nmf iteration, of the GCNMF iteration, and of the GCNMF
iteration with the graph's cell labels randomly permuted (P G P^T: the gathers leave spatial order).  The convolution's
time is the rhs_h + rhs_w phase time a graph adds over the plain iteration, per call.  Prints one JSON line.
usage: gcnmf_rate.py [side] [genes] [k] [iters]"""
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import singlet_amd as sa  # noqa: E402
import gcnmf_restatement as gr  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
genes = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
k = int(sys.argv[3]) if len(sys.argv) > 3 else 50
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 5
cells = side * side

dgc = types.SimpleNamespace(CSC=lambda x, i, p, nr, nc: sa.dgCMatrix(x, i, p, (nr, nc)))
t0 = time.perf_counter()
lattice = gr.lattice_graph(dgc, side)
shuffled = gr.lattice_graph(dgc, side, perm=np.random.default_rng(1).permutation(cells))
build_s = time.perf_counter() - t0

ctx = sa.Context(0)
ctx.synth(genes, cells, 20)
ctx.fit_init(k, None)
ctx.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)   # warm-up


def run(G):
    ctx.fit_init(k, None)
    if G is not None:
        ctx.set_graph(G)
    ctx.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)   # first iteration outside the timing (sweep-count packing starts cold)
    ctx.timing_enable(True)
    ctx.timing_get(reset=True)
    t = time.perf_counter()
    ctx.nmf_run(0.0, iters, 0.01, 0.01, 0.0, 0.0)
    dt = time.perf_counter() - t
    ph = ctx.timing_get(reset=True)
    ctx.timing_enable(False)
    return {"ms_per_iter": 1e3 * dt / iters, "phases_ms_per_iter": {p: v[0] / iters for p, v in ph.items() if v[1]}}


out = {"cells": cells, "genes": genes, "k": k, "iters": iters, "graph_nnz": lattice.nnz, "graph_build_s": build_s,
       "c_nmf": run(None), "gcnmf_lattice": run(lattice), "gcnmf_shuffled": run(shuffled)}
base = out["c_nmf"]["phases_ms_per_iter"]
for name in ("gcnmf_lattice", "gcnmf_shuffled"):
    r = out[name]
    ph = r["phases_ms_per_iter"]
    conv_ms = ((ph["rhs_h"] - base["rhs_h"]) + (ph["rhs_w"] - base["rhs_w"])) / 2   # two convolutions per iteration
    r["conv_ms_per_call"] = conv_ms
    r["ratio_to_c_nmf"] = r["ms_per_iter"] / out["c_nmf"]["ms_per_iter"]
    # unique bytes of one call: G (12 B per entry + 8 B per column pointer), X and Y (k doubles per cell each)
    r["conv_unique_GB"] = (12.0 * lattice.nnz + 8.0 * (cells + 1) + 2 * 8.0 * k * cells) / 1e9
    r["conv_gathered_GB"] = 8.0 * k * lattice.nnz / 1e9
    r["conv_unique_TBps"] = r["conv_unique_GB"] / conv_ms if conv_ms > 0 else None
ctx.close()
print(json.dumps(out))
