#!/usr/bin/env python3
"""Time graph-convolutional NMF on a one-device team against its two neighbours, on config 3's synthetic matrix
(30 000 x 1 000 000, k = 50) with the 1000 x 1000 lattice graph (tests/gcnmf_restatement.py lattice_graph):
  (a) the one-context GCNMF fit,
  (b) the GCNMF fit on a team of `ranks` ranks that share device 0 (halo exchange through the loopback kernel),
  (c) the plain fit on the same team.
Everything is seeded (synthetic matrix and initial w of the library's generator, fixed graph).  Each sample is one
nmf_run of `iters` iterations after a warm-up iteration.  Its headline figure, wall_ms_per_iter, is HOST WALL time per
iteration (nmf_run returns after the device has finished); the phase split comes from device events (hipEvent pairs
around every phase; team: mean over the ranks; ranks that share a device interleave, so a rank's phases do not add up to
the wall time), and phase_sum_ms_per_iter is their sum.  (b) and (c) alternate on one team; (a) is NOT interleaved with
them: it is sampled before and after the team's rounds, because the one-context fit and the team do not both stay
resident.  Medians are reported, with (b) / (a) and (b) - (c) of the wall times and the bytes per halo exchange from
graph_info().  Writes one JSON document.
usage: gcnmf_team_rate.py [--out FILE] [--ranks N] [--side S] [--genes G] [--k K] [--iters I] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import singlet_amd as sa  # noqa: E402
import gcnmf_restatement as gr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcnmf_team_rate.json"))
ap.add_argument("--ranks", type=int, default=8)
ap.add_argument("--side", type=int, default=1000)
ap.add_argument("--genes", type=int, default=30000)
ap.add_argument("--k", type=int, default=50)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
cells, k, iters = args.side * args.side, args.k, args.iters
L1 = 0.01

dgc = types.SimpleNamespace(CSC=lambda x, i, p, nr, nc: sa.dgCMatrix(x, i, p, (nr, nc)))
lattice = gr.lattice_graph(dgc, args.side)


def sample(fit, ctxs, graph):
    fit.fit_init(k, None)
    if graph:
        fit.set_graph(lattice)
    fit.nmf_run(0.0, 1, L1, L1, 0.0, 0.0)   # warm-up: the first iteration starts the sweep-count packing cold
    for c in ctxs:
        c.timing_enable(True)
        c.timing_get(reset=True)
    t = time.perf_counter()
    fit.nmf_run(0.0, iters, L1, L1, 0.0, 0.0)
    dt = time.perf_counter() - t
    ph = [c.timing_get(reset=True) for c in ctxs]
    for c in ctxs:
        c.timing_enable(False)
    names = [p for p in ph[0] if any(q[p][1] for q in ph)]
    return {"wall_ms_per_iter": 1e3 * dt / iters,
            "phases_ms_per_iter": {p: sum(q[p][0] for q in ph) / len(ph) / iters for p in names},
            "phase_calls_per_iter": {p: sum(q[p][1] for q in ph) / len(ph) / iters for p in names}}


def one_context(n):
    with sa.Context(0) as c:
        c.synth(args.genes, cells, 20)
        return [sample(c, [c], True) for _ in range(n)]


def summary(samples):
    out = {"samples_wall_ms_per_iter": [s["wall_ms_per_iter"] for s in samples],
           "wall_ms_per_iter": statistics.median(s["wall_ms_per_iter"] for s in samples)}
    for key in ("phases_ms_per_iter", "phase_calls_per_iter"):
        out[key] = {p: statistics.median(s[key][p] for s in samples) for p in samples[0][key]}
    out["phase_sum_ms_per_iter"] = sum(out["phases_ms_per_iter"].values())
    return out


a = one_context(args.rounds)
b, c_ = [], []
with sa.Multi([0] * args.ranks) as M:
    M.synth(args.genes, cells, 20)
    ctxs = [M.rank_ctx(r) for r in range(args.ranks)]
    info = None
    for _ in range(args.rounds):
        b.append(sample(M, ctxs, True))
        if info is None:
            info = M.graph_info()
        c_.append(sample(M, ctxs, False))
a += one_context(args.rounds)

out = {"cells": cells, "genes": args.genes, "k": k, "ranks": args.ranks, "iters_per_sample": iters, "graph_nnz": int(lattice.nnz),
       "graph_info": info, "halo_bytes_per_exchange_and_rank": info["halo_bytes"],
       "halo_bytes_per_iteration_and_rank": 2 * info["halo_bytes"],
       "a_one_context_gcnmf": summary(a), "b_team_gcnmf": summary(b), "c_team_plain": summary(c_)}
out["timing"] = ("wall_ms_per_iter: host wall time per iteration; phases_ms_per_iter: device events; (a) sampled before and after "
                 "the team's rounds, (b) and (c) alternated")
out["b_over_a_wall"] = out["b_team_gcnmf"]["wall_ms_per_iter"] / out["a_one_context_gcnmf"]["wall_ms_per_iter"]
out["b_minus_c_wall_ms"] = out["b_team_gcnmf"]["wall_ms_per_iter"] - out["c_team_plain"]["wall_ms_per_iter"]
out["transport"] = "loopback kernel (ranks share one device); RCCL's all-gather between devices is not measured"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({key: out[key] for key in ("b_over_a_wall", "b_minus_c_wall_ms", "graph_info")}))
