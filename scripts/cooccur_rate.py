#!/usr/bin/env python3
"""Time the co-occurrence calls (kernels_cooccur.hip) in one session, medians of 3 after a warm-up.  Writes one JSON line to
profiles/cooccur_rate.json (and prints it).

Workloads (K = 20 classes in blocks, T = 50 intervals):
  grid_1e6      10^6 cells jittered around the nodes of a 1000 x 1000 grid, r[T] = 8 grid units: the bucket grid;
  allpairs_1e5  10^5 cells (a 316 x 316 part of the same pattern), r[T] = half the diagonal: one bucket, all pairs;
  allpairs_1e6  the 10^6 cells with r[T] = half the diagonal -- run only when the 10^5 run, scaled by pairs, stays under a minute.
Per workload:
  stage_ms            the library's own events around the three stages (sgl_c_cooccur's stage_ms): sort + gather; tally; epilogue +
                      download;
  call_ms             the whole one-shot call, wall clock (context, uploads, download, host statistic);
  candidate_pairs     what sgl_cooccur_info counts: centres x staged candidates, every unordered candidate pair once (a tile's pairs
                      with itself counted whole);  pairs_per_s = candidate_pairs / the tally stage;
  landed_share        unordered pairs that landed in an interval (half the table's sum) / candidate_pairs;
  lds_vs_global       the tally operator on the plan's path and on the forced global path, by the "scale" phase of the context's
                      own timing (every kernel of the call);
  fp64_issue_bound    candidate_pairs x FP64_VALU_PER_PAIR wave-instructions of 64 lanes at 4 cycles each on 4 SIMDs of 256 CUs at
                      2.4 GHz -- the time the loop's FP64 vector instructions alone would take; fp64_issue_share = that / the tally
                      stage.  FP64_VALU_PER_PAIR = 7 is counted from the device assembly of this unit's own compile (hipcc -S of
                      kernels_cooccur.hip, the batch loop of co_tally_kernel: per candidate 2 v_add_f64 for dx and dy, 2
                      v_mul_f64, 1 v_add_f64 and 2 v_cmp_*_f64 against thr2[T] and thr2[0]; the interval search and the atomic run
                      only for pairs that land).
Baselines:
  host_restatement    tests/cooccur_restatement.py (numpy, dense blocks) on the largest part of the pattern that it is predicted to
                      finish in HOST_TARGET_S seconds (from a probe on HOST_PROBE_N points; at most HOST_MAX_N), timed on the host, and
                      SCALED by ordered pairs to each workload's candidate pairs -- named as scaled;
  interaction_matrix  for grid_1e6 only: sa.spatial_graph at max_dist = 8 and sa.interaction_matrix on it, wall clock.  It
                      answers a POORER question (one count per class pair within the radius, no distance profile, and
                      spatial_graph keeps at most max_k neighbours) at a similar cost in pair distances.
NOT measured: K near 256 on the global path, heavy clumping at scale, other T, hardware counters of the tally kernel."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "cooccur_rate.json")
K, T = 20, 50
FP64_VALU_PER_PAIR = 7
HOST_PROBE_N = 6000          # the host restatement is timed on this many points first ...
HOST_TARGET_S = 45.0         # ... and then run once on the n that its pair rate predicts for this time, at most HOST_MAX_N
HOST_MAX_N = 60000
ISSUE_PER_S = 256 * 4 * 2.4e9 / 4.0          # FP64 wave-instructions per second of the whole device


def med(v):
    return float(np.median(v))


def pattern(side, seed=0):
    rng = np.random.default_rng(seed)
    n = side * side
    x, y = (np.arange(n) % side).astype(np.float64), (np.arange(n) // side).astype(np.float64)
    lab = ((np.arange(n) % side) * 4 // side * 5 + (np.arange(n) // side) * 5 // side).astype(np.int32)
    order = rng.permutation(n)
    xy = np.stack([x, y], axis=1) + 0.4 * (rng.random((n, 2)) - 0.5)
    return xy[order], lab[order]


def workload(sa, xy, lab, r, reps=3):
    sa.c_cooccur(xy[:4096], lab[:4096], r, K)                                    # first use
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        out = sa.c_cooccur(xy, lab, r, K, timing=True)
        runs.append((1e3 * (time.perf_counter() - t), out["stage_ms"].copy()))
    info = out["info"]
    stage = [med([q[1][s] for q in runs]) for s in range(3)]
    landed = int(out["counts"].sum()) // 2
    res = {"cells": int(xy.shape[0]), "K": K, "T": T, "r_max": float(r[-1]), "runs": reps, "info": info,
           "stage_ms": {"sort_gather": stage[0], "tally": stage[1], "epilogue_download": stage[2]}, "call_ms": med([q[0] for q in runs]),
           "candidate_pairs": info["pairs"], "landed_pairs": landed, "landed_share": landed / max(info["pairs"], 1)}
    res["pairs_per_s"] = info["pairs"] / (stage[1] * 1e-3)
    res["fp64_issue_bound_ms"] = 1e3 * info["pairs"] / 64.0 * FP64_VALU_PER_PAIR / ISSUE_PER_S
    res["fp64_issue_share"] = res["fp64_issue_bound_ms"] / stage[1]
    with sa.Context(0) as c:
        c.timing_enable(True)
        paths = {}
        for name, path in (("plan", 0), ("global", 2)):
            ms = []
            for _ in range(reps):
                c.timing_get(reset=True)
                got = c.op_cooccur_tally(xy, lab, r, K, bin_path=path)
                ms.append(c.timing_get(reset=True)["scale"][0])
            paths[name + "_kernels_ms"] = med(ms)
            paths[name + "_bin_path"] = c.cooccur_info()["bin_path"]
            paths[name + "_equal"] = bool(np.array_equal(got, out["counts"]))
        paths["global_over_plan"] = paths["global_kernels_ms"] / paths["plan_kernels_ms"]
    res["lds_vs_global"] = paths
    return res


def main():
    import singlet_amd as sa
    import cooccur_restatement as co
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    res = {"device": "MI355X", "medians_of": 3, "fp64_valu_per_pair": FP64_VALU_PER_PAIR, "fp64_wave_instructions_per_s": ISSUE_PER_S}
    xy, lab = pattern(side)
    small_side = max(int(round(side * 0.316)), 8)
    sxy, slab = pattern(small_side, 1)
    # the host restatement, and the device against it on the same points
    hr = np.linspace(0.0, 8.0, T + 1)
    pxy, plab = pattern(int(np.sqrt(HOST_PROBE_N)), 3)
    t = time.perf_counter()
    co.tally(pxy[:, 0], pxy[:, 1], plab, K, hr, block=512)
    probe_s = time.perf_counter() - t
    host_n = min(int(pxy.shape[0] * np.sqrt(HOST_TARGET_S / probe_s)), HOST_MAX_N)
    hxy, hlab = pattern(int(np.sqrt(host_n)), 2)
    t = time.perf_counter()
    want = co.tally(hxy[:, 0], hxy[:, 1], hlab, K, hr, block=512)
    host_s = time.perf_counter() - t
    got = sa.c_cooccur(hxy, hlab, hr, K)["counts"]
    host_pairs = hxy.shape[0] * (hxy.shape[0] - 1) // 2
    res["host_restatement"] = {"cells": int(hxy.shape[0]), "unordered_pairs": host_pairs, "s": host_s, "pairs_per_s": host_pairs / host_s,
                               "equal_to_device": bool(np.array_equal(got, want)),
                               "probe": {"cells": int(pxy.shape[0]), "s": probe_s}, "target_s": HOST_TARGET_S}
    res["grid_1e6"] = workload(sa, xy, lab, np.linspace(0.0, 8.0, T + 1))
    res["allpairs_1e5"] = workload(sa, sxy, slab, co.default_interval(sxy[:, 0], sxy[:, 1], T))
    scaled = res["allpairs_1e5"]["stage_ms"]["tally"] * 1e-3 * (xy.shape[0] / sxy.shape[0]) ** 2
    res["allpairs_1e6_predicted_s"] = scaled
    if scaled < 60.0:
        res["allpairs_1e6"] = workload(sa, xy, lab, co.default_interval(xy[:, 0], xy[:, 1], T), reps=1 if scaled > 5.0 else 3)
    for name in ("grid_1e6", "allpairs_1e5", "allpairs_1e6"):
        if name in res:
            res[name]["host_restatement_scaled_s"] = res[name]["candidate_pairs"] / res["host_restatement"]["pairs_per_s"]
    # the poorer question at a similar cost: the class-pair counts of the radius graph
    try:
        t = time.perf_counter()
        G = sa.spatial_graph(xy[:, 0], xy[:, 1], 8.0, 256)
        t_graph = time.perf_counter() - t
        t = time.perf_counter()
        im = sa.interaction_matrix(lab, G)
        res["interaction_matrix_grid_1e6"] = {"spatial_graph_s": t_graph, "interaction_matrix_s": time.perf_counter() - t, "stored_entries": int(G.p[-1]),
                                              "counted": int(im.sum()), "note": "one count per class pair within the radius, no distance profile"}
    except Exception as e:                                                       # a graph too large for the host is a finding, not a failure
        res["interaction_matrix_grid_1e6"] = {"error": str(e)[:300]}
    res["not_measured"] = ["K near 256 on the global path", "heavy clumping at scale", "other T", "hardware counters of the tally kernel"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
