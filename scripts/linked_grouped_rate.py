#!/usr/bin/env python3
"""Time the two device pieces of the linked-NMF workflow at config-3 size.  Writes one JSON line to
profiles/linked_grouped_rate.json (and prints it).

On sgl_synth_csc 30 000 x 1 000 000 at 5 %, k = 50, G = 8 interleaved groups, 5 repeats after one warm-up each:
  (a) group_means   sgl_group_means of the fit's resident H (kernels_group.hip): the two kernels between the context's
                    hipEvents (booked under the "scale" phase) and the whole call's wall clock (counting sort of the labels
                    on the host, four small uploads, the kernels, k G doubles back).  group_means_GB_per_s = the bytes the
                    kernels must move (8 k n of H, 4 n of the cell list) over the kernel time, beside the 6 290 GB/s a
                    float4 copy reaches on this part (bench.py: HBM_MEASURED_GBS).
  (b) rhs_h         the "rhs_h" phase of sgl_step_h -- the sparse accumulate over A plus the link multiplication -- without
                    a link, with the dense k x n link (sgl_set_links: link_mul_kernel, unchanged) and with the grouped link
                    (sgl_set_links_grouped: link_mul_grouped_kernel, the k x G table staged in LDS).  The same link either
                    way: the dense matrix is table[:, group].
  (c) the device bytes each form of the link holds, and whether the two forms left the same H (bit for bit).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "linked_grouped_rate.json")
GENES, CELLS, K, G, REPEATS = 30000, 1000000, 50, 8, 5
COPY_GB_PER_S = 6290.0


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}


def rhs_h_phase(c, setter):
    """rhs_h milliseconds of REPEATS H-updates after one warm-up, from the same factors every time; returns (times, H)."""
    c.fit_init(K)
    setter(c)
    out = []
    for rep in range(REPEATS + 1):
        c.timing_get(reset=True)
        c.step_h(0.01, 0.0)
        t = c.timing_get(reset=True)["rhs_h"][0]
        if rep:
            out.append(t)
    return out, c.get_factors(w=False, d=False)[2]


def main():
    import singlet_amd as sa
    n, k = int(os.environ.get("LGR_CELLS", CELLS)), K
    rng = np.random.default_rng(1)
    group = rng.integers(0, G, n).astype(np.int32)
    table = (rng.random((k, G)) < 0.7) * (0.5 + rng.random((k, G)))
    res = {"genes": GENES, "cells": n, "k": k, "groups": G, "repeats": REPEATS, "copy_GB_per_s_guide": COPY_GB_PER_S}
    c = sa.Context(0)
    try:
        c.synth(GENES, n, 20)
        res["nnz"] = c.dims()[2]
        c.timing_enable(True)
        none_ms, _ = rhs_h_phase(c, lambda c: None)
        grouped_ms, Hg = rhs_h_phase(c, lambda c: c.set_links_grouped(table, group))
        # group means of the resident H (the H the grouped fit just solved)
        kern, wall = [], []
        for rep in range(REPEATS + 1):
            c.timing_get(reset=True)
            t0 = time.perf_counter()
            means, counts = c.group_means(group, G)
            t1 = time.perf_counter()
            if rep:
                kern.append(c.timing_get(reset=True)["scale"][0])
                wall.append(1e3 * (t1 - t0))
        t0 = time.perf_counter()
        dense = table[:, group]
        expand_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        dense_ms, Hd = rhs_h_phase(c, lambda c: c.set_links(dense, None))
        res["dense_fit_init_set_links_and_steps_s"] = time.perf_counter() - t0
    finally:
        c.close()
    moved = 8.0 * k * n + 4.0 * n
    res.update({
        "group_means_kernels_ms": stats(kern), "group_means_call_ms": stats(wall), "group_means_bytes": moved,
        "group_means_GB_per_s": moved / (float(np.median(kern)) * 1e6),
        "group_means_share_of_copy_rate": moved / (float(np.median(kern)) * 1e6) / COPY_GB_PER_S,
        "group_counts": [int(v) for v in counts], "group_means_finite": bool(np.all(np.isfinite(means))),
        "rhs_h_no_link_ms": stats(none_ms), "rhs_h_dense_link_ms": stats(dense_ms), "rhs_h_grouped_link_ms": stats(grouped_ms),
        "grouped_minus_dense_ms": float(np.median(grouped_ms) - np.median(dense_ms)),
        "dense_spread_ms": float(max(dense_ms) - min(dense_ms)), "grouped_spread_ms": float(max(grouped_ms) - min(grouped_ms)),
        "grouped_not_slower_beyond_spread": bool(np.median(grouped_ms) - np.median(dense_ms) <= max(max(dense_ms) - min(dense_ms), max(grouped_ms) - min(grouped_ms))),
        "link_device_bytes_dense": 8.0 * k * n, "link_device_bytes_grouped": 8.0 * k * G + 4.0 * n,
        "host_expand_dense_link_s": expand_s, "same_H_bits_dense_and_grouped": bool(np.array_equal(Hd, Hg)),
    })
    line = json.dumps(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
