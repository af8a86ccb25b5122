#!/usr/bin/env python3
"""Time RasterizeRowwise (kernels_raster.hip).  Writes one JSON line to profiles/rasterize_rate.json (and prints it).

  rasterize_rate.py [reps]      whole calls, median of `reps` after a warm-up:
      * one-shot sparse (rowwise_compress_sparse, n = 10) on pbmc3k and on a 30 000 x 200 000 host matrix at 5 %;
      * resident sparse at config 3 (sgl_synth_csc 30 000 x 10^6, 5 %, 1.5e9 entries) for n = 10 and 100: the whole
        sgl_rasterize_rowwise call between two hipEvents on the context's stream (the rasterising kernel plus the dense
        ingest of its result: count / scan / fill / transpose);
      * the test-side numpy restatement's CPU time per 1000 columns (a restatement, not the reference, which needs R).
  rasterize_rate.py --once      each case once, in the order above (for rocprofv3: one kernel launch per case).
  rasterize_rate.py --kernels DIR
      folds a `rocprofv3 --kernel-trace --memory-copy-trace` run of `--once` (its *kernel_trace.csv and
      *memory_copy_trace.csv under DIR) into the JSON: per case the rasterising kernel's time, its bytes under the HBM
      model (stored entries read once: 12 B each, + 8 B per output element written) and the fraction of the 8 TB/s bound;
      for the one-shot cases the host->device and device->host copy times; for the resident cases the kernels of the
      ingest that follows."""
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "rasterize_rate.json")
HBM = 8.0e12
CASES = ("oneshot_pbmc3k_n10", "oneshot_30000x200000_n10", "resident_config3_n10", "resident_config3_n100")


def pbmc3k(sa):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, di, x = g["p"].astype(np.int64), g["di"].astype(np.int64), g["x"].astype(np.float64)
    cs = np.cumsum(di)
    i = cs - np.repeat(cs[p[:-1]] - di[p[:-1]], np.diff(p))
    return sa.dgCMatrix(x, i.astype(np.int32), p.astype(np.int32), (int(g["dim"][0]), int(g["dim"][1])))


def host_matrix(sa, genes, cells):
    c = sa.Context(0)
    try:
        c.synth(genes, cells, 20)
        x, i, p = c.download(0)
    finally:
        c.close()
    return sa.dgCMatrix(x, i, p.astype(np.int32), (genes, cells))


def model_bytes(nnz, nrow, ncol, n):
    return 12.0 * nnz + 8.0 * (nrow // n) * ncol


def run(reps):
    import singlet_amd as sa
    hip = C.CDLL("libamdhip64.so")
    res = {"reps": reps}
    mats = {"oneshot_pbmc3k_n10": pbmc3k(sa), "oneshot_30000x200000_n10": host_matrix(sa, 30000, 200000)}
    for name, A in mats.items():
        ts = []
        for r in range(reps + (1 if reps > 1 else 0)):
            t = time.perf_counter()
            sa.rowwise_compress_sparse(A, 10)
            ts.append(time.perf_counter() - t)
        ts = ts[1:] if reps > 1 else ts
        res[name] = {"shape": list(A.Dim), "nnz": int(A.nnz), "call_ms": 1e3 * float(np.median(ts)),
                     "h2d_bytes": 12.0 * A.nnz + 4.0 * (A.ncol + 1), "d2h_bytes": 8.0 * (A.nrow // 10) * A.ncol,
                     "model_bytes": model_bytes(A.nnz, A.nrow, A.ncol, 10)}
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    for n in (10, 100):
        ms = []
        for r in range(max(1, reps // 2)):
            c = sa.Context(0)
            try:
                c.set_stream(stream.value)
                c.synth(30000, 1_000_000, 20)
                nnz = c.dims()[2]
                assert hip.hipStreamSynchronize(stream) == 0
                t = time.perf_counter()
                hip.hipEventRecord(ev[0], stream)
                c.rasterize_rowwise(n)
                hip.hipEventRecord(ev[1], stream)
                assert hip.hipEventSynchronize(ev[1]) == 0
                wall = time.perf_counter() - t
                f = C.c_float()
                hip.hipEventElapsedTime(C.byref(f), ev[0], ev[1])
                ms.append((f.value, 1e3 * wall, c.dims()[2]))
                c.set_stream(None)
            finally:
                c.close()
        res["resident_config3_n%d" % n] = {"nnz_in": int(nnz), "nnz_out": int(ms[-1][2]), "call_event_ms": float(np.median([m[0] for m in ms])),
                                           "call_wall_ms": float(np.median([m[1] for m in ms])),
                                           "model_bytes": model_bytes(nnz, 30000, 1_000_000, n)}
    import rowwise_compress_restatement as rr
    A = mats["oneshot_30000x200000_n10"]
    sub = A.col_slice(0, 200)
    t = time.perf_counter()
    rr.vectorised_sparse(sub, 10)
    res["restatement_cpu_s_per_1000_columns_30000_rows"] = (time.perf_counter() - t) * 5.0
    return res


def fold_kernels(d):
    import csv
    res = json.load(open(OUT))

    def rows(pat):
        f = sorted(glob.glob(os.path.join(d, "**", pat), recursive=True))
        return list(csv.DictReader(open(f[0]))) if f else []
    ks = sorted(rows("*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    cps = sorted(rows("*memory_copy_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    starts = [q for q, r in enumerate(ks) if "raster_sparse_kernel" in r["Kernel_Name"]]
    assert len(starts) == len(CASES), "expected one rasterising launch per case, found %d" % len(starts)
    for q, (name, s) in enumerate(zip(CASES, starts)):
        r = ks[s]
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        e = res[name]
        e["kernel_ms"] = ns / 1e6
        e["kernel_GB_per_s"] = e["model_bytes"] / ns
        e["fraction_of_8TBps"] = e["model_bytes"] / HBM / (ns / 1e9)
        t0, t1 = int(r["Start_Timestamp"]), (int(ks[starts[q + 1]]["Start_Timestamp"]) if q + 1 < len(starts) else 1 << 62)
        if name.startswith("oneshot"):
            lo = int(ks[starts[q - 1]]["End_Timestamp"]) if q else 0
            near = [c for c in cps if lo < int(c["Start_Timestamp"]) < t1]
            e["h2d_ms"] = sum(int(c["End_Timestamp"]) - int(c["Start_Timestamp"]) for c in near if int(c["Start_Timestamp"]) < t0 and "HOST_TO_DEVICE" in c["Direction"]) / 1e6
            e["d2h_ms"] = sum(int(c["End_Timestamp"]) - int(c["Start_Timestamp"]) for c in near if int(c["Start_Timestamp"]) > t0 and "DEVICE_TO_HOST" in c["Direction"]) / 1e6
        else:
            after = [k for k in ks[s + 1:] if int(k["Start_Timestamp"]) < t1 and "synth" not in k["Kernel_Name"]]
            e["ingest_kernels_ms"] = sum(int(k["End_Timestamp"]) - int(k["Start_Timestamp"]) for k in after) / 1e6
    return res


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        res = fold_kernels(sys.argv[2])
    else:
        once = len(sys.argv) > 1 and sys.argv[1] == "--once"
        res = run(1 if once else int(sys.argv[1]) if len(sys.argv) > 1 else 3)
        if once:
            print(json.dumps(res))
            sys.exit(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)
