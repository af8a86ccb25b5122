#!/usr/bin/env python3
"""Time the typed upload door (sgl_upload_typed, Context.upload_native) against the route it replaces.  Writes one JSON
line to profiles/native_ingest_rate.json (and prints it).

The matrix is sgl_synth_csc 30 000 x 200 000 at 5 % (3.0e8 entries), held on the host the way AnnData holds X: a SciPy
float32 CSR, cells x genes.  Wall clock around synchronised calls, each once after a small warm-up:
  (a) today's route: as_dgCMatrix(X.T) (host: sort check, float64 copy of the values) then Context.upload, timed apart;
  (b) upload_native(native(X, cells_by_genes=True)) from host memory;
  (c) the same from torch tensors that already live on the device (their upload is not timed);
  (d) (b) with the indices of every cell reversed: the device sort's cost.
bytes_copied is what each route reads from the caller's arrays ((a): 12 B per entry and the int32 offsets).  Every route's
resident state (both orientations: p, i, x) is hashed; same_bits_as_replaced_route says they all equal (a)'s."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "native_ingest_rate.json")
GENES, CELLS = 30000, 200000


def say(*a):
    print("[native_ingest_rate]", *a, flush=True)


def state_hash(c):
    h = hashlib.blake2b(digest_size=16)
    for which in (0, 1):
        for a in c.download(which):
            h.update(np.ascontiguousarray(a).view(np.uint8))
    return h.hexdigest()


def reversed_within_slices(data, indices, indptr, chunk=1 << 24):
    """Every slice's (index, value) pairs in reverse order, built slice range by slice range to bound the temporaries."""
    d, i = np.empty_like(data), np.empty_like(indices)
    n = indptr.shape[0] - 1
    c0 = 0
    while c0 < n:
        c1 = int(np.searchsorted(indptr, indptr[c0] + chunk, side="right"))
        c1 = min(max(c1 - 1, c0 + 1), n)
        lo, hi = int(indptr[c0]), int(indptr[c1])
        lens = np.diff(indptr[c0:c1 + 1])
        src = np.repeat(indptr[c0:c1] + indptr[c0 + 1:c1 + 1] - 1, lens) - np.arange(lo, hi, dtype=np.int64)
        d[lo:hi], i[lo:hi] = data[src], indices[src]
        c0 = c1
    return d, i


def timed(sync, fn):
    sync()
    t = time.perf_counter()
    out = fn()
    sync()
    return out, 1e3 * (time.perf_counter() - t)


def run(sa, sp, torch, genes, cells, record):
    sync = torch.cuda.synchronize
    with sa.Context(0) as c:
        c.synth(genes, cells, 20)
        x, i, p = c.download(0)                      # the CSC of A = the CSR of cells x genes
    X = sp.csr_matrix((x.astype(np.float32), i, p.astype(np.int32)), shape=(cells, genes))
    del x
    nnz = int(X.indptr[-1])
    res = {"matrix": [genes, cells], "inv_density": 20, "nnz": nnz, "held_as": "scipy float32 CSR cells x genes, int32 indices and indptr"}
    with sa.Context(0) as c:
        # (a)
        A, host_ms = timed(sync, lambda: sa.as_dgCMatrix(X.T))
        _, up_ms = timed(sync, lambda: c.upload(A, None))
        ref = state_hash(c) if record else None
        res["a_as_dgCMatrix_then_upload"] = {"host_convert_ms": host_ms, "upload_ms": up_ms, "total_ms": host_ms + up_ms,
                                             "bytes_copied": 12 * nnz + 4 * (cells + 1)}
        del A
        say("(a)", res["a_as_dgCMatrix_then_upload"])
        same = []

        def native_route(name, N):
            rep, ms = timed(sync, lambda: c.upload_native(N))
            res[name] = {"upload_ms": ms, "bytes_copied": rep["bytes_copied"], "sorted_lds": rep["sorted_lds"], "sorted_long": rep["sorted_long"],
                         "GB_per_s_of_bytes_copied": rep["bytes_copied"] / (ms * 1e6)}
            if record:
                same.append(state_hash(c) == ref)
            say(name, res[name])

        native_route("b_upload_native_host", sa.native(X, cells_by_genes=True))
        dev = [torch.from_numpy(a).to("cuda:0") for a in (X.data, X.indices, X.indptr)]
        native_route("c_upload_native_device", sa.native((dev[0], dev[1], dev[2], (cells, genes), "csr"), cells_by_genes=True))
        del dev
        d, ii = reversed_within_slices(X.data, X.indices, X.indptr)
        native_route("d_upload_native_host_reversed", sa.native((d, ii, X.indptr, (cells, genes), "csr"), cells_by_genes=True))
        res["d_sort_cost_ms"] = res["d_upload_native_host_reversed"]["upload_ms"] - res["b_upload_native_host"]["upload_ms"]
    res["same_bits_as_replaced_route"] = bool(same and all(same))
    return res


def main():
    import scipy.sparse as sp
    import torch
    import singlet_amd as sa
    say("warm-up")
    run(sa, sp, torch, 2000, 3000, False)
    say("30 000 x 200 000")
    res = run(sa, sp, torch, GENES, CELLS, True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    line = json.dumps(res)
    open(OUT, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
