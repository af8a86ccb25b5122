"""Rate of find_clusters (sgl_c_louvain) on an SNN graph of synthetic cells -> one JSON document (profiles/louvain_rate.json).

    python scripts/louvain_rate.py [cells] [out.json] [networkx time limit in s, 0 = skip]

The cells are Gaussian blobs in a 20-dimensional embedding; the graph is find_neighbors(k_param = 20) with the diagonal
dropped, as find_clusters sees it.  Timed by wall clock around the one-shot call (upload, validation, every level, download):
the whole call, and the call cut to one level with 1 and with 11 sweeps -- their difference over the sweeps kept is the cost
of one level-0 sweep with its modularity pass.  networkx's louvain_communities runs on the same graph in a child process
when networkx is installed, under a time limit."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import singlet_amd as sa  # noqa: E402

HBM_BYTES_PER_S = 8.0e12     # MI355X specification


def timed(fn, repeats=3):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return out, {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


NX_CHILD = """
import sys, time
import numpy as np, scipy.sparse as sp, networkx as nx
z = np.load(sys.argv[1])
G = sp.csc_matrix((z["x"], z["i"], z["p"]), shape=(len(z["p"]) - 1,) * 2)
t0 = time.perf_counter()
g = nx.from_scipy_sparse_array(G)
t1 = time.perf_counter()
parts = nx.community.louvain_communities(g, weight="weight", resolution=float(sys.argv[2]), seed=0)
t2 = time.perf_counter()
print("NX", t1 - t0, t2 - t1, len(parts), nx.community.modularity(g, parts, weight="weight", resolution=float(sys.argv[2])))
"""


def networkx_time(G, gamma, limit):
    try:
        import networkx  # noqa: F401
    except ImportError:
        return {"available": False, "note": "networkx is not installed on this machine"}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "g.npz")
        np.savez(path, p=G.p, i=G.i, x=G.x)
        try:
            r = subprocess.run([sys.executable, "-c", NX_CHILD, path, str(gamma)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            return {"available": True, "finished": False, "note": "louvain_communities did not finish within %d s" % limit}
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("NX ")]
    if r.returncode != 0 or not line:
        return {"available": True, "finished": False, "note": (r.stderr or r.stdout)[-300:]}
    f = line[0].split()
    return {"available": True, "finished": True, "graph_build_s": float(f[1]), "louvain_s": float(f[2]), "clusters": int(f[3]),
            "modularity": float(f[4])}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    out_path = sys.argv[2] if len(sys.argv) > 2 else "louvain_rate.json"
    nx_limit = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    gamma, K, dim, centres = 0.8, 20, 20, 30
    rng = np.random.default_rng(1)
    C = 6.0 * rng.standard_normal((centres, dim))
    lab = rng.integers(0, centres, n)
    E = C[lab] + rng.standard_normal((n, dim))
    t0 = time.perf_counter()
    graph = sa.find_neighbors(E, k_param=K)
    t_graph = time.perf_counter() - t0
    G = sa.api._without_diagonal(graph["snn"])
    deg = np.diff(G.p)
    doc = {"cells": n, "k_param": K, "resolution": gamma, "entries": int(G.nnz), "widest_column": int(deg.max()),
           "find_neighbors_s": t_graph, "hbm_bytes_per_s_spec": HBM_BYTES_PER_S}
    full, doc["call_ms"] = timed(lambda: sa.c_louvain(G, [gamma]))
    doc["info"] = sa.louvain_info()
    L = int(full["n_levels"][0])
    doc.update(clusters=int(full["n_clusters"][0]), levels=L, sweeps_levels=full["sweeps_levels"][0][:L].tolist(),
               q_levels=full["q_levels"][0][:L].tolist())
    a, ta = timed(lambda: sa.c_louvain(G, [gamma], max_sweeps=1, max_levels=1))
    b, tb = timed(lambda: sa.c_louvain(G, [gamma], max_sweeps=11, max_levels=1))
    ka, kb = int(a["sweeps_levels"][0][0]), int(b["sweeps_levels"][0][0])
    doc["one_level_1_sweep_ms"], doc["one_level_11_sweeps_ms"], doc["sweeps_kept"] = ta, tb, [ka, kb]
    if kb > ka:
        per = (tb["median"] - ta["median"]) / (kb - ka)
        doc["level0_sweep_with_modularity_ms"] = per
        doc["entries_per_s"] = G.nnz / (per * 1e-3)
        # what one sweep and its modularity pass must move: per entry the row index (4 B), the weight (8 B) and a label
        # (4 B), twice (the sweep and own_v)
        doc["model_bytes_per_sweep"] = 32 * int(G.nnz)
        doc["fraction_of_hbm"] = doc["model_bytes_per_sweep"] / (per * 1e-3) / HBM_BYTES_PER_S
    _, doc["op_sweep_call_ms"] = timed(lambda: sa.op_louvain_sweep(G, np.arange(n, dtype=np.int32), gamma))
    doc["networkx"] = networkx_time(G, gamma, nx_limit) if nx_limit > 0 else {"available": None, "note": "not asked for"}
    with open(out_path, "w") as f:
        json.dump(doc, f)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
