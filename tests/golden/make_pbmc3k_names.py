#!/usr/bin/env python3
"""Decodes the names of the reference's bundled data file data/pbmc3k.RData into tests/golden/pbmc3k_names.npz without R: the
13714 gene names (the row names of the counts matrix) as a bytes array, and the `cell_type` factor as int8 codes 1..9 with
0 for NA.  Data only; the counts themselves are tests/golden/pbmc3k_counts.npz (make_pbmc3k.py, whose XDR reader this
imports).  Run in the authoring container (reads the reference's data file); the output is committed DATA.
"""
import bz2
import os

import numpy as np

from make_pbmc3k import HERE, SRC, R, read_item


def main():
    raw = bz2.decompress(open(SRC, "rb").read())
    assert raw[:5] == b"RDX3\n" and raw[5:7] == b"X\n", raw[:8]
    r = R(raw)
    r.o = 7
    r.i32(); r.i32(); r.i32()          # format version, writer R version, min reader version
    n = r.i32()                        # native encoding
    r.o += n
    top = read_item(r, [])
    obj = dict((k, v) for k, v in top)["pbmc3k"]
    genes = obj["Dimnames"][0]
    assert len(genes) == 13714 and all(isinstance(g, str) and g.isascii() for g in genes)
    ct = np.asarray(obj["cell_type"], dtype=np.int64)   # a factor: codes 1 .. n_levels, NA = INT_MIN
    assert ct.shape == (2700,)
    na = ct == -2**31
    assert ct[~na].min() == 1 and ct[~na].max() == 9, (ct[~na].min(), ct[~na].max())
    codes = np.where(na, 0, ct).astype(np.int8)
    # the rows named MT-* are the mt_rows of the counts fixture
    counts = np.load(os.path.join(HERE, "pbmc3k_counts.npz"))
    mt = np.array([q for q, g in enumerate(genes) if g.startswith("MT-")], dtype=np.int32)
    assert np.array_equal(mt, counts["mt_rows"])
    np.savez_compressed(os.path.join(HERE, "pbmc3k_names.npz"), genes=np.array([g.encode("ascii") for g in genes]), cell_type=codes)
    print("pbmc3k names:", len(genes), "genes;", int(na.sum()), "cells without a type; cells per type", np.bincount(codes)[1:].tolist())


if __name__ == "__main__":
    main()
