"""The host model of the sliding-window entry stream (scripts/layout_emulate.py; kernels_tiled.hip: tiled_count_kernel): the
invariants the accumulate's bit equality rests on -- every non-zero stored exactly once, each column's entries in CSC order,
every entry inside the two LDS blocks of its stage -- and the padding it removes.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("layout_emulate", os.path.join(ROOT, "scripts", "layout_emulate.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


L = _model()


def _random_csc(m, n, density, seed):
    rng = np.random.default_rng(seed)
    D = rng.random((n, m)) < density
    D[rng.integers(0, n, 3)] = False                  # empty columns
    D[:, m // 3: m // 3 + 40] = False                 # rows without entries
    D[5] = True                                       # a dense column
    D[6, m - 30:] = True                              # a column whose entries sit in the last rows only
    i = np.nonzero(D)[1].astype(np.int64)
    p = np.concatenate([[0], np.cumsum(D.sum(axis=1))]).astype(np.int64)
    return p, i


@pytest.mark.parametrize("nsl,TR,ranges", [(2, 408, 1), (2, 408, 3), (4, 632, 1), (4, 96, 2), (2, 64, 5)])
def test_schedule_stores_every_entry_once_in_order_inside_its_window(nsl, TR, ranges):
    m, n = 2111, 300
    p, i = _random_csc(m, n, 0.04, 7 + TR)
    trace = []
    cnt = L.stream_counts(p, i, m, TR, nsl, ranges=ranges, trace=trace)
    D = TR // 2
    T = (m + TR - 1) // TR
    NB = (m + D - 1) // D
    assert cnt.max() <= 255
    ends = {}
    for b0, b1 in L.block_ranges(T, NB, min(ranges, T)):
        for b in range(b0, b1):
            ends[b] = b1
    seen = np.zeros(p[-1], dtype=np.int64)
    nxt = p[:-1].copy()
    for col, a, n_, b in trace:
        assert a == nxt[col], "entries of a column out of CSC order"
        nxt[col] += n_
        seen[a:a + n_] += 1
        rows = i[a:a + n_]
        assert rows.min() >= b * D and rows.max() < min(b + 2, ends[b]) * D, "an entry outside the LDS window of its stage"
    assert np.all(seen == 1)
    assert np.array_equal(nxt, p[1:])
    # the chunks are whole 64-slot sets
    assert np.all(cnt.sum(axis=2) % (16 // nsl) == 0)


def test_sliding_window_padding_on_iid_columns():
    """30 000 rows, 5 % non-zero, k = 50 (408-row tiles): at most 1.08 stored entries per non-zero, against 1.19 - 1.23 for
    runs padded in lock step per tile"""
    rng = np.random.default_rng(0)
    m, n = 30000, 1500
    D = rng.random((n, m)) < 0.05
    i = np.nonzero(D)[1].astype(np.int64)
    p = np.concatenate([[0], np.cumsum(D.sum(axis=1))]).astype(np.int64)
    nnz = int(p[-1])
    for nsl, k in ((2, 50), (4, 30)):
        TR = L.tile_rows(k, nsl)
        assert L.entries(p, i, m, k, nsl, TR) / nnz <= 1.08
        assert L.lockstep_entries(p, i, m, TR, nsl) / nnz >= 1.18
