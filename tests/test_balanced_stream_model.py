"""The balance rule of the entry-stream builder in its host model (scripts/layout_emulate.py `stream_counts(balance=True)`;
kernels_tiled.hip: tiled_count_kernel): a wave block whose chunk is shorter than the longest of its workgroup's eight takes
the difference as run-ahead.  The invariants the accumulate's bit equality rests on hold as without it -- every non-zero
stored exactly once, each column's entries in CSC order, every entry inside the two LDS blocks of its stage -- and the
chunks of a stage come out level.  `balance=False` is the rule before it, the reference here.  No GPU."""
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
    D[6, :] = False
    D[6, m - 30:] = True                              # a column whose entries sit in the last rows only
    i = np.nonzero(D)[1].astype(np.int64)
    p = np.concatenate([[0], np.cumsum(D.sum(axis=1))]).astype(np.int64)
    return p, i


def _check_invariants(p, i, m, TR, nsl, wg_ranges, **kw):
    """wg_ranges(wg) = the tile ranges of workgroup wg"""
    trace = []
    cnt = L.stream_counts(p, i, m, TR, nsl, trace=trace, balance=True, **kw)
    D = TR // 2
    T = (m + TR - 1) // TR
    NB = (m + D - 1) // D
    CW = 32 * nsl
    assert cnt.shape == ((p.size - 1 + CW - 1) // CW, NB, 32)
    assert cnt.max() <= 255
    pos_of = np.empty(p.size - 1, dtype=np.int64)
    pos_of[L.sorted_perm(p)] = np.arange(p.size - 1)
    ends = {}
    for wg in range((cnt.shape[0] + 7) // 8):
        for b0, b1 in L.block_ranges(T, NB, min(wg_ranges(wg), T)):
            for b in range(b0, b1):
                ends[wg, b] = b1
    seen = np.zeros(p[-1], dtype=np.int64)
    nxt = p[:-1].copy()
    last_b = np.full(p.size - 1, -1)
    for col, a, n_, b in trace:
        assert a == nxt[col], "entries of a column out of CSC order"
        assert b >= last_b[col], "a column's stages out of order"
        last_b[col] = b
        nxt[col] += n_
        seen[a:a + n_] += 1
        rows = i[a:a + n_]
        wg = pos_of[col] // (8 * CW)
        assert rows.min() >= b * D and rows.max() < min(b + 2, ends[wg, b]) * D, "an entry outside the LDS window of its stage"
        assert n_ <= 4 * cnt[pos_of[col] // CW, b, pos_of[col] % CW // nsl], "more entries than the unit's groups hold"
    assert np.all(seen == 1)
    assert np.array_equal(nxt, p[1:])
    # the chunks are whole 64-slot sets
    assert np.all(cnt.sum(axis=2) % (16 // nsl) == 0)
    return cnt


# 1100 columns: 18 wave blocks of pairs (1100 = 17 * 64 + 12), nine of quads (8 * 128 + 76) -- the last workgroup has two
# wave blocks or one, and its last wave block units without columns.  1101 columns add a unit with an absent column beside
# present ones in both layouts.
@pytest.mark.parametrize("ncol", [1100, 1101])
@pytest.mark.parametrize("nsl,TR,ranges", [(2, 408, 1), (2, 408, 3), (4, 632, 1), (4, 96, 2), (2, 64, 5)])
def test_balanced_schedule_stores_every_entry_once_in_order_inside_its_window(nsl, TR, ranges, ncol):
    m = 2111
    p, i = _random_csc(m, ncol, 0.04, 7 + TR)
    cnt = _check_invariants(p, i, m, TR, nsl, lambda wg: ranges, ranges=ranges)
    assert cnt.shape[0] % 8 != 0
    assert (ncol % nsl != 0) == (ncol == 1101)
    # the rule changes something on this matrix: the invariants above are not those of the reference rule by accident.  (Not
    # with blocks of 32 or 48 rows: a column has one or two entries in a window there, never the four of a whole group.)
    if TR >= 408:
        assert not np.array_equal(cnt, L.stream_counts(p, i, m, TR, nsl, ranges=ranges, balance=False))


def test_balanced_schedule_with_a_tail_split():
    """The workgroups from tail_wg0 on are cut into tail_R ranges, the others run the range whole"""
    m, ncol, nsl, TR = 2111, 1101, 2, 204      # three workgroups of pairs, the last one partial
    p, i = _random_csc(m, ncol, 0.04, 11)
    cnt = _check_invariants(p, i, m, TR, nsl, lambda wg: 4 if wg >= 1 else 1, tail_wg0=1, tail_R=4)
    assert cnt.shape[0] == 18
    whole = L.stream_counts(p, i, m, TR, nsl, balance=True)
    assert np.array_equal(cnt[:8], whole[:8]) and not np.array_equal(cnt[8:], whole[8:])


def test_entries_passes_the_flag_through():
    p, i = _random_csc(1500, 700, 0.05, 3)
    for bal in (False, True):
        assert L.entries(p, i, 1500, 50, 2, 408, balance=bal) == int(L.stream_counts(p, i, 1500, 408, 2, balance=bal).sum()) * 8


def test_level_spread():
    f = np.array([[0, 5, 1, 9, 9, 2] + [0] * 26, [3, 3, 3, 0, 0, 0] + [0] * 26, [1, 2, 0, 0, 0, 0] + [0] * 26])
    got = L.level_spread(f, np.array([14, 4, 7]))
    # E = 14: level 3 gives 0 + 3 + 1 + 3 + 3 + 2 = 12, level 4 would give 15; the two left go to units 4 and 3
    assert got[0, :6].tolist() == [0, 3, 1, 4, 4, 2]
    # E = 4 over three units of 3: level 1, the one left to the highest-numbered unit
    assert got[1, :6].tolist() == [1, 1, 2, 0, 0, 0]
    # the units cannot give E: each gives all it has, nothing is padded
    assert got[2, :6].tolist() == [1, 2, 0, 0, 0, 0]
    assert np.all(got[:, 6:] == 0)


def _iid(m, n, density, seed=0):
    D = np.random.default_rng(seed).random((n, m)) < density
    return np.concatenate([[0], np.cumsum(D.sum(axis=1))]).astype(np.int64), np.nonzero(D)[1].astype(np.int64)


def _critical_path(cnt):
    """(sum over workgroups and stages of the longest of the eight chunks, the same of their mean, stored groups)"""
    chunk = cnt.sum(axis=2)
    assert chunk.shape[0] % 8 == 0
    wg = chunk.reshape(chunk.shape[0] // 8, 8, -1)
    return int(wg.max(axis=1).sum()), float(wg.mean(axis=1).sum()), int(cnt.sum())


def test_balance_levels_the_chunks_of_column_pairs():
    """30 000 x 2048 i.i.d. at 5 %, k = 50 (config 3's cell side, four workgroups): the stages' longest chunks add up to at
    most 0.95 of the reference rule's, at no more than 1.005 of its stored entries, and the longest chunk of a stage is
    within 3 % of the mean"""
    m, n = 30000, 2048
    p, i = _iid(m, n, 0.05)
    TR = L.tile_rows(50, 2)
    ref = _critical_path(L.stream_counts(p, i, m, TR, 2, balance=False))
    got = _critical_path(L.stream_counts(p, i, m, TR, 2, balance=True))
    print("pair: critical path %d -> %d (x %.4f), groups %d -> %d (x %.4f), longest / mean %.4f -> %.4f"
          % (ref[0], got[0], got[0] / ref[0], ref[2], got[2], got[2] / ref[2], ref[0] / ref[1], got[0] / got[1]))
    assert got[0] <= 0.95 * ref[0]
    assert got[2] <= 1.005 * ref[2]
    assert got[0] / got[1] <= 1.03


def test_balance_levels_the_chunks_of_column_quads():
    """Quad layout, k = 30, 20 000 rows: critical path at most 0.98 of the reference rule's, entries at most 1.005 x"""
    m, n = 20000, 2048
    p, i = _iid(m, n, 0.05)
    TR = L.tile_rows(30, 4)
    ref = _critical_path(L.stream_counts(p, i, m, TR, 4, balance=False))
    got = _critical_path(L.stream_counts(p, i, m, TR, 4, balance=True))
    print("quad: critical path %d -> %d (x %.4f), groups %d -> %d (x %.4f)"
          % (ref[0], got[0], got[0] / ref[0], ref[2], got[2], got[2] / ref[2]))
    assert got[0] <= 0.98 * ref[0]
    assert got[2] <= 1.005 * ref[2]
