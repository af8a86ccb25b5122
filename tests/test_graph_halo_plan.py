"""The halo plan of graph-convolutional NMF on a team (sgl_graph_halo_plan, host only: include/singlet_hip.h section 2b)
against a few lines of numpy, and a static look at the pack / halo convolution kernels the build emitted
(singlet_amd/csrc/asm/kernels_graph.s, Makefile ASM_UNITS).  No GPU."""
import os
import re

import numpy as np
import pytest

import gcnmf_restatement as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "singlet_amd", "csrc", "asm", "kernels_graph.s")


def _even(n, ranks):
    """the split of Multi.synth: the first n % ranks blocks one cell longer"""
    base, rem = divmod(n, ranks)
    return np.concatenate([[0], np.cumsum([base + (r < rem) for r in range(ranks)])]).astype(np.int64)


def _np_plan(p, i, lo):
    """crossing entries, export lists and E straight from their definitions"""
    n, ranks = len(p) - 1, len(lo) - 1
    col = np.repeat(np.arange(n), np.diff(p))
    own_row = np.searchsorted(lo, i, side="right") - 1
    own_col = np.searchsorted(lo, col, side="right") - 1
    cross = own_row != own_col
    export = [np.unique(i[cross & (own_row == s)]) for s in range(ranks)]
    return int(cross.sum()), export, max(len(e) for e in export)


def _read_back(plan, p, lo):
    """global row of every entry, from the rewritten indices and the export lists"""
    E = plan["E"]
    out = np.empty_like(plan["i_local"])
    for r in range(len(lo) - 1):
        q0, q1 = p[lo[r]], p[lo[r + 1]]
        li = plan["i_local"][q0:q1].astype(np.int64)
        n_local = lo[r + 1] - lo[r]
        g = li + lo[r]
        far = li >= n_local
        if far.any():
            s, pos = np.divmod(li[far] - n_local, E)
            assert np.all(s != r) and np.all(s < len(lo) - 1)
            g[far] = np.array([plan["export"][a][b] for a, b in zip(s, pos)])
        out[q0:q1] = g
    return out


def _check_plan(sa, G, lo):
    plan = sa.graph_halo_plan(G.p, G.i, lo)
    crossing, export, E = _np_plan(np.asarray(G.p), np.asarray(G.i), lo)
    assert plan["edges"] == G.p[-1] and plan["crossing"] == crossing and plan["E"] == E
    assert len(plan["export"]) == len(lo) - 1
    for r, (got, ref) in enumerate(zip(plan["export"], export)):
        assert np.array_equal(got, ref), r                         # ascending and without duplicates, as np.unique gives them
        assert np.all(got >= lo[r]) and np.all(got < lo[r + 1]), r  # inside their owner's block
    # the rewritten graph names the same global row at every stored position (the values stay where they are)
    assert np.array_equal(_read_back(plan, np.asarray(G.p), lo), np.asarray(G.i))
    return plan


@pytest.mark.parametrize("side,ranks", [(18, 3), (18, 4), (24, 8)])
def test_small_lattices(sa, ora, side, ranks):
    G = gr.lattice_graph(ora, side)
    plan = _check_plan(sa, G, _even(side * side, ranks))
    assert 0 < plan["E"] <= 2 * (side + 1)


@pytest.mark.parametrize("ranks,crossing,E", [(8, 41972, 2000), (7, 35988, 2002)])
def test_million_cell_lattice(sa, ora, ranks, crossing, E):
    side = 1000
    G = gr.lattice_graph(ora, side)
    assert G.p[-1] == 8988004
    plan = _check_plan(sa, G, _even(side * side, ranks))
    assert plan["crossing"] == crossing and plan["E"] == E and E <= 2 * (side + 1)


@pytest.mark.parametrize("kind", ["directed", "odd", "hub", "lattice_perm"])
def test_uneven_boundaries(sa, ora, kind):
    n = 400
    if kind == "directed":
        G = gr.random_directed_graph(ora, n, 5, seed=11)
    elif kind == "odd":
        G = gr.sparse_odd_graph(ora, n, seed=12)
    elif kind == "hub":
        G = gr.hub_graph(ora, n, hub=123, hub_len=300, seed=9)
    else:
        G = gr.lattice_graph(ora, 20, perm=np.random.default_rng(4).permutation(n))
    for lo in ([0, 1, 130, 131, 300, 400], [0, 399, 400], [0, 400], [0, 57, 58, 59, 211, 212, 390, 400]):
        _check_plan(sa, G, np.array(lo, dtype=np.int64))


def test_block_without_any_crossing_edge(sa, ora):
    """cells 100 .. 149 only have edges among themselves: their rank exports nothing and imports nothing"""
    n = 300
    G = gr.random_directed_graph(ora, n, 4, seed=3)
    i, p, x = np.asarray(G.i), np.asarray(G.p), np.asarray(G.x)
    col = np.repeat(np.arange(n), np.diff(p))
    inside = lambda c: (c >= 100) & (c < 150)
    keep = inside(i) == inside(col)
    cnt = np.bincount(col[keep], minlength=n)
    G2 = ora.CSC(x[keep], i[keep], np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), n, n)
    lo = np.array([0, 100, 150, 151, 300], dtype=np.int64)
    plan = _check_plan(sa, G2, lo)
    assert plan["export"][1].size == 0 and plan["E"] > 0
    q0, q1 = G2.p[100], G2.p[150]
    assert np.all(plan["i_local"][q0:q1] < 50)


def test_identity_graph_has_no_halo(sa, ora):
    G = gr.identity_graph(ora, 50)
    plan = _check_plan(sa, G, np.array([0, 10, 11, 50], dtype=np.int64))
    assert plan["E"] == 0 and plan["crossing"] == 0 and all(e.size == 0 for e in plan["export"])
    assert np.array_equal(plan["i_local"], np.concatenate([np.arange(10), [0], np.arange(39)]))


def test_bad_plans_are_refused(sa, ora):
    G = gr.lattice_graph(ora, 6)
    for lo in ([0, 10, 10, 36], [0, 10, 30], [1, 10, 36]):
        with pytest.raises(sa.SingletHipError):
            sa.graph_halo_plan(G.p, G.i, np.array(lo, dtype=np.int64))
    bad = np.asarray(G.i).copy()
    bad[3] = 36
    with pytest.raises(sa.SingletHipError):
        sa.graph_halo_plan(G.p, bad, np.array([0, 18, 36], dtype=np.int64))


def _kernels(text):
    """{symbol: (body, private segment size)} of every kernel in the assembly"""
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\s*s_endpgm", text, flags=re.M | re.S):
        d = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(m.group(1)), text, flags=re.S)
        if d:
            out[m.group(1)] = (m.group(2), int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d.group(1)).group(1)))
    return out


def test_pack_and_halo_convolution_code(sa):
    if not os.path.exists(ASM):
        import __graft_entry__
        __graft_entry__.build()
    ks = _kernels(open(ASM).read())
    pack = {v: [n for n in ks if re.match(r"_Z17graph_pack_kernelILi%dEE" % v, n)] for v in (1, 2)}
    assert all(len(pack[v]) == 1 for v in (1, 2)), sorted(ks)
    # graph_conv_kernel<VEC, LPC, NP, SEGS, HALO>: the halo instances, main pass and hub segments, in both VEC forms
    conv = re.compile(r"_Z17graph_conv_kernelILi(\d)ELi(\d+)ELi(\d+)ELb([01])ELb([01])EE")
    halo = {}
    plain = 0
    for n in ks:
        m = conv.match(n)
        if not m:
            continue
        if m.group(5) == "1":
            halo.setdefault((int(m.group(1)), m.group(4) == "1"), []).append(n)
        else:
            plain += 1
    assert all(len(halo.get((v, s), [])) == 11 for v in (1, 2) for s in (False, True)), {k: len(v) for k, v in halo.items()}
    assert plain == 44   # the one-context instances are all still there
    for name in pack[1] + pack[2] + [n for v in halo.values() for n in v]:
        assert ks[name][1] == 0, (name, "scratch")
    for name in pack[2] + halo[(2, False)] + halo[(2, True)]:
        assert "global_load_dwordx4" in ks[name][0], name
    for name in pack[2]:
        assert "global_store_dwordx4" in ks[name][0], name
