"""The numpy restatement of the gene set enrichment test (gsea_restatement.py) against independent yardsticks, the Python
mirror's filters against a literal transcription of the reference's lines, and the host-side wiring: the header's entries
and their bindings, the exported names, the Makefile's object and flag, and the host logic of the library
(singlet_amd/csrc/gsea_host.h) compiled alone under the address and undefined-behaviour sanitizers.

Bounds.  ES against the textbook walk over all m genes: 1e-11.  The walk adds s hit steps and m - s miss steps one by one,
the rule forms cum_i / NR - misses_i / (m - s) from a prefix sum of at most s terms: at the shapes here (m <= 2000) the two
orders differ by about (s + m) * 2^-52, some 5e-13.
Calibration.  m = 1500, 65 % zeros, 600 random sets of sizes 11 to 60, nperm = 999: the share of p <= 0.05 per factor lies in
0.05 +- 0.045: four standard deviations of the binomial share of 600 sets (0.0089) combined with the sampling error of the
null's 5 % quantile (0.0069, shared by the sets of one size): 4 * sqrt(0.0089^2 + 0.0069^2) = 0.045.  Derived, not tuned."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gsea_restatement as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgl_c_gsea", "sgl_gsea_info", "sgl_op_gsea_es", "sgl_op_gsea_null")


def sets_of(rng, m, sizes):
    sets = [rng.choice(m, size=s, replace=False) for s in sizes]
    return np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64), np.concatenate(sets), sets


def l1_factor(rng, m, zeros=0.65):
    return rng.random(m) * (rng.random(m) >= zeros)


# ------------------------------------------------------------------------------------------ the score
def test_the_hash_is_the_oracles():
    from oracle.np_transcription import rand_np, rand_py
    rng = np.random.default_rng(0)
    i = rng.integers(0, 2**63, size=200, dtype=np.uint64)
    j = rng.integers(0, 2**63, size=200, dtype=np.uint64)
    assert np.array_equal(gr.rand2(12345, i, j), rand_np(12345, i, j))
    assert int(gr.rand2(7, [3], [11])[0]) == rand_py(7, 3, 11)


@pytest.mark.parametrize("m", [66, 700, 2000])
def test_es_equals_the_textbook_walk(m):
    rng = np.random.default_rng(m)
    w = np.stack([l1_factor(rng, m), np.round(rng.normal(size=m), 2), rng.random(m)], axis=1)
    sizes = [s for s in (1, 2, 11, 37, 63, 64, 65, 128, 129, 500, m - 1) if s < m]
    ptr, genes, sets = sets_of(rng, m, sizes)
    ep, en, es = gr.observed(w, ptr, genes)
    worst = 0.0
    for f in range(w.shape[1]):
        for j, s in enumerate(sets):
            hi, lo = gr.textbook_es(w[:, f], s)
            worst = max(worst, abs(hi - ep[j, f]), abs(lo - en[j, f]))
    print("m = %d: largest distance from the textbook walk %.3g" % (m, worst))
    assert worst <= 1e-11
    assert (ep >= 0).all() and (en <= 0).all()


def test_the_prefix_sums_follow_the_stated_order():
    """One block: lane l of the ladder is the pairwise tree of its 64-aligned history, not the sequential sum; the carry is
    added after the ladder.  Held on values where the orders differ in the last place."""
    rng = np.random.default_rng(1)
    a = rng.random((1, 130)) * 10.0 ** rng.integers(-8, 8, size=(1, 130))
    cum = gr.prefix_sums(a)[0]
    x = a[0]
    assert cum[0] == x[0] and cum[1] == x[0] + x[1]
    assert cum[3] == (x[0] + x[1]) + (x[2] + x[3])                      # not ((x0 + x1) + x2) + x3
    assert cum[2] == x[0] + (x[1] + x[2])                                # lane 2: d = 1 gives x1 + x2, d = 2 adds lane 0
    first = cum[63]
    assert cum[64] == first + x[64] and cum[65] == first + (x[64] + x[65])
    assert cum[127] == first + gr.prefix_sums(a[:, 64:128])[0][63] and cum[128] == cum[127] + x[128]
    seq = np.cumsum(x)
    assert np.abs(cum - seq).max() <= 130 * 2.0**-52 * seq[-1] and (cum != seq).any()


def test_zero_weight_hits_follow_fgseas_rule():
    """NR == 0: every hit steps 1 / s.  Not exotic: with 65 % zeros some null sets of size 11 have no weight at all."""
    m = 40
    w = np.zeros(m)
    w[:5] = [5, 4, 3, 2, 1]
    pos, aw = gr.ranking(w)
    p = np.array([[10, 20, 30]])
    ep, en = gr.scores(p, aw, m)
    tops = [1 / 3 - 10 / 37, 2 / 3 - 19 / 37, 3 / 3 - 28 / 37]
    assert ep[0] == max(tops) and en[0] == min(t - 1 / 3 for t in tops)
    rng = np.random.default_rng(3)
    wf = l1_factor(rng, 1500)
    null = gr.null_scores(wf[:, None], [11], 0, 5, 0, 999)
    pos, aw = gr.ranking(wf)
    sample = gr.null_sample(5, 0, 999, 1500, 11)
    weightless = int((aw[pos[sample]].sum(axis=1) == 0).sum())
    print("null sets of size 11 without weight: %d of 999" % weightless)
    assert weightless >= 1 and np.isfinite(null).all()


def test_ties_go_by_gene_index_and_both_zeros_are_one_run():
    w = np.array([0.0, 2.0, -0.0, 2.0, 0.0, -1.0, 3.0])
    pos, aw = gr.ranking(w)
    assert pos.tolist() == [3, 1, 4, 2, 5, 6, 0] and aw.tolist() == [3.0, 2.0, 2.0, 0.0, 0.0, 0.0, 1.0]
    # of two genes without weight the one with the smaller index ranks first: its set scores no lower
    ep = gr.observed(w[:, None], np.array([0, 1, 2]), [0, 4])[0]
    assert ep[0, 0] == 1.0 - 3.0 / 6.0 and ep[1, 0] == 1.0 - 5.0 / 6.0


def test_the_std_rule():
    assert gr.std_score([0.5, 0.25, 0.5, 0.0], [-0.25, -0.5, -0.5, 0.0]).tolist() == [0.5, -0.5, 0.0, 0.0]
    assert not np.signbit(gr.std_score([0.5], [-0.5]))[0]
    rng = np.random.default_rng(4)
    w = np.round(rng.normal(size=(400, 1)), 2)
    ptr, genes, _ = sets_of(rng, 400, [15] * 30)
    ep, en, es = gr.observed(w, ptr, genes)
    assert np.array_equal(es, np.where(ep > -en, ep, np.where(ep < -en, en, 0.0))) and (es > 0).any() and (es < 0).any()


def test_a_planted_set_reaches_the_floor():
    rng = np.random.default_rng(6)
    m, nperm = 1500, 999
    w = l1_factor(rng, m)[:, None]
    top = np.argsort(-w[:, 0], kind="stable")[:30]
    ptr, genes, _ = sets_of(rng, m, [30, 30])
    genes[:30] = top[rng.permutation(30)]
    out = gr.gsea(w, ptr, genes, 0, nperm, seed=11)
    assert abs(out["es"][0, 0] - 1.0) <= 2 * 2.0**-52
    assert out["n_ge"][0, 0] == 0 and out["pval"][0, 0] == 1.0 / (nperm + 1)
    assert out["pval"][1, 0] > 0.001 and out["nes"][0, 0] > out["nes"][1, 0]
    assert out["padj"][0, 0] == 2.0 / (nperm + 1)


# ------------------------------------------------------------------------------------------ the null
def test_the_null_sets_are_nested_and_shared_by_the_factors():
    s = gr.null_sample(21, 3, 9, 500, 40)
    assert s.shape == (6, 40) and all(np.unique(r).size == 40 for r in s)
    assert np.array_equal(gr.null_sample(21, 5, 6, 500, 17)[0], s[2, :17])
    key = gr.rand2(21, np.full(500, 5, dtype=np.uint64), np.arange(500, dtype=np.uint64))
    assert np.array_equal(s[2], np.argsort(key, kind="stable")[:40])


def test_the_statistics_of_one_factor_by_hand():
    rng = np.random.default_rng(8)
    m, nperm = 300, 60
    w = np.round(rng.normal(size=(m, 1)), 1)
    ptr, genes, _ = sets_of(rng, m, [12, 12, 20])
    for st in (0, 1, 2):
        out = gr.gsea(w, ptr, genes, st, nperm, seed=2)
        null = out["null"][0]
        for j, si in ((0, 0), (1, 0), (2, 1)):
            e, v = out["es"][j, 0], null[si]
            assert out["n_ge"][j, 0] == (v >= e).sum() and out["n_le"][j, 0] == (v <= e).sum()
            if st == 0:
                assert e >= 0 and out["pval"][j, 0] == (1 + (v >= e).sum()) / (1 + nperm) and out["n_side"][j, 0] == (v >= 0).sum()
            elif st == 1:
                assert e <= 0 and out["pval"][j, 0] == (1 + (v <= e).sum()) / (1 + nperm) and out["n_side"][j, 0] == (v <= 0).sum()
            else:
                side = v[v >= 0] if e >= 0 else v[v <= 0]
                hits = (side >= e).sum() if e >= 0 else (side <= e).sum()
                assert out["pval"][j, 0] == (1 + hits) / (1 + side.size) and out["n_side"][j, 0] == side.size
                assert abs(out["nes"][j, 0] - e / abs(side.mean())) <= 1e-12 * abs(out["nes"][j, 0])


def test_bh_equals_the_plain_form():
    rng = np.random.default_rng(9)
    for n in (1, 2, 17, 200):
        p = np.round(rng.random(n) ** 2, 2)            # ties among them
        p[rng.random(n) < 0.1] = np.nan
        a, b = gr.bh(p), gr.bh_plain(p)
        assert np.array_equal(np.isnan(a), np.isnan(p))
        ok = ~np.isnan(p)
        assert np.allclose(a[ok], b[ok], rtol=1e-14, atol=0) and (a[ok] >= p[ok]).all() and (a[ok] <= 1).all()
    assert np.isnan(gr.bh([np.nan, np.nan])).all() and gr.bh([]).size == 0


def test_calibration_on_random_sets():
    rng = np.random.default_rng(2025)
    m, nperm = 1500, 999
    w = np.stack([l1_factor(rng, m) for _ in range(3)], axis=1)
    ptr, genes, _ = sets_of(rng, m, rng.integers(11, 61, size=600).tolist())
    out = gr.gsea(w, ptr, genes, 0, nperm, seed=99)
    share = (out["pval"] <= 0.05).mean(axis=0)
    print("share of p <= 0.05 per factor:", share)
    assert (np.abs(share - 0.05) <= 0.045).all(), share


# ------------------------------------------------------------------------------------------ the mirror
def _reference_filters(pathways, rownames, w, min_size, max_size):
    """R/RunGSEA.R:36-64 and fgsea's preparePathwaysAndStats / padData, line by line, on Python lists."""
    pathways = {n: v for n, v in pathways.items() if len(v) > min_size}                        # l.36
    genes_in_pathways = set()                                                                 # l.39
    for v in pathways.values():
        genes_in_pathways.update(v)
    keep_rows = [i for i, g in enumerate(rownames) if g in genes_in_pathways]                 # l.54
    rn = [rownames[i] for i in keep_rows]
    w = w[keep_rows]
    pathways = {n: [g for g in v if g in set(rn)] for n, v in pathways.items()}               # l.55
    pathways = {n: v for n, v in pathways.items() if min_size < len(v) < max_size}            # l.56-57
    row_sum = w.sum(axis=1)                                                                   # l.60
    if (row_sum == 0).any():
        keep = np.nonzero(row_sum != 0)[0]
        w, rn, keep_rows = w[keep], [rn[i] for i in keep], [keep_rows[i] for i in keep]
    where = {g: i for i, g in enumerate(rn)}
    tested = {}
    for n, v in pathways.items():                                                             # fgsea: match, unique, size filter
        ids = []
        for g in v:
            if g in where and where[g] not in ids:
                ids.append(where[g])
        tested[n] = (ids, min_size <= len(ids) <= max_size)
    return keep_rows, tested


def test_the_mirrors_filters_equal_the_reference_lines(tmp_path):
    import singlet_amd as sa
    rng = np.random.default_rng(10)
    m = 400
    names = ["G%d" % i for i in range(m)]
    w = rng.random((m, 3)) * (rng.random((m, 3)) < 0.4)
    w[rng.random(m) < 0.3] = 0.0                                   # rows that are zero in every factor
    pathways = {}
    for q in range(60):
        size = int(rng.integers(3, 40))
        genes = [names[g] for g in rng.choice(m, size=size, replace=False)] + ["absent%d" % q] * int(rng.integers(0, 3))
        if q % 7 == 0:
            genes.append(genes[0])                                 # a gene listed twice
        pathways["set%d" % q] = genes
    pathways["exactly_min"] = names[:10]
    pathways["one_more"] = names[:11]
    pathways["zero_rows"] = [names[i] for i in np.nonzero(w.sum(axis=1) == 0)[0][:14]]
    min_size, max_size = 10, 30
    pnames, rows, sets, tested = sa.api.gsea_filter(pathways, names, w, min_size, max_size)
    ref_rows, ref = _reference_filters(pathways, names, w, min_size, max_size)
    assert rows.tolist() == ref_rows and pnames == list(ref)
    assert "exactly_min" not in pnames and "zero_rows" in pnames and not tested[pnames.index("zero_rows")]
    for n, ids, t in zip(pnames, sets, tested):
        assert ids.tolist() == ref[n][0] and bool(t) == ref[n][1], n
    assert tested.any() and not tested.all()
    # the GMT reader gives the same dict back
    path = tmp_path / "sets.gmt"
    path.write_text("".join("%s\thttp://example/%s\t%s\n" % (n, n, "\t".join(v)) for n, v in pathways.items()) + "\n")
    assert sa.read_gmt(str(path)) == pathways


def test_the_python_layer_refuses_what_it_cannot_marshal():
    import singlet_amd as sa
    w = np.ones((5, 2))
    with pytest.raises(ValueError, match="score_type"):
        sa.c_gsea(w, [0, 2], [0, 1], score_type="two-sided")
    with pytest.raises(ValueError, match="matrix"):
        sa.c_gsea(np.ones(5), [0, 2], [0, 1])
    with pytest.raises(ValueError, match="set_ptr points past"):
        sa.c_gsea(w, [0, 3], [0, 1])
    with pytest.raises(ValueError, match="integer gene indices"):
        sa.c_gsea(w, [0, 2], [0.5, 1])
    with pytest.raises(ValueError, match="gene_names"):
        sa.run_gsea(w, {}, ["a", "b"])


# ------------------------------------------------------------------------------------------ wiring
def test_the_makefile_builds_the_unit_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_gsea.o" in objs
    assert re.search(r"^kernels_gsea\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^kernels_gsea\.o:.*\bgsea_host\.h\b", mk, flags=re.M)


def test_the_header_declares_the_entries_and_the_binding_matches():
    from singlet_amd import _lib
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"SGL_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "NO team form and NO R shim entry" in header
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "gsea_host.h")).read()
    assert "#define GSEA_BLOCK %d" % gr.BLOCK in host and "#define GSEA_LDS_CAP %d" % gr.LDS_CAP in host
    assert "#define GSEA_MAX_K %d" % gr.MAX_K in host


def test_the_python_names_are_exported():
    import singlet_amd as sa
    for name in ("c_gsea", "run_gsea", "read_gmt"):
        assert callable(getattr(sa, name)), name
    for name in ("op_gsea_es", "op_gsea_null", "gsea_info"):
        assert callable(getattr(sa.Context, name)), name


# ------------------------------------------------------------------------------------------ the host logic, sanitized
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/gsea_host_main.cpp compiled with a host compiler and both sanitizers into a program of its own."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("gsea_host") / "gsea_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "gsea_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_host_logic_under_address_and_undefined_sanitizers(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("gsea_host: ok"), r.stdout


@pytest.mark.parametrize("score_type", [0, 1, 2])
def test_host_derived_statistics_equal_the_restatement(host_program, tmp_path, score_type):
    """The tallies and running sums of a restated test handed to the library's host logic: p, NES and padj bit for bit."""
    rng = np.random.default_rng(12 + score_type)
    m, k, nperm = 300, 2, 40
    w = np.round(rng.normal(size=(m, k)), 1)
    w[:, 1] = 0.0                                                  # NR == 0 everywhere
    ptr, genes, _ = sets_of(rng, m, rng.integers(5, 15, size=25).tolist())
    ref = gr.gsea(w, ptr, genes, score_type, nperm, seed=5)
    P, S = ptr.size - 1, ref["sizes"].size
    null = ref["null"]
    cnt_pos, cnt_neg = (null >= 0).sum(axis=2), (null <= 0).sum(axis=2)                # k x S
    sum_pos = np.array([[gr.running_sum(v[v >= 0]) for v in f] for f in null])
    sum_neg = np.array([[gr.running_sum(v[v <= 0]) for v in f] for f in null])
    blob = struct.pack("<5q", P, k, score_type, nperm, S) + np.searchsorted(ref["sizes"], ref["set_size"]).astype(np.int32).tobytes()
    blob += ref["es"].T.tobytes() + ref["n_ge"].T.astype(np.int64).tobytes() + ref["n_le"].T.astype(np.int64).tobytes()
    blob += cnt_pos.astype(np.int64).tobytes() + cnt_neg.astype(np.int64).tobytes() + sum_pos.tobytes() + sum_neg.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([host_program, "derive", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    f = np.frombuffer(raw[:3 * 8 * P * k], dtype=np.float64).reshape(3, k, P)
    side = np.frombuffer(raw[3 * 8 * P * k:], dtype=np.int64).reshape(k, P)
    for got, name in zip(f, ("nes", "pval", "padj")):
        want = np.ascontiguousarray(ref[name].T)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), name
        assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), name
    assert np.array_equal(side, ref["n_side"].T)
