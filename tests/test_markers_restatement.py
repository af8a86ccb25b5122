"""The numpy restatement of sgl_markers (markers_restatement.py) against scipy.stats.mannwhitneyu, its invariants, and the
host-side wiring: the header's entries and their bindings, the exported names, the Makefile's object and flag, and the host
logic of the library (singlet_amd/csrc/markers_host.h) compiled alone under the address and undefined-behaviour sanitizers.

The bound against scipy is 1e-12 relative wherever scipy's p >= 1e-300: both evaluate the same normal approximation with
the same tie and continuity corrections in double; scipy forms the rank sum in floating point (midranks n / 2), this library
in integers, and the survival function differs from erfc by a few units in the last place."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
from scipy import stats

import markers_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgl_markers", "sgl_c_markers", "sgl_markers_info", "sgl_op_marker_sums", "sgl_op_marker_ranks")


def _dense_gene(x, cells, n):
    d = np.zeros(n)
    d[cells] = x
    return d


def _gene(rng, n, density, values):
    cells = np.sort(rng.choice(n, size=int(round(density * n)), replace=False)).astype(np.int64)
    return values(rng, cells.shape[0]), cells


def _check_against_scipy(x, cells, labels, G):
    labels = np.asarray(labels)
    n = labels.shape[0]
    group_n, N = mr.group_counts(labels, G)
    pos, nz = mr.entry_counts(x, cells, labels, G)
    rank2, tie = mr.ranks(x, cells, labels, G)
    assert int(rank2.sum()) == N * (N + 1)
    d = mr.derive(group_n, pos, mr.group_sums(x, cells, labels, G, 0), rank2, tie, 1.0)
    dense = _dense_gene(x, cells, n)
    compared = 0
    for c in range(G):
        a, b = dense[labels == c], dense[(labels >= 0) & (labels != c)]
        if a.size == 0 or b.size == 0:
            assert math.isnan(d["p"][c]) and math.isnan(d["z"][c])
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = stats.mannwhitneyu(a, b, use_continuity=True, alternative="two-sided", method="asymptotic").pvalue
        if tie == N**3 - N:
            # every included value is equal: the deviation is exactly 0.  The stated rule (and R's wilcox.test) gives NaN;
            # this scipy divides -0.5 by the zero deviation and reports sf(-inf) * 2, clipped: 1.0.  The one place where
            # the yardstick and the rule part, held here as what each of them says.
            assert math.isnan(d["p"][c]) and math.isnan(d["z"][c]) and (math.isnan(ref) or ref == 1.0), (c, d["p"][c], ref)
            continue
        if math.isnan(ref):
            assert math.isnan(d["p"][c]), (c, d["p"][c])
            continue
        assert not math.isnan(d["p"][c]), c
        if ref >= 1e-300:
            assert abs(d["p"][c] - ref) <= 1e-12 * ref, (c, d["p"][c], ref)
        compared += 1
        assert d["pct_in"][c] == np.sum(a > 0) / a.size and d["pct_out"][c] == np.sum(b > 0) / b.size
    return compared


CASES = {
    "heavy ties (integer counts)": lambda r, k: r.integers(1, 4, size=k).astype(np.float64),
    "explicit zeros": lambda r, k: np.where(r.random(k) < 0.3, 0.0, r.integers(1, 6, size=k)).astype(np.float64),
    "negatives": lambda r, k: np.round(r.normal(size=k), 1) + 0.0,
    "continuous": lambda r, k: r.random(k) + 0.5,
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("G", [1, 2, 5])
def test_p_agrees_with_scipy(case, G):
    rng = np.random.default_rng(sorted(CASES).index(case) * 10 + G)
    n = 300
    labels = rng.integers(-1 if G > 1 else 0, G, size=n)   # excluded cells among them
    if G == 5:
        labels[labels == 3] = 2                             # an empty cluster
        labels[labels == 4] = 0
        labels[7] = 4                                       # a one-cell cluster
    total = 0
    for density in (0.05, 0.5, 1.0):
        x, cells = _gene(rng, n, density, CASES[case])
        total += _check_against_scipy(x, cells, labels, G)
    assert total > 0 or G == 1   # G = 1: the rest is empty, everything is NaN


def test_the_negatives_case_puts_the_zero_block_mid_order():
    labels = np.array([0, 0, 1, 1, 0, 1, -1])
    x, cells = np.array([-2.0, 3.0, -0.0, 3.0, -2.0]), np.array([0, 1, 2, 3, 5])
    # included values: c0 {-2, 3, 0 (cell 4)}, c1 {-0 -> zero, 3, -2}; order: -2 -2 | 0 0 | 3 3: runs [0,2) [2,4) [4,6)
    rank2, tie = mr.ranks(x, cells, labels, 2)
    assert rank2.tolist() == [3 + 7 + 11, 7 + 11 + 3] and tie == 3 * (2**3 - 2)
    pos, nz = mr.entry_counts(x, cells, labels, 2)
    assert pos.tolist() == [1, 1] and nz.tolist() == [2, 2]
    assert _check_against_scipy(x, cells, labels, 2) == 2


def test_an_all_zero_gene_and_an_all_equal_gene_give_nan():
    labels = np.array([0, 1, 0, 1, 1, -1])
    for x, cells in ((np.zeros(0), np.zeros(0, dtype=np.int64)), (np.full(6, 2.5), np.arange(6)), (np.zeros(3), np.arange(3))):
        rank2, tie = mr.ranks(x, cells, labels, 2)
        assert tie == 5**3 - 5 and rank2.tolist() == [2 * 6, 3 * 6]
        assert _check_against_scipy(x, cells, labels, 2) == 0


def test_the_tie_term_of_an_all_equal_gene_at_the_cell_limit_fits_uint64():
    N = 1 << 21
    labels = np.zeros(N, dtype=np.int32)
    labels[::2] = 1
    rank2, tie = mr.ranks(np.full(N, 1.5), np.arange(N), labels, 2)
    assert tie == N**3 - N and int(np.uint64(tie)) == N**3 - N and tie < 2**63
    assert int(rank2.sum()) == N * (N + 1) and rank2[0] == rank2[1]


def test_skipping_blocks_without_a_member_leaves_the_bits_unchanged():
    rng = np.random.default_rng(5)
    n = 3 * mr.SEG + 77
    labels = rng.integers(-1, 40, size=n)          # 40 clusters over blocks of 64: most blocks miss some cluster
    labels[1000:1200] = 3                            # whole blocks of one cluster
    x = np.round(rng.normal(size=n), 3)
    x[rng.random(n) < 0.1] = -0.0                    # a member holding -0.0: the partial of +0.0 and -0.0 lanes is +0.0
    cells = np.arange(n)
    for transform in (0, 1):
        full = mr.group_sums(x, cells, labels, 40, transform, skip_empty_blocks=False)
        skip = mr.group_sums(x, cells, labels, 40, transform, skip_empty_blocks=True)
        assert full.tobytes() == skip.tobytes()
        ref, cnt = mr.group_sums_reference(x, cells, labels, 40, transform)
        absref = np.array([np.abs(np.expm1(x[labels == c]) if transform else x[labels == c]).sum() for c in range(40)])
        assert np.all(np.abs(full - ref.astype(np.float64)) <= (cnt + 2) * 2.0**-53 * absref)


def test_the_order_of_the_segments_shows_in_the_bits():
    # 1 + 2^-53 + 2^-53 in one segment rounds up at the second addition only if the small terms meet first
    x = np.zeros(mr.SEG + 64)
    x[0], x[64], x[mr.SEG] = 1.0, 2.0**-53, 2.0**-53
    s = mr.group_sums(x, np.arange(x.shape[0]), np.zeros(x.shape[0], dtype=np.int64), 1, 0)
    assert s[0] == 1.0                               # (1 + 2^-53) rounds to 1 inside segment 0, then + 2^-53 again
    x[64], x[mr.SEG + 1] = 0.0, 2.0**-53
    s = mr.group_sums(x, np.arange(x.shape[0]), np.zeros(x.shape[0], dtype=np.int64), 1, 0)
    assert s[0] == 1.0 + 2.0**-52                    # the two small terms meet in segment 1's butterfly first


def test_check_args_names_the_first_defect():
    l = np.array([0, 1, -1, 2, 1])
    assert mr.check_args(l, 5, 3, 1, 1.0) is None
    assert mr.check_args(l, 5, 2, 1, 1.0) == ("label", 3, 2)
    assert mr.check_args(np.array([0, -2, 9]), 3, 3, 1, 1.0) == ("label", 1, -2)
    assert mr.check_args(l, 5, 0, 1, 1.0)[0] == "groups" and mr.check_args(l, 5, 1025, 1, 1.0)[0] == "groups"
    assert mr.check_args(l, 5, 3, 2, 1.0)[0] == "transform"
    assert mr.check_args(l, 5, 3, 1, -1.0)[0] == "pseudocount" and mr.check_args(l, 5, 3, 1, math.nan)[0] == "pseudocount"
    assert mr.check_args(l, (1 << 21) + 1, 3, 1, 1.0)[0] == "cells"


# ------------------------------------------------------------------------------------------ wiring
def test_the_makefile_builds_the_unit_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_markers.o" in objs
    assert re.search(r"^kernels_markers\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^kernels_markers\.o:.*\bmarkers_host\.h\b", mk, flags=re.M)


def test_the_header_declares_the_entries_and_the_binding_matches():
    from singlet_amd import _lib
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"SGL_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "NO team form and NO R shim entry" in header
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "markers_host.h")).read()
    assert "#define MARKERS_SEG %d" % mr.SEG in host and "#define MARKERS_MAX_GROUPS %d" % mr.MAX_GROUPS in host


def test_the_python_names_are_exported():
    import singlet_amd as sa
    for name in ("find_all_markers", "find_markers", "c_markers"):
        assert callable(getattr(sa, name)), name
    for name in ("markers", "markers_info", "op_marker_sums", "op_marker_ranks"):
        assert callable(getattr(sa.Context, name)), name


def test_the_python_layer_refuses_before_any_upload():
    import singlet_amd as sa
    import scipy.sparse as sp
    A = sa.as_dgCMatrix(sp.csc_matrix(np.eye(4)))
    with pytest.raises(ValueError, match="one cluster id per cell"):
        sa.c_markers(A, [0, 1, 0])
    with pytest.raises(ValueError, match="integer cluster ids"):
        sa.c_markers(A, [0.5, 1, 0, 1])
    with pytest.raises(ValueError, match="transform"):
        sa.c_markers(A, [0, 1, 0, 1], transform="log")
    with pytest.raises(ValueError, match="both groups"):
        sa.find_markers(A, [0, 1], [1, 2])
    with pytest.raises(ValueError, match="cell indices"):
        sa.find_markers(A, [0, 4])


# ------------------------------------------------------------------------------------------ the host logic, sanitized
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/markers_host_main.cpp compiled with a host compiler and both sanitizers into a program of its own."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("markers_host") / "markers_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "markers_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_host_logic_under_address_and_undefined_sanitizers(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("markers_host: ok"), r.stdout


def test_host_batches_equal_the_greedy_rule(host_program, tmp_path):
    rng = np.random.default_rng(11)
    for cap in (1, 50, 4000, 0):
        lens = rng.integers(1, 3000, size=200).astype(np.int64)
        lens[17] = 9000   # above every cap but the default
        (tmp_path / "in.bin").write_bytes(struct.pack("<qq", lens.size, cap) + lens.tobytes())
        r = subprocess.run([host_program, "batches", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.int64)
        limit = min(cap if cap > 0 else 1 << 27, 2**31 - 1)
        cut, s = [0], 0
        while s < lens.size:   # whole genes in order, greedily; a gene above the limit alone
            e, tot = s + 1, int(lens[s])
            while e < lens.size and tot + int(lens[e]) <= limit:
                tot += int(lens[e])
                e += 1
            cut.append(e)
            s = e
        assert got[0] == len(cut) - 1 and got[1:].tolist() == cut, cap


def test_host_derived_statistics_equal_the_restatement(host_program, tmp_path):
    """Integer inputs written here (consistent ones: rank sums and tie terms of real genes, plus an empty cluster and an
    all-tied gene): z bit for bit, p within 4 spacings of math.erfc, the ratios bit for bit, log2fc within the two log2's
    last places."""
    rng = np.random.default_rng(3)
    n, G, m = 500, 4, 60
    labels = rng.integers(-1, 3, size=n)   # cluster 3 is empty
    group_n, _ = mr.group_counts(labels, G)
    pos, sums, rank2 = np.zeros((m, G), dtype=np.int64), np.zeros((m, G)), np.zeros((m, G), dtype=np.int64)
    tie = np.zeros(m, dtype=np.uint64)
    for g in range(m):
        k = int(rng.integers(0, n + 1))
        cells = np.sort(rng.choice(n, size=k, replace=False))
        x = rng.integers(1, 5, size=k).astype(np.float64) if g % 2 else rng.random(k) * 3
        if g == 5:
            x, cells = np.full(n, 2.0), np.arange(n)
        pos[g], _ = mr.entry_counts(x, cells, labels, G)
        rank2[g], t = mr.ranks(x, cells, labels, G)
        tie[g] = t
        sums[g] = mr.group_sums(x, cells, labels, G, 1)
    blob = struct.pack("<iid", m, G, 0.5) + group_n.tobytes() + pos.T.tobytes() + sums.T.tobytes() + rank2.T.tobytes() + tie.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([host_program, "derive", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64).reshape(5, G, m)
    seen_nan = seen_num = 0
    for g in range(m):
        d = mr.derive(group_n, pos[g], sums[g], rank2[g], int(tie[g]), 0.5)
        for c in range(G):
            pi, po, fc, z, p = got[:, c, g]
            for a, b in ((pi, d["pct_in"][c]), (po, d["pct_out"][c]), (z, d["z"][c])):
                assert np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b)), (g, c, a, b)
            if math.isnan(d["p"][c]):
                assert math.isnan(p)
                seen_nan += 1
            else:
                assert abs(p - d["p"][c]) <= 4 * np.spacing(d["p"][c]), (g, c, p, d["p"][c])
                seen_num += 1
            if math.isnan(d["log2fc"][c]):
                assert math.isnan(fc)
            else:
                mean_in = sums[g, c] / group_n[c]
                bound = 4 * 2.0**-53 * (abs(math.log2(mean_in + 0.5)) + abs(d["log2fc"][c]) + 1.0)
                assert abs(fc - d["log2fc"][c]) <= bound, (g, c, fc, d["log2fc"][c])
    assert seen_nan >= m + 3 and seen_num >= 100   # the empty cluster everywhere, the all-tied gene, and real numbers
