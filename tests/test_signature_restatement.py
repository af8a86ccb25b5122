"""The numpy restatement of sgl_signature_scores (signature_restatement.py) against scipy.stats.rankdata on dense
materialisations, the range of the score, and the host-side wiring: the header's entries and their bindings, the exported
names, the Makefile's object and flag, the host half of score_signatures, the names fixture, and the host logic of the library
(singlet_amd/csrc/signature_host.h) compiled alone under the address and undefined-behaviour sanitizers.

Everything is integers up to the score: every comparison is array_equal."""
import os
import re
import subprocess

import numpy as np
import pytest

import signature_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgl_signature_scores", "sgl_c_signature_scores", "sgl_signature_info", "sgl_op_cell_ranks", "sgl_op_signature_scores")


def _dense(x, rows, m):
    d = np.zeros(m)
    d[rows] = x
    return d


def _check_cell(x, rows, m, R):
    """The integer form (closed zero block, shifted negatives) against rankdata on the dense cell."""
    x, rows = np.asarray(x, dtype=np.float64), np.asarray(rows, dtype=np.int64)
    got, zero2, z2, P, N = sr.cell_ranks(x, m, R)
    want = sr.dense_rank2(_dense(x, rows, m), R)
    assert np.array_equal(got, want[rows])
    rest = np.setdiff1d(np.arange(m), rows)
    assert np.array_equal(want[rest], np.full(rest.size, z2, dtype=np.uint64))
    Z = m - P - N
    assert zero2 == (z2 if Z > 0 else 0) and (Z > 0 or rest.size == 0)
    return got, z2


def test_restatement_equals_rankdata_on_random_cells():
    rng = np.random.default_rng(1)
    for trial in range(400):
        m = int(rng.integers(1, 60))
        L = int(rng.integers(0, m + 1))
        rows = np.sort(rng.choice(m, size=L, replace=False))
        kind = trial % 4
        if kind == 0:
            x = rng.integers(1, 4, size=L).astype(np.float64)                       # counts: long runs
        elif kind == 1:
            x = np.round(rng.normal(size=L), 1) + 0.0                               # negatives, ties, a few zeros
        elif kind == 2:
            x = rng.choice([-2.0, -1.0, 0.0, -0.0, 1.0, 3.0], size=L)               # stored zeros of either sign
        else:
            x = -rng.integers(1, 3, size=L).astype(np.float64)                      # P = 0
        R = int(rng.integers(1, m + 1))
        _check_cell(x, rows, m, R)


def test_the_named_edge_cells():
    m = 12
    for R in (1, 5, m):
        _check_cell([], [], m, R)                                                   # L = 0: all in the zero block
        _check_cell(np.full(m, 2.5), np.arange(m), m, R)                            # all equal, Z = 0
        _check_cell(np.arange(1, m + 1.0), np.arange(m), m, R)                      # Z = 0, all distinct
        _check_cell(-np.arange(1, m + 1.0), np.arange(m), m, R)                     # P = 0, Z = 0
        _check_cell([-1.0, -1.0, -3.0], [0, 4, 7], m, R)                            # P = 0
        _check_cell([0.0, -0.0, 2.0, -2.0], [1, 2, 3, 9], m, R)                     # +-0.0 stored
    got, _ = _check_cell([0.0, -0.0, 2.0, -2.0], [1, 2, 3, 9], m, m)
    assert got.tolist() == [1 + 11 + 1, 1 + 11 + 1, 2, 24]                          # the zero block [1, 11), the negative last


def test_a_midrank_of_exactly_R_is_kept_and_R_plus_a_half_is_capped():
    # positions [3, 6): midrank 5 (doubled 10); positions [3, 7): midrank 5.5 (doubled 11)
    m = 20
    x = np.array([9.0, 8.0, 7.0, 4.0, 4.0, 4.0, 1.0])
    got, _ = _check_cell(x, np.arange(7), m, 5)
    assert got[3:6].tolist() == [10, 10, 10] and got[6] == 12 and got[:3].tolist() == [2, 4, 6]
    x = np.array([9.0, 8.0, 7.0, 4.0, 4.0, 4.0, 4.0])
    got, _ = _check_cell(x, np.arange(7), m, 5)
    assert got[3:].tolist() == [12] * 4
    # the zero block itself at R and at R + 0.5: P = 2, Z = 5 -> [2, 7): midrank 5; Z = 6 -> 5.5
    assert sr.cell_ranks([3.0, 2.0], 7, 5)[2] == 10 and sr.cell_ranks([3.0, 2.0], 8, 5)[2] == 12
    # max_rank = 1: only an untied top gene keeps its rank
    assert sr.cell_ranks([3.0, 2.0], 7, 1)[0].tolist() == [2, 4] and sr.cell_ranks([3.0, 3.0], 7, 1)[0].tolist() == [4, 4]


def test_scores_equal_the_dense_form_and_stay_in_range():
    rng = np.random.default_rng(2)
    m, n = 40, 30
    import scipy.sparse as sp
    D = np.where(rng.random((m, n)) < 0.4, np.round(rng.normal(size=(m, n)), 1), 0.0)
    A = sp.csc_matrix(D)
    sets = [rng.choice(m, size=int(k), replace=False) for k in (1, 2, 5, 9, 10)] + [np.arange(m)[:10]]
    for R in (10, 17, m):
        rank2, score = sr.scores(A.data, A.indices, A.indptr, m, sets, R)
        for c in range(n):
            dense = sr.dense_rank2(D[:, c], R)
            for j, s in enumerate(sets):
                assert rank2[j, c] == dense[s].sum(dtype=np.uint64)
        for j, s in enumerate(sets):
            ns = len(s)
            assert np.array_equal(score[j], 1.0 - (rank2[j] - np.uint64(ns * (ns + 1))).astype(np.float64) / (2.0 * ns * R))
            assert score[j].max() <= 1.0 and score[j].min() >= (ns - 1) / (2.0 * R) - 1e-15
    # the two ends of the range are met: the top n_s genes untied; every gene capped
    assert sr.score_of(np.uint64(3 * 4), 3, 1500) == 1.0
    assert abs(float(sr.score_of(np.uint64(3 * 3002), 3, 1500)) - 2 / 3000.0) < 1e-15


def test_the_score_depends_only_on_the_order_within_a_cell():
    rng = np.random.default_rng(3)
    m, n = 50, 20
    import scipy.sparse as sp
    A = sp.csc_matrix(np.where(rng.random((m, n)) < 0.3, rng.integers(1, 6, size=(m, n)), 0).astype(np.float64))
    sets = [np.array([0, 3, 7]), np.arange(10, 25)]
    a = sr.scores(A.data, A.indices, A.indptr, m, sets, 20)
    b = sr.scores(np.log1p(A.data * 37.5), A.indices, A.indptr, m, sets, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ the host plan, restated
def test_check_args_names_the_first_defect():
    sp_, sg = np.array([0, 2, 3, 6]), np.array([4, 0, 9, 1, 4, 2])
    assert sr.check_args(sp_, sg, 3, 10, 3) is None
    assert sr.check_args(sp_, sg, 0, 10, 3) == ("sets", -1, 0)
    assert sr.check_args(sp_, sg, 3, 10, 11) == ("rank", -1, 11)
    assert sr.check_args(sp_, sg, 3, 10, 3, 0, -1, -1) == ("knob", 1, -1)
    assert sr.check_args(np.array([0, 2, 2, 3]), sg, 3, 10, 3) == ("empty", 1, 0)
    assert sr.check_args(sp_, sg, 3, 10, 2) == ("size", 2, 3)
    assert sr.check_args(sp_, sg, 3, 9, 3) == ("gene", 2, 9)
    assert sr.check_args(sp_, np.array([4, 0, 9, 1, 4, 1]), 3, 10, 3) == ("twice", 5, 1)


def test_the_plan_helpers():
    assert sr.passes(1024, 0) == 1 and sr.passes(1025, 0) == 2 and sr.passes(65, 64) == 2 and sr.passes(3, 1) == 3
    small, large, long_ = sr.split_paths([0, 1024, 1025, 4096, 4097], 0)
    assert small.tolist() == [0, 1] and large.tolist() == [2, 3] and long_.tolist() == [4]
    small, large, long_ = sr.split_paths([0, 64, 65, 300], 64)
    assert small.tolist() == [0, 1] and large.size == 0 and long_.tolist() == [2, 3]
    assert sr.batches([5, 5, 11, 3, 3, 3, 10], 10) == [0, 2, 3, 6, 7]
    ptr, flat = sr.gene_table([[4, 0], [9], [1, 4, 2]], 10)
    assert ptr.tolist() == [0, 1, 2, 3, 3, 5, 5, 5, 5, 5, 6] and flat.tolist() == [0, 2, 2, 0, 2, 1]


# ------------------------------------------------------------------------------------------ wiring
def test_the_makefile_builds_the_unit_without_contraction():
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_signature.o" in objs
    assert re.search(r"^kernels_signature\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    assert re.search(r"^kernels_signature\.o:.*\bsignature_host\.h\b", mk, flags=re.M)


def test_the_header_declares_the_entries_and_the_binding_matches():
    from singlet_amd import _lib
    header = open(os.path.join(ROOT, "include", "singlet_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"SGL_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "Signature scores" in header
    host = open(os.path.join(ROOT, "singlet_amd", "csrc", "signature_host.h")).read()
    for name, v in (("LDS_SMALL", sr.LDS_SMALL), ("LDS_CAP", sr.LDS_CAP), ("PASS_SETS", sr.PASS_SETS)):
        assert re.search(r"#define SIGNATURE_%s %d\b" % (name, v), host), name
    assert "#define SIGNATURE_BATCH_ENTRIES ((int64_t)1 << 27)" in host and sr.BATCH_ENTRIES == 1 << 27


def test_the_python_names_are_exported():
    import singlet_amd as sa
    for name in ("score_signatures", "c_signature_scores", "signature_parse"):
        assert callable(getattr(sa, name)), name
    for name in ("signature_scores", "signature_info", "op_cell_ranks", "op_signature_scores"):
        assert callable(getattr(sa.Context, name)), name


def test_score_signatures_parses_plus_and_minus_and_missing_genes():
    import singlet_amd as sa
    names = [b"CD3D", b"CD3E", "MS4A1", "CD79A", "LYZ"]
    sig = {"T": ["CD3D+", "CD3E", "CD3D", "MS4A1-", "NOPE", "GONE-"], "B": ["MS4A1", "CD79A"]}
    got = sa.signature_parse(sig, names, max_rank=3)
    assert got[0] == ["T", "B"]
    assert [a.tolist() for a in got[1]] == [[0, 1], [2, 3]] and [a.tolist() for a in got[2]] == [[2], []]
    assert got[3] == {"T": ["NOPE", "GONE"]}
    with pytest.raises(ValueError, match="'NOPE' of signature 'T'"):
        sa.signature_parse(sig, names, max_rank=3, missing="error")
    with pytest.raises(ValueError, match="no positive gene"):
        sa.signature_parse({"x": ["LYZ-"]}, names)
    with pytest.raises(ValueError, match="no positive gene left"):
        sa.signature_parse({"x": ["NOPE"]}, names)
    with pytest.raises(ValueError, match="more than max_rank = 1"):
        sa.signature_parse({"x": ["LYZ", "CD3D"]}, names, max_rank=1)
    with pytest.raises(ValueError, match="missing"):
        sa.signature_parse(sig, names, missing="impute")
    # int rows without names: duplicates dropped, the range held
    got = sa.signature_parse({"a": [3, 1, 3, 0]}, None, nrow=4)
    assert got[1][0].tolist() == [3, 1, 0] and got[2][0].size == 0 and got[3] == {}
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        sa.signature_parse({"a": [4]}, None, nrow=4)
    with pytest.raises(ValueError, match="int rows"):
        sa.signature_parse({"a": ["CD3D"]}, None, nrow=4)


def test_the_python_layer_refuses_before_any_upload(tmp_path):
    """No device here: every one of these raises before the library is asked for a context."""
    import singlet_amd as sa
    import scipy.sparse as sp
    A = sa.as_dgCMatrix(sp.csc_matrix(np.eye(4)))
    with pytest.raises(ValueError, match="max_rank = 1500"):
        sa.score_signatures(A, {"a": [0]})
    with pytest.raises(ValueError, match="no positive gene"):
        sa.score_signatures(A, {"a": ["g9"]}, gene_names=["g0", "g1", "g2", "g3"], max_rank=2)
    with pytest.raises(ValueError, match="more than max_rank = 2"):
        sa.score_signatures(A, {"a": [0, 1, 2]}, max_rank=2)
    with pytest.raises(ValueError, match="name the 4 rows"):
        sa.score_signatures(A, {"a": ["g0"]}, gene_names=["g0"], max_rank=2)
    with pytest.raises(ValueError, match="not among gene_names"):
        sa.score_signatures(A, {"a": ["g0", "zz"]}, gene_names=["g0", "g1", "g2", "g3"], max_rank=2, missing="error")
    gmt = tmp_path / "s.gmt"
    gmt.write_text("a\tdesc\tzz\tyy\n")
    with pytest.raises(ValueError, match="no positive gene left"):
        sa.score_signatures(A, str(gmt), gene_names=["g0", "g1", "g2", "g3"], max_rank=2)
    with pytest.raises(ValueError, match="0-based integer gene indices"):
        sa.c_signature_scores(A, [[0.5]], max_rank=2)


def test_the_names_fixture_agrees_with_mt_rows():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_names.npz"))
    counts = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    genes, ct = g["genes"], g["cell_type"]
    assert genes.shape == (int(counts["dim"][0]),) and genes.dtype.kind == "S" and np.unique(genes).size == genes.size
    assert ct.shape == (int(counts["dim"][1]),) and ct.dtype == np.int8 and ct.min() == 0 and ct.max() == 9
    mt = np.array([q for q, name in enumerate(genes) if name.startswith(b"MT-")], dtype=np.int32)
    assert np.array_equal(mt, counts["mt_rows"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pbmc3k_names.npz")) < 200 * 1024


# ------------------------------------------------------------------------------------------ the host logic, sanitized
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/signature_host_main.cpp compiled with a host compiler and both sanitizers into a program of its own."""
    cxx = next((c for c in ("g++", "clang++", "c++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("signature_host") / "signature_host_main")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "signature_host_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def _run(host_program, tmp_path, what, payload):
    (tmp_path / "in.bin").write_bytes(payload)
    r = subprocess.run([host_program, what, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return (tmp_path / "out.bin").read_bytes()


def test_host_logic_under_address_and_undefined_sanitizers(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("signature_host: ok"), r.stdout


def test_host_gene_table_equals_the_restatement(host_program, tmp_path):
    rng = np.random.default_rng(12)
    m = 300
    sets = [np.arange(m)] + [rng.choice(m, size=int(k), replace=False) for k in rng.integers(1, 40, size=70)] + [np.array([m - 1])]
    sp_ = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    sg = np.concatenate(sets).astype(np.int32)
    out = _run(host_program, tmp_path, "table", np.array([m, len(sets)], dtype=np.int64).tobytes() + sp_.tobytes() + sg.tobytes())
    ptr, flat = sr.gene_table(sets, m)
    assert np.array_equal(np.frombuffer(out[:8 * (m + 1)], dtype=np.int64), ptr)
    assert np.array_equal(np.frombuffer(out[8 * (m + 1):], dtype=np.int32), flat)


def test_host_batches_equal_the_greedy_rule(host_program, tmp_path):
    rng = np.random.default_rng(11)
    for cap in (1, 200, 4000, 0):
        lens = rng.integers(65, 3000, size=200).astype(np.int64)
        out = _run(host_program, tmp_path, "batches", np.array([lens.size, cap], dtype=np.int64).tobytes() + lens.tobytes())
        got = np.frombuffer(out, dtype=np.int64)
        want = sr.batches(lens, cap)
        assert got[0] == len(want) - 1 and got[1:].tolist() == want
        limit = sr.batch_cap(cap)
        for b in range(len(want) - 1):
            tot = int(lens[want[b]:want[b + 1]].sum())
            assert tot <= limit or want[b + 1] - want[b] == 1
            if want[b + 1] < lens.size:                      # greedy: the next cell did not fit
                assert tot + int(lens[want[b + 1]]) > limit


def test_host_paths_equal_the_restatement(host_program, tmp_path):
    rng = np.random.default_rng(13)
    lens = np.concatenate([[0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097], rng.integers(0, 6000, size=100)]).astype(np.int64)
    for knob in (0, 64, 1024, 1025, 2000, 4096, 100000):
        out = _run(host_program, tmp_path, "paths", np.array([lens.size, knob], dtype=np.int64).tobytes() + lens.tobytes())
        cnt = np.frombuffer(out[:24], dtype=np.int64)
        lists = np.frombuffer(out[24:], dtype=np.int32)
        want = sr.split_paths(lens, knob)
        assert cnt.tolist() == [w.size for w in want]
        assert np.array_equal(lists, np.concatenate(want))


def test_host_score_equals_the_numpy_expression(host_program, tmp_path):
    rng = np.random.default_rng(14)
    R = 1500
    ns = rng.integers(1, 201, size=5000).astype(np.uint64)
    lo, hi = ns * (ns + 1), ns * np.uint64(2 * R + 2)
    rank2 = (lo + (rng.random(5000) * (hi - lo).astype(np.float64)).astype(np.uint64)).astype(np.uint64)
    rank2[:3], ns[:3] = [12, 9006, 2], [3, 3, 1]
    out = _run(host_program, tmp_path, "score", np.array([rank2.size, R], dtype=np.int64).tobytes() + rank2.tobytes() + ns.tobytes())
    assert np.array_equal(np.frombuffer(out, dtype=np.float64), sr.score_of(rank2, ns, R))
