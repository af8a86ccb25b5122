"""The R shim's neighbour-graph entries (singlet_amd/r/singlet_hip_graph_shim.c) on the CPU: without R here, syntax-check
their calls into include/singlet_hip.h against prototype-only R API declarations (tests/r_api_stub/ plus the additions in
tests/r_api_stub_graph/), and check that the main shim registers them and backend.R rebinds them with the reference's
names and arities (src/RcppExports.cpp:466-467)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_shim_compiles_against_the_abi():
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "r_api_stub"),
                        "-include", os.path.join(ROOT, "tests", "r_api_stub_graph", "R_graph_api.h"),
                        os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_graph_shim.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_graph_entries_are_registered_and_rebound():
    shim = open(os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_shim.c")).read()
    graph = open(os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_graph_shim.c")).read()
    backend = open(os.path.join(ROOT, "singlet_amd", "r", "backend.R")).read()
    for sym, arity in (("_singlet_c_LKNN", 10), ("_singlet_c_SNN", 3)):
        assert re.search(r'\{"%s",\s*\(DL_FUNC\)&%s,\s*%d\}' % (sym, sym, arity), shim), sym
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % sym, graph, flags=re.M)
        assert m and len(m.group(1).split(",")) == arity, sym
        assert 'rebind("%s"' % sym[len("_singlet_"):] in backend, sym
