"""The R shim's spatial_graph entry (singlet_amd/r/singlet_hip_graph_shim.c) on the CPU: without R here, syntax-check it
against prototype-only R API declarations (tests/r_api_stub/ plus tests/r_api_stub_graph/), and check that the main shim
registers _singlet_spatial_graph with the reference's arity (src/RcppExports.cpp:465, 5 args) and backend.R rebinds it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spatial_graph_shim_compiles_against_the_abi():
    graph = open(os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_graph_shim.c")).read()
    assert "sgl_spatial_graph(" in graph
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "r_api_stub"),
                        "-include", os.path.join(ROOT, "tests", "r_api_stub_graph", "R_graph_api.h"),
                        os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_graph_shim.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_spatial_graph_is_registered_and_rebound():
    shim = open(os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_shim.c")).read()
    graph = open(os.path.join(ROOT, "singlet_amd", "r", "singlet_hip_graph_shim.c")).read()
    backend = open(os.path.join(ROOT, "singlet_amd", "r", "backend.R")).read()
    sym = "_singlet_spatial_graph"
    assert re.search(r'\{"%s",\s*\(DL_FUNC\)&%s,\s*5\}' % (sym, sym), shim)
    m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % sym, graph, flags=re.M)
    assert m and len(m.group(1).split(",")) == 5
    m = re.search(r'rebind\("spatial_graph", function\(([^)]*)\)\s*\n\s*\.Call\(dll\[\["%s"\]\],([^)]*)\)' % sym, backend)
    assert m and len(m.group(1).split(",")) == 5 and len(m.group(2).split(",")) == 5
    # the reference wrapper's defaults, so that spatial_graph(c1, c2, max_dist) works as before
    assert "formals(sg)$max_k <- 100L" in backend and "formals(sg)$threads <- 0L" in backend
