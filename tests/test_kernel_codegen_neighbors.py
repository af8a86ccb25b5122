"""The LKNN distance kernels (singlet_amd/csrc/kernels_neighbors.hip) are bit-exact with the reference only if no float
multiply and add were fused: the reference is built for x86-64 without FMA.  Check the gfx950 assembly the build kept
(singlet_amd/csrc/asm/kernels_neighbors.s, Makefile ASM_UNITS) for any fused f32 instruction in those kernels.  Their
roots, quotients and logs go through double on purpose, so no f32 FMA is expected there at all."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "singlet_amd", "csrc", "asm", "kernels_neighbors.s")
FUSED = re.compile(r"^\s*(v_fma_f32|v_fmac_f32\w*|v_mad_f32|v_mac_f32\w*|v_pk_fma_f32|v_fma_mix\w*|v_mad_mix\w*|"
                   r"v_fma_legacy_f32|v_fmac_legacy_f32\w*|v_dot2\w*_f32\w*)\b", re.M)


def _functions(text):
    """{symbol: body} of every function in the assembly"""
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\s*s_endpgm", text, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


def test_lknn_distance_kernels_hold_no_fused_f32_op():
    if not os.path.exists(ASM):
        import __graft_entry__
        __graft_entry__.build()
    funcs = _functions(open(ASM).read())
    dist = {name: body for name, body in funcs.items() if "lknn_fast_kernel" in name or "lknn_slow_keys_kernel" in name}
    assert len(dist) == 12, sorted(funcs)   # six metrics x (LDS path, segmented-sort path)
    for name, body in dist.items():
        assert "v_sqrt_f32" not in body and "v_rcp_f32" not in body, name   # roots and quotients go through double
        bad = FUSED.findall(body)
        assert not bad, (name, bad[:5])
    # the check can see a fused op: the euclidean distance kernels do multiply and add
    assert all(re.search(r"v_(pk_)?mul_f32", b) and re.search(r"v_(pk_)?add_f32", b) for b in dist.values())


@pytest.mark.parametrize("unit", ["kernels_neighbors"])
def test_neighbors_unit_is_built_without_contraction(unit):
    mk = open(os.path.join(ROOT, "singlet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^%s\.o: CXXFLAGS \+= -ffp-contract=off$" % unit, mk, flags=re.M)
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "singlet_amd", "csrc", unit + ".hip")).read()
