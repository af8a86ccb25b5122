"""The spatial_graph kernels (sg_merge_kernel<FILL> in singlet_amd/csrc/kernels_neighbors.hip) in the gfx950 assembly the
build kept (singlet_amd/csrc/asm/kernels_neighbors.s): no scratch, the LDS and occupancy they were written for, the
correctly rounded double root and quotient expansions (no fast-math / afn forms), and the distance's multiplies and adds
left unfused (the unit is built with -ffp-contract=off; the GPU tests hold pairs a fused form would change)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "singlet_amd", "csrc", "asm", "kernels_neighbors.s")
LDS = 9 * 64 * (4 + 8 + 2) + 9 * 4   # accepted indices, weights, rank order, per-list counts


def _kernels():
    if not os.path.exists(ASM):
        import __graft_entry__
        __graft_entry__.build()
    text = open(ASM).read()
    out = {}
    for m in re.finditer(r"^(_Z\S*sg_merge_kernel\S*):[^\n]*\n(.*?)^\s*s_endpgm(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.M | re.S):
        out[m.group(1)] = (m.group(2), m.group(3))
    return out


def test_both_passes_are_built():
    import singlet_amd as sa
    assert callable(sa.spatial_graph)
    names = sorted(_kernels())
    assert len(names) == 2 and any("ILb0E" in n for n in names) and any("ILb1E" in n for n in names), names


@pytest.mark.parametrize("fill", [0, 1])
def test_resources(fill):
    body, meta = next(v for k, v in _kernels().items() if "ILb%dE" % fill in k)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta)
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1))
    assert LDS <= lds <= LDS + 16, lds   # (+ alignment of the arrays)
    vgpr = int(re.search(r"\.amdhsa_accum_offset (\d+)", meta).group(1))
    assert vgpr <= 64, vgpr   # 64-lane workgroups of 8 KB LDS: 5 per SIMD, bound by the LDS, not the registers
    assert "scratch_" not in body and "buffer_store" not in body


@pytest.mark.parametrize("fill", [0, 1])
def test_correctly_rounded_root_and_quotient(fill):
    body, _ = next(v for k, v in _kernels().items() if "ILb%dE" % fill in k)
    # the IEEE root of llvm.sqrt.f64: rsq seed, refinement, scaling of tiny / huge inputs, class test of 0 / inf
    n_rsq = len(re.findall(r"^\s*v_rsq_f64", body, flags=re.M))
    assert n_rsq == 9, n_rsq   # the nine lists of the 3 x 3 buckets, unrolled
    assert len(re.findall(r"^\s*v_ldexp_f64", body, flags=re.M)) >= 2 * n_rsq
    assert len(re.findall(r"^\s*v_cmp_class_f64", body, flags=re.M)) >= n_rsq
    assert not re.search(r"^\s*v_sqrt_f64", body, flags=re.M)   # the bare (approximate) root is the fast-math form
    # the distance's squares and sum, unfused
    assert len(re.findall(r"^\s*v_mul_f64", body, flags=re.M)) >= 2 * n_rsq
    assert len(re.findall(r"^\s*v_add_f64", body, flags=re.M)) >= n_rsq
    if fill:   # the column division: the full div_scale / div_fmas / div_fixup expansion
        for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64"):
            assert re.search(r"^\s*%s" % op, body, flags=re.M), op
