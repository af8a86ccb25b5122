"""Static checks of the bounded-tol lane solve (kernels_nnls_asm_bounded.hip) on the device assembly this toolchain emits, as
tests/test_kernel_codegen.py makes them for the exact kernels: the kernel keeps the exact instance's registers and therefore its
waves per SIMD at every rank, hipcc stays below the registers the one asm statement owns, and no instruction reads a
transcendental's result in the slot right behind it."""
import os
import re
import subprocess

import pytest

from test_kernel_codegen import CSRC, HIPCC, ROOT, _vregs

UNITS = {"exact": "kernels_nnls_asm", "bounded": "kernels_nnls_asm_bounded"}


def _asm(unit, tmpdir):
    """the assembly the build kept beside the shipped object, when no source of it is newer; else compiled here"""
    src = os.path.join(CSRC, unit + ".hip")
    kept = os.path.join(CSRC, "asm", unit + ".s")
    deps = [src, os.path.join(CSRC, "nnls_lane_gen.inc"), os.path.join(CSRC, "sgl_internal.h"), os.path.join(CSRC, "nnls_static_for.h"),
            os.path.join(ROOT, "include", "singlet_hip.h")]
    if os.path.exists(kept) and all(os.path.getmtime(kept) >= os.path.getmtime(d) for d in deps):
        return open(kept).read()
    out = os.path.join(str(tmpdir), unit + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                    "--cuda-device-only", "-o", out, src], check=True, capture_output=True, timeout=900)
    return open(out).read()


def _kernel(text, name):
    m = re.search(r"^(_Z\d+%s\w*):[^\n]*\n(.*?)s_endpgm" % name, text, re.S | re.M)
    assert m, name + " not found"
    meta = text[text.index(".amdhsa_kernel " + m.group(1)):]
    return m.group(2), meta[:meta.index(".end_amdhsa_kernel")]


def _waves(meta):
    """waves per SIMD the kernel descriptor allows: 512 registers per lane and SIMD, vector and accumulator together, in blocks of 8"""
    nfree = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    acc = re.search(r"\.amdhsa_accum_offset (\d+)", meta)
    assert acc is None or int(acc.group(1)) >= nfree - 7      # no accumulator registers behind the vector ones
    return max(1, min(8, 512 // ((nfree + 7) // 8 * 8))), nfree


def test_bounded_kernels_keep_the_exact_kernels_registers_and_waves(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    subprocess.run(["make", "-C", CSRC, "nnls_lane_gen.inc"], check=True, capture_output=True, timeout=120)
    inc = open(os.path.join(CSRC, "nnls_lane_gen.inc")).read()
    kps = [int(v) for v in re.findall(r"X_\((\d+)\)", inc.split("SGL_NNLS_ASMB_INSTANCES(X_)")[1].splitlines()[0])]
    assert kps == list(range(2, 51, 2))         # every rank whose x lives in the vector registers
    tmp = tmp_path_factory.mktemp("asm")
    text = {w: _asm(u, tmp) for w, u in UNITS.items()}
    for KP in kps:
        vt = int(re.search(r"#define NNLS_ASM_VT_%d (\d+)" % KP, inc).group(1))
        clob = re.search(r"#define NNLS_ASM_VCLOB_%d (.*)" % KP, inc).group(1)
        top = max(int(v) for v in re.findall(r'"v(\d+)"', clob)) + 1
        plan_waves = int(re.search(r"#define NNLS_ASM_WAVES_%d (\d+)" % KP, inc).group(1))
        _, meta_e = _kernel(text["exact"], "nnls_lane_asm_kernel_%d" % KP)
        body, meta = _kernel(text["bounded"], "nnls_lane_asmb_kernel_%d" % KP)
        (we, _), (wb, nfree) = _waves(meta_e), _waves(meta)
        assert wb == we == plan_waves, (KP, wb, we, plan_waves)
        assert top <= nfree <= (top + 7) // 8 * 8, (KP, nfree, top)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, KP      # no scratch
        in_asm, worst = False, -1
        for line in body.splitlines():
            if "#ASMSTART" in line:
                in_asm = True
                continue
            if "#ASMEND" in line:
                in_asm = False
                continue
            code = line.split(";")[0]
            if in_asm or not code.strip():
                continue
            r = _vregs(code)
            if r:
                worst = max(worst, max(r))
        assert 0 <= worst < vt, "KP=%d: hipcc allocated v%d, the generated sweep owns v[%d:%d]" % (KP, worst, vt, top - 1)
        blocks = [b for b in re.findall(r"#ASMSTART(.*?)#ASMEND", body, re.S) if "v_fmac_f64_dpp" in b]
        assert len(blocks) == 1
        assert blocks[0].count("v_fmac_f64_dpp") == KP * KP
        assert "scratch_" not in blocks[0] and "buffer_" not in blocks[0]
        # every register the statement names is inside the plan or an operand hipcc placed below it
        named = set()
        for line in blocks[0].splitlines():
            named |= _vregs(line.split(";")[0])
        assert max(named) < top and not [r for r in named if vt <= r < top and '"v%d"' % r not in clob]
        # a transcendental's result is at least one instruction away from its first reader (gfx940+ hazard)
        lines = [x.strip() for x in blocks[0].splitlines() if x.strip()]
        nrcp = 0
        for a, b in zip(lines, lines[1:]):
            mm = re.match(r"v_rcp_f64 (v\[\d+:\d+\])", a)
            if mm:
                nrcp += 1
                assert mm.group(1) not in b.split(",", 1)[-1] or b.startswith("s_nop"), (KP, a, b)
        assert nrcp == KP + 2      # one per coordinate, and 1 / k of the stop test before and inside the sweep loop
