"""Static checks of the tiled accumulate's staging prefetch (no GPU needed: hipcc cross-compiles).

acc_tiled_kernel<2> (pair layout, KS == k == ldf) loads the factor rows of row block b + 2 into v[24:63] before the chunk of
stage b (tiled_issue) and writes them into the LDS ring slot after it (tiled_commit).  The loads are only worth issuing early
if nothing waits for them before the chunk, and the registers are only safe if hipcc never touches them: it is capped at
v0..v23 in that instance and does not know the loads are in flight."""
import re

import pytest

from test_kernel_codegen import tiled_asm, _vregs  # noqa: F401  (module fixture: the kept device assembly)

PIECES = 10
PIECE_REGS = set(range(24, 64))


def _blocks(body):
    """(start, end, text) of every inline-asm block, in text order"""
    return [(m.start(), m.end(), m.group(1)) for m in re.finditer(r"#ASMSTART(.*?)#ASMEND", body, re.S)]


def _is_issue(text):
    return len(re.findall(r"global_load_dwordx4 v\[(\d+):\d+\]", text)) == PIECES


def test_compiler_never_touches_the_piece_registers(tiled_asm):
    body, _ = tiled_asm[2]
    in_asm = False
    for line in body.splitlines():
        if "#ASMSTART" in line:
            in_asm = True
            continue
        if "#ASMEND" in line:
            in_asm = False
            continue
        code = line.split(";")[0]
        if not in_asm and code.strip():
            assert not (_vregs(code) & PIECE_REGS), "hipcc uses a piece register of tiled_issue: %s" % code.strip()


def test_next_block_is_loaded_before_the_chunk_and_stays_in_flight(tiled_asm):
    body, _ = tiled_asm[2]
    blocks = _blocks(body)
    chunk = [b for b in blocks if "v_fmac_f64_dpp" in b[2]]
    assert len(chunk) == 1
    issues = [b for b in blocks if _is_issue(b[2])]
    assert len(issues) >= 1
    for _, _, text in issues:
        dst = [int(r) for r in re.findall(r"global_load_dwordx4 v\[(\d+):\d+\]", text)]
        assert sorted(dst) == list(range(24, 64, 4)), dst
        assert "s_waitcnt" not in text
    # the issue of block b + 2: the last one in front of the chunk; nothing between them waits for it
    before = [b for b in issues if b[1] <= chunk[0][0]]
    assert before, "no F load of the next block is issued before the chunk"
    between = body[before[-1][1]:chunk[0][0]]
    for n in re.findall(r"s_waitcnt[^\n;]*vmcnt\((\d+)\)", between):
        assert int(n) >= PIECES, "s_waitcnt vmcnt(%s) between the prefetch and the chunk" % n
    assert "scratch_" not in between and "buffer_" not in between


def test_commit_waits_for_the_pieces_only(tiled_asm):
    """Two commits: vmcnt(0) (range start, short chunks) and vmcnt(16) (a whole ring lap of the chunk's refills stays in flight);
    ten masked 16-byte LDS writes of the piece registers, exec restored, the writes landed before the barrier."""
    body, _ = tiled_asm[2]
    commits = [b[2] for b in _blocks(body) if "ds_write_b128" in b[2]]
    waits = set()
    for text in commits:
        lines = [x.strip() for x in text.splitlines() if x.strip() and not x.strip().startswith(";")]
        m = re.match(r"s_waitcnt vmcnt\((\d+)\)$", lines[0])
        assert m, lines[0]
        waits.add(int(m.group(1)))
        writes = re.findall(r"ds_write_b128 v\d+, v\[(\d+):\d+\]", text)
        assert [int(r) for r in writes] == list(range(24, 64, 4)), writes
        assert text.count("s_and_b64 exec, exec, vcc") == PIECES
        assert lines[-2].startswith("s_mov_b64 exec, s[") and lines[-1] == "s_waitcnt lgkmcnt(0)", lines[-2:]
    assert waits == {0, 16}, waits
