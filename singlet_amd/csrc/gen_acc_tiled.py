#!/usr/bin/env python3
"""Generates acc_tiled_gen.inc: the hand-scheduled chunk loop of the LDS-tiled accumulate (kernels_tiled.hip).

Same entry stream, same arithmetic and the same order of operations as a compiler-scheduled loop (results are
bit-identical); what the hand schedule adds:

  * an entry TUPLE is one v_add_u32_dpp (LDS address), one ds_read_b128 (two factors per lane) and two v_fmac_f64_dpp;
    it serves two non-zeros in the pair layout (ranks 33 - 64: lanes 0-31 one column, 32-63 its partner) and four in
    the quad layout (parts up to 32 factors: each 16-lane DPP row its own column of a column quad);
  * the LDS reads run ONE OCTET (8 tuples) ahead without ever draining: the read of tuple j of the next octet is
    issued right after the two FMAs of tuple j of this one, into the register quad those FMAs just consumed (one
    buffer of 8 quads; counted lgkmcnt: LDS returns in order);
  * the accumulators of the 32 column units (pairs / quads) stay IN PLACE in v[128:255]: VGPR index mode is on for
    the whole loop and M0 (destination-relative, 0x8000 | 4 * unit) selects the running unit's registers;
  * the column-unit bookkeeping is a SCHEDULE TABLE: the stream builder writes one u16 per group of four tuples --
    the M0 word of the unit the group belongs to -- and a group head is ONE instruction,
        s_bfe_u32 m0, s[TAB0 + g / 2], <16 bits at 16 (g & 1)>
    with g = 4 d + 2 o + group static in the unrolled lap of 8 ring slots x 2 octets x 2 groups = 32 groups = 64
    bytes of table = one s_load_dwordx16.  The next lap's words are loaded a lap ahead into TAB1 and moved down at
    the wrap of the ring (s_waitcnt lgkmcnt(0) there: SMEM returns out of order, so only a full drain proves it has
    landed; LDS waits in between stay correct with the scalar load outstanding -- the counter then only over-counts).
    A chunk entered at ring slot `phase` loads the lap that contains its first group (table address of the chunk
    - 8 * phase bytes) and the one behind it;
  * the stream arrives through a ring of 8 slots in flight (counted vmcnt: loads return in order).  A slot is
    64 lanes x one entry: a whole 64-slot set in the quad layout (row h of the wave = column slot h of the quad,
    exactly the operand layout row_newbcast wants); HALF a set in the pair layout, loaded with the lane rows doubled
    (lanes 0-15 and 16-31 both read the A half's entries 16 s .. 16 s + 15, lanes 32-47 and 48-63 the B half's) --
    the [A A B B] layout the row broadcasts want.  The address adds and the FMAs read the ring registers themselves,
    written by vector loads only: no VALU-write -> DPP-read hazard can exist.  %[voff4] / %[voff8] carry the lane
    mapping.  A slot is consumed in two octets and refilled once its last operand has been read.

Stream (kernels_tiled.hip): sets of 64 entry slots; row offsets u32, values f64; gtab = the schedule words, one per group.

Register plan (asm-owned; the compiler is capped at v0..v63 by amdgpu_waves_per_eu(8, 8)):
    v64..71 row-offset ring, v72..87 value ring (8 slots)   v88..95 LDS addresses   v96..127 8 factor quads
    v128..255 accumulators (unit p: v[128 + 4p : 131 + 4p])
    s[52:67] the running lap's 32 schedule words, s[68:83] the next lap's, s[84:85] / s[86:87] next slot to load
    (row offsets / values), s88 fetching slots left, s91 scratch (the index-mode operand), s[92:93] next table block
"""
import os
import sys

NS = 8                                  # ring slots
ER = [64 + i for i in range(NS)]        # row offsets of slot i
EX = [72 + 2 * i for i in range(NS)]    # values of slot i
AD = [88 + j for j in range(8)]         # LDS addresses of the octet's 8 tuples
W = [96 + 4 * j for j in range(8)]      # their factor quads
ACC = 128
S_RP, S_XP, S_NS, S_ACC = 84, 86, 88, 91
S_TP = 92            # s[92:93]: next 64-byte block of the schedule table to load (even-aligned pair)
TAB0, TAB1 = 52, 68  # s[52:67] the running lap's 32 schedule words (u16), s[68:83] the next lap's
S_END = 100          # both clobber lists run up to s99 (the ring fills write s[84:87] only; the lists are kept as they are, since
                     # narrowing them may move the compiler's scalar allocation around the asm)


def r2(b):
    return f"v[{b}:{b + 1}]"


class Gen:
    """pair = True: two columns per LDS instruction (half-set ring slots, doubled lane rows); pair = False: four."""

    def __init__(self, pair, pf=0):
        self.L = []
        self.lab = 0
        self.pair = pair
        self.pf = pf   # > 0: at every wrap of the ring, touch the stream `pf` laps beyond the lap being loaded (below)

    def A(self, s):
        self.L.append(s)

    def label(self, stem):
        self.lab += 1
        return f".Ltiled_{stem}_{self.lab}_%="

    def text(self):
        return " \\\n".join(f'    "{ins}\\n\\t"' for ins in self.L)

    def refill(self, i):
        """ring slot i <- the slot NS ahead of the one it held.  s[S_RP] / s[S_XP] point at what goes into slot 0 of the
        current lap; slots are refilled in the order 0 .. NS - 1, so the pointers advance once per lap (after the last
        slot) and the slot is an immediate offset"""
        if self.pair:   # half a set: entries 16 (i & 1) .. 16 (i & 1) + 15 of each half of set i >> 1
            st, sub = i >> 1, i & 1
            ro, xo, lap_r = 256 * st + 64 * sub, 512 * st + 128 * sub, 128 * NS
        else:
            ro, xo, lap_r = 256 * i, 512 * i, 256 * NS
        A = self.A
        A(f"global_load_dword v{ER[i]}, %[voff4], s[{S_RP}:{S_RP + 1}] offset:{ro}")
        A(f"global_load_dwordx2 {r2(EX[i])}, %[voff8], s[{S_XP}:{S_XP + 1}] offset:{xo}")
        if i == NS - 1:
            A(f"s_add_u32 s{S_RP}, s{S_RP}, {lap_r}")
            A(f"s_addc_u32 s{S_RP + 1}, s{S_RP + 1}, 0")
            A(f"s_add_u32 s{S_XP}, s{S_XP}, {2 * lap_r}")
            A(f"s_addc_u32 s{S_XP + 1}, s{S_XP + 1}, 0")

    def addrs(self, slot, o):
        """LDS addresses of the 8 entry tuples of octet o (0, 1) of the slot"""
        for j in range(8):
            self.A(f"v_add_u32_dpp v{AD[j]}, v{ER[slot]}, %[lane16] row_newbcast:{8 * o + j} row_mask:0xf bank_mask:0xf")

    def octet(self, d, o, reads):
        """the 16 FMAs of octet o of slot d; reads: issue the next octet's read of tuple j behind tuple j"""
        A = self.A
        x = EX[d]
        for g in range(2):
            gi = 4 * d + 2 * o + g
            A(f"s_bfe_u32 m0, s{TAB0 + gi // 2}, {hex((16 * (gi & 1)) | (16 << 16))}")
            # ONE wait per group: before tuple 4 g the wave has 8 reads in flight (8 - 4 g of this octet, 4 g of the next),
            # and the group needs the 4 oldest -- without reads ahead (a chunk's last octet) the ones left after them
            A(f"s_waitcnt lgkmcnt({4 if reads else 4 - 4 * g})")
            for j in range(4 * g, 4 * g + 4):
                bc = f"row_newbcast:{8 * o + j} row_mask:0xf bank_mask:0xf"
                A(f"v_fmac_f64_dpp {r2(ACC)}, {r2(x)}, {r2(W[j])} {bc}")
                A(f"v_fmac_f64_dpp {r2(ACC + 2)}, {r2(x)}, {r2(W[j] + 2)} {bc}")
                if reads:
                    A(f"ds_read_b128 v[{W[j]}:{W[j] + 3}], v{AD[j]}")

    def wrap(self):
        """wrap of the ring = end of a lap of 32 groups: the next lap's schedule words move down, the one behind is fetched"""
        A = self.A
        A("s_waitcnt lgkmcnt(0)")
        for w in range(8):
            A(f"s_mov_b64 s[{TAB0 + 2 * w}:{TAB0 + 2 * w + 1}], s[{TAB1 + 2 * w}:{TAB1 + 2 * w + 1}]")
        A(f"s_load_dwordx16 s[{TAB1}:{TAB1 + 15}], s[{S_TP}:{S_TP + 1}], 0x0")
        A(f"s_add_u32 s{S_TP}, s{S_TP}, 64")
        A(f"s_addc_u32 s{S_TP + 1}, s{S_TP + 1}, 0")
        if self.pf:
            # Stream prefetch into L2.  The ring keeps one lap (8 slots) of the stream in flight per wave: a slot's data must
            # make the whole trip from HBM inside one lap of the loop (~3 us), and every load that takes longer stalls the
            # wave at its counted vmcnt.  Once per lap two more loads touch every 128-byte line of the lap `pf` laps beyond the
            # one being loaded (lane stride = lap bytes / 64; %[pfl] = lane * stride + pf * lap bytes of the row-offset stream,
            # the value stream is twice that): the ring's own loads of that lap then hit L2.  Destination v63 is a dummy:
            # nothing reads it, and both loads are older than ring slot 0's refill, so the vmcnt wait of body(NS - 1) -- a lap
            # later -- has seen them land before v63 is written again.
            A("s_mov_b32 m0, 0")   # index mode is on and M0 still points the last group's destinations at its accumulators
            A("v_lshlrev_b32 v63, 1, %[pfl]")
            A(f"global_load_dword v63, v63, s[{S_XP}:{S_XP + 1}]")
            A(f"global_load_dword v63, %[pfl], s[{S_RP}:{S_RP + 1}]")

    def body(self, d, L_body, L_last):
        """a slot that is NOT the chunk's last one: both octets fetch ahead; s[S_NS] counts the fetching slots still to come
        and its borrow sends the flow to the last slot's own code (no test inside the body)"""
        A = self.A
        dn = (d + 1) % NS
        A(f"{L_body[d]}:")
        A("s_mov_b32 m0, 0")
        self.addrs(d, 1)
        self.octet(d, 0, True)
        A("s_mov_b32 m0, 0")
        # slot d + 1 has landed: of the 2 (NS - 1) ring loads in flight its two are the oldest; with the two prefetch loads of
        # the last wrap in flight as well (issued between the refills of slot NS - 1 and slot 0) two more may stay
        # outstanding, except at d = NS - 1, where they are older than the slot waited for
        A(f"s_waitcnt vmcnt({2 * (NS - 2) + (2 if (self.pf and d != NS - 1) else 0)})")
        self.addrs(dn, 0)
        self.octet(d, 1, True)
        self.refill(d)
        if d == NS - 1:
            self.wrap()
        A(f"s_sub_u32 s{S_NS}, s{S_NS}, 1")
        A(f"s_cbranch_scc1 {L_last[dn]}")
        if d == NS - 1:
            A(f"s_branch {L_body[0]}")

    def last(self, d, L_last, L_end):
        """the chunk's last slot at ring slot d: nothing of the next chunk is fetched (another tile will be in LDS)"""
        A = self.A
        A(f"{L_last[d]}:")
        A("s_mov_b32 m0, 0")
        self.addrs(d, 1)
        self.octet(d, 0, True)
        self.octet(d, 1, False)
        self.refill(d)
        A(f"s_mov_b32 %[phase], {(d + 1) % NS}")
        A(f"s_branch {L_end}")

    def chunk(self):
        """%[ns] slots starting at ring slot %[phase], schedule words from %[tp]"""
        A = self.A
        L_body = [self.label(f"b{d}") for d in range(NS)]
        L_pro = [self.label(f"p{d}") for d in range(NS)]
        L_last = [self.label(f"last{d}") for d in range(NS)]
        L_end = self.label("end")
        A(f"s_mov_b64 s[{S_RP}:{S_RP + 1}], %[rp]")
        A(f"s_mov_b64 s[{S_XP}:{S_XP + 1}], %[xp]")
        A(f"s_sub_u32 s{S_NS}, %[ns], 2")    # fetching slots behind the first: ns - 2 more borrows later (ns = 1: straight to `last`)
        # schedule words: the lap holding the chunk's first group starts 4 * phase groups = 8 * phase bytes before it
        A(f"s_lshl_b32 s{S_ACC}, %[phase], 3")
        A(f"s_mov_b64 s[{S_TP}:{S_TP + 1}], %[tp]")
        A(f"s_sub_u32 s{S_TP}, s{S_TP}, s{S_ACC}")
        A(f"s_subb_u32 s{S_TP + 1}, s{S_TP + 1}, 0")
        A(f"s_load_dwordx16 s[{TAB0}:{TAB0 + 15}], s[{S_TP}:{S_TP + 1}], 0x0")
        A(f"s_load_dwordx16 s[{TAB1}:{TAB1 + 15}], s[{S_TP}:{S_TP + 1}], 0x40")
        A(f"s_add_u32 s{S_TP}, s{S_TP}, 128")
        A(f"s_addc_u32 s{S_TP + 1}, s{S_TP + 1}, 0")
        A(f"s_mov_b32 s{S_ACC}, 0")
        A(f"s_set_gpr_idx_on s{S_ACC}, 0")   # index mode on, no operand indexed while M0[15:12] = 0
        A("s_mov_b32 m0, 0")
        for d in range(1, NS):
            A(f"s_cmp_eq_u32 %[phase], {d}")
            A(f"s_cbranch_scc1 {L_pro[d]}")
        for d in range(NS):
            A(f"{L_pro[d]}:")
            A(f"s_waitcnt vmcnt({2 * (NS - 1)})")   # all NS slots in flight, slot d the oldest
            self.addrs(d, 0)
            for j in range(8):
                A(f"ds_read_b128 v[{W[j]}:{W[j] + 3}], v{AD[j]}")
            A("s_waitcnt lgkmcnt(0)")        # the schedule words (and the first reads) have landed
            A(f"s_cmp_eq_u32 %[ns], 1")
            A(f"s_cbranch_scc1 {L_last[d]}")
            A(f"s_branch {L_body[d]}")
        for d in range(NS):
            self.body(d, L_body, L_last)
        for d in range(NS):
            self.last(d, L_last, L_end)
        A(f"{L_end}:")
        A("s_waitcnt lgkmcnt(0)")            # a schedule load may still be in flight: its registers are not ours past this block
        A("s_mov_b32 m0, 0")
        A("s_set_gpr_idx_off")
        A(f"s_mov_b64 %[rp], s[{S_RP}:{S_RP + 1}]")
        A(f"s_mov_b64 %[xp], s[{S_XP}:{S_XP + 1}]")

    def ring_fill(self):
        """the ring's first lap, before a wave's first chunk"""
        A = self.A
        A(f"s_mov_b64 s[{S_RP}:{S_RP + 1}], %[rp]")
        A(f"s_mov_b64 s[{S_XP}:{S_XP + 1}], %[xp]")
        for i in range(NS):
            self.refill(i)
        A(f"s_mov_b64 %[rp], s[{S_RP}:{S_RP + 1}]")
        A(f"s_mov_b64 %[xp], s[{S_XP}:{S_XP + 1}]")


def main():
    # laps of L2 prefetch ahead of the ring.  Default 0: measured at config 3 (one box, two runs each, rhs_h / rhs_w ms per
    # pass) 0 laps 10.25 / 10.21 and 10.28 / 10.24, 2 laps 10.47 / 10.47 and 10.56 / 10.48, 4 laps 10.65 / 10.66 and 10.73 / 10.65;
    # config 2 0.220 -> 0.262: the waves are not waiting for the stream, and the two extra loads per lap cost what loads cost.
    pf = int(os.environ.get("SGL_GEN_PF", "0"))
    out = ["// generated by gen_acc_tiled.py -- do not edit", "#pragma once"]
    g = Gen(pair=False)
    for c in range(128):
        g.A(f"v_mov_b32 v{ACC + c}, 0")
    out.append(f"#define ACC_TILED_ZERO_ASM \\\n{g.text()}")
    out.append("#define ACC_TILED_CLOBBERS " + ", ".join([f'"s{r}"' for r in range(83, S_END)] + ['"memory"', '"scc"']))
    for tag, pair in (("2", True), ("4", False)):
        g = Gen(pair)
        g.ring_fill()
        out.append("")
        out.append(f"#define ACC_TILED{tag}_RING_FILL_ASM \\\n{g.text()}")
        g = Gen(pair, pf)
        g.chunk()
        out.append("")
        out.append(f"#define ACC_TILED{tag}_CHUNK_ASM \\\n{g.text()}")
    tclob = [f'"s{r}"' for r in range(TAB0, S_END)] + ['"memory"', '"scc"'] + (['"v63"'] if pf else [])
    out.append("#define ACC_TILED_CHUNK_CLOBBERS " + ", ".join(tclob))
    out.append(f"#define ACC_TILED_PF_LAPS {pf}")
    sys.stdout.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
