// ---- the mask as lists (included by kernels_mask.hip) ---------------------------------------------------------------
// mask_gram_mfma_kernel hashes nrow x ncol (row, column) pairs per pass, ~110 VALU instructions per 64 rows, to find
// the 1 / inv_density of them that are drawn -- and on this part an FP64 MFMA and the VALU work of the same SIMD do
// not overlap (measured: kernel time = MFMA time + the time of everything else, interleaved or not, at one wave
// per SIMD or four; profiles/r3_mask_gram_ablation.md), so the hash is paid in full: 20 % of the pass at k = 100, well
// over half below k = 50.  The mask is a function of (seed, inv_density, cell, gene) alone: it is listed ONCE per
// fit (two hashing passes: count, scan, fill; 4 B per drawn pair) and every later pass reads the lists.
__device__ __forceinline__ uint64_t mg_mix_j(uint64_t j) {   // the j-only part of sgl_rand2
    j ^= j >> 7;
    j ^= j << 23;
    j ^= j >> 8;
    return j;
}
__device__ __forceinline__ uint64_t mg_finish(uint64_t xi, uint64_t jm) {   // sgl_rand2 from its two halves
    uint64_t x = xi + jm;
    x ^= x >> 7;
    x ^= x << 53;
    x ^= x >> 4;
    return x;
}
// one wave per column; FILL = false: cnt[col] = number of drawn rows; FILL = true: idx[ptr[col] ...] = the rows, ascending
template <bool FILL>
__global__ __launch_bounds__(256) void mask_list_kernel(int64_t ncol, int32_t nrow, uint64_t seed, SglDiv dv, int mask_t,
                                                        int64_t col_off, int64_t row_off, int64_t* __restrict__ cnt,
                                                        const int64_t* __restrict__ ptr, int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= ncol) return;
    const uint64_t gcol = (uint64_t)(col + col_off);
    // draw(cell, gene) = rand2(seed, cell, gene): the column is the cell (mask_t = 0) or the gene (mask_t = 1)
    const uint64_t col_i = sgl_rand_i(seed, gcol), col_j = mg_mix_j(gcol);
    int64_t base = FILL ? ptr[col] : 0;
    int total = 0;
    for (int64_t r0 = 0; r0 < nrow; r0 += 64) {
        const int64_t r = r0 + lane;
        const uint64_t grow = (uint64_t)(r + row_off);
        const uint64_t x = mask_t ? mg_finish(sgl_rand_i(seed, grow), col_j) : mg_finish(col_i, mg_mix_j(grow));
        const bool drawn = r < nrow && sgl_divides(x, dv);
        const unsigned long long m = __ballot(drawn);
        if (FILL) {
            if (drawn) idx[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)r;
            base += __popcll(m);
        } else {
            total += __popcll(m);
        }
    }
    if (!FILL && lane == 0) cnt[col] = total;
}

void sgl_mask_list_free(DevMaskList& L) {
    if (L.ptr) (void)sgl_pool_free(L.ptr);
    if (L.idx) (void)sgl_pool_free(L.idx);
    if (L.val) (void)sgl_pool_free(L.val);
    L = DevMaskList();
}

// Lists for (ncol columns x nrow rows) under the given key; a no-op when they are there already.  Returns SGL_OK
// with L.mask_t < 0 (nothing built) when the lists would not fit the memory budget -- the caller then hashes.
int sgl_mask_list_build(sgl_ctx* c, DevMaskList& L, int64_t ncol, int32_t nrow, uint64_t seed, uint64_t inv_density, int mask_t,
                        int64_t col_offset, int64_t row_offset) {
    if (L.ncol == ncol && L.nrow == nrow && L.seed == seed && L.inv == inv_density && L.col_off == col_offset &&
        L.row_off == row_offset && (L.mask_t == mask_t || (L.refused && L.mask_t == -2 - mask_t)))
        return SGL_OK;
    hipStream_t s = c->stream;
    L.mask_t = -1;
    L.refused = false;
    L.val_ok = L.val_refused = false;
    L.ncol = ncol; L.nrow = nrow; L.seed = seed; L.inv = inv_density; L.col_off = col_offset; L.row_off = row_offset;
    auto refuse = [&]() { L.refused = true; L.mask_t = -2 - mask_t; return SGL_OK; };
    if (ncol <= 0 || nrow <= 0 || inv_density == 0) return refuse();
    // budget: the expected size must fit a quarter of what is free now (dense masks -- inv_density 1 or 2 on a large
    // matrix -- would need tens of GB: they keep the hashing kernel)
    size_t free_b = 0, total_b = 0;
    HIPCHK(sgl_pool_mem_info(&free_b, &total_b));
    const double expect = (double)ncol * (double)nrow / (double)inv_density * 4.0 * 1.05 + 8.0 * (double)(ncol + 1);
    if (expect > 0.25 * ((double)free_b + 4.0 * (double)L.cap_idx)) return refuse();
    if (L.cap_ptr < (size_t)ncol + 2) {
        if (L.ptr) (void)sgl_pool_free(L.ptr);
        L.ptr = nullptr; L.cap_ptr = 0;
        if (sgl_pool_malloc(&L.ptr, sizeof(int64_t) * ((size_t)ncol + 2)) != hipSuccess) { (void)hipGetLastError(); return refuse(); }
        L.cap_ptr = (size_t)ncol + 2;
    }
    int64_t* cnt = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    auto cleanup = [&]() { if (cnt) (void)sgl_pool_free(cnt); if (tmp) (void)sgl_pool_free(tmp); cnt = nullptr; tmp = nullptr; };
    if (sgl_pool_malloc(&cnt, sizeof(int64_t) * ((size_t)ncol + 1)) != hipSuccess) { (void)hipGetLastError(); return refuse(); }
    const SglDiv dv = sgl_div_make(inv_density);
    const dim3 g((unsigned)((ncol + 3) / 4)), b(256);
    int rc = SGL_OK;
    int64_t total = 0;
    do {
        if (hipMemsetAsync(cnt + ncol, 0, sizeof(int64_t), s) != hipSuccess) { rc = SGL_EHIP; break; }
        mask_list_kernel<false><<<g, b, 0, s>>>(ncol, nrow, seed, dv, mask_t, col_offset, row_offset, cnt, nullptr, nullptr);
        if (hipGetLastError() != hipSuccess) { rc = SGL_EHIP; break; }
        if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, L.ptr, (int)(ncol + 1), s) != hipSuccess) { rc = SGL_EHIP; break; }
        if (sgl_pool_malloc(&tmp, tmp_bytes ? tmp_bytes : 16) != hipSuccess) { (void)hipGetLastError(); cleanup(); return refuse(); }
        if (hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, L.ptr, (int)(ncol + 1), s) != hipSuccess) { rc = SGL_EHIP; break; }
        if (hipMemcpyAsync(&total, L.ptr + ncol, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) { rc = SGL_EHIP; break; }
        if (hipStreamSynchronize(s) != hipSuccess) { rc = SGL_EHIP; break; }
    } while (0);
    cleanup();
    if (rc != SGL_OK) { sgl_set_error("mask lists: HIP error while counting"); return rc; }
    if (L.cap_idx < (size_t)total + 64) {
        if (L.idx) (void)sgl_pool_free(L.idx);
        L.idx = nullptr; L.cap_idx = 0;
        const size_t want = (size_t)((double)total * 1.02) + 1024;   // the next mask of this shape is a little longer or shorter
        if (sgl_pool_malloc(&L.idx, sizeof(int32_t) * want) != hipSuccess) { (void)hipGetLastError(); return refuse(); }
        L.cap_idx = want;
    }
    mask_list_kernel<true><<<g, b, 0, s>>>(ncol, nrow, seed, dv, mask_t, col_offset, row_offset, nullptr, L.ptr, L.idx);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(L.ptr + ncol + 1, 0, sizeof(int64_t), s));   // eight zero bytes: the 0.0 the downdate kernel loads for operands past the rank
    L.total = total;
    L.mask_t = mask_t;
    return SGL_OK;
}

static bool ml_has_key(const DevMaskList& L, int64_t ncol, int32_t nrow, uint64_t seed, uint64_t inv_density, int mask_t,
                       int64_t col_offset, int64_t row_offset) {
    return L.ncol == ncol && L.nrow == nrow && L.seed == seed && L.inv == inv_density && L.col_off == col_offset &&
           L.row_off == row_offset && (L.mask_t == mask_t || (L.refused && L.mask_t == -2 - mask_t));
}

void sgl_mask_lists_free_all(sgl_ctx* c) {
    for (int o = 0; o < 2; ++o) {
        sgl_mask_list_free(c->ML[o]);
        for (int q = 0; q < SGL_ML_KEEP; ++q) sgl_mask_list_free(c->MLkeep[o][q]);
    }
}

// How many earlier masks stay resident per orientation: SGL_MASK_KEEP (0 .. SGL_ML_KEEP, default 2: with the current one
// the three replicate seeds of R's defaults).  A kept mask costs 4 B per drawn pair for its list and, on the cell side, 8 B
// per pair for the listed matrix values (6 + 12 GB at config 5); nothing is kept once the kept masks AND the current one
// together -- both arrays counted (round-4 advice: the values were not) -- would exceed 3 / 10 of the device memory.  Kept
// masks are also the first thing given back when an allocation of the fit fails (sgl_mask_lists_release_kept).
static int ml_keep_slots(const DevMaskList& cur) {
    static const int want = [] {
        const char* e = getenv("SGL_MASK_KEEP");
        const int v = e ? atoi(e) : 2;
        return v < 0 ? 0 : (v > SGL_ML_KEEP ? SGL_ML_KEEP : v);
    }();
    if (want == 0) return 0;
    size_t free_b = 0, total_b = 0;
    if (sgl_pool_mem_info(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const double per_mask = 4.0 * (double)cur.cap_idx + 8.0 * (double)std::max(cur.cap_val, cur.val_refused ? (size_t)0 : cur.cap_idx);
    return (per_mask * (double)(want + 1) > 0.3 * (double)total_b) ? 0 : want;
}

// Memory pressure: free the kept (not the current) masks of both orientations; returns true if anything was freed.
bool sgl_mask_lists_release_kept(sgl_ctx* c) {
    bool any = false;
    for (int o = 0; o < 2; ++o)
        for (int q = 0; q < SGL_ML_KEEP; ++q) {
            any = any || c->MLkeep[o][q].idx != nullptr || c->MLkeep[o][q].val != nullptr || c->MLkeep[o][q].ptr != nullptr;
            sgl_mask_list_free(c->MLkeep[o][q]);
        }
    return any;
}

int sgl_mask_list_select(sgl_ctx* c, int which, int64_t ncol, int32_t nrow, uint64_t seed, uint64_t inv_density, int mask_t,
                         int64_t col_offset, int64_t row_offset) {
    DevMaskList& cur = c->ML[which];
    DevMaskList* keep = c->MLkeep[which];
    if (ml_has_key(cur, ncol, nrow, seed, inv_density, mask_t, col_offset, row_offset)) return SGL_OK;
    const int slots = ml_keep_slots(cur);
    for (int q = 0; q < slots; ++q) {
        if (!ml_has_key(keep[q], ncol, nrow, seed, inv_density, mask_t, col_offset, row_offset)) continue;
        const DevMaskList hit = keep[q];          // kept: it becomes the current one, the current one the most recent kept
        for (int t = q; t > 0; --t) keep[t] = keep[t - 1];
        keep[0] = cur;
        cur = hit;
        return SGL_OK;
    }
    if (slots > 0 && cur.mask_t >= 0) {           // retire the current lists; the oldest kept ones give their buffers to the new mask
        const DevMaskList oldest = keep[slots - 1];
        for (int t = slots - 1; t > 0; --t) keep[t] = keep[t - 1];
        keep[0] = cur;
        cur = oldest;
    }
    for (int q = slots; q < SGL_ML_KEEP; ++q) sgl_mask_list_free(keep[q]);   // (the budget shrank)
    ++c->ml_builds[which];
    return sgl_mask_list_build(c, cur, ncol, nrow, seed, inv_density, mask_t, col_offset, row_offset);
}

// Accumulator tiles of mask_gram_list_kernel: tile t lives in a[8 t : 8 t + 7], named in the instruction text and OUTSIDE
// hipcc's register allocation (the kernel has no other use for AGPRs; mg_agpr_reserve makes the kernel descriptor
// cover them).  With the MFMA builtin -- and equally with an "a"-constrained operand -- hipcc carried the tiles
// through this kernel's loop in VGPRs and moved every one of them to the AGPR file and back around the MFMAs of each
// iteration (240 v_accvgpr moves per three groups at NT = 5; the hashing kernel's loop does not provoke it).
template <int NREG>   // makes the kernel's register count cover a[0 : NREG - 1]
__device__ __forceinline__ void mg_agpr_reserve() {
    static_assert(NREG <= 192, "accumulator file");
    if constexpr (NREG <= 8) asm volatile("" ::: "a7");
    else if constexpr (NREG <= 16) asm volatile("" ::: "a15");
    else if constexpr (NREG <= 24) asm volatile("" ::: "a23");
    else if constexpr (NREG <= 32) asm volatile("" ::: "a31");
    else if constexpr (NREG <= 40) asm volatile("" ::: "a39");
    else if constexpr (NREG <= 48) asm volatile("" ::: "a47");
    else if constexpr (NREG <= 56) asm volatile("" ::: "a55");
    else if constexpr (NREG <= 64) asm volatile("" ::: "a63");
    else if constexpr (NREG <= 72) asm volatile("" ::: "a71");
    else if constexpr (NREG <= 80) asm volatile("" ::: "a79");
    else if constexpr (NREG <= 88) asm volatile("" ::: "a87");
    else if constexpr (NREG <= 96) asm volatile("" ::: "a95");
    else if constexpr (NREG <= 104) asm volatile("" ::: "a103");
    else if constexpr (NREG <= 112) asm volatile("" ::: "a111");
    else if constexpr (NREG <= 120) asm volatile("" ::: "a119");
    else if constexpr (NREG <= 128) asm volatile("" ::: "a127");
    else if constexpr (NREG <= 136) asm volatile("" ::: "a135");
    else if constexpr (NREG <= 144) asm volatile("" ::: "a143");
    else if constexpr (NREG <= 152) asm volatile("" ::: "a151");
    else if constexpr (NREG <= 160) asm volatile("" ::: "a159");
    else if constexpr (NREG <= 168) asm volatile("" ::: "a167");
    else if constexpr (NREG <= 176) asm volatile("" ::: "a175");
    else if constexpr (NREG <= 184) asm volatile("" ::: "a183");
    else if constexpr (NREG <= 192) asm volatile("" ::: "a191");
}
template <int NREG>
__device__ __forceinline__ void mg_agpr_zero() {
    static_for<NREG>([&](auto rc) { asm volatile("v_accvgpr_write_b32 a[%0], 0" ::"n"(decltype(rc)::value)); });
    asm volatile("s_nop 4");
}
// v_mfma_f64_4x4x4_4b_f64 (probed on gfx950, scripts/ubench/mfma444.hip): four independent 4 x 4 x 4 products,
// A[blk][i][k] in lane 16 k + 4 blk + i, B[blk][k][j] in lane 16 k + 4 blk + j, D[blk][i][j] in lane 16 i + 4 blk + j.
template <int R0>
__device__ __forceinline__ void mg_agpr_mfma444(double a, double b) {
    asm volatile("v_mfma_f64_4x4x4_4b_f64 a[%2:%3], %0, %1, a[%2:%3]" ::"v"(a), "v"(b), "n"(R0), "n"(R0 + 1));
}
template <int R0>
__device__ __forceinline__ double mg_agpr_read1() {
    int lo, hi;
    asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(lo) : "n"(R0));
    asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(hi) : "n"(R0 + 1));
    return __hiloint2double(hi, lo);
}
// acc += (lane J of the 16-lane row's g) * v: one FP64 FMA with the DPP row broadcast on its first source
template <int J>
__device__ __forceinline__ void mg_dpp_fmac(double& acc, double g, double v) {
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(g), "v"(v), "n"(J));
}
template <int T>
__device__ __forceinline__ void mg_agpr_mfma(double a, double b) {
    asm volatile("v_mfma_f64_16x16x4_f64 a[%2:%3], %0, %1, a[%2:%3]" ::"v"(a), "v"(b), "n"(8 * T), "n"(8 * T + 7));
}
template <int T>
__device__ __forceinline__ mg_d4 mg_agpr_read() {
    int w[8];
#define MG_RD(R_) asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(w[R_]) : "n"(8 * T + R_))
    MG_RD(0); MG_RD(1); MG_RD(2); MG_RD(3); MG_RD(4); MG_RD(5); MG_RD(6); MG_RD(7);
#undef MG_RD
    return mg_d4{__hiloint2double(w[1], w[0]), __hiloint2double(w[3], w[2]), __hiloint2double(w[5], w[4]), __hiloint2double(w[7], w[6])};
}

// The downdate from the lists: one workgroup per column as in mask_gram_mfma_kernel, wave w takes the groups
// w, w + 4, ... of four consecutive listed rows (the last, partial group goes to the wave whose turn it is).  No
// hash, no queue: per group one 4-byte index load, NB operand loads, the MFMAs.  Operands rotate through three
// register slots without copies (a gather has two groups' MFMAs to arrive in; the index of the next gather is
// loaded before the current gather so that waiting for it does not wait for the gather in flight).  The sums are
// taken in a different order than in the hashing kernel (there: rows dealt to the waves in chunks of 64): equal up
// to rounding, both deterministic.
// REMV > 0 (round 6): the rows beyond 16 NT on the VALU instead -- rows 16 NT + i (i < REMV, REMV = 4, 8, 12) against every column
// block as v_fmac_f64_dpp (the row's factor 16 NT + i sits in lane i of block NT's operand and reaches its 16 lanes by the DPP
// row broadcast: REMV (NT + 1) FMAs of ~4.7 cycles per group where a remainder quad costs (NT + 1) quarter-MFMAs of ~22 and a
// further tile row NT + 1 MFMAs of 64; FP64 MFMA and VALU time add up on this part, profiles/r3_mask_gram_ablation.md).  The
// partial sums of the four row groups and four waves are added in the epilogue (wave order, then lane-row order).
template <int NT, int NPARTS = 1, int PART = 0, int REM = 0, int REMV = 0>
__global__ __launch_bounds__(256) void mask_gram_list_kernel(int64_t col0, int64_t ncols, const int64_t* __restrict__ col_nnz,
                                                             const int64_t* __restrict__ lptr, const int32_t* __restrict__ lidx,
                                                             const double* __restrict__ F, const double* __restrict__ G, int k,
                                                             double* __restrict__ Gout, int raw, const double* __restrict__ zero) {
    constexpr int NTILES_ALL = NT * (NT + 1) / 2;
    constexpr int NTILES = (NTILES_ALL - PART + NPARTS - 1) / NPARTS;
    extern __shared__ __attribute__((aligned(16))) double mg_epi_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kk = lane >> 4;
    const int64_t lc = blockIdx.x;
    if (lc >= ncols) return;
    const int64_t col = col0 + lc;
    double* out = Gout + (size_t)lc * k * k;
    if (col_nnz != nullptr && col_nnz[col] == 0) return;
    constexpr int NB = NT + ((REM > 0 || REMV > 0) ? 1 : 0);
    constexpr int NQ = (REM + 3) / 4;   // remainder rows in quads of four (REM = 2, 4: one; 8: two; 12: three)
    static_assert((REM == 0 && REMV == 0) || NPARTS == 1, "the remainder rows are built for single-part launches");
    static_assert(REM == 0 || REMV == 0, "remainder rows either as quarter-MFMAs or on the VALU");
    double accr[REMV > 0 ? REMV : 1][NB];   // REMV: rows 16 NT + i against columns 16 b + r16, this lane row's groups
#pragma unroll
    for (int i = 0; i < (REMV > 0 ? REMV : 1); ++i)
#pragma unroll
        for (int b = 0; b < NB; ++b) accr[i][b] = 0.0;
    // a[0 : 8 NTILES - 1]: the 16 x 16 tiles; REM > 0: a[8 NTILES + 2 (q NB + b) ...] the remainder rows 16 NT + 4 q + i
    // (i < 4) against column block b as one 4x4x4_4b product per group -- A = factors 16 NT + 4 q .. + 3 of the group's four
    // rows in every quad of the lane rows (each of the four 4-column blocks meets the same four factors): its own load per
    // lane, column 16 NT + 4 q + lane % 4 clamped to the rank (round 3 copied quad 0 of the remainder block across the row
    // with four DPP moves: VALU work, which does not run beside an FP64 MFMA); B = block b as loaded; D lane
    // (i = lane / 16, c = lane % 16) = entry (16 NT + 4 q + i, 16 b + c).  NQ NB quarter-MFMAs of ~22 cycles (measured; a
    // 16x16x4 takes 64): k = 70 is 10 tiles + 2 x 5 of them where the next tile count takes 15 tiles -- the dispatch in
    // kernels_mask.hip lists which (NT, REM) pay.
    constexpr int NREG = 8 * NTILES + 2 * NB * NQ;
    mg_agpr_reserve<NREG>();
    mg_agpr_zero<NREG>();
    const int64_t p0 = lptr[col];
    const int n = (int)(lptr[col + 1] - p0);
    const int nfull = n >> 2;                                   // complete groups of the column
    const int ng = nfull > wave ? (nfull - wave + 3) >> 2 : 0;  // ... of this wave: groups wave + 4 j
    const int32_t* ip = lidx + p0 + 4 * wave + kk;              // entry of lane row kk in group j: ip[16 j]
    // Operands reach the MFMAs straight from their loads: hipcc does not see an MFMA in the asm statements and would
    // not pad the VALU-write -> MFMA-read hazard of a select.  A lane past the rank (only possible in the last block)
    // loads the 0.0 kept behind the list pointers instead.
    const bool last_ok = (NB - 1) * 16 + r16 < k;
    constexpr int NF = NB + NQ;   // operands of a group: NB column blocks, then the NQ remainder quads
    int qcol[NQ > 0 ? NQ : 1];    // (element offsets past the rank would leave the factor row: clamped, their products are never stored)
#pragma unroll
    for (int q = 0; q < NQ; ++q) { const int cq = 16 * NT + 4 * q + (r16 & 3); qcol[q] = (cq < k ? cq : k - 1) - r16; }
    auto gather = [&](double (&f)[NF], int row) {
        const double* src = F + (int64_t)row * k + r16;
#pragma unroll
        for (int b = 0; b + 1 < NB; ++b) f[b] = src[16 * b];
        f[NB - 1] = *(last_ok ? src + 16 * (NB - 1) : zero);
#pragma unroll
        for (int q = 0; q < NQ; ++q) f[NB + q] = src[qcol[q]];
    };
    auto mfma_group = [&](const double (&f)[NF]) {
        if constexpr (NTILES < 3) asm volatile("s_nop 15");   // a tile's next MFMA depends on its last one: keep them apart (hipcc pads this for the builtin)
        static_for<NTILES>([&](auto qc) {   // tile qi of this part is tile t = PART + qi * NPARTS of the triangle
            constexpr int qi = decltype(qc)::value, t = PART + qi * NPARTS;
            mg_agpr_mfma<qi>(f[mg_tile_bi(t)], f[mg_tile_bj(t)]);
        });
        static_for<NQ * NB>([&](auto bc) {
            constexpr int qb = decltype(bc)::value, q = qb / NB, b = qb % NB;
            mg_agpr_mfma444<8 * NTILES + 2 * qb>(f[NB + q], f[b]);
        });
        static_for<REMV * NB>([&](auto bc) {   // (the DPP source f[NT] comes straight from its load: no VALU write for hipcc to miss)
            constexpr int ib = decltype(bc)::value, i = ib / NB, b = ib % NB;
            mg_dpp_fmac<i>(accr[i][b], f[NT], f[b]);
        });
    };
    // Steady state: ONE basic block per three groups, no conditionals (the compiler then counts its loads exactly:
    // with branches inside the loop it waits for vmcnt(0) before every group and nothing is prefetched).  The at most
    // five groups left over run unpipelined.
    double fA[NF], fB[NF], fC[NF];
    int rn = 0;                     // row of the next gather
    if (0 < ng) gather(fA, ip[0]);
    if (2 < ng) rn = ip[32];
    if (1 < ng) gather(fB, ip[16]);
    int j = 0;
    for (; j + 5 < ng; j += 3) {
        int rc = rn;
        rn = ip[16 * (j + 3)];
        gather(fC, rc);
        mfma_group(fA);
        rc = rn;
        rn = ip[16 * (j + 4)];
        gather(fA, rc);
        mfma_group(fB);
        rc = rn;
        rn = ip[16 * (j + 5)];
        gather(fB, rc);
        mfma_group(fC);
    }
    if (j < ng) mfma_group(fA);
    if (j + 1 < ng) mfma_group(fB);
    for (int jj = j + 2; jj < ng; ++jj) {
        gather(fC, ip[16 * jj]);
        mfma_group(fC);
    }
    if ((n & 3) != 0 && wave == (nfull & 3)) {   // the partial group: rows beyond the list contribute zeros
        const bool valid = kk < (n & 3);
        const int row = valid ? lidx[p0 + 4 * nfull + kk] : 0;
        double fz[NF];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int fr = b * 16 + r16;
            fz[b] = *((valid && fr < k) ? F + (int64_t)row * k + fr : zero);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) fz[NB + q] = *(valid ? F + (int64_t)row * k + r16 + qcol[q] : zero);
        mfma_group(fz);
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMA's write-back before the accumulators are read (hipcc sees no MFMA)
    {
        const double none[1][NB] = {};
        mg_epilogue<NT, NPARTS, PART, 0, MG_TB(NTILES, (REMV > 0 ? 4 : REM), NB), NTILES>([&](auto qc) { return mg_agpr_read<decltype(qc)::value>(); }, none, mg_epi_raw,
                                                                         wave, lane, G, out, k, raw);
    }
    static_for<NQ>([&](auto qq) {   // remainder rows, a quad at a time: the four waves' sums in wave order
        constexpr int q = decltype(qq)::value;
        __syncthreads();
        static_for<NB>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            mg_epi_raw[(b * 4 + wave) * 64 + lane] = mg_agpr_read1<8 * NTILES + 2 * (q * NB + b)>();
        });
        __syncthreads();
        for (int o = wave * 64 + lane; o < NB * 64; o += 256) {
            const int b = o >> 6, l = o & 63, i = l >> 4, c16 = l & 15;
            const double* src = mg_epi_raw + (size_t)b * 4 * 64 + l;
            double sub = ((src[0] + src[64]) + src[128]) + src[192];
            const int row = 16 * NT + 4 * q + i, cc = 16 * b + c16;
            if (4 * q + i < REM && row < k && cc < k && cc <= row) {
                if (row == cc && !raw) sub += 1e-15;
                const double v = raw ? sub : G[(size_t)cc * k + row] - sub;
                out[(size_t)cc * k + row] = v;
                if (row != cc) out[(size_t)row * k + cc] = v;
            }
        }
    });
    static_for<(REMV + 3) / 4>([&](auto qq) {   // VALU remainder rows, four at a time: the partials of the 4 waves x 4 lane rows in fixed order
        constexpr int q4 = decltype(qq)::value, nrows = (REMV - 4 * q4 < 4) ? REMV - 4 * q4 : 4;
        __syncthreads();
        static_for<nrows>([&](auto ic) {
            constexpr int il = decltype(ic)::value;
#pragma unroll
            for (int b = 0; b < NB; ++b) mg_epi_raw[((il * NB + b) * 4 + wave) * 64 + lane] = accr[4 * q4 + il][b];
        });
        __syncthreads();
        for (int o = wave * 64 + lane; o < nrows * NB * 16; o += 256) {
            const int ib = o >> 4, c16 = o & 15, il = ib / NB, b = ib - il * NB;
            const double* src = mg_epi_raw + (size_t)ib * 4 * 64 + c16;
            double sub = 0.0;
            for (int w = 0; w < 4; ++w)
                for (int g = 0; g < 4; ++g) sub += src[w * 64 + g * 16];
            const int row = 16 * NT + 4 * q4 + il, cc = 16 * b + c16;
            if (row < k && cc < k && cc <= row) {
                if (row == cc && !raw) sub += 1e-15;
                const double v = raw ? sub : G[(size_t)cc * k + row] - sub;
                out[(size_t)cc * k + row] = v;
                if (row != cc) out[(size_t)row * k + cc] = v;
            }
        }
    });
}

template <int NT, int NPARTS = 1, int PART = 0, int REM = 0, int REMV = 0>
static int launch_mask_gram_list(dim3 g, dim3 b, hipStream_t s, int64_t col0, int64_t ncols, const int64_t* col_nnz, const DevMaskList* L,
                                 const double* F, const double* G, int k, double* Gcols, int raw) {
    constexpr int NTILES = (NT * (NT + 1) / 2 - PART + NPARTS - 1) / NPARTS, NB = NT + ((REM > 0 || REMV > 0) ? 1 : 0);
    constexpr size_t lds = (size_t)MG_TB(NTILES, (REMV > 0 ? 4 : REM), NB) * 4 * 256 * sizeof(double);   // REMV: batches of four rows x NB blocks
    SGLCHK((sgl_allow_dynamic_lds<&mask_gram_list_kernel<NT, NPARTS, PART, REM, REMV>>((int)lds)));
    mask_gram_list_kernel<NT, NPARTS, PART, REM, REMV><<<g, b, lds, s>>>(col0, ncols, col_nnz, L->ptr, L->idx, F, G, k, Gcols, raw,
                                                                   reinterpret_cast<const double*>(L->ptr + L->ncol + 1));
    return SGL_OK;
}
