// LDS-tiled sparse accumulate:  B[:, c] = sum_{(r, v) in column c} v * F[:, r]
// (predict, src/singlet.cpp:341-343) with the gathered operand F served from
// LDS instead of L2.
//
// Why: every non-zero needs k doubles of F (400 B at k = 50) against 12 B of
// matrix data, so the accumulate is bound by operand delivery, not by the HBM
// stream.  L2 delivers ~34 TB/s chip-wide, LDS ~150 TB/s.
// Measured on MI355X (scripts/ubench/lds_rate.hip): the LDS retires one wave
// instruction per ~1.7 ns per CU whether it is ds_read_b64 or ds_read_b128, so
// the kernel is built around ds_read_b128: a lane reads TWO consecutive factor
// rows of F, 32 lanes cover k <= 64, and the two half-waves work on two
// different non-zeros at once (two non-zeros per LDS instruction).
//
// Layout ("re-blocked stream", built once per (matrix, k) by sgl_tiled_build):
//   * rows are cut into tiles of TR rows, TR * KS * 8 B <= 160 KiB - 512 B (one LDS
//     tile; KS = k rounded up to even so every row starts 16-byte aligned);
//   * the LDS tile is a ring of two slots of D = TR / 2 rows: row block b (rows [b D, (b + 1) D)) sits in slot
//     b % 2, and stage b of the loop has blocks b and b + 1 in LDS.  After stage b one barrier frees the slot of
//     block b, block b + 2 is staged into it, a second barrier; the first stage of a tile range stages two blocks;
//   * columns are cut into wave blocks of 64 columns; a workgroup of 8 waves
//     owns 512 columns and keeps their k-vectors in VGPRs across all row tiles.
//     Lanes 0-31 of a wave accumulate column p of the block, lanes 32-63 column
//     32 + p ("column pair" p = 0..31), lane l holding factors 2(l&31), +1;
//   * per (wave block wb, stage b) -- a chunk -- the entries of the pair's two
//     columns are stored as two half-streams that advance in lockstep.  Sliding window (round 7): in stage b every
//     column finishes its entries of block b and may run ahead into block b + 1 -- the pair takes n = the most
//     block-b entries either column has left, rounded up to 4, and each column fills those n steps with its own
//     next entries of the window (x = 0 pads only where it has none left; tiled_count_kernel).  Balanced chunks:
//     the workgroup's eight waves meet at a barrier after every stage, so a stage lasts as long as its longest
//     chunk; a wave block whose chunk is shorter than the longest of the eight takes the difference as further
//     run-ahead, spread level over its pairs and only in groups that hold real entries for both columns -- the
//     waves' chunks of a stage come out within ~1 % of each other instead of ~9 % (i.i.d. columns), for slightly
//     fewer stored entries (SGL_TILED_NO_BALANCE=1: the rule before).  The chunk is
//     rounded up to a multiple of 32 entries per half the same way, by extra groups on the last pairs.  64
//     consecutive stream slots hold 32 entries of the A half then 32 of the B half, so one coalesced
//     64-lane load fetches a "set".  Two arrays: roff (byte offset of the row inside the LDS ring: slot
//     (r / D) % 2, row r % D) and x.  Chunks are ordered (wb, b): one wave reads ONE linear stream;
//   * cnt[(wb * NB + b) * 32 + p] = number of 4-entry groups of pair p.
// The schedule never runs ahead across the edge of a tile range (blockIdx.y, tail pieces): each range is a slab of
// its own.  Against runs padded to equal length inside every tile (rounds 1 - 6: 1.207 stored entries per
// non-zero at config 3) the window stores ~1.05 (scripts/layout_emulate.py models the count exactly).
// Inside a column the products are added in stored (ascending row) order, as
// in the reference; pads add x = 0 times a finite F entry.
//
// Ranks up to 32 use FOUR columns per LDS instruction instead of two (NSL = 4, round 4): a lane still holds two
// factors, so one 16-lane DPP row covers the rank and the four rows of a wave work on four columns (a column QUAD);
// a set of 64 stream slots holds 16 entries of each of the quad's columns -- the operand layout row_newbcast wants,
// so a set needs no preparation -- a wave owns 32 quads = 128 columns, and the LDS tile rows are 256 B apart whatever
// the rank (every tile row starts on bank 0: the 16-lane groups of ds_read_b128 mix two DPP rows and stay
// conflict-free only then).  Everything below is written for NSL column slots per instruction (2 or 4).
//
// When the column count is too small to fill the chip (W-update: 30 k genes)
// the tile range is split over blockIdx.y; each split writes a partial k x ncol
// slab and acc_tiled_reduce sums the slabs in a fixed order.
#include "sgl_internal.h"
#include <hipcub/hipcub.hpp>
#include <stdlib.h>
#include <utility>
#include <type_traits>

#define TILED_NW 8           // waves per workgroup (512 threads -> 256 VGPRs per lane)
#define TILED_CW 64          // columns per wave
#define TILED_NP 32          // column pairs per wave
#define TILED_LDS_BYTES (160 * 1024 - 512)  // the whole 160 KiB of a CU minus the read-past-the-row slack
#define TILED_SLACK 4096     // stream entries readable past the end (ring prefetch: 256 - 512 entries, + the L2 prefetch laps beyond it)

// ---------------------------------------------------------------- build -----
// groups per (wb, t, pair) and entries per chunk
// Slot (half h, pair p) of wave block wb holds the column at SORTED position wb * 64 + 2p + h: the columns are taken in
// the order of descending non-zero count (perm), so the two columns of a pair are neighbours in that order and the
// runs they are padded to are of similar length whatever the skew of the matrix.
__device__ __forceinline__ int64_t tiled_slot_col(const int32_t* __restrict__ perm, int64_t ncol, int64_t wb, int h, int p, int nsl) {
    const int64_t pos = wb * (TILED_NP * nsl) + nsl * p + h;
    if (pos >= ncol) return -1;
    return perm ? (int64_t)perm[pos] : pos;
}

// Tile ranges of wave block wb (blockIdx.y of the accumulate, or the pieces of a tail-split workgroup): nr ranges of floor / ceil
// of T / nr tiles.  The range holding row block b ends at block tiled_range_end(...) (exclusive): the schedule never runs ahead
// across it -- an entry taken into another range would land in another slab and change the sums.
__device__ __forceinline__ int tiled_ranges_of(int64_t wb, int R, int64_t tail_wg0, int tail_R) {
    return (tail_R > 1 && tail_wg0 >= 0 && wb / TILED_NW >= tail_wg0) ? tail_R : R;
}
__device__ __forceinline__ int tiled_range_end(int b, int T, int NB, int nr) {
    const int t = b >> 1;
    const int y = (int)(((int64_t)(t + 1) * nr - 1) / T);           // range of tile t: floor(y T / nr) <= t < floor((y + 1) T / nr)
    const int b1 = 2 * (int)(((int64_t)(y + 1) * T) / nr);
    return b1 < NB ? b1 : NB;
}

// The schedule (sliding window).  The LDS tile is a ring of two row blocks of D = TR / 2 rows; stage b of a tile range holds
// blocks b and b + 1.  In the chunk (wb, b) every column finishes its entries of block b and may run ahead into block b + 1:
// a column unit (pair / quad) takes n = the most entries any of its columns has left in block b, rounded up to groups of
// four, and each of its columns fills those n steps with its own next entries of the window -- pads (x = 0) only where a
// column has none left.
// Balance: the eight waves of an accumulate workgroup meet at a barrier after every stage, so a stage lasts as long as
// the longest of their chunks.  With tot = a wave block's must groups, target = the largest tot of the workgroup's wave
// blocks in whole sets: no stage can be shorter.  A wave block below it takes E = target - tot further groups as run-ahead
// now -- work it would otherwise do in stage b + 1 -- but only groups that hold a real entry for every present column of
// the unit: f = floor(the least window entries left over those columns / 4) - must groups a unit can give.  They are
// spread level: t = the largest level with sum(min(f, t)) <= E, unit p gets min(f_p, t), what is left goes one each to
// the highest-numbered units with f_p > t.  A wave block whose units cannot give E takes all they can and stays short:
// it is never padded up to the target.  (SGL_TILED_NO_BALANCE=1: no such groups, the rule before.)
// The chunk is then rounded up to whole 64-slot sets by extra groups on the last units, each taking as many as its
// columns still have window entries for; what no unit can fill goes on unit 31 as pads.
// One workgroup of eight waves per (accumulate workgroup, tile range) -- a range starts over at its first block, so the
// ranges are independent -- one wave per wave block, lane p = unit p (lanes 32-63 mirror 0-31), walking the stages of the
// range in order; the eight tot are exchanged through LDS.  The wave blocks of a workgroup share their range count.
// cnt = groups per (chunk, unit) -- at most 2 D / 4 + 7 <= 253: a byte; ahead = entries of block b a column took in
// stage b - 1 (<= D); chunk_entries = stored entries of the chunk (all slots).
__device__ __forceinline__ int tiled_sum32(int v) {
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}
// sum of v over the units above this one (p + 1 .. 31)
__device__ __forceinline__ int tiled_sum_above(int v, int p) {
    int suf = v;
    for (int o = 1; o < 32; o <<= 1) {
        const int w = __shfl_down(suf, o, 32);
        if (p + o < 32) suf += w;
    }
    return suf - v;
}

__global__ __launch_bounds__(64 * TILED_NW) void tiled_count_kernel(const int64_t* __restrict__ seg, const int32_t* __restrict__ perm,
                                                                    int64_t ncol, int T, int NB, int64_t nwb, int R, int64_t tail_wg0,
                                                                    int tail_R, uint8_t* __restrict__ cnt, uint16_t* __restrict__ ahead,
                                                                    int64_t* __restrict__ chunk_entries, int nsl, int balance) {
    __shared__ int wtot[TILED_NW];
    const int lane = threadIdx.x & 63, p = lane & 31, wave = (int)(threadIdx.x >> 6);
    const int64_t wb = (int64_t)blockIdx.x * TILED_NW + wave;
    const bool wact = wb < nwb;   // wave-uniform; a wave without a wave block still goes through the barriers
    const int gps = 16 / nsl;     // groups (of 4 entries per slot) in a 64-slot set
    // tile range blockIdx.y of the workgroup's nr (<= T: none is empty), the ranges of tiled_range_end
    const int nr = tiled_ranges_of((int64_t)blockIdx.x * TILED_NW, R, tail_wg0, tail_R);
    if ((int)blockIdx.y >= nr) return;   // workgroup-uniform
    const int b0 = 2 * (int)(((int64_t)blockIdx.y * T) / nr);
    const int e1 = 2 * (int)((((int64_t)blockIdx.y + 1) * T) / nr);
    const int b1 = e1 < NB ? e1 : NB;
    int64_t col[4], pos[4];
    for (int h = 0; h < 4; ++h) col[h] = (wact && h < nsl) ? tiled_slot_col(perm, ncol, wb, h, p, nsl) : -1;
    for (int h = 0; h < 4; ++h) pos[h] = (col[h] >= 0 && b0 < b1) ? seg[(int64_t)b0 * ncol + col[h]] : 0;
    for (int b = b0; b < b1; ++b) {
        const int hi = b + 2 < b1 ? b + 2 : b1;
        int64_t must = 0, avail = 0, least = INT64_MAX, ew[4];
        for (int h = 0; h < 4; ++h) {
            ew[h] = 0;
            if (col[h] >= 0) {
                const int64_t eb = seg[(int64_t)(b + 1) * ncol + col[h]];
                ew[h] = seg[(int64_t)hi * ncol + col[h]];
                must = eb - pos[h] > must ? eb - pos[h] : must;
                avail = ew[h] - pos[h] > avail ? ew[h] - pos[h] : avail;
                least = ew[h] - pos[h] < least ? ew[h] - pos[h] : least;
            }
        }
        int g = (int)((must + 3) >> 2);
        int tot = tiled_sum32(g);
        if (balance) {
            if (lane == 0) wtot[wave] = tot;   // 0 for a wave without a wave block
            __syncthreads();
            int sets = 0;
            for (int w = 0; w < TILED_NW; ++w) sets = max(sets, (wtot[w] + gps - 1) / gps);
            __syncthreads();   // everyone has read wtot: the next stage may write it
            const int E = sets * gps - tot;
            int f = least == INT64_MAX ? 0 : (int)(least >> 2) - g;
            if (f < 0) f = 0;
            int t = 0;   // the largest level in [0, 255] with sum(min(f, t)) <= E (f <= 2 D / 4 <= 246)
            for (int step = 128; step > 0; step >>= 1)
                if (tiled_sum32(min(f, t + step)) <= E) t += step;
            int add = min(f, t);
            const int left = E - tiled_sum32(add);
            const int hot = f > t ? 1 : 0;
            const int hot_above = tiled_sum_above(hot, p);   // (every lane takes part in the shuffles)
            if (hot && hot_above < left) ++add;
            g += add;
            tot = tiled_sum32(g);
        }
        const int cap = (int)((avail + 3) >> 2) - g;
        const int rem = (gps - (tot & (gps - 1))) & (gps - 1);
        const int above = tiled_sum_above(cap, p);   // run-ahead groups units p + 1 .. 31 can fill
        int extra = rem - above < cap ? rem - above : cap;
        if (extra < 0) extra = 0;
        const int all = __shfl(above + cap, 0, 32);
        if (p == TILED_NP - 1 && rem > all) extra += rem - all;
        g += extra;
        const int64_t u = wb * NB + b;
        if (wact && lane < 32) {
            cnt[u * TILED_NP + p] = (uint8_t)g;
            for (int h = 0; h < nsl; ++h)
                ahead[u * (TILED_NP * nsl) + nsl * p + h] = col[h] >= 0 ? (uint16_t)(pos[h] - seg[(int64_t)b * ncol + col[h]]) : (uint16_t)0;
        }
        if (wact && lane == 0) chunk_entries[u] = (int64_t)(tot + rem) * 4 * nsl;
        for (int h = 0; h < 4; ++h) pos[h] += (4 * (int64_t)g < ew[h] - pos[h]) ? 4 * (int64_t)g : ew[h] - pos[h];
    }
}

// one wave per chunk (wb, b): copy / pad the runs of the 32 column units.  roff is ring-relative: row r of block r / D sits
// in LDS slot (r / D) % 2
__global__ __launch_bounds__(256) void tiled_fill_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                         const int64_t* __restrict__ seg, const int32_t* __restrict__ perm,
                                                         int64_t ncol, int T, int NB, int64_t nwb, int R, int64_t tail_wg0, int tail_R,
                                                         int D, int row_bytes, const uint8_t* __restrict__ cnt,
                                                         const uint16_t* __restrict__ ahead, const int64_t* __restrict__ cstart,
                                                         uint32_t* __restrict__ sroff, double* __restrict__ sx,
                                                         int masked, uint64_t seed, SglDiv inv_density, int mask_t,
                                                         int64_t col_off, int64_t row_off, int nsl) {
    const int lane = threadIdx.x & 63;
    const int eps = 64 / nsl, eps_sh = nsl == 4 ? 4 : 5;   // entries of one column slot in a 64-slot set
    const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = gw; u < nwb * NB; u += nw) {
        const int64_t wb = u / NB;
        const int b = (int)(u - wb * NB);
        const int b1 = tiled_range_end(b, T, NB, tiled_ranges_of(wb, R, tail_wg0, tail_R));
        const int hi = b + 2 < b1 ? b + 2 : b1;
        const int64_t c0 = cstart[u];
        int P = 0;  // position in the half-streams
        for (int p = 0; p < TILED_NP; ++p) {
            const int n4 = 4 * (int)cnt[u * TILED_NP + p];
            if (n4 == 0) continue;
            for (int h = 0; h < nsl; ++h) {
                const int64_t col = tiled_slot_col(perm, ncol, wb, h, p, nsl);
                int64_t a = 0, e = 0;
                if (col >= 0) {
                    a = seg[(int64_t)b * ncol + col] + ahead[u * (TILED_NP * nsl) + nsl * p + h];
                    e = seg[(int64_t)hi * ncol + col];
                }
                for (int q = lane; q < n4; q += 64) {
                    uint32_t ro = 0;
                    double xv = 0.0;
                    if (a + q < e) {
                        const int32_t r = idx[a + q];
                        const int blk = r >= (b + 1) * D ? b + 1 : b;
                        ro = (uint32_t)((blk & 1) * D + (r - blk * D)) * (uint32_t)row_bytes;
                        xv = x[a + q];
                        if (masked) {  // predict_mask leaves the drawn entries out (src/singlet.cpp:449-457): x = 0 adds +0 * F
                            const uint64_t gc = (uint64_t)(col + col_off), gr = (uint64_t)(r + row_off);
                            if (mask_t ? sgl_draw(seed, gr, gc, inv_density) : sgl_draw(seed, gc, gr, inv_density)) xv = 0.0;
                        }
                    }
                    const int pos = P + q;
                    const int64_t dst = c0 + (int64_t)(pos >> eps_sh) * 64 + h * eps + (pos & (eps - 1));
                    if (sroff != nullptr) sroff[dst] = ro;
                    sx[dst] = xv;
                }
            }
            P += n4;
        }
    }
}

// schedule table of the chunk loop (gen_acc_tiled.py, GenTab): one u16 per group of four entry tuples, in stream order --
// the M0 word (destination-relative register index 4 * unit, 0x8000 = VDST_REL) of the column unit the group belongs
// to; the padding groups at the end of a chunk are booked on the last unit, like their entries.  One wave per chunk.
__global__ __launch_bounds__(256) void tiled_gtab_kernel(const uint8_t* __restrict__ cnt, const int64_t* __restrict__ cstart,
                                                         int64_t nchunks, int nsl, uint16_t* __restrict__ gtab) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = gw; u < nchunks; u += nw) {
        int64_t g0 = cstart[u] / (4 * nsl);
        for (int p = 0; p < TILED_NP; ++p) {
            const int n = (int)cnt[u * TILED_NP + p];
            for (int q = lane; q < n; q += 64) gtab[g0 + q] = (uint16_t)(0x8000u | (unsigned)(4 * p));
            g0 += n;
        }
    }
}

template <typename T_>
static int t_alloc(T_** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = sgl_pool_malloc((void**)p, count * sizeof(T_));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sgl_set_error("hipMalloc of %zu bytes failed: %s", count * sizeof(T_), hipGetErrorString(e));
        return SGL_ENOMEM;
    }
    return SGL_OK;
}

// grow-only buffer: keeps the allocation when it is large enough (3 % headroom on growth: the stream size moves
// by a few per cent with the rank)
template <typename T_>
static int t_reserve(T_** p, size_t* cap, size_t count) {
    if (*p != nullptr && *cap >= count) return SGL_OK;
    if (*p) (void)sgl_pool_free(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = count + count / 32 + 64;
    SGLCHK(t_alloc(p, want));
    *cap = want;
    return SGL_OK;
}

void sgl_tiled_free(DevTiled& S) {
    if (S.seg) (void)sgl_pool_free(S.seg);
    if (S.perm) (void)sgl_pool_free(S.perm);
    if (S.roff) (void)sgl_pool_free(S.roff);
    if (S.x) (void)sgl_pool_free(S.x);
    if (S.cstart) (void)sgl_pool_free(S.cstart);
    if (S.cnt) (void)sgl_pool_free(S.cnt);
    if (S.ahead) (void)sgl_pool_free(S.ahead);
    if (S.gtab) (void)sgl_pool_free(S.gtab);
    if (S.part) (void)sgl_pool_free(S.part);
    if (S.xm) (void)sgl_pool_free(S.xm);
    S = DevTiled();
}

// SGL_TILED_SORT=0 keeps the columns in matrix order (the round-2 layout; kept for A/B measurements and the tests)
static bool tiled_sort_columns() {
    const char* e = getenv("SGL_TILED_SORT");
    return !(e && *e == '0');
}
// SGL_TILED_NO_BALANCE=1 leaves the waves' chunks of a stage as unequal as their must groups are (the rule before the
// balance of tiled_count_kernel; kept for A/B measurements and the tests)
static bool tiled_balance_chunks() {
    const char* e = getenv("SGL_TILED_NO_BALANCE");
    return !(e && *e && *e != '0');
}

__global__ void tiled_col_keys_kernel(const int64_t* __restrict__ p, int64_t ncol, uint32_t* __restrict__ keys, int32_t* __restrict__ iota) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncol; c += (int64_t)gridDim.x * blockDim.x) {
        keys[c] = (uint32_t)(p[c + 1] - p[c]);
        iota[c] = (int32_t)c;
    }
}

// S.perm[pos] = column at position pos of the descending-count order
static int tiled_build_perm(sgl_ctx* c, const DevCSC& M, DevTiled& S) {
    hipStream_t s = c->stream;
    const int64_t n = M.ncol;
    SGLCHK(t_reserve(&S.perm, &S.cap_perm, (size_t)n));
    uint32_t *keys = nullptr, *keys_out = nullptr;
    int32_t* iota = nullptr;
    void* tmp = nullptr;
    int rc = t_alloc(&keys, (size_t)n);
    if (rc == SGL_OK) rc = t_alloc(&keys_out, (size_t)n);
    if (rc == SGL_OK) rc = t_alloc(&iota, (size_t)n);
    if (rc == SGL_OK && n > 0) {
        const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
        tiled_col_keys_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(M.p, n, keys, iota);
        size_t tmp_bytes = 0;
        if (hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, keys, keys_out, iota, S.perm, n, 0, 32, s) != hipSuccess) rc = SGL_EHIP;
        if (rc == SGL_OK && sgl_pool_malloc(&tmp, tmp_bytes ? tmp_bytes : 1) != hipSuccess) { (void)hipGetLastError(); rc = SGL_ENOMEM; }
        if (rc == SGL_OK && hipcub::DeviceRadixSort::SortPairsDescending(tmp, tmp_bytes, keys, keys_out, iota, S.perm, n, 0, 32, s) != hipSuccess) rc = SGL_EHIP;
    }
    // share of the non-zeros held by the heaviest workgroup's columns (the first 8 x 64 of the order): the tile-range
    // split below sizes its work units by it
    static_assert(TILED_CW == 64, "pair layout: 64 columns per wave");
    std::vector<uint32_t> top_v((size_t)TILED_NW * TILED_CW * 2);   // quad layout: 128 columns per wave
    uint32_t* top = top_v.data();
    const int64_t ntop = std::min<int64_t>(n, (int64_t)top_v.size());
    if (rc == SGL_OK && ntop > 0 && hipMemcpyAsync(top, keys_out, sizeof(uint32_t) * (size_t)ntop, hipMemcpyDeviceToHost, s) != hipSuccess) rc = SGL_EHIP;
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == SGL_OK && e == hipSuccess) {
        int64_t tn = 0, tn2 = 0;
        for (int64_t q = 0; q < ntop; ++q) {
            if (q < TILED_NW * TILED_CW) tn += top[q];
            tn2 += top[q];
        }
        S.top_share = M.nnz > 0 ? (double)tn / (double)M.nnz : 0.0;
        S.top_share4 = M.nnz > 0 ? (double)tn2 / (double)M.nnz : 0.0;
    }
    if (keys) (void)sgl_pool_free(keys);
    if (keys_out) (void)sgl_pool_free(keys_out);
    if (iota) (void)sgl_pool_free(iota);
    if (tmp) (void)sgl_pool_free(tmp);
    if (rc == SGL_OK && e != hipSuccess) rc = SGL_EHIP;
    if (rc != SGL_OK) { sgl_set_error("tiled build: sorting the columns by their non-zero count failed"); return rc; }
    S.perm_nnz = M.nnz;
    return SGL_OK;
}

void sgl_trace_setup(const char* what);   // singlet_hip.hip (SGL_TRACE_SETUP=1)

int sgl_tiled_build(sgl_ctx* c, const DevCSC& M, int k, DevTiled& S) {
    hipStream_t s = c->stream;
    // ranks up to 32: four columns per LDS instruction (SGL_TILED_NO_QUAD=1: the pair layout at every rank; A/B, tests)
    const int nsl = (k <= 32 && !getenv("SGL_TILED_NO_QUAD")) ? 4 : 2;
    // same matrix (any change of it frees the streams), same part size: the stream is still valid
    const bool balance = tiled_balance_chunks();
    if (S.built && S.k == k && S.NSL == nsl && S.ncol == M.ncol && S.nrow == M.nrow && S.src_nnz == M.nnz &&
        (S.perm != nullptr) == tiled_sort_columns() && S.balance == balance)
        return SGL_OK;
    S.built = false;
    S.balance = balance;
    S.xm_mask_t = -1;   // the masked value array follows the stream layout
    S.k = k;
    S.NSL = nsl;
    S.CW = TILED_NP * nsl;
    // LDS row stride in doubles.  Pair layout: k rounded up to even (rows start 16-byte aligned).  Quad layout: 32 for
    // every rank -- all tile rows must start on the same bank (header comment)
    const int KS = nsl == 4 ? 32 : ((k + 1) & ~1);
    S.KS = KS;
    int TR = TILED_LDS_BYTES / (KS * 8);
    TR = TR / 8 * 8;
    if (TR > 984) TR = 984;  // groups per pair (+ <= 7 chunk-padding groups) must fit a byte
    static_assert(984 / 4 + 7 <= 255, "cnt: a unit's groups of one stage -- at most its window of TR rows in fours, + 7 pads -- in a byte");
    if (TR < 8 || k > 64) { sgl_set_error("tiled accumulate: k=%d unsupported", k); return SGL_EINVAL; }
    S.nwb = ((int64_t)M.ncol + S.CW - 1) / S.CW;
    // A small matrix cannot fill the chip with LDS-sized tiles even when every tile is a range of its own (pbmc3k: 3 column
    // groups x 22 tiles on the cell side, 14 x 5 on the gene side): shorter tiles -- at least 128 rows, so that a column still
    // brings a few entries per tile -- until column groups x tiles reach the 256 CUs.  (SGL_TILED_FULL_TILES=1: tests of the
    // chunk loop's extremes -- a column dense over a whole LDS-sized tile.)
    {
        const int64_t groups = (S.nwb + TILED_NW - 1) / TILED_NW, T0 = ((int64_t)M.nrow + TR - 1) / TR;
        if (groups * T0 < 256 && !getenv("SGL_TILED_FULL_TILES")) {
            const int64_t want = std::min<int64_t>((256 + groups - 1) / groups, ((int64_t)M.nrow + 127) / 128);
            if (want > T0) TR = std::min<int>(TR, (int)(((((int64_t)M.nrow + want - 1) / want) + 7) / 8 * 8));
        }
    }
    S.TR = TR;
    S.T = (int)((M.nrow + TR - 1) / TR);
    const int D = TR / 2;   // rows of one LDS ring slot (TR is a multiple of 8)
    S.NB = (int)((M.nrow + D - 1) / D);
    S.ncol = M.ncol;
    S.nrow = M.nrow;
    S.src_nnz = M.nnz;
    const int64_t nchunks = S.nwb * S.NB;

    // column order of the stream: descending non-zero count (stable: ties in matrix order); depends on the matrix
    // only, so a rank sweep computes it once
    int rc = SGL_OK;
    if (!tiled_sort_columns()) {
        if (S.perm) { (void)sgl_pool_free(S.perm); S.perm = nullptr; S.cap_perm = 0; }
    } else if (!S.perm || S.perm_nnz != M.nnz || S.cap_perm < (size_t)M.ncol) {
        rc = tiled_build_perm(c, M, S);
    }
    sgl_trace_setup("  stream: column order");
    // split of the tile range over blockIdx.y so that the grid fills 256 CUs (1 workgroup per CU).  Decided before the stream is
    // counted: the schedule does not run ahead across a range edge.  Its cost model needs the stream size, estimated here from
    // the padding of the sliding-window layout (1.03 - 1.06 entries per non-zero on i.i.d. columns; scripts/layout_emulate.py).
    const double E_est = (double)M.nnz * 1.06;
    // Two reasons to split: too few column groups to fill the chip (W-update: 30 k genes = 59 workgroups), and -- with
    // the columns sorted by count -- a heaviest workgroup that alone would outlast the average CU's whole share (skewed
    // genes: the top 512 of 30 000 held 11 % of the non-zeros and the pass took 22 ms instead of 11): its tile range is
    // cut until one unit is about a third of a CU's share; workgroups are dispatched heaviest first.
    const int64_t nwg_x = (S.nwb + TILED_NW - 1) / TILED_NW;
    int R = 1;
    const int r_fill = nwg_x < 1024 ? (int)std::max<int64_t>(1, (512 + nwg_x - 1) / nwg_x) : 1;
    // (only when that workgroup really stands out: on i.i.d. columns its share is 1 / nwg_x and the fill rule decides,
    // with the column groups running fastest -- sizing by balance there cost 8 GB of factor-tile traffic per pass)
    const double top_share = nsl == 4 ? S.top_share4 : S.top_share;   // of the heaviest workgroup's 512 / 1024 columns
    const bool skewed = S.perm && top_share * (double)nwg_x > 1.5;
    const int r_bal = skewed ? (int)std::min<double>(256.0, ceil(top_share * 256.0 / 0.35)) : 1;
    if (r_bal > r_fill) {
        double best = -1.0;
        // (a fill factor beyond the tile count: every tile its own range -- round 3 left the range whole there, "such a matrix is
        // tiny", and the gene side of pbmc3k -- 14 column groups, 5 tiles, half of the non-zeros in the first group -- ran 1.07 ms)
        const int rmin = std::max(r_fill, (int)std::min<int64_t>(r_bal, std::max(1, S.T)));
        if (rmin > S.T) R = std::max(1, S.T);
        for (int r = rmin; r <= std::min<int64_t>(S.T, rmin + rmin / 4 + 4); ++r) {
            const int tpr = (S.T + r - 1) / r;
            const int reff = (S.T + tpr - 1) / tpr;  // ranges actually non-empty
            const double wgs = (double)nwg_x * reff;
            const double eff = wgs / (ceil(wgs / 256.0) * 256.0);
            if (eff > best + 1e-9) { best = eff; R = reff; }
        }
    } else if (r_fill > 1 && S.T > 1) {
        // (matrices of every size: for most of round 4 the range stayed whole below 4 M entries -- "a pass takes microseconds
        // either way" -- and pbmc3k, 2.3 M non-zeros in 3 column groups of the quad layout, ran its 22 tiles on THREE CUs:
        // 0.83 / 1.07 ms per pass where config 2, with 22 times the non-zeros, takes 0.21.  A split adds the ranges' partial
        // sums: equal to the whole range up to rounding, and SGL_TILED_RANGES=1 keeps the reference's order for the tests that
        // compare bits.)
        // Too few column groups to fill the chip: cut the tile range into R pieces (sizes floor / ceil of T / R), R by a
        // cost model.  (Taking the count of workgroups nearest a multiple of 256 instead gave R = T at
        // BASELINE config 2 in the quad layout (49 column groups x 32 tiles: 1568 workgroups of ONE tile each, every
        // one clearing and staging 160 KB and writing a 245 KB slab: 0.41 ms per pass; 5 ranges: see profiles/.)
        //   time(R) = rounds x (largest unit x t_tile + t_wg) + t_reduce(R),   rounds = ceil(groups x R / 256 CUs)
        // t_tile = one workgroup's entry tuples of one tile at the measured 2.4 ns per tuple per CU + 2.5 us of staging,
        // t_wg = 6 us per workgroup (launch, zeroing, output), t_reduce = the slabs written and read back at 4 TB/s.
        const double t_tile = E_est / (double)nsl / ((double)nwg_x * (double)S.T) * 2.4e-9 + 2.5e-6;
        const double t_wg = 6e-6;
        double best = 1e300;
        for (int r = 1; r <= std::min<int64_t>(S.T, 64); ++r) {
            const double wgs = (double)nwg_x * r;
            const double rounds = ceil(wgs / 256.0);
            const int largest = (S.T + r - 1) / r;
            const double cost = rounds * ((double)largest * t_tile + t_wg) + (r > 1 ? (double)r * (double)k * (double)M.ncol * 16.0 / 4e12 : 0.0);
            if (cost < best * (1.0 - 1e-9)) { best = cost; R = r; }
        }
    }
    if (const char* fr = getenv("SGL_TILED_RANGES")) {   // tests: force the slab path (or the whole range) on small matrices
        if (atoi(fr) > 0) R = atoi(fr);
    }
    S.range_fastest = r_bal > r_fill;
    S.R = std::max(1, std::min(R, std::max(1, S.T)));   // range y = tiles [y T / R, (y + 1) T / R): none empty
    S.tiles_per_range = (S.T + S.R - 1) / S.R;
    // Tail split (round 4).  With enough column groups to fill the chip the range stays whole (R = 1), but the workgroups then
    // run in rounds of 256: config 3's H side has 1954 of them = 7.63 rounds -- the last round keeps 37 % of the CUs idle for a
    // whole workgroup's 74 tiles (4.6 % of the pass).  Only the workgroups of that last, partly filled round get their tile
    // range cut into tail_R pieces (dispatched last: blockIdx.x ascends), so that the pieces fill whole rounds of their own;
    // only their columns go through slabs.  Same cost model as above.
    S.tail_wg0 = -1;
    S.tail_R = 1;
    if (S.R == 1 && !S.range_fastest && nwg_x > 256 && S.T > 1 && E_est >= (double)(4ll << 20) && !getenv("SGL_TILED_NO_TAIL")) {
        const int64_t tail = nwg_x % 256;
        if (tail > 0) {
            const double t_tile = E_est / (double)nsl / ((double)nwg_x * (double)S.T) * 2.4e-9 + 2.5e-6;
            const double t_wg = 6e-6;
            const double tail_cols = (double)tail * TILED_NW * S.CW;
            double best = (double)S.T * t_tile + t_wg;   // left whole: one more round of full length
            int Rt = 1;
            for (int r = 2; r <= std::min<int64_t>(S.T, 16); ++r) {
                const double rounds = ceil((double)tail * r / 256.0);
                const double cost = rounds * ((double)((S.T + r - 1) / r) * t_tile + t_wg) + (double)r * (double)k * tail_cols * 16.0 / 4e12;
                if (cost < best * (1.0 - 1e-9)) { best = cost; Rt = r; }
            }
            if (Rt > 1) { S.tail_wg0 = nwg_x - tail; S.tail_R = Rt; }
        }
    }
    // segment starts per (row block, column); kept for the masked value array
    if (rc == SGL_OK) rc = t_reserve(&S.seg, &S.cap_seg, (size_t)(S.NB + 1) * (size_t)M.ncol);
    sgl_trace_setup("  stream: segment buffer reserved");
    DevCSC tmp = M;
    tmp.tile_rows = D;
    tmp.ntiles = S.NB;
    tmp.seg = S.seg;
    if (rc == SGL_OK) rc = k_build_segments(s, tmp);
    int64_t* chunk_entries = nullptr;
    if (rc == SGL_OK) rc = t_alloc(&chunk_entries, (size_t)nchunks);
    if (rc == SGL_OK) rc = t_reserve(&S.cnt, &S.cap_cnt, (size_t)nchunks * TILED_NP);
    if (rc == SGL_OK) rc = t_reserve(&S.ahead, &S.cap_ahead, (size_t)nchunks * (size_t)S.CW);
    if (rc == SGL_OK) rc = t_reserve(&S.cstart, &S.cap_cstart, (size_t)nchunks + 1);
    if (rc == SGL_OK && S.nwb > 0) {
        // one workgroup per (accumulate workgroup, tile range); a workgroup with fewer ranges than the grid has leaves the rest
        tiled_count_kernel<<<dim3((unsigned)nwg_x, (unsigned)std::max(S.R, S.tail_R)), dim3(64 * TILED_NW), 0, s>>>(
            S.seg, S.perm, M.ncol, S.T, S.NB, S.nwb, S.R, S.tail_wg0, S.tail_R, S.cnt, S.ahead, chunk_entries, nsl, balance ? 1 : 0);
        if (hipGetLastError() != hipSuccess) { sgl_set_error("tiled build: count kernel launch failed"); rc = SGL_EHIP; }
    }
    if (rc == SGL_OK) rc = k_exclusive_scan(c, chunk_entries, S.cstart, nchunks);
    if (rc == SGL_OK) rc = k_scan_total(s, chunk_entries, S.cstart, nchunks);
    int64_t E = 0;
    if (rc == SGL_OK) {
        if (hipMemcpyAsync(&E, S.cstart + nchunks, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { sgl_set_error("tiled build: reading the stream size failed"); rc = SGL_EHIP; }
    }
    S.E = E;
    sgl_trace_setup("  stream: segments, counts, scan");
    // + TILED_SLACK entries of slack: the kernel prefetches its ring (four or eight 64-entry sets) past the end
    if (rc == SGL_OK) rc = t_reserve(&S.roff, &S.cap_roff, (size_t)E + TILED_SLACK);
    if (rc == SGL_OK) rc = t_reserve(&S.x, &S.cap_x, (size_t)E + TILED_SLACK);
    sgl_trace_setup("  stream: roff / x buffers reserved");
    if (rc == SGL_OK) {
        if (hipMemsetAsync(S.roff + E, 0, TILED_SLACK * sizeof(uint32_t), s) != hipSuccess ||
            hipMemsetAsync(S.x + E, 0, TILED_SLACK * sizeof(double), s) != hipSuccess) { sgl_set_error("tiled build: clearing the stream slack failed"); rc = SGL_EHIP; }
    }
    if (rc == SGL_OK && nchunks > 0) {
        int64_t blocks = (nchunks + 3) / 4;
        if (blocks > 256 * 64) blocks = 256 * 64;
        tiled_fill_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(M.x, M.i, S.seg, S.perm, M.ncol, S.T, S.NB, S.nwb, S.R, S.tail_wg0,
                                                                       S.tail_R, D, KS * 8, S.cnt, S.ahead, S.cstart, S.roff, S.x,
                                                                       0, 0, sgl_div_make(1), 0, 0, 0, nsl);
        if (hipGetLastError() != hipSuccess) { sgl_set_error("tiled build: fill kernel launch failed"); rc = SGL_EHIP; }
    }
    // the chunk loop's schedule table: E / (4 nsl) groups + slack (a lap of 32 groups is loaded one ahead)
    const size_t ngroups = (size_t)(E / (4 * nsl));
    if (rc == SGL_OK) rc = t_reserve(&S.gtab, &S.cap_gtab, ngroups + 256);
    if (rc == SGL_OK) {
        if (hipMemsetAsync(S.gtab + ngroups, 0, 256 * sizeof(uint16_t), s) != hipSuccess) { sgl_set_error("tiled build: clearing the schedule slack failed"); rc = SGL_EHIP; }
    }
    if (rc == SGL_OK && nchunks > 0) {
        int64_t blocks = (nchunks + 3) / 4;
        if (blocks > 256 * 64) blocks = 256 * 64;
        tiled_gtab_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(S.cnt, S.cstart, nchunks, nsl, S.gtab);
        if (hipGetLastError() != hipSuccess) { sgl_set_error("tiled build: schedule kernel launch failed"); rc = SGL_EHIP; }
    }
    if (rc == SGL_OK && S.R > 1) rc = t_reserve(&S.part, &S.cap_part, (size_t)S.R * (size_t)k * (size_t)M.ncol);
    if (rc == SGL_OK && S.tail_R > 1)
        rc = t_reserve(&S.part, &S.cap_part, (size_t)S.tail_R * (size_t)k * (size_t)((nwg_x - S.tail_wg0) * TILED_NW * S.CW));
    hipError_t e = hipStreamSynchronize(s);
    if (chunk_entries) (void)sgl_pool_free(chunk_entries);
    if (rc == SGL_OK && e != hipSuccess) { sgl_set_error("tiled build failed: %s", hipGetErrorString(e)); rc = SGL_EHIP; }
    if (rc != SGL_OK) { sgl_tiled_free(S); return rc; }
    S.built = true;
    ++S.builds;
    return rc;
}

// ------------------------------------------------------- masked value array --
// The cross-validation mask of c_ard_nmf is fixed for a fit (seed, inv_density): predict_mask leaves the drawn
// entries out of the right-hand sides (src/singlet.cpp:449-457).  Instead of hashing every entry in every
// iteration (acc_kernel<MASK>), a second VALUE array of the entry stream is built once per fit with x = 0 at
// the drawn entries -- the tiled kernel then runs unchanged on it (a zero adds +0 * F: the sums are those of
// skipping the entry, as with the stream's pads).  8 B per stored entry on top of the 12.
// S.xm = the stream's value array for the mask (seed, inv_density); rebuilt only when the mask changes.  The hash
// runs inside the fill kernel (no temporary copy of the matrix values: at config-5 size that copy was a 12 GB
// allocation per fit and orientation).
int sgl_tiled_mask_values(sgl_ctx* c, const DevCSC& M, DevTiled& S, uint64_t seed, uint64_t inv_density, int mask_t,
                          int64_t col_off, int64_t row_off) {
    if (!S.built || !S.seg || !S.ahead) { sgl_set_error("masked values: no entry stream"); return SGL_ESTATE; }
    if (S.xm && S.xm_seed == seed && S.xm_inv == inv_density && S.xm_mask_t == mask_t) return SGL_OK;
    hipStream_t s = c->stream;
    S.xm_mask_t = -1;
    SGLCHK(t_reserve(&S.xm, &S.cap_xm, (size_t)S.E + TILED_SLACK));
    HIPCHK(hipMemsetAsync(S.xm + S.E, 0, TILED_SLACK * sizeof(double), s));
    const int64_t nchunks = S.nwb * S.NB;
    if (nchunks > 0) {
        const int KS = S.KS;
        int64_t blocks = (nchunks + 3) / 4;
        if (blocks > 256 * 64) blocks = 256 * 64;
        tiled_fill_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(M.x, M.i, S.seg, S.perm, M.ncol, S.T, S.NB, S.nwb, S.R, S.tail_wg0,
                                                                       S.tail_R, S.TR / 2, KS * 8, S.cnt, S.ahead, S.cstart, nullptr, S.xm,
                                                                       1, seed, sgl_div_make(inv_density), mask_t, col_off, row_off, S.NSL);
        HIPCHK(hipGetLastError());
    }
    S.xm_seed = seed; S.xm_inv = inv_density; S.xm_mask_t = mask_t;
    return SGL_OK;
}

// ---------------------------------------------------------------- kernel ----
// Broadcasting the (roff, x) of each entry to the 32 lanes that work on it is
// the VALU cost that decides this kernel: three v_readlane per non-zero cost
// ~30 cycles (measured: VALU-bound at 35 cyc/nz/SIMD).  Instead the 16-lane
// ROWS of the wave hold 16 entries each -- rows 0,1 the same 16 entries of the A
// half, rows 2,3 sixteen of the B half -- and DPP row_newbcast:j (the only DPP
// mode gfx950 allows on FP64 ALU ops) feeds entry j to all lanes of its rows
// inside the consuming instruction itself:
//     v_add_u32_dpp  addr, roff, lane16        row_newbcast:j   (LDS address)
//     ds_read_b128   w, addr                                   (F[2l, 2l+1 ; row])
//     v_fmac_f64_dpp acc0, x, w.x              row_newbcast:j   (acc += x_j * w)
//     v_fmac_f64_dpp acc1, x, w.y              row_newbcast:j
// The stream ring loads each half of a 64-entry set straight into that
// layout: lanes 0-15 and 16-31 read the same 16 entries of the A half, lanes
// 32-47 and 48-63 the same 16 of the B half (two 16-pair batches per set).
//
// Register plan.  The 32 pairs x 2 FP64 accumulators of a wave live in v[128:255], OUTSIDE the compiler's register
// allocation, and are updated IN PLACE: VGPR index mode is on inside the chunk loop and M0 (destination-relative,
// 0x8000 | 4 * pair) selects the running pair's registers for the FMAs (gen_acc_tiled.py).  Letting hipcc index
// a register array dynamically was tried first: it either moved the array to scratch memory or copied whole
// 32-register vectors around every slot change.  (Rounds 1 - 2 ran the loop as compiler-scheduled C++ with the
// running pair swapped in and out of fixed registers: same arithmetic, 6 % slower; see DESIGN.md.)
//
// Eight ring slots of the stream are in flight per wave, each refilled once its last operand has been read and waited
// with a counted vmcnt (loads return in order); which ring slot is next is the wave-uniform `phase`.

// accumulators of pair p -> (v0, v1), for the output stage
__device__ __forceinline__ void acc_load(int idx4, double& v0, double& v1) {
    int a, b, c, d;
    asm volatile(
        "s_set_gpr_idx_on %4, gpr_idx(SRC0)\n\tv_mov_b32 %0, v128\n\tv_mov_b32 %1, v129\n\tv_mov_b32 %2, v130\n\t"
        "v_mov_b32 %3, v131\n\ts_set_gpr_idx_off"
        : "=v"(a), "=v"(b), "=v"(c), "=v"(d) : "s"(idx4) : "memory");
    v0 = __hiloint2double(b, a);
    v1 = __hiloint2double(d, c);
}

#include "acc_tiled_gen.inc"

// Stage `rows` rows of F (first row src, row stride ldf) into the LDS ring slot at `tile` (row stride KS doubles; 32 in the quad
// layout).  sync: the workgroup barrier between the first round's loads and the writes -- every wave is done with what the
// slot held before (the loads in front of it overlap the tail of the other waves' chunk).
template <int NSL>
__device__ __forceinline__ void tiled_stage(double* __restrict__ tile, const double* __restrict__ src, int rows, int k, int KS, int ldf,
                                            bool sync) {
    const int n = rows * k;
    if constexpr (NSL == 4) {
        // Quad layout: LDS rows of 32 doubles.  16 lanes per tile row (lane c moves the 16-byte piece c, or -- odd
        // rank / unaligned rows -- the doubles c and c + 16), 32 rows per round of the workgroup: no divisions, every
        // row's k * 8 contiguous bytes read by neighbouring lanes.  First round's loads before the barrier.
        const int c16 = (int)threadIdx.x & 15, r0 = (int)threadIdx.x >> 4;
        constexpr int RPR = 64 * TILED_NW / 16;   // rows per round
        const bool vec = ((k | ldf) & 1) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
        if (vec) {
            constexpr int RST = 4;
            double2 stg[RST];
            const bool cact = 2 * c16 < k;
#pragma unroll
            for (int j = 0; j < RST; ++j) {
                const int r = r0 + j * RPR;
                stg[j] = double2{0.0, 0.0};
                if (cact && r < rows) stg[j] = *reinterpret_cast<const double2*>(src + (int64_t)r * ldf + 2 * c16);
            }
            if (sync) __syncthreads();  // everyone is done with what the slot held
            for (int rb = 0; rb < rows; rb += RST * RPR) {
#pragma unroll
                for (int j = 0; j < RST; ++j) {
                    const int r = rb + r0 + j * RPR;
                    if (cact && r < rows) *reinterpret_cast<double2*>(tile + r * 32 + 2 * c16) = stg[j];
                }
                if (rb + RST * RPR < rows) {
#pragma unroll
                    for (int j = 0; j < RST; ++j) {
                        const int r = rb + RST * RPR + r0 + j * RPR;
                        stg[j] = double2{0.0, 0.0};
                        if (cact && r < rows) stg[j] = *reinterpret_cast<const double2*>(src + (int64_t)r * ldf + 2 * c16);
                    }
                }
            }
        } else {
            if (sync) __syncthreads();
            for (int r = r0; r < rows; r += RPR) {
                if (c16 < k) tile[r * 32 + c16] = src[(int64_t)r * ldf + c16];
                if (c16 + 16 < k) tile[r * 32 + c16 + 16] = src[(int64_t)r * ldf + c16 + 16];
            }
        }
    } else {
        // (pair layout with KS == k == ldf: tiled_issue / tiled_commit below, from the stage loop of acc_tiled_kernel)
        // odd k: rows are re-pitched to KS = k + 1 doubles (the pad column is never summed into a
        // stored factor row: lane 2l+1 == k is not written out)
        if (sync) __syncthreads();
        // (also the path of a rank split into parts: rows of F are then ldf > k apart)
        if (((k | ldf) & 1) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const int hp = k >> 1;  // 16-byte pieces per row
            for (int e = (int)threadIdx.x; e < rows * hp; e += 64 * TILED_NW) {
                const int r = e / hp, c2 = (e - r * hp) * 2;
                *reinterpret_cast<double2*>(tile + r * KS + c2) = *reinterpret_cast<const double2*>(src + (int64_t)r * ldf + c2);
            }
        } else {
            for (int e = (int)threadIdx.x; e < n; e += 64 * TILED_NW) {
                const int r = e / k, f = e - r * k;
                tile[r * KS + f] = src[(int64_t)r * ldf + f];
            }
        }
        if (KS != k)
            for (int r = (int)threadIdx.x; r < rows; r += 64 * TILED_NW) tile[r * KS + k] = 0.0;
    }
}

// Pair layout with KS == k == ldf (even ranks 34 - 64: both passes of config 3).  A row block is n = rows * k contiguous
// doubles, moved by the workgroup as 16-byte pieces: piece j of thread t is doubles 2 (t + 512 j), 2 (t + 512 j) + 1, so a
// ring slot (at most TILED_LDS_BYTES / 2 bytes) is at most TILED_PIECES pieces per thread -- 40 registers.
// The stage loop splits the move in two: tiled_issue loads a thread's pieces of block b + 2 into registers BEFORE the chunk
// of stage b (the last reader of the slot the block goes to), and they stay in flight while it runs; tiled_commit writes them
// into the slot between the two barriers after it.  Both are inline asm, because hipcc cannot count these loads right: the
// chunk issues ring refills behind them (loads the compiler does not see), and its own wait before the writes -- vmcnt(9 - j)
// for piece j -- would drain the ring's refills at every edge.  Loads retire in issue order: after a chunk of s >= 4 sets the
// chunk's refills (two loads per half-set slot: 4 s >= 16) are all younger than the pieces, so vmcnt(16) covers every piece
// and leaves a whole ring lap in flight; after a shorter chunk (or none) vmcnt(0).  (The chunk's own counted ring waits stay
// correct with the pieces in flight: older loads only make them wait longer.)
// Every piece is loaded (a piece past the block reads the block's last one, clamped), so the count is static; the writes of
// pieces past the block are masked off.
#define TILED_PIECES 10
static_assert(TILED_PIECES * 64 * TILED_NW * 16 >= TILED_LDS_BYTES / 2, "the pieces must cover a whole ring slot");
// The pieces sit in v[24:63] from the issue to the commit, OUTSIDE hipcc's allocation (acc_tiled_kernel<2> caps it at v0..v23):
// hipcc must never copy, spill or reuse a register whose load is still in flight, and it cannot know that it is.
#define TILED_PIECE_CLOBBERS "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", \
    "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", \
    "v58", "v59", "v60", "v61", "v62", "v63"

#define TILED_ISSUE_PIECE(regs, off) \
    "v_add_u32 %[t], " off ", %[o]\n\tv_min_u32 %[t], %[last], %[t]\n\tglobal_load_dwordx4 " regs ", %[t], %[src]\n\t"

// thread's pieces of the block at src (n doubles, 16-byte aligned) -> v[24:63]; returns at once
__device__ __forceinline__ void tiled_issue(const double* src, int n) {
    static_assert(TILED_PIECES == 10, "tiled_issue / tiled_commit move ten pieces");
    const unsigned o = threadIdx.x * 16u, last = (unsigned)n * 8u - 16u;
    unsigned t;
    asm volatile(
        "v_min_u32 %[t], %[last], %[o]\n\tglobal_load_dwordx4 v[24:27], %[t], %[src]\n\t"
        TILED_ISSUE_PIECE("v[28:31]", "0x2000") TILED_ISSUE_PIECE("v[32:35]", "0x4000") TILED_ISSUE_PIECE("v[36:39]", "0x6000")
        TILED_ISSUE_PIECE("v[40:43]", "0x8000") TILED_ISSUE_PIECE("v[44:47]", "0xa000") TILED_ISSUE_PIECE("v[48:51]", "0xc000")
        TILED_ISSUE_PIECE("v[52:55]", "0xe000") TILED_ISSUE_PIECE("v[56:59]", "0x10000") TILED_ISSUE_PIECE("v[60:63]", "0x12000")
        : [t] "=&v"(t)
        : [o] "v"(o), [last] "s"(last), [src] "s"(src)
        : TILED_PIECE_CLOBBERS);
}

// piece j at LDS byte a (+ 8192 j; past the 16-bit offset field from a1 = a + 65536) if a + 8192 j < lim, else masked off
#define TILED_COMMIT_PIECE(regs, addr, off) \
    "v_cmp_gt_i32 vcc, %[lim], %[a]\n\ts_and_b64 exec, exec, vcc\n\tds_write_b128 " addr ", " regs off "\n\ts_sub_i32 %[lim], %[lim], 0x2000\n\t"
#define TILED_COMMIT_ASM(wait) \
    "s_waitcnt vmcnt(" wait ")\n\ts_mov_b64 %[sv], exec\n\t" \
    TILED_COMMIT_PIECE("v[24:27]", "%[a]", "") TILED_COMMIT_PIECE("v[28:31]", "%[a]", " offset:8192") \
    TILED_COMMIT_PIECE("v[32:35]", "%[a]", " offset:16384") TILED_COMMIT_PIECE("v[36:39]", "%[a]", " offset:24576") \
    TILED_COMMIT_PIECE("v[40:43]", "%[a]", " offset:32768") TILED_COMMIT_PIECE("v[44:47]", "%[a]", " offset:40960") \
    TILED_COMMIT_PIECE("v[48:51]", "%[a]", " offset:49152") TILED_COMMIT_PIECE("v[52:55]", "%[a]", " offset:57344") \
    TILED_COMMIT_PIECE("v[56:59]", "%[a1]", "") TILED_COMMIT_PIECE("v[60:63]", "%[a1]", " offset:8192") \
    "s_mov_b64 exec, %[sv]\n\ts_waitcnt lgkmcnt(0)"
#define TILED_COMMIT_OPERANDS : [sv] "=&s"(sv), [lim] "+s"(lim) : [a] "v"(a), [a1] "v"(a + 65536u) : "vcc", "scc", "memory"

// v[24:63] -> the ring slot at tile (n doubles of the block); the LDS writes have landed on return.  ring_after: a chunk of at
// least four sets ran since tiled_issue (above)
__device__ __forceinline__ void tiled_commit(double* tile, int n, bool ring_after) {
    typedef __attribute__((address_space(3))) char lds_char;
    const unsigned base = (unsigned)(uintptr_t)(lds_char*)tile;
    const unsigned a = base + threadIdx.x * 16u;
    int lim = (int)(base + (unsigned)n * 8u);
    uint64_t sv;
    if (ring_after)
        asm volatile(TILED_COMMIT_ASM("16") TILED_COMMIT_OPERANDS);
    else
        asm volatile(TILED_COMMIT_ASM("0") TILED_COMMIT_OPERANDS);
}

// The chunk loop is the hand-scheduled inline asm of gen_acc_tiled.py (register plan there).  The compiler's budget
// is v0..v63 (amdgpu_waves_per_eu(8, 8) caps its allocation at 512 / 8 registers); the clobber makes the kernel
// descriptor allocate all 256: v64..v255 belong to the asm, whose stream ring stays in flight across compiler code.
// The pair instance gives hipcc v0..v23 only: v24..v63 hold tiled_issue's pieces across the chunk.
// NSL = 2: pairs of columns on half-set ring slots loaded with doubled lane rows (parts of 33 - 64 factors);  NSL = 4: quads
// of columns (parts up to 32).  Both walk the schedule table gtab.
#define ACC_TILED_PARAMS                                                                                                          \
    const uint32_t* __restrict__ sroff, const double* __restrict__ sx, const int64_t* __restrict__ cstart,                            \
        const uint8_t* __restrict__ cnt, int T, int NB, int64_t nwb, const double* __restrict__ F, int k, int TR, int64_t nrow,       \
        int tiles_per_range, double* __restrict__ Bout, int64_t ncol, int KS, int ldf, int ldb, int64_t slab,                        \
        const int32_t* __restrict__ perm, int range_fastest, const uint16_t* __restrict__ gtab, int tail_wg0, int tail_R,            \
        double* __restrict__ tail_part, int64_t tail_slab
#define ACC_TILED_ARGS \
    sroff, sx, cstart, cnt, T, NB, nwb, F, k, TR, nrow, tiles_per_range, Bout, ncol, KS, ldf, ldb, slab, perm, range_fastest, gtab, \
        tail_wg0, tail_R, tail_part, tail_slab
template <int NSL>
__device__ __forceinline__ void acc_tiled_body(ACC_TILED_PARAMS) {
    // k = factor rows handled by this launch (a part of the rank when it is above 64), KS = LDS row
    // stride the stream's offsets were built for, ldf / ldb = strides (doubles) between rows of F /
    // columns of the output, slab = doubles between the outputs of two tile ranges (blockIdx.y).
    // cnt is unused (gtab carries the schedule); it stays because dropping it reorders the pair instance's scalar code.
    asm volatile("" ::: "v255");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* tile = reinterpret_cast<double*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // work units in the order (column group, tile range), the range running fastest: the column groups come heaviest
    // first (sorted columns), so the longest units are dispatched first whatever the number of ranges
    // (only when the split was sized by that imbalance: otherwise the column groups run fastest, so that the
    // workgroups resident on one XCD stage the SAME factor tiles at about the same time and share them in its L2)
    unsigned bx = blockIdx.x, by = blockIdx.y;
    if (range_fastest) {
        const unsigned unit = blockIdx.x + gridDim.x * blockIdx.y, nranges = gridDim.y;
        bx = unit / nranges;
        by = unit - bx * nranges;
    }
    // tail split: the workgroups of the last, partly filled round of 256 come as tail_R pieces each (x = tail_wg0 + u)
    unsigned nry = gridDim.y;
    bool tail_piece = false;
    if (tail_R > 1 && (int)bx >= tail_wg0) {
        const unsigned u = bx - (unsigned)tail_wg0;
        bx = (unsigned)tail_wg0 + u / (unsigned)tail_R;
        by = u % (unsigned)tail_R;
        nry = (unsigned)tail_R;
        tail_piece = true;
    }
    const int64_t wb = (int64_t)bx * TILED_NW + wave;
    // tile range `by` of nry: sizes floor / ceil of T / ranges (tiles_per_range = the ceil, kept for the layout query)
    const int t0 = (int)(((int64_t)by * T) / nry);
    const int t1 = (int)((((int64_t)by + 1) * T) / nry);
    // its stages: row blocks [b0, b1) of D = TR / 2 rows; block j of F sits in LDS ring slot j & 1
    const int D = TR >> 1;
    const int b0 = 2 * t0, b1 = 2 * t1 < NB ? 2 * t1 : NB;
    const bool wact = wb < nwb;
    typedef __attribute__((address_space(3))) char lds_char;
    // LDS byte address of this lane's pair of factor rows inside a tile row (NSL = 4: 16 lanes cover a column)
    constexpr int LMASK = NSL == 4 ? 15 : 31;
    const unsigned lane16 = (unsigned)(uintptr_t)(lds_char*)smem + (lane & LMASK) * 16;
    // stream slot this lane loads of a (half) set.  NSL = 2: lane rows doubled -- lanes 0-15 and 16-31 the A half's 16
    // entries, lanes 32-47 and 48-63 the B half's (slots 32 ..): the [A A B B] layout the row broadcasts read
    const unsigned slot = NSL == 2 ? (unsigned)((lane >> 5) * 32 + (lane & 15)) : (unsigned)lane;
    const unsigned voff4 = slot * 4, voff8 = slot * 8;
    // L2 prefetch of the stream (gen_acc_tiled.py, GenTab.wrap): lane offset into the row-offset stream that spreads the 64
    // lanes over one lap of it (8 ring slots: 1 KB in the pair layout, 2 KB in the quad layout), ACC_TILED_PF_LAPS laps ahead
    constexpr unsigned LAP_R = (NSL == 4 ? 256u : 128u) * 8u;
    const unsigned pfl = (unsigned)lane * (LAP_R / 64u) + (unsigned)ACC_TILED_PF_LAPS * LAP_R;

    asm volatile(ACC_TILED_ZERO_ASM ::: "memory");

    uint64_t rp = 0, xp = 0;   // next 64-entry set to LOAD (row offsets / values)
    int phase = 0;
    // start of the next chunk, read on the scalar side one stage ahead: wb is wave-uniform
    int64_t pos_next = 0;
    if (wact) {
        const int64_t pos = cstart[wb * NB + b0];
        pos_next = cstart[wb * NB + b0 + 1];
        const uint64_t r_ = reinterpret_cast<uint64_t>(sroff + pos), x_ = reinterpret_cast<uint64_t>(sx + pos);
        rp = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)(r_ >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((unsigned)r_);
        xp = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)(x_ >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((unsigned)x_);
        if constexpr (NSL == 4)
            asm volatile(ACC_TILED4_RING_FILL_ASM : [rp] "+s"(rp), [xp] "+s"(xp) : [voff4] "v"(voff4), [voff8] "v"(voff8) : ACC_TILED_CLOBBERS);
        else
            asm volatile(ACC_TILED2_RING_FILL_ASM : [rp] "+s"(rp), [xp] "+s"(xp) : [voff4] "v"(voff4), [voff8] "v"(voff8) : ACC_TILED_CLOBBERS);
    }
    if constexpr (NSL == 4) {
        // the tile rows are 256 B apart whatever the rank: bytes k * 8 .. 255 of a row are never staged; clear them
        // once (they only ever reach accumulator lanes that are not written out, but must stay finite: 0 * NaN)
        for (int e = (int)threadIdx.x; e < TILED_LDS_BYTES / 8; e += 64 * TILED_NW) tile[e] = 0.0;
    }

    // pair layout, rows of F contiguous: block b + 2 is loaded while the chunk of stage b runs (tiled_issue)
    const bool pf = NSL == 2 && KS == k && ldf == k;
    auto block_rows = [&](int j) { const int64_t row0 = (int64_t)j * D; return (int)(nrow - row0 < D ? nrow - row0 : D); };
    int64_t pos_cur = wact ? cstart[wb * NB + b0] : 0;
    for (int b = b0; b < b1; ++b) {
        const int nsets = (int)((pos_next - pos_cur) >> 6);  // 64-entry sets (32 per half) of this chunk
        const int64_t pos_chunk = pos_cur;                   // its first entry
        pos_cur = pos_next;
        if (wact && b + 1 < b1) pos_next = cstart[wb * NB + b + 2];

        // stage b reads blocks b and b + 1: the range's first stage stages both, every later one block b + 1 into the slot
        // block b - 1 held (the chunk of stage b - 1 was its last reader)
        if (pf) {
            if (b == b0) {
#pragma clang loop unroll(disable)
                for (int j = b; j <= b + 1 && j < b1; ++j) {
                    tiled_issue(F + (int64_t)j * D * ldf, block_rows(j) * k);
                    tiled_commit(tile + (j & 1) * D * KS, block_rows(j) * k, false);
                }
                __syncthreads();
            }
            if (b + 2 < b1) tiled_issue(F + (int64_t)(b + 2) * D * ldf, block_rows(b + 2) * k);
        } else {
            // (one call site: the staging's registers come out of the compiler's budget)
#pragma clang loop unroll(disable)
            for (int j = b == b0 ? b : b + 1; j <= b + 1 && j < b1; ++j) {
                const int64_t row0 = (int64_t)j * D;
                tiled_stage<NSL>(tile + (j & 1) * D * KS, F + row0 * ldf, block_rows(j), k, KS, ldf, j == b || b != b0);
            }
            // all staging loads (and the ring loads in front of them) have landed: the asm's counted vmcnt waits see
            // only its own ring loads in flight.  (The range's last stage stages nothing: its blocks landed behind the
            // barrier of the stage before.)
            if (b == b0 || b + 1 < b1) {
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
                __syncthreads();
            }
        }
        if (wact && nsets > 0) {
            // first schedule word of this chunk (wave-uniform address)
            const uint64_t t_ = reinterpret_cast<uint64_t>(gtab + pos_chunk / (4 * NSL));
            const uint64_t tp = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)(t_ >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((unsigned)t_);
            if constexpr (NSL == 2)
                asm volatile(ACC_TILED2_CHUNK_ASM
                             : [rp] "+s"(rp), [xp] "+s"(xp), [phase] "+s"(phase)
                             : [ns] "s"(2 * nsets), [tp] "s"(tp), [lane16] "v"(lane16), [voff4] "v"(voff4), [voff8] "v"(voff8), [pfl] "v"(pfl)
                             : ACC_TILED_CHUNK_CLOBBERS);
            else
                asm volatile(ACC_TILED4_CHUNK_ASM
                             : [rp] "+s"(rp), [xp] "+s"(xp), [phase] "+s"(phase)
                             : [ns] "s"(nsets), [tp] "s"(tp), [lane16] "v"(lane16), [voff4] "v"(voff4), [voff8] "v"(voff8), [pfl] "v"(pfl)
                             : ACC_TILED_CHUNK_CLOBBERS);
        }
        if (pf && b + 2 < b1) {
            __syncthreads();   // every wave is done with block b: its slot takes block b + 2
            tiled_commit(tile + (b & 1) * D * KS, block_rows(b + 2) * k, wact && nsets >= 4);
            __syncthreads();
        }
    }
    // Up to eight refills (issued past the end of this wave's range, into the stream's slack) are still in flight;
    // they write the ring registers v64..v87 only, which nothing below touches
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (wact) {
        double* out = Bout + (size_t)by * (size_t)slab;
        const int f = 2 * (lane & LMASK);
        const int64_t tail_pos0 = (int64_t)tail_wg0 * TILED_NW * (TILED_NP * NSL);
        for (int p = 0; p < TILED_NP; ++p) {
            double v0, v1;
            acc_load(4 * p, v0, v1);
            const int h = NSL == 4 ? (lane >> 4) : (lane >> 5);
            const int64_t col = tiled_slot_col(perm, ncol, wb, h, p, NSL);
            if (col >= 0) {
                if (tail_piece) {   // compact slab of this piece, indexed by the column's position in the stream's order
                    const int64_t pos = wb * (TILED_NP * NSL) + NSL * p + h;
                    double* o = tail_part + (size_t)by * (size_t)tail_slab + (pos - tail_pos0) * k;
                    if (f < k) o[f] = v0;
                    if (f + 1 < k) o[f + 1] = v1;
                } else {
                    if (f < k) out[col * ldb + f] = v0;
                    if (f + 1 < k) out[col * ldb + f + 1] = v1;
                }
            }
        }
    }
}

template <int NSL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) void acc_tiled_kernel(ACC_TILED_PARAMS) {
    acc_tiled_body<NSL>(ACC_TILED_ARGS);
}
// the pair instance: v24..v63 hold tiled_issue's pieces across the chunk, hipcc gets v0..v23.  (On gfx950 amdgpu_num_vgpr counts
// the unified register file, arch + accumulation registers: 12 here caps the arch registers at 24.)
template <>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8), amdgpu_num_vgpr(12))) void acc_tiled_kernel<2>(ACC_TILED_PARAMS) {
    acc_tiled_body<2>(ACC_TILED_ARGS);
}

// B[col * ldb + f] = sum over the R tile-range slabs (compact k x ncol each, fixed order)
__global__ void acc_tiled_reduce_kernel(const double* __restrict__ part, int R, int64_t n, int k, int ldb, double* __restrict__ B) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        double s = part[e];
        for (int r = 1; r < R; ++r) s += part[(size_t)r * n + e];
        if (ldb == k) {
            B[e] = s;
        } else {
            const int64_t col = e / k;
            B[col * ldb + (e - col * k)] = s;
        }
    }
}

// tail split: B[col(pos) * ldb + f] = sum over the pieces' compact slabs, in piece order, for the stream positions pos >= pos0
__global__ void acc_tiled_reduce_tail_kernel(const double* __restrict__ part, int R, int64_t slab, int64_t pos0, int64_t ncol,
                                             const int32_t* __restrict__ perm, int k, int ldb, double* __restrict__ B) {
    const int64_t n = (ncol - pos0) * k;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        double s = part[e];
        for (int r = 1; r < R; ++r) s += part[(size_t)r * slab + e];
        const int64_t q = e / k;
        const int64_t col = perm ? (int64_t)perm[pos0 + q] : pos0 + q;
        B[col * ldb + (e - q * k)] = s;
    }
}

// F: first factor row of this part (row stride ldf), B: its first output row (column stride ldb), kf <= S.k
// factor rows.  One launch = one pass over the stream.
int k_acc_tiled(hipStream_t s, const DevTiled& S, const double* F, int ldf, double* B, int ldb, int kf, const double* xvals) {
    if (S.ncol <= 0) return SGL_OK;
    if (kf <= 0 || kf > S.k) { sgl_set_error("k_acc_tiled: bad part size %d (stream built for %d)", kf, S.k); return SGL_EINVAL; }
    const int KS = S.KS;
    const size_t lds = S.NSL == 4 ? (size_t)TILED_LDS_BYTES + 512 : (size_t)S.TR * KS * 8 + 512;
    SGLCHK(sgl_allow_dynamic_lds<&acc_tiled_kernel<2>>(TILED_LDS_BYTES + 512));
    SGLCHK(sgl_allow_dynamic_lds<&acc_tiled_kernel<4>>(TILED_LDS_BYTES + 512));
    const int64_t nwg_x = (S.nwb + TILED_NW - 1) / TILED_NW;
    const bool slabs = S.R > 1;
    double* out = slabs ? S.part : B;
    const int64_t n = (int64_t)kf * S.ncol;
    const bool tail = !slabs && S.tail_R > 1 && S.tail_wg0 >= 0;
    const int64_t tail_cols = tail ? (nwg_x - S.tail_wg0) * TILED_NW * S.CW : 0;
    const int64_t tail_slab = tail_cols * kf;
    const dim3 grid(tail ? (unsigned)(S.tail_wg0 + (nwg_x - S.tail_wg0) * S.tail_R) : (unsigned)nwg_x, (unsigned)S.R);
    auto launch = [&](auto nsl) {
        acc_tiled_kernel<decltype(nsl)::value><<<grid, dim3(64 * TILED_NW), lds, s>>>(
            S.roff, xvals ? xvals : S.x, S.cstart, S.cnt, S.T, S.NB, S.nwb, F, kf, S.TR, S.nrow, S.tiles_per_range, out, S.ncol, KS, ldf,
            slabs ? kf : ldb, slabs ? n : 0, S.perm, S.range_fastest ? 1 : 0, S.gtab, tail ? (int)S.tail_wg0 : -1, tail ? S.tail_R : 1,
            S.part, tail_slab);
    };
    if (S.NSL == 4) launch(std::integral_constant<int, 4>());
    else launch(std::integral_constant<int, 2>());
    HIPCHK(hipGetLastError());
    if (tail) {
        const int64_t pos0 = S.tail_wg0 * TILED_NW * S.CW;
        const int64_t ne = (S.ncol - pos0) * kf;
        if (ne > 0) {
            int64_t blocks = (ne + 255) / 256;
            if (blocks > 4096) blocks = 4096;
            acc_tiled_reduce_tail_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(S.part, S.tail_R, tail_slab, pos0, S.ncol, S.perm, kf, ldb, B);
            HIPCHK(hipGetLastError());
        }
    }
    if (slabs) {
        int64_t blocks = (n + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        acc_tiled_reduce_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(S.part, S.R, n, kf, ldb, B);
        HIPCHK(hipGetLastError());
    }
    return SGL_OK;
}

// the whole rank: one pass per part of at most S.k factor rows (one part for k <= 64)
int k_acc_tiled_all(hipStream_t s, const DevTiled& S, const double* F, double* B, int k, const double* xvals) {
    for (int f0 = 0; f0 < k; f0 += S.k) {
        const int kf = (k - f0 < S.k) ? (k - f0) : S.k;
        SGLCHK(k_acc_tiled(s, S, F + f0, k, B + f0, k, kf, xvals));
    }
    return SGL_OK;
}

// part size the entry streams are built for at rank k (0: no tiled path): even, at most 64.  A pass costs the same whatever its
// part size within a layout (one address add, one ds_read_b128, two FMAs per entry tuple), and the quad layout of parts up to 32
// serves FOUR columns per tuple where the pair layout serves two: ranks 65 - 96 run as THREE quad passes (1.5 x the cost of a
// k = 64 pass) instead of two pair passes (2 x); 97 - 128 as FOUR quad passes (2.0 x the k = 64 pass; the two pair passes measure
// 2.4 x -- rhs_h per 200 000 cells at k = 100: 5.84 -> 4.89 ms, k = 128: 6.48 -> 5.01; profiles/r5_k_sweep_200k_cells.txt).
// One pass over half-height tiles with four factors per lane was priced and loses: 15 % more LDS time than the two passes
// (scripts/r5/r5_pad_model.py).
// Round 6: ranks above 128 too -- ceil(k / 32) quad passes over the same stream (the reference's nnls / predict have no rank
// limit, src/singlet.cpp:229-250, and RunNMF hands ard_nmf k_max = 1e4, R/RunNMF.R:131); until then they fell to the plain
// wave-per-column gather (acc_kernel).
int tiled_part_size(int k) {
    if (k <= 64) return k;
    if (k > SGL_MAX_K) return 0;
    const bool quad = !getenv("SGL_TILED_NO_QUAD");
    const int parts = quad ? (k <= 96 ? 3 : (k + 31) / 32) : (k + 63) / 64;
    return ((k + parts - 1) / parts + 1) & ~1;
}
