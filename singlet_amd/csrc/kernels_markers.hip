// Marker genes of every cluster (include/singlet_hip.h, "Marker genes"): the one-vs-rest Wilcoxon rank-sum test of every gene
// against every cluster from ONE ordering of the gene's values, and the group sums of the fold change.  All passes read the
// gene-side image t(A) (one column per gene, 64-bit offsets) and the label of the cell of every stored entry.  This file holds
//   1. mk_sums_kernel<TRANSFORM> / mk_sums_finish_kernel: ONE WAVE PER SEGMENT of MARKERS_SEG stored entries.  A block of 64
//      consecutive entries is reduced once per label present in it (ballots pick the labels): the 64 lane values, +0.0 for a
//      non-member, go through the butterfly (lane ^ 32, 16, ... 1) and the block partial is added to the cluster's segment sum,
//      which lane (c & 63) keeps in LDS next to the packed counts of x > 0 and x != 0.  The finish kernel adds a gene's
//      segment sums in ascending order from +0.0.  The counts leave through integer atomics, one per (segment, cluster).
//   2. mk_count_kernel: the included non-zero entries of every gene (integer atomics), which decide its rank path.
//   3. mk_rank_lds_kernel: one workgroup per short gene: the (key, label) pairs of its included non-zero entries are
//      gathered into LDS, sorted there (bitonic), and walked.
//   4. mk_fill_kernel / hipcub's segmented radix sort / mk_rank_walk_kernel: the long genes in batches through scratch.
//   The walk (mk_walk) is shared: a forward pass gives every position its run start a (max-scan over run heads), a backward
//   pass its run end b (min-scan), in chunks of MARKERS_WALK with a and b carried across chunk edges; a + [b + 1] is added to
//   the label's 64-bit counter in LDS, t^3 - t is taken at run heads.  The zero block is closed in the same kernel.
// The statistic is all integers: no tiling, batching or order of the atomics can change a bit of it.  Only the group sums
// are floating point; their order is stated, there is no floating-point atomic, no loop whose trip count follows the launch
// size, and the unit is compiled with -ffp-contract=off.  tests/markers_restatement.py restates all of it in numpy.
#include "sgl_internal.h"
#include "markers_host.h"

#include <hipcub/hipcub.hpp>
#include <climits>
#include <cmath>

#define MK_THREADS 256
#define MK_WAVES (MK_THREADS / SGL_WAVE)
#define MK_PER_THREAD (MARKERS_WALK / MK_THREADS)
#define MK_SUMS_SCRATCH ((int64_t)256 << 20)   // bytes of segment partials per batch of the sums pass
static_assert(MARKERS_WALK % MK_THREADS == 0, "a walk chunk is whole rounds of the workgroup");
static_assert(MARKERS_SEG < 65536, "the packed counts of a segment hold 16 bits each");
static_assert((MARKERS_LDS_CAP & (MARKERS_LDS_CAP - 1)) == 0 && MARKERS_LDS_CAP >= MK_THREADS, "capacity: a power of two");
static_assert(MARKERS_LDS_CAP * 12 + MARKERS_MAX_GROUPS * 12 + 1024 <= 64 * 1024, "the LDS sort stays below 64 KiB: no launch attribute");
static_assert(MK_WAVES * MARKERS_MAX_GROUPS * 12 <= 64 * 1024, "the segment sums of four waves stay below 64 KiB");

typedef unsigned long long mk_u64;

// v of lane ^ 8, 2, 1 through one DPP move per half (row_ror:8 and the two quad permutations are those exchanges exactly)
template <int CTRL>
__device__ __forceinline__ double mk_dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// v of lane ^ 4: the lanes 0-3 and 8-11 of a row take lane + 4 (row_shl:4 under bank mask 0101), the others lane - 4
__device__ __forceinline__ int mk_dpp_xor4(int x) {
    int t = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);
    return __builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);
}
// The butterfly of the stated order (lane ^ 32, 16, 8, 4, 2, 1), every lane ending with the sum: the two steps that cross
// rows of 16 lanes go through the LDS crossbar, the four inside a row are DPP moves.  All 64 lanes must be active.
__device__ __forceinline__ double mk_wave_sum(double v) {
    v += __shfl_xor(v, 32, SGL_WAVE);
    v += __shfl_xor(v, 16, SGL_WAVE);
    v += mk_dpp_f64<0x128>(v);
    v += __hiloint2double(mk_dpp_xor4(__double2hiint(v)), mk_dpp_xor4(__double2loint(v)));
    v += mk_dpp_f64<0x4E>(v);
    v += mk_dpp_f64<0xB1>(v);
    return v;
}

// order-preserving image of a finite non-zero double: negatives below 2^63 ascending, positives above
__device__ __forceinline__ mk_u64 mk_key(double x) {
    const mk_u64 u = (mk_u64)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// ---- 1. group sums --------------------------------------------------------------------------------------------------------
template <int TRANSFORM>
__global__ __launch_bounds__(MK_THREADS) void mk_sums_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                            const int64_t* __restrict__ p, const int32_t* __restrict__ lab,
                                                            const int32_t* __restrict__ seg_gene, const int64_t* __restrict__ seg_first,
                                                            int64_t seg0, int64_t nseg, int32_t G, int64_t m, double* __restrict__ part,
                                                            mk_u64* __restrict__ pos, mk_u64* __restrict__ nz) {
    extern __shared__ double mk_lds[];
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t sl = (int64_t)blockIdx.x * MK_WAVES + w;   // segment of this batch
    if (sl >= nseg) return;                                  // (no workgroup barrier below: a wave works alone)
    double* acc = mk_lds + (size_t)w * G;                                                  // segment sum of cluster c: lane c & 63 owns it
    uint32_t* cnt = reinterpret_cast<uint32_t*>(mk_lds + (size_t)MK_WAVES * G) + (size_t)w * G;   // (x > 0) << 16 | (x != 0)
    for (int c = lane; c < G; c += SGL_WAVE) { acc[c] = 0.0; cnt[c] = 0u; }
    const int64_t seg = seg0 + sl;
    const int32_t g = seg_gene[seg];
    const int64_t lo = p[g] + (seg - seg_first[g]) * (int64_t)MARKERS_SEG;
    int64_t hi = p[g + 1];
    if (hi - lo > MARKERS_SEG) hi = lo + MARKERS_SEG;
    for (int64_t q0 = lo; q0 < hi; q0 += SGL_WAVE) {
        const int64_t q = q0 + lane;
        double xv = 0.0;
        int32_t l = -1;
        if (q < hi) { xv = x[q]; l = lab[idx[q]]; }
        const double fv = TRANSFORM ? expm1(xv) : xv;
        mk_u64 todo = __ballot(l >= 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const int32_t c = __shfl(l, src, SGL_WAVE);
            const bool member = l == c;
            const double s = mk_wave_sum(member ? fv : 0.0);
            const mk_u64 mb = __ballot(member);
            const uint32_t np = (uint32_t)__popcll(__ballot(member && xv > 0.0));
            const uint32_t nn = (uint32_t)__popcll(__ballot(member && xv != 0.0));
            if (lane == (c & (SGL_WAVE - 1))) { acc[c] += s; cnt[c] += (np << 16) | nn; }
            todo &= ~mb;
        }
    }
    for (int c = lane; c < G; c += SGL_WAVE) {
        part[(size_t)sl * G + c] = acc[c];
        const uint32_t u = cnt[c];
        if (u >> 16) atomicAdd(&pos[(size_t)g + (size_t)m * c], (mk_u64)(u >> 16));
        if (u & 0xffffu) atomicAdd(&nz[(size_t)g + (size_t)m * c], (mk_u64)(u & 0xffffu));
    }
}

// sum[g, c] of the genes [g0, g1): their segments are [seg_first[g0], seg_first[g1]) = the batch, in order
__global__ __launch_bounds__(MK_THREADS) void mk_sums_finish_kernel(const double* __restrict__ part, const int64_t* __restrict__ seg_first,
                                                                   int32_t g0, int32_t g1, int32_t G, int64_t m, double* __restrict__ sum) {
    const int64_t t = (int64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    if (t >= (int64_t)(g1 - g0) * G) return;
    const int32_t g = g0 + (int32_t)(t / G), c = (int32_t)(t % G);
    const int64_t base = seg_first[g0];
    double s = 0.0;
    for (int64_t sg = seg_first[g]; sg < seg_first[g + 1]; ++sg) s += part[(size_t)(sg - base) * G + c];
    sum[(size_t)g + (size_t)m * c] = s;
}

// ---- 2. included non-zero entries per gene ---------------------------------------------------------------------------------
__global__ __launch_bounds__(MK_THREADS) void mk_count_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                             const int64_t* __restrict__ p, const int32_t* __restrict__ lab,
                                                             const int32_t* __restrict__ seg_gene, const int64_t* __restrict__ seg_first,
                                                             int64_t nseg, mk_u64* __restrict__ count) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t seg = (int64_t)blockIdx.x * MK_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (seg >= nseg) return;
    const int32_t g = seg_gene[seg];
    const int64_t lo = p[g] + (seg - seg_first[g]) * (int64_t)MARKERS_SEG;
    int64_t hi = p[g + 1];
    if (hi - lo > MARKERS_SEG) hi = lo + MARKERS_SEG;
    uint32_t n = 0;
    for (int64_t q = lo + lane; q < hi; q += SGL_WAVE) n += (x[q] != 0.0 && lab[idx[q]] >= 0) ? 1u : 0u;
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) n += __shfl_xor(n, off, SGL_WAVE);
    if (lane == 0 && n) atomicAdd(&count[g], (mk_u64)n);
}

// ---- the walk over a gene's sorted (key, label) pairs -------------------------------------------------------------------------
// exclusive prefix maximum / suffix minimum of one value per thread over the workgroup; *total = over all threads
__device__ __forceinline__ int mk_prefix_max(int v, int* sc, int* total) {
    const int lane = threadIdx.x & (SGL_WAVE - 1), w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < SGL_WAVE; off <<= 1) {
        const int o = __shfl_up(inc, off, SGL_WAVE);
        if (lane >= off) inc = max(inc, o);
    }
    if (lane == SGL_WAVE - 1) sc[w] = inc;
    __syncthreads();
    int ex = __shfl_up(inc, 1, SGL_WAVE);
    if (lane == 0) ex = INT_MIN;
    int tot = INT_MIN;
#pragma unroll
    for (int i = 0; i < MK_WAVES; ++i) {
        const int t = sc[i];
        if (i < w) ex = max(ex, t);
        tot = max(tot, t);
    }
    __syncthreads();   // sc is free again
    *total = tot;
    return ex;
}
__device__ __forceinline__ int mk_suffix_min(int v, int* sc, int* total) {
    const int lane = threadIdx.x & (SGL_WAVE - 1), w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < SGL_WAVE; off <<= 1) {
        const int o = __shfl_down(inc, off, SGL_WAVE);
        if (lane + off < SGL_WAVE) inc = min(inc, o);
    }
    if (lane == 0) sc[w] = inc;
    __syncthreads();
    int ex = __shfl_down(inc, 1, SGL_WAVE);
    if (lane == SGL_WAVE - 1) ex = INT_MAX;
    int tot = INT_MAX;
#pragma unroll
    for (int i = 0; i < MK_WAVES; ++i) {
        const int t = sc[i];
        if (i > w) ex = min(ex, t);
        tot = min(tot, t);
    }
    __syncthreads();
    *total = tot;
    return ex;
}

// The L sorted pairs of one gene (L <= 2^21; LDS or global memory), all MK_THREADS threads of the workgroup.  Adds to
// R[label] the doubled midranks of the members (positions counted over the N values of the gene: the Z zeros sit between
// the negatives and the positives), to cnt[label] their number; returns through *neg_out the negatives and adds t^3 - t of
// every run to *tie_acc (both LDS, zero on entry).  Ends with a barrier.
__device__ void mk_walk(const mk_u64* key, const int32_t* lab, int L, int64_t Z, mk_u64* R, uint32_t* cnt, int* sc, mk_u64* tie_acc,
                        uint32_t* neg_out) {
    const int tid = threadIdx.x;
    // forward: a = the start of the run a position lies in
    int carry = 0;
    mk_u64 tie = 0;
    uint32_t neg = 0;
    for (int base = 0; base < L; base += MARKERS_WALK) {
        const int j0 = base + tid * MK_PER_THREAD;
        mk_u64 k[MK_PER_THREAD];
        bool head[MK_PER_THREAD];
        int v = INT_MIN;
        mk_u64 prev = j0 > 0 && j0 < L ? key[j0 - 1] : 0;
#pragma unroll
        for (int e = 0; e < MK_PER_THREAD; ++e) {
            const int j = j0 + e;
            head[e] = false;
            k[e] = 0;
            if (j < L) {
                k[e] = key[j];
                head[e] = j == 0 || k[e] != prev;
                prev = k[e];
                if (head[e]) v = j;
            }
        }
        int total;
        int cur = max(mk_prefix_max(v, sc, &total), carry);
#pragma unroll
        for (int e = 0; e < MK_PER_THREAD; ++e) {
            const int j = j0 + e;
            if (j < L) {
                if (head[e]) cur = j;
                const bool positive = (k[e] >> 63) != 0;
                neg += positive ? 0u : 1u;
                const int32_t l = lab[j];
                atomicAdd(&R[l], (mk_u64)((int64_t)cur + (positive ? Z : 0)));
                atomicAdd(&cnt[l], 1u);
            }
        }
        carry = max(carry, total);
    }
    // backward: b = the end of the run; a run head takes the tie term
    int carry_b = L;
    const int last = L > 0 ? ((L - 1) / MARKERS_WALK) * MARKERS_WALK : -1;
    for (int base = last; base >= 0; base -= MARKERS_WALK) {
        const int j0 = base + tid * MK_PER_THREAD;
        mk_u64 k[MK_PER_THREAD];
        bool tail[MK_PER_THREAD], head[MK_PER_THREAD];
        int v = INT_MAX;
        mk_u64 prev = j0 > 0 && j0 < L ? key[j0 - 1] : 0;
#pragma unroll
        for (int e = 0; e < MK_PER_THREAD; ++e) {
            const int j = j0 + e;
            k[e] = j < L ? key[j] : 0;
        }
        const int jn = j0 + MK_PER_THREAD;
        const mk_u64 next = jn < L ? key[jn] : 0;
#pragma unroll
        for (int e = 0; e < MK_PER_THREAD; ++e) {
            const int j = j0 + e;
            tail[e] = head[e] = false;
            if (j < L) {
                head[e] = j == 0 || k[e] != prev;
                prev = k[e];
                const int en = e + 1 < MK_PER_THREAD ? e + 1 : e;
                const mk_u64 nx = e + 1 < MK_PER_THREAD ? k[en] : next;
                tail[e] = j + 1 == L || nx != k[e];
                if (tail[e] && v == INT_MAX) v = j + 1;   // the lowest end among this thread's positions
            }
        }
        int total;
        int cur = min(mk_suffix_min(v, sc, &total), carry_b);
#pragma unroll
        for (int e = MK_PER_THREAD - 1; e >= 0; --e) {
            const int j = j0 + e;
            if (j < L) {
                if (tail[e]) cur = j + 1;
                const bool positive = (k[e] >> 63) != 0;
                atomicAdd(&R[lab[j]], (mk_u64)((int64_t)cur + 1 + (positive ? Z : 0)));
                if (head[e]) {
                    const mk_u64 t = (mk_u64)(cur - j);
                    tie += t * t * t - t;
                }
            }
        }
        carry_b = min(carry_b, total);
    }
    if (tie) atomicAdd(tie_acc, tie);
    if (neg) atomicAdd(neg_out, neg);
    __syncthreads();
}

// closes a gene: the zero block's share of every cluster and its tie term
__device__ __forceinline__ void mk_close(int32_t g, int64_t m, int32_t G, int64_t N, int64_t L, const int64_t* __restrict__ group_n,
                                         const mk_u64* R, const uint32_t* cnt, mk_u64 tie, uint32_t neg, int64_t* __restrict__ rank2,
                                         mk_u64* __restrict__ tie_out) {
    const int64_t Z = N - L;
    const int64_t zr = 2 * (int64_t)neg + Z + 1;   // doubled midrank of the zero block [neg, neg + Z)
    for (int c = threadIdx.x; c < G; c += MK_THREADS)
        rank2[(size_t)g + (size_t)m * c] = (int64_t)R[c] + (group_n[c] - (int64_t)cnt[c]) * zr;
    if (threadIdx.x == 0) tie_out[g] = tie + ((mk_u64)Z * (mk_u64)Z * (mk_u64)Z - (mk_u64)Z);
}

// ---- 3. short genes: sort in LDS -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MK_THREADS) void mk_rank_lds_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                const int64_t* __restrict__ p, const int32_t* __restrict__ lab,
                                                                const int32_t* __restrict__ list, int32_t G, int64_t m, int64_t N,
                                                                const int64_t* __restrict__ group_n, int64_t* __restrict__ rank2,
                                                                mk_u64* __restrict__ tie_out) {
    __shared__ mk_u64 key[MARKERS_LDS_CAP];
    __shared__ int32_t lb[MARKERS_LDS_CAP];
    __shared__ mk_u64 R[MARKERS_MAX_GROUPS];
    __shared__ uint32_t cnt[MARKERS_MAX_GROUPS];
    __shared__ int sc[MK_WAVES];
    __shared__ mk_u64 tie_acc;
    __shared__ uint32_t neg, fill;
    const int tid = threadIdx.x;
    const int32_t g = list[blockIdx.x];
    for (int c = tid; c < G; c += MK_THREADS) { R[c] = 0; cnt[c] = 0; }
    if (tid == 0) { tie_acc = 0; neg = 0; fill = 0; }
    __syncthreads();
    const int64_t lo = p[g], hi = p[g + 1];
    for (int64_t q0 = lo; q0 < hi; q0 += MK_THREADS) {   // (the order of the gathered pairs is free: they are sorted next)
        const int64_t q = q0 + tid;
        if (q < hi) {
            const double xv = x[q];
            const int32_t l = lab[idx[q]];
            if (xv != 0.0 && l >= 0) {
                const uint32_t at = atomicAdd(&fill, 1u);
                if (at < MARKERS_LDS_CAP) { key[at] = mk_key(xv); lb[at] = l; }   // (the host sent only genes that fit)
            }
        }
    }
    __syncthreads();
    const int L = (int)min(fill, (uint32_t)MARKERS_LDS_CAP);
    int P = 2;
    while (P < L) P <<= 1;
    for (int i = L + tid; i < P; i += MK_THREADS) { key[i] = ~0ull; lb[i] = 0; }   // above every key of a finite value
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += MK_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const mk_u64 a = key[i], b = key[o];
                    if ((a > b) == ((i & k) == 0)) {
                        key[i] = b; key[o] = a;
                        const int32_t t = lb[i]; lb[i] = lb[o]; lb[o] = t;
                    }
                }
            }
            __syncthreads();
        }
    mk_walk(key, lb, L, N - (int64_t)L, R, cnt, sc, &tie_acc, &neg);
    mk_close(g, m, G, N, (int64_t)L, group_n, R, cnt, tie_acc, neg, rank2, tie_out);
}

// ---- 4. long genes: scratch, segmented sort, walk ----------------------------------------------------------------------------
// one workgroup per gene of the batch: its included non-zero entries as (key, label) at off[b] ..; a wave reserves its places at once
__global__ __launch_bounds__(MK_THREADS) void mk_fill_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                            const int64_t* __restrict__ p, const int32_t* __restrict__ lab,
                                                            const int32_t* __restrict__ list, const int64_t* __restrict__ off,
                                                            mk_u64* __restrict__ filled, mk_u64* __restrict__ key, int32_t* __restrict__ lb) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int b = blockIdx.x;
    const int32_t g = list[b];
    const int64_t o = off[b], cap = off[b + 1] - o;
    const int64_t lo = p[g], hi = p[g + 1];
    for (int64_t q0 = lo; q0 < hi; q0 += MK_THREADS) {
        const int64_t q = q0 + threadIdx.x;
        double xv = 0.0;
        int32_t l = -1;
        if (q < hi) { xv = x[q]; l = lab[idx[q]]; }
        const bool take = xv != 0.0 && l >= 0;
        const mk_u64 mb = __ballot(take);
        if (mb) {
            mk_u64 first = 0;
            if (lane == __ffsll((long long)mb) - 1) first = atomicAdd(&filled[b], (mk_u64)__popcll(mb));
            first = __shfl(first, __ffsll((long long)mb) - 1, SGL_WAVE);
            const int64_t at = (int64_t)first + __popcll(mb & ((1ull << lane) - 1ull));
            if (take && at < cap) { key[o + at] = mk_key(xv); lb[o + at] = l; }   // (cap = the count of the same entries)
        }
    }
}

__global__ __launch_bounds__(MK_THREADS) void mk_rank_walk_kernel(const mk_u64* __restrict__ key, const int32_t* __restrict__ lb,
                                                                 const int32_t* __restrict__ list, const int64_t* __restrict__ off, int32_t G,
                                                                 int64_t m, int64_t N, const int64_t* __restrict__ group_n,
                                                                 int64_t* __restrict__ rank2, mk_u64* __restrict__ tie_out) {
    __shared__ mk_u64 R[MARKERS_MAX_GROUPS];
    __shared__ uint32_t cnt[MARKERS_MAX_GROUPS];
    __shared__ int sc[MK_WAVES];
    __shared__ mk_u64 tie_acc;
    __shared__ uint32_t neg;
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < G; c += MK_THREADS) { R[c] = 0; cnt[c] = 0; }
    if (threadIdx.x == 0) { tie_acc = 0; neg = 0; }
    __syncthreads();
    const int64_t o = off[b];
    const int L = (int)(off[b + 1] - o);
    mk_walk(key + o, lb + o, L, N - (int64_t)L, R, cnt, sc, &tie_acc, &neg);
    mk_close(list[b], m, G, N, (int64_t)L, group_n, R, cnt, tie_acc, neg, rank2, tie_out);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
namespace {
struct MkPlan {
    std::vector<int64_t> p, first;   // host: the gene offsets of t(A), the first segment of every gene
    DevBuf<int32_t> seg_gene, lab;
    DevBuf<int64_t> seg_first, group_n;
    int64_t nseg = 0;
    int32_t m = 0;
};

int mk_plan(sgl_ctx* c, MkPlan& P, const int32_t* labels, int32_t G, const int64_t* group_n) {
    const DevCSC& M = c->At;
    const int32_t m = M.ncol;
    P.m = m;
    P.p.assign((size_t)m + 1, 0);
    P.first.assign((size_t)m + 1, 0);
    HIPCHK(hipMemcpyAsync(P.p.data(), M.p, sizeof(int64_t) * P.p.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int32_t g = 0; g < m; ++g) P.first[(size_t)g + 1] = P.first[g] + (P.p[(size_t)g + 1] - P.p[g] + MARKERS_SEG - 1) / MARKERS_SEG;
    P.nseg = P.first[m];
    if ((P.nseg + MK_WAVES - 1) / MK_WAVES > INT32_MAX) { sgl_set_error("markers: %lld segments are more than one launch holds", (long long)P.nseg); return SGL_EINVAL; }
    std::vector<int32_t> sg((size_t)std::max<int64_t>(P.nseg, 1));
    for (int32_t g = 0; g < m; ++g)
        for (int64_t s = P.first[g]; s < P.first[(size_t)g + 1]; ++s) sg[(size_t)s] = g;
    SGLCHK(P.seg_gene.alloc(sg.size()));
    SGLCHK(P.seg_first.alloc(P.first.size()));
    SGLCHK(P.lab.alloc((size_t)std::max(M.nrow, 1)));
    SGLCHK(P.group_n.alloc((size_t)G));
    HIPCHK(hipMemcpyAsync(P.seg_gene.p, sg.data(), sizeof(int32_t) * sg.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.seg_first.p, P.first.data(), sizeof(int64_t) * P.first.size(), hipMemcpyHostToDevice, c->stream));
    if (M.nrow > 0) HIPCHK(hipMemcpyAsync(P.lab.p, labels, sizeof(int32_t) * (size_t)M.nrow, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.group_n.p, group_n, sizeof(int64_t) * (size_t)G, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the host vector goes
    return SGL_OK;
}

int mk_sums_on(sgl_ctx* c, MkPlan& P, int32_t G, int transform, int64_t* pos, int64_t* nz, double* sum) {
    const DevCSC& M = c->At;
    const int32_t m = P.m;
    const size_t mg = (size_t)std::max(m, 1) * (size_t)G;
    DevBuf<mk_u64> dpos, dnz;
    DevBuf<double> dsum, part;
    SGLCHK(dpos.alloc(mg));
    SGLCHK(dnz.alloc(mg));
    SGLCHK(dsum.alloc(mg));
    HIPCHK(hipMemsetAsync(dpos.p, 0, sizeof(mk_u64) * mg, c->stream));
    HIPCHK(hipMemsetAsync(dnz.p, 0, sizeof(mk_u64) * mg, c->stream));
    // batches of whole genes whose segment partials fit the scratch (a gene holds at most 2^21 / MARKERS_SEG segments)
    const int64_t seg_cap = std::max<int64_t>(MK_SUMS_SCRATCH / ((int64_t)sizeof(double) * G), MARKERS_MAX_CELLS / MARKERS_SEG + 1);
    SGLCHK(part.alloc((size_t)std::max<int64_t>(std::min(seg_cap, P.nseg), 1) * (size_t)G));
    const size_t lds = (size_t)MK_WAVES * (size_t)G * 12;
    {
        Phase ph(c, SGL_PH_SCALE);
        for (int32_t g0 = 0; g0 < m;) {
            int32_t g1 = g0 + 1;
            while (g1 < m && P.first[(size_t)g1 + 1] - P.first[g0] <= seg_cap) ++g1;
            const int64_t s0 = P.first[g0], ns = P.first[g1] - s0;
            if (ns > 0) {
                const dim3 grid((unsigned)((ns + MK_WAVES - 1) / MK_WAVES));
                if (transform)
                    mk_sums_kernel<1><<<grid, dim3(MK_THREADS), lds, c->stream>>>(M.x, M.i, M.p, P.lab.p, P.seg_gene.p, P.seg_first.p, s0, ns, G,
                                                                                  (int64_t)m, part.p, dpos.p, dnz.p);
                else
                    mk_sums_kernel<0><<<grid, dim3(MK_THREADS), lds, c->stream>>>(M.x, M.i, M.p, P.lab.p, P.seg_gene.p, P.seg_first.p, s0, ns, G,
                                                                                  (int64_t)m, part.p, dpos.p, dnz.p);
                HIPCHK(hipGetLastError());
            }
            const int64_t cells = (int64_t)(g1 - g0) * G;
            mk_sums_finish_kernel<<<dim3((unsigned)((cells + MK_THREADS - 1) / MK_THREADS)), dim3(MK_THREADS), 0, c->stream>>>(
                part.p, P.seg_first.p, g0, g1, G, (int64_t)m, dsum.p);
            HIPCHK(hipGetLastError());
            g0 = g1;
        }
    }
    if (m > 0) {
        const size_t n = (size_t)m * (size_t)G;
        if (pos) HIPCHK(hipMemcpyAsync(pos, dpos.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (nz) HIPCHK(hipMemcpyAsync(nz, dnz.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (sum) HIPCHK(hipMemcpyAsync(sum, dsum.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return SGL_OK;
}

int mk_ranks_on(sgl_ctx* c, MkPlan& P, int32_t G, int64_t N, int64_t max_batch_entries, int64_t* rank2, uint64_t* tie) {
    const DevCSC& M = c->At;
    const int32_t m = P.m;
    hipStream_t s = c->stream;
    const size_t mg = (size_t)std::max(m, 1) * (size_t)G, m1 = (size_t)std::max(m, 1);
    DevBuf<mk_u64> dcount, dtie;
    DevBuf<int64_t> drank;
    SGLCHK(dcount.alloc(m1));
    SGLCHK(dtie.alloc(m1));
    SGLCHK(drank.alloc(mg));
    HIPCHK(hipMemsetAsync(dcount.p, 0, sizeof(mk_u64) * m1, s));
    std::vector<int64_t> count(m1, 0);
    {
        Phase ph(c, SGL_PH_SCALE);
        if (P.nseg > 0) {
            mk_count_kernel<<<dim3((unsigned)((P.nseg + MK_WAVES - 1) / MK_WAVES)), dim3(MK_THREADS), 0, s>>>(M.x, M.i, M.p, P.lab.p, P.seg_gene.p,
                                                                                                        P.seg_first.p, P.nseg, dcount.p);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipMemcpyAsync(count.data(), dcount.p, sizeof(int64_t) * m1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<int32_t> short_list(m1), long_list(m1);
    std::vector<int64_t> long_len(m1), cut(m1 + 1);
    int64_t ns = 0, nl = 0;
    markers_split_paths(count.data(), m, MARKERS_LDS_CAP, short_list.data(), &ns, long_list.data(), long_len.data(), &nl);
    const int64_t runs = nl > 0 ? markers_batches(long_len.data(), nl, max_batch_entries, cut.data()) : 0;
    c->markers_last[0] = ns;
    c->markers_last[1] = nl;
    c->markers_last[2] = runs;
    c->markers_last[3] = MARKERS_LDS_CAP;
    DevBuf<int32_t> dlist;
    SGLCHK(dlist.alloc(m1));
    if (ns > 0) {
        HIPCHK(hipMemcpyAsync(dlist.p, short_list.data(), sizeof(int32_t) * (size_t)ns, hipMemcpyHostToDevice, s));
        Phase ph(c, SGL_PH_SCALE);
        mk_rank_lds_kernel<<<dim3((unsigned)ns), dim3(MK_THREADS), 0, s>>>(M.x, M.i, M.p, P.lab.p, dlist.p, G, (int64_t)m, N, P.group_n.p,
                                                                          drank.p, dtie.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));   // dlist is rewritten below
    }
    if (nl > 0) {
        int64_t max_entries = 0, max_genes = 0;
        for (int64_t b = 0; b < runs; ++b) {
            int64_t sum = 0;
            for (int64_t g = cut[(size_t)b]; g < cut[(size_t)b + 1]; ++g) sum += long_len[(size_t)g];
            max_entries = std::max(max_entries, sum);
            max_genes = std::max(max_genes, cut[(size_t)b + 1] - cut[(size_t)b]);
        }
        if (max_entries > INT32_MAX) { sgl_set_error("markers: a batch holds %lld entries", (long long)max_entries); return SGL_EINVAL; }
        DevBuf<mk_u64> k1, k2, filled;
        DevBuf<int32_t> l1, l2;
        DevBuf<int64_t> doff;
        DevBuf<char> tmp;
        SGLCHK(k1.alloc((size_t)max_entries));
        SGLCHK(k2.alloc((size_t)max_entries));
        SGLCHK(l1.alloc((size_t)max_entries));
        SGLCHK(l2.alloc((size_t)max_entries));
        SGLCHK(doff.alloc((size_t)max_genes + 1));
        SGLCHK(filled.alloc((size_t)max_genes));
        HIPCHK(hipMemcpyAsync(dlist.p, long_list.data(), sizeof(int32_t) * (size_t)nl, hipMemcpyHostToDevice, s));
        std::vector<int64_t> off;
        size_t tmp_cap = 0;
        Phase ph(c, SGL_PH_SCALE);
        for (int64_t b = 0; b < runs; ++b) {
            const int64_t g0 = cut[(size_t)b], ng = cut[(size_t)b + 1] - g0;
            off.assign((size_t)ng + 1, 0);
            for (int64_t g = 0; g < ng; ++g) off[(size_t)g + 1] = off[(size_t)g] + long_len[(size_t)(g0 + g)];
            const int64_t tot = off[(size_t)ng];
            HIPCHK(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * ((size_t)ng + 1), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(filled.p, 0, sizeof(mk_u64) * (size_t)ng, s));
            mk_fill_kernel<<<dim3((unsigned)ng), dim3(MK_THREADS), 0, s>>>(M.x, M.i, M.p, P.lab.p, dlist.p + g0, doff.p, filled.p, k1.p, l1.p);
            HIPCHK(hipGetLastError());
            size_t bytes = 0;
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, k1.p, k2.p, l1.p, l2.p, (int)tot, (int)ng, doff.p, doff.p + 1, 0, 64, s));
            if (bytes > tmp_cap) {
                HIPCHK(hipStreamSynchronize(s));
                SGLCHK(tmp.alloc(bytes));
                tmp_cap = bytes;
            }
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(tmp.p, bytes, k1.p, k2.p, l1.p, l2.p, (int)tot, (int)ng, doff.p, doff.p + 1, 0, 64, s));
            mk_rank_walk_kernel<<<dim3((unsigned)ng), dim3(MK_THREADS), 0, s>>>(k2.p, l2.p, dlist.p + g0, doff.p, G, (int64_t)m, N, P.group_n.p,
                                                                               drank.p, dtie.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));   // `off` is rewritten for the next batch
        }
    }
    if (m > 0) {
        if (rank2) HIPCHK(hipMemcpyAsync(rank2, drank.p, sizeof(int64_t) * (size_t)m * (size_t)G, hipMemcpyDeviceToHost, s));
        if (tie) HIPCHK(hipMemcpyAsync(tie, dtie.p, sizeof(uint64_t) * (size_t)m, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return SGL_OK;
}
}   // namespace

int sgl_markers_args_check(const char* who, const int32_t* labels, int64_t ncol, int32_t n_groups, int transform, double pseudocount) {
    int64_t pos = -1;
    int32_t val = 0;
    switch (markers_check_args(labels, ncol, n_groups, transform, pseudocount, &pos, &val)) {
    case MARKERS_ARGS_OK: return SGL_OK;
    case MARKERS_ARGS_NULL: sgl_set_error("%s: NULL labels", who); break;
    case MARKERS_ARGS_GROUPS: sgl_set_error("%s: n_groups = %d is outside [1, %d]", who, n_groups, MARKERS_MAX_GROUPS); break;
    case MARKERS_ARGS_TRANSFORM: sgl_set_error("%s: transform = %d is neither 0 (identity) nor 1 (expm1)", who, transform); break;
    case MARKERS_ARGS_PSEUDOCOUNT: sgl_set_error("%s: pseudocount = %g: a pseudocount is finite and not negative", who, pseudocount); break;
    case MARKERS_ARGS_CELLS: sgl_set_error("%s: ncol = %lld: the tie term fits 64 bits up to 2^21 cells", who, (long long)ncol); break;
    case MARKERS_ARGS_LABEL: sgl_set_error("%s: labels[%lld] = %d is outside [-1, %d)", who, (long long)pos, val, n_groups); break;
    }
    return SGL_EINVAL;
}

int sgl_markers_core(sgl_ctx* c, const int32_t* labels, int32_t G, int transform, int64_t max_batch_entries, bool sums, bool ranks,
                     int64_t* group_n, int64_t* pos, int64_t* nz, double* sum, int64_t* rank2, uint64_t* tie) {
    std::vector<int64_t> gn((size_t)G);
    const int64_t N = markers_group_counts(labels, c->At.nrow, G, gn.data());
    if (group_n) std::copy(gn.begin(), gn.end(), group_n);
    MkPlan P;
    int rc = mk_plan(c, P, labels, G, gn.data());
    if (rc == SGL_OK && sums) rc = mk_sums_on(c, P, G, transform, pos, nz, sum);
    if (rc == SGL_OK && ranks) rc = mk_ranks_on(c, P, G, N, max_batch_entries, rank2, tie);
    // every return path waits for the stream before the plan's buffers (and the caller's host arrays) go
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("markers: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

int sgl_markers_all(sgl_ctx* c, const int32_t* labels, int32_t G, int transform, double pseudocount, int64_t* group_n, int64_t* pos,
                    double* sum, int64_t* rank2, uint64_t* tie, double* pct_in, double* pct_out, double* log2fc, double* z, double* p) {
    const int32_t m = c->At.ncol;
    const size_t mg = (size_t)std::max(m, 1) * (size_t)G;
    std::vector<int64_t> gn((size_t)G), hpos(mg), hrank(mg);
    std::vector<double> hsum(mg);
    std::vector<uint64_t> htie((size_t)std::max(m, 1));
    SGLCHK(sgl_markers_core(c, labels, G, transform, 0, true, true, gn.data(), hpos.data(), nullptr, hsum.data(), hrank.data(), htie.data()));
    markers_derive(m, G, gn.data(), hpos.data(), hsum.data(), hrank.data(), htie.data(), pseudocount, pct_in, pct_out, log2fc, z, p);
    const size_t n = (size_t)m * (size_t)G;
    if (group_n) std::copy(gn.begin(), gn.end(), group_n);
    if (pos) std::copy(hpos.begin(), hpos.begin() + n, pos);
    if (sum) std::copy(hsum.begin(), hsum.begin() + n, sum);
    if (rank2) std::copy(hrank.begin(), hrank.begin() + n, rank2);
    if (tie) std::copy(htie.begin(), htie.begin() + m, tie);
    return SGL_OK;
}
