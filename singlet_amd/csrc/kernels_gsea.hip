// Gene set enrichment of the factors (include/singlet_hip.h, "Gene set enrichment"): the pre-ranked weighted
// Kolmogorov-Smirnov score of every gene set in every factor, and a permutation null of random sets of the same sizes drawn
// from the counter hash.  This file holds
//   1. gs_rank_keys_kernel / hipcub's segmented radix sort / gs_rank_scatter_kernel: per factor the genes by (w descending,
//      gene ascending) -- the sort is stable and the genes enter in ascending order -- giving pos_f[g] and the rank-ordered |w|.
//   2. gs_es_kernel: ONE WAVE per (set, factor): the positions of the set's genes gathered into LDS, sorted there (bitonic),
//      scored by gs_score.
//   3. gs_sample_keys_kernel / the segmented sort / gs_sample_gather_kernel: per permutation the keys of the m genes, the
//      s_max smallest by (key, gene) kept in that order -- the full sort's prefix by construction.
//   4. gs_null_kernel: ONE WAVE per (permutation, factor): the s_max sampled genes' (position, arrival index) pairs sorted once
//      by position in LDS; for every distinct size s a ballot compacts the elements with arrival index < s (order kept),
//      and gs_score scores them.  The plain per-size pass; an incremental form was not built.
//   5. gs_tally_sets_kernel / gs_tally_sizes_kernel: the integer counts per (set, factor) over a batch's permutations, and
//      per (size, factor) the counts of either sign with the running sums added in ascending r.
// gs_score is the stated order itself: blocks of 64 hits, the Kogge-Stone ladder through wave shifts, the carry added
// afterwards; max / min by a wave reduction.  No floating-point atomics, no loop whose trip count follows the launch size;
// the unit is compiled with -ffp-contract=off and every division is an IEEE division.  tests/gsea_restatement.py restates
// all of it in numpy.
#include "sgl_internal.h"
#include "gsea_host.h"

#include <hipcub/hipcub.hpp>
#include <climits>
#include <cmath>

#define GS_THREADS 256                 // the element-wise kernels
#define GS_WAVE SGL_WAVE               // the scoring kernels: one wave per workgroup
static_assert(GSEA_BLOCK == SGL_WAVE, "a block of hits is one wave wide");
static_assert((GSEA_LDS_CAP & (GSEA_LDS_CAP - 1)) == 0, "capacity: a power of two");

typedef unsigned long long gs_u64;

// Image of a finite double under which an ASCENDING unsigned order is the DESCENDING order of the values; both zeros share
// the image of +0.0, so that the zeros of a factor are one tie run
__device__ __forceinline__ gs_u64 gs_desc_key(double x) {
    x = x + 0.0;   // -0.0 + 0.0 = +0.0; every other value is kept
    const gs_u64 u = (gs_u64)__double_as_longlong(x);
    const gs_u64 asc = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return ~asc;
}

// ---- 1. rankings --------------------------------------------------------------------------------------------------------------
// the factors [f0, f0 + nf): key and gene of every (factor, gene), factor-major
__global__ __launch_bounds__(GS_THREADS) void gs_rank_keys_kernel(const double* __restrict__ w, int64_t m, int64_t f0, int64_t n,
                                                                 gs_u64* __restrict__ key, int32_t* __restrict__ gene) {
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (t >= n) return;
    key[t] = gs_desc_key(w[f0 * m + t]);
    gene[t] = (int32_t)(t % m);
}
__global__ __launch_bounds__(GS_THREADS) void gs_rank_scatter_kernel(const double* __restrict__ w, const int32_t* __restrict__ order,
                                                                    int64_t m, int64_t f0, int64_t n, int32_t* __restrict__ pos,
                                                                    double* __restrict__ aw) {
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (t >= n) return;
    const int64_t f = f0 + t / m, p = t % m;
    const int32_t g = order[t];
    pos[f * m + g] = (int32_t)p;
    aw[f * m + p] = fabs(w[f * m + g]);
}
// offsets of n + 1 segments of m items
__global__ __launch_bounds__(GS_THREADS) void gs_offsets_kernel(int64_t m, int64_t n1, int64_t* __restrict__ off) {
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (t < n1) off[t] = t * m;
}

// ---- the score of one set, one wave --------------------------------------------------------------------------------------------
// cp[0, s): the ascending positions of the hits (LDS); cum[0, s): LDS scratch; aw: the rank-ordered |w| of the factor.  All
// 64 lanes of the one wave of the workgroup take part; every lane returns max top and min bottom.  Ends with a barrier.
__device__ __forceinline__ void gs_score(const int32_t* cp, double* cum, int s, const double* __restrict__ aw, int64_t m, double* es_pos,
                                         double* es_neg) {
    const int lane = threadIdx.x;
    double carry = 0.0;
    for (int b0 = 0; b0 < s; b0 += GSEA_BLOCK) {
        const int i = b0 + lane;
        double v = i < s ? aw[cp[i]] : 0.0;
#pragma unroll
        for (int d = 1; d < GSEA_BLOCK; d <<= 1) {
            const double o = __shfl_up(v, d, GS_WAVE);
            if (lane >= d) v = v + o;
        }
        if (i < s) cum[i] = carry + v;
        carry = carry + __shfl(v, GSEA_BLOCK - 1, GS_WAVE);
    }
    __syncthreads();
    const double NR = cum[s - 1];
    const double ds = (double)s, dmiss = (double)(m - (int64_t)s);
    double mx = -INFINITY, mn = INFINITY;
    for (int i = lane; i < s; i += GS_WAVE) {
        const int32_t p = cp[i];
        double hit, step;
        if (NR == 0.0) {
            hit = (double)(i + 1) / ds;
            step = 1.0 / ds;
        } else {
            hit = cum[i] / NR;
            step = aw[p] / NR;
        }
        const double top = hit - (double)(p - i) / dmiss;
        const double bottom = top - step;
        mx = fmax(mx, top);
        mn = fmin(mn, bottom);
    }
#pragma unroll
    for (int off = GS_WAVE / 2; off > 0; off >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, off, GS_WAVE));
        mn = fmin(mn, __shfl_xor(mn, off, GS_WAVE));
    }
    *es_pos = mx;
    *es_neg = mn;
    __syncthreads();   // cp and cum are free again
}

__device__ __forceinline__ double gs_pick(int score_type, double es_pos, double es_neg) {
    return score_type == 0 ? es_pos : (score_type == 1 ? es_neg : gsea_std_score(es_pos, es_neg));
}

// ascending bitonic sort of n (a power of two) LDS values by the one wave of the workgroup
template <typename T>
__device__ __forceinline__ void gs_sort(T* a, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += GS_WAVE) {
                const int o = i ^ j;
                if (o > i) {
                    const T x = a[i], y = a[o];
                    if ((x > y) == ((i & k) == 0)) { a[i] = y; a[o] = x; }
                }
            }
            __syncthreads();
        }
}
__host__ __device__ inline int gs_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// ---- 2. observed scores ----------------------------------------------------------------------------------------------------------
// LDS: cum (double) [cap], cp (int32) [pow2(cap)]; es: three planes of P x k (pos, neg, std), set fastest
__global__ __launch_bounds__(GS_WAVE) void gs_es_kernel(const int32_t* __restrict__ pos, const double* __restrict__ aw,
                                                       const int64_t* __restrict__ set_ptr, const int32_t* __restrict__ set_genes, int64_t m,
                                                       int64_t P, int64_t k, int cap, double* __restrict__ es) {
    extern __shared__ __attribute__((aligned(16))) char gs_smem[];
    double* cum = reinterpret_cast<double*>(gs_smem);
    int32_t* cp = reinterpret_cast<int32_t*>(gs_smem + (size_t)cap * sizeof(double));
    const int64_t j = blockIdx.x, f = blockIdx.y;
    const int64_t lo = set_ptr[j];
    const int s = (int)(set_ptr[j + 1] - lo);   // 1 <= s <= cap: the host checked
    const int n = gs_pow2(s);
    for (int i = threadIdx.x; i < n; i += GS_WAVE) cp[i] = i < s ? pos[f * m + set_genes[lo + i]] : INT_MAX;
    __syncthreads();
    gs_sort(cp, n);
    double ep, en;
    gs_score(cp, cum, s, aw + f * m, m, &ep, &en);
    if (threadIdx.x == 0) {
        const size_t at = (size_t)j + (size_t)P * (size_t)f, plane = (size_t)P * (size_t)k;
        es[at] = ep;
        es[plane + at] = en;
        es[2 * plane + at] = gsea_std_score(ep, en);
    }
}

// ---- 3. null sample ---------------------------------------------------------------------------------------------------------------
// permutations [r0, r0 + nb): key(r, g) and g, permutation-major
__global__ __launch_bounds__(GS_THREADS) void gs_sample_keys_kernel(uint64_t seed, int64_t r0, int64_t m, int64_t n, gs_u64* __restrict__ key,
                                                                   int32_t* __restrict__ gene) {
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (t >= n) return;
    const int64_t g = t % m;
    key[t] = sgl_rand2(seed, (uint64_t)(r0 + t / m), (uint64_t)g);
    gene[t] = (int32_t)g;
}
// sample[rl, t] = the gene at place t of permutation rl's sorted order, t < s_max
__global__ __launch_bounds__(GS_THREADS) void gs_sample_gather_kernel(const int32_t* __restrict__ order, int64_t m, int64_t s_max, int64_t n,
                                                                     int32_t* __restrict__ sample) {
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (t >= n) return;
    sample[t] = order[(t / s_max) * m + t % s_max];
}

// ---- 4. null scores ---------------------------------------------------------------------------------------------------------------
// LDS: pr (u64) [pow2(s_max)], cum (double) [s_max rounded to 2], cp (int32) [s_max]; null[(f S + si) ld + rl]
__global__ __launch_bounds__(GS_WAVE) void gs_null_kernel(const int32_t* __restrict__ pos, const double* __restrict__ aw,
                                                         const int32_t* __restrict__ sample, const int32_t* __restrict__ sizes, int S, int s_max,
                                                         int64_t m, int64_t ld, int score_type, double* __restrict__ null_out) {
    extern __shared__ __attribute__((aligned(16))) char gs_smem[];
    const int n = gs_pow2(s_max), s_even = (s_max + 1) & ~1;
    gs_u64* pr = reinterpret_cast<gs_u64*>(gs_smem);
    double* cum = reinterpret_cast<double*>(gs_smem + (size_t)n * sizeof(gs_u64));
    int32_t* cp = reinterpret_cast<int32_t*>(gs_smem + (size_t)n * sizeof(gs_u64) + (size_t)s_even * sizeof(double));
    const int lane = threadIdx.x;
    const int64_t rl = blockIdx.x, f = blockIdx.y;
    for (int i = lane; i < n; i += GS_WAVE)
        pr[i] = i < s_max ? (((gs_u64)(uint32_t)pos[f * m + sample[rl * s_max + i]] << 32) | (gs_u64)(uint32_t)i) : ~0ull;
    __syncthreads();
    gs_sort(pr, n);
    for (int si = 0; si < S; ++si) {
        const int s = sizes[si];
        int base = 0;
        for (int i0 = 0; i0 < s_max && base < s; i0 += GS_WAVE) {   // (base and s are the same in every lane)
            const int i = i0 + lane;
            const gs_u64 e = i < s_max ? pr[i] : ~0ull;
            const bool take = i < s_max && (int)(uint32_t)(e & 0xffffffffull) < s;
            const gs_u64 mb = __ballot(take);
            if (take) cp[base + __popcll(mb & ((1ull << lane) - 1ull))] = (int32_t)(e >> 32);
            base += __popcll(mb);
        }
        __syncthreads();
        double ep, en;
        gs_score(cp, cum, s, aw + f * m, m, &ep, &en);
        if (lane == 0) null_out[((size_t)f * (size_t)S + (size_t)si) * (size_t)ld + (size_t)rl] = gs_pick(score_type, ep, en);
    }
}

// ---- 5. tallies -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GS_THREADS) void gs_tally_sets_kernel(const double* __restrict__ es, const int32_t* __restrict__ size_idx,
                                                                  const double* __restrict__ null_in, int64_t P, int64_t k, int64_t S,
                                                                  int64_t ld, int64_t nb, gs_u64* __restrict__ n_ge, gs_u64* __restrict__ n_le) {
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (t >= P * k) return;
    const int64_t j = t % P, f = t / P;
    const double e = es[t];
    const double* nl = null_in + ((size_t)f * (size_t)S + (size_t)size_idx[j]) * (size_t)ld;
    gs_u64 ge = 0, le = 0;
    for (int64_t r = 0; r < nb; ++r) {
        const double v = nl[r];
        ge += v >= e ? 1u : 0u;
        le += v <= e ? 1u : 0u;
    }
    n_ge[t] += ge;
    n_le[t] += le;
}
// per (size, factor): the running state lives in global memory across the batches, so the sums are added in ascending r
__global__ __launch_bounds__(GS_THREADS) void gs_tally_sizes_kernel(const double* __restrict__ null_in, int64_t n, int64_t ld, int64_t nb,
                                                                   gs_u64* __restrict__ cnt_pos, gs_u64* __restrict__ cnt_neg,
                                                                   double* __restrict__ sum_pos, double* __restrict__ sum_neg) {
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (t >= n) return;
    const double* nl = null_in + (size_t)t * (size_t)ld;
    gs_u64 cp = cnt_pos[t], cn = cnt_neg[t];
    double sp = sum_pos[t], sn = sum_neg[t];
    for (int64_t r = 0; r < nb; ++r) {
        const double v = nl[r];
        if (v >= 0.0) { ++cp; sp = sp + v; }
        if (v <= 0.0) { ++cn; sn = sn + v; }
    }
    cnt_pos[t] = cp;
    cnt_neg[t] = cn;
    sum_pos[t] = sp;
    sum_neg[t] = sn;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {
inline unsigned gs_blocks(int64_t n) { return (unsigned)((n + GS_THREADS - 1) / GS_THREADS); }

// stage timer of sgl_c_gsea's stage_ms: events around a stage when the caller asked for the times
struct GsTimer {
    hipStream_t s;
    double* ms;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    GsTimer(hipStream_t s_, double* ms_) : s(s_), ms(ms_) {
        if (ms && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) { (void)hipGetLastError(); ms = nullptr; }
    }
    ~GsTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void begin() { if (ms) (void)hipEventRecord(e0, s); }
    void end(int stage) {
        if (!ms) return;
        float t = 0.f;
        if (hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms[stage] += t;
        else (void)hipGetLastError();
    }
};

struct GsRank {
    DevBuf<double> w, aw;
    DevBuf<int32_t> pos;
};

// one segmented sort of nseg segments of m (key, gene) pairs each; the buffers hold nseg * m items
int gs_segmented_sort(hipStream_t s, gs_u64* k1, gs_u64* k2, int32_t* v1, int32_t* v2, int64_t m, int64_t nseg, int64_t* off, DevBuf<char>& tmp,
                      size_t& tmp_cap) {
    gs_offsets_kernel<<<dim3(gs_blocks(nseg + 1)), dim3(GS_THREADS), 0, s>>>(m, nseg + 1, off);
    HIPCHK(hipGetLastError());
    size_t bytes = 0;
    HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, k1, k2, v1, v2, (int)(m * nseg), (int)nseg, off, off + 1, 0, 64, s));
    if (bytes > tmp_cap) {
        HIPCHK(hipStreamSynchronize(s));
        SGLCHK(tmp.alloc(bytes));
        tmp_cap = bytes;
    }
    HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(tmp.p, bytes, k1, k2, v1, v2, (int)(m * nseg), (int)nseg, off, off + 1, 0, 64, s));
    return SGL_OK;
}

// stage 1: w (host, m x k) -> R.w, R.pos, R.aw
int gs_rank(sgl_ctx* c, GsRank& R, const double* w, int64_t m, int64_t k) {
    hipStream_t s = c->stream;
    const size_t mk = (size_t)m * (size_t)k;
    SGLCHK(R.w.alloc(mk));
    SGLCHK(R.aw.alloc(mk));
    SGLCHK(R.pos.alloc(mk));
    HIPCHK(hipMemcpyAsync(R.w.p, w, sizeof(double) * mk, hipMemcpyHostToDevice, s));
    const int64_t nf_max = std::min<int64_t>(k, std::max<int64_t>(GSEA_SORT_ITEMS / m, 1));
    const size_t items = (size_t)nf_max * (size_t)m;
    DevBuf<gs_u64> k1, k2;
    DevBuf<int32_t> v1, v2;
    DevBuf<int64_t> off;
    DevBuf<char> tmp;
    size_t tmp_cap = 0;
    SGLCHK(k1.alloc(items));
    SGLCHK(k2.alloc(items));
    SGLCHK(v1.alloc(items));
    SGLCHK(v2.alloc(items));
    SGLCHK(off.alloc((size_t)nf_max + 1));
    Phase ph(c, SGL_PH_SCALE);
    for (int64_t f0 = 0; f0 < k; f0 += nf_max) {
        const int64_t nf = std::min(nf_max, k - f0), n = nf * m;
        gs_rank_keys_kernel<<<dim3(gs_blocks(n)), dim3(GS_THREADS), 0, s>>>(R.w.p, m, f0, n, k1.p, v1.p);
        HIPCHK(hipGetLastError());
        SGLCHK(gs_segmented_sort(s, k1.p, k2.p, v1.p, v2.p, m, nf, off.p, tmp, tmp_cap));
        gs_rank_scatter_kernel<<<dim3(gs_blocks(n)), dim3(GS_THREADS), 0, s>>>(R.w.p, v2.p, m, f0, n, R.pos.p, R.aw.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));   // the sort's buffers go
    return SGL_OK;
}

// stage 2: the three planes of observed scores (device, 3 P k) of the sets on the device
int gs_observed(sgl_ctx* c, const GsRank& R, const int64_t* dptr, const int32_t* dgenes, int64_t m, int64_t P, int64_t k, int s_max, double* des) {
    const int cap = (s_max + 1) & ~1;
    const size_t lds = (size_t)cap * sizeof(double) + (size_t)gs_pow2(s_max) * sizeof(int32_t);
    Phase ph(c, SGL_PH_SCALE);
    gs_es_kernel<<<dim3((unsigned)P, (unsigned)k), dim3(GS_WAVE), lds, c->stream>>>(R.pos.p, R.aw.p, dptr, dgenes, m, P, k, cap, des);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

struct GsSampler {
    DevBuf<gs_u64> k1, k2;
    DevBuf<int32_t> v1, v2;
    DevBuf<int64_t> off;
    DevBuf<char> tmp;
    size_t tmp_cap = 0;
    int64_t perms = 0;
    int alloc(int64_t m, int64_t batch) {
        perms = gsea_sort_perms(m, batch);
        const size_t items = (size_t)perms * (size_t)m;
        SGLCHK(k1.alloc(items));
        SGLCHK(k2.alloc(items));
        SGLCHK(v1.alloc(items));
        SGLCHK(v2.alloc(items));
        return off.alloc((size_t)perms + 1);
    }
};
// stage 3: sample[rl, 0 .. s_max) of the permutations [r0, r0 + nb)
int gs_sample(sgl_ctx* c, GsSampler& Q, uint64_t seed, int64_t r0, int64_t nb, int64_t m, int64_t s_max, int32_t* dsample) {
    hipStream_t s = c->stream;
    Phase ph(c, SGL_PH_SCALE);
    for (int64_t q0 = 0; q0 < nb; q0 += Q.perms) {
        const int64_t nq = std::min(Q.perms, nb - q0), n = nq * m;
        gs_sample_keys_kernel<<<dim3(gs_blocks(n)), dim3(GS_THREADS), 0, s>>>(seed, r0 + q0, m, n, Q.k1.p, Q.v1.p);
        HIPCHK(hipGetLastError());
        SGLCHK(gs_segmented_sort(s, Q.k1.p, Q.k2.p, Q.v1.p, Q.v2.p, m, nq, Q.off.p, Q.tmp, Q.tmp_cap));
        gs_sample_gather_kernel<<<dim3(gs_blocks(nq * s_max)), dim3(GS_THREADS), 0, s>>>(Q.v2.p, m, s_max, nq * s_max, dsample + q0 * s_max);
        HIPCHK(hipGetLastError());
    }
    return SGL_OK;
}

size_t gs_null_lds(int s_max) {
    return (size_t)gs_pow2(s_max) * sizeof(gs_u64) + (size_t)((s_max + 1) & ~1) * sizeof(double) + (size_t)s_max * sizeof(int32_t);
}
// stage 4: null[(f S + si) ld + rl] of the nb sampled permutations
int gs_null(sgl_ctx* c, const GsRank& R, const int32_t* dsample, const int32_t* dsizes, int S, int s_max, int64_t m, int64_t k, int64_t nb,
            int64_t ld, int score_type, double* dnull) {
    const size_t lds = gs_null_lds(s_max);
    SGLCHK(sgl_allow_dynamic_lds<&gs_null_kernel>((int)gs_null_lds(GSEA_LDS_CAP)));
    Phase ph(c, SGL_PH_SCALE);
    gs_null_kernel<<<dim3((unsigned)nb, (unsigned)k), dim3(GS_WAVE), lds, c->stream>>>(R.pos.p, R.aw.p, dsample, dsizes, S, s_max, m, ld, score_type,
                                                                                    dnull);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

void gs_record(sgl_ctx* c, int64_t sets, int64_t sizes, int64_t s_max, int64_t batches, int64_t batch) {
    const int64_t v[5] = {sets, sizes, s_max, batches, batch};
    std::copy(v, v + 5, c->gsea_last);
}

// the gene sets on the device (the copies are enqueued; the host arrays outlive the call)
struct GsSets {
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> genes;
    int upload(sgl_ctx* c, const int64_t* set_ptr, const int32_t* set_genes, int64_t P) {
        SGLCHK(ptr.alloc((size_t)P + 1));
        SGLCHK(genes.alloc((size_t)set_ptr[P]));
        HIPCHK(hipMemcpyAsync(ptr.p, set_ptr, sizeof(int64_t) * ((size_t)P + 1), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(genes.p, set_genes, sizeof(int32_t) * (size_t)set_ptr[P], hipMemcpyHostToDevice, c->stream));
        return SGL_OK;
    }
};
}   // namespace

static int gs_refuse(const char* who, GseaArgError e, int64_t m, int64_t k, int score_type, int64_t nperm, int64_t batch, int64_t at, int64_t val) {
    switch (e) {
    case GSEA_ARGS_OK: return SGL_OK;
    case GSEA_ARGS_NULL: sgl_set_error("%s: NULL w, set_ptr, set_genes or sizes", who); break;
    case GSEA_ARGS_K: sgl_set_error("%s: k = %lld is outside [1, %d]", who, (long long)k, GSEA_MAX_K); break;
    case GSEA_ARGS_GENES: sgl_set_error("%s: m = %lld genes: a ranking holds at least 2", who, (long long)m); break;
    case GSEA_ARGS_SETS: sgl_set_error("%s: no gene set (or no size) given", who); break;
    case GSEA_ARGS_SCORE: sgl_set_error("%s: score_type = %d is none of 0 (pos), 1 (neg), 2 (std)", who, score_type); break;
    case GSEA_ARGS_NPERM: sgl_set_error("%s: nperm = %lld is outside [1, %d]", who, (long long)nperm, (int)GSEA_MAX_NPERM); break;
    case GSEA_ARGS_BATCH: sgl_set_error("%s: batch = %lld is negative", who, (long long)batch); break;
    case GSEA_ARGS_W: sgl_set_error("%s: w[%lld, %lld] is not finite", who, (long long)(at % m), (long long)(at / m)); break;
    case GSEA_ARGS_PTR: sgl_set_error("%s: set_ptr[%lld] = %lld: set_ptr starts at 0 and ascends", who, (long long)at, (long long)val); break;
    case GSEA_ARGS_EMPTY: sgl_set_error("%s: set %lld is empty", who, (long long)at); break;
    case GSEA_ARGS_WHOLE: sgl_set_error("%s: set %lld holds %lld genes of %lld: a set is smaller than the ranking", who, (long long)at, (long long)val, (long long)m); break;
    case GSEA_ARGS_CAP: sgl_set_error("%s: set %lld holds %lld genes, above the cap of %d", who, (long long)at, (long long)val, GSEA_LDS_CAP); break;
    case GSEA_ARGS_GENE: sgl_set_error("%s: set_genes[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)m); break;
    case GSEA_ARGS_TWICE: sgl_set_error("%s: set_genes[%lld] = %lld occurs twice in its set", who, (long long)at, (long long)val); break;
    case GSEA_ARGS_SIZES: sgl_set_error("%s: sizes[%lld] = %lld: sizes ascend strictly within [1, min(m - 1, %d)]", who, (long long)at, (long long)val, GSEA_LDS_CAP); break;
    case GSEA_ARGS_RANGE: sgl_set_error("%s: permutations [%lld, %lld): not 0 <= r0 < r1 <= %d", who, (long long)at, (long long)val, (int)GSEA_MAX_NPERM); break;
    }
    return SGL_EINVAL;
}

int sgl_gsea_args_check(const char* who, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P,
                        int score_type, int64_t nperm, int64_t batch) {
    int64_t at = -1, val = 0;
    GseaArgError e = (!w || !set_ptr || !set_genes) ? GSEA_ARGS_NULL : gsea_check_scalars(m, k, score_type, nperm, batch);
    if (e == GSEA_ARGS_OK && P < 1) e = GSEA_ARGS_SETS;
    if (e == GSEA_ARGS_OK) e = gsea_check_w(w, m, k, &at);
    if (e == GSEA_ARGS_OK) {
        std::vector<int32_t> stamp((size_t)m);
        e = gsea_check_sets(set_ptr, set_genes, P, m, stamp.data(), &at, &val);
    }
    return gs_refuse(who, e, m, k, score_type, nperm, batch, at, val);
}

int sgl_gsea_null_args_check(const char* who, const double* w, int64_t m, int64_t k, const int32_t* sizes, int64_t n_sizes, int score_type,
                             int64_t r0, int64_t r1, int64_t batch) {
    int64_t at = -1, val = 0;
    GseaArgError e = !w ? GSEA_ARGS_NULL : gsea_check_scalars(m, k, score_type, 1, batch);
    if (e == GSEA_ARGS_OK && !(0 <= r0 && r0 < r1 && r1 <= GSEA_MAX_NPERM)) { e = GSEA_ARGS_RANGE; at = r0; val = r1; }
    if (e == GSEA_ARGS_OK) e = gsea_check_w(w, m, k, &at);
    if (e == GSEA_ARGS_OK) e = gsea_check_sizes(sizes, n_sizes, m, &at, &val);
    return gs_refuse(who, e, m, k, score_type, 1, batch, at, val);
}

static int gs_finish(sgl_ctx* c, int rc) {   // every return path waits for the stream before the buffers (and the host arrays) go
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("gsea: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

static int gs_es_on(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P, double* es3) {
    hipStream_t s = c->stream;
    int s_max = 0;
    for (int64_t j = 0; j < P; ++j) s_max = std::max(s_max, (int)(set_ptr[j + 1] - set_ptr[j]));
    GsRank R;
    SGLCHK(gs_rank(c, R, w, m, k));
    GsSets sets;
    DevBuf<double> des;
    SGLCHK(sets.upload(c, set_ptr, set_genes, P));
    SGLCHK(des.alloc(3 * (size_t)P * (size_t)k));
    SGLCHK(gs_observed(c, R, sets.ptr.p, sets.genes.p, m, P, k, s_max, des.p));
    HIPCHK(hipMemcpyAsync(es3, des.p, sizeof(double) * 3 * (size_t)P * (size_t)k, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    gs_record(c, P, 0, s_max, 0, 0);
    return SGL_OK;
}
int sgl_gsea_es(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P, double* es3) {
    return gs_finish(c, gs_es_on(c, w, m, k, set_ptr, set_genes, P, es3));
}

static int gs_null_on(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int32_t* sizes, int64_t S, int score_type, uint64_t seed, int64_t r0,
                      int64_t r1, int64_t batch, double* null_out, int32_t* sample) {
    hipStream_t s = c->stream;
    const int s_max = sizes[S - 1];
    const int64_t nperm = r1 - r0, B = gsea_batch_size(k, S, nperm, batch, 0), rows = k * S;
    GsRank R;
    SGLCHK(gs_rank(c, R, w, m, k));
    GsSampler Q;
    SGLCHK(Q.alloc(m, B));
    DevBuf<int32_t> dsizes, dsample;
    DevBuf<double> dnull;
    SGLCHK(dsizes.alloc((size_t)S));
    SGLCHK(dsample.alloc((size_t)B * (size_t)s_max));
    SGLCHK(dnull.alloc((size_t)rows * (size_t)B));
    HIPCHK(hipMemcpyAsync(dsizes.p, sizes, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, s));
    int64_t batches = 0;
    for (int64_t b0 = 0; b0 < nperm; b0 += B, ++batches) {
        const int64_t nb = std::min(B, nperm - b0);
        SGLCHK(gs_sample(c, Q, seed, r0 + b0, nb, m, s_max, dsample.p));
        SGLCHK(gs_null(c, R, dsample.p, dsizes.p, (int)S, s_max, m, k, nb, B, score_type, dnull.p));
        if (null_out)   // row (f, si) of the batch into its place among the nperm columns
            HIPCHK(hipMemcpy2DAsync(null_out + b0, sizeof(double) * (size_t)nperm, dnull.p, sizeof(double) * (size_t)B, sizeof(double) * (size_t)nb,
                                    (size_t)rows, hipMemcpyDeviceToHost, s));
        if (sample) HIPCHK(hipMemcpyAsync(sample + b0 * s_max, dsample.p, sizeof(int32_t) * (size_t)nb * (size_t)s_max, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    gs_record(c, 0, S, s_max, batches, B);
    return SGL_OK;
}
int sgl_gsea_null(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int32_t* sizes, int64_t S, int score_type, uint64_t seed, int64_t r0,
                  int64_t r1, int64_t batch, double* null_out, int32_t* sample) {
    return gs_finish(c, gs_null_on(c, w, m, k, sizes, S, score_type, seed, r0, r1, batch, null_out, sample));
}

static int gs_all_on(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P, int score_type,
                     int64_t nperm, uint64_t seed, int64_t batch, double* es, double* nes, double* pval, double* padj, int64_t* n_ge, int64_t* n_le,
                     int64_t* n_side, int32_t* set_size, double* stage_ms) {
    hipStream_t s = c->stream;
    const size_t pk = (size_t)P * (size_t)k;
    std::vector<int32_t> sizes((size_t)P), size_idx((size_t)P);
    const int64_t S = gsea_size_table(set_ptr, P, sizes.data(), size_idx.data(), set_size);
    const int s_max = sizes[(size_t)S - 1];
    const int64_t B = gsea_batch_size(k, S, nperm, batch, 0), rows = k * S;
    if (stage_ms) std::fill(stage_ms, stage_ms + 5, 0.0);
    GsTimer T(s, stage_ms);
    // 1. rankings
    GsRank R;
    T.begin();
    SGLCHK(gs_rank(c, R, w, m, k));
    T.end(0);
    // 2. observed scores
    GsSets sets;
    DevBuf<int32_t> dsizes, dsize_idx, dsample;
    DevBuf<double> des3, dnull, dsum;
    DevBuf<gs_u64> dcnt;
    SGLCHK(sets.upload(c, set_ptr, set_genes, P));
    SGLCHK(dsizes.alloc((size_t)S));
    SGLCHK(dsize_idx.alloc((size_t)P));
    SGLCHK(des3.alloc(3 * pk));
    SGLCHK(dcnt.alloc(2 * pk + 2 * (size_t)rows));   // n_ge, n_le | cnt_pos, cnt_neg
    SGLCHK(dsum.alloc(2 * (size_t)rows));            // sum_pos | sum_neg
    HIPCHK(hipMemcpyAsync(dsizes.p, sizes.data(), sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dsize_idx.p, size_idx.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dcnt.p, 0, sizeof(gs_u64) * (2 * pk + 2 * (size_t)rows), s));
    HIPCHK(hipMemsetAsync(dsum.p, 0, sizeof(double) * 2 * (size_t)rows, s));   // +0.0
    T.begin();
    SGLCHK(gs_observed(c, R, sets.ptr.p, sets.genes.p, m, P, k, s_max, des3.p));
    T.end(1);
    const double* des = des3.p + (size_t)score_type * pk;
    // 3 - 5. the permutations in batches
    GsSampler Q;
    SGLCHK(Q.alloc(m, B));
    SGLCHK(dsample.alloc((size_t)B * (size_t)s_max));
    SGLCHK(dnull.alloc((size_t)rows * (size_t)B));
    int64_t batches = 0;
    for (int64_t b0 = 0; b0 < nperm; b0 += B, ++batches) {
        const int64_t nb = std::min(B, nperm - b0);
        T.begin();
        SGLCHK(gs_sample(c, Q, seed, b0, nb, m, s_max, dsample.p));
        T.end(2);
        T.begin();
        SGLCHK(gs_null(c, R, dsample.p, dsizes.p, (int)S, s_max, m, k, nb, B, score_type, dnull.p));
        T.end(3);
        T.begin();
        {
            Phase ph(c, SGL_PH_SCALE);
            gs_tally_sets_kernel<<<dim3(gs_blocks((int64_t)pk)), dim3(GS_THREADS), 0, s>>>(des, dsize_idx.p, dnull.p, P, k, S, B, nb, dcnt.p, dcnt.p + pk);
            HIPCHK(hipGetLastError());
            gs_tally_sizes_kernel<<<dim3(gs_blocks(rows)), dim3(GS_THREADS), 0, s>>>(dnull.p, rows, B, nb, dcnt.p + 2 * pk, dcnt.p + 2 * pk + rows, dsum.p,
                                                                                   dsum.p + rows);
            HIPCHK(hipGetLastError());
        }
        T.end(4);
    }
    std::vector<double> hes(pk), hsum(2 * (size_t)rows), hp(pk);
    std::vector<int64_t> hcnt(2 * pk + 2 * (size_t)rows);
    HIPCHK(hipMemcpyAsync(hes.data(), des, sizeof(double) * pk, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hsum.data(), dsum.p, sizeof(double) * hsum.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hcnt.data(), dcnt.p, sizeof(int64_t) * hcnt.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    gsea_derive(P, k, score_type, nperm, size_idx.data(), S, hes.data(), hcnt.data(), hcnt.data() + pk, hcnt.data() + 2 * pk, hcnt.data() + 2 * pk + rows,
                hsum.data(), hsum.data() + rows, nes, hp.data(), n_side);
    if (padj)
        for (int64_t f = 0; f < k; ++f) gsea_bh(hp.data() + (size_t)P * (size_t)f, P, padj + (size_t)P * (size_t)f);
    if (es) std::copy(hes.begin(), hes.end(), es);
    if (pval) std::copy(hp.begin(), hp.end(), pval);
    if (n_ge) std::copy(hcnt.begin(), hcnt.begin() + pk, n_ge);
    if (n_le) std::copy(hcnt.begin() + pk, hcnt.begin() + 2 * pk, n_le);
    gs_record(c, P, S, s_max, batches, B);
    return SGL_OK;
}
int sgl_gsea_all(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P, int score_type,
                 int64_t nperm, uint64_t seed, int64_t batch, double* es, double* nes, double* pval, double* padj, int64_t* n_ge, int64_t* n_le,
                 int64_t* n_side, int32_t* set_size, double* stage_ms) {
    return gs_finish(c, gs_all_on(c, w, m, k, set_ptr, set_genes, P, score_type, nperm, seed, batch, es, nes, pval, padj, n_ge, n_le, n_side, set_size,
                                  stage_ms));
}
