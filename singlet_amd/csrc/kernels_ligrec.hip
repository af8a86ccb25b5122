// Ligand-receptor interactions between clusters (include/singlet_hip.h, "Ligand-receptor interactions"): the per-class sums of the
// listed genes under the caller's labels and under nperm relabellings, the scores of the pairs and how often a relabelling reaches
// the observed score.  This file holds
//   1. the labels: the interleaved tables of kernels_nhood.hip (groups of 16 label vectors, 16 adjacent bytes per cell) -- the
//      same keys, sorts and gather, so vector r is sgl_op_nhood_permute's lab_r.
//   2. lr_sums_kernel: one wave owns (one segment of a gene's stored entries, a group of up to 64 label vectors), lane l owns
//      vector l of the group.  The wave walks the segment in stored order -- 64 entries per coalesced load, handed round by
//      readlane -- and every lane adds the value to ITS OWN bin [class][lane] of the wave's bins, in LDS (lane-fastest: no bank
//      conflict) or, on the global path, in a scratch of the same shape.  That is the sequential order of the rules: no atomics,
//      no butterflies, no barrier (a lane touches no other lane's bins).  The segment partials go to scratch as [segment][class]
//      [vector].
//   3. lr_finish_kernel: one thread per (gene, class, vector) adds the gene's segment partials in ascending order from +0.0 and
//      divides by the class size.
//   4. lr_nz_kernel (observed only; integer atomics), lr_score_kernel, lr_tally_kernel: one thread per (q, a, b) walks the batch's
//      mean tables and carries n_ge from batch to batch.
#include "sgl_internal.h"
#include "ligrec_host.h"

#define LR_THREADS 256   // the element-wise kernels
#define LR_AHEAD 8       // label loads of the sums kernel in flight per lane

typedef unsigned long long lr_u64;

// ---- 2. the sums ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double lr_readlane_f64(double v, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// x / idx: the values and cells of At's stored entries.  seg_begin / seg_end: nseg entry ranges of at most LIGREC_SEG entries.
// lab8: the interleaved labels of nvec vectors (every byte < K; the cells in [0, n) by the matrix's own validation).  Work item
// (segment s, group w), w fastest: the waves of a segment share its entries in the cache.  part[(s K + c) nvec + v].
// gbins (global path): K x vpw doubles per wave of the grid.
template <bool LDS>
__global__ __launch_bounds__(LIGREC_MAX_WAVES * SGL_WAVE) void lr_sums_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                             const int64_t* __restrict__ seg_begin,
                                                                             const int64_t* __restrict__ seg_end, int64_t nseg,
                                                                             const uint8_t* __restrict__ lab8, int64_t n, int K, int vpw, int64_t nvec,
                                                                             double* __restrict__ gbins, double* __restrict__ part) {
    extern __shared__ double lr_lds[];
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)(blockDim.x >> 6);
    const int64_t wave_id = (int64_t)blockIdx.x * waves + wave, grid_waves = (int64_t)gridDim.x * waves;
    const int64_t groups = (nvec + vpw - 1) / vpw, items = nseg * groups;
    double* __restrict__ bins = LDS ? lr_lds + (size_t)wave * (size_t)K * (size_t)vpw : gbins + (size_t)wave_id * (size_t)K * (size_t)vpw;
    for (int64_t item = wave_id; item < items; item += grid_waves) {
        const int64_t s = item / groups, w = item % groups;
        const int64_t v = w * vpw + lane;
        const bool on = lane < vpw && v < nvec;
        if (on)
            for (int c = 0; c < K; ++c) bins[c * vpw + lane] = 0.0;
        const uint8_t* __restrict__ L = lab8 + (size_t)(on ? v >> 4 : 0) * (size_t)n * 16 + (size_t)(on ? v & 15 : 0);
        const int64_t e1 = seg_end[s];
        for (int64_t e0 = seg_begin[s]; e0 < e1; e0 += SGL_WAVE) {
            const int cnt = (int)(e1 - e0 < SGL_WAVE ? e1 - e0 : SGL_WAVE);
            int32_t my_cell = 0;
            double my_x = 0.0;
            if (lane < cnt) {
                my_cell = idx[e0 + lane];
                my_x = x[e0 + lane];
            }
            // eight label loads in flight, then the eight additions in stored order (the bins may be one and the same: the
            // additions stay sequential)
            int j = 0;
            for (; j + LR_AHEAD <= cnt; j += LR_AHEAD) {
                int c[LR_AHEAD];
#pragma unroll
                for (int u = 0; u < LR_AHEAD; ++u) c[u] = on ? L[(size_t)__builtin_amdgcn_readlane(my_cell, j + u) * 16] : 0;
#pragma unroll
                for (int u = 0; u < LR_AHEAD; ++u) {
                    const double val = lr_readlane_f64(my_x, j + u);
                    if (on) bins[c[u] * vpw + lane] += val;
                }
            }
            for (; j < cnt; ++j) {
                const int64_t cell = __builtin_amdgcn_readlane(my_cell, j);
                const double val = lr_readlane_f64(my_x, j);
                if (on) {
                    const int c = L[(size_t)cell * 16];
                    bins[c * vpw + lane] += val;
                }
            }
        }
        if (on)
            for (int c = 0; c < K; ++c) part[((size_t)s * (size_t)K + (size_t)c) * (size_t)nvec + (size_t)v] = bins[c * vpw + lane];
    }
}

// ---- 3. segment partials -> sums and means ----------------------------------------------------------------------------------------
// sum_out / mean_out[(v G + g) K + c]; either may be NULL
__global__ __launch_bounds__(LR_THREADS) void lr_finish_kernel(const double* __restrict__ part, const int64_t* __restrict__ seg_first, int64_t G, int K,
                                                              int64_t nvec, const int64_t* __restrict__ group_n, double* __restrict__ sum_out,
                                                              double* __restrict__ mean_out) {
    const int64_t t = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (t >= G * K * nvec) return;
    const int64_t v = t % nvec, c = (t / nvec) % K, g = t / (nvec * K);
    double acc = 0.0;
    for (int64_t s = seg_first[g]; s < seg_first[g + 1]; ++s) acc += part[((size_t)s * (size_t)K + (size_t)c) * (size_t)nvec + (size_t)v];
    const size_t at = ((size_t)v * (size_t)G + (size_t)g) * (size_t)K + (size_t)c;
    if (sum_out) sum_out[at] = acc;
    if (mean_out) mean_out[at] = acc / (double)group_n[c];
}

// ---- 4. the rest ------------------------------------------------------------------------------------------------------------------
// range[2 g], range[2 g + 1] = the stored entries of listed gene g
__global__ __launch_bounds__(LR_THREADS) void lr_ranges_kernel(const int64_t* __restrict__ p, const int32_t* __restrict__ genes, int64_t G,
                                                              int64_t* __restrict__ range) {
    const int64_t g = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (g >= G) return;
    range[2 * g] = p[genes[g]];
    range[2 * g + 1] = p[genes[g] + 1];
}

// nz[g K + c] += the stored x != 0 of listed gene g in class c; one workgroup per gene; nz zero on entry
__global__ __launch_bounds__(LR_THREADS) void lr_nz_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx, const int64_t* __restrict__ range,
                                                          const int32_t* __restrict__ lab, int K, lr_u64* __restrict__ nz) {
    const int64_t g = blockIdx.x;
    for (int64_t e = range[2 * g] + threadIdx.x; e < range[2 * g + 1]; e += LR_THREADS)
        if (x[e] != 0.0) atomicAdd(&nz[(size_t)g * (size_t)K + (size_t)lab[idx[e]]], 1ull);
}

// (a NaN mean compares false)
__device__ __forceinline__ double lr_score(double ma, double mb) { return (ma > 0.0 && mb > 0.0) ? 0.5 * (ma + mb) : 0.0; }

// score[q + P (a + K b)] of one mean table
__global__ __launch_bounds__(LR_THREADS) void lr_score_kernel(const double* __restrict__ mean, const int32_t* __restrict__ lig, const int32_t* __restrict__ rec,
                                                             int64_t P, int K, double* __restrict__ score) {
    const int64_t t = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (t >= P * K * K) return;
    const int64_t q = t % P, a = (t / P) % K, b = t / (P * K);
    score[t] = lr_score(mean[(size_t)lig[q] * K + a], mean[(size_t)rec[q] * K + b]);
}

// means: nb tables of G x K; n_ge carried from batch to batch; null (nb x P K K) may be NULL
__global__ __launch_bounds__(LR_THREADS) void lr_tally_kernel(const double* __restrict__ score, const double* __restrict__ means, int64_t nb, int64_t G,
                                                             const int32_t* __restrict__ lig, const int32_t* __restrict__ rec, int64_t P, int K,
                                                             int64_t* __restrict__ n_ge, double* __restrict__ null) {
    const int64_t PKK = P * K * K;
    const int64_t t = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
    if (t >= PKK) return;
    const int64_t q = t % P, a = (t / P) % K, b = t / (P * K);
    const size_t ia = (size_t)lig[q] * K + a, ib = (size_t)rec[q] * K + b;
    const double s = score[t];
    int64_t ge = n_ge[t];
    for (int64_t r = 0; r < nb; ++r) {
        const double* __restrict__ M = means + (size_t)r * (size_t)G * (size_t)K;
        const double sr = lr_score(M[ia], M[ib]);
        ge += sr >= s;
        if (null) null[(size_t)r * (size_t)PKK + (size_t)t] = sr;
    }
    n_ge[t] = ge;
}

// =================================================================================================================================
namespace {
inline unsigned lr_blocks(int64_t n) { return (unsigned)((n + LR_THREADS - 1) / LR_THREADS); }

struct LrTimer {   // stage_ms of sgl_c_ligrec: events around a stage when the caller asked for the times
    hipStream_t s;
    double* ms;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    LrTimer(hipStream_t s_, double* ms_) : s(s_), ms(ms_) {
        if (ms && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) { (void)hipGetLastError(); ms = nullptr; }
    }
    ~LrTimer() {
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

struct LabellerHolder {
    sgl_nhood_labeller* h = nullptr;
    ~LabellerHolder() { if (h) sgl_nhood_labeller_free(h); }
};

// the listed genes on the device, their entry ranges and the segments
struct LrGenes {
    DevBuf<int32_t> genes;
    DevBuf<int64_t> range, seg_first, seg_begin, seg_end;
    std::vector<int64_t> h_range, h_first, h_begin, h_end;   // (the uploads read them: they live as long as the struct)
    int64_t G = 0, nseg = 0;
    int build(sgl_ctx* c, const int32_t* hgenes, int64_t G_) {
        hipStream_t s = c->stream;
        G = G_;
        SGLCHK(genes.alloc((size_t)G));
        SGLCHK(range.alloc(2 * (size_t)G));
        HIPCHK(hipMemcpyAsync(genes.p, hgenes, sizeof(int32_t) * (size_t)G, hipMemcpyHostToDevice, s));
        lr_ranges_kernel<<<dim3(lr_blocks(G)), dim3(LR_THREADS), 0, s>>>(c->At.p, genes.p, G, range.p);
        HIPCHK(hipGetLastError());
        h_range.resize(2 * (size_t)G);
        HIPCHK(hipMemcpyAsync(h_range.data(), range.p, sizeof(int64_t) * h_range.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ligrec_segments(h_range.data(), G, h_first, h_begin, h_end);
        nseg = (int64_t)h_begin.size();
        SGLCHK(seg_first.alloc((size_t)G + 1));
        SGLCHK(seg_begin.alloc((size_t)nseg));
        SGLCHK(seg_end.alloc((size_t)nseg));
        HIPCHK(hipMemcpyAsync(seg_first.p, h_first.data(), sizeof(int64_t) * ((size_t)G + 1), hipMemcpyHostToDevice, s));
        if (nseg > 0) {
            HIPCHK(hipMemcpyAsync(seg_begin.p, h_begin.data(), sizeof(int64_t) * (size_t)nseg, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(seg_end.p, h_end.data(), sizeof(int64_t) * (size_t)nseg, hipMemcpyHostToDevice, s));
        }
        return SGL_OK;
    }
};

// the scratch of the sums of up to `cap` vectors at a time
struct LrScratch {
    DevBuf<double> part, gbins;
    int64_t grid_waves = 0;
    int alloc(const LrGenes& Q, const LigrecPlan& P, int K, int64_t cap) {
        SGLCHK(part.alloc((size_t)Q.nseg * (size_t)K * (size_t)cap));
        const int64_t groups = (cap + P.vpw - 1) / P.vpw;
        const int64_t limit = P.path == 2 ? LIGREC_GRID_WAVES / 4 : LIGREC_GRID_WAVES;
        grid_waves = std::max<int64_t>(std::min(Q.nseg * groups, limit), 1);
        grid_waves = (grid_waves + P.waves - 1) / P.waves * P.waves;
        if (P.path == 2) SGLCHK(gbins.alloc((size_t)grid_waves * (size_t)K * (size_t)P.vpw));
        return SGL_OK;
    }
};

// sum_out / mean_out (nvec x G x K on the device, either may be NULL) of the nvec label vectors of lab8
int lr_sums(sgl_ctx* c, const LrGenes& Q, const LigrecPlan& P, LrScratch& S, const uint8_t* lab8, int64_t n, int K, int64_t nvec, const int64_t* group_n,
            double* sum_out, double* mean_out) {
    hipStream_t s = c->stream;
    Phase ph(c, SGL_PH_SCALE);
    if (Q.nseg > 0) {
        const int64_t groups = (nvec + P.vpw - 1) / P.vpw;
        const int64_t want = (std::min(Q.nseg * groups, S.grid_waves) + P.waves - 1) / P.waves;
        const dim3 grid((unsigned)std::max<int64_t>(want, 1)), block((unsigned)(P.waves * SGL_WAVE));
        if (P.path == 1) {
            SGLCHK((sgl_allow_dynamic_lds<&lr_sums_kernel<true>>((int)LIGREC_WG_LDS_BYTES)));
            lr_sums_kernel<true><<<grid, block, (size_t)P.lds_bytes, s>>>(c->At.x, c->At.i, Q.seg_begin.p, Q.seg_end.p, Q.nseg, lab8, n, K, P.vpw, nvec, nullptr,
                                                                          S.part.p);
        } else {
            lr_sums_kernel<false><<<grid, block, 0, s>>>(c->At.x, c->At.i, Q.seg_begin.p, Q.seg_end.p, Q.nseg, lab8, n, K, P.vpw, nvec, S.gbins.p, S.part.p);
        }
        HIPCHK(hipGetLastError());
    }
    lr_finish_kernel<<<dim3(lr_blocks(Q.G * K * nvec)), dim3(LR_THREADS), 0, s>>>(S.part.p, Q.seg_first.p, Q.G, K, nvec, group_n, sum_out, mean_out);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

void lr_record(sgl_ctx* c, const LigrecPlan& P, int64_t batches, int64_t batch, int64_t G) {
    const int64_t v[8] = {P.path, P.vpw, batches, batch, P.lds_bytes, P.waves, P.path == 1 ? G : 0, P.path == 2 ? G : 0};
    std::copy(v, v + 8, c->ligrec_last);
}

inline int64_t lr_groups16(int64_t nvec) { return (nvec + 15) / 16; }
}   // namespace

static int lr_refuse(const char* who, LigrecArgError e, int64_t K, int64_t m, int64_t G, int64_t ncol, int64_t at, int64_t val) {
    switch (e) {
    case LIGREC_ARGS_OK: return SGL_OK;
    case LIGREC_ARGS_NULL: sgl_set_error("%s: NULL lab, genes, lig, rec or another input array", who); break;
    case LIGREC_ARGS_K: sgl_set_error("%s: K = %lld is outside [1, %d]", who, (long long)val, LIGREC_MAX_K); break;
    case LIGREC_ARGS_G: sgl_set_error("%s: G = %lld is outside [1, %lld] (the genes of the matrix)", who, (long long)val, (long long)m); break;
    case LIGREC_ARGS_P: sgl_set_error("%s: P = %lld: at least one pair", who, (long long)val); break;
    case LIGREC_ARGS_NPERM: sgl_set_error("%s: nperm = %lld is outside [1, %lld]", who, (long long)val, (long long)LIGREC_MAX_NPERM); break;
    case LIGREC_ARGS_LABEL: sgl_set_error("%s: lab[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)K); break;
    case LIGREC_ARGS_GENE: sgl_set_error("%s: genes[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)m); break;
    case LIGREC_ARGS_GENE_TWICE: sgl_set_error("%s: genes[%lld] = %lld is listed twice", who, (long long)at, (long long)val); break;
    case LIGREC_ARGS_LIG: sgl_set_error("%s: lig[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)G); break;
    case LIGREC_ARGS_REC: sgl_set_error("%s: rec[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)G); break;
    case LIGREC_ARGS_THRESHOLD: sgl_set_error("%s: threshold is outside [0, 1]", who); break;
    case LIGREC_ARGS_BATCH: sgl_set_error("%s: batch = %lld is negative", who, (long long)val); break;
    case LIGREC_ARGS_N: sgl_set_error("%s: n = %lld labels, the matrix has %lld cells", who, (long long)val, (long long)ncol); break;
    case LIGREC_ARGS_PATH: sgl_set_error("%s: path = %lld is none of 0 (automatic), 1 (LDS), 2 (global)", who, (long long)val); break;
    case LIGREC_ARGS_VPW:
        sgl_set_error("%s: vectors_per_wave = %lld is no power of two in [1, %lld] (what a wave holds at K = %lld)", who, (long long)val, (long long)at,
                      (long long)K);
        break;
    case LIGREC_ARGS_NB: sgl_set_error("%s: nb = %lld: at least one label vector", who, (long long)val); break;
    }
    return SGL_EINVAL;
}

int sgl_ligrec_args_check(const char* who, const int32_t* lab, int64_t n, int64_t K, const int32_t* genes, int64_t G, int64_t m, const int32_t* lig,
                          const int32_t* rec, int64_t P, int64_t nperm, double threshold, int64_t batch, int64_t ncol) {
    int64_t at = -1, val = 0;
    const LigrecArgError e = ligrec_check_call(lab, n, K, genes, G, m, lig, rec, P, nperm, threshold, batch, ncol, &at, &val);
    return lr_refuse(who, e, K, m, G, ncol, at, val);
}

int sgl_ligrec_sums_args_check(const char* who, const int32_t* labs, int64_t n, int64_t nb, int64_t K, const int32_t* genes, int64_t G, int64_t m,
                               int path, int64_t vpw, int64_t ncol) {
    int64_t at = -1, val = 0;
    LigrecArgError e = LIGREC_ARGS_OK;
    if (!labs || !genes) e = LIGREC_ARGS_NULL;
    else if (K < 1 || K > LIGREC_MAX_K) { e = LIGREC_ARGS_K; val = K; }
    else if (G < 1 || G > m) { e = LIGREC_ARGS_G; val = G; }
    else if (nb < 1 || nb > LIGREC_MAX_NPERM + 1) { e = LIGREC_ARGS_NB; val = nb; }
    if (e == LIGREC_ARGS_OK) e = ligrec_check_labels(labs, n > 0 ? n : 0, nb, K, &at, &val);
    if (e == LIGREC_ARGS_OK) e = ligrec_check_genes(genes, G, m, &at, &val);
    if (e == LIGREC_ARGS_OK) {
        LigrecPlan P;
        e = ligrec_plan(n, K, G, 0, nb, 0, path, vpw, &P, &at, &val);
    }
    if (e == LIGREC_ARGS_OK && n != ncol) { e = LIGREC_ARGS_N; val = n; }
    return lr_refuse(who, e, K, m, G, ncol, at, val);
}

int sgl_ligrec_tally_args_check(const char* who, const double* mean_obs, const double* means, int64_t nb, int64_t K, int64_t G, const int32_t* lig,
                                const int32_t* rec, int64_t P) {
    int64_t at = -1, val = 0;
    LigrecArgError e = LIGREC_ARGS_OK;
    if (!mean_obs || !means || !lig || !rec) e = LIGREC_ARGS_NULL;
    else if (K < 1 || K > LIGREC_MAX_K) { e = LIGREC_ARGS_K; val = K; }
    else if (G < 1) { e = LIGREC_ARGS_G; val = G; }
    else if (P < 1) { e = LIGREC_ARGS_P; val = P; }
    else if (nb < 1 || nb > LIGREC_MAX_NPERM) { e = LIGREC_ARGS_NB; val = nb; }
    if (e == LIGREC_ARGS_OK) e = ligrec_check_pairs(lig, rec, P, G, &at, &val);
    return lr_refuse(who, e, K, INT32_MAX, G, 0, at, val);
}

static int lr_finish(sgl_ctx* c, int rc) {   // every return path waits for the stream before the buffers (and the host arrays) go
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("ligrec: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

// ---- the sums of given label vectors ----------------------------------------------------------------------------------------------
static int lr_sums_on(sgl_ctx* c, const int32_t* labs, int64_t nb, int K, const int32_t* genes, int64_t G, int path, int64_t vpw, double* sum_out) {
    hipStream_t s = c->stream;
    const int64_t n = c->At.nrow;
    LrGenes Q;
    SGLCHK(Q.build(c, genes, G));
    LigrecPlan P;
    int64_t at, val;
    if (ligrec_plan(n, K, G, Q.nseg, nb, 0, path, vpw, &P, &at, &val) != LIGREC_ARGS_OK) { sgl_set_error("ligrec: the plan refused knobs the check accepted"); return SGL_EINVAL; }
    // the label vectors in chunks within the batch budget: 5 n bytes of labels (int32 and interleaved) and the plan's share per vector
    int64_t chunk = std::max<int64_t>(LIGREC_BATCH_BYTES / (5 * n + (Q.nseg + 2 * G) * K * 8), 1);
    chunk = std::max<int64_t>(chunk - chunk % LIGREC_MAX_VPW, LIGREC_MAX_VPW);
    chunk = std::min(chunk, nb);
    DevBuf<int32_t> dlabs;
    DevBuf<uint8_t> d8;
    DevBuf<double> dsum;
    DevBuf<int64_t> dn;
    LrScratch S;
    SGLCHK(dlabs.alloc((size_t)chunk * (size_t)n));
    SGLCHK(d8.alloc((size_t)lr_groups16(chunk) * 16 * (size_t)n));
    SGLCHK(dsum.alloc((size_t)chunk * (size_t)G * (size_t)K));
    SGLCHK(dn.alloc((size_t)K));
    SGLCHK(S.alloc(Q, P, K, chunk));
    HIPCHK(hipMemsetAsync(dn.p, 0, sizeof(int64_t) * (size_t)K, s));   // (no mean is asked for: the sizes are not read)
    int64_t batches = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += chunk, ++batches) {
        const int64_t nq = std::min(chunk, nb - b0);
        HIPCHK(hipMemcpyAsync(dlabs.p, labs + (size_t)b0 * (size_t)n, sizeof(int32_t) * (size_t)nq * (size_t)n, hipMemcpyHostToDevice, s));
        SGLCHK(sgl_nhood_labels_given(c, dlabs.p, n, n, nq, d8.p));
        SGLCHK(lr_sums(c, Q, P, S, d8.p, n, K, nq, dn.p, dsum.p, nullptr));
        if (sum_out) HIPCHK(hipMemcpyAsync(sum_out + (size_t)b0 * (size_t)G * (size_t)K, dsum.p, sizeof(double) * (size_t)nq * (size_t)G * (size_t)K, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    lr_record(c, P, batches, chunk, G);
    return SGL_OK;
}
int sgl_ligrec_sums_core(sgl_ctx* c, const int32_t* labs, int64_t nb, int K, const int32_t* genes, int64_t G, int path, int64_t vpw, double* sum_out) {
    return lr_finish(c, lr_sums_on(c, labs, nb, K, genes, G, path, vpw, sum_out));
}

// ---- the tally from means -----------------------------------------------------------------------------------------------------------
namespace {
// the pairs on the device and the carried tallies
struct LrPairs {
    DevBuf<int32_t> lig, rec;
    DevBuf<double> score, null;
    DevBuf<int64_t> n_ge;
    int64_t P = 0, PKK = 0, null_rows = 0;
    int build(sgl_ctx* c, const int32_t* hlig, const int32_t* hrec, int64_t P_, int K, bool want_null, int64_t nb_max) {
        hipStream_t s = c->stream;
        P = P_;
        PKK = P * K * K;
        SGLCHK(lig.alloc((size_t)P));
        SGLCHK(rec.alloc((size_t)P));
        SGLCHK(score.alloc((size_t)PKK));
        SGLCHK(n_ge.alloc((size_t)PKK));
        if (want_null) {
            null_rows = std::min(std::max<int64_t>(LIGREC_BATCH_BYTES / (PKK * 8), 1), nb_max);
            SGLCHK(null.alloc((size_t)null_rows * (size_t)PKK));
        }
        HIPCHK(hipMemcpyAsync(lig.p, hlig, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(rec.p, hrec, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(n_ge.p, 0, sizeof(int64_t) * (size_t)PKK, s));
        return SGL_OK;
    }
    int observe(sgl_ctx* c, const double* mean_obs, int K) {
        Phase ph(c, SGL_PH_SCALE);
        lr_score_kernel<<<dim3(lr_blocks(PKK)), dim3(LR_THREADS), 0, c->stream>>>(mean_obs, lig.p, rec.p, P, K, score.p);
        HIPCHK(hipGetLastError());
        return SGL_OK;
    }
    // the nb mean tables of a batch (device); null_out (host, may be NULL): the rows of these nb vectors
    int tally(sgl_ctx* c, const double* means, int64_t nb, int64_t G, int K, double* null_out) {
        hipStream_t s = c->stream;
        const int64_t step = null_out ? null_rows : nb;
        for (int64_t r0 = 0; r0 < nb; r0 += step) {
            const int64_t nr = std::min(step, nb - r0);
            {
                Phase ph(c, SGL_PH_SCALE);
                lr_tally_kernel<<<dim3(lr_blocks(PKK)), dim3(LR_THREADS), 0, s>>>(score.p, means + (size_t)r0 * (size_t)G * (size_t)K, nr, G, lig.p, rec.p, P, K,
                                                                                 n_ge.p, null_out ? null.p : nullptr);
                HIPCHK(hipGetLastError());
            }
            if (null_out) {
                HIPCHK(hipMemcpyAsync(null_out + (size_t)r0 * (size_t)PKK, null.p, sizeof(double) * (size_t)nr * (size_t)PKK, hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));   // (the next step writes the same rows)
            }
        }
        return SGL_OK;
    }
    int fetch(sgl_ctx* c, double* score_out, int64_t* n_ge_out) {
        hipStream_t s = c->stream;
        if (score_out) HIPCHK(hipMemcpyAsync(score_out, score.p, sizeof(double) * (size_t)PKK, hipMemcpyDeviceToHost, s));
        if (n_ge_out) HIPCHK(hipMemcpyAsync(n_ge_out, n_ge.p, sizeof(int64_t) * (size_t)PKK, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return SGL_OK;
    }
};
}   // namespace

static int lr_tally_on(sgl_ctx* c, const double* mean_obs, const double* means, int64_t nb, int K, int64_t G, const int32_t* lig, const int32_t* rec,
                       int64_t P, double* score_out, int64_t* n_ge_out, double* null_out) {
    hipStream_t s = c->stream;
    const int64_t GK = G * K;
    const int64_t chunk = std::min(std::max<int64_t>(LIGREC_BATCH_BYTES / (GK * 8), 1), nb);
    std::vector<double> h_score;
    std::vector<int64_t> h_ge;
    if (score_out) h_score.resize((size_t)(P * K * K));
    if (n_ge_out) h_ge.resize((size_t)(P * K * K));
    LrPairs T;
    DevBuf<double> dobs, dmeans;
    SGLCHK(T.build(c, lig, rec, P, K, null_out != nullptr, chunk));
    SGLCHK(dobs.alloc((size_t)GK));
    SGLCHK(dmeans.alloc((size_t)chunk * (size_t)GK));
    HIPCHK(hipMemcpyAsync(dobs.p, mean_obs, sizeof(double) * (size_t)GK, hipMemcpyHostToDevice, s));
    SGLCHK(T.observe(c, dobs.p, K));
    for (int64_t b0 = 0; b0 < nb; b0 += chunk) {
        const int64_t nq = std::min(chunk, nb - b0);
        HIPCHK(hipMemcpyAsync(dmeans.p, means + (size_t)b0 * (size_t)GK, sizeof(double) * (size_t)nq * (size_t)GK, hipMemcpyHostToDevice, s));
        SGLCHK(T.tally(c, dmeans.p, nq, G, K, null_out ? null_out + (size_t)b0 * (size_t)T.PKK : nullptr));
        HIPCHK(hipStreamSynchronize(s));
    }
    SGLCHK(T.fetch(c, score_out ? h_score.data() : nullptr, n_ge_out ? h_ge.data() : nullptr));
    if (score_out) std::copy(h_score.begin(), h_score.end(), score_out);
    if (n_ge_out) std::copy(h_ge.begin(), h_ge.end(), n_ge_out);
    return SGL_OK;
}
int sgl_ligrec_tally_core(sgl_ctx* c, const double* mean_obs, const double* means, int64_t nb, int K, int64_t G, const int32_t* lig,
                          const int32_t* rec, int64_t P, double* score_out, int64_t* n_ge_out, double* null_out) {
    return lr_finish(c, lr_tally_on(c, mean_obs, means, nb, K, G, lig, rec, P, score_out, n_ge_out, null_out));
}

// ---- the whole call ---------------------------------------------------------------------------------------------------------------
static int lr_all_on(sgl_ctx* c, const int32_t* lab, int K, const int32_t* genes, int64_t G, const int32_t* lig, const int32_t* rec, int64_t P,
                     int64_t nperm, uint64_t seed, int64_t batch, int64_t* group_n, int64_t* nz, double* sum, double* mean, double* score, int64_t* n_ge,
                     double* null_out, double* stage_ms) {
    hipStream_t s = c->stream;
    const int64_t n = c->At.nrow, GK = G * K;
    if (stage_ms) std::fill(stage_ms, stage_ms + 3, 0.0);
    LrTimer T(s, stage_ms);
    std::vector<int64_t> h_n((size_t)K, 0);
    for (int64_t q = 0; q < n; ++q) ++h_n[(size_t)lab[q]];
    LrGenes Q;
    SGLCHK(Q.build(c, genes, G));
    LigrecPlan Pl;
    int64_t at, val;
    if (ligrec_plan(n, K, G, Q.nseg, nperm, batch, 0, 0, &Pl, &at, &val) != LIGREC_ARGS_OK) { sgl_set_error("ligrec: the plan refused a batch the check accepted"); return SGL_EINVAL; }
    const int64_t B = Pl.batch;
    DevBuf<int32_t> dlab;
    DevBuf<uint8_t> d8;
    DevBuf<int64_t> dn, dnz;
    DevBuf<double> dobs, dmeans;   // sum | mean of the observed vector; the batch's mean tables
    LrScratch S;
    LrPairs Tp;
    LabellerHolder H;
    SGLCHK(dlab.alloc((size_t)n));
    SGLCHK(d8.alloc((size_t)lr_groups16(B) * 16 * (size_t)n));
    SGLCHK(dn.alloc((size_t)K));
    SGLCHK(dnz.alloc((size_t)GK));
    SGLCHK(dobs.alloc(2 * (size_t)GK));
    SGLCHK(dmeans.alloc((size_t)B * (size_t)GK));
    SGLCHK(S.alloc(Q, Pl, K, B));
    SGLCHK(Tp.build(c, lig, rec, P, K, null_out != nullptr, B));
    SGLCHK(sgl_nhood_labeller_create(c, n, B, &H.h));
    HIPCHK(hipMemcpyAsync(dlab.p, lab, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dn.p, h_n.data(), sizeof(int64_t) * (size_t)K, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dnz.p, 0, sizeof(int64_t) * (size_t)GK, s));
    // the observed vector: the identity, alone in its table
    T.begin();
    SGLCHK(sgl_nhood_labels_given(c, dlab.p, 0, n, 1, d8.p));
    T.end(0);
    T.begin();
    SGLCHK(lr_sums(c, Q, Pl, S, d8.p, n, K, 1, dn.p, dobs.p, dobs.p + GK));
    {
        Phase ph(c, SGL_PH_SCALE);
        lr_nz_kernel<<<dim3((unsigned)G), dim3(LR_THREADS), 0, s>>>(c->At.x, c->At.i, Q.range.p, dlab.p, K, reinterpret_cast<lr_u64*>(dnz.p));
        HIPCHK(hipGetLastError());
    }
    T.end(1);
    T.begin();
    SGLCHK(Tp.observe(c, dobs.p + GK, K));
    T.end(2);
    int64_t batches = 0;
    for (int64_t b0 = 0; b0 < nperm; b0 += B, ++batches) {
        const int64_t nb = std::min(B, nperm - b0);
        T.begin();
        SGLCHK(sgl_nhood_labels_permuted(c, H.h, dlab.p, n, seed, b0, nb, d8.p));
        T.end(0);
        T.begin();
        SGLCHK(lr_sums(c, Q, Pl, S, d8.p, n, K, nb, dn.p, nullptr, dmeans.p));
        T.end(1);
        T.begin();
        SGLCHK(Tp.tally(c, dmeans.p, nb, G, K, null_out ? null_out + (size_t)b0 * (size_t)Tp.PKK : nullptr));
        T.end(2);
    }
    std::vector<double> h_obs(2 * (size_t)GK), h_score(score ? (size_t)Tp.PKK : 0);
    std::vector<int64_t> h_nz((size_t)GK), h_ge(n_ge ? (size_t)Tp.PKK : 0);
    HIPCHK(hipMemcpyAsync(h_obs.data(), dobs.p, sizeof(double) * h_obs.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_nz.data(), dnz.p, sizeof(int64_t) * h_nz.size(), hipMemcpyDeviceToHost, s));
    SGLCHK(Tp.fetch(c, score ? h_score.data() : nullptr, n_ge ? h_ge.data() : nullptr));
    if (group_n) std::copy(h_n.begin(), h_n.end(), group_n);
    if (nz) std::copy(h_nz.begin(), h_nz.end(), nz);
    if (sum) std::copy(h_obs.begin(), h_obs.begin() + GK, sum);
    if (mean) std::copy(h_obs.begin() + GK, h_obs.end(), mean);
    if (score) std::copy(h_score.begin(), h_score.end(), score);
    if (n_ge) std::copy(h_ge.begin(), h_ge.end(), n_ge);
    lr_record(c, Pl, batches, B, G);
    return SGL_OK;
}
int sgl_ligrec_all(sgl_ctx* c, const int32_t* lab, int K, const int32_t* genes, int64_t G, const int32_t* lig, const int32_t* rec, int64_t P,
                   int64_t nperm, uint64_t seed, int64_t batch, int64_t* group_n, int64_t* nz, double* sum, double* mean, double* score, int64_t* n_ge,
                   double* null_out, double* stage_ms) {
    return lr_finish(c, lr_all_on(c, lab, K, genes, G, lig, rec, P, nperm, seed, batch, group_n, nz, sum, mean, score, n_ge, null_out, stage_ms));
}
