// Factor annotation (include/singlet_hip.h, "Factor annotation"): the group moments of a means model ~ 0 + column -- group
// counts, group sums and the residual sum of squares around the group means -- of the rows of a k x n embedding and of the
// genes of the resident matrix.  The counts and the sums are the library's own: sgl_group_sums_on (kernels_group.hip) on the
// embedding side, sgl_markers_core (kernels_markers.hip, transform 0) on the gene side.  This file holds the residual passes:
//   1. ann_rss_chunk_kernel / ann_rss_finish_kernel: the second pass over F in the shape of group_chunk_kernel.  One
//      workgroup per chunk of 256 cells of one group; slot s takes the positions s, s + S, ... in turn, each term one
//      subtraction of the group's mean (read from the k x G table through the cache) and one multiplication; the S slot sums
//      go through the binary tree in LDS.  One lane per factor then adds the chunk sums of ALL groups in ascending chunk
//      order from +0.0.
//   2. ann_gene_rss_kernel / ann_gene_finish_kernel: ONE WAVE PER SEGMENT of 8192 stored entries of a gene, as
//      hvg_segment_kernel.  A lane of a block of 64 consecutive entries holds (x - mean[g, c])^2, or +0.0 for an excluded
//      cell, a stored zero or a place past the end; ONE butterfly (lane ^ 32, 16, ... 1) per block; the block sums are added
//      in ascending order.  The label is gathered 4 bytes per cell, the gene's G means from a table laid out gene by gene
//      (160 contiguous bytes at G = 20).  One lane per gene adds its segment sums in ascending order from +0.0.
//      The zeros' share Z[g] and rss = E + Z are formed on the HOST (m G operations).
// No floating-point atomics, no loop whose trip count follows the launch size; compiled with -ffp-contract=off, so the
// subtraction, the product and the addition round separately.  tests/annotate_restatement.py restates all of it in numpy.
#include "sgl_internal.h"
#include "annotate_host.h"

#define ANN_THREADS 256
#define ANN_WAVES (ANN_THREADS / SGL_WAVE)
static_assert(SGL_GROUP_CHUNK % ANN_THREADS == 0, "a chunk is whole rounds of the slots");
static_assert(ANNOTATE_SEG % (4 * SGL_WAVE) == 0, "a full segment is whole rounds of the unrolled block loop");

__device__ __forceinline__ double ann_wave_sum(double v) {
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SGL_WAVE);
    return v;
}

// ---- 1. embedding side -----------------------------------------------------------------------------------------------------
// mean[f, g] = sum[f, g] / (double)n_g: one true division (an empty group: 0.0 / 0.0 = NaN, which no chunk reads)
__global__ __launch_bounds__(ANN_THREADS) void ann_mean_kernel(const double* __restrict__ sum, int k, int32_t n_groups,
                                                              const int64_t* __restrict__ goff, double* __restrict__ mean) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)k * n_groups) return;
    const int32_t g = (int32_t)(e / k);
    mean[e] = sum[e] / (double)(goff[g + 1] - goff[g]);
}

// fl_shift: log2(FL).  cbeg[ch] .. cbeg[ch + 1]: the chunk's positions in perm; cgroup[ch]: its group.
__global__ __launch_bounds__(ANN_THREADS) void ann_rss_chunk_kernel(const double* __restrict__ F, int k, const int32_t* __restrict__ perm,
                                                                   const int64_t* __restrict__ cbeg, const int32_t* __restrict__ cgroup,
                                                                   int fl_shift, const double* __restrict__ mean, double* __restrict__ part) {
    __shared__ double tree[ANN_THREADS];
    const int FL = 1 << fl_shift;
    const int S = ANN_THREADS >> fl_shift;
    const int fl = threadIdx.x & (FL - 1);
    const int slot = threadIdx.x >> fl_shift;
    const int64_t ch = blockIdx.x;
    const int64_t p0 = cbeg[ch], p1 = cbeg[ch + 1];
    const double* mg = mean + (int64_t)cgroup[ch] * k;
    for (int f0 = 0; f0 < k; f0 += FL) {
        const int f = f0 + fl;
        double acc = 0.0;
        if (f < k) {
            const double mu = mg[f];
            // four columns in flight per lane; the additions stay in position order
            int64_t p = p0 + slot;
            for (; p + 3 * (int64_t)S < p1; p += 4 * (int64_t)S) {
                const double d0 = F[(int64_t)perm[p] * k + f] - mu;
                const double d1 = F[(int64_t)perm[p + S] * k + f] - mu;
                const double d2 = F[(int64_t)perm[p + 2 * S] * k + f] - mu;
                const double d3 = F[(int64_t)perm[p + 3 * S] * k + f] - mu;
                acc += d0 * d0;
                acc += d1 * d1;
                acc += d2 * d2;
                acc += d3 * d3;
            }
            for (; p < p1; p += S) {
                const double d = F[(int64_t)perm[p] * k + f] - mu;
                acc += d * d;
            }
        }
        __syncthreads();   // the tree of the previous pass has been read
        tree[threadIdx.x] = acc;   // [slot][fl]
        __syncthreads();
        for (int stride = S >> 1; stride > 0; stride >>= 1) {
            if (slot < stride) tree[threadIdx.x] += tree[threadIdx.x + (stride << fl_shift)];
            __syncthreads();
        }
        if (slot == 0 && f < k) part[ch * k + f] = tree[fl];
    }
}

// rss[f] = the chunk sums of all groups in ascending chunk order (group 0's chunks, then group 1's, ...) from +0.0
__global__ __launch_bounds__(ANN_THREADS) void ann_rss_finish_kernel(const double* __restrict__ part, int k, int64_t nchunks,
                                                                    double* __restrict__ rss) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= k) return;
    double s = 0.0;
#pragma unroll 32
    for (int64_t ch = 0; ch < nchunks; ++ch) s += part[ch * k + f];   // (one chain per factor: the unrolling keeps 32 loads in flight)
    rss[f] = s;
}

// ---- 2. gene side ------------------------------------------------------------------------------------------------------------
// meanT: m x G, the G means of gene g at meanT[g G ..]
__global__ __launch_bounds__(ANN_THREADS) void ann_gene_rss_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                  const int64_t* __restrict__ p, const int32_t* __restrict__ lab,
                                                                  const int32_t* __restrict__ seg_gene, const int64_t* __restrict__ seg_first,
                                                                  int64_t nseg, int32_t G, const double* __restrict__ meanT,
                                                                  double* __restrict__ part) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t seg = (int64_t)blockIdx.x * ANN_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (seg >= nseg) return;
    const int32_t g = seg_gene[seg];
    const int64_t lo = p[g] + (seg - seg_first[g]) * (int64_t)ANNOTATE_SEG;
    int64_t hi = p[g + 1];
    if (hi - lo > ANNOTATE_SEG) hi = lo + ANNOTATE_SEG;
    const double* mu = meanT + (int64_t)g * G;
    double acc = 0.0;
    // four blocks in flight per wave; the block sums are added in ascending order (a block past the end adds +0.0 to a sum
    // that is never -0.0: no bit changes)
    for (int64_t q0 = lo; q0 < hi; q0 += 4 * SGL_WAVE) {
        double xv[4];
        int32_t cell[4], l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = q0 + u * SGL_WAVE + lane;
            xv[u] = 0.0;
            cell[u] = -1;
            if (q < hi) { xv[u] = x[q]; cell[u] = idx[q]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) l[u] = cell[u] >= 0 ? lab[cell[u]] : -1;
        double term[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            term[u] = 0.0;
            if (l[u] >= 0 && xv[u] != 0.0) {
                const double d = xv[u] - mu[l[u]];
                term[u] = d * d;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += ann_wave_sum(term[u]);
    }
    if (lane == 0) part[seg] = acc;
}

__global__ __launch_bounds__(ANN_THREADS) void ann_gene_finish_kernel(const double* __restrict__ part, const int64_t* __restrict__ seg_first,
                                                                     int32_t ngenes, double* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * ANN_THREADS + threadIdx.x;
    if (g >= ngenes) return;
    double s = 0.0;
    for (int64_t sg = seg_first[g]; sg < seg_first[g + 1]; ++sg) s += part[sg];
    out[g] = s;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int sgl_annotate_args_check(const char* who, const int32_t* labels, int64_t n, int32_t n_groups, int32_t k) {
    int64_t pos = -1;
    int32_t val = 0;
    switch (annotate_check_args(labels, n, n_groups, k, &pos, &val)) {
    case ANNOTATE_ARGS_OK: return SGL_OK;
    case ANNOTATE_ARGS_NULL: sgl_set_error("%s: NULL labels", who); break;
    case ANNOTATE_ARGS_GROUPS: sgl_set_error("%s: n_groups = %d is outside [1, %d]", who, n_groups, ANNOTATE_MAX_GROUPS); break;
    case ANNOTATE_ARGS_K: sgl_set_error("%s: k = %d is outside [1, %d]", who, k, ANNOTATE_MAX_K); break;
    case ANNOTATE_ARGS_LABEL: sgl_set_error("%s: labels[%lld] = %d is outside [-1, %d)", who, (long long)pos, val, n_groups); break;
    }
    return SGL_EINVAL;
}

static int ann_drain(sgl_ctx* c, int rc, const char* who) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("%s: HIP call failed: %s", who, hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

// what a call's queued work reads and writes: owned by the entry function, which drains the stream before any of it goes
namespace {
struct AnnEmbedScratch {
    GroupPlan P;
    DevBuf<double> dpart, dsum, dmean, drss;
};
struct AnnGeneScratch {
    std::vector<int64_t> first;   // host images of asynchronous uploads
    std::vector<int32_t> sg;
    std::vector<double> meanT;
    DevBuf<int32_t> dseg, dlab;
    DevBuf<int64_t> dfirst;
    DevBuf<double> dmean, dpart, dE;
};
}   // namespace

static int ann_group_moments_on(sgl_ctx* c, AnnEmbedScratch& S, const double* F, int k, int64_t n, const int32_t* labels, int32_t G,
                                int64_t* group_n, double* sum, double* rss) {
    GroupPlan& P = S.P;
    DevBuf<double>&dpart = S.dpart, &dsum = S.dsum, &dmean = S.dmean, &drss = S.drss;
    SGLCHK(sgl_group_plan(c, P, n, labels, G));
    if (group_n) std::copy(P.counts.begin(), P.counts.end(), group_n);
    const size_t kg = (size_t)k * (size_t)G;
    SGLCHK(dpart.alloc((size_t)std::max<int64_t>(P.nchunks, 1) * (size_t)k));
    SGLCHK(dsum.alloc(kg));
    SGLCHK(dmean.alloc(kg));
    SGLCHK(drss.alloc((size_t)k));
    SGLCHK(sgl_group_sums_on(c, P, F, k, G, false, dpart.p, dsum.p));
    int fl_shift = 0;
    while ((1 << fl_shift) < k && fl_shift < 6) ++fl_shift;
    {
        Phase ph(c, SGL_PH_SCALE);
        ann_mean_kernel<<<dim3((unsigned)((kg + ANN_THREADS - 1) / ANN_THREADS)), dim3(ANN_THREADS), 0, c->stream>>>(dsum.p, k, G, P.goff.p, dmean.p);
        HIPCHK(hipGetLastError());
        if (P.nchunks > 0) {   // (part is free again: the sums' finish kernel ran before on the same stream)
            ann_rss_chunk_kernel<<<dim3((unsigned)P.nchunks), dim3(ANN_THREADS), 0, c->stream>>>(F, k, P.perm.p, P.cbeg.p, P.cgroup.p, fl_shift,
                                                                                                dmean.p, dpart.p);
            HIPCHK(hipGetLastError());
        }
        ann_rss_finish_kernel<<<dim3((unsigned)((k + ANN_THREADS - 1) / ANN_THREADS)), dim3(ANN_THREADS), 0, c->stream>>>(dpart.p, k, P.nchunks, drss.p);
        HIPCHK(hipGetLastError());
    }
    if (sum) HIPCHK(hipMemcpyAsync(sum, dsum.p, sizeof(double) * kg, hipMemcpyDeviceToHost, c->stream));
    if (rss) HIPCHK(hipMemcpyAsync(rss, drss.p, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SGL_OK;
}

// F on the DEVICE, k x n column-major; labels on the host, checked by the caller.  The plan and the buffers live here: on
// every return path of the inner function the stream is drained before they go.
int sgl_group_moments_dev(sgl_ctx* c, const double* F, int k, int64_t n, const int32_t* labels, int32_t G, int64_t* group_n, double* sum,
                          double* rss) {
    AnnEmbedScratch S;
    return ann_drain(c, ann_group_moments_on(c, S, F, k, n, labels, G, group_n, sum, rss), "group moments");
}

static int ann_gene_moments_on(sgl_ctx* c, AnnGeneScratch& S, const int32_t* labels, int32_t G, int64_t* group_n, int64_t* nz, double* sum,
                               double* rss) {
    const DevCSC& M = c->At;
    const int32_t m = M.ncol;
    const size_t m1 = (size_t)std::max(m, 1), mg = m1 * (size_t)G;
    std::vector<int64_t> gn((size_t)G), hnz(mg);
    std::vector<double> hsum(mg);
    // counts and sums: the marker genes' own pass, transform 0
    SGLCHK(sgl_markers_core(c, labels, G, 0, 0, true, false, gn.data(), nullptr, hnz.data(), hsum.data(), nullptr, nullptr));
    std::vector<double>& meanT = S.meanT;
    std::vector<double> E(m1, 0.0);
    meanT.assign(mg, 0.0);
    for (int32_t g = 0; g < m; ++g)
        for (int32_t cl = 0; cl < G; ++cl) meanT[(size_t)g * G + cl] = hsum[(size_t)g + (size_t)m * cl] / (double)gn[cl];
    // the segment table of t(A)
    std::vector<int64_t> p((size_t)m + 1);
    std::vector<int64_t>& first = S.first;
    first.assign((size_t)m + 1, 0);
    HIPCHK(hipMemcpyAsync(p.data(), M.p, sizeof(int64_t) * p.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int32_t g = 0; g < m; ++g) first[(size_t)g + 1] = first[g] + (p[(size_t)g + 1] - p[g] + ANNOTATE_SEG - 1) / ANNOTATE_SEG;
    const int64_t nseg = first[m];
    if ((nseg + ANN_WAVES - 1) / ANN_WAVES > INT32_MAX) { sgl_set_error("gene group moments: %lld segments are more than one launch holds", (long long)nseg); return SGL_EINVAL; }
    std::vector<int32_t>& sg = S.sg;
    sg.assign((size_t)std::max<int64_t>(nseg, 1), 0);
    for (int32_t g = 0; g < m; ++g)
        for (int64_t s = first[g]; s < first[(size_t)g + 1]; ++s) sg[(size_t)s] = g;
    DevBuf<int32_t>&dseg = S.dseg, &dlab = S.dlab;
    DevBuf<int64_t>& dfirst = S.dfirst;
    DevBuf<double>&dmean = S.dmean, &dpart = S.dpart, &dE = S.dE;
    SGLCHK(dseg.alloc(sg.size()));
    SGLCHK(dlab.alloc((size_t)std::max(M.nrow, 1)));
    SGLCHK(dfirst.alloc(first.size()));
    SGLCHK(dmean.alloc(mg));
    SGLCHK(dpart.alloc(sg.size()));
    SGLCHK(dE.alloc(m1));
    HIPCHK(hipMemcpyAsync(dseg.p, sg.data(), sizeof(int32_t) * sg.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dfirst.p, first.data(), sizeof(int64_t) * first.size(), hipMemcpyHostToDevice, c->stream));
    if (M.nrow > 0) HIPCHK(hipMemcpyAsync(dlab.p, labels, sizeof(int32_t) * (size_t)M.nrow, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dmean.p, meanT.data(), sizeof(double) * mg, hipMemcpyHostToDevice, c->stream));
    {
        Phase ph(c, SGL_PH_SCALE);
        if (nseg > 0) {
            ann_gene_rss_kernel<<<dim3((unsigned)((nseg + ANN_WAVES - 1) / ANN_WAVES)), dim3(ANN_THREADS), 0, c->stream>>>(
                M.x, M.i, M.p, dlab.p, dseg.p, dfirst.p, nseg, G, dmean.p, dpart.p);
            HIPCHK(hipGetLastError());
        }
        if (m > 0) {
            ann_gene_finish_kernel<<<dim3((unsigned)((m + ANN_THREADS - 1) / ANN_THREADS)), dim3(ANN_THREADS), 0, c->stream>>>(dpart.p, dfirst.p, m, dE.p);
            HIPCHK(hipGetLastError());
        }
    }
    if (m > 0) HIPCHK(hipMemcpyAsync(E.data(), dE.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // the zeros' share, on the host: Z[g] = sum over c ascending of (n_c - nz[g, c]) * mean^2 (an empty group has no zeros either)
    for (int32_t g = 0; g < m; ++g) {
        double Z = 0.0;
        for (int32_t cl = 0; cl < G; ++cl) {
            if (gn[cl] == 0) continue;
            const double mu = meanT[(size_t)g * G + cl];
            Z += (double)(gn[cl] - hnz[(size_t)g + (size_t)m * cl]) * (mu * mu);
        }
        if (rss) rss[g] = E[g] + Z;
    }
    const size_t nout = (size_t)m * (size_t)G;
    if (group_n) std::copy(gn.begin(), gn.end(), group_n);
    if (nz) std::copy(hnz.begin(), hnz.begin() + nout, nz);
    if (sum) std::copy(hsum.begin(), hsum.begin() + nout, sum);
    return SGL_OK;
}

int sgl_gene_moments_core(sgl_ctx* c, const int32_t* labels, int32_t G, int64_t* group_n, int64_t* nz, double* sum, double* rss) {
    AnnGeneScratch S;   // (lives until the stream is drained, on every return path of the inner function)
    return ann_drain(c, ann_gene_moments_on(c, S, labels, G, group_n, nz, sum, rss), "gene group moments");
}
