// Spatial autocorrelation (include/singlet_hip.h, "Spatial autocorrelation"): the device passes behind Moran's I of the genes
// of the resident matrix and of the rows of an embedding over a sparse n x n cell graph G.  The header states the rules for the
// caller, moran_host.h holds the graph moments and the assembly; this file holds
//   1. moran_moments_kernel / moran_moments_finish_kernel: Q2 = sum (x - m)^2, Q4 = sum ((x - m)^2)^2 and T = sum x * t[cell]
//      over the stored entries of a gene in ONE pass of the shape of hvg_segment_kernel (one wave per segment of 8192
//      entries, lane l takes the entries l, l + 64, ..., the butterfly 32 .. 1, segment sums ascending from +0.0), closed
//      with the zeros' share: M2 = Q2 + (double)(n - c) * (m * m), M4 = Q4 + (double)(n - c) * ((m * m) * (m * m)).
//      20 bytes per entry (value, cell, the gathered t).
//   2. the cross term P_g = sum over the stored entries e (cell j) of x_j * q_e, q_e = the sequential stored-order sum over
//      column j of G of w * x_r for the rows r that gene g stores.  Two paths, the same bits:
//        moran_search_kernel  one workgroup per gene of at most lds_cap entries: the gene's ascending cells and its values
//                             are staged in LDS, every lane owns an entry, walks its cell's column of G and finds each
//                             neighbour by binary search in LDS;
//        moran_table_kernel   a batch of B longer genes scatters its values into a B x n table in global memory
//                             (moran_scatter_kernel; a plain value table on a +0.0 background), one wave per segment reads
//                             the neighbours straight from the table, and the table is cleared by walking the entries again.
//      Both sum the p_e in blocks of 64 with ONE butterfly per block, block sums ascending from +0.0 within a segment of 8192,
//      segment sums ascending from +0.0.  An absent neighbour adds w * +0.0 = +-0.0 on the table path and nothing on the
//      search path: q starts at +0.0 and a sum that starts there is never -0.0, so the bits agree.
//   3. the embedding form: moran_center_kernel (z = F - mean), moran_conv_kernel (y_j = the sequential stored-order sum over
//      column j of G of w * z_r, then z * y, z * z and (z * z) * (z * z) per element); the sums over the cells are
//      sgl_group_sums_on's (kernels_group.hip) with all cells in one group.
// Hub columns of G are walked sequentially by their lane: the stated order demands it.  No floating-point atomics, no loop whose
// trip count follows the launch size, vector stores only; compiled with -ffp-contract=off, so every product and the addition
// after it round separately.  tests/moran_restatement.py restates all of it in numpy.
#include "sgl_internal.h"
#include "moran_host.h"

#include <numeric>

#define MORAN_THREADS 256
#define MORAN_WAVES (MORAN_THREADS / SGL_WAVE)
static_assert(MORAN_SEG % SGL_WAVE == 0, "a segment is whole blocks of 64");
static_assert(MORAN_LDS_CAP <= MORAN_SEG, "a gene of the search path is one segment");
// the search path's LDS: values, block sums, cells
#define MORAN_LDS_BYTES(cap) ((size_t)(cap) * 8 + (((size_t)(cap) + SGL_WAVE - 1) / SGL_WAVE + 1) * 8 + (size_t)(cap) * 4)

__device__ __forceinline__ double moran_wave_sum(double v) {
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SGL_WAVE);
    return v;
}

// the entries of segment `seg` of the gene at list position g: [lo, hi)
__device__ __forceinline__ void moran_segment(const int64_t* __restrict__ gstart, const int64_t* __restrict__ glen,
                                              const int64_t* __restrict__ seg_first, int32_t g, int64_t seg, int64_t& lo, int64_t& hi) {
    const int64_t off = (seg - seg_first[g]) * (int64_t)MORAN_SEG;
    lo = gstart[g] + off;
    int64_t len = glen[g] - off;
    if (len > MORAN_SEG) len = MORAN_SEG;
    hi = lo + len;
}

// ---- 1. the moments --------------------------------------------------------------------------------------------------------------
// part: 3 x nseg (Q2, Q4, T)
__global__ __launch_bounds__(MORAN_THREADS) void moran_moments_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                     const int64_t* __restrict__ gstart, const int64_t* __restrict__ glen,
                                                                     const int32_t* __restrict__ seg_gene, const int64_t* __restrict__ seg_first,
                                                                     int64_t nseg, const double* __restrict__ gmean, const double* __restrict__ t,
                                                                     double* __restrict__ part) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t seg = (int64_t)blockIdx.x * MORAN_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (seg >= nseg) return;
    const int32_t g = seg_gene[seg];
    int64_t lo, hi;
    moran_segment(gstart, glen, seg_first, g, seg, lo, hi);
    const double m = gmean[g];
    double a2 = 0.0, a4 = 0.0, at = 0.0;
    for (int64_t q = lo + lane; q < hi; q += SGL_WAVE) {
        const double v = x[q];
        const double tc = t[idx[q]];
        const double d = v - m;
        const double d2 = d * d;
        a2 += d2;
        a4 += d2 * d2;
        at += v * tc;
    }
    a2 = moran_wave_sum(a2);
    a4 = moran_wave_sum(a4);
    at = moran_wave_sum(at);
    if (lane == 0) {
        part[seg] = a2;
        part[nseg + seg] = a4;
        part[2 * nseg + seg] = at;
    }
}

// out: 6 x ng column-major (mean, M2, M4, T, P, c); P is written by the cross term
__global__ __launch_bounds__(MORAN_THREADS) void moran_moments_finish_kernel(const double* __restrict__ part, const int64_t* __restrict__ seg_first,
                                                                            const int64_t* __restrict__ glen, const double* __restrict__ gmean,
                                                                            int64_t nseg, int64_t ng, int64_t n, double* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * MORAN_THREADS + threadIdx.x;
    if (g >= ng) return;
    double q2 = 0.0, q4 = 0.0, tt = 0.0;
    for (int64_t s = seg_first[g]; s < seg_first[g + 1]; ++s) {
        q2 += part[s];
        q4 += part[nseg + s];
        tt += part[2 * nseg + s];
    }
    const int64_t c = glen[g];
    const double m = gmean[g];
    const double mm = m * m;
    const double zeros = (double)(n - c);
    out[6 * g] = m;
    out[6 * g + 1] = q2 + zeros * mm;
    out[6 * g + 2] = q4 + zeros * (mm * mm);
    out[6 * g + 3] = tt;
    out[6 * g + 5] = (double)c;
}

// ---- 2. the cross term -----------------------------------------------------------------------------------------------------------
// one workgroup per gene of the search list; dynamic LDS: xs[cap] | bs[cap / 64 + 1] | ids[cap]
__global__ __launch_bounds__(MORAN_THREADS) void moran_search_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                    const int64_t* __restrict__ gstart, const int64_t* __restrict__ glen,
                                                                    const int32_t* __restrict__ sgenes, const int64_t* __restrict__ Gp,
                                                                    const int32_t* __restrict__ Gi, const double* __restrict__ Gx, int cap,
                                                                    double* __restrict__ P, int64_t pstride) {
    extern __shared__ double moran_lds[];
    double* xs = moran_lds;
    double* bs = xs + cap;
    int32_t* ids = reinterpret_cast<int32_t*>(bs + (cap + SGL_WAVE - 1) / SGL_WAVE + 1);
    const int32_t g = sgenes[blockIdx.x];
    const int64_t lo = gstart[g];
    int len = (int)glen[g];
    if (len > cap) len = cap;   // (the host sends no longer gene here: nothing is read or written past the staged arrays)
    for (int e = threadIdx.x; e < len; e += MORAN_THREADS) {
        xs[e] = x[lo + e];
        ids[e] = idx[lo + e];
    }
    __syncthreads();
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nb = (len + SGL_WAVE - 1) / SGL_WAVE;
    for (int b = wave; b < nb; b += MORAN_WAVES) {
        const int e = b * SGL_WAVE + lane;
        double term = 0.0;   // a lane past the end holds +0.0
        if (e < len) {
            const int32_t j = ids[e];
            double qs = 0.0;
            for (int64_t q = Gp[j]; q < Gp[j + 1]; ++q) {
                const int32_t r = Gi[q];
                int a = 0, z = len;   // lower bound of r among the gene's cells
                while (a < z) {
                    const int mid = (a + z) >> 1;
                    if (ids[mid] < r) a = mid + 1;
                    else z = mid;
                }
                if (a < len && ids[a] == r) qs += Gx[q] * xs[a];
            }
            term = xs[e] * qs;
        }
        term = moran_wave_sum(term);
        if (lane == 0) bs[b] = term;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double seg = 0.0;
        for (int b = 0; b < nb; ++b) seg += bs[b];
        P[(int64_t)g * pstride] = 0.0 + seg;   // (one segment: the segment sums ascending from +0.0)
    }
}

// the segments [s0, s1) of the table list: table[slot, cell] = x (set) or +0.0 (clear)
__global__ __launch_bounds__(MORAN_THREADS) void moran_scatter_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                     const int64_t* __restrict__ gstart, const int64_t* __restrict__ glen,
                                                                     const int32_t* __restrict__ seg_gene, const int64_t* __restrict__ seg_first,
                                                                     const int32_t* __restrict__ gslot, int64_t s0, int64_t s1, int64_t n, int set,
                                                                     double* __restrict__ table) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t seg = s0 + (int64_t)blockIdx.x * MORAN_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (seg >= s1) return;
    const int32_t g = seg_gene[seg];
    int64_t lo, hi;
    moran_segment(gstart, glen, seg_first, g, seg, lo, hi);
    double* tab = table + (int64_t)gslot[g] * n;
    for (int64_t q = lo + lane; q < hi; q += SGL_WAVE) tab[idx[q]] = set ? x[q] : 0.0;
}

__global__ __launch_bounds__(MORAN_THREADS) void moran_table_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                   const int64_t* __restrict__ gstart, const int64_t* __restrict__ glen,
                                                                   const int32_t* __restrict__ seg_gene, const int64_t* __restrict__ seg_first,
                                                                   const int32_t* __restrict__ gslot, int64_t s0, int64_t s1, int64_t n,
                                                                   const int64_t* __restrict__ Gp, const int32_t* __restrict__ Gi,
                                                                   const double* __restrict__ Gx, const double* __restrict__ table,
                                                                   double* __restrict__ part) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t seg = s0 + (int64_t)blockIdx.x * MORAN_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (seg >= s1) return;
    const int32_t g = seg_gene[seg];
    int64_t lo, hi;
    moran_segment(gstart, glen, seg_first, g, seg, lo, hi);
    const double* tab = table + (int64_t)gslot[g] * n;
    double acc = 0.0;
    for (int64_t q0 = lo; q0 < hi; q0 += SGL_WAVE) {
        const int64_t e = q0 + lane;
        double term = 0.0;
        if (e < hi) {
            const int32_t j = idx[e];
            double qs = 0.0;
            for (int64_t q = Gp[j]; q < Gp[j + 1]; ++q) qs += Gx[q] * tab[Gi[q]];
            term = x[e] * qs;
        }
        acc += moran_wave_sum(term);
    }
    if (lane == 0) part[seg] = acc;
}

// P of the genes of the table list: the segment sums ascending from +0.0
__global__ __launch_bounds__(MORAN_THREADS) void moran_table_finish_kernel(const double* __restrict__ part, const int64_t* __restrict__ seg_first,
                                                                          const int32_t* __restrict__ tgenes, int64_t nt,
                                                                          double* __restrict__ P, int64_t pstride) {
    const int64_t q = (int64_t)blockIdx.x * MORAN_THREADS + threadIdx.x;
    if (q >= nt) return;
    const int32_t g = tgenes[q];
    double s = 0.0;
    for (int64_t sg = seg_first[g]; sg < seg_first[g + 1]; ++sg) s += part[sg];
    P[(int64_t)g * pstride] = s;
}

// ---- 3. the embedding form --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MORAN_THREADS) void moran_center_kernel(const double* __restrict__ F, const double* __restrict__ mean, int k,
                                                                    int64_t total, double* __restrict__ Z) {
    const int64_t e = (int64_t)blockIdx.x * MORAN_THREADS + threadIdx.x;
    if (e >= total) return;
    Z[e] = F[e] - mean[e % k];
}

// one lane per element (f, j), f fastest: the lanes of a column share its (row, weight) pairs
__global__ __launch_bounds__(MORAN_THREADS) void moran_conv_kernel(const double* __restrict__ Z, int k, int64_t total, const int64_t* __restrict__ Gp,
                                                                  const int32_t* __restrict__ Gi, const double* __restrict__ Gx,
                                                                  double* __restrict__ ZY, double* __restrict__ Z2, double* __restrict__ Z4) {
    const int64_t e = (int64_t)blockIdx.x * MORAN_THREADS + threadIdx.x;
    if (e >= total) return;
    const int64_t j = e / k;
    const int f = (int)(e - j * k);
    double y = 0.0;
    for (int64_t q = Gp[j]; q < Gp[j + 1]; ++q) y += Gx[q] * Z[(int64_t)Gi[q] * k + f];
    const double z = Z[e];
    const double z2 = z * z;
    ZY[e] = z * y;
    Z2[e] = z2;
    Z4[e] = z2 * z2;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
namespace {
int moran_drain(sgl_ctx* c, int rc, const char* who) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("%s: HIP call failed: %s", who, hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

// the graph on the device: 64-bit offsets, and t where the moments need it
struct MoranGraph {
    std::vector<int64_t> p64;   // host image of an asynchronous upload
    DevBuf<int64_t> p;
    DevBuf<int32_t> i;
    DevBuf<double> x, t;
};
int moran_graph_upload(sgl_ctx* c, MoranGraph& G, const double* Gx, const int32_t* Gi, const int32_t* Gp, int64_t n, const double* t) {
    G.p64.resize((size_t)n + 1);
    for (int64_t j = 0; j <= n; ++j) G.p64[(size_t)j] = Gp[j];
    const int64_t nnz = Gp[n];
    SGLCHK(G.p.alloc((size_t)n + 1));
    SGLCHK(G.i.alloc((size_t)std::max<int64_t>(nnz, 1)));
    SGLCHK(G.x.alloc((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(hipMemcpyAsync(G.p.p, G.p64.data(), sizeof(int64_t) * G.p64.size(), hipMemcpyHostToDevice, c->stream));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(G.i.p, Gi, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(G.x.p, Gx, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
    }
    if (t) {
        SGLCHK(G.t.alloc((size_t)n));
        HIPCHK(hipMemcpyAsync(G.t.p, t, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    return SGL_OK;
}

// everything a gene call's queued work reads: owned by the entry function, which drains the stream before any of it goes
struct MoranScratch {
    MoranGraph G;
    std::vector<int64_t> gstart, glen, first, tfirst;
    std::vector<int32_t> sg, tsg, sgenes, tgenes, gslot;
    std::vector<double> gmean, mean_all, t, out;
    std::vector<int64_t> count_all;
    DevBuf<int64_t> dstart, dlen, dfirst, dtfirst;
    DevBuf<int32_t> dsg, dtsg, dsgenes, dtgenes, dslot;
    DevBuf<double> dmean, dpart, dtpart, dout, table;
};

int moran_genes_on(sgl_ctx* c, MoranScratch& S, const double* Gx, const int32_t* Gi, const int32_t* Gp, const int32_t* genes, int64_t n_genes,
                   int path, int64_t lds_cap, int64_t table_batch, bool want_moments, double* moments_out, double* P_out, int64_t info[6]) {
    const DevCSC& M = c->At;
    const int32_t m = M.ncol;
    const int64_t n = M.nrow;
    const int64_t ng = genes ? n_genes : (int64_t)m;
    std::fill(info, info + 6, 0);
    info[5] = moran_lds_cap(lds_cap);
    if (ng == 0) return SGL_OK;
    // the graph moments (host, O(nnz(G))) before anything is uploaded: a graph without weight is refused
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    if (want_moments) {
        S.t.resize((size_t)n);
        if (moran_graph_moments(Gx, Gi, Gp, n, &S0, &S1, &S2, S.t.data())) {
            sgl_set_error("sgl_moran: the graph's weights sum to S0 = %g, or a graph moment is not finite: Moran's I is not defined", S0);
            return SGL_EINVAL;
        }
    }
    SGLCHK(moran_graph_upload(c, S.G, Gx, Gi, Gp, n, want_moments ? S.t.data() : nullptr));
    // the offsets of t(A) and, for the moments, sgl_op_gene_mean's own pass over all genes
    std::vector<int64_t> p((size_t)m + 1);
    HIPCHK(hipMemcpyAsync(p.data(), M.p, sizeof(int64_t) * p.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (want_moments) {
        S.mean_all.resize((size_t)m);
        S.count_all.resize((size_t)m);
        SGLCHK(sgl_hvg_pass(c, 0, nullptr, nullptr, 0.0, S.mean_all.data(), S.count_all.data()));
    }
    // per listed gene: its entries; the segment table of the whole list (moments) and of the table path; the path lists
    S.gstart.resize((size_t)ng);
    S.glen.resize((size_t)ng);
    S.gmean.assign((size_t)ng, 0.0);
    S.first.assign((size_t)ng + 1, 0);
    S.tfirst.assign((size_t)ng + 1, 0);
    S.gslot.assign((size_t)ng, 0);
    int64_t max_search = 0;
    for (int64_t q = 0; q < ng; ++q) {
        const int32_t g = genes ? genes[q] : (int32_t)q;
        const int64_t len = p[(size_t)g + 1] - p[g];
        S.gstart[(size_t)q] = p[g];
        S.glen[(size_t)q] = len;
        if (want_moments) S.gmean[(size_t)q] = S.mean_all[g];
        const int64_t segs = (len + MORAN_SEG - 1) / MORAN_SEG;
        S.first[(size_t)q + 1] = S.first[(size_t)q] + segs;
        if (moran_gene_path(len, path, lds_cap) == 1) {
            S.sgenes.push_back((int32_t)q);
            S.tfirst[(size_t)q + 1] = S.tfirst[(size_t)q];
            max_search = std::max(max_search, len);
        } else {
            S.tgenes.push_back((int32_t)q);
            S.tfirst[(size_t)q + 1] = S.tfirst[(size_t)q] + segs;
        }
    }
    const int64_t nseg = S.first[(size_t)ng], ntseg = S.tfirst[(size_t)ng];
    const int64_t ns = (int64_t)S.sgenes.size(), nt = (int64_t)S.tgenes.size();
    if ((std::max(nseg, ntseg) + MORAN_WAVES - 1) / MORAN_WAVES > INT32_MAX || ns > INT32_MAX) {
        sgl_set_error("sgl_moran: %lld segments are more than one launch holds", (long long)std::max(nseg, ntseg));
        return SGL_EINVAL;
    }
    S.sg.assign((size_t)std::max<int64_t>(nseg, 1), 0);
    S.tsg.assign((size_t)std::max<int64_t>(ntseg, 1), 0);
    for (int64_t q = 0; q < ng; ++q) {
        for (int64_t s = S.first[(size_t)q]; s < S.first[(size_t)q + 1]; ++s) S.sg[(size_t)s] = (int32_t)q;
        for (int64_t s = S.tfirst[(size_t)q]; s < S.tfirst[(size_t)q + 1]; ++s) S.tsg[(size_t)s] = (int32_t)q;
    }
    // the table batch: from the free memory (a quarter of it), or the caller's
    int64_t B = 0;
    if (nt > 0) {
        size_t free_b = 0, total_b = 0;
        if (sgl_pool_mem_info(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)1 << 30; }
        B = std::max<int64_t>(1, (int64_t)(free_b / 4 / (sizeof(double) * (size_t)n)));
        B = std::min<int64_t>(B, 4096);
        if (table_batch > 0) B = table_batch;
        B = std::min(B, nt);
        for (int64_t q = 0; q < nt; ++q) S.gslot[(size_t)S.tgenes[(size_t)q]] = (int32_t)(q % B);
    }
    auto up = [&](auto& dev, const auto& host) -> int {
        SGLCHK(dev.alloc(std::max<size_t>(host.size(), 1)));
        if (!host.empty()) HIPCHK(hipMemcpyAsync(dev.p, host.data(), sizeof(host[0]) * host.size(), hipMemcpyHostToDevice, c->stream));
        return SGL_OK;
    };
    SGLCHK(up(S.dstart, S.gstart));
    SGLCHK(up(S.dlen, S.glen));
    SGLCHK(up(S.dmean, S.gmean));
    SGLCHK(up(S.dfirst, S.first));
    SGLCHK(up(S.dtfirst, S.tfirst));
    SGLCHK(up(S.dsg, S.sg));
    SGLCHK(up(S.dtsg, S.tsg));
    SGLCHK(up(S.dsgenes, S.sgenes));
    SGLCHK(up(S.dtgenes, S.tgenes));
    SGLCHK(up(S.dslot, S.gslot));
    SGLCHK(S.dout.alloc((size_t)ng * 6));
    SGLCHK(S.dpart.alloc((size_t)std::max<int64_t>(nseg, 1) * 3));
    SGLCHK(S.dtpart.alloc((size_t)std::max<int64_t>(ntseg, 1)));
    HIPCHK(hipMemsetAsync(S.dout.p, 0, sizeof(double) * (size_t)ng * 6, c->stream));
    if (B > 0) {
        SGLCHK(S.table.alloc((size_t)B * (size_t)n));
        HIPCHK(hipMemsetAsync(S.table.p, 0, sizeof(double) * (size_t)B * (size_t)n, c->stream));   // once: afterwards the entries are walked again
    }
    const int cap = (int)std::max<int64_t>(max_search, 1);
    const size_t lds = MORAN_LDS_BYTES(cap);
    if (ns > 0) SGLCHK(sgl_allow_dynamic_lds<&moran_search_kernel>((int)MORAN_LDS_BYTES(MORAN_LDS_CAP)));
    int64_t batches = 0;
    {
        Phase ph(c, SGL_PH_SCALE);
        if (want_moments) {
            if (nseg > 0) {
                moran_moments_kernel<<<dim3((unsigned)((nseg + MORAN_WAVES - 1) / MORAN_WAVES)), dim3(MORAN_THREADS), 0, c->stream>>>(
                    M.x, M.i, S.dstart.p, S.dlen.p, S.dsg.p, S.dfirst.p, nseg, S.dmean.p, S.G.t.p, S.dpart.p);
                HIPCHK(hipGetLastError());
            }
            moran_moments_finish_kernel<<<dim3((unsigned)((ng + MORAN_THREADS - 1) / MORAN_THREADS)), dim3(MORAN_THREADS), 0, c->stream>>>(
                S.dpart.p, S.dfirst.p, S.dlen.p, S.dmean.p, nseg, ng, n, S.dout.p);
            HIPCHK(hipGetLastError());
        }
        if (ns > 0) {
            moran_search_kernel<<<dim3((unsigned)ns), dim3(MORAN_THREADS), lds, c->stream>>>(M.x, M.i, S.dstart.p, S.dlen.p, S.dsgenes.p, S.G.p.p, S.G.i.p,
                                                                                           S.G.x.p, cap, S.dout.p + 4, 6);
            HIPCHK(hipGetLastError());
        }
        for (int64_t b0 = 0; b0 < nt; b0 += B) {
            const int64_t b1 = std::min(b0 + B, nt);
            // the table genes are in list order, so a batch's segments are one range of the table list
            const int64_t s0 = S.tfirst[(size_t)S.tgenes[(size_t)b0]], s1 = S.tfirst[(size_t)S.tgenes[(size_t)b1 - 1] + 1];
            ++batches;
            if (s1 == s0) continue;
            const dim3 grid((unsigned)((s1 - s0 + MORAN_WAVES - 1) / MORAN_WAVES));
            moran_scatter_kernel<<<grid, dim3(MORAN_THREADS), 0, c->stream>>>(M.x, M.i, S.dstart.p, S.dlen.p, S.dtsg.p, S.dtfirst.p, S.dslot.p, s0, s1, n, 1,
                                                                             S.table.p);
            HIPCHK(hipGetLastError());
            moran_table_kernel<<<grid, dim3(MORAN_THREADS), 0, c->stream>>>(M.x, M.i, S.dstart.p, S.dlen.p, S.dtsg.p, S.dtfirst.p, S.dslot.p, s0, s1, n,
                                                                           S.G.p.p, S.G.i.p, S.G.x.p, S.table.p, S.dtpart.p);
            HIPCHK(hipGetLastError());
            moran_scatter_kernel<<<grid, dim3(MORAN_THREADS), 0, c->stream>>>(M.x, M.i, S.dstart.p, S.dlen.p, S.dtsg.p, S.dtfirst.p, S.dslot.p, s0, s1, n, 0,
                                                                             S.table.p);
            HIPCHK(hipGetLastError());
        }
        if (nt > 0) {
            moran_table_finish_kernel<<<dim3((unsigned)((nt + MORAN_THREADS - 1) / MORAN_THREADS)), dim3(MORAN_THREADS), 0, c->stream>>>(
                S.dtpart.p, S.dtfirst.p, S.dtgenes.p, nt, S.dout.p + 4, 6);
            HIPCHK(hipGetLastError());
        }
    }
    S.out.resize((size_t)ng * 6);
    HIPCHK(hipMemcpyAsync(S.out.data(), S.dout.p, sizeof(double) * (size_t)ng * 6, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (moments_out) std::copy(S.out.begin(), S.out.end(), moments_out);
    if (P_out)
        for (int64_t q = 0; q < ng; ++q) P_out[q] = S.out[(size_t)q * 6 + 4];
    info[0] = ns;
    info[1] = nt;
    info[2] = batches;
    info[3] = B;
    info[4] = B * n * (int64_t)sizeof(double);
    return SGL_OK;
}

struct MoranEmbedScratch {
    MoranGraph G;
    GroupPlan P;
    std::vector<int32_t> labels;
    DevBuf<double> part, mean, Z, ZY, Z2, Z4, sums;
};

int moran_embedding_on(sgl_ctx* c, MoranEmbedScratch& S, const double* Gx, const int32_t* Gi, const int32_t* Gp, const double* F, int k, int64_t n,
                       double* moments_out, double* mean_out) {
    SGLCHK(moran_graph_upload(c, S.G, Gx, Gi, Gp, n, nullptr));
    S.labels.assign((size_t)n, 0);   // all cells, one group: sgl_group_means' chunk order over all cells
    SGLCHK(sgl_group_plan(c, S.P, n, S.labels.data(), 1));
    const size_t kn = (size_t)k * (size_t)n;
    const int64_t total = (int64_t)kn;
    SGLCHK(S.part.alloc((size_t)std::max<int64_t>(S.P.nchunks, 1) * (size_t)k));
    SGLCHK(S.mean.alloc((size_t)k));
    SGLCHK(S.sums.alloc((size_t)k * 3));
    SGLCHK(S.Z.alloc(kn));
    SGLCHK(S.ZY.alloc(kn));
    SGLCHK(S.Z2.alloc(kn));
    SGLCHK(S.Z4.alloc(kn));
    SGLCHK(sgl_group_sums_on(c, S.P, F, k, 1, true, S.part.p, S.mean.p));
    if ((total + MORAN_THREADS - 1) / MORAN_THREADS > INT32_MAX) { sgl_set_error("sgl_moran_embedding: k x n = %lld elements are more than one launch holds", (long long)total); return SGL_EINVAL; }
    const dim3 grid((unsigned)((total + MORAN_THREADS - 1) / MORAN_THREADS));
    {
        Phase ph(c, SGL_PH_SCALE);
        moran_center_kernel<<<grid, dim3(MORAN_THREADS), 0, c->stream>>>(F, S.mean.p, k, total, S.Z.p);
        HIPCHK(hipGetLastError());
        moran_conv_kernel<<<grid, dim3(MORAN_THREADS), 0, c->stream>>>(S.Z.p, k, total, S.G.p.p, S.G.i.p, S.G.x.p, S.ZY.p, S.Z2.p, S.Z4.p);
        HIPCHK(hipGetLastError());
    }
    // (part is free again each time: the finish kernel of the sums before ran on the same stream)
    SGLCHK(sgl_group_sums_on(c, S.P, S.ZY.p, k, 1, false, S.part.p, S.sums.p));
    SGLCHK(sgl_group_sums_on(c, S.P, S.Z2.p, k, 1, false, S.part.p, S.sums.p + k));
    SGLCHK(sgl_group_sums_on(c, S.P, S.Z4.p, k, 1, false, S.part.p, S.sums.p + 2 * (size_t)k));
    std::vector<double> h((size_t)k * 4);
    HIPCHK(hipMemcpyAsync(h.data(), S.sums.p, sizeof(double) * (size_t)k * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h.data() + 3 * (size_t)k, S.mean.p, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int f = 0; f < k; ++f) {
        if (moments_out) {
            double* mo = moments_out + 6 * (size_t)f;
            mo[0] = 0.0;                       // the rows are centred: the mean the assembly sees
            mo[1] = h[(size_t)k + f];          // M2
            mo[2] = h[2 * (size_t)k + f];      // M4
            mo[3] = 0.0;                       // T
            mo[4] = h[(size_t)f];              // P = C
            mo[5] = (double)n;
        }
        if (mean_out) mean_out[f] = h[3 * (size_t)k + f];
    }
    return SGL_OK;
}
}   // namespace

int sgl_moran_args_check(const char* who, const double* Gx, const int32_t* Gi, const int32_t* Gp, int64_t G_n, int64_t ncells, const int32_t* genes,
                         int64_t n_genes, int64_t m, int64_t path, int64_t lds_cap, int64_t table_batch) {
    if (!Gx || !Gi || !Gp) { sgl_set_error("%s: NULL graph array (Gx, Gi and Gp are required)", who); return SGL_EINVAL; }
    if (G_n != ncells || G_n > (int64_t)INT32_MAX) {
        sgl_set_error("%s: G is %lld x %lld, the matrix has %lld cells (G must be n x n)", who, (long long)G_n, (long long)G_n, (long long)ncells);
        return SGL_EINVAL;
    }
    if (G_n < MORAN_MIN_N) { sgl_set_error("%s: n = %lld cells: the variance of Moran's I needs at least %d", who, (long long)G_n, MORAN_MIN_N); return SGL_EINVAL; }
    SGLCHK(sgl_graph_check(who, Gx, Gi, Gp, (int32_t)G_n, (int32_t)G_n, G_n));
    int64_t at = -1, val = 0;
    switch (moran_check_genes(genes, n_genes, m, path, lds_cap, table_batch, &at, &val)) {
    case MORAN_ARGS_OK: return SGL_OK;
    case MORAN_ARGS_PATH: sgl_set_error("%s: path = %lld is none of 0 (automatic), 1 (search), 2 (table)", who, (long long)val); break;
    case MORAN_ARGS_CAP: sgl_set_error("%s: a knob of %lld is negative (0: the default)", who, (long long)val); break;
    case MORAN_ARGS_NGENES: sgl_set_error("%s: n_genes = %lld is outside [0, 2^31)", who, (long long)val); break;
    case MORAN_ARGS_RANGE: sgl_set_error("%s: genes[%lld] = %lld is outside [0, nrow = %lld)", who, (long long)at, (long long)val, (long long)m); break;
    case MORAN_ARGS_REPEAT: sgl_set_error("%s: genes[%lld] = %lld is listed twice (the genes must be distinct)", who, (long long)at, (long long)val); break;
    default: sgl_set_error("%s: bad arguments", who); break;
    }
    return SGL_EINVAL;
}

int sgl_moran_genes_core(sgl_ctx* c, const double* Gx, const int32_t* Gi, const int32_t* Gp, const int32_t* genes, int64_t n_genes, int path,
                         int64_t lds_cap, int64_t table_batch, bool want_moments, double* moments_out, double* P_out) {
    MoranScratch S;   // (lives until the stream is drained, on every return path of the inner function)
    int64_t info[6];
    const int rc = moran_drain(c, moran_genes_on(c, S, Gx, Gi, Gp, genes, n_genes, path, lds_cap, table_batch, want_moments, moments_out, P_out, info),
                               "sgl_moran");
    if (rc == SGL_OK) std::copy(info, info + 6, c->moran_last);
    return rc;
}

int sgl_moran_embedding_core(sgl_ctx* c, const double* Gx, const int32_t* Gi, const int32_t* Gp, const double* F, int k, int64_t n,
                             double* moments_out, double* mean_out) {
    MoranEmbedScratch S;
    return moran_drain(c, moran_embedding_on(c, S, Gx, Gi, Gp, F, k, n, moments_out, mean_out), "sgl_moran_embedding");
}
