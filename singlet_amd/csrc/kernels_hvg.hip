// Variable features of the resident counts (include/singlet_hip.h, sgl_variable_features): Seurat's
// FindVariableFeatures(selection.method = "vst"), the selection RunNMF.Seurat reads as "var.features" (R/RunNMF.R:73-74).
// The header states the rules for the caller; this file holds
//   1. hvg_segment_kernel<MODE> / hvg_finish_kernel<MODE>: the three gene passes over t(A) (one column per gene, 64-bit
//      offsets).  A gene's entries, in stored order, are cut into segments of HVG_SEG; ONE WAVE PER SEGMENT: lane l adds the
//      terms of the segment's entries l, l + 64, ... in that order from +0.0, the 64 lane sums go through a butterfly
//      (lane ^ 32, 16, ... 1).  One lane per gene then adds the gene's segment sums in segment order from +0.0 and applies
//      the pass's closing formula.  MODE 0: term x, S / n.  MODE 1: term (x - mu)^2, (Q + (n - c) mu^2) / (n - 1).
//      MODE 2: term min((x - mu) / sd, vmax)^2, (Q + (n - c) ((0 - mu) / sd)^2) / (n - 1), +0.0 where sd == 0.
//      The segment table (gene of every segment, first segment of every gene) comes from the host, which reads the m + 1
//      offsets for it.  Bandwidth kernels: 8 bytes per stored entry, the offsets by scalar loads.
//   2. loess_direct_kernel: the trend, one wave per evaluation point: window search (every admissible start, lanes over
//      the starts), tricube weights, eight moment sums in fixed lanes and the same butterfly, the closed-form intercept.
//   3. the host side of the composite: log10, the sort by (x, gene), pow, sqrt, the ranking.
// No floating-point atomics, no loop whose trip count follows the launch size; compiled with -ffp-contract=off, so every
// product and the addition after it round separately: the results are functions of the inputs alone, restated operation by
// operation in tests/variable_features_restatement.py.
#include "sgl_internal.h"

#include <cmath>
#include <numeric>

#define HVG_THREADS 256
#define HVG_WAVES (HVG_THREADS / SGL_WAVE)
#define HVG_SEG 8192   // entries per segment: part of the stated summation order (header, restatement)
static_assert(HVG_SEG % (4 * SGL_WAVE) == 0, "a full segment is whole rounds of the unrolled lane loop");

__device__ __forceinline__ double hvg_wave_sum(double v) {
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SGL_WAVE);
    return v;
}

template <int MODE>
__device__ __forceinline__ double hvg_term(double x, double mu, double sd, double vmax) {
    if (MODE == 0) return x;
    if (MODE == 1) {
        const double d = x - mu;
        return d * d;
    }
    double z = (x - mu) / sd;
    z = z > vmax ? vmax : z;
    return z * z;
}

template <int MODE>
__global__ __launch_bounds__(HVG_THREADS) void hvg_segment_kernel(const double* __restrict__ x, const int64_t* __restrict__ p,
                                                                 const int32_t* __restrict__ seg_gene,
                                                                 const int64_t* __restrict__ seg_first, int64_t nseg,
                                                                 const double* __restrict__ mu, const double* __restrict__ sd,
                                                                 double vmax, double* __restrict__ part) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t seg = (int64_t)blockIdx.x * HVG_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (seg >= nseg) return;
    const int32_t g = seg_gene[seg];
    const int64_t lo = p[g] + (seg - seg_first[g]) * (int64_t)HVG_SEG;
    int64_t hi = p[g + 1];
    if (hi - lo > HVG_SEG) hi = lo + HVG_SEG;
    const double m = MODE ? mu[g] : 0.0;
    const double s = MODE == 2 ? sd[g] : 1.0;
    double acc = 0.0;
    if (MODE != 2 || s != 0.0) {   // (sd == 0: the closing formula gives +0.0 whatever is summed)
        int64_t q = lo + lane;
        // four entries in flight per lane; the additions stay in stored order
        for (; q + 3 * SGL_WAVE < hi; q += 4 * SGL_WAVE) {
            const double v0 = x[q], v1 = x[q + SGL_WAVE], v2 = x[q + 2 * SGL_WAVE], v3 = x[q + 3 * SGL_WAVE];
            acc += hvg_term<MODE>(v0, m, s, vmax);
            acc += hvg_term<MODE>(v1, m, s, vmax);
            acc += hvg_term<MODE>(v2, m, s, vmax);
            acc += hvg_term<MODE>(v3, m, s, vmax);
        }
        for (; q < hi; q += SGL_WAVE) acc += hvg_term<MODE>(x[q], m, s, vmax);
    }
    acc = hvg_wave_sum(acc);
    if (lane == 0) part[seg] = acc;
}

template <int MODE>
__global__ __launch_bounds__(HVG_THREADS) void hvg_finish_kernel(const double* __restrict__ part, const int64_t* __restrict__ seg_first,
                                                                const int64_t* __restrict__ p, int32_t ngenes, int64_t n,
                                                                const double* __restrict__ mu, const double* __restrict__ sd,
                                                                double* __restrict__ out, int64_t* __restrict__ count) {
    const int64_t g = (int64_t)blockIdx.x * HVG_THREADS + threadIdx.x;
    if (g >= ngenes) return;
    const int64_t s0 = seg_first[g], s1 = seg_first[g + 1];
    double q = 0.0;
    for (int64_t s = s0; s < s1; ++s) q += part[s];
    const int64_t c = p[g + 1] - p[g];
    if (MODE == 0) {
        out[g] = q / (double)n;
        count[g] = c;
        return;
    }
    const double m = mu[g];
    double z;
    if (MODE == 1) {
        z = (double)(n - c) * (m * m);
    } else {
        const double s = sd[g];
        if (s == 0.0) { out[g] = 0.0; return; }
        const double z0 = (0.0 - m) / s;
        z = (double)(n - c) * (z0 * z0);
    }
    out[g] = (q + z) / (double)(n - 1);
}

// One wave per evaluation point i of the sorted (x, y), n points, windows of q (1 <= q <= n, checked by the caller).
__global__ __launch_bounds__(HVG_THREADS) void loess_direct_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n,
                                                                  int64_t q, double* __restrict__ fitted) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t i = (int64_t)blockIdx.x * HVG_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= n) return;
    const double xi = x[i];
    // the window: the start s in [lo, hi] whose farthest member is nearest, ties to the lowest s
    const int64_t lo = i - q + 1 > 0 ? i - q + 1 : 0;
    const int64_t hi = i < n - q ? i : n - q;
    double bf = INFINITY;
    int64_t bs = hi + 1;
    for (int64_t s = lo + lane; s <= hi; s += SGL_WAVE) {   // ascending s per lane: `<` keeps the lowest
        const double a = xi - x[s], b = x[s + q - 1] - xi;
        const double f = a > b ? a : b;
        if (f < bf) { bf = f; bs = s; }
    }
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) {
        const double of = __shfl_xor(bf, off, SGL_WAVE);
        const long long os = __shfl_xor((long long)bs, off, SGL_WAVE);
        if (of < bf || (of == bf && os < bs)) { bf = of; bs = os; }
    }
    const double hmax = bf;
    const int64_t s0 = bs;
    if (s0 < lo || s0 > hi) {   // no finite distance (cannot happen on the finite ascending x the caller checked): no read out of range
        if (lane == 0) fitted[i] = NAN;
        return;
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0;
    int distinct = 0;
    for (int64_t j = s0 + lane; j < s0 + q; j += SGL_WAVE) {
        const double xj = x[j], yj = y[j];
        const double u = xj - xi;
        const double a = fabs(u);
        double w = 1.0;
        if (hmax != 0.0) {
            const double r = a / hmax;
            const double r3 = (r * r) * r;
            const double c = 1.0 - r3;
            w = (c * c) * c;
        }
        // a new distinct x among the members of positive weight (they are contiguous: |u| < hmax is an interval of the sorted x)
        if (hmax == 0.0 || a < hmax) {
            bool fresh = j == s0;
            if (!fresh) {
                const double xp = x[j - 1];
                fresh = xp != xj || !(hmax == 0.0 || fabs(xp - xi) < hmax);
            }
            distinct += fresh ? 1 : 0;
        }
        const double wu = w * u, wu2 = wu * u, wu3 = wu2 * u, wu4 = wu3 * u;
        S0 += w;
        S1 += wu;
        S2 += wu2;
        S3 += wu3;
        S4 += wu4;
        T0 += w * yj;
        T1 += wu * yj;
        T2 += wu2 * yj;
    }
    S0 = hvg_wave_sum(S0);
    S1 = hvg_wave_sum(S1);
    S2 = hvg_wave_sum(S2);
    S3 = hvg_wave_sum(S3);
    S4 = hvg_wave_sum(S4);
    T0 = hvg_wave_sum(T0);
    T1 = hvg_wave_sum(T1);
    T2 = hvg_wave_sum(T2);
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) distinct += __shfl_xor(distinct, off, SGL_WAVE);
    double fit;
    if (distinct >= 3) {
        const double A = S2 * S4 - S3 * S3;
        const double num = (T0 * A - S1 * (T1 * S4 - S3 * T2)) + S2 * (T1 * S3 - S2 * T2);
        const double den = (S0 * A - S1 * (S1 * S4 - S3 * S2)) + S2 * (S1 * S3 - S2 * S2);
        fit = num / den;
    } else if (distinct == 2) {
        fit = (S2 * T0 - S1 * T1) / (S0 * S2 - S1 * S1);
    } else {
        fit = T0 / S0;
    }
    if (lane == 0) fitted[i] = fit;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
namespace {
// the segment table of c->At and the pass's device arrays; built once per call (the composite shares it among its passes)
struct HvgPlan {
    DevBuf<int32_t> seg_gene;
    DevBuf<int64_t> seg_first, count;
    DevBuf<double> part, mu, sd, out;
    int64_t nseg = 0;
    int32_t m = 0;
};

int hvg_plan(sgl_ctx* c, HvgPlan& P) {
    const DevCSC& M = c->At;
    const int32_t m = M.ncol;
    P.m = m;
    std::vector<int64_t> p((size_t)m + 1), first((size_t)m + 1, 0);
    HIPCHK(hipMemcpyAsync(p.data(), M.p, sizeof(int64_t) * p.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int32_t g = 0; g < m; ++g) first[(size_t)g + 1] = first[g] + (p[(size_t)g + 1] - p[g] + HVG_SEG - 1) / HVG_SEG;
    P.nseg = first[m];
    if ((P.nseg + HVG_WAVES - 1) / HVG_WAVES > INT32_MAX) { sgl_set_error("variable features: %lld segments are more than one launch holds", (long long)P.nseg); return SGL_EINVAL; }
    std::vector<int32_t> sg((size_t)std::max<int64_t>(P.nseg, 1));
    for (int32_t g = 0; g < m; ++g)
        for (int64_t s = first[g]; s < first[(size_t)g + 1]; ++s) sg[(size_t)s] = g;
    SGLCHK(P.seg_gene.alloc(sg.size()));
    SGLCHK(P.seg_first.alloc(first.size()));
    SGLCHK(P.part.alloc(sg.size()));
    SGLCHK(P.mu.alloc((size_t)std::max(m, 1)));
    SGLCHK(P.sd.alloc((size_t)std::max(m, 1)));
    SGLCHK(P.out.alloc((size_t)std::max(m, 1)));
    SGLCHK(P.count.alloc((size_t)std::max(m, 1)));
    HIPCHK(hipMemcpyAsync(P.seg_gene.p, sg.data(), sizeof(int32_t) * sg.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.seg_first.p, first.data(), sizeof(int64_t) * first.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the host vectors go
    return SGL_OK;
}

template <int MODE>
int hvg_launch(sgl_ctx* c, HvgPlan& P, double vmax) {
    const DevCSC& M = c->At;
    Phase ph(c, SGL_PH_SCALE);   // where scripts/variable_features_rate.py reads the kernels' time
    if (P.nseg > 0) {
        hvg_segment_kernel<MODE><<<dim3((unsigned)((P.nseg + HVG_WAVES - 1) / HVG_WAVES)), dim3(HVG_THREADS), 0, c->stream>>>(
            M.x, M.p, P.seg_gene.p, P.seg_first.p, P.nseg, P.mu.p, P.sd.p, vmax, P.part.p);
        HIPCHK(hipGetLastError());
    }
    if (P.m > 0) {
        hvg_finish_kernel<MODE><<<dim3((unsigned)((P.m + HVG_THREADS - 1) / HVG_THREADS)), dim3(HVG_THREADS), 0, c->stream>>>(
            P.part.p, P.seg_first.p, M.p, P.m, (int64_t)M.nrow, P.mu.p, P.sd.p, P.out.p, P.count.p);
        HIPCHK(hipGetLastError());
    }
    return SGL_OK;
}

int hvg_pass_on(sgl_ctx* c, HvgPlan& P, int mode, const double* mu, const double* sd, double vmax, double* out, int64_t* count) {
    const size_t bytes = sizeof(double) * (size_t)P.m;
    if (P.m == 0) return SGL_OK;
    if (mode >= 1) HIPCHK(hipMemcpyAsync(P.mu.p, mu, bytes, hipMemcpyHostToDevice, c->stream));
    if (mode == 2) HIPCHK(hipMemcpyAsync(P.sd.p, sd, bytes, hipMemcpyHostToDevice, c->stream));
    SGLCHK(mode == 0 ? hvg_launch<0>(c, P, vmax) : mode == 1 ? hvg_launch<1>(c, P, vmax) : hvg_launch<2>(c, P, vmax));
    HIPCHK(hipMemcpyAsync(out, P.out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    if (mode == 0 && count) HIPCHK(hipMemcpyAsync(count, P.count.p, sizeof(int64_t) * (size_t)P.m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SGL_OK;
}

// every return path waits for the stream before the plan's buffers (and the caller's host arrays) go
int hvg_drain(sgl_ctx* c, int rc, const char* who) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("%s: HIP call failed: %s", who, hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}
}   // namespace

int sgl_hvg_pass(sgl_ctx* c, int mode, const double* mu, const double* sd, double vmax, double* out, int64_t* count) {
    HvgPlan P;
    int rc = hvg_plan(c, P);
    if (rc == SGL_OK) rc = hvg_pass_on(c, P, mode, mu, sd, vmax, out, count);
    return hvg_drain(c, rc, "variable features");
}

int sgl_loess_direct(sgl_ctx* c, const double* x, const double* y, int64_t n, int64_t q, double* fitted) {
    DevBuf<double> dx, dy, df;
    const size_t bytes = sizeof(double) * (size_t)n;
    int rc = dx.alloc((size_t)n);
    if (rc == SGL_OK) rc = dy.alloc((size_t)n);
    if (rc == SGL_OK) rc = df.alloc((size_t)n);
    if (rc == SGL_OK && (hipMemcpyAsync(dx.p, x, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                         hipMemcpyAsync(dy.p, y, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)) rc = SGL_EHIP;
    if (rc == SGL_OK) {
        Phase ph(c, SGL_PH_SCALE);
        loess_direct_kernel<<<dim3((unsigned)((n + HVG_WAVES - 1) / HVG_WAVES)), dim3(HVG_THREADS), 0, c->stream>>>(dx.p, dy.p, n, q, df.p);
        if (hipGetLastError() != hipSuccess) rc = SGL_EHIP;
    }
    if (rc == SGL_OK && hipMemcpyAsync(fitted, df.p, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = SGL_EHIP;
    if (rc == SGL_EHIP) sgl_set_error("sgl_op_loess_direct: HIP call failed");
    return hvg_drain(c, rc, "sgl_op_loess_direct");
}

int sgl_hvg_args_check(const char* who, int32_t nrow, int32_t ncol, int32_t nfeatures, double span, const double* expected_var,
                       const int32_t* features, const int32_t* n_out) {
    if (!features || !n_out) { sgl_set_error("%s: NULL features or n_out", who); return SGL_EINVAL; }
    if (nfeatures < 1) { sgl_set_error("%s: nfeatures = %d: at least one feature is selected", who, nfeatures); return SGL_EINVAL; }
    if (!(span > 0.0 && span <= 1.0)) { sgl_set_error("%s: span = %g is outside (0, 1]", who, span); return SGL_EINVAL; }
    if (ncol < 2) { sgl_set_error("%s: ncol = %d: a variance needs at least two cells", who, ncol); return SGL_EINVAL; }
    if (expected_var)
        for (int32_t g = 0; g < nrow; ++g)
            if (!(expected_var[g] >= 0.0) || std::isinf(expected_var[g])) {
                sgl_set_error("%s: expected_var[%d] = %g: an expected variance is finite and not negative", who, g, expected_var[g]);
                return SGL_EINVAL;
            }
    return SGL_OK;
}

static int hvg_select_on(sgl_ctx* c, HvgPlan& P, int32_t nfeatures, double span, double vmax, const double* expected_var,
                         int32_t* features, int32_t* n_out, double* info) {
    const int32_t m = c->A.nrow;
    const int64_t n = c->A.ncol;
    std::vector<double> mean((size_t)m), var((size_t)m), expd((size_t)m, 0.0), sd((size_t)m), stdv((size_t)m);
    SGLCHK(hvg_pass_on(c, P, 0, nullptr, nullptr, 0.0, mean.data(), nullptr));
    SGLCHK(hvg_pass_on(c, P, 1, mean.data(), nullptr, 0.0, var.data(), nullptr));
    std::vector<int32_t> live;   // the genes of positive variance
    for (int32_t g = 0; g < m; ++g)
        if (var[g] > 0.0) {
            if (!(mean[g] > 0.0)) {
                sgl_set_error("sgl_variable_features: gene %d has variance %g but mean %g: the selection is defined on counts "
                              "(log10 of a mean that is not positive)", g, var[g], mean[g]);
                return SGL_EINVAL;
            }
            live.push_back(g);
        }
    if (expected_var) {
        std::copy(expected_var, expected_var + m, expd.begin());
    } else if (!live.empty()) {
        const int64_t ml = (int64_t)live.size();
        std::vector<double> lx((size_t)m);
        for (int32_t g : live) lx[g] = log10(mean[g]);
        std::sort(live.begin(), live.end(), [&](int32_t a, int32_t b) { return lx[a] < lx[b] || (lx[a] == lx[b] && a < b); });
        std::vector<double> xs((size_t)ml), ys((size_t)ml), fit((size_t)ml);
        for (int64_t r = 0; r < ml; ++r) { xs[r] = lx[live[r]]; ys[r] = log10(var[live[r]]); }
        const int64_t q = std::max<int64_t>(std::min<int64_t>(ml, 3), (int64_t)floor(span * (double)ml));
        SGLCHK(sgl_loess_direct(c, xs.data(), ys.data(), ml, q, fit.data()));
        for (int64_t r = 0; r < ml; ++r) expd[live[r]] = pow(10.0, fit[r]);
    }
    for (int32_t g = 0; g < m; ++g) sd[g] = sqrt(expd[g]);
    if (!(vmax > 0.0)) vmax = sqrt((double)n);
    SGLCHK(hvg_pass_on(c, P, 2, mean.data(), sd.data(), vmax, stdv.data(), nullptr));
    // rank: standardised variance descending, ties to the lower gene index, NaN last
    std::vector<int32_t> order((size_t)m);
    std::iota(order.begin(), order.end(), 0);
    auto key = [&](int32_t g) { return std::isnan(stdv[g]) ? -INFINITY : stdv[g]; };
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key(a) > key(b); });
    const int32_t take = std::min(nfeatures, m);
    std::copy(order.begin(), order.begin() + take, features);
    *n_out = take;
    if (info)
        for (int32_t g = 0; g < m; ++g) {
            info[4 * (size_t)g] = mean[g];
            info[4 * (size_t)g + 1] = var[g];
            info[4 * (size_t)g + 2] = expd[g];
            info[4 * (size_t)g + 3] = stdv[g];
        }
    return SGL_OK;
}

int sgl_hvg_select(sgl_ctx* c, int32_t nfeatures, double span, double vmax, const double* expected_var, int32_t* features,
                   int32_t* n_out, double* info) {
    HvgPlan P;
    int rc = hvg_plan(c, P);
    if (rc == SGL_OK) rc = hvg_select_on(c, P, nfeatures, span, vmax, expected_var, features, n_out, info);
    return hvg_drain(c, rc, "sgl_variable_features");
}
