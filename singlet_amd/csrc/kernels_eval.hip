// Model error (include/singlet_hip.h, sgl_evaluate): per column j of one orientation of the resident matrix the sum of the
// squared residuals over ALL rows, zeros included, from the sparse structure alone:
//
//     loss[j] = sum_i (A_ij - sum_f x_fj F^_fi)^2 = ||a_j||^2 - 2 x_j . b_j + x_j^T G x_j,      b_j = F^ a_j,   G = F^ F^^T
//
// Cell side: columns of A, x = h, F^ = diag(d) w.  Gene side: columns of At, x = w, F^ = diag(d) h.  b is what the fit's
// accumulate produces and G its Gram (diag_add = 0); this file adds the three pieces an ALS iteration does not have:
//   1. eval_colsumsq_kernel: ||a_j||^2.  One wave per column (64-bit offsets); lane l adds the squares of the entries
//      l, l + 64, ... of the column in stored order, the 64 lane sums are added by a butterfly (lane ^ 32, 16, ... 1).
//   2. eval_epilogue_kernel: one workgroup per EVAL_BLOCK_COLS columns, G staged in LDS once per workgroup up to
//      k = EVAL_G_LDS_MAX_K (k^2 doubles: 128 KiB of the CU's 160) and read through the cache above.  A wave carries
//      EVAL_WCOLS columns at once through G, so every element of G is loaded once per four columns; lane f (and f + 64, ...)
//      forms t_f = sum_g G[f, g] x_g with g ascending, then x_f t_f and x_f b_f; the lane sums go through the butterfly.
//      loss = (ss - 2 dot) + quad, and a result <= 0 becomes +0.0 when `clamp` (NaN stays NaN).
//   3. eval_chunk_sum_kernel / eval_finish_kernel: the sum of the losses.  Chunks of EVAL_CHUNK = 1024 consecutive columns;
//      thread t of 256 adds the columns t, t + 256, t + 512, t + 768 of its chunk in that order, the 256 sums are added by a
//      binary tree in LDS (t += t + stride, stride = 128 ... 1); one lane adds the chunk sums in chunk order from +0.0.
// No floating-point atomics and no loop whose trip count follows the launch size: every result is a function of (matrix, k,
// factors) alone.  The scaled factor F^ is made in the fit's scratch (red / B), never over W or H.
#include "sgl_internal.h"

#define EVAL_THREADS 256
#define EVAL_WAVES (EVAL_THREADS / SGL_WAVE)
#define EVAL_WCOLS 4
#define EVAL_BLOCK_COLS 256
#define EVAL_ROUNDS (EVAL_BLOCK_COLS / (EVAL_WAVES * EVAL_WCOLS))
#define EVAL_CHUNK 1024
#define EVAL_G_LDS_MAX_K 128
// dynamic LDS of the epilogue: [k x k of G when staged] + EVAL_WAVES x EVAL_WCOLS columns of x
#define EVAL_LDS_MAX_BYTES (8 * (EVAL_G_LDS_MAX_K * EVAL_G_LDS_MAX_K + EVAL_WAVES * EVAL_WCOLS * EVAL_G_LDS_MAX_K))
static_assert(8 * EVAL_WAVES * EVAL_WCOLS * SGL_MAX_K <= EVAL_LDS_MAX_BYTES, "the x columns of the largest rank fit the same budget");
static_assert(EVAL_LDS_MAX_BYTES <= 160 * 1024, "one CU's LDS");
static_assert(EVAL_CHUNK % EVAL_THREADS == 0, "a chunk is whole rounds of the threads");

__device__ __forceinline__ double eval_wave_sum(double v) {
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SGL_WAVE);
    return v;
}

__global__ __launch_bounds__(EVAL_THREADS) void eval_colsumsq_kernel(const double* __restrict__ x, const int64_t* __restrict__ p,
                                                                    int64_t ncols, double* __restrict__ ss) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t col = (int64_t)blockIdx.x * EVAL_WAVES + (threadIdx.x >> 6);
    if (col >= ncols) return;
    const int64_t hi = p[col + 1];
    int64_t q = p[col] + lane;
    double acc = 0.0;
    // four entries in flight per lane; the additions stay in stored order
    for (; q + 3 * SGL_WAVE < hi; q += 4 * SGL_WAVE) {
        const double v0 = x[q], v1 = x[q + SGL_WAVE], v2 = x[q + 2 * SGL_WAVE], v3 = x[q + 3 * SGL_WAVE];
        acc = fma(v0, v0, acc);
        acc = fma(v1, v1, acc);
        acc = fma(v2, v2, acc);
        acc = fma(v3, v3, acc);
    }
    for (; q < hi; q += SGL_WAVE) acc = fma(x[q], x[q], acc);
    acc = eval_wave_sum(acc);
    if (lane == 0) ss[col] = acc;
}

// X, B: k x ncols column-major; G: k x k; loss holds ||a_j||^2 on entry and the loss on return
template <bool G_LDS>
__global__ __launch_bounds__(EVAL_THREADS) void eval_epilogue_kernel(const double* __restrict__ X, const double* __restrict__ B,
                                                                    const double* __restrict__ G, int k, int64_t ncols,
                                                                    double* __restrict__ loss, int clamp) {
    extern __shared__ double eval_lds[];
    const int lane = threadIdx.x & (SGL_WAVE - 1), wave = threadIdx.x >> 6;
    double* xs = eval_lds + (G_LDS ? k * k : 0) + wave * (EVAL_WCOLS * k);
    if (G_LDS)
        for (int e = threadIdx.x; e < k * k; e += EVAL_THREADS) eval_lds[e] = G[e];
    const double* Gm = G_LDS ? eval_lds : G;
    const int64_t c0 = (int64_t)blockIdx.x * EVAL_BLOCK_COLS;
    for (int round = 0; round < EVAL_ROUNDS; ++round) {   // the same trip count for every wave: the barrier below is uniform
        const int64_t col = c0 + (int64_t)(round * EVAL_WAVES + wave) * EVAL_WCOLS;
        // the wave's columns are contiguous in X; columns past the end read as zeros
        for (int e = lane; e < EVAL_WCOLS * k; e += SGL_WAVE) xs[e] = (col + e / k < ncols) ? X[col * k + e] : 0.0;
        __syncthreads();   // x (and, in round 0, G) is in LDS; a wave's own buffer is rewritten only after its own reads
        double quad[EVAL_WCOLS], dot[EVAL_WCOLS];
#pragma unroll
        for (int c = 0; c < EVAL_WCOLS; ++c) quad[c] = dot[c] = 0.0;
        for (int f = lane; f < k; f += SGL_WAVE) {
            double t[EVAL_WCOLS];
#pragma unroll
            for (int c = 0; c < EVAL_WCOLS; ++c) t[c] = 0.0;
            for (int g = 0; g < k; ++g) {
                const double gv = Gm[g * k + f];
#pragma unroll
                for (int c = 0; c < EVAL_WCOLS; ++c) t[c] = fma(gv, xs[c * k + g], t[c]);
            }
#pragma unroll
            for (int c = 0; c < EVAL_WCOLS; ++c) {
                const double xf = xs[c * k + f];
                quad[c] = fma(xf, t[c], quad[c]);
                if (col + c < ncols) dot[c] = fma(xf, B[(col + c) * k + f], dot[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < EVAL_WCOLS; ++c) {
            const double q = eval_wave_sum(quad[c]), d = eval_wave_sum(dot[c]);
            if (lane == 0 && col + c < ncols) {
                double v = (loss[col + c] - 2.0 * d) + q;
                if (clamp && v <= 0.0) v = 0.0;   // cancellation (the true value is >= 0); NaN <= 0 is false
                loss[col + c] = v;
            }
        }
    }
}

__global__ __launch_bounds__(EVAL_THREADS) void eval_chunk_sum_kernel(const double* __restrict__ loss, int64_t n, double* __restrict__ part) {
    __shared__ double tree[EVAL_THREADS];
    const int64_t base = (int64_t)blockIdx.x * EVAL_CHUNK;
    double a = 0.0;
#pragma unroll
    for (int r = 0; r < EVAL_CHUNK / EVAL_THREADS; ++r) {
        const int64_t q = base + r * EVAL_THREADS + threadIdx.x;
        if (q < n) a += loss[q];
    }
    tree[threadIdx.x] = a;
    __syncthreads();
    for (int stride = EVAL_THREADS >> 1; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) tree[threadIdx.x] += tree[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = tree[0];
}

__global__ void eval_finish_kernel(const double* __restrict__ part, int64_t nchunks, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
#pragma unroll 8
    for (int64_t ch = 0; ch < nchunks; ++ch) s += part[ch];
    out[0] = s;
}

// losses of one side into dloss (device, one per column).  side 0: cells (A, x = H, F^ = d W in red, b in B); side 1: genes
// (At, x = W, F^ = d H in B, b in red).  red, B, G and the workspace are scratch every half-iteration fills before it reads.
static int eval_side(sgl_ctx* c, int side, bool clamp, double* dloss) {
    const int k = c->k;
    const DevCSC& M = side ? c->At : c->A;
    const DevTiled& T = side ? c->TAt : c->TA;
    const int64_t ncols = M.ncol, nsrc = M.nrow;
    const double* X = side ? c->W : c->H;
    double* Fs = side ? c->B : c->red;
    double* Bs = side ? c->red : c->B;
    if (ncols <= 0) return SGL_OK;
    hipStream_t s = c->stream;
    SGLCHK(k_wd(s, side ? c->H : c->W, c->d, k, nsrc, Fs));
    { Phase ph(c, SGL_PH_GRAM); SGLCHK(k_gram(c, Fs, k, nsrc, c->G, 0.0)); }
    { Phase ph(c, side ? SGL_PH_RHS_W : SGL_PH_RHS_H);
      if (M.nnz == 0) HIPCHK(hipMemsetAsync(Bs, 0, sizeof(double) * (size_t)k * (size_t)ncols, s));
      else if (c->use_tiled && T.roff) SGLCHK(k_acc_tiled_all(s, T, Fs, Bs, k));
      else SGLCHK(k_acc(s, M, Fs, k, Bs, 0, 1, 0, 0, 0)); }
    eval_colsumsq_kernel<<<dim3((unsigned)((ncols + EVAL_WAVES - 1) / EVAL_WAVES)), dim3(EVAL_THREADS), 0, s>>>(M.x, M.p, ncols, dloss);
    HIPCHK(hipGetLastError());
    const dim3 g((unsigned)((ncols + EVAL_BLOCK_COLS - 1) / EVAL_BLOCK_COLS)), b(EVAL_THREADS);
    const size_t xbytes = sizeof(double) * EVAL_WAVES * EVAL_WCOLS * (size_t)k;
    if (k <= EVAL_G_LDS_MAX_K) {
        SGLCHK(sgl_allow_dynamic_lds<&eval_epilogue_kernel<true>>(EVAL_LDS_MAX_BYTES));
        eval_epilogue_kernel<true><<<g, b, sizeof(double) * (size_t)k * k + xbytes, s>>>(X, Bs, c->G, k, ncols, dloss, clamp ? 1 : 0);
    } else {
        SGLCHK(sgl_allow_dynamic_lds<&eval_epilogue_kernel<false>>(EVAL_LDS_MAX_BYTES));
        eval_epilogue_kernel<false><<<g, b, xbytes, s>>>(X, Bs, c->G, k, ncols, dloss, clamp ? 1 : 0);
    }
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

static int eval_shard_enqueue(sgl_ctx* c, bool clamp_genes, double* cell_sum, double* cell_loss, double* gene_loss, DevBuf<double>& dcell,
                              DevBuf<double>& dgene, DevBuf<double>& dpart) {
    const int64_t n = c->A.ncol, m = c->A.nrow;
    const int64_t nchunks = (n + EVAL_CHUNK - 1) / EVAL_CHUNK;
    hipStream_t s = c->stream;
    SGLCHK(dcell.alloc((size_t)std::max<int64_t>(n, 1)));
    SGLCHK(dpart.alloc((size_t)nchunks + 1));
    SGLCHK(eval_side(c, 0, true, dcell.p));
    if (nchunks > 0) {
        eval_chunk_sum_kernel<<<dim3((unsigned)nchunks), dim3(EVAL_THREADS), 0, s>>>(dcell.p, n, dpart.p);
        HIPCHK(hipGetLastError());
    }
    eval_finish_kernel<<<dim3(1), dim3(SGL_WAVE), 0, s>>>(dpart.p, nchunks, dpart.p + nchunks);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cell_sum, dpart.p + nchunks, sizeof(double), hipMemcpyDeviceToHost, s));
    if (cell_loss && n > 0) HIPCHK(hipMemcpyAsync(cell_loss, dcell.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (gene_loss && m > 0) {
        SGLCHK(dgene.alloc((size_t)m));
        SGLCHK(eval_side(c, 1, clamp_genes, dgene.p));
        HIPCHK(hipMemcpyAsync(gene_loss, dgene.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, s));
    }
    return SGL_OK;
}

int sgl_eval_shard(sgl_ctx* c, bool clamp_genes, double* cell_sum, double* cell_loss, double* gene_loss) {
    DevBuf<double> dcell, dgene, dpart;
    const int rc = eval_shard_enqueue(c, clamp_genes, cell_sum, cell_loss, gene_loss, dcell, dgene, dpart);
    // the device buffers are released on return: nothing may still be in flight then
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc != SGL_OK) return rc;
    if (e != hipSuccess) { sgl_set_error("sgl_evaluate: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return SGL_OK;
}
