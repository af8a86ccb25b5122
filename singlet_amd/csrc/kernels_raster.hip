// Row-wise rasterisation (RasterizeRowwise, R/rasterize_rowwise.R): rowwise_compress_sparse / rowwise_compress_dense
// (src/singlet.cpp:146-180) on the GPU.  Entry (b, j) of the floor(nrow / n) x ncol result is the mean of rows
// [b n, b n + n) of column j: the sum in ascending row order from +0.0, then one IEEE division by (double)n.  The last
// nrow mod n rows are left out (the reference is undefined there: include/singlet_hip.h, sgl_c_rowwise_compress_sparse).
//
// Why the sparse and the dense forms, and this build and the reference, agree bit for bit: the dense sum adds every row of
// the bin, the sparse sum only the stored entries; the difference is a number of additions of +0.0.  Adding +0.0 changes no
// running sum s except s = -0.0 (-0.0 + +0.0 = +0.0), and a sum that starts at +0.0 and adds values in order is never -0.0:
// +0.0 + x is x for x != 0 and +0.0 for x = +-0.0, and a non-zero s + x rounds to -0.0 never (an exact zero of a sum of
// two finite numbers is +0.0 in round-to-nearest; NaN and +-Inf are not -0.0).  So skipping zeros, stored -0.0 included,
// leaves every partial sum as it is.  Only additions and one division: no contraction is possible, and the unit is built
// with -ffp-contract=off all the same.
#include "sgl_internal.h"

#pragma clang fp contract(off)

namespace {

// ---- sparse: one 64-lane workgroup per column --------------------------------------------------------------------------
// The column's bins are taken in chunks of 64, lane l owning bin B0 + l; its entries are taken in windows of 64 (one entry
// per lane, coalesced), each entry read once.  The rows ascend, so the entries of one bin are one run of consecutive
// lanes: the first and last lane of every run in the chunk write the run's bounds to LDS at the owner's slot, and the
// owner adds the run from LDS, in order.  A window whose last entry lies beyond the chunk stays for the next chunk; a
// window that ends inside it is replaced by the next one.  When the chunk is done every owner writes its mean (empty bins
// +0.0 / n = +0.0): each output element is written once, 64 consecutive doubles per store.  Entries of the last
// nrow mod n rows have bins >= nb and fall in no chunk.
__global__ __launch_bounds__(64) void raster_sparse_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                           const int64_t* __restrict__ p, int64_t ncol, uint32_t n, int64_t nb,
                                                           double* __restrict__ out) {
    __shared__ double sv[64];
    __shared__ int st[64], en[64];
    const int lane = threadIdx.x;
    const double dn = (double)n;
    for (int64_t col = blockIdx.x; col < ncol; col += gridDim.x) {
        const int64_t hi = p[col + 1];
        int64_t e0 = p[col];   // first entry of the window
        double v = 0.0;
        int64_t bin = INT64_MAX;   // bin of this lane's entry; INT64_MAX past the column's end
        if (e0 + lane < hi) {
            v = x[e0 + lane];
            bin = (uint32_t)idx[e0 + lane] / n;
        }
        double* o = out + col * nb;
        double acc = 0.0;
        for (int64_t B0 = 0; B0 < nb;) {
            const int64_t Bend = std::min<int64_t>(B0 + 64, nb);
            const bool in = bin >= B0 && bin < Bend;
            if (__ballot(in)) {
                st[lane] = 0;
                en[lane] = 0;
                sv[lane] = v;
                __syncthreads();
                const int64_t prev = __shfl(bin, lane == 0 ? 0 : lane - 1), next = __shfl(bin, lane == 63 ? 63 : lane + 1);
                if (in && (lane == 0 || prev != bin)) st[bin - B0] = lane;
                if (in && (lane == 63 || next != bin)) en[bin - B0] = lane + 1;
                __syncthreads();
                const int s = st[lane], t = en[lane];
                for (int k = s; k < t; ++k) acc += sv[k];
                __syncthreads();   // the next window or chunk rewrites the LDS
            }
            // the window ends inside the chunk and more entries follow: the next window may hold more of the chunk
            const int64_t nv = std::min<int64_t>(64, hi - e0);
            if (nv > 0 && __shfl(bin, (int)nv - 1) < Bend && e0 + 64 < hi) {
                e0 += 64;
                v = 0.0;
                bin = INT64_MAX;
                if (e0 + lane < hi) {
                    v = x[e0 + lane];
                    bin = (uint32_t)idx[e0 + lane] / n;
                }
                continue;
            }
            if (B0 + lane < nb) o[B0 + lane] = acc / dn;
            acc = 0.0;
            B0 += 64;
        }
    }
}

// ---- dense: a workgroup of 256 lanes per tile of 256 bins of one column ------------------------------------------------
// The tile's rows (256 n consecutive doubles of the column) are staged through LDS in pieces of RD_PIECE rows with
// coalesced loads; after each piece lane l adds the rows of bin B0 + l inside it, in order, to its running sum.  One pass
// over the first nb n rows of every column, one store per output element.
constexpr int RD_BINS = 256;
constexpr int RD_PIECE = 4096;   // 32 KB of LDS

__global__ __launch_bounds__(RD_BINS) void raster_dense_kernel(const double* __restrict__ A, int64_t nrow, int64_t ncol, uint32_t n,
                                                               int64_t nb, double* __restrict__ out) {
    __shared__ double sh[RD_PIECE];
    const int lane = threadIdx.x;
    const double dn = (double)n;
    const int64_t tiles_per_col = (nb + RD_BINS - 1) / RD_BINS, ntiles = tiles_per_col * ncol;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t col = t / tiles_per_col, B0 = (t - col * tiles_per_col) * RD_BINS;
        const int64_t nbins = std::min<int64_t>(RD_BINS, nb - B0), span = nbins * n;
        const double* a = A + col * nrow + B0 * n;
        const int64_t r0 = (int64_t)lane * n, r1 = r0 + n;   // this lane's rows, relative to the tile
        double acc = 0.0;
        for (int64_t q0 = 0; q0 < span; q0 += RD_PIECE) {
            const int m = (int)std::min<int64_t>(RD_PIECE, span - q0);
            __syncthreads();   // the previous piece has been read
#pragma unroll 4
            for (int k = lane; k < m; k += RD_BINS) sh[k] = a[q0 + k];
            __syncthreads();
            if (lane < nbins) {
                const int64_t s = std::max(r0, q0), e = std::min<int64_t>(r1, q0 + m);
                for (int64_t r = s; r < e; ++r) acc += sh[r - q0];
            }
        }
        if (lane < nbins) out[col * nb + B0 + lane] = acc / dn;
    }
}

unsigned grid_cap(int64_t units) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(units, 1 << 16)); }

int hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return SGL_OK;
    (void)hipGetLastError();
    sgl_set_error("%s failed: %s", what, hipGetErrorString(e));
    return SGL_EHIP;
}
#define RCHK(expr, what) SGLCHK(hip_ok((expr), what))

}  // namespace

// nb = floor(A.nrow / n) >= 1 and n <= A.nrow (so n fits 32 bits); A a valid CSC image (rows in [0, nrow), ascending).
int k_raster_sparse(hipStream_t s, const DevCSC& A, int64_t n, int64_t nb, double* out) {
    if (A.ncol <= 0 || nb <= 0) return SGL_OK;
    raster_sparse_kernel<<<dim3(grid_cap(A.ncol)), dim3(64), 0, s>>>(A.x, A.i, A.p, A.ncol, (uint32_t)n, nb, out);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

int k_raster_dense(hipStream_t s, const double* A, int64_t nrow, int64_t ncol, int64_t n, int64_t nb, double* out) {
    if (ncol <= 0 || nb <= 0) return SGL_OK;
    const int64_t tiles = (nb + RD_BINS - 1) / RD_BINS * ncol;
    raster_dense_kernel<<<dim3(grid_cap(tiles)), dim3(RD_BINS), 0, s>>>(A, nrow, ncol, (uint32_t)n, nb, out);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

static int bin_count(const char* who, int32_t nrow, int64_t n, int64_t* nb) {
    if (n < 1) { sgl_set_error("%s: n = %lld: the bin size must be at least 1", who, (long long)n); return SGL_EINVAL; }
    *nb = n > nrow ? 0 : nrow / n;
    return SGL_OK;
}

extern "C" int sgl_c_rowwise_compress_sparse(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol,
                                             int64_t n, double* out) {
    const char* who = "rowwise_compress_sparse";
    if (!Ap || nrow < 0 || ncol < 0) { sgl_set_error("%s: missing column pointers or negative dimensions", who); return SGL_EINVAL; }
    int64_t nb = 0;
    SGLCHK(bin_count(who, nrow, n, &nb));
    if (nb * (int64_t)ncol > 0 && !out) { sgl_set_error("%s: NULL output", who); return SGL_EINVAL; }
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    if (nrow == 0 || ncol == 0) {   // nothing can be stored; nothing to write
        if (Ap[0] != 0 || Ap[ncol] != 0) { sgl_set_error("%s: a matrix with %d rows and %d columns holds no entries", who, nrow, ncol); return SGL_EINVAL; }
        return SGL_OK;
    }
    if (!Ax || !Ai) { sgl_set_error("%s: missing slot", who); return SGL_EINVAL; }
    sgl_ctx* c = hd.c;
    SGLCHK(sgl_upload_A_structure(c, Ax, Ai, Ap, nrow, ncol));   // row indices valid and ascending; values as they are
    if (nb == 0) return SGL_OK;
    const size_t tot = (size_t)nb * (size_t)ncol;
    DevBuf<double> R;
    SGLCHK(R.alloc(tot));
    SGLCHK(k_raster_sparse(c->stream, c->A, n, nb, R.p));
    RCHK(hipMemcpyAsync(out, R.p, sizeof(double) * tot, hipMemcpyDeviceToHost, c->stream), "download of the result");
    RCHK(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    return SGL_OK;
}

extern "C" int sgl_c_rowwise_compress_dense(const double* A, int32_t nrow, int32_t ncol, int64_t n, double* out) {
    const char* who = "rowwise_compress_dense";
    if (nrow < 0 || ncol < 0 || (!A && (int64_t)nrow * ncol > 0)) { sgl_set_error("%s: missing matrix or negative dimensions", who); return SGL_EINVAL; }
    int64_t nb = 0;
    SGLCHK(bin_count(who, nrow, n, &nb));
    if (nb * (int64_t)ncol > 0 && !out) { sgl_set_error("%s: NULL output", who); return SGL_EINVAL; }
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    if (nb == 0 || ncol == 0) return SGL_OK;
    hipStream_t s = hd.c->stream;
    const size_t tin = (size_t)nrow * (size_t)ncol, tot = (size_t)nb * (size_t)ncol;
    DevBuf<double> dA, R;
    SGLCHK(dA.alloc(tin));
    SGLCHK(R.alloc(tot));
    RCHK(hipMemcpyAsync(dA.p, A, sizeof(double) * tin, hipMemcpyHostToDevice, s), "upload of A");
    SGLCHK(k_raster_dense(s, dA.p, nrow, ncol, n, nb, R.p));
    RCHK(hipMemcpyAsync(out, R.p, sizeof(double) * tot, hipMemcpyDeviceToHost, s), "download of the result");
    RCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    return SGL_OK;
}
