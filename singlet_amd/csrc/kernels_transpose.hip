// Device-side replacement of Matrix::t(A) (R/run_nmf.R:40): CSC of the shard
// -> CSC of its transpose, row indices ascending within each column.  A stable
// radix sort of the non-zeros by row index keeps the (ascending) column order
// inside every row, which is exactly what R's t() produces.  HBM-bound index
// work; rocPRIM (via hipcub) does the sort.
#include "sgl_internal.h"
#include <hipcub/hipcub.hpp>

// Columns [c0, c1) of A, whose entries are [q0, ...): colof = column of each entry, iota = its position local to
// the batch (the values the sort carries; < 2^31 by the batch cap).
__global__ void expand_cols_kernel(const int64_t* __restrict__ p, int64_t c0, int64_t c1, int64_t q0,
                                   int32_t* __restrict__ colof, uint32_t* __restrict__ iota) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = c0 + wave; c < c1; c += nwaves) {
        const int64_t lo = p[c], hi = p[c + 1];
        for (int64_t q = lo + lane; q < hi; q += 64) {
            colof[q - q0] = (int32_t)c;
            iota[q - q0] = (uint32_t)(q - q0);
        }
    }
}

__global__ void row_hist_kernel(const int32_t* __restrict__ idx, int64_t nnz, unsigned long long* __restrict__ counts) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&counts[idx[q]], 1ull);
}

// One batch for the whole matrix: sorted position d is the position in t(A).
__global__ void gather_kernel(const uint32_t* __restrict__ perm, int64_t nnz, const int32_t* __restrict__ colof,
                              const double* __restrict__ x, int32_t* __restrict__ ti, double* __restrict__ tx) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < nnz; d += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t q = perm[d];
        ti[d] = colof[q];
        tx[d] = x[q];
    }
}

// Batched: rstart[r] = first sorted position of row r in this batch (rows absent from the batch are not written and
// not read).
__global__ void run_start_kernel(const int32_t* __restrict__ keys, int64_t n, int64_t* __restrict__ rstart) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x)
        if (d == 0 || keys[d - 1] != keys[d]) rstart[keys[d]] = d;
}

// Batched: entry d of the sorted batch goes to cursor[r] + (d - rstart[r]); cursor[r] = T.p[r] + the entries of row r
// in the earlier batches (lower columns), so rows stay in ascending column order.  x points at the batch's first entry.
__global__ void gather_batch_kernel(const int32_t* __restrict__ keys, const uint32_t* __restrict__ perm, int64_t n,
                                    const int64_t* __restrict__ rstart, const int64_t* __restrict__ cursor,
                                    const int32_t* __restrict__ colof, const double* __restrict__ x,
                                    int32_t* __restrict__ ti, double* __restrict__ tx) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = keys[d];
        const int64_t dst = cursor[r] + (d - rstart[r]);
        const uint32_t q = perm[d];
        ti[dst] = colof[q];
        tx[dst] = x[q];
    }
}

// Batched, after the gather: the last entry of each row's run moves that row's cursor past the batch.
__global__ void advance_kernel(const int32_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ rstart,
                               int64_t* __restrict__ cursor) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x)
        if (d == n - 1 || keys[d + 1] != keys[d]) cursor[keys[d]] += d + 1 - rstart[keys[d]];
}

static unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32); }

template <typename T>
static int talloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = sgl_pool_malloc((void**)p, count * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sgl_set_error("hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
        return SGL_ENOMEM;
    }
    return SGL_OK;
}

// Fills T (empty on entry) with the transpose of A, sorting at most max_batch_entries non-zeros at a time (<= 0: the default, 2^31 - 1).  A batch
// is a run of whole columns (a column with more entries than the cap is a batch of its own; no column holds 2^31 or
// more), so the positions the sort carries fit in 32 bits at any nnz and the temporaries stay at one batch.  A matrix
// that fits one batch takes the single sort and gather.
int sgl_device_transpose_into(sgl_ctx* c, const DevCSC& A, DevCSC& T, int64_t max_batch_entries) {
    hipStream_t s = c->stream;
    const int64_t nnz = A.nnz;
    const int64_t cap = (max_batch_entries <= 0 || max_batch_entries > INT32_MAX) ? (int64_t)INT32_MAX : max_batch_entries;
    T.nrow = A.ncol;
    T.ncol = A.nrow;
    T.nnz = nnz;
    SGLCHK(talloc(&T.x, (size_t)nnz));
    SGLCHK(talloc(&T.i, (size_t)nnz));
    SGLCHK(talloc(&T.p, (size_t)T.ncol + 1));

    // batch boundaries (columns) from A's column pointers
    std::vector<int64_t> cut{0, (int64_t)A.ncol}, hp;
    int64_t max_n = nnz;
    if (nnz > cap) {
        hp.resize((size_t)A.ncol + 1);
        HIPCHK(hipMemcpyAsync(hp.data(), A.p, sizeof(int64_t) * hp.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        cut.assign(1, 0);
        max_n = 0;
        for (int64_t c0 = 0; c0 < A.ncol;) {
            int64_t c1 = c0 + 1;
            while (c1 < A.ncol && hp[(size_t)c1 + 1] - hp[(size_t)c0] <= cap) ++c1;
            max_n = std::max(max_n, hp[(size_t)c1] - hp[(size_t)c0]);
            cut.push_back(c1);
            c0 = c1;
        }
    }
    const bool batched = cut.size() > 2;

    int64_t *counts = nullptr, *cursor = nullptr, *rstart = nullptr;
    int32_t *colof = nullptr, *keys_out = nullptr;
    uint32_t *iota = nullptr, *perm = nullptr;
    void* tmp = nullptr;
    size_t tmp_cap = 0;
    int rc = SGL_OK;
    do {
        if ((rc = talloc(&counts, (size_t)T.ncol)) != SGL_OK) break;
        if ((rc = talloc(&colof, (size_t)max_n)) != SGL_OK) break;
        if ((rc = talloc(&keys_out, (size_t)max_n)) != SGL_OK) break;
        if ((rc = talloc(&iota, (size_t)max_n)) != SGL_OK) break;
        if ((rc = talloc(&perm, (size_t)max_n)) != SGL_OK) break;
        if (batched) {
            if ((rc = talloc(&cursor, (size_t)T.ncol)) != SGL_OK) break;
            if ((rc = talloc(&rstart, (size_t)T.ncol)) != SGL_OK) break;
        }
        if (hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)T.ncol, s) != hipSuccess) { rc = SGL_EHIP; break; }
        if (nnz > 0) row_hist_kernel<<<dim3(grid_for(nnz)), dim3(256), 0, s>>>(A.i, nnz, (unsigned long long*)counts);
        if ((rc = k_exclusive_scan(c, counts, T.p, T.ncol)) != SGL_OK) break;
        if ((rc = k_scan_total(s, counts, T.p, T.ncol)) != SGL_OK) break;
        if (batched && hipMemcpyAsync(cursor, T.p, sizeof(int64_t) * (size_t)T.ncol, hipMemcpyDeviceToDevice, s) != hipSuccess) { rc = SGL_EHIP; break; }
        int end_bit = 1;
        while (((int64_t)1 << end_bit) < (int64_t)A.nrow && end_bit < 31) ++end_bit;
        for (size_t b = 0; b + 1 < cut.size() && rc == SGL_OK; ++b) {
            const int64_t c0 = cut[b], c1 = cut[b + 1];
            const int64_t q0 = batched ? hp[(size_t)c0] : 0, n = batched ? hp[(size_t)c1] - q0 : nnz;
            if (n == 0) continue;
            const int64_t wb = std::min<int64_t>((c1 - c0 + 3) / 4, 256 * 32);
            expand_cols_kernel<<<dim3((unsigned)wb), dim3(256), 0, s>>>(A.p, c0, c1, q0, colof, iota);
            size_t tmp_bytes = 0;
            if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, A.i + q0, keys_out, iota, perm, n, 0, end_bit, s) != hipSuccess) { rc = SGL_EHIP; break; }
            if (tmp_bytes > tmp_cap) {
                if (tmp) { (void)sgl_pool_free(tmp); tmp = nullptr; }
                if (sgl_pool_malloc(&tmp, tmp_bytes) != hipSuccess) { (void)hipGetLastError(); sgl_set_error("transpose: temp alloc failed"); rc = SGL_ENOMEM; break; }
                tmp_cap = tmp_bytes;
            }
            if (hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, A.i + q0, keys_out, iota, perm, n, 0, end_bit, s) != hipSuccess) { rc = SGL_EHIP; break; }
            if (!batched) {
                gather_kernel<<<dim3(grid_for(n)), dim3(256), 0, s>>>(perm, n, colof, A.x, T.i, T.x);
            } else {
                run_start_kernel<<<dim3(grid_for(n)), dim3(256), 0, s>>>(keys_out, n, rstart);
                gather_batch_kernel<<<dim3(grid_for(n)), dim3(256), 0, s>>>(keys_out, perm, n, rstart, cursor, colof, A.x + q0, T.i, T.x);
                advance_kernel<<<dim3(grid_for(n)), dim3(256), 0, s>>>(keys_out, n, rstart, cursor);
            }
            if (hipGetLastError() != hipSuccess) rc = SGL_EHIP;
        }
        if (rc == SGL_OK && hipGetLastError() != hipSuccess) rc = SGL_EHIP;
    } while (0);
    hipError_t e = hipStreamSynchronize(s);
    if (rc == SGL_EHIP || e != hipSuccess) { sgl_set_error("device transpose failed: %s", hipGetErrorString(e)); rc = SGL_EHIP; }
    if (counts) (void)sgl_pool_free(counts);
    if (cursor) (void)sgl_pool_free(cursor);
    if (rstart) (void)sgl_pool_free(rstart);
    if (colof) (void)sgl_pool_free(colof);
    if (keys_out) (void)sgl_pool_free(keys_out);
    if (iota) (void)sgl_pool_free(iota);
    if (perm) (void)sgl_pool_free(perm);
    if (tmp) (void)sgl_pool_free(tmp);
    return rc;
}

// the resident pair: c->At from c->A
int sgl_device_transpose(sgl_ctx* c, int64_t max_batch_entries) { return sgl_device_transpose_into(c, c->A, c->At, max_batch_entries); }
