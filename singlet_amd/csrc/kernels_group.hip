// Group sums of a k x n factor matrix (include/singlet_hip.h, sgl_group_means): out[f, g] = sum of F[f, c] over the cells c
// of group g -- the k x G table behind RunLNMF.Seurat's link cut-off (R/RunLNMF.R:136-143) and MetadataSummary
// (R/MetadataSummary.R:18-26), which R forms with k G calls of mean(h[which(...)]).
//
// Rules (the header states them for the caller):
//  * the summation order is a function of (n, group, n_groups) alone: no floating-point atomics, no grid-stride loop whose
//    trip count follows the launch size, nothing that depends on the occupancy;
//  * the mean is ONE true division of the sum by (double)count; a count of 0 gives 0.0 / 0.0 = NaN;
//  * any n_groups, any k up to the library's 1024; F stays where it is (the H of a fit is read in place).
//
// Shape: the group list arrives from the host, where a stable counting sort gives the permutation of the cells by group
// (ascending cell index inside a group) and the n_groups + 1 offsets.  The cell list of every group is cut into chunks of
// SGL_GROUP_CHUNK cells -- a chunk never spans two groups -- and
//   1. group_chunk_kernel: one workgroup per chunk.  FL = min(64, k rounded up to a power of two) lanes run over the
//      factors and S = 256 / FL slots over the cells: slot s adds the columns at positions s, s + S, ... of the chunk, in
//      that order, to a register per factor (a gathered column is 8 k contiguous bytes, read 8 FL bytes at a time); the S
//      slot sums are then added by a binary tree in LDS (slot s += slot s + stride, stride = S / 2 ... 1).  Ranks above 64
//      take the factors in passes of 64.  The chunk's k sums go to part[chunk, :].
//   2. group_finish_kernel: one lane per (factor, group) adds the group's chunk sums in chunk order, starting from +0.0,
//      and divides by the count when asked to.
// Registers and a 2 KiB LDS tree; reads F once, at the rate of a strided gather of 8 k-byte pieces.
#include "sgl_internal.h"

#define GROUP_THREADS 256
static_assert(SGL_GROUP_CHUNK % GROUP_THREADS == 0 && SGL_GROUP_CHUNK >= GROUP_THREADS, "a chunk is whole rounds of the slots");

// fl_shift: log2(FL).  cbeg[ch] .. cbeg[ch + 1]: the chunk's positions in perm (at most SGL_GROUP_CHUNK of them).
__global__ __launch_bounds__(GROUP_THREADS) void group_chunk_kernel(const double* __restrict__ F, int k, const int32_t* __restrict__ perm,
                                                                   const int64_t* __restrict__ cbeg, int fl_shift,
                                                                   double* __restrict__ part) {
    __shared__ double tree[GROUP_THREADS];
    const int FL = 1 << fl_shift;
    const int S = GROUP_THREADS >> fl_shift;
    const int fl = threadIdx.x & (FL - 1);
    const int slot = threadIdx.x >> fl_shift;
    const int64_t ch = blockIdx.x;
    const int64_t p0 = cbeg[ch], p1 = cbeg[ch + 1];
    for (int f0 = 0; f0 < k; f0 += FL) {
        const int f = f0 + fl;
        double acc = 0.0;
        if (f < k) {
            // four columns in flight per lane; the additions stay in position order
            int64_t p = p0 + slot;
            for (; p + 3 * (int64_t)S < p1; p += 4 * (int64_t)S) {
                const double a0 = F[(int64_t)perm[p] * k + f];
                const double a1 = F[(int64_t)perm[p + S] * k + f];
                const double a2 = F[(int64_t)perm[p + 2 * S] * k + f];
                const double a3 = F[(int64_t)perm[p + 3 * S] * k + f];
                acc += a0;
                acc += a1;
                acc += a2;
                acc += a3;
            }
            for (; p < p1; p += S) acc += F[(int64_t)perm[p] * k + f];
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

// gfirst[g] .. gfirst[g + 1]: the chunks of group g; goff: the n_groups + 1 offsets into perm (counts by difference)
__global__ __launch_bounds__(GROUP_THREADS) void group_finish_kernel(const double* __restrict__ part, int k, int32_t n_groups,
                                                                    const int64_t* __restrict__ gfirst, const int64_t* __restrict__ goff,
                                                                    int divide, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)k * n_groups) return;
    const int32_t g = (int32_t)(e / k);
    const int f = (int)(e - (int64_t)g * k);
    const int64_t c0 = gfirst[g], c1 = gfirst[g + 1];
    double s = 0.0;
#pragma unroll 8
    for (int64_t ch = c0; ch < c1; ++ch) s += part[ch * k + f];
    if (divide) s = s / (double)(goff[g + 1] - goff[g]);
    out[e] = s;
}

int sgl_group_ids_check(const char* who, const char* name, const int32_t* group, int64_t n, int32_t n_groups) {
    for (int64_t q = 0; q < n; ++q)
        if (group[q] < 0 || group[q] >= n_groups) {
            sgl_set_error("%s: %s[%lld] = %d is outside [0, n_groups = %d)", who, name, (long long)q, group[q], n_groups);
            return SGL_EINVAL;
        }
    return SGL_OK;
}

int sgl_group_plan(sgl_ctx* c, GroupPlan& P, int64_t n, const int32_t* group, int32_t n_groups) {
    if (n > INT32_MAX) { sgl_set_error("sgl_group_sums: %lld cells: the cell list holds 32-bit indices", (long long)n); return SGL_EINVAL; }
    // stable counting sort of the cells by group (a negative id leaves its cell out), and the chunk boundaries
    std::vector<int64_t>&goff = P.h_goff, &gfirst = P.h_gfirst, &cbeg = P.h_cbeg;
    std::vector<int32_t>&perm = P.h_perm, &cgroup = P.h_cgroup;
    goff.assign((size_t)n_groups + 1, 0);
    gfirst.assign((size_t)n_groups + 1, 0);
    for (int64_t q = 0; q < n; ++q)
        if (group[q] >= 0) ++goff[(size_t)group[q] + 1];
    P.counts.assign((size_t)n_groups, 0);
    for (int32_t g = 0; g < n_groups; ++g) {
        P.counts[g] = goff[(size_t)g + 1];
        gfirst[(size_t)g + 1] = gfirst[g] + (goff[(size_t)g + 1] + SGL_GROUP_CHUNK - 1) / SGL_GROUP_CHUNK;
        goff[(size_t)g + 1] += goff[g];
    }
    const int64_t nchunks = gfirst[n_groups], n_in = goff[n_groups];
    P.nchunks = nchunks;
    P.n_in = n_in;
    perm.assign((size_t)std::max<int64_t>(n_in, 1), 0);
    {
        std::vector<int64_t> at(goff.begin(), goff.end() - 1);
        for (int64_t q = 0; q < n; ++q)
            if (group[q] >= 0) perm[(size_t)at[group[q]]++] = (int32_t)q;
    }
    cbeg.assign((size_t)nchunks + 1, 0);
    cgroup.assign((size_t)std::max<int64_t>(nchunks, 1), 0);
    for (int32_t g = 0; g < n_groups; ++g)
        for (int64_t ch = gfirst[g]; ch < gfirst[(size_t)g + 1]; ++ch) {
            cbeg[(size_t)ch] = goff[g] + (ch - gfirst[g]) * SGL_GROUP_CHUNK;
            cgroup[(size_t)ch] = g;
        }
    cbeg[(size_t)nchunks] = n_in;
    // (chunk ch ends where chunk ch + 1 begins: the next chunk of its group, or the first cell of the next non-empty group)

    SGLCHK(P.perm.alloc(perm.size()));
    SGLCHK(P.cgroup.alloc(cgroup.size()));
    SGLCHK(P.cbeg.alloc(cbeg.size()));
    SGLCHK(P.gfirst.alloc(gfirst.size()));
    SGLCHK(P.goff.alloc(goff.size()));
    // the uploads are asynchronous and read the plan's own host vectors: the caller synchronises before the plan goes
    HIPCHK(hipMemcpyAsync(P.perm.p, perm.data(), sizeof(int32_t) * perm.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.cgroup.p, cgroup.data(), sizeof(int32_t) * cgroup.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.cbeg.p, cbeg.data(), sizeof(int64_t) * cbeg.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.gfirst.p, gfirst.data(), sizeof(int64_t) * gfirst.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.goff.p, goff.data(), sizeof(int64_t) * goff.size(), hipMemcpyHostToDevice, c->stream));
    return SGL_OK;
}

int sgl_group_sums_on(sgl_ctx* c, GroupPlan& P, const double* F, int k, int32_t n_groups, bool divide, double* part, double* out) {
    int fl_shift = 0;
    while ((1 << fl_shift) < k && fl_shift < 6) ++fl_shift;
    Phase ph(c, SGL_PH_SCALE);   // "row sums, scale, cor, copies": where scripts/linked_grouped_rate.py reads the kernels' time
    if (P.nchunks > 0) {
        group_chunk_kernel<<<dim3((unsigned)P.nchunks), dim3(GROUP_THREADS), 0, c->stream>>>(F, k, P.perm.p, P.cbeg.p, fl_shift, part);
        if (hipGetLastError() != hipSuccess) return SGL_EHIP;
    }
    const int64_t total = (int64_t)k * n_groups;
    group_finish_kernel<<<dim3((unsigned)((total + GROUP_THREADS - 1) / GROUP_THREADS)), dim3(GROUP_THREADS), 0, c->stream>>>(
        part, k, n_groups, P.gfirst.p, P.goff.p, divide ? 1 : 0, out);
    if (hipGetLastError() != hipSuccess) return SGL_EHIP;
    return SGL_OK;
}

int sgl_group_sums_dev(sgl_ctx* c, const double* F, int k, int64_t n, const int32_t* group, int32_t n_groups, bool divide,
                       double* out, int64_t* counts) {
    GroupPlan P;   // (outlives the synchronisation below on every path: its uploads and the kernels read it)
    DevBuf<double> dpart, dout;
    int rc = sgl_group_plan(c, P, n, group, n_groups);
    if (rc == SGL_EINVAL) return rc;   // refused before anything was queued
    if (rc == SGL_OK) std::copy(P.counts.begin(), P.counts.end(), counts);
    if (rc == SGL_OK) rc = dpart.alloc((size_t)std::max<int64_t>(P.nchunks, 1) * (size_t)k);
    if (rc == SGL_OK) rc = dout.alloc((size_t)k * (size_t)n_groups);
    if (rc == SGL_OK) rc = sgl_group_sums_on(c, P, F, k, n_groups, divide, dpart.p, dout.p);
    if (rc == SGL_OK && hipMemcpyAsync(out, dout.p, sizeof(double) * (size_t)k * (size_t)n_groups, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = SGL_EHIP;
    // the host vectors and the device buffers above are released on return: nothing may still be in flight then
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_ENOMEM) return rc;
    if (rc != SGL_OK || e != hipSuccess) { sgl_set_error("sgl_group_sums: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return SGL_OK;
}
