// nnls_half_kernel<KH> instances for 64 < k <= 128 (two lanes per column, see nnls_half.h)
#include "nnls_half.h"

template <int KH>
static int launch_half(dim3 g, dim3 b, hipStream_t s, const double* Gpad, double* B, double* X, const int64_t* col_nnz, int k,
                       int64_t ncols, double L1, double L2, unsigned long long* sweep_counter, const NnlsPass& ps) {
    constexpr size_t lds = nnls_half_lds_bytes<KH>();
    SGLCHK(sgl_allow_dynamic_lds<&nnls_half_kernel<KH>>((int)lds));
    nnls_half_kernel<KH><<<g, b, lds, s>>>(Gpad, B, X, col_nnz, k, ncols, L1, L2, sweep_counter, ps);
    HIPCHK(hipGetLastError());   // up to 131 KB of dynamic LDS: a refused launch must not leave X stale unnoticed
    return SGL_OK;
}

// KP = 72 ... 128 in steps of 8.  Workgroups of 256 threads (128 columns); where the staged Gram leaves room for only one
// workgroup per CU (KP = 104: 94 KB of LDS) and there are columns enough, 512 threads, so that a SIMD still has two waves.
int k_nnls_half_launch(hipStream_t s, const double* Gpad, int KP, double* B, double* X, const int64_t* col_nnz, int k,
                       int64_t ncols, double L1, double L2, unsigned long long* sweep_counter, const NnlsPass& ps) {
    const bool big = KP > 96 && KP <= 104 && ncols >= 256 * 256;   // (above 104: x in AGPRs, one wave per SIMD, 256 threads)
    const int cpb = big ? 256 : 128;
    const dim3 g((unsigned)((ncols + cpb - 1) / cpb)), b(2 * cpb);
    if (KP % 8 != 0 || KP < 72 || KP > 128) { sgl_set_error("k_nnls_half: unsupported KP=%d", KP); return SGL_EINVAL; }
    return sgl_rank_dispatch<9, 16>(KP / 8, [&](auto kp8) {
        return launch_half<4 * decltype(kp8)::value>(g, b, s, Gpad, B, X, col_nnz, k, ncols, L1, L2, sweep_counter, ps);
    });
}
