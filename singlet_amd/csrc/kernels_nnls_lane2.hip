// nnls_lane_kernel<KP> instances for KP = 42 .. 64 (see nnls_lane.h)
#include "nnls_lane.h"

int k_nnls_lane_launch2(hipStream_t s, const double* Gpad, int KP, double* B, double* X, const int64_t* col_nnz, int k,
                        int64_t ncols, double L1, double L2, unsigned long long* sweep_counter, const NnlsPass& ps, dim3 g,
                        dim3 b) {
    return nnls_lane_launch<42, 64, true>(s, Gpad, KP, B, X, col_nnz, k, ncols, L1, L2, sweep_counter, ps, g, b);
}
