// The device stage of the layout transform (kernels_umap_transform.hip) as sgl_knn_index_project (kernels_knn_ivf.hip) runs
// it on every batch of a search: memberships, start and all epochs on device arrays.  Include after sgl_internal.h.
#pragma once
#include <stdint.h>

// idx / dist: K x nq on the device, as the searches write them (not validated again); Yref dim x n_ref; W a scratch of
// K x nq; Y0 (may be null) and Y dim x nq.  stats (may be null; unsigned long long[2], zeroed by the caller): [0] becomes
// the widest list, [1] counts the queries without a valid slot.  *launches = the launches of the transform kernel.
int sgl_umap_transform_dev(hipStream_t s, const int32_t* idx, const double* dist, int32_t K, int64_t nq, const double* Yref, int32_t dim,
                           int64_t n_ref, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed,
                           int64_t query_offset, double* W, double* Y0, double* Y, unsigned long long* stats, int64_t* launches);
// The refusals of the layout arguments (the lists of sgl_knn_index_project come from its own search).
int sgl_umap_transform_args(const char* who, int64_t n_query, int32_t K, int64_t n_ref, int32_t dim, double a, double b, int32_t n_epochs,
                            double alpha0, int32_t neg_rate);
// What sgl_umap_transform_info reports of a call that ran through sgl_umap_transform_dev.
void sgl_umap_transform_note(int32_t dim, double b, int64_t widest, int64_t empty, int64_t launches);
