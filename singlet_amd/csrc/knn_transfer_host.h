// Host logic of the neighbour index and of the label / value transfer (include/singlet_hip.h, "Neighbour index and transfer")
// that makes no HIP call: the argument rules in their order, the check of a label list, the check of a caller's neighbour
// slots and the batch plan of sgl_knn_index_map.  Plain C++ over plain pointers, so tests/knn_transfer_host_main.cpp compiles
// it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <stdint.h>

#include "knn_host.h"

#define KNN_TRANSFER_MAX_CLASSES 65536
#define KNN_TRANSFER_MAX_VALUES 1024
#define KNN_TRANSFER_WEIGHTING_MAX 1            // 0: every neighbour votes 1.0; 1: Dudani's distance weights
#define KNN_TRANSFER_SCRATCH_BYTES (1ll << 30)  // what one batch of sgl_knn_index_map keeps on the device stays below this

enum KnnTransferArgError {
    KNN_TRANSFER_ARGS_OK = 0,
    KNN_TRANSFER_ARGS_WEIGHTING,   // weighting outside [0, 1]
    KNN_TRANSFER_ARGS_NEIGHBORS,   // n_neighbors outside [1, 256]
    KNN_TRANSFER_ARGS_NQUERY,      // n_query < 0
    KNN_TRANSFER_ARGS_NREF,        // n_ref outside [1, 2^31)
    KNN_TRANSFER_ARGS_CLASSES,     // labels given with n_classes outside [1, 65536]
    KNN_TRANSFER_ARGS_VALUES,      // V given with n_values outside [1, 1024]
};

// The argument refusals of the transfer in this order.  n_classes is read only with labels, n_values only with V.
inline KnnTransferArgError knn_transfer_check_args(int32_t weighting, int32_t n_neighbors, int64_t n_query, int64_t n_ref, bool has_labels,
                                                   int32_t n_classes, bool has_values, int32_t n_values) {
    if (weighting < 0 || weighting > KNN_TRANSFER_WEIGHTING_MAX) return KNN_TRANSFER_ARGS_WEIGHTING;
    if (n_neighbors < 1 || n_neighbors > KNN_MAX_NEIGHBORS) return KNN_TRANSFER_ARGS_NEIGHBORS;
    if (n_query < 0) return KNN_TRANSFER_ARGS_NQUERY;
    if (n_ref < 1 || n_ref > (int64_t)INT32_MAX) return KNN_TRANSFER_ARGS_NREF;
    if (has_labels && (n_classes < 1 || n_classes > KNN_TRANSFER_MAX_CLASSES)) return KNN_TRANSFER_ARGS_CLASSES;
    if (has_values && (n_values < 1 || n_values > KNN_TRANSFER_MAX_VALUES)) return KNN_TRANSFER_ARGS_VALUES;
    return KNN_TRANSFER_ARGS_OK;
}

// The first label outside [-1, n_classes): its position, or -1.
inline int64_t knn_transfer_first_bad_label(const int32_t* labels, int64_t n_ref, int32_t n_classes) {
    for (int64_t r = 0; r < n_ref; ++r)
        if (labels[r] < -1 || labels[r] >= n_classes) return r;
    return -1;
}

enum KnnTransferSlotError {
    KNN_TRANSFER_SLOTS_OK = 0,
    KNN_TRANSFER_SLOTS_RANGE,      // an entry outside [-1, n_ref)
    KNN_TRANSFER_SLOTS_ORDER,      // a valid slot behind a padding slot
};

// idx is n_neighbors x n_query column-major.  The first defective entry in column-major order: *query, *slot and *value name it.
inline KnnTransferSlotError knn_transfer_check_slots(const int32_t* idx, int32_t n_neighbors, int64_t n_query, int64_t n_ref, int64_t* query,
                                                     int32_t* slot, int32_t* value) {
    for (int64_t j = 0; j < n_query; ++j) {
        bool padded = false;
        for (int32_t t = 0; t < n_neighbors; ++t) {
            const int32_t v = idx[j * n_neighbors + t];
            *query = j;
            *slot = t;
            *value = v;
            if (v < -1 || (int64_t)v >= n_ref) return KNN_TRANSFER_SLOTS_RANGE;
            if (v >= 0 && padded) return KNN_TRANSFER_SLOTS_ORDER;
            if (v < 0) padded = true;
        }
    }
    *query = -1;
    *slot = -1;
    *value = 0;
    return KNN_TRANSFER_SLOTS_OK;
}

// Bytes one query of a map batch keeps on the device: the candidates of its search (search_slots x n_neighbors x 12: the probe
// slots of the inverted lists, the reference segments of the exact scan), its neighbour list (n_neighbors x 12), pred and best
// (12), and its scores and values where they are asked for.
inline int64_t knn_transfer_query_bytes(int32_t search_slots, int32_t n_neighbors, int32_t n_classes_out, int32_t n_values_out) {
    return ((int64_t)search_slots + 1) * n_neighbors * 12 + 12 + 8 * ((int64_t)n_classes_out + n_values_out);
}

// Queries per batch of sgl_knn_index_map: as many as keep query_bytes each below `budget`, at least one, at most n_query (>= 1).
inline int64_t knn_transfer_batch(int64_t n_query, int64_t query_bytes, int64_t budget) {
    int64_t b = budget / (query_bytes > 0 ? query_bytes : 1);
    if (b < 1) b = 1;
    return b < n_query ? b : n_query;
}
