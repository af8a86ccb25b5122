// Host logic of sgl_upload_typed (include/singlet_hip.h) that makes no HIP call: the argument rules, the layout mapping,
// the offset checks of a HOST-space call and the batch edges of the long sort path.  Plain C++ over plain pointers, so
// tests/ingest_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <stdint.h>

// the codes of include/singlet_hip.h, restated so that this header stands alone
enum { INGEST_F64 = 0, INGEST_F32 = 1, INGEST_I32 = 2, INGEST_I64 = 3 };

enum IngestArgError {
    INGEST_ARGS_OK = 0,
    INGEST_ARGS_NULL,        // a missing array
    INGEST_ARGS_X_TYPE,      // x_type is none of F64 / F32 / I32 / I64
    INGEST_ARGS_IDX_TYPE,    // idx_type is neither I32 nor I64
    INGEST_ARGS_PTR_TYPE,    // ptr_type is neither I32 nor I64
    INGEST_ARGS_EXTENT,      // n_major or n_minor outside [1, INT32_MAX]
    INGEST_ARGS_MAJOR,       // major_is_genes is neither 0 nor 1
    INGEST_ARGS_SPACE,       // space is neither HOST nor DEVICE
    INGEST_ARGS_FLAGS,       // a flag bit this version does not know
};

inline int ingest_type_bytes(int t) { return t == INGEST_F32 || t == INGEST_I32 ? 4 : 8; }

inline IngestArgError ingest_check_args(const void* x, int x_type, const void* idx, int idx_type, const void* ptr, int ptr_type,
                                        int64_t n_major, int64_t n_minor, int major_is_genes, int space, uint32_t flags,
                                        uint32_t known_flags) {
    if (!x || !idx || !ptr) return INGEST_ARGS_NULL;
    if (x_type < INGEST_F64 || x_type > INGEST_I64) return INGEST_ARGS_X_TYPE;
    if (idx_type != INGEST_I32 && idx_type != INGEST_I64) return INGEST_ARGS_IDX_TYPE;
    if (ptr_type != INGEST_I32 && ptr_type != INGEST_I64) return INGEST_ARGS_PTR_TYPE;
    if (n_major < 1 || n_major > INT32_MAX || n_minor < 1 || n_minor > INT32_MAX) return INGEST_ARGS_EXTENT;
    if (major_is_genes != 0 && major_is_genes != 1) return INGEST_ARGS_MAJOR;
    if (space != 0 && space != 1) return INGEST_ARGS_SPACE;
    if (flags & ~known_flags) return INGEST_ARGS_FLAGS;
    return INGEST_ARGS_OK;
}

// The arrays are the CSC of `filled` (0: A, genes x cells; 1: t(A), cells x genes): its columns are the major slices.
struct IngestLayout {
    int filled;              // which resident orientation the arrays fill; the other one is its device transpose
    int32_t genes, cells;    // nrow / ncol of A
};
inline IngestLayout ingest_layout(int major_is_genes, int64_t n_major, int64_t n_minor) {
    IngestLayout L;
    L.filled = major_is_genes ? 1 : 0;
    L.genes = (int32_t)(major_is_genes ? n_major : n_minor);
    L.cells = (int32_t)(major_is_genes ? n_minor : n_major);
    return L;
}

// ptr[0] == 0 and ptr non-decreasing over its n_major + 1 values: -1 when both hold (the entry count is then
// ptr[n_major] >= 0), else the first position q whose ptr[q] breaks the rule (0: ptr[0] != 0).
template <typename P>
inline int64_t ingest_check_offsets(const P* ptr, int64_t n_major, int64_t* entries) {
    *entries = 0;
    if (ptr[0] != 0) return 0;
    for (int64_t q = 0; q < n_major; ++q)
        if (ptr[q + 1] < ptr[q]) return q + 1;
    *entries = (int64_t)ptr[n_major];
    return -1;
}

// Batch edges of the long sort path: the n long slices (len[s] entries each, in list order) are cut into runs
// [cut[b], cut[b + 1]) of whole slices whose entries sum to at most max_entries, greedily; a slice longer than
// max_entries is a run of its own (it cannot occur: a slice holds at most n_minor <= INT32_MAX entries and the caller
// passes max_entries = INT32_MAX).  cut has room for n + 1 values; returns the number of runs (cut[runs] = n).
inline int64_t ingest_batch_edges(const int64_t* len, int64_t n, int64_t max_entries, int64_t* cut) {
    int64_t runs = 0;
    cut[0] = 0;
    for (int64_t s = 0; s < n;) {
        int64_t sum = len[s], e = s + 1;
        while (e < n && len[e] <= max_entries - sum) sum += len[e++];
        cut[++runs] = e;
        s = e;
    }
    return runs;
}
