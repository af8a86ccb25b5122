// Stand-alone driver of singlet_amd/csrc/knn_transfer_host.h (the host logic of the neighbour index and of the label / value
// transfer), meant for a host compiler with -fsanitize=address,undefined: tests/test_knn_transfer_restatement.py builds and
// runs it.  Every array has exactly the stated number of entries on the heap, so a read or write past them is the sanitizer's
// to find.  Exit status 0 and the line "knn_transfer_host: ok" mean every check held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/knn_transfer_host.h"

#include <stdio.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static KnnTransferSlotError slots(const std::vector<int32_t>& idx, int32_t K, int64_t n_ref, int64_t* query, int32_t* slot, int32_t* value) {
    return knn_transfer_check_slots(idx.data(), K, (int64_t)idx.size() / K, n_ref, query, slot, value);
}

int main() {
    // the argument order: weighting, n_neighbors, n_query, n_ref, n_classes (with labels only), n_values (with V only)
    EXPECT(knn_transfer_check_args(0, 1, 0, 1, false, 0, false, 0) == KNN_TRANSFER_ARGS_OK);
    EXPECT(knn_transfer_check_args(1, 256, 5, INT32_MAX, true, 65536, true, 1024) == KNN_TRANSFER_ARGS_OK);
    EXPECT(knn_transfer_check_args(2, 0, -1, 0, true, 0, true, 0) == KNN_TRANSFER_ARGS_WEIGHTING);
    EXPECT(knn_transfer_check_args(-1, 20, 1, 10, false, 0, false, 0) == KNN_TRANSFER_ARGS_WEIGHTING);
    EXPECT(knn_transfer_check_args(1, 0, -1, 0, true, 0, true, 0) == KNN_TRANSFER_ARGS_NEIGHBORS);
    EXPECT(knn_transfer_check_args(1, 257, 1, 10, false, 0, false, 0) == KNN_TRANSFER_ARGS_NEIGHBORS);
    EXPECT(knn_transfer_check_args(1, 20, -1, 0, true, 0, true, 0) == KNN_TRANSFER_ARGS_NQUERY);
    EXPECT(knn_transfer_check_args(1, 20, 1, 0, true, 0, true, 0) == KNN_TRANSFER_ARGS_NREF);
    EXPECT(knn_transfer_check_args(1, 20, 1, (int64_t)INT32_MAX + 1, false, 0, false, 0) == KNN_TRANSFER_ARGS_NREF);
    EXPECT(knn_transfer_check_args(1, 20, 1, 10, true, 0, true, 0) == KNN_TRANSFER_ARGS_CLASSES);
    EXPECT(knn_transfer_check_args(1, 20, 1, 10, true, 65537, true, 1) == KNN_TRANSFER_ARGS_CLASSES);
    EXPECT(knn_transfer_check_args(1, 20, 1, 10, false, 0, true, 0) == KNN_TRANSFER_ARGS_VALUES);
    EXPECT(knn_transfer_check_args(1, 20, 1, 10, true, 3, true, 1025) == KNN_TRANSFER_ARGS_VALUES);
    EXPECT(knn_transfer_check_args(1, 20, 1, 10, false, -7, false, 9999) == KNN_TRANSFER_ARGS_OK);   // neither is read

    // labels: every entry in [-1, n_classes)
    {
        std::vector<int32_t> lab = {0, 2, -1, 1, 2};
        EXPECT(knn_transfer_first_bad_label(lab.data(), 5, 3) == -1);
        EXPECT(knn_transfer_first_bad_label(lab.data(), 5, 2) == 1);
        lab[3] = -2;
        EXPECT(knn_transfer_first_bad_label(lab.data(), 5, 3) == 3);
        EXPECT(knn_transfer_first_bad_label(lab.data(), 3, 3) == -1);
        EXPECT(knn_transfer_first_bad_label(lab.data(), 0, 1) == -1);
    }

    // slots: entries in [-1, n_ref), the padding last; the first offender in column-major order is named
    {
        int64_t q = 0;
        int32_t t = 0, v = 0;
        EXPECT(slots({0, 4, 2, 3, -1, -1, -1, -1, -1}, 3, 5, &q, &t, &v) == KNN_TRANSFER_SLOTS_OK && q == -1 && t == -1);
        EXPECT(slots({0, 4, 2, 3, 5, -1}, 3, 5, &q, &t, &v) == KNN_TRANSFER_SLOTS_RANGE && q == 1 && t == 1 && v == 5);
        EXPECT(slots({0, -2, 2}, 3, 5, &q, &t, &v) == KNN_TRANSFER_SLOTS_RANGE && q == 0 && t == 1 && v == -2);
        EXPECT(slots({0, 1, 2, -1, 3, -1}, 3, 5, &q, &t, &v) == KNN_TRANSFER_SLOTS_ORDER && q == 1 && t == 1 && v == 3);
        EXPECT(slots({1, -1, -1, 0}, 2, 2, &q, &t, &v) == KNN_TRANSFER_SLOTS_ORDER && q == 1 && t == 1 && v == 0);
        EXPECT(slots({-1, 7}, 2, 2, &q, &t, &v) == KNN_TRANSFER_SLOTS_RANGE && v == 7);   // the range comes first
        std::vector<int32_t> none;
        EXPECT(knn_transfer_check_slots(none.data(), 4, 0, 9, &q, &t, &v) == KNN_TRANSFER_SLOTS_OK);
        std::vector<int32_t> wide((size_t)256 * 3, 0);
        wide[(size_t)256 * 3 - 1] = -1;
        EXPECT(knn_transfer_check_slots(wide.data(), 256, 3, 1, &q, &t, &v) == KNN_TRANSFER_SLOTS_OK);
    }

    // the batch plan: at least one query, at most all of them, the budget kept whenever one query fits it
    {
        EXPECT(knn_transfer_query_bytes(3, 20, 0, 0) == 4 * 20 * 12 + 12);
        EXPECT(knn_transfer_query_bytes(64, 256, 65536, 1024) == 65ll * 256 * 12 + 12 + 8 * (65536ll + 1024));
        EXPECT(knn_transfer_batch(1000, 972, KNN_TRANSFER_SCRATCH_BYTES) == 1000);
        EXPECT(knn_transfer_batch(10, 972, 5000) == 5);
        EXPECT(knn_transfer_batch(10, 972, 100) == 1);
        EXPECT(knn_transfer_batch(1, 1, 0) == 1);
        EXPECT(knn_transfer_batch(7, 0, 100) == 7);
        const int64_t per = knn_transfer_query_bytes(64, 256, 65536, 1024);
        const int64_t b = knn_transfer_batch((int64_t)INT32_MAX, per, KNN_TRANSFER_SCRATCH_BYTES);
        EXPECT(b >= 1 && b * per <= KNN_TRANSFER_SCRATCH_BYTES && (b + 1) * per > KNN_TRANSFER_SCRATCH_BYTES);
    }

    if (failures) { printf("knn_transfer_host: %d checks FAILED\n", failures); return 1; }
    printf("knn_transfer_host: ok\n");
    return 0;
}
