// Stand-alone driver of singlet_amd/csrc/knn_host.h (the host logic of sgl_knn that makes no HIP call: the argument rules,
// the check of dims, the launch plan), meant for a host compiler with -fsanitize=address,undefined:
// tests/test_embedding_knn_restatement.py builds and runs it.  Exit status 0 and the line "knn_host: ok" mean every check
// held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/knn_host.h"

#include <stdio.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static KnnArgError args(int32_t k, int64_t n_ref, int64_t nq, const std::vector<int32_t>* dims, int32_t K, int32_t* pos, int32_t* val) {
    // exactly n_dims entries on the heap: a read past them is the sanitizer's to find
    return knn_check_args(k, n_ref, nq, dims ? dims->data() : nullptr, dims ? (int32_t)dims->size() : 0, K, pos, val);
}

int main() {
    int32_t pos = 0, val = 0;
    const int64_t two31 = 2147483648LL;
    // ---- arguments
    EXPECT(args(50, 1000, 1000, nullptr, 20, &pos, &val) == KNN_ARGS_OK && pos == -1);
    EXPECT(args(50, 1000, 0, nullptr, 20, &pos, &val) == KNN_ARGS_OK);
    EXPECT(args(50, 1000, 10, nullptr, 0, &pos, &val) == KNN_ARGS_NEIGHBORS);
    EXPECT(args(50, 1000, 10, nullptr, 257, &pos, &val) == KNN_ARGS_NEIGHBORS);
    EXPECT(args(50, 1000, 10, nullptr, 256, &pos, &val) == KNN_ARGS_OK);
    EXPECT(args(50, 19, 10, nullptr, 20, &pos, &val) == KNN_ARGS_NEIGHBORS);
    EXPECT(args(50, 20, 10, nullptr, 20, &pos, &val) == KNN_ARGS_OK);
    EXPECT(args(0, 1000, 10, nullptr, 20, &pos, &val) == KNN_ARGS_RANK);
    EXPECT(args(1025, 1000, 10, nullptr, 20, &pos, &val) == KNN_ARGS_RANK);
    EXPECT(args(1024, 1000, 10, nullptr, 20, &pos, &val) == KNN_ARGS_OK);
    EXPECT(args(50, 0, 10, nullptr, 1, &pos, &val) == KNN_ARGS_NREF);
    EXPECT(args(50, two31, 10, nullptr, 1, &pos, &val) == KNN_ARGS_NREF);
    EXPECT(args(50, two31 - 1, 10, nullptr, 1, &pos, &val) == KNN_ARGS_OK);
    EXPECT(args(50, 1000, -1, nullptr, 20, &pos, &val) == KNN_ARGS_NQUERY);
    // ---- dims
    std::vector<int32_t> good{4, 0, 49}, low{3, -1, 2}, high{3, 50}, twice{7, 3, 9, 3, 7}, all(1024);
    for (int q = 0; q < 1024; ++q) all[(size_t)q] = 1023 - q;
    EXPECT(knn_check_args(50, 1000, 10, good.data(), 0, 20, &pos, &val) == KNN_ARGS_NDIMS);
    EXPECT(args(2, 1000, 10, &good, 20, &pos, &val) == KNN_ARGS_NDIMS);
    EXPECT(args(50, 1000, 10, &good, 20, &pos, &val) == KNN_ARGS_OK && pos == -1);
    EXPECT(args(50, 1000, 10, &low, 20, &pos, &val) == KNN_ARGS_DIM_RANGE && pos == 1 && val == -1);
    EXPECT(args(50, 1000, 10, &high, 20, &pos, &val) == KNN_ARGS_DIM_RANGE && pos == 1 && val == 50);
    EXPECT(args(50, 1000, 10, &twice, 20, &pos, &val) == KNN_ARGS_DIM_REPEAT && pos == 3 && val == 3);
    EXPECT(args(1024, 1000, 10, &all, 20, &pos, &val) == KNN_ARGS_OK);
    all[1023] = 1023;
    EXPECT(args(1024, 1000, 10, &all, 20, &pos, &val) == KNN_ARGS_DIM_REPEAT && pos == 1023 && val == 1023);
    // ---- instances
    const int edge[] = {1, 8, 9, 16, 17, 32, 33, 64, 65, 1024};
    const int inst[] = {0, 0, 1, 1, 2, 2, 3, 3, 4, 4};
    for (int q = 0; q < 10; ++q) EXPECT(knn_instance(edge[q]) == inst[q]);
    // ---- plans: every segment non-empty, the segments cover the references, LDS within 48 KiB
    const int64_t nqs[] = {1, 3, 64, 65, 128, 129, 2700, 131071, 131072, 131073, 1000000};
    const int64_t nrs[] = {1, 20, 1023, 1024, 2048, 4095, 4096, 50000, 1000000, two31 - 1};
    const int nds[] = {1, 3, 8, 9, 16, 17, 32, 33, 50, 64, 65, 130, 1024};
    const int Ks[] = {1, 2, 20, 32, 33, 256};
    for (int64_t nq : nqs)
        for (int64_t nr : nrs)
            for (int nd : nds)
                for (int K : Ks) {
                    if (K > nr) continue;
                    const KnnPlan P = knn_plan(nq, nr, nd, K);
                    EXPECT(P.instance == knn_instance(nd));
                    EXPECT(P.queries_per_wg == 64 * P.queries_per_lane && (P.queries_per_lane == 1 || P.queries_per_lane == 2));
                    EXPECT(P.query_blocks * P.queries_per_wg >= nq && (P.query_blocks - 1) * P.queries_per_wg < nq);
                    EXPECT(P.segments >= 1 && P.segments <= KNN_MAX_SEGMENTS);
                    EXPECT(P.segment_refs * P.segments >= nr && P.segment_refs * (P.segments - 1) < nr);
                    EXPECT(P.segments == 1 || (P.query_blocks < KNN_TARGET_WAVES && P.segment_refs >= KNN_MIN_SEGMENT_REFS && P.segment_refs >= 4 * K));
                    EXPECT(P.lists_global == (K > KNN_LDS_MAX_NEIGHBORS ? 1 : 0));
                    EXPECT(P.lds_bytes <= 48 * 1024 && (P.lists_global ? P.lds_bytes == 0 : P.lds_bytes == (int64_t)P.queries_per_wg * K * 12));
                }
    // the cases the GPU tests name
    EXPECT(knn_plan(3, 50000, 3, 20).segments == 48);
    EXPECT(knn_plan(130945, 50000, 3, 20).segments == 1);   // 1024 workgroups of 128 queries
    EXPECT(knn_plan(130944, 50000, 3, 20).segments == 2);
    EXPECT(knn_plan(1000000, 1000000, 50, 20).segments == 1);
    if (failures == 0) printf("knn_host: ok\n");
    return failures == 0 ? 0 : 1;
}
