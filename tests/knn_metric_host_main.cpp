// Stand-alone driver of the metric's argument rule in singlet_amd/csrc/knn_host.h (sgl_knn_metric), meant for a host compiler
// with -fsanitize=address,undefined: tests/test_knn_metric_restatement.py builds and runs it.  Exit status 0 and the line
// "knn_metric_host: ok" mean every check held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/knn_host.h"

#include <stdio.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    // ---- the codes the header and the binding name
    EXPECT(KNN_METRIC_EUCLIDEAN == 0 && KNN_METRIC_COSINE == 1 && KNN_METRIC_CORRELATION == 2 && KNN_METRIC_MAX == 2);
    // ---- the rule: [0, 2], nothing else; the ends of int32_t
    EXPECT(knn_metric_ok(0) && knn_metric_ok(1) && knn_metric_ok(2));
    EXPECT(!knn_metric_ok(-1) && !knn_metric_ok(3) && !knn_metric_ok(7));
    EXPECT(!knn_metric_ok(INT32_MAX) && !knn_metric_ok(INT32_MIN));
    for (int32_t m = -300; m <= 300; ++m) EXPECT(knn_metric_ok(m) == (m >= 0 && m <= KNN_METRIC_MAX));
    // ---- its place: after the argument rules, which do not depend on it.  A call that both rules refuse is refused by the
    // argument rule (the entries test the metric second); a call only the metric refuses has passed knn_check_args.
    int32_t pos = 0, val = 0;
    std::vector<int32_t> twice{7, 3, 9, 3};   // exactly n_dims entries on the heap: a read past them is the sanitizer's to find
    EXPECT(knn_check_args(50, 1000, 10, nullptr, 0, 0, &pos, &val) == KNN_ARGS_NEIGHBORS && !knn_metric_ok(7));
    EXPECT(knn_check_args(50, 1000, 10, twice.data(), (int32_t)twice.size(), 20, &pos, &val) == KNN_ARGS_DIM_REPEAT && pos == 3 && val == 3);
    EXPECT(knn_check_args(50, 1000, 10, nullptr, 0, 20, &pos, &val) == KNN_ARGS_OK && !knn_metric_ok(7) && !knn_metric_ok(-1));
    // ---- the plan does not depend on the metric: the shapes the GPU tests name, per (instance, list home)
    EXPECT(knn_plan(128, 2049, 3, 32).segments == 2 && knn_plan(128, 2049, 3, 32).instance == 0);
    EXPECT(knn_plan(3, 50000, 3, 20).segments == 48);
    EXPECT(knn_plan(65, 257, 9, 20).instance == 1 && knn_plan(130, 130, 16, 33).lists_global == 1);
    EXPECT(knn_plan(65, 300, 17, 20).instance == 2 && knn_plan(127, 127, 32, 127).lists_global == 1);
    EXPECT(knn_plan(1025, 1025, 50, 20).instance == 3 && knn_plan(65, 300, 64, 33).lists_global == 1);
    EXPECT(knn_plan(3, 7, 66, 7).instance == KNN_GENERIC_INSTANCE && knn_plan(63, 257, 130, 256).lists_global == 1);
    if (failures == 0) printf("knn_metric_host: ok\n");
    return failures == 0 ? 0 : 1;
}
