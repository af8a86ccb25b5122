// Stand-alone driver of singlet_amd/csrc/knn_ivf_host.h (the host logic of the inverted-list neighbour search), meant for a
// host compiler with -fsanitize=address,undefined: tests/test_knn_ivf_restatement.py builds and runs it.  Every array has
// exactly the stated number of entries on the heap, so a read or write past them is the sanitizer's to find.  Exit status 0
// and the line "knn_ivf_host: ok" mean every check held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/knn_ivf_host.h"

#include <stdio.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the task table of `probes` (n_query x n_probe) at pairs_per_block, checked against its contract
static void check_tasks(const std::vector<int32_t>& probes, int64_t nq, int32_t np, int32_t n_lists, int ppb) {
    std::vector<int64_t> first((size_t)n_lists + 1), cursor((size_t)n_lists);
    const int64_t blocks = knn_ivf_task_count(probes.data(), nq, np, n_lists, ppb, first.data());
    const int64_t n_pairs = nq * np;
    EXPECT(first[0] == 0 && first[(size_t)n_lists] == n_pairs);
    std::vector<int32_t> pq((size_t)n_pairs), ps((size_t)n_pairs), bl((size_t)blocks);
    std::vector<int64_t> bb((size_t)blocks + 1);
    knn_ivf_task_fill(probes.data(), nq, np, n_lists, ppb, first.data(), cursor.data(), pq.data(), ps.data(), bl.data(), bb.data());
    // every pair once, at a place of its own list, in (query, slot) order inside a list
    std::vector<int> seen((size_t)n_pairs, 0);
    for (int32_t g = 0; g < n_lists; ++g)
        for (int64_t at = first[(size_t)g]; at < first[(size_t)g + 1]; ++at) {
            const int64_t e = (int64_t)pq[(size_t)at] * np + ps[(size_t)at];
            EXPECT(pq[(size_t)at] >= 0 && pq[(size_t)at] < nq && ps[(size_t)at] >= 0 && ps[(size_t)at] < np);
            EXPECT(probes[(size_t)e] == g);
            ++seen[(size_t)e];
            if (at > first[(size_t)g]) {
                const int64_t before = (int64_t)pq[(size_t)at - 1] * np + ps[(size_t)at - 1];
                EXPECT(before < e);   // stable
            }
        }
    for (int64_t e = 0; e < n_pairs; ++e) EXPECT(seen[(size_t)e] == 1);
    // the blocks tile the pair array, none is empty or longer than ppb, none crosses a list edge
    EXPECT(bb[0] == 0 && bb[(size_t)blocks] == n_pairs);
    for (int64_t b = 0; b < blocks; ++b) {
        const int32_t g = bl[(size_t)b];
        EXPECT(g >= 0 && g < n_lists);
        EXPECT(bb[(size_t)b] < bb[(size_t)b + 1] && bb[(size_t)b + 1] - bb[(size_t)b] <= ppb);
        EXPECT(bb[(size_t)b] >= first[(size_t)g] && bb[(size_t)b + 1] <= first[(size_t)g + 1]);
        if (b > 0) EXPECT(bl[(size_t)b - 1] <= g);
    }
}

int main() {
    // ---- the refusals, in their order: n_lists, n_probe, n_iter, metric
    EXPECT(knn_ivf_check_args(1000, 32, 8, 10, 0) == KNN_IVF_ARGS_OK);
    EXPECT(knn_ivf_check_args(1000, 0, 8, 10, 0) == KNN_IVF_ARGS_LISTS && knn_ivf_check_args(1000, -1, 8, 10, 0) == KNN_IVF_ARGS_LISTS);
    EXPECT(knn_ivf_check_args(1000, 1001, 8, 10, 0) == KNN_IVF_ARGS_LISTS && knn_ivf_check_args(1000, 1000, 8, 10, 0) == KNN_IVF_ARGS_OK);
    EXPECT(knn_ivf_check_args(1 << 20, 65536, 8, 10, 0) == KNN_IVF_ARGS_OK && knn_ivf_check_args(1 << 20, 65537, 8, 10, 0) == KNN_IVF_ARGS_LISTS);
    EXPECT(knn_ivf_check_args(1000, 32, 0, 10, 0) == KNN_IVF_ARGS_PROBES && knn_ivf_check_args(1000, 32, 33, 10, 0) == KNN_IVF_ARGS_PROBES);
    EXPECT(knn_ivf_check_args(1000, 32, 32, 10, 0) == KNN_IVF_ARGS_OK);
    EXPECT(knn_ivf_check_args(1000, 100, 64, 10, 0) == KNN_IVF_ARGS_OK && knn_ivf_check_args(1000, 100, 65, 10, 0) == KNN_IVF_ARGS_PROBES);
    EXPECT(knn_ivf_check_args(1000, 32, 8, -1, 0) == KNN_IVF_ARGS_ITER && knn_ivf_check_args(1000, 32, 8, 1001, 0) == KNN_IVF_ARGS_ITER);
    EXPECT(knn_ivf_check_args(1000, 32, 8, 0, 0) == KNN_IVF_ARGS_OK && knn_ivf_check_args(1000, 32, 8, 1000, 2) == KNN_IVF_ARGS_OK);
    EXPECT(knn_ivf_check_args(1000, 32, 8, 10, 3) == KNN_IVF_ARGS_METRIC && knn_ivf_check_args(1000, 32, 8, 10, -1) == KNN_IVF_ARGS_METRIC);
    EXPECT(knn_ivf_check_args(1000, 0, 0, -1, 7) == KNN_IVF_ARGS_LISTS);     // the first in the order wins
    EXPECT(knn_ivf_check_args(1000, 32, 0, -1, 7) == KNN_IVF_ARGS_PROBES);
    EXPECT(knn_ivf_check_args(1000, 32, 8, -1, 7) == KNN_IVF_ARGS_ITER);
    EXPECT(knn_ivf_check_args(1, 1, 1, 0, 0) == KNN_IVF_ARGS_OK && knn_ivf_check_args(1, 2, 1, 0, 0) == KNN_IVF_ARGS_LISTS);
    EXPECT(knn_ivf_check_args(INT32_MAX, INT32_MAX, 1, 0, 0) == KNN_IVF_ARGS_LISTS && knn_ivf_check_args(1000, INT32_MIN, 1, 0, 0) == KNN_IVF_ARGS_LISTS);
    EXPECT(KNN_IVF_MAX_PROBES == KNN_MAX_SEGMENTS && KNN_IVF_DEFAULT_PROBES >= 1 && KNN_IVF_DEFAULT_PROBES <= KNN_IVF_MAX_PROBES);
    EXPECT((KNN_IVF_DEFAULT_PROBES & (KNN_IVF_DEFAULT_PROBES - 1)) == 0);

    // ---- training picks at 64 n_lists - 1, 64 n_lists, 64 n_lists + 1, and at the ends of the ranges
    for (int32_t L : {1, 3, 45}) {
        for (int64_t n_ref : {(int64_t)64 * L - 1, (int64_t)64 * L, (int64_t)64 * L + 1, (int64_t)1000003}) {
            if (n_ref < L) continue;
            const int64_t T = knn_ivf_train_count(n_ref, L);
            EXPECT(T == (n_ref < 64 * L ? n_ref : 64 * L));
            int64_t last = -1;
            for (int64_t t = 0; t < T; ++t) {
                const int64_t r = knn_ivf_pick(t, n_ref, T);
                EXPECT(r > last && r < n_ref);   // strictly ascending: no cell trains twice
                if (T == n_ref) EXPECT(r == t);   // every cell trains
                last = r;
            }
            EXPECT(knn_ivf_pick(0, n_ref, T) == 0);
            last = -1;
            for (int32_t g = 0; g < L; ++g) {
                const int64_t t = knn_ivf_pick(g, T, L);
                EXPECT(t > last && t < T);
                last = t;
            }
        }
    }
    EXPECT(knn_ivf_train_count(INT32_MAX, 65536) == (int64_t)64 * 65536);
    EXPECT(knn_ivf_pick((int64_t)64 * 65536 - 1, INT32_MAX, (int64_t)64 * 65536) == ((int64_t)64 * 65536 - 1) * (int64_t)INT32_MAX / ((int64_t)64 * 65536));
    EXPECT(knn_ivf_pick((int64_t)64 * 65536 - 1, INT32_MAX, (int64_t)64 * 65536) < INT32_MAX);

    // ---- a caller's assignment: the first offender
    {
        std::vector<int32_t> a{0, 2, 1, 3, -1, 7};
        EXPECT(knn_ivf_first_bad_assign(a.data(), 6, 4) == 4);
        EXPECT(knn_ivf_first_bad_assign(a.data(), 4, 4) == -1);
        EXPECT(knn_ivf_first_bad_assign(a.data(), 4, 3) == 3);
        EXPECT(knn_ivf_first_bad_assign(a.data(), 0, 1) == -1);
    }

    // ---- list offsets with empty lists (first, middle, last), members in ascending cell index
    {
        std::vector<int32_t> a{3, 1, 3, 3, 1, 5, 3};
        const int32_t L = 7;
        std::vector<int64_t> off((size_t)L + 1);
        std::vector<int32_t> cell(a.size());
        knn_ivf_bucket(a.data(), (int64_t)a.size(), L, off.data(), cell.data());
        const int64_t want_off[8] = {0, 0, 2, 2, 6, 6, 7, 7};
        const int32_t want_cell[7] = {1, 4, 0, 2, 3, 6, 5};
        for (int g = 0; g <= L; ++g) EXPECT(off[(size_t)g] == want_off[g]);
        for (int p = 0; p < 7; ++p) EXPECT(cell[(size_t)p] == want_cell[p]);
        int64_t lo = -1, hi = -1, empty = -1;
        knn_ivf_list_stats(off.data(), L, &lo, &hi, &empty);
        EXPECT(lo == 0 && hi == 4 && empty == 4);
        // one list, and one member per list
        std::vector<int32_t> zeros(5, 0), iota{0, 1, 2, 3, 4};
        std::vector<int64_t> off1(2), off5(6);
        std::vector<int32_t> cell5(5);
        knn_ivf_bucket(zeros.data(), 5, 1, off1.data(), cell5.data());
        EXPECT(off1[0] == 0 && off1[1] == 5 && cell5[0] == 0 && cell5[4] == 4);
        knn_ivf_bucket(iota.data(), 5, 5, off5.data(), cell5.data());
        for (int g = 0; g <= 5; ++g) EXPECT(off5[(size_t)g] == g);
        knn_ivf_list_stats(off5.data(), 5, &lo, &hi, &empty);
        EXPECT(lo == 1 && hi == 1 && empty == 0);
    }

    // ---- the task table: blocks never cross a list edge, every pair once
    EXPECT(knn_ivf_pairs_per_block(1) == 128 && knn_ivf_pairs_per_block(32) == 128 && knn_ivf_pairs_per_block(33) == 64 &&
           knn_ivf_pairs_per_block(64) == 64 && knn_ivf_pairs_per_block(65) == 64 && knn_ivf_pairs_per_block(1024) == 64);
    for (int ppb : {64, 128}) {
        for (int64_t nq : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)129, (int64_t)300}) {
            // every query probes list 2 first (a list with 1, 63, 64, 65, ... pairs: whole blocks and a rest), then a list of its own
            const int32_t np = 3, L = 11;
            std::vector<int32_t> probes((size_t)(nq * np));
            for (int64_t j = 0; j < nq; ++j) {
                probes[(size_t)(j * np)] = 2;
                probes[(size_t)(j * np + 1)] = (int32_t)((j * 7 + 3) % L == 2 ? 5 : (j * 7 + 3) % L);
                probes[(size_t)(j * np + 2)] = (int32_t)(j % 2 ? 10 : 0);   // lists 1, 9 and others may stay unprobed
            }
            check_tasks(probes, nq, np, L, ppb);
        }
        // one probe, one list; and every list probed by every query
        check_tasks(std::vector<int32_t>(200, 0), 200, 1, 1, ppb);
        std::vector<int32_t> all;
        for (int j = 0; j < 70; ++j)
            for (int p = 0; p < 4; ++p) all.push_back((p + j) % 4);
        check_tasks(all, 70, 4, 4, ppb);
    }

    // ---- the batch plan at its edges
    const int64_t budget = KNN_IVF_SCRATCH_BYTES;
    EXPECT(knn_ivf_batch(1000, 16, 20, 0, budget) == 1000);                       // everything fits
    EXPECT(knn_ivf_batch(1000000, 16, 20, 0, budget) == budget / (16 * 20 * 12));  // 279620 queries
    EXPECT(knn_ivf_batch(1000000, 16, 20, 0, budget) * 16 * 20 * 12 <= budget);
    EXPECT(knn_ivf_batch(1000000, 64, 256, 0, budget) == budget / (64 * 256 * 12));
    EXPECT(knn_ivf_batch(5, 64, 256, 0, 1) == 1);                                  // never below one query
    EXPECT(knn_ivf_batch(1000, 16, 20, 1, budget) == 1 && knn_ivf_batch(1000, 16, 20, 7, budget) == 7);
    EXPECT(knn_ivf_batch(1000, 16, 20, 1000, budget) == 1000 && knn_ivf_batch(1000, 16, 20, 5000, budget) == 1000);
    EXPECT(knn_ivf_batch(1, 1, 1, 0, budget) == 1);
    EXPECT(knn_ivf_batch(INT32_MAX, 64, 256, 0, budget) * (int64_t)64 * 256 * 12 <= budget);

    if (failures == 0) printf("knn_ivf_host: ok\n");
    return failures == 0 ? 0 : 1;
}
