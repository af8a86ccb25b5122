// Stand-alone driver of singlet_amd/csrc/umap_transform_host.h (the host logic of the layout transform that makes no HIP
// call: the refusals of the arguments, of the query lists, of the memberships and of the positions, the plan that
// sgl_umap_transform_info reports and the cut of the epochs into launches), meant for a host compiler with
// -fsanitize=address,undefined: tests/test_umap_transform_restatement.py builds and runs it.  Exit status 0 and the line
// "umap_transform_host: ok" mean every check held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/umap_transform_host.h"

#include <stdio.h>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// exactly as many elements on the heap as the lists have: a read past them is the sanitizer's to find
struct Lists {
    std::vector<int32_t> idx;
    std::vector<double> dist;
    int64_t n;
    int32_t K;
};

static UtDefect check(const Lists& l, int64_t n_ref, int64_t* q, int32_t* s) {
    return ut_check_lists(l.idx.data(), l.dist.data(), nullptr, l.n, l.K, n_ref, q, s);
}

static UtDefect scalars(int64_t nq, int32_t K, int64_t n_ref, int32_t dim, double a, double b, int32_t ne, int64_t t0, int64_t t1, double alpha,
                        int32_t neg, int64_t off) {
    return ut_check_scalars(nq, K, n_ref, true, dim, a, b, ne, t0, t1, alpha, neg, off);
}

int main() {
    int64_t q = 0, pos = 0;
    int32_t s = 0;
    // ---- the scalar arguments
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_OK);
    EXPECT(scalars(0, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_OK);
    EXPECT(scalars(-1, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_NQ);
    EXPECT(scalars(3, 0, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_K);
    EXPECT(scalars(3, 257, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_K);
    EXPECT(scalars(3, 1, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_OK);
    EXPECT(scalars(3, 256, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_OK);
    EXPECT(scalars(3, 3, 0, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_NREF);
    EXPECT(scalars(3, 3, (int64_t)1 << 31, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_NREF);
    EXPECT(scalars(3, 3, ((int64_t)1 << 31) - 1, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_OK);
    EXPECT(scalars(3, 3, 10, 0, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_DIM);
    EXPECT(scalars(3, 3, 10, 9, 1.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_DIM);
    EXPECT(scalars(3, 3, 10, 2, 0.0, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_AB);
    EXPECT(scalars(3, 3, 10, 2, 1.0, NAN, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_AB);
    EXPECT(scalars(3, 3, 10, 2, INFINITY, 1.0, 30, 1, 30, 0.25, 5, 0) == UT_ARGS_AB);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 0, 1, 1, 0.25, 5, 0) == UT_ARGS_EPOCHS);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, (1 << 20) + 1, 1, 1, 0.25, 5, 0) == UT_ARGS_EPOCHS);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 0, 30, 0.25, 5, 0) == UT_ARGS_RANGE);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 8, 7, 0.25, 5, 0) == UT_ARGS_RANGE);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 31, 0.25, 5, 0) == UT_ARGS_RANGE);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 7, 7, 0.25, 5, 0) == UT_OK);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.0, 5, 0) == UT_ARGS_ALPHA);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, -1, 0) == UT_ARGS_NEG);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 256, 0) == UT_ARGS_NEG);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 0, 0) == UT_OK);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, -1) == UT_ARGS_OFFSET);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, ((int64_t)1 << 55) - 3) == UT_OK);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, ((int64_t)1 << 55) - 2) == UT_ARGS_OFFSET);
    EXPECT(scalars(3, 3, 10, 2, 1.0, 1.0, 30, 1, 30, 0.25, 5, INT64_MAX) == UT_ARGS_OFFSET);
    EXPECT(ut_check_scalars(3, 3, 10, false, 0, 0, 0, 0, 0, 0, 0, 0, -5) == UT_OK);   // sgl_c_fuzzy_query: the lists' arguments only

    // ---- the lists: 3 queries, 3 slots each; the second ends in one padding slot, the third is empty
    const Lists ok{{4, 1, 7, 2, 9, -1, -1, -1, -1}, {0.0, 1.0, 1.0, 0.5, 0.75, INFINITY, INFINITY, INFINITY, INFINITY}, 3, 3};
    EXPECT(check(ok, 10, &q, &s) == UT_OK && q == -1 && s == -1);
    {
        Lists l = ok;
        l.idx[2] = 10;
        EXPECT(check(l, 10, &q, &s) == UT_INDEX_RANGE && q == 0 && s == 2);
        l.idx[2] = -2;
        EXPECT(check(l, 10, &q, &s) == UT_INDEX_RANGE && q == 0 && s == 2);
        l = ok;
        l.idx[5] = 3;
        l.idx[4] = -1;
        EXPECT(check(l, 10, &q, &s) == UT_VALID_AFTER_PAD && q == 1 && s == 2);
        l = ok;
        l.idx[2] = 4;
        EXPECT(check(l, 10, &q, &s) == UT_INDEX_REPEATED && q == 0 && s == 2);
        l = ok;
        l.dist[1] = INFINITY;
        EXPECT(check(l, 10, &q, &s) == UT_DIST_NOT_FINITE && q == 0 && s == 1);
        l.dist[1] = NAN;
        EXPECT(check(l, 10, &q, &s) == UT_DIST_NOT_FINITE && q == 0 && s == 1);
        l = ok;
        l.dist[3] = -0.5;
        EXPECT(check(l, 10, &q, &s) == UT_DIST_NEGATIVE && q == 1 && s == 0);
        l = ok;
        l.dist[4] = 0.25;
        EXPECT(check(l, 10, &q, &s) == UT_DIST_ORDER && q == 1 && s == 1);
        l = ok;
        l.dist[5] = NAN;   // the distance of a padding slot is not read
        EXPECT(check(l, 10, &q, &s) == UT_OK);
    }
    {   // the stage operator: no distances, the memberships of the valid slots in [0, 1]
        std::vector<double> W{1.0, 0.5, 0.0, 1.0, 0.25, 7.0, -1.0, NAN, 2.0};
        EXPECT(ut_check_lists(ok.idx.data(), nullptr, W.data(), 3, 3, 10, &q, &s) == UT_OK);
        W[1] = 1.0000000000000002;
        EXPECT(ut_check_lists(ok.idx.data(), nullptr, W.data(), 3, 3, 10, &q, &s) == UT_W_RANGE && q == 0 && s == 1);
        W[1] = NAN;
        EXPECT(ut_check_lists(ok.idx.data(), nullptr, W.data(), 3, 3, 10, &q, &s) == UT_W_RANGE && q == 0 && s == 1);
        W[1] = 0.5;
        W[4] = -1e-300;
        EXPECT(ut_check_lists(ok.idx.data(), nullptr, W.data(), 3, 3, 10, &q, &s) == UT_W_RANGE && q == 1 && s == 1);
    }
    {   // the widest list the rules allow, with the repeat at its very end
        Lists l{std::vector<int32_t>(256), std::vector<double>(256, 1.0), 1, 256};
        for (int t = 0; t < 256; ++t) l.idx[(size_t)t] = 255 - t;
        EXPECT(check(l, 256, &q, &s) == UT_OK);
        l.idx[255] = 255;
        EXPECT(check(l, 256, &q, &s) == UT_INDEX_REPEATED && q == 0 && s == 255);
    }
    // ---- the positions
    {
        std::vector<double> Y{0.0, 1.0, -2.0, 3.0, 4.0, 5.0};
        EXPECT(ut_all_finite(Y.data(), 6, &pos) && pos == -1);
        Y[4] = INFINITY;
        EXPECT(!ut_all_finite(Y.data(), 6, &pos) && pos == 4);
        EXPECT(ut_all_finite(Y.data(), 0, &pos));
        // Yin: the column of the empty third query is not read
        std::vector<double> Yin{0.0, 1.0, 2.0, 3.0, NAN, NAN};
        EXPECT(ut_yin_finite(Yin.data(), ok.idx.data(), 3, 3, 2, &q, &s) && q == -1);
        Yin[3] = NAN;
        EXPECT(!ut_yin_finite(Yin.data(), ok.idx.data(), 3, 3, 2, &q, &s) && q == 1 && s == 1);
    }
    // ---- the plan
    {
        const UtPlan P = ut_plan(ok.idx.data(), 3, 3, 2, 1.0, 1, 30);
        EXPECT(P.instance == 1 && P.widest == 3 && P.empty == 1 && P.launches == 1);
        EXPECT(ut_plan(ok.idx.data(), 3, 3, 3, 0.9, 1, 129).instance == 2 && ut_plan(ok.idx.data(), 3, 3, 3, 0.9, 1, 129).launches == 2);
        EXPECT(ut_plan(ok.idx.data(), 3, 3, 5, 1.0, 1, 1).instance == 5 && ut_plan(ok.idx.data(), 0, 3, 8, 0.5, 7, 7).instance == 4);
        EXPECT(ut_plan(ok.idx.data(), 0, 3, 8, 0.5, 7, 7).widest == 0 && ut_plan(ok.idx.data(), 0, 3, 8, 0.5, 7, 7).empty == 0);
    }
    // ---- the launches: every epoch in exactly one, ascending, none longer than the cut; the largest call is 8192 launches
    for (const auto& range : std::vector<std::pair<int64_t, int64_t>>{{1, 1}, {1, 30}, {1, 128}, {1, 129}, {7, 7}, {8, 30}, {100, 400}, {1, 1 << 20}}) {
        int rc = -1;
        int64_t next = range.first, longest = 0;
        const int64_t n = ut_run_launches(range.first, range.second, [&](int64_t first, int64_t last) -> int {
            EXPECT(first == next && last >= first && last <= range.second);
            longest = std::max(longest, last - first + 1);
            next = last + 1;
            return 0;
        }, &rc);
        EXPECT(rc == 0 && next == range.second + 1 && longest <= UMAP_TRANSFORM_EPOCHS_PER_LAUNCH);
        EXPECT(n == ut_launch_count(range.first, range.second));
    }
    EXPECT(ut_launch_count(1, 1 << 20) == 8192);
    {   // the profiling switch: a whole number in [1, 128], anything else is the default
        EXPECT(ut_epochs_per_launch(nullptr) == 128 && ut_epochs_per_launch("") == 128 && ut_epochs_per_launch("1") == 1);
        EXPECT(ut_epochs_per_launch("128") == 128 && ut_epochs_per_launch("17") == 17 && ut_epochs_per_launch("0") == 128);
        EXPECT(ut_epochs_per_launch("129") == 128 && ut_epochs_per_launch("-3") == 128 && ut_epochs_per_launch("7x") == 128);
        EXPECT(ut_epochs_per_launch("99999999999999999999999999") == 128);
        int rc = -1;
        int64_t next = 8;
        const int64_t n = ut_run_launches(8, 30, [&](int64_t first, int64_t last) -> int { EXPECT(first == next && last == first); ++next; return 0; }, &rc, 1);
        EXPECT(n == 23 && next == 31 && n == ut_launch_count(8, 30, 1));
    }
    {   // a failing launch ends the loop with its status
        int rc = 0, calls = 0;
        const int64_t n = ut_run_launches(1, 1000, [&](int64_t, int64_t) -> int { return ++calls == 3 ? -7 : 0; }, &rc);
        EXPECT(rc == -7 && n == 2 && calls == 3);
    }
    if (failures) { printf("umap_transform_host: %d FAILED\n", failures); return 1; }
    printf("umap_transform_host: ok\n");
    return 0;
}
