// Stand-alone driver of singlet_amd/csrc/umap_host.h (the host logic of the layout stage that makes no HIP call: the refusals
// of the k-NN lists and of the graph, the maximum weight, the learning rate, the firing rule, the instance choice, the chunk
// plan, the merge split, the column pointers and the epoch loop), meant for a host compiler with
// -fsanitize=address,undefined: tests/test_umap_restatement.py builds and runs it.  Exit status 0 and the line
// "umap_host: ok" mean every check held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/umap_host.h"

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

static FuzzyDefect check(const Lists& l, int64_t* cell, int32_t* slot) { return fuzzy_check(l.idx.data(), l.dist.data(), l.n, l.K, cell, slot); }

struct G {
    std::vector<int32_t> p, i;
    std::vector<double> x;
    int64_t n() const { return (int64_t)p.size() - 1; }
};

static UmapDefect gcheck(const G& g, const std::vector<double>& Y, int32_t dim, double a, double b, int32_t epochs, double alpha0,
                         int32_t neg, int64_t t, bool op, int64_t* pos, int64_t* col) {
    return umap_check(g.x.data(), g.i.data(), g.p.data(), g.n(), Y.data(), dim, a, b, epochs, alpha0, neg, t, op, pos, col);
}

int main() {
    int64_t cell = 0, pos = 0, col = 0;
    int32_t slot = 0;
    // ---- the k-NN lists: 3 cells, 2 candidates each
    const Lists ok{{0, 1, 1, 2, 2, 0}, {0.0, 1.0, 0.0, 0.5, 0.0, 2.0}, 3, 2};
    EXPECT(check(ok, &cell, &slot) == FUZZY_OK && cell == -1 && slot == -1);
    EXPECT(fuzzy_check(nullptr, ok.dist.data(), 3, 2, &cell, &slot) == FUZZY_ARGS_NULL);
    EXPECT(fuzzy_check(ok.idx.data(), nullptr, 3, 2, &cell, &slot) == FUZZY_ARGS_NULL);
    EXPECT(fuzzy_check(ok.idx.data(), ok.dist.data(), 3, 1, &cell, &slot) == FUZZY_ARGS_K);
    EXPECT(fuzzy_check(ok.idx.data(), ok.dist.data(), 3, 257, &cell, &slot) == FUZZY_ARGS_K);
    EXPECT(fuzzy_check(ok.idx.data(), ok.dist.data(), 0, 2, &cell, &slot) == FUZZY_ARGS_N);
    EXPECT(fuzzy_check(ok.idx.data(), ok.dist.data(), (int64_t)1 << 31, 2, &cell, &slot) == FUZZY_ARGS_N);
    {
        Lists l = ok;
        l.idx[3] = 3;
        EXPECT(check(l, &cell, &slot) == FUZZY_INDEX_RANGE && cell == 1 && slot == 1);
        l.idx[3] = -1;
        EXPECT(check(l, &cell, &slot) == FUZZY_INDEX_RANGE && cell == 1 && slot == 1);
        l = ok;
        l.idx[5] = 2;
        EXPECT(check(l, &cell, &slot) == FUZZY_INDEX_REPEATED && cell == 2 && slot == 1);
        l = ok;
        l.dist[1] = INFINITY;
        EXPECT(check(l, &cell, &slot) == FUZZY_DIST_NOT_FINITE && cell == 0 && slot == 1);
        l.dist[1] = NAN;
        EXPECT(check(l, &cell, &slot) == FUZZY_DIST_NOT_FINITE && cell == 0 && slot == 1);
        l = ok;
        l.dist[2] = -1e-300;
        EXPECT(check(l, &cell, &slot) == FUZZY_DIST_NEGATIVE && cell == 1 && slot == 0);
        l = ok;
        l.dist[4] = 3.0;
        EXPECT(check(l, &cell, &slot) == FUZZY_DIST_ORDER && cell == 2 && slot == 1);
        // one cell cannot fill two places without a repeat
        const Lists one{{0, 0}, {0.0, 0.0}, 1, 2};
        EXPECT(check(one, &cell, &slot) == FUZZY_INDEX_REPEATED && cell == 0 && slot == 1);
    }
    // ---- the merge split and the column pointers
    {
        const std::vector<int64_t> indeg{0, UMAP_MERGE_WIDTH - 15, UMAP_MERGE_WIDTH - 14, 5000};
        std::vector<int32_t> fast, slow;
        std::vector<int64_t> soff;
        fuzzy_split(indeg.data(), 4, 15, fast, slow, soff);
        EXPECT(fast == (std::vector<int32_t>{0, 1}) && slow == (std::vector<int32_t>{2, 3}));
        EXPECT(soff == (std::vector<int64_t>{0, UMAP_MERGE_WIDTH + 1, UMAP_MERGE_WIDTH + 1 + 5015}));
        const std::vector<int32_t> cnt{2, 0, 3};
        std::vector<int32_t> p(4, -7);
        int64_t nnz = -1;
        EXPECT(fuzzy_pointers(cnt.data(), 3, p.data(), &nnz) && nnz == 5 && p == (std::vector<int32_t>{0, 2, 2, 5}));
        const std::vector<int32_t> big{INT32_MAX, 1};
        std::vector<int32_t> q(3, -7);
        EXPECT(!fuzzy_pointers(big.data(), 2, q.data(), &nnz) && nnz == (int64_t)INT32_MAX + 1 && q == (std::vector<int32_t>{-7, -7, -7}));
    }
    // ---- the graph of the layout: a path 0 - 1 - 2 with a diagonal entry on 1, column 3 empty
    const G g{{0, 1, 4, 5, 5}, {1, 0, 1, 2, 1}, {2.0, 2.0, 0.5, 3.0, 3.0}};
    const std::vector<double> Y(8, 0.25);
    EXPECT(gcheck(g, Y, 2, 1.5, 0.9, 200, 1.0, 5, 0, false, &pos, &col) == UMAP_OK && pos == -1 && col == -1);
    EXPECT(gcheck(g, Y, 2, 1.5, 0.9, 200, 1.0, 0, 200, true, &pos, &col) == UMAP_OK);
    EXPECT(umap_check(g.x.data(), g.i.data(), nullptr, 4, Y.data(), 2, 1.0, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_NULL);
    EXPECT(umap_check(g.x.data(), g.i.data(), g.p.data(), 4, nullptr, 2, 1.0, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_NULL);
    EXPECT(umap_check(nullptr, g.i.data(), g.p.data(), 4, Y.data(), 2, 1.0, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_NULL);
    EXPECT(umap_check(g.x.data(), g.i.data(), g.p.data(), 0, Y.data(), 2, 1.0, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_N);
    EXPECT(gcheck(g, Y, 0, 1.0, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_DIM);
    EXPECT(gcheck(g, Y, 9, 1.0, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_DIM);
    EXPECT(gcheck(g, Y, 2, 0.0, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_AB);
    EXPECT(gcheck(g, Y, 2, 1.0, NAN, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_AB);
    EXPECT(gcheck(g, Y, 2, INFINITY, 1.0, 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_AB);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, 0, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_EPOCHS);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, UMAP_MAX_EPOCHS + 1, 1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_EPOCHS);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, UMAP_MAX_EPOCHS, 1.0, 0, 0, false, &pos, &col) == UMAP_OK);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, 10, 1.0, 0, 0, true, &pos, &col) == UMAP_ARGS_EPOCH);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, 10, 1.0, 0, 11, true, &pos, &col) == UMAP_ARGS_EPOCH);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, 10, -1.0, 0, 0, false, &pos, &col) == UMAP_ARGS_ALPHA);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, 10, 1.0, -1, 0, false, &pos, &col) == UMAP_ARGS_NEG);
    EXPECT(gcheck(g, Y, 2, 1.0, 1.0, 10, 1.0, 256, 0, false, &pos, &col) == UMAP_ARGS_NEG);
    {
        G b = g;
        b.p[0] = 1;
        EXPECT(gcheck(b, Y, 2, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_ARGS_P0);
        b = g;
        b.p[2] = 0;
        EXPECT(gcheck(b, Y, 2, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_ARGS_P_DECREASES && pos == 1);
        std::vector<double> Yb = Y;
        Yb[5] = NAN;
        EXPECT(gcheck(g, Yb, 2, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_Y_NOT_FINITE && pos == 5);
        EXPECT(gcheck(g, Yb, 1, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_OK);   // dim 1 reads 4 positions only
        b = g;
        b.i[4] = 4;
        EXPECT(gcheck(b, Y, 2, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_ROW_RANGE && pos == 4 && col == 2);
        b = g;
        b.i[2] = 0;
        EXPECT(gcheck(b, Y, 2, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_ROW_ORDER && pos == 2 && col == 1);
        b = g;
        b.x[3] = INFINITY;
        EXPECT(gcheck(b, Y, 2, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_WEIGHT_NOT_FINITE && pos == 3 && col == 1);
        b = g;
        b.x[0] = -0.5;
        EXPECT(gcheck(b, Y, 2, 1.0, 1.0, 10, 1.0, 5, 0, false, &pos, &col) == UMAP_WEIGHT_NEGATIVE && pos == 0 && col == 0);
    }
    // ---- maximum weight, learning rate, firing
    EXPECT(umap_w_max(g.x.data(), 5) == 3.0 && umap_w_max(g.x.data(), 0) == 0.0);
    EXPECT(umap_alpha(1.0, 1, 200) == 1.0 && umap_alpha(1.0, 200, 200) == 1.0 * (1.0 - 199.0 / 200.0) && umap_alpha(0.5, 3, 4) == 0.25);
    {
        // weights 1, 1/2, 1/4, 3/4 of the maximum over 5 epochs: every epoch; 2 and 4; 4; 2, 3 and 4
        const double w[4] = {3.0, 1.5, 0.75, 2.25};
        const int want[4][5] = {{1, 1, 1, 1, 1}, {0, 1, 0, 1, 0}, {0, 0, 0, 1, 0}, {0, 1, 1, 1, 0}};
        for (int e = 0; e < 4; ++e)
            for (int t = 1; t <= 5; ++t) EXPECT(umap_fires(w[e], 3.0, t) == (want[e][t - 1] != 0));
        int fired = 0;
        for (int t = 1; t <= 200; ++t) fired += umap_fires(3.0 / 400.0, 3.0, t) ? 1 : 0;   // below w_max / n_epochs: never
        EXPECT(fired == 0);
        EXPECT(!umap_fires(0.0, 3.0, 1));
    }
    // ---- instance and chunk plan
    EXPECT(umap_instance(2, 0.9) == 0 && umap_instance(2, 1.0) == 1 && umap_instance(3, 0.9) == 2 && umap_instance(3, 1.0) == 3);
    EXPECT(umap_instance(1, 0.9) == 4 && umap_instance(5, 0.9) == 4 && umap_instance(8, 1.0) == 5);
    {
        const UmapPlan P = umap_plan(g.p.data(), 4, 3, 1.0, 30);
        EXPECT(P.widest == 3 && P.multi_chunk == 0 && P.instance == 3 && P.epochs == 30);
        const std::vector<int32_t> wide{0, 64, 129, 129, 194};
        const UmapPlan Q = umap_plan(wide.data(), 4, 5, 0.5, 1);
        EXPECT(Q.widest == 65 && Q.multi_chunk == 2 && Q.instance == 4);
    }
    // ---- the epoch loop: buffers swap, alpha follows the epoch, a failure ends it
    {
        std::vector<double> alphas;
        std::vector<int> froms;
        int rc = -1;
        int last = umap_run_epochs(4, 1.0, [&](int64_t t, double alpha, int from, int to) {
            EXPECT(to == 1 - from && (int64_t)alphas.size() == t - 1);
            alphas.push_back(alpha);
            froms.push_back(from);
            return 0;
        }, &rc);
        EXPECT(rc == 0 && last == 0 && froms == (std::vector<int>{0, 1, 0, 1}));
        EXPECT(alphas == (std::vector<double>{1.0, 0.75, 0.5, 0.25}));
        last = umap_run_epochs(3, 1.0, [&](int64_t, double, int, int) { return 0; }, &rc);
        EXPECT(rc == 0 && last == 1);
        int calls = 0;
        last = umap_run_epochs(5, 1.0, [&](int64_t t, double, int, int) { ++calls; return t == 2 ? -3 : 0; }, &rc);
        EXPECT(rc == -3 && calls == 2 && last == 1);
    }
    if (failures) return 1;
    printf("umap_host: ok\n");
    return 0;
}
