// The host logic of the spatial autocorrelation calls (singlet_amd/csrc/moran_host.h) as a program of its own, for the address
// and undefined-behaviour sanitizers: the graph moments on graphs with empty columns, at n = 4, with a column that is all
// diagonal and with one-sided and two-sided pairs for the merge behind S1, held against a dense computation; the refusals of
// the gene list; the path split; the assembly on hand-made moments, a constant row included.  No HIP call, no device.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../singlet_amd/csrc/moran_host.h"

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("moran_host: FAILED %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct Graph {
    int64_t n;
    std::vector<double> x;
    std::vector<int32_t> i, p;
};
// the CSC image of the non-zeros of a dense n x n W (row-major W[i * n + j] = w_ij)
static Graph csc_of(const std::vector<double>& W, int64_t n) {
    Graph g;
    g.n = n;
    g.p.push_back(0);
    for (int64_t j = 0; j < n; ++j) {
        for (int64_t i = 0; i < n; ++i)
            if (W[(size_t)(i * n + j)] != 0.0) { g.i.push_back((int32_t)i); g.x.push_back(W[(size_t)(i * n + j)]); }
        g.p.push_back((int32_t)g.i.size());
    }
    if (g.i.empty()) { g.i.push_back(0); g.x.push_back(0.0); }   // (an address for an empty graph)
    return g;
}

// small integer weights: every sum below is exact, so the dense computation in any order must match to the bit
static int check_graph(const std::vector<double>& W, int64_t n, int expect_refused) {
    const Graph g = csc_of(W, n);
    double S0 = -1, S1 = -1, S2 = -1;
    std::vector<double> t((size_t)n, -1.0);
    const int rc = moran_graph_moments(g.x.data(), g.i.data(), g.p.data(), n, &S0, &S1, &S2, t.data());
    double d0 = 0, d1 = 0, d2 = 0;
    for (int64_t i = 0; i < n; ++i) {
        double ti = 0;
        for (int64_t j = 0; j < n; ++j) {
            const double a = W[(size_t)(i * n + j)], b = W[(size_t)(j * n + i)];
            d0 += a;
            d1 += (a + b) * (a + b);
            ti += a + b;
        }
        REQUIRE(t[(size_t)i] == ti);
        d2 += ti * ti;
    }
    REQUIRE(S0 == d0 && S1 == 0.5 * d1 && S2 == d2);
    REQUIRE(rc == expect_refused);
    // t may be NULL
    REQUIRE(moran_graph_moments(g.x.data(), g.i.data(), g.p.data(), n, &S0, &S1, &S2, nullptr) == expect_refused);
    return 0;
}

int main() {
    // n = 4, an empty first and last column, a one-sided pair (0 -> 1), a two-sided pair (1 <-> 2) with unequal weights, a
    // column that is all diagonal (3), a negative weight
    {
        const int64_t n = 4;
        std::vector<double> W((size_t)(n * n), 0.0);
        W[0 * n + 1] = 2.0;                  // w_01 only
        W[1 * n + 2] = 3.0;
        W[2 * n + 1] = -1.0;                 // two-sided, asymmetric
        W[2 * n + 2] = 5.0;                  // a diagonal next to off-diagonals
        REQUIRE(check_graph(W, n, 0) == 0);
        W[3 * n + 3] = 4.0;                  // column 3 is all diagonal
        REQUIRE(check_graph(W, n, 0) == 0);
    }
    // every column empty: S0 == 0 is refused, and nothing is read out of range
    {
        std::vector<double> W(25, 0.0);
        REQUIRE(check_graph(W, 5, 1) == 0);
        W[1 * 5 + 3] = 1.0;
        W[3 * 5 + 1] = -1.0;                 // weights that cancel: S0 == 0
        REQUIRE(check_graph(W, 5, 1) == 0);
    }
    // a denser pseudo-random graph with empty columns in between
    {
        const int64_t n = 37;
        std::vector<double> W((size_t)(n * n), 0.0);
        uint64_t s = 12345;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < n; ++j) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                if (j % 5 != 0 && (s >> 33) % 4 == 0) W[(size_t)(i * n + j)] = (double)((s >> 40) % 7) - 2.0;
            }
        REQUIRE(check_graph(W, n, 0) == 0);
    }
    // an overflowing weight sum is not finite: refused
    {
        const double x[2] = {1.7e308, 1.7e308};
        const int32_t i[2] = {0, 1}, p[5] = {0, 2, 2, 2, 2};
        double S0, S1, S2;
        REQUIRE(moran_graph_moments(x, i, p, 4, &S0, &S1, &S2, nullptr) == 1);
    }
    // the gene list
    {
        int64_t at, val;
        const int32_t ok[4] = {3, 0, 2, 1}, rep[3] = {1, 2, 1}, out[2] = {0, 4}, neg[1] = {-1};
        REQUIRE(moran_check_genes(nullptr, 0, 4, 0, 0, 0, &at, &val) == MORAN_ARGS_OK);
        REQUIRE(moran_check_genes(ok, 4, 4, 2, 64, 1, &at, &val) == MORAN_ARGS_OK);
        REQUIRE(moran_check_genes(ok, 0, 4, 0, 0, 0, &at, &val) == MORAN_ARGS_OK);
        REQUIRE(moran_check_genes(rep, 3, 4, 0, 0, 0, &at, &val) == MORAN_ARGS_REPEAT && at == 2 && val == 1);
        REQUIRE(moran_check_genes(out, 2, 4, 0, 0, 0, &at, &val) == MORAN_ARGS_RANGE && at == 1 && val == 4);
        REQUIRE(moran_check_genes(neg, 1, 4, 0, 0, 0, &at, &val) == MORAN_ARGS_RANGE && at == 0 && val == -1);
        REQUIRE(moran_check_genes(ok, 1, 0, 0, 0, 0, &at, &val) == MORAN_ARGS_RANGE);
        REQUIRE(moran_check_genes(ok, -1, 4, 0, 0, 0, &at, &val) == MORAN_ARGS_NGENES);
        REQUIRE(moran_check_genes(ok, 4, 4, 3, 0, 0, &at, &val) == MORAN_ARGS_PATH && val == 3);
        REQUIRE(moran_check_genes(ok, 4, 4, 0, -1, 0, &at, &val) == MORAN_ARGS_CAP);
        REQUIRE(moran_check_genes(ok, 4, 4, 0, 0, -5, &at, &val) == MORAN_ARGS_CAP && val == -5);
    }
    // the path split
    REQUIRE(moran_lds_cap(0) == MORAN_LDS_CAP && moran_lds_cap(64) == 64 && moran_lds_cap(MORAN_LDS_CAP + 1) == MORAN_LDS_CAP);
    REQUIRE(moran_gene_path(64, 0, 64) == 1 && moran_gene_path(65, 0, 64) == 2 && moran_gene_path(0, 0, 64) == 1);
    REQUIRE(moran_gene_path(65, 1, 64) == 1 && moran_gene_path(MORAN_LDS_CAP + 1, 1, 0) == 2 && moran_gene_path(1, 2, 0) == 2);
    // the assembly: x = (1, 0, 0, 1) on the path graph 0 - 1 - 2 - 3 (symmetric unit weights), a constant row, NULL outputs
    {
        // S0 = 6, S1 = 12, t = (2, 4, 4, 2), S2 = 40; m = 0.5, d = (+, -, -, +) 0.5: C = 2 * 0.25 * (-1 + 1 - 1) = -0.5
        const double mo[12] = {0.5, 1.0, 0.25, 4.0, 0.0, 2.0,     // mean, M2, M4, T = 1 * 2 + 1 * 2, P = 0 (no stored neighbours), c
                               2.0, 0.0, 0.0, 24.0, 24.0, 4.0};   // constant 2: M2 = 0
        double I[2], EI[2], sd[2], z[2], p[2], padj[2];
        for (int variance = 0; variance < 2; ++variance)
            for (int alt = 0; alt < 3; ++alt) {
                moran_stats(4, 6.0, 12.0, 40.0, 2, mo, variance, alt, I, EI, sd, z, p, padj);
                REQUIRE(I[0] == (4.0 / 6.0) * (-0.5 / 1.0));
                REQUIRE(EI[0] == -1.0 / 3.0 && EI[1] == EI[0]);
                REQUIRE(I[1] != I[1] && z[1] != z[1] && p[1] != p[1] && padj[1] != padj[1]);
                REQUIRE(p[0] >= 0.0 && p[0] <= 1.0 && padj[0] == p[0]);
                if (variance == 1) REQUIRE(sd[0] == sd[1] && sd[0] > 0.0);
            }
        moran_stats(4, 6.0, 12.0, 40.0, 2, mo, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        moran_stats(4, 6.0, 12.0, 40.0, 0, nullptr, 0, 0, I, EI, sd, z, p, padj);
    }
    printf("moran_host: ok\n");
    return 0;
}
