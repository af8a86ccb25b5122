// The host logic of the ligand-receptor calls (singlet_amd/csrc/ligrec_host.h) as a program of its own, for the address and
// undefined-behaviour sanitizers: the plan at both sides of every K at which the vectors per wave change, the waves per
// workgroup, the batch, the knobs' refusals, every refusal of the whole call in its stated order with the offender it names, the
// cut into segments at its edges, and the statistics with an empty class, the NaN mask and both Benjamini-Hochberg scopes on
// hand-made tallies.  No HIP call, no device.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../singlet_amd/csrc/ligrec_host.h"

#define REQUIRE(cond)                                                       \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("ligrec_host: FAILED %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int check_plan() {
    const struct { int K, vpw, waves; } want[] = {{1, 64, 8}, {2, 64, 8}, {16, 64, 8}, {17, 64, 7}, {20, 64, 6}, {32, 64, 4}, {33, 64, 3}, {64, 64, 2},
                                                  {65, 32, 3}, {128, 32, 2}, {129, 16, 3}, {255, 16, 2}, {256, 16, 2}};
    for (const auto& w : want) {
        LigrecPlan P;
        int64_t at, val;
        REQUIRE(ligrec_plan(9000, w.K, 10, 12, 200, 0, 0, 0, &P, &at, &val) == LIGREC_ARGS_OK);
        REQUIRE(P.path == 1 && P.vpw == w.vpw && P.waves == w.waves);
        REQUIRE(P.lds_bytes == (int64_t)w.vpw * w.K * 8 * w.waves && P.lds_bytes <= LIGREC_WG_LDS_BYTES);
        REQUIRE((int64_t)w.vpw * w.K * 8 <= LIGREC_WAVE_LDS_BYTES && ligrec_vpw_max(w.K) == w.vpw);
        if (w.vpw < LIGREC_MAX_VPW) REQUIRE((int64_t)2 * w.vpw * w.K * 8 > LIGREC_WAVE_LDS_BYTES);   // the step is forced
        REQUIRE(ligrec_plan(9000, w.K, 10, 12, 200, 0, 2, 0, &P, &at, &val) == LIGREC_ARGS_OK && P.path == 2 && P.vpw == w.vpw && P.lds_bytes == 0);
        REQUIRE(ligrec_plan(9000, w.K, 10, 12, 200, 0, 1, 0, &P, &at, &val) == LIGREC_ARGS_OK && P.path == 1);
        for (int v = -1; v <= 128; ++v) {
            const bool ok = v >= 0 && v <= w.vpw && (v & (v - 1)) == 0;
            for (int path = 0; path <= 2; ++path) {
                const LigrecArgError e = ligrec_plan(9000, w.K, 10, 12, 200, 0, path, v, &P, &at, &val);
                REQUIRE(e == (ok ? LIGREC_ARGS_OK : LIGREC_ARGS_VPW));
                if (ok) REQUIRE(P.vpw == (v ? v : w.vpw) && P.waves >= 1 && P.waves <= LIGREC_MAX_WAVES);
                else REQUIRE(val == v && at == w.vpw);
            }
        }
    }
    LigrecPlan P;
    int64_t at, val;
    REQUIRE(ligrec_plan(9000, 20, 10, 12, 200, 0, 3, 0, &P, &at, &val) == LIGREC_ARGS_PATH && val == 3);
    REQUIRE(ligrec_plan(9000, 20, 10, 12, 200, 0, -1, 0, &P, &at, &val) == LIGREC_ARGS_PATH && val == -1);
    REQUIRE(ligrec_plan(9000, 20, 10, 12, 200, -1, 0, 0, &P, &at, &val) == LIGREC_ARGS_BATCH && val == -1);
    // batch: forced as given (capped by the vectors), else by the budget in multiples of 64, at least 64
    REQUIRE(ligrec_plan(1000, 3, 10, 12, 200, 7, 0, 0, &P, &at, &val) == LIGREC_ARGS_OK && P.batch == 7);
    REQUIRE(ligrec_plan(1000, 3, 10, 12, 200, 500, 0, 0, &P, &at, &val) == LIGREC_ARGS_OK && P.batch == 200);
    REQUIRE(ligrec_plan(1000, 3, 10, 12, 200, 0, 0, 0, &P, &at, &val) == LIGREC_ARGS_OK && P.batch == 200);
    REQUIRE(ligrec_plan(1000000, 20, 1000, 7000, 1000, 0, 0, 0, &P, &at, &val) == LIGREC_ARGS_OK);
    REQUIRE(P.batch == LIGREC_BATCH_BYTES / (1000000 + 9000 * 20 * 8) / 64 * 64 && P.batch == 64);
    REQUIRE(ligrec_plan(2000000000, 256, 1000, 7000, 1000, 0, 0, 0, &P, &at, &val) == LIGREC_ARGS_OK && P.batch == 64);
    REQUIRE(ligrec_plan(100000, 20, 100, 100, 100000, 0, 0, 0, &P, &at, &val) == LIGREC_ARGS_OK && P.batch == 1792);   // 268435456 / 148000 = 1813, down to a multiple of 64
    return 0;
}

static int check_refusals() {
    const int64_t n = 6, K = 3, m = 5, G = 3, P = 2;
    const int32_t lab[6] = {0, 1, 2, 0, 1, 2}, genes[3] = {4, 0, 2}, lig[2] = {0, 2}, rec[2] = {1, 2};
    int64_t at, val;
#define CALL(lab_, n_, K_, genes_, G_, lig_, rec_, P_, nperm_, thr_, batch_, ncol_) \
    ligrec_check_call(lab_, n_, K_, genes_, G_, m, lig_, rec_, P_, nperm_, thr_, batch_, ncol_, &at, &val)
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_OK);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, 1, 0.0, 0, n) == LIGREC_ARGS_OK && CALL(lab, n, K, genes, G, lig, rec, P, 1 << 20, 1.0, 5, n) == LIGREC_ARGS_OK);
    // one defect at a time
    REQUIRE(CALL(nullptr, n, K, genes, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_NULL && CALL(lab, n, K, nullptr, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_NULL);
    REQUIRE(CALL(lab, n, K, genes, G, nullptr, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_NULL && CALL(lab, n, K, genes, G, lig, nullptr, P, 10, 0.01, 0, n) == LIGREC_ARGS_NULL);
    REQUIRE(CALL(lab, n, 0, genes, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_K && val == 0);
    REQUIRE(CALL(lab, n, 257, genes, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_K && val == 257);
    REQUIRE(CALL(lab, n, K, genes, 0, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_G && val == 0);
    REQUIRE(CALL(lab, n, K, genes, m + 1, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_G && val == m + 1);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, 0, 10, 0.01, 0, n) == LIGREC_ARGS_P && val == 0);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, 0, 0.01, 0, n) == LIGREC_ARGS_NPERM && val == 0);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, (1 << 20) + 1, 0.01, 0, n) == LIGREC_ARGS_NPERM && val == (1 << 20) + 1);
    int32_t bad_lab[6] = {0, 1, 2, 0, 3, -1};
    REQUIRE(CALL(bad_lab, n, K, genes, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_LABEL && at == 4 && val == 3);
    bad_lab[4] = 1;
    REQUIRE(CALL(bad_lab, n, K, genes, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_LABEL && at == 5 && val == -1);
    const int32_t out_gene[3] = {4, 5, 2}, neg_gene[3] = {-1, 0, 2}, twice[3] = {4, 0, 4};
    REQUIRE(CALL(lab, n, K, out_gene, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_GENE && at == 1 && val == 5);
    REQUIRE(CALL(lab, n, K, neg_gene, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_GENE && at == 0 && val == -1);
    REQUIRE(CALL(lab, n, K, twice, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_GENE_TWICE && at == 2 && val == 4);
    const int32_t bad_lig[2] = {0, 3}, bad_rec[2] = {-1, 2};
    REQUIRE(CALL(lab, n, K, genes, G, bad_lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_LIG && at == 1 && val == 3);
    REQUIRE(CALL(lab, n, K, genes, G, lig, bad_rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_REC && at == 0 && val == -1);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, 10, -0.01, 0, n) == LIGREC_ARGS_THRESHOLD && CALL(lab, n, K, genes, G, lig, rec, P, 10, 1.5, 0, n) == LIGREC_ARGS_THRESHOLD);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, 10, NAN, 0, n) == LIGREC_ARGS_THRESHOLD);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, 10, 0.01, -2, n) == LIGREC_ARGS_BATCH && val == -2);
    REQUIRE(CALL(lab, n, K, genes, G, lig, rec, P, 10, 0.01, 0, n + 1) == LIGREC_ARGS_N && val == n);
    REQUIRE(CALL(lab, n - 1, K, genes, G, lig, rec, P, 10, 0.01, 0, n) == LIGREC_ARGS_N && val == n - 1);
    // the stated order: every defect at once, then one fewer from the front each time
    const LigrecArgError order[] = {LIGREC_ARGS_K, LIGREC_ARGS_G, LIGREC_ARGS_P, LIGREC_ARGS_NPERM, LIGREC_ARGS_LABEL, LIGREC_ARGS_GENE, LIGREC_ARGS_LIG,
                                    LIGREC_ARGS_THRESHOLD, LIGREC_ARGS_BATCH, LIGREC_ARGS_N};
    bad_lab[5] = 7;
    for (int fixed = 0; fixed < 10; ++fixed) {
        const LigrecArgError e = CALL(fixed > 4 ? lab : bad_lab, n, fixed > 0 ? K : 0, fixed > 5 ? genes : out_gene, fixed > 1 ? G : 0, fixed > 6 ? lig : bad_lig,
                                      rec, fixed > 2 ? P : 0, fixed > 3 ? 10 : 0, fixed > 7 ? 0.5 : 2.0, fixed > 8 ? 0 : -1, n + 1);
        REQUIRE(e == order[fixed]);
    }
#undef CALL
    return 0;
}

static int check_segments() {
    // genes of 0, 1, 8192, 8193 and 16385 entries
    const int64_t range[10] = {5, 5, 5, 6, 6, 8198, 8198, 16391, 16391, 32776};
    std::vector<int64_t> first, begin, end;
    REQUIRE(ligrec_count_segments(range, 5) == 0 + 1 + 1 + 2 + 3);
    ligrec_segments(range, 5, first, begin, end);
    const int64_t want_first[6] = {0, 0, 1, 2, 4, 7};
    REQUIRE(first.size() == 6 && begin.size() == 7 && end.size() == 7);
    for (int g = 0; g <= 5; ++g) REQUIRE(first[(size_t)g] == want_first[g]);
    for (int g = 0; g < 5; ++g) {
        int64_t e = range[2 * g];
        for (int64_t s = first[(size_t)g]; s < first[(size_t)g + 1]; ++s) {
            REQUIRE(begin[(size_t)s] == e && end[(size_t)s] > e && end[(size_t)s] - e <= LIGREC_SEG);
            if (s + 1 < first[(size_t)g + 1]) REQUIRE(end[(size_t)s] - e == LIGREC_SEG);
            e = end[(size_t)s];
        }
        REQUIRE(e == range[2 * g + 1]);
    }
    REQUIRE(end[6] - begin[6] == 1 && end[3] - begin[3] == 1 && end[1] - begin[1] == LIGREC_SEG);
    return 0;
}

static int check_stats() {
    // K = 3 with class 2 empty, G = 2, P = 3 (a repeated pair, lig == rec)
    const int64_t K = 3, G = 2, P = 3, nperm = 9;
    const int64_t group_n[3] = {10, 4, 0}, nz[6] = {5, 0, 0, 1, 4, 0};   // gene 0: 0.5, 0, -; gene 1: 0.1, 1, -
    const int32_t lig[3] = {0, 0, 1}, rec[3] = {1, 1, 1};
    std::vector<int64_t> n_ge((size_t)(P * K * K));
    for (size_t q = 0; q < n_ge.size(); ++q) n_ge[q] = (int64_t)(q % 10);
    std::vector<uint8_t> ex((size_t)(G * K));
    std::vector<double> p((size_t)(P * K * K)), padj(p.size()), padj_q(p.size());
    ligrec_stats(K, G, P, nperm, group_n, nz, lig, rec, n_ge.data(), 0.2, 0, ex.data(), p.data(), padj.data());
    const uint8_t want_ex[6] = {1, 0, 0, 0, 1, 0};
    for (int q = 0; q < 6; ++q) REQUIRE(ex[(size_t)q] == want_ex[q]);
    int valid = 0;
    for (int64_t b = 0; b < K; ++b)
        for (int64_t a = 0; a < K; ++a)
            for (int64_t q = 0; q < P; ++q) {
                const size_t at = (size_t)(q + P * (a + K * b));
                const bool on = want_ex[lig[q] * K + a] && want_ex[rec[q] * K + b];
                if (on) {
                    ++valid;
                    REQUIRE(p[at] == (double)(1 + n_ge[at]) / 10.0 && padj[at] >= p[at] && padj[at] <= 1.0);
                } else {
                    REQUIRE(p[at] != p[at] && padj[at] != padj[at]);   // NaN outside the mask, and left out of the adjustment
                }
            }
    REQUIRE(valid == 3);   // (0, a = 0, b = 1), its repeat, (2, a = 1, b = 1)
    // the smallest of three valid p is multiplied by 3 at most; per interaction every q has one valid value: padj == p
    ligrec_stats(K, G, P, nperm, group_n, nz, lig, rec, n_ge.data(), 0.2, 1, nullptr, nullptr, padj_q.data());
    for (size_t at = 0; at < p.size(); ++at) {
        if (p[at] == p[at]) REQUIRE(padj_q[at] == p[at] && padj[at] <= 3.0 * p[at]);
        else REQUIRE(padj_q[at] != padj_q[at]);
    }
    // threshold 0: every class with cells is expressed, the empty class never; threshold 1: only the full class
    ligrec_stats(K, G, P, nperm, group_n, nz, lig, rec, n_ge.data(), 0.0, 0, ex.data(), nullptr, nullptr);
    const uint8_t want0[6] = {1, 1, 0, 1, 1, 0};
    for (int q = 0; q < 6; ++q) REQUIRE(ex[(size_t)q] == want0[q]);
    ligrec_stats(K, G, P, nperm, group_n, nz, lig, rec, n_ge.data(), 1.0, 0, ex.data(), p.data(), nullptr);
    const uint8_t want1[6] = {0, 0, 0, 0, 1, 0};
    for (int q = 0; q < 6; ++q) REQUIRE(ex[(size_t)q] == want1[q]);
    REQUIRE(p[(size_t)(2 + P * (1 + K * 1))] == (double)(1 + n_ge[(size_t)(2 + P * (1 + K * 1))]) / 10.0 && p[0] != p[0]);
    REQUIRE(ligrec_threshold_ok(0.0) && ligrec_threshold_ok(1.0) && !ligrec_threshold_ok(NAN) && !ligrec_threshold_ok(-1e-300) && !ligrec_threshold_ok(1.0000001));
    return 0;
}

int main() {
    if (check_plan() || check_refusals() || check_segments() || check_stats()) return 1;
    printf("ligrec_host: ok\n");
    return 0;
}
