// Stand-alone driver of singlet_amd/csrc/gsea_host.h (the host logic of sgl_c_gsea that makes no HIP call: the argument rules
// and the naming of the offender, the size table, the batch plan, p, NES, the same-side tally and Benjamini-Hochberg), meant
// for a host compiler with -fsanitize=address,undefined: tests/test_gsea_restatement.py builds and runs it.
//   gsea_host_main                    the built-in checks; exit status 0 and the line "gsea_host: ok" mean every check held and
//                                     the sanitizers saw nothing
//   gsea_host_main derive IN OUT      IN: int64 P, k, score_type, nperm, S; int32 size_idx[P]; double es[P k]; int64 n_ge[P k],
//                                     n_le[P k], cnt_pos[S k], cnt_neg[S k]; double sum_pos[S k], sum_neg[S k].
//                                     OUT: double nes[P k], pval[P k], padj[P k]; int64 n_side[P k]
#include "../singlet_amd/csrc/gsea_host.h"

#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run_derive(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int64_t hd[5];
    if (fread(hd, sizeof(int64_t), 5, f) != 5) { fclose(f); return 2; }
    const int64_t P = hd[0], k = hd[1], nperm = hd[3], S = hd[4];
    const int st = (int)hd[2];
    const size_t pk = (size_t)P * (size_t)k, sk = (size_t)S * (size_t)k;
    std::vector<int32_t> size_idx;
    std::vector<double> es, sum_pos, sum_neg;
    std::vector<int64_t> n_ge, n_le, cnt_pos, cnt_neg;
    const bool ok = read_n(f, size_idx, (size_t)P) && read_n(f, es, pk) && read_n(f, n_ge, pk) && read_n(f, n_le, pk) && read_n(f, cnt_pos, sk) &&
                    read_n(f, cnt_neg, sk) && read_n(f, sum_pos, sk) && read_n(f, sum_neg, sk);
    fclose(f);
    if (!ok) return 2;
    // exactly P k values each on the heap: a write past them is the sanitizer's to find
    std::vector<double> nes(pk, -1.0), pval(pk, -1.0), padj(pk, -1.0);
    std::vector<int64_t> n_side(pk, -1);
    gsea_derive(P, k, st, nperm, size_idx.data(), S, es.data(), n_ge.data(), n_le.data(), cnt_pos.data(), cnt_neg.data(), sum_pos.data(),
                sum_neg.data(), nes.data(), pval.data(), n_side.data());
    // NULL outputs are skipped
    gsea_derive(P, k, st, nperm, size_idx.data(), S, es.data(), n_ge.data(), n_le.data(), cnt_pos.data(), cnt_neg.data(), sum_pos.data(),
                sum_neg.data(), nullptr, nullptr, nullptr);
    for (int64_t c = 0; c < k; ++c) gsea_bh(pval.data() + (size_t)P * (size_t)c, P, padj.data() + (size_t)P * (size_t)c);
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    bool wrote = true;
    if (pk) wrote = fwrite(nes.data(), 8, pk, g) == pk && fwrite(pval.data(), 8, pk, g) == pk && fwrite(padj.data(), 8, pk, g) == pk &&
                    fwrite(n_side.data(), 8, pk, g) == pk;
    fclose(g);
    return wrote ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "derive")) return run_derive(argv[2], argv[3]);
    int64_t at = 0, val = 0;
    // ---- scalars, in their order
    EXPECT(gsea_check_scalars(100, 3, 0, 1000, 0) == GSEA_ARGS_OK);
    EXPECT(gsea_check_scalars(100, 1024, 2, GSEA_MAX_NPERM, 7) == GSEA_ARGS_OK);
    EXPECT(gsea_check_scalars(100, 0, 9, 0, -1) == GSEA_ARGS_K);
    EXPECT(gsea_check_scalars(100, 1025, 0, 10, 0) == GSEA_ARGS_K);
    EXPECT(gsea_check_scalars(1, 3, 9, 0, -1) == GSEA_ARGS_GENES);
    EXPECT(gsea_check_scalars(100, 3, 3, 0, -1) == GSEA_ARGS_SCORE);
    EXPECT(gsea_check_scalars(100, 3, -1, 10, 0) == GSEA_ARGS_SCORE);
    EXPECT(gsea_check_scalars(100, 3, 1, 0, -1) == GSEA_ARGS_NPERM);
    EXPECT(gsea_check_scalars(100, 3, 1, (int64_t)GSEA_MAX_NPERM + 1, 0) == GSEA_ARGS_NPERM);
    EXPECT(gsea_check_scalars(100, 3, 1, 10, -1) == GSEA_ARGS_BATCH);
    // ---- w
    {
        std::vector<double> w{0.0, -1.5, 2.0, -0.0, 1e308, 3.0};
        EXPECT(gsea_check_w(w.data(), 3, 2, &at) == GSEA_ARGS_OK);
        w[4] = INFINITY;
        EXPECT(gsea_check_w(w.data(), 3, 2, &at) == GSEA_ARGS_W && at == 4);
        w[1] = NAN;
        EXPECT(gsea_check_w(w.data(), 3, 2, &at) == GSEA_ARGS_W && at == 1);   // the first one is named
        w[1] = -INFINITY;
        EXPECT(gsea_check_w(w.data(), 3, 1, &at) == GSEA_ARGS_W && at == 1);
        EXPECT(gsea_check_w(w.data(), 1, 1, &at) == GSEA_ARGS_OK);             // only m k values are read
    }
    // ---- sets
    {
        const int64_t m = 8;
        std::vector<int32_t> stamp((size_t)m);
        const std::vector<int64_t> ptr{0, 2, 5, 6};
        std::vector<int32_t> genes{0, 7, 3, 1, 2, 7};
        EXPECT(gsea_check_sets(ptr.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_OK && at == -1);
        std::vector<int64_t> p2{1, 2, 5, 6};
        EXPECT(gsea_check_sets(p2.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_PTR && at == 0 && val == 1);
        p2 = {0, 2, 1, 6};
        EXPECT(gsea_check_sets(p2.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_PTR && at == 2 && val == 1);
        p2 = {0, 2, 2, 6};
        EXPECT(gsea_check_sets(p2.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_EMPTY && at == 1);
        // a set of m genes (and of more) is the whole ranking
        std::vector<int32_t> all{0, 1, 2, 3, 4, 5, 6, 7, 0};
        p2 = {0, 8};
        EXPECT(gsea_check_sets(p2.data(), all.data(), 1, m, stamp.data(), &at, &val) == GSEA_ARGS_WHOLE && at == 0 && val == 8);
        p2 = {0, 7};
        EXPECT(gsea_check_sets(p2.data(), all.data(), 1, m, stamp.data(), &at, &val) == GSEA_ARGS_OK);   // s = m - 1 is taken
        // the structure of every set is checked before any gene is read
        genes[0] = 99;
        p2 = {0, 2, 5, 5};
        EXPECT(gsea_check_sets(p2.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_EMPTY && at == 2);
        EXPECT(gsea_check_sets(ptr.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_GENE && at == 0 && val == 99);
        genes[0] = 0;
        genes[4] = -1;
        EXPECT(gsea_check_sets(ptr.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_GENE && at == 4 && val == -1);
        genes[4] = 3;   // set 1 = {3, 1, 3}
        EXPECT(gsea_check_sets(ptr.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_TWICE && at == 4 && val == 3);
        genes[4] = 7;   // 7 is in sets 0, 1 and 2, once each
        EXPECT(gsea_check_sets(ptr.data(), genes.data(), 3, m, stamp.data(), &at, &val) == GSEA_ARGS_OK);
        // the cap
        const int64_t big = GSEA_LDS_CAP + 10;
        std::vector<int32_t> bstamp((size_t)big), ids((size_t)GSEA_LDS_CAP + 1);
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int32_t)i;
        p2 = {0, GSEA_LDS_CAP + 1};
        EXPECT(gsea_check_sets(p2.data(), ids.data(), 1, big, bstamp.data(), &at, &val) == GSEA_ARGS_CAP && val == GSEA_LDS_CAP + 1);
        p2 = {0, GSEA_LDS_CAP};
        EXPECT(gsea_check_sets(p2.data(), ids.data(), 1, big, bstamp.data(), &at, &val) == GSEA_ARGS_OK);
    }
    // ---- the sizes of the stage operator
    {
        const std::vector<int32_t> ok{1, 5, 9}, tie{1, 5, 5}, zero{0, 5}, whole{3, 10};
        EXPECT(gsea_check_sizes(ok.data(), 3, 10, &at, &val) == GSEA_ARGS_OK);
        EXPECT(gsea_check_sizes(tie.data(), 3, 10, &at, &val) == GSEA_ARGS_SIZES && at == 2 && val == 5);
        EXPECT(gsea_check_sizes(zero.data(), 2, 10, &at, &val) == GSEA_ARGS_SIZES && at == 0);
        EXPECT(gsea_check_sizes(whole.data(), 2, 10, &at, &val) == GSEA_ARGS_SIZES && at == 1 && val == 10);
        EXPECT(gsea_check_sizes(nullptr, 2, 10, &at, &val) == GSEA_ARGS_NULL);
        EXPECT(gsea_check_sizes(ok.data(), 0, 10, &at, &val) == GSEA_ARGS_SETS);
        const std::vector<int32_t> cap{GSEA_LDS_CAP, GSEA_LDS_CAP + 1};
        EXPECT(gsea_check_sizes(cap.data(), 1, 100000, &at, &val) == GSEA_ARGS_OK);
        EXPECT(gsea_check_sizes(cap.data(), 2, 100000, &at, &val) == GSEA_ARGS_SIZES && at == 1);
    }
    // ---- the size table
    {
        const std::vector<int64_t> ptr{0, 5, 7, 12, 13, 15};
        std::vector<int32_t> sizes(5, -1), idx(5, -1), ss(5, -1);
        EXPECT(gsea_size_table(ptr.data(), 5, sizes.data(), idx.data(), ss.data()) == 3);
        EXPECT(sizes[0] == 1 && sizes[1] == 2 && sizes[2] == 5);
        EXPECT(idx[0] == 2 && idx[1] == 1 && idx[2] == 2 && idx[3] == 0 && idx[4] == 1);
        EXPECT(ss[0] == 5 && ss[3] == 1);
        EXPECT(gsea_size_table(ptr.data(), 1, sizes.data(), idx.data(), nullptr) == 1 && sizes[0] == 5 && idx[0] == 0);
    }
    // ---- the batch plan
    EXPECT(gsea_batch_size(15, 489, 1000, 0, 0) == 1000);                     // the default budget holds them all
    EXPECT(gsea_batch_size(15, 489, 1000, 7, 0) == 7);
    EXPECT(gsea_batch_size(15, 489, 1000, 5000, 0) == 1000);
    EXPECT(gsea_batch_size(1024, 4096, 1000, 0, 0) == 8);                     // 256 MiB / (1024 * 4096 * 8)
    EXPECT(gsea_batch_size(1024, 4096, 1000, 0, 1) == 1);                     // never below one permutation
    EXPECT(gsea_sort_perms(13714, 1000) == 1000 && gsea_sort_perms(30000, 1000) == 559 && gsea_sort_perms((int64_t)1 << 30, 9) == 1);
    // ---- the std rule
    EXPECT(gsea_std_score(0.5, -0.25) == 0.5 && gsea_std_score(0.25, -0.5) == -0.5);
    EXPECT(gsea_std_score(0.5, -0.5) == 0.0 && !std::signbit(gsea_std_score(0.5, -0.5)) && gsea_std_score(0.0, 0.0) == 0.0);
    // ---- p, NES and the side of a worked case: one factor, two sets of one size, 9 permutations
    {
        const int32_t idx[2] = {0, 0};
        const double es[2] = {0.5, -0.25};
        const int64_t ge[2] = {2, 8}, le[2] = {7, 3}, cp[1] = {6}, cn[1] = {4};
        const double sp[1] = {1.5}, sn[1] = {-2.0};
        double nes[2], p[2];
        int64_t side[2];
        gsea_derive(2, 1, 0, 9, idx, 1, es, ge, le, cp, cn, sp, sn, nes, p, side);
        EXPECT(p[0] == 0.3 && p[1] == 0.9 && side[0] == 6 && side[1] == 6 && nes[0] == 2.0 && nes[1] == -1.0);
        gsea_derive(2, 1, 1, 9, idx, 1, es, ge, le, cp, cn, sp, sn, nes, p, side);
        EXPECT(p[0] == 0.8 && p[1] == 0.4 && side[0] == 4 && nes[0] == 1.0 && nes[1] == -0.5);
        gsea_derive(2, 1, 2, 9, idx, 1, es, ge, le, cp, cn, sp, sn, nes, p, side);
        EXPECT(p[0] == 3.0 / 7.0 && p[1] == 4.0 / 5.0 && side[0] == 6 && side[1] == 4 && nes[0] == 2.0 && nes[1] == -0.5);
        // an empty side and a side whose mean is 0 give NaN
        const int64_t none[1] = {0};
        const double zero[1] = {0.0};
        gsea_derive(2, 1, 0, 9, idx, 1, es, ge, le, none, cn, sp, sn, nes, p, side);
        EXPECT(std::isnan(nes[0]) && side[0] == 0 && p[0] == 0.3);
        gsea_derive(2, 1, 0, 9, idx, 1, es, ge, le, cp, cn, zero, sn, nes, p, side);
        EXPECT(std::isnan(nes[0]) && std::isnan(nes[1]));
    }
    // ---- Benjamini-Hochberg: a worked case, ties, NaN rows left out, nothing at all
    {
        const double p[6] = {0.001, 0.04, NAN, 0.03, 0.04, 0.5};
        double q[6];
        gsea_bh(p, 6, q);
        EXPECT(q[0] == (5.0 / 1.0) * 0.001 && q[3] == (5.0 / 4.0) * 0.04 && q[1] == (5.0 / 4.0) * 0.04 && q[4] == q[1] && q[5] == 0.5);
        EXPECT(std::isnan(q[2]));
        const double one[1] = {0.7}, nan1[1] = {NAN};
        gsea_bh(one, 1, q);
        EXPECT(q[0] == 0.7);
        gsea_bh(nan1, 1, q);
        EXPECT(std::isnan(q[0]));
        gsea_bh(one, 0, q);
        const double big[2] = {0.9, 0.8};
        gsea_bh(big, 2, q);
        EXPECT(q[0] == 0.9 && q[1] == 0.9);   // min(1, 2 * 0.8) capped by the rank above it
    }
    if (failures) { printf("gsea_host: %d check(s) failed\n", failures); return 1; }
    printf("gsea_host: ok\n");
    return 0;
}
