// Stand-alone driver of singlet_amd/csrc/signature_host.h (the host logic of sgl_signature_scores that makes no HIP call: the
// argument rules and the naming of the first defect, the gene -> sets table, the paths, the batches of the long path, the set
// passes, the cap and the score), meant for a host compiler with -fsanitize=address,undefined:
// tests/test_signature_restatement.py builds and runs it.
//   signature_host_main                    the built-in checks; exit status 0 and the line "signature_host: ok" mean every
//                                          check held and the sanitizers saw nothing
//   signature_host_main table IN OUT       IN: int64 m, n_sets, set_ptr[n_sets + 1]; int32 set_genes[set_ptr[n_sets]].
//                                          OUT: int64 gene_ptr[m + 1]; int32 gene_sets[set_ptr[n_sets]]
//   signature_host_main batches IN OUT     IN: int64 n, max_batch_entries, len[n].  OUT: int64 runs, cut[runs + 1]
//   signature_host_main paths IN OUT       IN: int64 n, lds_cap knob, len[n].  OUT: int64 n_small, n_large, n_long, then the
//                                          three lists as int32
//   signature_host_main score IN OUT       IN: int64 n, R; uint64 rank2[n], n_s[n].  OUT: double score[n]
#include "../singlet_amd/csrc/signature_host.h"

#include <stdio.h>
#include <string.h>

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
template <typename T>
static bool write_n(FILE* f, const std::vector<T>& v, size_t n) {
    return n == 0 || fwrite(v.data(), sizeof(T), n, f) == n;
}

static int run_table(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int64_t hd[2];
    std::vector<int64_t> sp;
    std::vector<int32_t> sg;
    bool ok = fread(hd, sizeof(int64_t), 2, f) == 2 && read_n(f, sp, (size_t)hd[1] + 1);
    ok = ok && read_n(f, sg, (size_t)sp[(size_t)hd[1]]);
    fclose(f);
    if (!ok) return 2;
    // exactly m + 1 and set_ptr[n_sets] values on the heap: a write past them is the sanitizer's to find
    std::vector<int64_t> gp((size_t)hd[0] + 1, -1);
    std::vector<int32_t> gs(sg.size(), -1);
    signature_gene_table(sp.data(), sg.data(), hd[1], hd[0], gp.data(), gs.data());
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    ok = write_n(g, gp, gp.size()) && write_n(g, gs, gs.size());
    fclose(g);
    return ok ? 0 : 2;
}

static int run_batches(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int64_t hd[2];
    if (fread(hd, sizeof(int64_t), 2, f) != 2) { fclose(f); return 2; }
    std::vector<int64_t> len;
    const bool ok = read_n(f, len, (size_t)hd[0]);
    fclose(f);
    if (!ok) return 2;
    std::vector<int64_t> cut((size_t)hd[0] + 1);
    const int64_t runs = signature_batches(len.data(), hd[0], hd[1], cut.data());
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    fwrite(&runs, sizeof(int64_t), 1, g);
    fwrite(cut.data(), sizeof(int64_t), (size_t)runs + 1, g);
    fclose(g);
    return 0;
}

static int run_paths(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int64_t hd[2];
    if (fread(hd, sizeof(int64_t), 2, f) != 2) { fclose(f); return 2; }
    std::vector<int64_t> len;
    const bool ok = read_n(f, len, (size_t)hd[0]);
    fclose(f);
    if (!ok) return 2;
    const size_t n = (size_t)hd[0];
    std::vector<int32_t> a(n), b(n), l(n);
    std::vector<int64_t> ll(n);
    int64_t cnt[3] = {0, 0, 0};
    signature_split_paths(len.data(), hd[0], signature_lds_cap(hd[1]), a.data(), &cnt[0], b.data(), &cnt[1], l.data(), ll.data(), &cnt[2]);
    for (int64_t j = 0; j < cnt[2]; ++j)
        if (ll[(size_t)j] != len[(size_t)l[(size_t)j]]) return 3;
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    fwrite(cnt, sizeof(int64_t), 3, g);
    write_n(g, a, (size_t)cnt[0]);
    write_n(g, b, (size_t)cnt[1]);
    write_n(g, l, (size_t)cnt[2]);
    fclose(g);
    return 0;
}

static int run_score(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int64_t hd[2];
    if (fread(hd, sizeof(int64_t), 2, f) != 2) { fclose(f); return 2; }
    std::vector<uint64_t> r2, ns;
    const bool ok = read_n(f, r2, (size_t)hd[0]) && read_n(f, ns, (size_t)hd[0]);
    fclose(f);
    if (!ok) return 2;
    std::vector<double> sc((size_t)hd[0]);
    for (size_t j = 0; j < sc.size(); ++j) sc[j] = signature_score(r2[j], ns[j], (uint64_t)hd[1]);
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    write_n(g, sc, sc.size());
    fclose(g);
    return 0;
}

static SignatureArgError args(const std::vector<int64_t>& sp, const std::vector<int32_t>& sg, int64_t m, int64_t R, int64_t k0, int64_t k1,
                              int64_t k2, int64_t* at, int64_t* val) {
    std::vector<int32_t> stamp((size_t)(m > 0 ? m : 1));   // exactly m values of scratch
    return signature_check_args(sp.data(), sg.data(), (int64_t)sp.size() - 1, m, R, k0, k1, k2, stamp.data(), at, val);
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "table")) return run_table(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "batches")) return run_batches(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "paths")) return run_paths(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "score")) return run_score(argv[2], argv[3]);
    int64_t at = 0, val = 0;
    const std::vector<int64_t> sp{0, 2, 3, 6};
    const std::vector<int32_t> sg{4, 0, 9, 1, 4, 2};
    // ---- arguments
    EXPECT(args(sp, sg, 10, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_OK && at == -1);
    EXPECT(args(sp, sg, 10, 10, 64, 200, 5, &at, &val) == SIGNATURE_ARGS_OK);
    {
        int32_t stamp[10];
        EXPECT(signature_check_args(nullptr, sg.data(), 3, 10, 3, 0, 0, 0, stamp, &at, &val) == SIGNATURE_ARGS_NULL);
        EXPECT(signature_check_args(sp.data(), nullptr, 3, 10, 3, 0, 0, 0, stamp, &at, &val) == SIGNATURE_ARGS_NULL);
        EXPECT(signature_check_args(sp.data(), sg.data(), 0, 10, 3, 0, 0, 0, stamp, &at, &val) == SIGNATURE_ARGS_SETS && val == 0);
        EXPECT(signature_check_args(sp.data(), sg.data(), -2, 10, 3, 0, 0, 0, stamp, &at, &val) == SIGNATURE_ARGS_SETS && val == -2);
    }
    EXPECT(args(sp, sg, 10, 0, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_RANK && val == 0);
    EXPECT(args(sp, sg, 10, 11, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_RANK && val == 11);
    EXPECT(args(sp, sg, 10, 3, -1, 0, 0, &at, &val) == SIGNATURE_ARGS_KNOB && at == 0 && val == -1);
    EXPECT(args(sp, sg, 10, 3, 0, -7, 0, &at, &val) == SIGNATURE_ARGS_KNOB && at == 1 && val == -7);
    EXPECT(args(sp, sg, 10, 3, 0, 0, -3, &at, &val) == SIGNATURE_ARGS_KNOB && at == 2 && val == -3);
    EXPECT(args({1, 2}, sg, 10, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_PTR && at == 0 && val == 1);
    EXPECT(args({0, 2, 1}, sg, 10, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_PTR && at == 2 && val == 1);
    EXPECT(args({0, 2, 2, 3}, sg, 10, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_EMPTY && at == 1);
    EXPECT(args(sp, sg, 10, 2, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_SIZE && at == 2 && val == 3);   // n_s > max_rank
    EXPECT(args(sp, sg, 9, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_GENE && at == 2 && val == 9);
    EXPECT(args(sp, {4, 0, -1, 1, 4, 2}, 10, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_GENE && at == 2 && val == -1);
    EXPECT(args(sp, {4, 0, 9, 1, 4, 1}, 10, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_TWICE && at == 5 && val == 1);
    EXPECT(args(sp, {4, 4, 9, 1, 4, 2}, 10, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_TWICE && at == 1 && val == 4);
    // a gene in several sets is no defect (4 is in sets 0 and 2 above); n_s = max_rank is none
    EXPECT(args({0, 3}, {0, 1, 2}, 3, 3, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_OK);
    // the order of the refusals: sets, rank, knobs, offsets, empty, size, gene, twice -- the first one is named
    EXPECT(args({0, 0}, {0}, 10, 0, -1, 0, 0, &at, &val) == SIGNATURE_ARGS_RANK);
    EXPECT(args({0, 0}, {0}, 10, 1, -1, -1, 0, &at, &val) == SIGNATURE_ARGS_KNOB && at == 0);
    EXPECT(args({0, 0, 5}, {11, 11, 0, 0, 0}, 10, 2, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_EMPTY && at == 0);
    EXPECT(args({0, 1, 4}, {11, 11, 0, 0}, 10, 2, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_SIZE && at == 1);   // all sizes before any gene
    EXPECT(args({0, 2, 4}, {3, 3, 11, 0}, 10, 2, 0, 0, 0, &at, &val) == SIGNATURE_ARGS_TWICE && at == 1);   // set by set
    // ---- the gene -> sets table
    {
        std::vector<int64_t> gp(11, -1);
        std::vector<int32_t> gs(6, -1);
        signature_gene_table(sp.data(), sg.data(), 3, 10, gp.data(), gs.data());
        const int64_t want_p[11] = {0, 1, 2, 3, 3, 5, 5, 5, 5, 5, 6};
        const int32_t want_s[6] = {0, 2, 2, 0, 2, 1};
        for (int g = 0; g < 11; ++g) EXPECT(gp[(size_t)g] == want_p[g]);
        for (int q = 0; q < 6; ++q) EXPECT(gs[(size_t)q] == want_s[q]);
    }
    // ---- the caps in force, the passes
    EXPECT(signature_lds_cap(0) == SIGNATURE_LDS_CAP && signature_lds_cap(64) == 64 && signature_lds_cap(1 << 20) == SIGNATURE_LDS_CAP);
    EXPECT(signature_pass_size(0) == SIGNATURE_PASS_SETS && signature_pass_size(5) == 5 && signature_pass_size(4000) == SIGNATURE_PASS_SETS);
    EXPECT(signature_passes(1, 0) == 1 && signature_passes(1024, 0) == 1 && signature_passes(1025, 0) == 2 && signature_passes(65, 64) == 2);
    EXPECT(signature_batch_cap(0) == SIGNATURE_BATCH_ENTRIES && signature_batch_cap(200) == 200 && signature_batch_cap((int64_t)1 << 40) == INT32_MAX);
    // ---- the paths
    {
        const std::vector<int64_t> len{0, 1024, 1025, 4096, 4097, 7, 30000};
        std::vector<int32_t> a(7), b(7), l(7);
        std::vector<int64_t> ll(7);
        int64_t na = 0, nb = 0, nl = 0;
        signature_split_paths(len.data(), 7, signature_lds_cap(0), a.data(), &na, b.data(), &nb, l.data(), ll.data(), &nl);
        EXPECT(na == 3 && a[0] == 0 && a[1] == 1 && a[2] == 5);
        EXPECT(nb == 2 && b[0] == 2 && b[1] == 3);
        EXPECT(nl == 2 && l[0] == 4 && l[1] == 6 && ll[0] == 4097 && ll[1] == 30000);
        signature_split_paths(len.data(), 7, signature_lds_cap(7), a.data(), &na, b.data(), &nb, l.data(), ll.data(), &nl);
        EXPECT(na == 2 && nb == 0 && nl == 5);   // a cap below the small instance: no cell for the large one
        signature_split_paths(len.data(), 7, signature_lds_cap(2000), a.data(), &na, b.data(), &nb, l.data(), ll.data(), &nl);
        EXPECT(na == 3 && nb == 1 && b[0] == 2 && nl == 3);
        signature_split_paths(len.data(), 0, SIGNATURE_LDS_CAP, a.data(), &na, b.data(), &nb, l.data(), ll.data(), &nl);
        EXPECT(na == 0 && nb == 0 && nl == 0);
    }
    // ---- batches: whole cells, in order, a cell above the cap alone; the default and the int limit
    {
        const std::vector<int64_t> len{5, 5, 11, 3, 3, 3, 10};
        std::vector<int64_t> cut(8);
        EXPECT(signature_batches(len.data(), 7, 10, cut.data()) == 4);
        EXPECT(cut[0] == 0 && cut[1] == 2 && cut[2] == 3 && cut[3] == 6 && cut[4] == 7);
        EXPECT(signature_batches(len.data(), 7, 0, cut.data()) == 1 && cut[1] == 7);
        EXPECT(signature_batches(len.data(), 7, 1, cut.data()) == 7);
        EXPECT(signature_batches(len.data(), 0, 10, cut.data()) == 0 && cut[0] == 0);
        const std::vector<int64_t> big{(int64_t)1 << 30, (int64_t)1 << 30, 1};
        EXPECT(signature_batches(big.data(), 3, (int64_t)1 << 40, cut.data()) == 2 && cut[1] == 1 && cut[2] == 3);
    }
    // ---- the cap and the score
    EXPECT(signature_cap_rank(2 * 5, 5) == 10 && signature_cap_rank(2 * 5 + 1, 5) == 12 && signature_cap_rank(1000, 5) == 12 && signature_cap_rank(2, 5) == 2);
    EXPECT(signature_zero_rank(3, 4, 100) == 11 && signature_zero_rank(3, 4, 5) == 12 && signature_zero_rank(0, 1, 1) == 2);
    EXPECT(signature_score(3 * 4, 3, 1500) == 1.0);                         // the three top genes, untied
    EXPECT(signature_score(3 * (2 * 1500 + 2), 3, 1500) == 1.0 - (double)(3 * 3002 - 12) / (2.0 * 3.0 * 1500.0));
    EXPECT(signature_score(2 * (2 * 7 + 2), 2, 7) == 1.0 - 26.0 / 28.0);    // all capped: (n_s - 1) / (2 R) = 1 / 14
    if (failures) { printf("signature_host: %d check(s) failed\n", failures); return 1; }
    printf("signature_host: ok\n");
    return 0;
}
