// Stand-alone driver of singlet_amd/csrc/markers_host.h (the host logic of sgl_markers that makes no HIP call: the argument
// rules and the naming of a defective label, the cluster sizes, the split into the two rank paths, the batches of the long
// path, the derived statistics), meant for a host compiler with -fsanitize=address,undefined:
// tests/test_markers_restatement.py builds and runs it.
//   markers_host_main                      the built-in checks; exit status 0 and the line "markers_host: ok" mean every
//                                          check held and the sanitizers saw nothing
//   markers_host_main derive IN OUT        IN: int32 m, G; double pseudocount; int64 group_n[G], pos[m G]; double sum[m G];
//                                          int64 rank2[m G]; uint64 tie[m].  OUT: pct_in, pct_out, log2fc, z, p, m G doubles each
//   markers_host_main batches IN OUT       IN: int64 n, max_batch_entries, len[n].  OUT: int64 runs, cut[runs + 1]
#include "../singlet_amd/csrc/markers_host.h"

#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static MarkersArgError args(const std::vector<int32_t>& l, int32_t G, int transform, double pc, int64_t* pos, int32_t* val) {
    return markers_check_args(l.data(), (int64_t)l.size(), G, transform, pc, pos, val);
}

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run_derive(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int32_t hd[2];
    double pc;
    if (fread(hd, sizeof(int32_t), 2, f) != 2 || fread(&pc, sizeof(double), 1, f) != 1) { fclose(f); return 2; }
    const int32_t m = hd[0], G = hd[1];
    const size_t mg = (size_t)m * (size_t)G;
    std::vector<int64_t> gn, pos, rank2;
    std::vector<double> sum;
    std::vector<uint64_t> tie;
    const bool ok = read_n(f, gn, (size_t)G) && read_n(f, pos, mg) && read_n(f, sum, mg) && read_n(f, rank2, mg) && read_n(f, tie, (size_t)m);
    fclose(f);
    if (!ok) return 2;
    // exactly m G doubles each on the heap: a write past them is the sanitizer's to find
    std::vector<double> o[5];
    for (auto& v : o) v.assign(mg, -1.0);
    markers_derive(m, G, gn.data(), pos.data(), sum.data(), rank2.data(), tie.data(), pc, o[0].data(), o[1].data(), o[2].data(), o[3].data(),
                   o[4].data());
    // NULL outputs and inputs are skipped, not read
    markers_derive(m, G, gn.data(), nullptr, nullptr, rank2.data(), tie.data(), pc, nullptr, nullptr, nullptr, nullptr, o[4].data());
    markers_derive(m, G, gn.data(), pos.data(), sum.data(), nullptr, nullptr, pc, o[0].data(), nullptr, o[2].data(), nullptr, nullptr);
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    for (auto& v : o)
        if (mg && fwrite(v.data(), sizeof(double), mg, g) != mg) { fclose(g); return 2; }
    fclose(g);
    return 0;
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
    const int64_t runs = markers_batches(len.data(), hd[0], hd[1], cut.data());
    FILE* g = fopen(out, "wb");
    if (!g) return 2;
    fwrite(&runs, sizeof(int64_t), 1, g);
    fwrite(cut.data(), sizeof(int64_t), (size_t)runs + 1, g);
    fclose(g);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "derive")) return run_derive(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "batches")) return run_batches(argv[2], argv[3]);
    int64_t pos = 0;
    int32_t val = 0;
    const std::vector<int32_t> l{0, 1, -1, 2, 1};
    // ---- arguments
    EXPECT(args(l, 3, 1, 1.0, &pos, &val) == MARKERS_ARGS_OK && pos == -1);
    EXPECT(args(l, 1024, 0, 0.0, &pos, &val) == MARKERS_ARGS_OK);
    EXPECT(markers_check_args(nullptr, 5, 3, 1, 1.0, &pos, &val) == MARKERS_ARGS_NULL);
    EXPECT(args(l, 0, 1, 1.0, &pos, &val) == MARKERS_ARGS_GROUPS);
    EXPECT(args(l, 1025, 1, 1.0, &pos, &val) == MARKERS_ARGS_GROUPS);
    EXPECT(args(l, 3, 2, 1.0, &pos, &val) == MARKERS_ARGS_TRANSFORM);
    EXPECT(args(l, 3, -1, 1.0, &pos, &val) == MARKERS_ARGS_TRANSFORM);
    EXPECT(args(l, 3, 1, -1e-300, &pos, &val) == MARKERS_ARGS_PSEUDOCOUNT);
    EXPECT(args(l, 3, 1, INFINITY, &pos, &val) == MARKERS_ARGS_PSEUDOCOUNT);
    EXPECT(args(l, 3, 1, NAN, &pos, &val) == MARKERS_ARGS_PSEUDOCOUNT);
    EXPECT(markers_check_args(l.data(), MARKERS_MAX_CELLS + 1, 3, 1, 1.0, &pos, &val) == MARKERS_ARGS_CELLS);   // before the list is read
    EXPECT(markers_check_args(l.data(), -1, 3, 1, 1.0, &pos, &val) == MARKERS_ARGS_CELLS);
    EXPECT(args(l, 2, 1, 1.0, &pos, &val) == MARKERS_ARGS_LABEL && pos == 3 && val == 2);
    EXPECT(args({0, -2, 5}, 3, 1, 1.0, &pos, &val) == MARKERS_ARGS_LABEL && pos == 1 && val == -2);   // the first one is named
    EXPECT(markers_check_args(l.data(), 0, 3, 1, 1.0, &pos, &val) == MARKERS_ARGS_OK);   // no cell: nothing is read
    // the order of the refusals: groups before transform before pseudocount before cells before labels
    EXPECT(args({7}, 0, 9, -1.0, &pos, &val) == MARKERS_ARGS_GROUPS);
    EXPECT(args({7}, 3, 9, -1.0, &pos, &val) == MARKERS_ARGS_TRANSFORM);
    EXPECT(args({7}, 3, 1, -1.0, &pos, &val) == MARKERS_ARGS_PSEUDOCOUNT);
    // ---- cluster sizes
    {
        std::vector<int64_t> gn(4, -1);
        EXPECT(markers_group_counts(l.data(), 5, 4, gn.data()) == 4);
        EXPECT(gn[0] == 1 && gn[1] == 2 && gn[2] == 1 && gn[3] == 0);
        const std::vector<int32_t> none{-1, -1};
        EXPECT(markers_group_counts(none.data(), 2, 1, gn.data()) == 0 && gn[0] == 0);
    }
    // ---- the two paths
    {
        const std::vector<int64_t> count{0, 2048, 2049, 7, 1 << 21};
        std::vector<int32_t> s(5), g(5);
        std::vector<int64_t> len(5);
        int64_t ns = 0, nl = 0;
        markers_split_paths(count.data(), 5, MARKERS_LDS_CAP, s.data(), &ns, g.data(), len.data(), &nl);
        EXPECT(ns == 3 && s[0] == 0 && s[1] == 1 && s[2] == 3);
        EXPECT(nl == 2 && g[0] == 2 && g[1] == 4 && len[0] == 2049 && len[1] == (1 << 21));
        markers_split_paths(count.data(), 0, MARKERS_LDS_CAP, s.data(), &ns, g.data(), len.data(), &nl);
        EXPECT(ns == 0 && nl == 0);
    }
    // ---- batches: whole genes, in order, a gene above the cap alone; the default and the int limit
    {
        const std::vector<int64_t> len{5, 5, 11, 3, 3, 3, 10};
        std::vector<int64_t> cut(8);
        EXPECT(markers_batches(len.data(), 7, 10, cut.data()) == 4);
        EXPECT(cut[0] == 0 && cut[1] == 2 && cut[2] == 3 && cut[3] == 6 && cut[4] == 7);
        EXPECT(markers_batches(len.data(), 7, 0, cut.data()) == 1 && cut[1] == 7);    // the default holds them all
        EXPECT(markers_batches(len.data(), 7, 1, cut.data()) == 7);
        EXPECT(markers_batches(len.data(), 0, 10, cut.data()) == 0 && cut[0] == 0);
        const std::vector<int64_t> big{(int64_t)1 << 30, (int64_t)1 << 30, 1};
        EXPECT(markers_batches(big.data(), 3, (int64_t)1 << 40, cut.data()) == 2 && cut[1] == 1 && cut[2] == 3);   // never above INT32_MAX
    }
    // ---- derived statistics of a worked case: values 1 2 | 3 4, no ties: U = 0 for cluster 0
    {
        const int64_t gn[2] = {2, 2}, ps[2] = {2, 2}, r2[2] = {2 * 3, 2 * 7};
        const double sm[2] = {3.0, 7.0};
        const uint64_t tie[1] = {0};
        double pi[2], po[2], fc[2], z[2], p[2];
        markers_derive(1, 2, gn, ps, sm, r2, tie, 1.0, pi, po, fc, z, p);
        EXPECT(pi[0] == 1.0 && po[0] == 1.0 && pi[1] == 1.0);
        EXPECT(fc[0] == log2(2.5) - log2(4.5) && fc[1] == -fc[0]);
        // U2 = 6 - 6 = 0, D = -4, a = 1.5, var = (4 / 12) * 5
        EXPECT(z[0] == -(1.5 / sqrt((2.0 * 2.0 / 12.0) * 5.0)) && z[1] == -z[0]);
        EXPECT(p[0] == p[1] && p[0] > 0.24 && p[0] < 0.25);
        // an empty cluster and an all-tied gene give NaN
        const int64_t gn0[2] = {4, 0}, r0[2] = {4 * 5, 0}, ps0[2] = {2, 0};
        const uint64_t tall[1] = {4 * 4 * 4 - 4};
        markers_derive(1, 2, gn0, ps0, sm, r0, tie, 1.0, pi, po, fc, z, p);
        EXPECT(std::isnan(z[0]) && std::isnan(p[0]) && std::isnan(z[1]) && std::isnan(pi[1]) && std::isnan(po[0]));
        markers_derive(1, 2, gn, ps, sm, r2, tall, 1.0, pi, po, fc, z, p);
        EXPECT(std::isnan(z[0]) && std::isnan(p[1]));
    }
    if (failures) { printf("markers_host: %d check(s) failed\n", failures); return 1; }
    printf("markers_host: ok\n");
    return 0;
}
