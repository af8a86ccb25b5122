// Stand-alone driver of singlet_amd/csrc/cluster_host.h (the host logic of sgl_c_louvain that makes no HIP call: the argument
// rules, the naming of a defective entry, the guard and the sweep bookkeeping, the split into the two sweep paths, the
// renumbering by size), meant for a host compiler with -fsanitize=address,undefined: tests/test_louvain_restatement.py
// builds and runs it.  Exit status 0 and the line "cluster_host: ok" mean every check held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/cluster_host.h"

#include <stdio.h>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// exactly as many entries on the heap as the graph has: a read past them is the sanitizer's to find
struct G {
    std::vector<int32_t> p, i;
    std::vector<double> x;
    int64_t n() const { return (int64_t)p.size() - 1; }
};

static LouvainArgError args(const G& g, std::vector<double> res, double tol, int32_t sweeps, int32_t levels, int64_t* pos) {
    return louvain_check_args(g.n(), g.p.data(), g.i.data(), g.x.data(), (int32_t)res.size(), res.data(), tol, sweeps, levels, pos);
}

int main() {
    int64_t pos = 0;
    // a path 0 - 1 - 2 with a self-loop on 1, column 3 empty
    G g{{0, 1, 4, 5, 5}, {1, 0, 1, 2, 1}, {2.0, 2.0, 0.5, 3.0, 3.0}};
    // ---- arguments
    EXPECT(args(g, {1.0}, 1e-7, 64, 32, &pos) == LOUVAIN_ARGS_OK && pos == -1);
    EXPECT(args(g, {0.5, 1.0, 2.0}, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_OK);
    EXPECT(args(g, {1.0}, 0.0, 1024, 32, &pos) == LOUVAIN_ARGS_OK);
    EXPECT(args(g, {}, 1e-7, 64, 32, &pos) == LOUVAIN_ARGS_NRES);
    EXPECT(louvain_check_args(4, g.p.data(), g.i.data(), g.x.data(), 1, nullptr, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_NRES);
    EXPECT(args(g, {1.0, 0.0}, 1e-7, 64, 32, &pos) == LOUVAIN_ARGS_RESOLUTION && pos == 1);
    EXPECT(args(g, {-1.0}, 1e-7, 64, 32, &pos) == LOUVAIN_ARGS_RESOLUTION && pos == 0);
    EXPECT(args(g, {1.0, 2.0, INFINITY}, 1e-7, 64, 32, &pos) == LOUVAIN_ARGS_RESOLUTION && pos == 2);
    EXPECT(args(g, {NAN}, 1e-7, 64, 32, &pos) == LOUVAIN_ARGS_RESOLUTION && pos == 0);
    EXPECT(args(g, {1.0}, -1e-300, 64, 32, &pos) == LOUVAIN_ARGS_TOL);
    EXPECT(args(g, {1.0}, NAN, 64, 32, &pos) == LOUVAIN_ARGS_TOL);
    EXPECT(args(g, {1.0}, 0.0, 0, 32, &pos) == LOUVAIN_ARGS_SWEEPS);
    EXPECT(args(g, {1.0}, 0.0, 1025, 32, &pos) == LOUVAIN_ARGS_SWEEPS);
    EXPECT(args(g, {1.0}, 0.0, 64, 0, &pos) == LOUVAIN_ARGS_LEVELS);
    EXPECT(args(g, {1.0}, 0.0, 64, 33, &pos) == LOUVAIN_ARGS_LEVELS);
    const double one = 1.0;
    EXPECT(louvain_check_args(-1, nullptr, nullptr, nullptr, 1, &one, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_N);
    EXPECT(louvain_check_args(0, nullptr, nullptr, nullptr, 1, &one, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_OK);   // nothing is read
    EXPECT(louvain_check_args(3, nullptr, nullptr, nullptr, 1, &one, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_NULL);
    EXPECT(louvain_check_args(4, g.p.data(), nullptr, g.x.data(), 1, &one, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_NULL);
    G empty{{0, 0, 0}, {}, {}};
    EXPECT(louvain_check_args(2, empty.p.data(), nullptr, nullptr, 1, &one, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_OK);
    G p0{{1, 1, 1}, {}, {}}, down{{0, 2, 1, 3}, {0, 1, 2}, {1.0, 1.0, 1.0}};
    EXPECT(args(p0, {1.0}, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_P0);
    EXPECT(args(down, {1.0}, 0.0, 1, 1, &pos) == LOUVAIN_ARGS_P_DECREASES && pos == 1);

    // ---- the column of an entry, across empty columns
    G gaps{{0, 0, 0, 2, 2, 3, 3}, {0, 1, 2}, {1.0, 1.0, 1.0}};
    EXPECT(louvain_column_of(gaps.p.data(), 6, 0) == 2 && louvain_column_of(gaps.p.data(), 6, 1) == 2);
    EXPECT(louvain_column_of(gaps.p.data(), 6, 2) == 4);
    for (int64_t e = 0; e < 5; ++e) {
        const int64_t c = louvain_column_of(g.p.data(), 4, e);
        EXPECT(g.p[(size_t)c] <= e && e < g.p[(size_t)c + 1]);
    }

    // ---- the defect of an entry
    const int64_t n = 4;
    for (int64_t e = 0; e < 5; ++e)
        EXPECT(louvain_entry_defect(g.p.data(), g.i.data(), g.x.data(), n, louvain_column_of(g.p.data(), n, e), e, true) == LOUVAIN_ENTRY_OK);
    G bad = g;
    bad.i[3] = 4;
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 1, 3, false) == LOUVAIN_ROW_RANGE);
    bad.i[3] = -1;
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 1, 3, false) == LOUVAIN_ROW_RANGE);
    bad = g;
    bad.i[2] = 0;   // column 1: rows 0, 0, 2
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 1, 2, false) == LOUVAIN_ROW_ORDER);
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 1, 1, false) == LOUVAIN_ENTRY_OK);   // the first of a column has no one before it
    bad = g;
    bad.x[4] = INFINITY;
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 2, 4, false) == LOUVAIN_NOT_FINITE);
    bad.x[4] = NAN;
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 2, 4, false) == LOUVAIN_NOT_FINITE);
    bad.x[4] = -3.0;
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 2, 4, false) == LOUVAIN_NEGATIVE);
    bad.x[4] = 3.0000000000000004;   // one ulp off its mirror
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 2, 4, true) == LOUVAIN_ASYMMETRIC);
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 1, 3, true) == LOUVAIN_ASYMMETRIC);
    EXPECT(louvain_entry_defect(bad.p.data(), bad.i.data(), bad.x.data(), n, 2, 4, false) == LOUVAIN_ENTRY_OK);
    G lone{{0, 0, 1, 1}, {2}, {1.0}};   // (2, 1) without (1, 2): column 2 is empty, the search reads nothing
    EXPECT(louvain_entry_defect(lone.p.data(), lone.i.data(), lone.x.data(), 3, 1, 0, true) == LOUVAIN_ASYMMETRIC);
    G lone2{{0, 1, 1, 1}, {2}, {1.0}};  // (2, 0) without (0, 2): column 2, the last one, is empty
    EXPECT(louvain_entry_defect(lone2.p.data(), lone2.i.data(), lone2.x.data(), 3, 0, 0, true) == LOUVAIN_ASYMMETRIC);

    // ---- the guard and the sweep count
    LouvainPhase ph = louvain_phase_begin(0.25, 1e-3, 3);
    EXPECT(louvain_phase_wants_sweep(ph));
    EXPECT(louvain_phase_after_sweep(ph, 5, 0.5) == LOUVAIN_KEEP_GO && ph.q == 0.5 && ph.kept == 1);
    EXPECT(louvain_phase_after_sweep(ph, 2, 0.5005) == LOUVAIN_KEEP_END && ph.q == 0.5005 && ph.kept == 2 && !louvain_phase_wants_sweep(ph));
    ph = louvain_phase_begin(0.25, 0.0, 3);
    EXPECT(louvain_phase_after_sweep(ph, 9, 0.25) == LOUVAIN_DISCARD_END && ph.q == 0.25 && ph.kept == 0 && !louvain_phase_wants_sweep(ph));
    ph = louvain_phase_begin(0.25, 0.0, 3);
    EXPECT(louvain_phase_after_sweep(ph, 9, 0.2) == LOUVAIN_DISCARD_END && ph.q == 0.25);
    ph = louvain_phase_begin(0.25, 0.0, 3);
    EXPECT(louvain_phase_after_sweep(ph, 0, 123.0) == LOUVAIN_DISCARD_END && ph.q == 0.25);   // nothing moved: q_new is not read
    ph = louvain_phase_begin(0.25, 0.0, 3);
    EXPECT(louvain_phase_after_sweep(ph, 1, NAN) == LOUVAIN_DISCARD_END && ph.q == 0.25);
    ph = louvain_phase_begin(0.0, 0.0, 3);
    for (int q = 1; q <= 3; ++q) EXPECT(louvain_phase_wants_sweep(ph) && louvain_phase_after_sweep(ph, 1, 0.1 * q) == LOUVAIN_KEEP_GO);
    EXPECT(!louvain_phase_wants_sweep(ph) && ph.kept == 3 && ph.tried == 3);

    // ---- the two sweep paths
    std::vector<int64_t> wide{0, 0, LOUVAIN_FAST_DEGREE, 2 * LOUVAIN_FAST_DEGREE + 1, 2 * LOUVAIN_FAST_DEGREE + 2, 3 * LOUVAIN_FAST_DEGREE + 10};
    std::vector<int32_t> fast, slow;
    std::vector<int64_t> soff;
    louvain_split(wide.data(), 5, fast, slow, soff);
    EXPECT(fast == (std::vector<int32_t>{0, 1, 3}) && slow == (std::vector<int32_t>{2, 4}));
    EXPECT(soff == (std::vector<int64_t>{0, LOUVAIN_FAST_DEGREE + 1, 2 * LOUVAIN_FAST_DEGREE + 9}));
    louvain_split(g.p.data(), 4, fast, slow, soff);
    EXPECT(fast.size() == 4 && slow.empty() && soff == std::vector<int64_t>{0});
    louvain_split(g.p.data(), 0, fast, slow, soff);
    EXPECT(fast.empty() && slow.empty() && soff.size() == 1);

    // ---- the renumbering: by size descending, ties by smallest member
    std::vector<int32_t> a{5, 2, 2, 5, 0, 2, 7, 7}, lab(8);
    EXPECT(louvain_renumber_by_size(a.data(), 8, lab.data()) == 4);
    EXPECT(lab == (std::vector<int32_t>{1, 0, 0, 1, 3, 0, 2, 2}));   // sizes 3 (id 2), 2 (id 5, first member 0), 2 (id 7, first 6), 1
    EXPECT(louvain_renumber_by_size(a.data(), 8, a.data()) == 4 && a == lab);   // in place
    std::vector<int32_t> single{0};
    EXPECT(louvain_renumber_by_size(single.data(), 1, single.data()) == 1 && single[0] == 0);
    EXPECT(louvain_renumber_by_size(nullptr, 0, nullptr) == 0);
    if (failures == 0) printf("cluster_host: ok\n");
    return failures == 0 ? 0 : 1;
}
