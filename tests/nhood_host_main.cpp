// The host logic of the neighbourhood enrichment calls (singlet_amd/csrc/nhood_host.h) as a program of its own, for the address
// and undefined-behaviour sanitizers: the plan at every edge of K, the batch and sort choices, the knobs' refusals, every
// validator refusal with the offender it names, the overflow refusal at its exact boundary, the statistics on hand-made
// tallies with D == 0 and an empty class, and -- given a file as its argument -- the 128-bit statistics against values the
// calling test computed from Python integers (lines "nperm C S1 S2 z mean sd", the doubles as hexadecimal floats, z "nan" when
// D == 0).  No HIP call, no device.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../singlet_amd/csrc/nhood_host.h"

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("nhood_host: FAILED %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

static int check_plan_edges() {
    // permutations per group at both sides of every step, the LDS bytes, and the global path above the last tile
    const struct { int K, pg, path; } want[] = {{1, 16, 1}, {2, 16, 1}, {45, 16, 1}, {46, 8, 1}, {64, 8, 1}, {65, 4, 1}, {90, 4, 1}, {91, 2, 1},
                                                {128, 2, 1}, {129, 1, 1}, {181, 1, 1}, {182, 16, 2}, {256, 16, 2}};
    for (const auto& w : want) {
        NhoodPlan P;
        int64_t at, val;
        REQUIRE(nhood_plan(9000, 70000, w.K, 200, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK);
        REQUIRE(P.path == w.path && P.pg == w.pg);
        REQUIRE(P.lds_bytes == (w.path == 1 ? (int64_t)w.pg * w.K * w.K * 4 : 0) && P.lds_bytes <= NHOOD_LDS_TILE_BYTES);
        REQUIRE(nhood_pg_max(w.K) == (w.path == 1 ? w.pg : 0));
        if (w.path == 1 && w.pg < NHOOD_MAX_PG) REQUIRE((int64_t)2 * w.pg * w.K * w.K * 4 > NHOOD_LDS_TILE_BYTES);   // the step is forced
        // forced: the global path at every K; every power of two up to the cap; nothing above it, no other value
        REQUIRE(nhood_plan(9000, 70000, w.K, 200, 0, 2, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.path == 2 && P.pg == 16 && P.lds_bytes == 0);
        const int cap = w.path == 1 ? w.pg : NHOOD_MAX_PG;
        for (int pg = 1; pg <= 32; ++pg) {
            const bool ok = pg <= cap && (pg & (pg - 1)) == 0;
            const NhoodArgError e = nhood_plan(9000, 70000, w.K, 200, 0, 1, pg, 0, &P, &at, &val);
            REQUIRE(e == (ok ? NHOOD_ARGS_OK : NHOOD_ARGS_PG));
            if (ok) REQUIRE(P.pg == pg && P.path == w.path);
            else REQUIRE(val == pg && at == cap);
        }
    }
    return 0;
}

static int check_plan_rest() {
    NhoodPlan P;
    int64_t at, val;
    // batch: forced as given (capped by nperm), else by the budget in multiples of 16, at least 16
    REQUIRE(nhood_plan(1000, 8000, 3, 200, 7, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.batch == 7);
    REQUIRE(nhood_plan(1000, 8000, 3, 200, 500, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.batch == 200);
    REQUIRE(nhood_plan(1000000, 8000000, 20, 1000, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.batch == 256 && P.sort == 1 && P.sort_perms == 16);
    REQUIRE(nhood_plan(2000000000, 1, 256, 1000, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.batch == 16);
    REQUIRE(nhood_plan(1000, 8000, 3, 1000, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.batch == 1000 && P.sort == 0);
    REQUIRE(P.sort_perms == 1008 && P.sort_perms % 16 == 0);
    REQUIRE(nhood_plan(1000, 8000, 3, 5, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.batch == 5 && P.sort_perms == 16);
    // the sort switch: the default, and the threshold argument on both of its sides
    REQUIRE(nhood_plan(NHOOD_SORT_SWITCH, 1, 3, 10, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.sort == 0);
    REQUIRE(nhood_plan(NHOOD_SORT_SWITCH + 1, 1, 3, 10, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK && P.sort == 1);
    REQUIRE(nhood_plan(64, 1, 3, 10, 0, 0, 0, 64, &P, &at, &val) == NHOOD_ARGS_OK && P.sort == 0);
    REQUIRE(nhood_plan(65, 1, 3, 10, 0, 0, 0, 64, &P, &at, &val) == NHOOD_ARGS_OK && P.sort == 1);
    // the entry cut: whole segments, at most NHOOD_MAX_WG workgroups, every entry covered, none for an empty graph
    const int64_t nnzs[] = {0, 1, NHOOD_SEG, NHOOD_SEG + 1, 9000, (int64_t)NHOOD_SEG * NHOOD_MAX_WG, (int64_t)NHOOD_SEG * NHOOD_MAX_WG + 1, 2147483647};
    for (int64_t nnz : nnzs) {
        REQUIRE(nhood_plan(1000, nnz, 3, 10, 0, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_OK);
        REQUIRE(P.wg_entries % NHOOD_SEG == 0 && P.wg_entries >= NHOOD_SEG && P.wgs <= NHOOD_MAX_WG);
        REQUIRE(P.wgs * P.wg_entries >= nnz && (P.wgs == 0 ? nnz == 0 : (P.wgs - 1) * P.wg_entries < nnz));
    }
    // the knobs' refusals
    REQUIRE(nhood_plan(1000, 8000, 3, 10, 0, 3, 0, 0, &P, &at, &val) == NHOOD_ARGS_PATH && val == 3);
    REQUIRE(nhood_plan(1000, 8000, 3, 10, 0, -1, 0, 0, &P, &at, &val) == NHOOD_ARGS_PATH);
    REQUIRE(nhood_plan(1000, 8000, 3, 10, -1, 0, 0, 0, &P, &at, &val) == NHOOD_ARGS_BATCH && val == -1);
    REQUIRE(nhood_plan(1000, 8000, 3, 10, 0, 0, -2, 0, &P, &at, &val) == NHOOD_ARGS_PG && val == -2);
    return 0;
}

static int check_validators() {
    int64_t at, val;
    // a 4-cell graph: column 0 empty, a repeated row and unsorted rows in column 1, a self-loop in column 2, column 3 empty
    const int32_t Gp[5] = {0, 0, 3, 5, 5}, Gi[5] = {3, 0, 3, 2, 1}, lab[4] = {0, 2, 1, 2};
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_OK);
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 256, NHOOD_MAX_NPERM, 7, &at, &val) == NHOOD_ARGS_OK);
    REQUIRE(nhood_check_call(nullptr, Gp, 4, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_NULL);
    REQUIRE(nhood_check_call(Gi, nullptr, 4, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_NULL);
    REQUIRE(nhood_check_call(Gi, Gp, 4, nullptr, 3, 100, 0, &at, &val) == NHOOD_ARGS_NULL);
    REQUIRE(nhood_check_call(Gi, Gp, 0, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_N);
    REQUIRE(nhood_check_call(Gi, Gp, -1, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_N);
    {
        const int32_t p1[5] = {1, 1, 3, 5, 5}, p2[5] = {0, 3, 2, 5, 5};
        REQUIRE(nhood_check_call(Gi, p1, 4, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_PTR && at == 0 && val == 1);
        REQUIRE(nhood_check_call(Gi, p2, 4, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_PTR && at == 2 && val == 2);
    }
    {
        const int32_t hi[5] = {3, 0, 3, 2, 4}, lo[5] = {3, -1, 3, 2, 1};
        REQUIRE(nhood_check_call(hi, Gp, 4, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_ROW && at == 4 && val == 4);
        REQUIRE(nhood_check_call(lo, Gp, 4, lab, 3, 100, 0, &at, &val) == NHOOD_ARGS_ROW && at == 1 && val == -1);
    }
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 0, 100, 0, &at, &val) == NHOOD_ARGS_K);
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 257, 100, 0, &at, &val) == NHOOD_ARGS_K);
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 2, 100, 0, &at, &val) == NHOOD_ARGS_LABEL && at == 1 && val == 2);
    {
        const int32_t neg[4] = {0, 1, 1, -1};
        REQUIRE(nhood_check_call(Gi, Gp, 4, neg, 3, 100, 0, &at, &val) == NHOOD_ARGS_LABEL && at == 3 && val == -1);
    }
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 3, 0, 0, &at, &val) == NHOOD_ARGS_NPERM && val == 0);
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 3, NHOOD_MAX_NPERM + 1, 0, &at, &val) == NHOOD_ARGS_NPERM);
    REQUIRE(nhood_check_call(Gi, Gp, 4, lab, 3, 100, -1, &at, &val) == NHOOD_ARGS_BATCH && val == -1);
    // several label vectors: the offset of the offender
    {
        const int32_t two[8] = {0, 2, 1, 2, 0, 1, 3, 0};
        REQUIRE(nhood_check_labels(two, 4, 2, 4, &at, &val) == NHOOD_ARGS_OK);
        REQUIRE(nhood_check_labels(two, 4, 2, 3, &at, &val) == NHOOD_ARGS_LABEL && at == 6 && val == 3);
        REQUIRE(nhood_check_labels(two, 4, 1, 3, &at, &val) == NHOOD_ARGS_OK);
    }
    // the range of the stage operator
    REQUIRE(nhood_check_range(0, 1) == NHOOD_ARGS_OK && nhood_check_range(NHOOD_MAX_NPERM - 1, 1) == NHOOD_ARGS_OK);
    REQUIRE(nhood_check_range(0, NHOOD_MAX_NPERM) == NHOOD_ARGS_OK && nhood_check_range(1, NHOOD_MAX_NPERM) == NHOOD_ARGS_RANGE);
    REQUIRE(nhood_check_range(-1, 1) == NHOOD_ARGS_RANGE && nhood_check_range(0, 0) == NHOOD_ARGS_RANGE);
    return 0;
}

static int check_overflow() {
    int64_t val = 0;
    // nnz = 2^21: nnz^2 = 2^42, nperm * 2^42 < 2^63 <=> nperm < 2^21: every nperm of the range fits
    REQUIRE(nhood_max_nperm((int64_t)1 << 21) == ((int64_t)1 << 21) - 1);
    REQUIRE(nhood_check_nperm(NHOOD_MAX_NPERM, (int64_t)1 << 21, 0, &val) == NHOOD_ARGS_OK);
    // nnz = 2^22: nperm < 2^19; the boundary itself is refused, the value below it is taken, and the message's value is exact
    REQUIRE(nhood_max_nperm((int64_t)1 << 22) == ((int64_t)1 << 19) - 1);
    REQUIRE(nhood_check_nperm(((int64_t)1 << 19) - 1, (int64_t)1 << 22, 0, &val) == NHOOD_ARGS_OK);
    REQUIRE(nhood_check_nperm((int64_t)1 << 19, (int64_t)1 << 22, 0, &val) == NHOOD_ARGS_OVERFLOW && val == ((int64_t)1 << 19) - 1);
    // an odd nnz: the quotient by hand.  nnz = 3 000 000 000 does not occur (Gp is int32); 2 000 000 001 does
    {
        const int64_t nnz = 2000000001;
        const unsigned __int128 sq = (unsigned __int128)nnz * nnz;
        const int64_t m = nhood_max_nperm(nnz);
        REQUIRE(m == 2);   // 2 * 4.000000004e18 = 8.0e18 < 2^63 = 9.22e18 <= 3 * 4.0e18
        REQUIRE((unsigned __int128)m * sq < ((unsigned __int128)1 << 63) && (unsigned __int128)(m + 1) * sq >= ((unsigned __int128)1 << 63));
        REQUIRE(nhood_check_nperm(2, nnz, 0, &val) == NHOOD_ARGS_OK && nhood_check_nperm(3, nnz, 0, &val) == NHOOD_ARGS_OVERFLOW && val == 2);
    }
    REQUIRE(nhood_max_nperm(2147483647) == 2 && nhood_max_nperm(0) == INT64_MAX && nhood_max_nperm(1) == INT64_MAX);
    return 0;
}

static int check_stats() {
    // K = 2, nperm = 4.  pair 0: C_r = 1, 2, 3, 2 against C = 3; pair 1: every C_r = 5 (D == 0); pairs 2, 3: an empty class
    const int64_t C[4] = {3, 5, 0, 0}, S1[4] = {8, 20, 0, 0}, S2[4] = {18, 100, 0, 0}, ge[4] = {1, 4, 4, 4}, le[4] = {4, 4, 4, 4};
    double z[4], mean[4], sd[4], pe[4], pd[4], ae[4], ad[4];
    nhood_stats(2, 4, C, S1, S2, ge, le, z, mean, sd, pe, pd, ae, ad);
    REQUIRE(nhood_D(4, 8, 18) == 8 && nhood_D(4, 20, 100) == 0);
    REQUIRE(mean[0] == 2.0 && sd[0] == sqrt(8.0) / 4.0 && z[0] == 4.0 / sqrt(8.0));   // (3 - 2) / sqrt(0.5)
    REQUIRE(mean[1] == 5.0 && sd[1] == 0.0 && z[1] != z[1]);
    REQUIRE(z[2] != z[2] && z[3] != z[3] && mean[2] == 0.0 && sd[3] == 0.0);
    REQUIRE(pe[0] == 2.0 / 5.0 && pd[0] == 1.0 && pe[1] == 1.0 && pe[2] == 1.0);
    REQUIRE(ae[0] == 1.0 && ad[0] == 1.0);   // BH over (0.4, 1, 1, 1): min(1, 4 * 0.4)
    nhood_stats(2, 4, C, S1, S2, ge, le, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    // the largest values the refusals admit: S1 = nperm * nnz, S2 = nperm * nnz^2 with every C_r = nnz: D == 0 exactly
    {
        const int64_t nperm = ((int64_t)1 << 19) - 1, nnz = (int64_t)1 << 22;
        REQUIRE(nhood_D(nperm, nperm * nnz, nperm * nnz * nnz) == 0);
        // and one permutation lower by 1: D = nperm * (2 nnz - 1) ... computed both ways in 128 bits
        const __int128 s1 = (__int128)nperm * nnz - 1, s2 = (__int128)nperm * nnz * nnz - 2 * nnz + 1;
        REQUIRE(nhood_D(nperm, (int64_t)s1, (int64_t)s2) == (__int128)nperm * s2 - s1 * s1 && nhood_D(nperm, (int64_t)s1, (int64_t)s2) == nperm - 1);
    }
    return 0;
}

// lines "nperm C S1 S2 z mean sd"
static int check_file(const char* path) {
    FILE* f = fopen(path, "r");
    REQUIRE(f != nullptr);
    long long nperm, C, S1, S2;
    char zs[64], ms[64], ss[64];
    int lines = 0;
    while (fscanf(f, "%lld %lld %lld %lld %63s %63s %63s", &nperm, &C, &S1, &S2, zs, ms, ss) == 7) {
        const int64_t c = C, s1 = S1, s2 = S2, one = 1;
        double z, mean, sd, pe, pd;
        nhood_stats(1, nperm, &c, &s1, &s2, &one, &one, &z, &mean, &sd, &pe, &pd, nullptr, nullptr);
        const double wz = strtod(zs, nullptr), wm = strtod(ms, nullptr), ws = strtod(ss, nullptr);
        if (!same_bits(z, wz) || !same_bits(mean, wm) || !same_bits(sd, ws)) {
            printf("nhood_host: FAILED line %d of %s: z %a (want %a), mean %a (want %a), sd %a (want %a)\n", lines + 1, path, z, wz, mean, wm, sd, ws);
            fclose(f);
            return 1;
        }
        ++lines;
    }
    fclose(f);
    REQUIRE(lines > 0);
    printf("nhood_host: %d lines of %s\n", lines, path);
    return 0;
}

int main(int argc, char** argv) {
    if (check_plan_edges() || check_plan_rest() || check_validators() || check_overflow() || check_stats()) return 1;
    if (argc > 1 && check_file(argv[1])) return 1;
    printf("nhood_host: ok\n");
    return 0;
}
