// The host logic of the co-occurrence calls (singlet_amd/csrc/cooccur_host.h) as a program of its own, for the address and
// undefined-behaviour sanitizers: every refusal in its stated order with the offender it names, the squared thresholds, the
// bucket grid at the 3 x 3 switch and on an overflowing extent, the bin plan at both sides of the LDS / global switch and of the
// workgroup cap, the flush bound's arithmetic at its edges, the table check and both statistics on hand-made tables.  No HIP
// call, no device.
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../singlet_amd/csrc/cooccur_host.h"

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("cooccur_host: FAILED %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

static int check_refusals() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> x = {0.0, 1.0, 2.0, 3.0}, y = {0.5, 0.25, 4.0, -1.0}, r = {0.0, 1.0, 2.5};
    std::vector<int32_t> lab = {0, 1, 2, 1};
    double thr2[COOCCUR_MAX_T + 1];
    int64_t at, val;
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, r.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_OK);
    REQUIRE(thr2[0] == 0.0 && thr2[1] == 1.0 && thr2[2] == 6.25);
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, r.data(), 2, nullptr, &at, &val) == COOCCUR_ARGS_OK);
    // the order: NULL before n before a coordinate before K before a label before T before r before thr2
    REQUIRE(cooccur_check_call(nullptr, y.data(), 0, lab.data(), 0, r.data(), 0, thr2, &at, &val) == COOCCUR_ARGS_NULL);
    REQUIRE(cooccur_check_call(x.data(), nullptr, 4, lab.data(), 3, r.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_NULL);
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, nullptr, 3, r.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_NULL);
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, nullptr, 2, thr2, &at, &val) == COOCCUR_ARGS_NULL);
    REQUIRE(cooccur_check_call(x.data(), y.data(), 0, lab.data(), 0, r.data(), 0, thr2, &at, &val) == COOCCUR_ARGS_N);
    REQUIRE(cooccur_check_call(x.data(), y.data(), -5, lab.data(), 3, r.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_N);
    std::vector<double> bx = x, by = y;
    by[2] = nan;
    REQUIRE(cooccur_check_call(x.data(), by.data(), 4, lab.data(), 0, r.data(), 0, thr2, &at, &val) == COOCCUR_ARGS_COORD && at == 2 && val == 2);
    bx[3] = -inf;
    REQUIRE(cooccur_check_call(bx.data(), by.data(), 4, lab.data(), 3, r.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_COORD && at == 2 && val == 2);
    by[2] = 0.0;
    REQUIRE(cooccur_check_call(bx.data(), by.data(), 4, lab.data(), 3, r.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_COORD && at == 3 && val == 1);
    for (int64_t K : {0, -1, 257}) REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), K, r.data(), 0, thr2, &at, &val) == COOCCUR_ARGS_K);
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 2, r.data(), 0, thr2, &at, &val) == COOCCUR_ARGS_LABEL && at == 2 && val == 2);
    std::vector<int32_t> neg = lab;
    neg[1] = -7;
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, neg.data(), 256, r.data(), 0, thr2, &at, &val) == COOCCUR_ARGS_LABEL && at == 1 && val == -7);
    for (int64_t T : {0, -1, 65}) REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, r.data(), T, thr2, &at, &val) == COOCCUR_ARGS_T);
    std::vector<double> q = {-0.5, 1.0, 2.0};
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_R && at == 0);
    q = {nan, 1.0, 2.0};
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_R && at == 0);
    q = {0.0, 1.0, inf};
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_R && at == 2);
    q = {0.0, 1.0, 1.0};
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_THR2 && at == 2);
    q = {0.0, 2.0, 1.0};
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_THR2 && at == 2);
    q = {0.0, 1.0, 1e200};   // finite, its square is not
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_THR2 && at == 2);
    q = {1e-200, 2e-200, 1.0};   // ascending, their squares both underflow to 0
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_THR2 && at == 1);
    q = {1.0, 1.0 + 0x1p-52, 2.0};   // ascending by one ulp: the squares still differ
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 3, q.data(), 2, thr2, &at, &val) == COOCCUR_ARGS_OK && thr2[1] > thr2[0]);
    // T = 64 and K = 256 are taken
    std::vector<double> r64(65);
    for (int t = 0; t <= 64; ++t) r64[(size_t)t] = 0.25 * t;
    REQUIRE(cooccur_check_call(x.data(), y.data(), 4, lab.data(), 256, r64.data(), 64, thr2, &at, &val) == COOCCUR_ARGS_OK && thr2[64] == 256.0);
    // the knobs
    REQUIRE(cooccur_check_knobs(0, 0, 0, &at, &val) == COOCCUR_ARGS_OK && cooccur_check_knobs(2, 2, COOCCUR_FLUSH_PAIRS, &at, &val) == COOCCUR_ARGS_OK);
    REQUIRE(cooccur_check_knobs(-1, 0, 0, &at, &val) == COOCCUR_ARGS_KNOB && at == 0 && val == -1);
    REQUIRE(cooccur_check_knobs(3, 0, 0, &at, &val) == COOCCUR_ARGS_KNOB && at == 0 && val == 3);
    REQUIRE(cooccur_check_knobs(0, -2, 0, &at, &val) == COOCCUR_ARGS_KNOB && at == 1 && val == -2);
    REQUIRE(cooccur_check_knobs(0, 3, 0, &at, &val) == COOCCUR_ARGS_KNOB && at == 1);
    REQUIRE(cooccur_check_knobs(0, 0, -1, &at, &val) == COOCCUR_ARGS_KNOB && at == 2 && val == -1);
    REQUIRE(cooccur_check_knobs(0, 0, COOCCUR_FLUSH_PAIRS + 1, &at, &val) == COOCCUR_ARGS_KNOB && at == 2);
    return 0;
}

static int check_grid() {
    const double inf = std::numeric_limits<double>::infinity();
    // 100 x 100 extent, reach 10: side 10 (1 + 2^-10), floor(100 / side) = 9, W = H = 11
    CooccurGrid g = cooccur_grid(0.0, 100.0, -50.0, 50.0, 10.0, 0);
    REQUIRE(g.mode == 2 && g.W == 11 && g.H == 11 && g.side == 10.0 * (1.0 + 0x1p-10) && g.xmin == 0.0 && g.ymin == -50.0);
    // the 3 x 3 switch: W = floor(ext / side) + 2 <= 3 on both axes is one bucket; 4 on either axis is the grid
    g = cooccur_grid(0.0, 100.0, 0.0, 100.0, 60.0, 0);
    REQUIRE(g.mode == 1 && g.W == 1 && g.H == 1);
    g = cooccur_grid(0.0, 100.0, 0.0, 100.0, 60.0, 2);
    REQUIRE(g.mode == 2 && g.W == 3 && g.H == 3);
    g = cooccur_grid(0.0, 100.0, 0.0, 10.0, 49.0, 0);
    REQUIRE(g.mode == 2 && g.W == 4 && g.H == 2);
    g = cooccur_grid(0.0, 10.0, 0.0, 100.0, 49.0, 0);
    REQUIRE(g.mode == 2 && g.W == 2 && g.H == 4);
    g = cooccur_grid(0.0, 100.0, 0.0, 100.0, 10.0, 1);
    REQUIRE(g.mode == 1 && g.W == 1 && g.H == 1);
    // squidpy's default: half the diagonal is one bucket
    g = cooccur_grid(0.0, 1.0, 0.0, 1.0, 0.70710678, 0);
    REQUIRE(g.mode == 1);
    // an overflowing extent is one bucket in every mode
    for (int mode = 0; mode <= 2; ++mode) {
        g = cooccur_grid(-1.7e308, 1.7e308, 0.0, 1.0, 1.0, mode);
        REQUIRE(g.mode == 1 && g.W == 1 && g.H == 1);
    }
    REQUIRE(cooccur_grid(0.0, inf, 0.0, 1.0, 1.0, 2).mode == 1);
    // a tiny reach: the side is raised so that no bucket coordinate passes 2^30
    g = cooccur_grid(0.0, 1.0, 0.0, 0.5, 0.0, 2);
    REQUIRE(g.mode == 2 && g.side == 0x1p-30 && g.W == (((int64_t)1 << 30) + 2) && g.H == (((int64_t)1 << 29) + 2));
    // all points in one spot, reach 0: the floor keeps the side positive
    g = cooccur_grid(3.0, 3.0, 4.0, 4.0, 0.0, 2);
    REQUIRE(g.mode == 2 && g.W == 2 && g.H == 2 && g.side > 0.0);
    return 0;
}

static int check_plan() {
    CooccurPlan P;
    // the LDS / global switch: T K^2 4 + 6144 <= 131072, i.e. T K^2 <= 31232
    REQUIRE(cooccur_lds_fits(20, 50) && cooccur_lds_fits(176, 1) && !cooccur_lds_fits(177, 1) && cooccur_lds_fits(22, 64) && !cooccur_lds_fits(23, 64));
    REQUIRE(cooccur_lds_fits(1, 64) && !cooccur_lds_fits(256, 1) && cooccur_lds_fits(5, 7));
    cooccur_plan(1500, 20, 50, 2, 0, 0, &P);
    REQUIRE(P.path == 1 && P.lds_bytes == 6144 + 50 * 400 * 4 && P.tiles == 6 && P.tiles_per_wg == 1 && P.wgs == 6 && P.split == 1);
    REQUIRE(P.flush_pairs == COOCCUR_FLUSH_PAIRS && P.lds_bytes <= COOCCUR_LDS_BYTES);
    cooccur_plan(1500, 177, 1, 2, 1, 0, &P);   // forced LDS, bins that do not fit: global all the same
    REQUIRE(P.path == 2 && P.lds_bytes == 6144);
    cooccur_plan(1500, 5, 7, 2, 2, 50000, &P);
    REQUIRE(P.path == 2 && P.lds_bytes == 6144 && P.flush_pairs == 50000);
    // the all-pairs regime splits the candidates: 6 tiles give min(ceil(2048 / 6), 64, 6) = 6
    cooccur_plan(1500, 5, 7, 1, 0, 0, &P);
    REQUIRE(P.split == 6 && P.wgs == 6);
    cooccur_plan(100000, 20, 50, 1, 0, 0, &P);
    REQUIRE(P.tiles == 391 && P.wgs == 391 && P.split == 6);
    cooccur_plan(1, 1, 1, 1, 0, 0, &P);
    REQUIRE(P.tiles == 1 && P.wgs == 1 && P.split == 1);
    // the workgroup cap: 1024 tiles are 1024 workgroups, one more makes every workgroup take two
    cooccur_plan((int64_t)COOCCUR_MAX_WG * COOCCUR_TILE, 5, 7, 2, 0, 0, &P);
    REQUIRE(P.tiles == 1024 && P.tiles_per_wg == 1 && P.wgs == 1024);
    cooccur_plan((int64_t)COOCCUR_MAX_WG * COOCCUR_TILE + 1, 5, 7, 2, 0, 0, &P);
    REQUIRE(P.tiles == 1025 && P.tiles_per_wg == 2 && P.wgs == 513);
    cooccur_plan(2147483647, 5, 7, 1, 0, 0, &P);
    REQUIRE(P.tiles == 8388608 && P.tiles_per_wg == 8192 && P.wgs == 1024 && P.split == 2);
    return 0;
}

static int check_flush() {
    const int64_t B = COOCCUR_FLUSH_PAIRS, stage = (int64_t)COOCCUR_TILE * COOCCUR_TILE;
    REQUIRE(!cooccur_must_flush(0, stage, B) && !cooccur_must_flush(0, stage, 1));          // nothing to flush
    REQUIRE(!cooccur_must_flush(B - stage, stage, B));                                        // lands exactly on the bound: fits
    REQUIRE(cooccur_must_flush(B - stage + 1, stage, B));                                     // one more would pass it
    REQUIRE(cooccur_must_flush(B, 1, B) && !cooccur_must_flush(B - 1, 1, B));
    REQUIRE(cooccur_must_flush(1, stage, 50000) && cooccur_must_flush(1, 2, 2) && !cooccur_must_flush(1, 1, 2));
    REQUIRE(cooccur_must_flush(INT64_MAX, stage, B));                                         // no sum is formed: nothing overflows
    // a walk: stages of 65 536 pairs under the plan's bound flush after 65 535 of them
    int64_t since = 0, flushes = 0;
    for (int64_t s = 0; s < 65536 + 3; ++s) {
        if (cooccur_must_flush(since, stage, B)) { since = 0; ++flushes; }
        since += stage;
        REQUIRE(since <= B);
    }
    REQUIRE(flushes == 1);
    return 0;
}

static int check_stats() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // K = 3 (class 2 empty), T = 2
    const int64_t K = 3, T = 2, KK = 9;
    std::vector<int64_t> N((size_t)(KK * T), 0);
    auto at3 = [&](int64_t a, int64_t b, int64_t t) -> int64_t& { return N[(size_t)(a + K * b + KK * t)]; };
    at3(0, 0, 0) = 4; at3(0, 1, 0) = 3; at3(1, 0, 0) = 3; at3(1, 1, 0) = 2;
    at3(0, 0, 1) = 6; at3(0, 1, 1) = 10; at3(1, 0, 1) = 10; at3(1, 1, 1) = 0;
    int64_t at;
    REQUIRE(cooccur_table_ok(K, T, N.data(), &at) && at == -1);
    std::vector<double> ratio((size_t)(KK * T));
    std::vector<int64_t> scratch((size_t)(KK + K));
    cooccur_stats(K, T, N.data(), false, ratio.data(), scratch.data());
    // interval 0: row = (7, 5, 0), tot = 12
    REQUIRE(same_bits(ratio[0], (4.0 / 7.0) / (7.0 / 12.0)) && same_bits(ratio[0 + K * 1], (3.0 / 7.0) / (5.0 / 12.0)));
    REQUIRE(same_bits(ratio[1 + K * 0], (3.0 / 5.0) / (7.0 / 12.0)) && same_bits(ratio[1 + K * 1], (2.0 / 5.0) / (5.0 / 12.0)));
    for (int64_t q = 0; q < K; ++q) REQUIRE(same_bits(ratio[(size_t)(2 + K * q)], nan) && same_bits(ratio[(size_t)(q + K * 2)], nan));
    // interval 1: row = (16, 10, 0), tot = 26; a zero count with both rows present is 0, not NaN
    REQUIRE(same_bits(ratio[(size_t)(KK + 1 + K * 1)], 0.0) && same_bits(ratio[(size_t)(KK + 0)], (6.0 / 16.0) / (16.0 / 26.0)));
    cooccur_stats(K, T, N.data(), true, ratio.data(), scratch.data());
    // cumulative interval 1: N = (10, 13; 13, 2), row = (23, 15), tot = 38
    REQUIRE(same_bits(ratio[(size_t)(KK + 0 + K * 1)], (13.0 / 23.0) / (15.0 / 38.0)) && same_bits(ratio[(size_t)(KK + 1 + K * 1)], (2.0 / 15.0) / (15.0 / 38.0)));
    REQUIRE(same_bits(ratio[0], (4.0 / 7.0) / (7.0 / 12.0)));
    // what is no tally
    std::vector<int64_t> bad = N;
    bad[(size_t)(0 + K * 1)] = 4;   // asymmetric
    REQUIRE(!cooccur_table_ok(K, T, bad.data(), &at) && at == 1);
    bad = N;
    bad[(size_t)(KK + 1 + K * 1)] = 3;   // an odd diagonal
    REQUIRE(!cooccur_table_ok(K, T, bad.data(), &at) && at == KK + 4);
    bad = N;
    bad[0] = -2;
    REQUIRE(!cooccur_table_ok(K, T, bad.data(), &at) && at == 0);
    bad = N;
    bad[0] = INT64_MAX - 1;   // even, symmetric, and the total passes 2^63
    REQUIRE(!cooccur_table_ok(K, T, bad.data(), &at));
    // Ripley: class 0 of 3 points, class 1 of 2, class 2 empty; area 8
    const int64_t gn[3] = {3, 2, 0};
    std::vector<double> Kf((size_t)(K * T)), L((size_t)(K * T));
    REQUIRE(cooccur_ripley_check(K, T, N.data(), gn, 8.0, &at) == 3 && at == 0);   // 10 ordered pairs among 3 points cannot be
    at3(0, 0, 0) = 2; at3(0, 0, 1) = 4;
    REQUIRE(cooccur_ripley_check(K, T, N.data(), gn, 8.0, &at) == 0);
    cooccur_ripley(K, T, N.data(), gn, 8.0, Kf.data(), L.data());
    REQUIRE(same_bits(Kf[0], (8.0 * 2.0) / 6.0) && same_bits(Kf[(size_t)K], (8.0 * 6.0) / 6.0) && same_bits(Kf[1], (8.0 * 2.0) / 2.0));
    REQUIRE(same_bits(L[0], sqrt(((8.0 * 2.0) / 6.0) / COOCCUR_PI)) && same_bits(Kf[2], nan) && same_bits(L[(size_t)(K + 2)], nan));
    cooccur_ripley(K, T, N.data(), gn, 8.0, nullptr, L.data());
    cooccur_ripley(K, T, N.data(), gn, 8.0, Kf.data(), nullptr);
    const int64_t one[3] = {3, 1, 0};   // a class of one point: NaN, and its diagonal must be empty
    REQUIRE(cooccur_ripley_check(K, T, N.data(), one, 8.0, &at) == 3 && at == 1);
    REQUIRE(cooccur_ripley_check(K, T, N.data(), gn, 0.0, &at) == 1 && cooccur_ripley_check(K, T, N.data(), gn, -1.0, &at) == 1);
    REQUIRE(cooccur_ripley_check(K, T, N.data(), gn, nan, &at) == 1 && cooccur_ripley_check(K, T, N.data(), gn, std::numeric_limits<double>::infinity(), &at) == 1);
    const int64_t negn[3] = {3, -1, 0};
    REQUIRE(cooccur_ripley_check(K, T, N.data(), negn, 8.0, &at) == 2 && at == 1);
    return 0;
}

int main() {
    if (check_refusals() || check_grid() || check_plan() || check_flush() || check_stats()) return 1;
    printf("cooccur_host: ok\n");
    return 0;
}
