// The host logic of the simulated doublets (singlet_amd/csrc/doublet_host.h) as a program of its own, for the address and
// undefined-behaviour sanitizers: the rules of the parent lists and the naming of the first offender, the LDS cap in force
// and the path split by lds_cap, and the slot formula of the kernels (lower bounds and shared-before counts) held against
// the two-pointer merge on random and on edge-case pairs.  No HIP call, no device.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../singlet_amd/csrc/doublet_host.h"

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("doublet_host: FAILED %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint32_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}

struct Col {
    std::vector<int32_t> i;
    std::vector<double> x;
};
// a column of nrow rows keeping every row with probability num / 8, values small integers (0 included: an explicit zero)
static Col random_col(int32_t nrow, uint32_t num) {
    Col c;
    for (int32_t r = 0; r < nrow; ++r)
        if (lcg() % 8 < num) { c.i.push_back(r); c.x.push_back((double)(lcg() % 7) - 3.0); }
    return c;
}

static int check_pair(const Col& a, const Col& b) {
    const int64_t la = (int64_t)a.i.size(), lb = (int64_t)b.i.size();
    std::vector<int32_t> i1((size_t)(la + lb) + 1, -7), i2((size_t)(la + lb) + 1, -7);
    std::vector<double> x1((size_t)(la + lb) + 1, -7.0), x2((size_t)(la + lb) + 1, -7.0);
    int64_t s0 = -1, s1 = -1, s2 = -1;
    const int64_t n0 = doublet_merge_pair(a.i.data(), a.x.data(), la, b.i.data(), b.x.data(), lb, nullptr, nullptr, &s0);
    const int64_t n1 = doublet_merge_pair(a.i.data(), a.x.data(), la, b.i.data(), b.x.data(), lb, i1.data(), x1.data(), &s1);
    const int64_t n2 = doublet_merge_pair_by_slots(a.i.data(), a.x.data(), la, b.i.data(), b.x.data(), lb, i2.data(), x2.data(), &s2);
    REQUIRE(n0 == n1 && n1 == n2 && s0 == s1 && s1 == s2 && n1 == la + lb - s1);
    REQUIRE(i1[(size_t)n1] == -7 && i2[(size_t)n2] == -7);                       // nothing past the column
    for (int64_t q = 0; q < n1; ++q) {
        REQUIRE(i1[(size_t)q] == i2[(size_t)q]);
        REQUIRE(memcmp(&x1[(size_t)q], &x2[(size_t)q], sizeof(double)) == 0);    // bits, a signed zero included
        if (q) REQUIRE(i1[(size_t)q - 1] < i1[(size_t)q]);                       // strictly ascending: every slot written once
    }
    return 0;
}

int main() {
    int list = 0;
    int64_t at = 0, val = 0;
    const int32_t pa[4] = {0, 3, 2, 9}, pb[4] = {1, 10, -1, 2};
    // the scalars first, in their order
    REQUIRE(doublet_check_args(pa, pb, 0, 10, 0, &list, &at, &val) == DOUBLET_ARGS_NSIM && val == 0);
    REQUIRE(doublet_check_args(pa, pb, (int64_t)INT32_MAX + 1, 10, 0, &list, &at, &val) == DOUBLET_ARGS_NSIM);
    REQUIRE(doublet_check_args(nullptr, pb, 4, 10, 0, &list, &at, &val) == DOUBLET_ARGS_NULL && list == 0);
    REQUIRE(doublet_check_args(pa, nullptr, 4, 10, 0, &list, &at, &val) == DOUBLET_ARGS_NULL && list == 1);
    REQUIRE(doublet_check_args(pa, pb, 4, 10, -1, &list, &at, &val) == DOUBLET_ARGS_CAP && val == -1);
    // the first offender position by position, parent_a before parent_b: parent_b[1] = 10 with ncol = 10 ...
    REQUIRE(doublet_check_args(pa, pb, 4, 10, 0, &list, &at, &val) == DOUBLET_ARGS_PARENT && list == 1 && at == 1 && val == 10);
    // ... with ncol = 11 it is the negative one at position 2, and a list cut before it passes (the last read is at n_sim - 1)
    REQUIRE(doublet_check_args(pa, pb, 4, 11, 0, &list, &at, &val) == DOUBLET_ARGS_PARENT && list == 1 && at == 2 && val == -1);
    REQUIRE(doublet_check_args(pa, pb, 2, 11, 0, &list, &at, &val) == DOUBLET_ARGS_OK && list == -1 && at == -1);
    REQUIRE(doublet_check_args(pa, pb, 1, 2, 0, &list, &at, &val) == DOUBLET_ARGS_OK);
    // parent_a at the same position wins over parent_b
    const int32_t qa[2] = {0, 12}, qb[2] = {0, 13};
    REQUIRE(doublet_check_args(qa, qb, 2, 10, 0, &list, &at, &val) == DOUBLET_ARGS_PARENT && list == 0 && at == 1 && val == 12);
    // lists in heap blocks of exactly n_sim values: a read past the end is the sanitizer's to find
    {
        std::vector<int32_t> ha(1000), hb(1000);
        for (int q = 0; q < 1000; ++q) { ha[(size_t)q] = (int32_t)(lcg() % 50); hb[(size_t)q] = (int32_t)(lcg() % 50); }
        REQUIRE(doublet_check_args(ha.data(), hb.data(), 1000, 50, 0, &list, &at, &val) == DOUBLET_ARGS_OK);
        hb[999] = 50;
        REQUIRE(doublet_check_args(ha.data(), hb.data(), 1000, 50, 0, &list, &at, &val) == DOUBLET_ARGS_PARENT && list == 1 && at == 999);
    }

    // the cap in force and the path split
    REQUIRE(doublet_lds_cap(0) == DOUBLET_LDS_CAP && doublet_lds_cap(DOUBLET_LDS_CAP + 1) == DOUBLET_LDS_CAP);
    REQUIRE(doublet_lds_cap(1) == 1 && doublet_lds_cap(128) == 128 && doublet_lds_cap(DOUBLET_LDS_CAP) == DOUBLET_LDS_CAP);
    REQUIRE(doublet_pair_in_lds(64, 64, 128) && doublet_pair_in_lds(127, 0, 128) && !doublet_pair_in_lds(64, 65, 128));
    REQUIRE(doublet_pair_in_lds(0, 0, 1) && doublet_pair_in_lds(1, 0, 1) && !doublet_pair_in_lds(1, 1, 1));
    REQUIRE(!doublet_pair_in_lds(INT32_MAX, INT32_MAX, DOUBLET_LDS_CAP));   // the joint length is taken in 64 bits

    // lower bounds at the edges
    const int32_t asc[5] = {1, 3, 3 + 2, 8, 13};
    REQUIRE(doublet_lower_bound(asc, 5, 0) == 0 && doublet_lower_bound(asc, 5, 1) == 0 && doublet_lower_bound(asc, 5, 2) == 1);
    REQUIRE(doublet_lower_bound(asc, 5, 13) == 4 && doublet_lower_bound(asc, 5, 14) == 5 && doublet_lower_bound(asc, 0, 3) == 0);

    // the slot formula against the two-pointer merge: edge pairs, then random ones at lengths around a chunk of 64
    Col empty, one, full, evens, odds, low, high, neg;
    one.i = {5}; one.x = {2.0};
    for (int32_t r = 0; r < 200; ++r) {
        full.i.push_back(r); full.x.push_back(1.0 + r);
        neg.i.push_back(r); neg.x.push_back(-(1.0 + r));                      // x and -x: every sum a stored zero
        ((r & 1) ? odds : evens).i.push_back(r);
        ((r & 1) ? odds : evens).x.push_back(0.5 * r);
        (r < 100 ? low : high).i.push_back(r);
        (r < 100 ? low : high).x.push_back(3.0);
    }
    const Col* edge[] = {&empty, &one, &full, &evens, &odds, &low, &high, &neg};
    for (const Col* a : edge)
        for (const Col* b : edge)
            if (check_pair(*a, *b)) return 1;
    for (int rep = 0; rep < 300; ++rep) {
        const int32_t nrow = (int32_t)(1 + lcg() % 300);
        const Col a = random_col(nrow, 1 + lcg() % 8), b = random_col(nrow, 1 + lcg() % 8);
        if (check_pair(a, b) || check_pair(a, a)) return 1;
    }
    printf("doublet_host: ok\n");
    return 0;
}
