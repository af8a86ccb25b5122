// Host logic of sgl_simulate_doublets / sgl_op_pair_columns (include/singlet_hip.h, "Simulated doublets") that makes no HIP
// call: the rules of the parent lists and the naming of the first offender, the LDS cap in force, the path a pair takes,
// the slot formulas of the merge that the device evaluates with the same text, and a plain two-pointer merge of one pair
// that states what the kernels must write.  Plain C++ over plain pointers, so tests/doublet_host_main.cpp compiles it alone
// under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define DBL_HD __host__ __device__
#else
#define DBL_HD
#endif

#define DOUBLET_LDS_CAP 4096   // row indices of both parents together that one wave stages in LDS: the default (and largest) lds_cap

enum DoubletArgError {
    DOUBLET_ARGS_OK = 0,
    DOUBLET_ARGS_NSIM,     // n_sim outside [1, INT32_MAX]; *val = n_sim
    DOUBLET_ARGS_NULL,     // a NULL list; *list = 0 parent_a, 1 parent_b
    DOUBLET_ARGS_CAP,      // lds_cap < 0; *val = lds_cap
    DOUBLET_ARGS_PARENT,   // list *list holds *val outside [0, ncol) at position *at
};

// The refusals that need no device, in this order: n_sim, the lists' addresses, the knob, then every position s in
// ascending order, parent_a[s] before parent_b[s].  Both lists are read completely before anything is launched or freed.
inline DoubletArgError doublet_check_args(const int32_t* parent_a, const int32_t* parent_b, int64_t n_sim, int64_t ncol, int64_t lds_cap,
                                          int* list, int64_t* at, int64_t* val) {
    *list = -1;
    *at = -1;
    *val = 0;
    if (n_sim < 1 || n_sim > (int64_t)INT32_MAX) { *val = n_sim; return DOUBLET_ARGS_NSIM; }
    if (!parent_a) { *list = 0; return DOUBLET_ARGS_NULL; }
    if (!parent_b) { *list = 1; return DOUBLET_ARGS_NULL; }
    if (lds_cap < 0) { *val = lds_cap; return DOUBLET_ARGS_CAP; }
    for (int64_t s = 0; s < n_sim; ++s) {
        if (parent_a[s] < 0 || parent_a[s] >= ncol) { *list = 0; *at = s; *val = parent_a[s]; return DOUBLET_ARGS_PARENT; }
        if (parent_b[s] < 0 || parent_b[s] >= ncol) { *list = 1; *at = s; *val = parent_b[s]; return DOUBLET_ARGS_PARENT; }
    }
    return DOUBLET_ARGS_OK;
}

// the cap in force: a knob of 0 is the default, a larger one is cut to it
inline int64_t doublet_lds_cap(int64_t lds_cap) { return lds_cap > 0 && lds_cap < DOUBLET_LDS_CAP ? lds_cap : DOUBLET_LDS_CAP; }

// the path of a pair: its parents' la + lb row indices are staged in LDS when they fit the cap, else it is long
DBL_HD inline bool doublet_pair_in_lds(int64_t la, int64_t lb, int64_t cap) { return la + lb <= cap; }

// lower bound of `row` in the ascending idx[0 .. n): the number of entries below it
template <typename Ptr>
DBL_HD inline int32_t doublet_lower_bound(Ptr idx, int32_t n, int32_t row) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < row) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The slot of entry j of one parent within the merged column: the j entries of its own parent below it, the `below`
// entries of the other parent below its row, less the rows among them that both parents store (`shared_before`: counted
// once, not twice).  The a-side writes every one of its entries (the sum at a shared row); the b-side writes only its
// unshared ones, with the same formula over its own order.
DBL_HD inline int64_t doublet_slot(int64_t j, int64_t below, int64_t shared_before) { return j + below - shared_before; }

// One pair by the textbook two-pointer merge: what the kernels must write, bit for bit.  Writes the merged column to io /
// xo (room for la + lb; either may be NULL: count only) and returns its length; *shared receives the rows in both parents.
inline int64_t doublet_merge_pair(const int32_t* ia, const double* xa, int64_t la, const int32_t* ib, const double* xb, int64_t lb,
                                  int32_t* io, double* xo, int64_t* shared) {
    int64_t a = 0, b = 0, o = 0, sh = 0;
    while (a < la || b < lb) {
        if (b >= lb || (a < la && ia[a] < ib[b])) {
            if (io) { io[o] = ia[a]; xo[o] = xa[a]; }
            ++a;
        } else if (a >= la || ib[b] < ia[a]) {
            if (io) { io[o] = ib[b]; xo[o] = xb[b]; }
            ++b;
        } else {
            if (io) { io[o] = ia[a]; xo[o] = xa[a] + xb[b]; }
            ++a;
            ++b;
            ++sh;
        }
        ++o;
    }
    if (shared) *shared = sh;
    return o;
}

// The same pair by the kernels' rule, entry by entry (lower bounds and shared-before counts instead of two pointers): the
// stand-alone program holds the two against each other, which is the check of the slot formula itself.
inline int64_t doublet_merge_pair_by_slots(const int32_t* ia, const double* xa, int64_t la, const int32_t* ib, const double* xb, int64_t lb,
                                           int32_t* io, double* xo, int64_t* shared) {
    int64_t sh = 0;
    for (int64_t j = 0; j < la; ++j) {
        const int32_t lbb = doublet_lower_bound(ib, (int32_t)lb, ia[j]);
        const bool hit = lbb < lb && ib[lbb] == ia[j];
        const int64_t o = doublet_slot(j, lbb, sh);
        io[o] = ia[j];
        xo[o] = hit ? xa[j] + xb[lbb] : xa[j];
        sh += hit;
    }
    int64_t shb = 0;
    for (int64_t i = 0; i < lb; ++i) {
        const int32_t lba = doublet_lower_bound(ia, (int32_t)la, ib[i]);
        const bool hit = lba < la && ia[lba] == ib[i];
        if (!hit) {
            const int64_t o = doublet_slot(i, lba, shb);
            io[o] = ib[i];
            xo[o] = xb[i];
        }
        shb += hit;
    }
    if (shared) *shared = sh;
    return la + lb - sh;
}
