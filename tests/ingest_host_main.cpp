// Stand-alone driver of singlet_amd/csrc/ingest_host.h (the host logic of sgl_upload_typed that makes no HIP call), meant
// for a host compiler with -fsanitize=address,undefined: tests/test_native_host.py builds and runs it.  Exit status 0
// and the line "ingest_host: ok" mean every check held and the sanitizers saw nothing.
#include "../singlet_amd/csrc/ingest_host.h"

#include <stdio.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static std::vector<int64_t> edges(const std::vector<int64_t>& len, int64_t cap) {
    std::vector<int64_t> cut(len.size() + 1, -1);   // exactly n + 1 values: a write past it is the sanitizer's to find
    const int64_t runs = ingest_batch_edges(len.data(), (int64_t)len.size(), cap, cut.data());
    cut.resize((size_t)runs + 1);
    return cut;
}

int main() {
    const int64_t I32MAX = 2147483647;
    int dummy = 0;
    const void* p = &dummy;
    // ---- arguments
    EXPECT(ingest_check_args(p, 1, p, 3, p, 2, 5, 200, 0, 0, 1u, 1u) == INGEST_ARGS_OK);
    EXPECT(ingest_check_args(nullptr, 1, p, 3, p, 2, 5, 200, 0, 0, 0u, 1u) == INGEST_ARGS_NULL);
    EXPECT(ingest_check_args(p, 4, p, 3, p, 2, 5, 200, 0, 0, 0u, 1u) == INGEST_ARGS_X_TYPE);
    EXPECT(ingest_check_args(p, -1, p, 3, p, 2, 5, 200, 0, 0, 0u, 1u) == INGEST_ARGS_X_TYPE);
    EXPECT(ingest_check_args(p, 0, p, 0, p, 2, 5, 200, 0, 0, 0u, 1u) == INGEST_ARGS_IDX_TYPE);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 1, 5, 200, 0, 0, 0u, 1u) == INGEST_ARGS_PTR_TYPE);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 2, 0, 200, 0, 0, 0u, 1u) == INGEST_ARGS_EXTENT);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 2, 5, I32MAX + 1, 0, 0, 0u, 1u) == INGEST_ARGS_EXTENT);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 2, I32MAX + 1, 5, 0, 0, 0u, 1u) == INGEST_ARGS_EXTENT);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 2, I32MAX, I32MAX, 1, 1, 0u, 1u) == INGEST_ARGS_OK);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 2, 5, 200, 2, 0, 0u, 1u) == INGEST_ARGS_MAJOR);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 2, 5, 200, 0, 2, 0u, 1u) == INGEST_ARGS_SPACE);
    EXPECT(ingest_check_args(p, 0, p, 2, p, 2, 5, 200, 0, 0, 2u, 1u) == INGEST_ARGS_FLAGS);
    EXPECT(ingest_type_bytes(INGEST_F64) == 8 && ingest_type_bytes(INGEST_F32) == 4 && ingest_type_bytes(INGEST_I32) == 4 && ingest_type_bytes(INGEST_I64) == 8);
    // ---- layout
    IngestLayout L = ingest_layout(0, 90, 60);
    EXPECT(L.filled == 0 && L.genes == 60 && L.cells == 90);
    L = ingest_layout(1, 60, 90);
    EXPECT(L.filled == 1 && L.genes == 60 && L.cells == 90);
    // ---- offsets, both widths
    int64_t nnz = -7;
    {
        std::vector<int32_t> a{0, 5, 135, 135, 142, 145};
        EXPECT(ingest_check_offsets(a.data(), 5, &nnz) == -1 && nnz == 145);
        a[0] = 1;
        EXPECT(ingest_check_offsets(a.data(), 5, &nnz) == 0 && nnz == 0);
        a[0] = 0;
        a[3] = 134;
        EXPECT(ingest_check_offsets(a.data(), 5, &nnz) == 3);
        a[3] = 135;
        a[5] = 141;
        EXPECT(ingest_check_offsets(a.data(), 5, &nnz) == 5);
        std::vector<int32_t> one{0, 0};
        EXPECT(ingest_check_offsets(one.data(), 1, &nnz) == -1 && nnz == 0);
    }
    {
        std::vector<int64_t> a{0, (int64_t)1 << 31, ((int64_t)1 << 32) + 3};
        EXPECT(ingest_check_offsets(a.data(), 2, &nnz) == -1 && nnz == ((int64_t)1 << 32) + 3);
        a[2] = ((int64_t)1 << 31) - 1;
        EXPECT(ingest_check_offsets(a.data(), 2, &nnz) == 2);
    }
    // ---- batch edges around 2^31 entries: no run may reach 2^31
    for (int64_t total : {I32MAX, I32MAX + 1, I32MAX + 2}) {
        // 1000 + a slice that straddles the edge + 7
        const std::vector<int64_t> len{1000, total - 1007, 7};
        const std::vector<int64_t> cut = edges(len, I32MAX);
        if (total == I32MAX) EXPECT((cut == std::vector<int64_t>{0, 3}));
        else EXPECT((cut == std::vector<int64_t>{0, 2, 3}));
        int64_t covered = 0;
        for (size_t b = 0; b + 1 < cut.size(); ++b) {
            int64_t sum = 0;
            for (int64_t s = cut[b]; s < cut[b + 1]; ++s) sum += len[(size_t)s];
            EXPECT(sum <= I32MAX && cut[b + 1] > cut[b]);
            covered += sum;
        }
        EXPECT(covered == total);
    }
    EXPECT((edges({}, I32MAX) == std::vector<int64_t>{0}));
    EXPECT((edges({I32MAX, I32MAX, 1}, I32MAX) == std::vector<int64_t>{0, 1, 2, 3}));
    EXPECT((edges({5, 9, 2}, 4) == std::vector<int64_t>{0, 1, 2, 3}));           // slices above the cap stand alone
    EXPECT((edges({0, 0, 4, 0, 1}, 4) == std::vector<int64_t>{0, 4, 5}));
    EXPECT((edges({INT64_MAX / 2, INT64_MAX / 2, INT64_MAX / 2}, INT64_MAX) == std::vector<int64_t>{0, 2, 3}));   // no overflow in the sum
    if (failures == 0) printf("ingest_host: ok\n");
    return failures == 0 ? 0 : 1;
}
