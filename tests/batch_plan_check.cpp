// The plan of the on-chip batch solvers (csrc/batch_plan.hpp) against the numbers the header states, restated here: a stand-alone
// program on the header alone, built by tests/test_batch_plan_cpu.py with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>

#include "batch_plan.hpp"

using namespace sprs;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    // B(n) = min(256, 64 ceil(n / 64)), 64 for n = 0
    const long ns[] = {0, 1, 64, 65, 128, 129, 256, 257, 1024};
    const int want[] = {64, 64, 64, 128, 128, 192, 256, 256, 256};
    for (int k = 0; k < 9; ++k) CHECK(batch_threads(ns[k]) == want[k]);
    for (long n = 0; n <= 5000; ++n) {
        const int b = batch_threads(n);
        CHECK(b % 64 == 0 && b >= 64 && b <= 256);
        CHECK(n == 0 || b == 256 || (b >= n && b - 64 < n));                 // below 256: the fewest whole wavefronts that hold n
    }
    // the vectors, the LDS bytes and the caps: all four scalar types (dtype codes 0 f64, 1 c64, 2 f32, 3 c32), both solvers
    const long bytes[] = {8, 16, 4, 8};
    const long cap_bicg[] = {1024, 512, 2048, 1024}, cap_cg[] = {1600, 768, 3264, 1600};
    CHECK(batch_vectors(BATCH_BICGSTAB) == 8 && batch_vectors(BATCH_CG) == 5 && batch_vectors(2) == 0);
    CHECK(BATCH_SCRATCH == 128 && BATCH_SCRATCH % 16 == 0 && BATCH_LDS_BUDGET == 64 * 1024);
    for (int dt = 0; dt < 4; ++dt) {
        CHECK(batch_scalar_bytes(dt) == bytes[dt]);
        for (int solver = 0; solver < 2; ++solver) {
            const long nv = solver == BATCH_BICGSTAB ? 8 : 5;
            const long cap = (long)batch_max_rows(solver, bytes[dt]);
            CHECK(cap == (solver == BATCH_BICGSTAB ? cap_bicg[dt] : cap_cg[dt]));
            CHECK(cap % 64 == 0 && cap > 0);
            CHECK(batch_vector_bytes(solver, bytes[dt], cap) == nv * bytes[dt] * cap);
            CHECK(batch_vector_bytes(solver, bytes[dt], cap) <= 64 * 1024);          // the cap fits the budget ...
            CHECK(batch_vector_bytes(solver, bytes[dt], cap + 64) > 64 * 1024);      // ... and the next multiple of 64 does not
            const long sizes[] = {0, 1, 30, 64, 65, 300, cap};
            for (long n : sizes) {
                CHECK(batch_lds_bytes(solver, bytes[dt], n) == 128 + nv * bytes[dt] * n);
                CHECK((batch_lds_bytes(solver, bytes[dt], n) - 128) % bytes[dt] == 0);
                CHECK(batch_lds_bytes(solver, bytes[dt], n) <= 160 * 1024 / 2);      // at least two workgroups a CU
            }
        }
    }
    CHECK(batch_scalar_bytes(4) == 0 && batch_scalar_bytes(-1) == 0);
    CHECK(batch_max_rows(2, 8) == -1 && batch_max_rows(BATCH_CG, 0) == -1);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("batch plan ok\n");
    return 0;
}
