// The plan of the on-chip batch solvers (batch.hip): how many threads work one system, how much LDS a workgroup asks for,
// and how many rows a solver takes.  It is part of the arithmetic statement in the header (sprs_batch_*): the bits of a sum over
// rows depend on B(n), so the header, this file and the tests' reference (tests/_batch_ref.py) state the same numbers.
//
//  * Threads per workgroup: B(n) = min(256, 64 * ceil(n / 64)), and 64 for n = 0 — whole wavefronts, one row per thread up to
//    256 rows, then rows t, t + B, .. per thread.
//  * LDS per workgroup: NV vectors of n scalars — CG 5 (x, r, z, p, q), BiCGStab 8 (x, r, r0, y, p, v, t, z) — behind
//    BATCH_SCRATCH bytes of reduction scratch: two rows of one 16-byte cell per wavefront (a pair of sums shares its barriers).
//    The scratch comes first, so that every vector starts on a multiple of 16 bytes plus a multiple of sizeof(T): each scalar
//    keeps its natural alignment.
//  * Row cap: the vectors of one workgroup take at most BATCH_LDS_BUDGET = 64 KiB (two workgroups and more per CU of 160 KiB):
//    max_rows = floor(65536 / (NV * sizeof(T))) rounded down to a multiple of 64.
//
// Plain C++17 on the standard library alone, so a host compiler can build and test it on its own.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sprs {

constexpr int BATCH_WAVE = 64;
constexpr int BATCH_MAX_THREADS = 256;
constexpr int64_t BATCH_LDS_BUDGET = 65536;
constexpr int64_t BATCH_SCRATCH = 2 * (BATCH_MAX_THREADS / BATCH_WAVE) * 16;     // 128 bytes

enum : int { BATCH_BICGSTAB = 0, BATCH_CG = 1 };     // = SPRS_BATCH_BICGSTAB / SPRS_BATCH_CG

// vectors of n a solver keeps in LDS; 0 for an unknown solver
constexpr int batch_vectors(int solver) { return solver == BATCH_BICGSTAB ? 8 : solver == BATCH_CG ? 5 : 0; }

// sizeof(T) of the handles' dtype codes (0 f64, 1 c64, 2 f32, 3 c32); 0 for an unknown code
constexpr int64_t batch_scalar_bytes(int dtype) { return dtype == 0 ? 8 : dtype == 1 ? 16 : dtype == 2 ? 4 : dtype == 3 ? 8 : 0; }

constexpr int batch_threads(int64_t n) {
    if (n <= 0) return BATCH_WAVE;
    const int64_t b = (n + BATCH_WAVE - 1) / BATCH_WAVE * BATCH_WAVE;
    return (int)(b < BATCH_MAX_THREADS ? b : BATCH_MAX_THREADS);
}

// bytes of the vectors alone (what the budget bounds), and of the whole dynamic LDS request
constexpr int64_t batch_vector_bytes(int solver, int64_t scalar_bytes, int64_t n) { return (int64_t)batch_vectors(solver) * scalar_bytes * n; }
constexpr int64_t batch_lds_bytes(int solver, int64_t scalar_bytes, int64_t n) { return BATCH_SCRATCH + batch_vector_bytes(solver, scalar_bytes, n); }

// -1 for an unknown solver or scalar size
constexpr int64_t batch_max_rows(int solver, int64_t scalar_bytes) {
    if (batch_vectors(solver) == 0 || scalar_bytes <= 0) return -1;
    return BATCH_LDS_BUDGET / (batch_vectors(solver) * scalar_bytes) / BATCH_WAVE * BATCH_WAVE;
}

}  // namespace sprs
