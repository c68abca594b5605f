// The one grid walk of every fused recurrence kernel, and the small host helpers of the solvers' translation units.  A kernel
// is a functor F: prologue() (re-reduce the producer's partials, the scalar logic; false = this launch has nothing to do),
// run<PK, NT>(i) (pack i of the vectors) and epilogue() (hand this workgroup's partials over).
#pragma once
#include "device.hpp"

namespace sprs {

__device__ __forceinline__ bool first_thread() { return blockIdx.x == 0 && threadIdx.x == 0; }

// A functor whose n is always a whole number of packs says `static constexpr bool whole_packs = true;`: the kernel then has no
// scalar tail (run<1, NT> is not even instantiated).
template <class F, class = void> struct whole_packs : std::false_type {};
template <class F> struct whole_packs<F, std::enable_if_t<F::whole_packs>> : std::true_type {};

// ======================================================================= fused kernel skeleton
// NT: the vector operands are read and the results written with non-temporal accesses.  At HBM sizes every vector is
// streamed once per pass and evicted long before its next use; accesses that do not allocate on the way leave the caches
// to the SpMV's gathers and run faster in the read/write mix (profiles/r02_tuning.md §20).  Vectors that live in the
// Infinity Cache lose with it.
template <int PK, bool NT, class F>
__global__ __launch_bounds__(BLOCK) void fused_kernel(int64_t n, F f, int chunked) {
    if (!f.prologue()) return;
    if (chunked) {
        // one contiguous eighth of the vectors per XCD (workgroup id mod 8), the same eighth in every kernel and the one
        // whose rows that XCD multiplies in the SpMV (xcd_chunk): what a kernel writes is read from the same L2
        const int64_t np = n / PK, chunk = ((np + 7) / 8 + BLOCK - 1) / BLOCK * BLOCK;
        const int xcd = blockIdx.x & 7;
        const int64_t end = min(np, (int64_t)(xcd + 1) * chunk), st = (int64_t)(gridDim.x >> 3) * BLOCK;
        for (int64_t i = xcd * chunk + (int64_t)(blockIdx.x >> 3) * BLOCK + threadIdx.x; i < end; i += st) f.template run<PK, NT>(i);
    } else {
        SPRS_FOREACH_PACK(n, PK, i) f.template run<PK, NT>(i);
    }
    if constexpr (PK > 1 && !whole_packs<F>::value) {
        int64_t i = (n / PK) * PK + (int64_t)blockIdx.x * BLOCK + threadIdx.x;
        if (i < n) f.template run<1, NT>(i);
    }
    f.epilogue();
}

template <class T, class F>
static int launch_fused(sprs_ctx *c, size_t n, int grid, int chunked_walk, F f) {
    constexpr int PKW = pack_width<T>::value;
    const int chunked = (chunked_walk && grid % 8 == 0 && grid >= 8) ? 1 : 0;
    if (stream_loads_nt(c, n * sizeof(T)))
        hipLaunchKernelGGL((fused_kernel<PKW, true, F>), dim3(grid), dim3(BLOCK), 0, c->stream, (int64_t)n, f, chunked);
    else
        hipLaunchKernelGGL((fused_kernel<PKW, false, F>), dim3(grid), dim3(BLOCK), 0, c->stream, (int64_t)n, f, chunked);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

// A solver's scalar kernel: one workgroup of BLOCK threads on the context's stream, lds_bytes of dynamic LDS.
template <class K, class... Args>
static int launch_small(sprs_ctx *c, K kernel, size_t lds_bytes, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(BLOCK), lds_bytes, c->stream, args...);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

// a run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{})
template <class F>
static int dispatch_bool(bool flag, F &&f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }

// small helpers on the context stream
template <class T>
static int dcopy(sprs_ctx *c, T *dst, const T *src, size_t n) {
    SPRS_HIP_TRY(c, hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToDevice, c->stream));
    return SPRS_OK;
}
template <class T>
static int dzero(sprs_ctx *c, T *dst, size_t n) {
    SPRS_HIP_TRY(c, hipMemsetAsync(dst, 0, sizeof(T) * n, c->stream));
    return SPRS_OK;
}

}  // namespace sprs
