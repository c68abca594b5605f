// The sliced-row layout that ILU(0)'s factors (ilu0.hip) and every operator of the AMG hierarchy (amg.hip) are stored in, and
// the one row fold both apply them with.
//
// Positions come in slices of 64 (one wavefront): position p = 64 * slice + lane holds one row or nothing.  A slice is stored
// slice-column-major — entry e of the row at position p is slot sbase[p / 64] + e * 64 + p % 64 — so lane t of a wavefront
// reads entry e of its row next to its neighbours': every value and column load is one coalesced wavefront load.  A slice is
// as wide as its longest row; the slots a shorter row leaves hold column 0 and the value zero.  Row lengths are kept per
// position and those padded slots are SKIPPED, never multiplied (0 * inf and -0.0 would change bits).
//
// Which row sits at which position is the caller's: position = row (AMG, the Jacobi-sweep factors), or the rows of one
// dependency level after another with every level starting a new slice (the exact triangular solves).
//
// The host part below is plain C++17 on the standard library alone, so a host compiler can build and test it on its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sprs {

constexpr int SELL_SLICE = 64;           // positions per slice = lanes of a wavefront

template <class T>
struct SellPacked {
    std::vector<int32_t> len;            // per position, padded to whole slices: entries of its row (0: no row, or an empty one)
    std::vector<int64_t> sbase;          // per slice: its first slot
    std::vector<int32_t> col;            // per slot
    std::vector<T> val;
    int64_t slots = 0;
};

// Positions [0, npos): row_of(p) is the row at position p, or -1; row i's entries are the CSR positions [eb(i), ee(i)) of ci / v.
// each(p, i) is called once for every position p that holds a row i, in the pass that measures the rows: what a caller keeps
// per position beside the layout (ILU(0)'s pivots) rides along there instead of walking the positions again.
template <class T, class ROW, class EB, class EE, class EACH>
SellPacked<T> sell_pack(int64_t npos, ROW row_of, EB eb, EE ee, const int32_t *ci, const T *v, EACH each) {
    SellPacked<T> S;
    const size_t np = (size_t)npos, nslice = (np + SELL_SLICE - 1) / SELL_SLICE;
    S.len.assign(nslice * SELL_SLICE, 0);
    S.sbase.assign(nslice, 0);
    for (size_t s = 0; s < nslice; ++s) {
        int32_t width = 0;
        for (size_t p = s * SELL_SLICE; p < std::min((s + 1) * SELL_SLICE, np); ++p) {
            const int32_t i = row_of(p);
            if (i < 0) continue;
            S.len[p] = ee(i) - eb(i);
            each(p, i);
            width = std::max(width, S.len[p]);
        }
        S.sbase[s] = S.slots;
        S.slots += (int64_t)width * SELL_SLICE;
    }
    S.col.assign((size_t)S.slots, 0);
    S.val.assign((size_t)S.slots, T{});
    for (size_t p = 0; p < np; ++p) {
        if (!S.len[p]) continue;
        const size_t b = (size_t)eb(row_of(p)), d = (size_t)S.sbase[p / SELL_SLICE] + p % SELL_SLICE;
        for (size_t e = 0; e < (size_t)S.len[p]; ++e) { S.col[d + e * SELL_SLICE] = ci[b + e]; S.val[d + e * SELL_SLICE] = v[b + e]; }
    }
    return S;
}
template <class T, class ROW, class EB, class EE>
SellPacked<T> sell_pack(int64_t npos, ROW row_of, EB eb, EE ee, const int32_t *ci, const T *v) {
    return sell_pack<T>(npos, row_of, eb, ee, ci, v, [](size_t, int32_t) {});
}

}  // namespace sprs

// The device-facing part, for the HIP translation units of the library only (hipcc defines __HIPCC__ in both of its passes; a
// host compiler stops here).  It sits in an UNNAMED namespace on purpose: the kernels of ilu0.hip and amg.hip take SellDev by
// value and live in their files' unnamed namespaces, and a kernel's symbol spells out its parameter types — moving the view
// into `sprs` would rename every one of those kernels.  The price: each including file gets types of its own, so never pass a
// SellDev or a SellMat between translation units; hand over the four arrays instead.
#ifdef __HIPCC__
#include "internal.hpp"

namespace {

template <class T>
struct SellDev {
    const int32_t *len;                  // per position
    const int64_t *sbase;                // per slice
    const int32_t *col;
    const T *val;
};

struct SellMat {                         // type-erased owner of one packed layout's device arrays
    int32_t n = 0, nslice = 0;           // positions, slices
    int32_t *len = nullptr; int64_t *sbase = nullptr; int32_t *col = nullptr; void *val = nullptr;
    template <class T> bool upload(int64_t npos, const sprs::SellPacked<T> &S) {
        n = (int32_t)npos; nslice = (int32_t)S.sbase.size();
        T *dval = nullptr;
        const bool ok = sprs::dev_upload(&len, S.len.data(), S.len.size()) && sprs::dev_upload(&sbase, S.sbase.data(), S.sbase.size()) &&
                        sprs::dev_upload(&col, S.col.data(), S.col.size()) && sprs::dev_upload(&dval, S.val.data(), S.val.size());
        val = dval;
        return ok;
    }
    void release() {
        for (void *p : {(void *)len, (void *)sbase, (void *)col, val}) if (p) (void)hipFree(p);
        len = nullptr; sbase = nullptr; col = nullptr; val = nullptr;
    }
    template <class T> SellDev<T> dev() const { return SellDev<T>{len, sbase, col, (const T *)val}; }
};

// sigma = sum_e val_e x[col_e] over the entries of the row at position p, left to right from zero: the serial loop's bits
template <class T>
__device__ __forceinline__ T sell_fold(const SellDev<T> &M, int p, const T *x) {
    using namespace sprs;
    const int len = M.len[p];
    const int64_t b = M.sbase[p >> 6] + (p & (SELL_SLICE - 1));
    T sigma = szero<T>();
    int e = 0;
    for (; e + 4 <= len; e += 4) {                                   // four gathers in flight, folded in order
        int c[4]; T v[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { c[u] = M.col[b + (int64_t)(e + u) * SELL_SLICE]; v[u] = M.val[b + (int64_t)(e + u) * SELL_SLICE]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u) sigma = sadd(sigma, smul(v[u], xv[u]));
    }
    for (; e < len; ++e) sigma = sadd(sigma, smul(M.val[b + (int64_t)e * SELL_SLICE], x[M.col[b + (int64_t)e * SELL_SLICE]]));
    return sigma;
}

}  // namespace
#endif
