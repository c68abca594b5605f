// The wave-packed layout that the block-Jacobi preconditioner (bjacobi.hip) keeps its inverse blocks in, and the plan that
// places the blocks.
//
// Positions come in slices of 64 (one wavefront): position p = 64 * slice + lane holds one ROW of one block, or nothing.  A
// slice holds whole consecutive blocks in natural row order — the rows of a slice are srow[slice] .. srow[slice] + scnt[slice]
// - 1, one per lane from lane 0 — and a block never straddles two slices: a block that does not fit what is left of a slice
// starts the next one, and the lanes it leaves behind hold nothing.  Entry (i, j) of the block whose row i sits at lane l is
// slot sbase[slice] + j * 64 + l, so lane l of a wavefront reads entry j of its row next to its neighbours': every matrix load
// is one coalesced wavefront load.  A slice is as wide as its largest block; the slots a smaller block leaves are padding that is
// SKIPPED, never multiplied.  Per position: code[p] = (the lane of the block's first row) | (the block's size m << 8), 0 where
// the lane holds nothing (m >= 1 otherwise).
//
// The host part below is plain C++17 on the standard library alone, so a host compiler can build and test it on its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sprs {

constexpr int BJ_SLICE = 64;             // positions per slice = lanes of a wavefront
constexpr int BJ_MAX_BLOCK = 32;         // = SPRS_BJACOBI_MAX_BLOCK

struct BjacobiPlan {
    int64_t n = 0, nblocks = 0, max_block = 0, slots = 0;
    bool fits = true;                    // every position is below 2^31 (bpos and the kernels index positions with 32 bits); else nothing below bpos is valid
    std::vector<int64_t> block_ptr;      // nblocks + 1
    std::vector<int32_t> srow, scnt;     // per slice: its first row and its rows
    std::vector<int64_t> sbase;          // per slice: its first slot
    std::vector<uint16_t> code;          // per position, padded to whole slices
    std::vector<int32_t> bpos;           // per block: the position of its first row
    int64_t nslice() const { return (int64_t)srow.size(); }
    // slot of entry (i, j) of block b
    int64_t slot(int64_t b, int i, int j) const {
        const int64_t p = (int64_t)bpos[(size_t)b] + i;
        return sbase[(size_t)(p / BJ_SLICE)] + (int64_t)j * BJ_SLICE + p % BJ_SLICE;
    }
};

// block_size > 0: the uniform blocks 0, bs, 2 bs, .., n (a ragged last block); else the nblocks + 1 entries of block_ptr.
// -> 0, or what is wrong: 1 block_ptr does not start at 0, 2 it does not increase strictly (*at = the block), 3 it does not end
// at n, 4 a block has more than BJ_MAX_BLOCK rows (*at = the block).  The caller has checked that exactly one of the two is given.
inline int bjacobi_block_ptr(int64_t n, int64_t block_size, const int64_t *block_ptr, int64_t nblocks, std::vector<int64_t> &bp, int64_t *at) {
    *at = -1;
    bp.clear();
    if (block_size > 0) {
        if (block_size > BJ_MAX_BLOCK) { *at = 0; return 4; }
        for (int64_t s = 0; s < n; s += block_size) bp.push_back(s);
        bp.push_back(n);
        return 0;
    }
    if (nblocks < 0 || block_ptr[0] != 0) return 1;
    for (int64_t b = 0; b < nblocks; ++b)
        if (block_ptr[b + 1] <= block_ptr[b]) { *at = b; return 2; }
    if (block_ptr[nblocks] != n) return 3;
    for (int64_t b = 0; b < nblocks; ++b)
        if (block_ptr[b + 1] - block_ptr[b] > BJ_MAX_BLOCK) { *at = b; return 4; }
    bp.assign(block_ptr, block_ptr + nblocks + 1);
    return 0;
}

// The layout of the blocks bp (checked: 0 = bp[0] < bp[1] < .. = n, each block of 1 .. BJ_MAX_BLOCK rows).
inline BjacobiPlan bjacobi_plan(const std::vector<int64_t> &bp) {
    BjacobiPlan P;
    P.block_ptr = bp;
    P.nblocks = (int64_t)bp.size() - 1;
    P.n = bp.back();
    P.bpos.resize((size_t)P.nblocks);
    std::vector<int32_t> width;
    int used = BJ_SLICE;                 // lanes taken in the current slice (none yet: the first block opens one)
    for (int64_t b = 0; b < P.nblocks; ++b) {
        const int m = (int)(bp[(size_t)b + 1] - bp[(size_t)b]);
        if (used + m > BJ_SLICE) {
            P.srow.push_back((int32_t)bp[(size_t)b]); P.scnt.push_back(0); width.push_back(0);
            used = 0;
        }
        const size_t s = P.srow.size() - 1;
        const int64_t pos = (int64_t)s * BJ_SLICE + used;
        if (pos + m > INT32_MAX) { P.fits = false; return P; }
        P.bpos[(size_t)b] = (int32_t)pos;
        P.scnt[s] += m; width[s] = std::max<int32_t>(width[s], m);
        used += m;
        P.max_block = std::max<int64_t>(P.max_block, m);
    }
    P.sbase.resize(P.srow.size());
    for (size_t s = 0; s < P.srow.size(); ++s) { P.sbase[s] = P.slots; P.slots += (int64_t)width[s] * BJ_SLICE; }
    P.code.assign(P.srow.size() * BJ_SLICE, 0);
    for (int64_t b = 0; b < P.nblocks; ++b) {
        const int m = (int)(bp[(size_t)b + 1] - bp[(size_t)b]), first = P.bpos[(size_t)b] % BJ_SLICE;
        for (int i = 0; i < m; ++i) P.code[(size_t)P.bpos[(size_t)b] + i] = (uint16_t)(first | (m << 8));
    }
    return P;
}

}  // namespace sprs

// The device-facing part, for bjacobi.hip only (hipcc defines __HIPCC__ in both of its passes; a host compiler stops here).  As in
// sell.hpp it sits in an unnamed namespace: the kernels take the view by value and live in their file's unnamed namespace.
#ifdef __HIPCC__
namespace {

template <class T>
struct BjacobiDev {
    const int32_t *srow, *scnt;          // per slice
    const int64_t *sbase;                // per slice
    const uint16_t *code;                // per position
    const T *minv;                       // per slot
};

}  // namespace
#endif
