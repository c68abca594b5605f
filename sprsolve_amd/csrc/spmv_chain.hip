// Plane-streaming chains of the f64 PAIR-CODE stream (knob "spmv_chain"; profiles/r04_tuning.md §2, scripts/micro/fused_window.hip).
//
// The LDS x-window tiles (spmv_tile.hip) stage the NEAR columns of 4096 rows once and load the FAR windows — the +-plane
// neighbours of a 3-D stencil — row pair by row pair: (T + 2W) / T + 2 sixteen-byte loads per lane and 128 rows, and the far
// loads are served by an XCD's L2 only while what that XCD's workgroups hold in flight fits it (scripts/micro/fused_window.hip:
// the same kernel with two input vectors falls from 5.6 to 3 TB/s when it does not).  Here a workgroup owns a COLUMN of tiles —
// CH_ROWS rows at ts, ts + Pf, ts + 2 Pf, ... (Pf = the far offset; each tile within 127 rows of that on the 128-row block grid) —
// and keeps the windows of three consecutive tiles in LDS: the -Pf / +Pf operands of a tile are the centres of its neighbours'
// windows.  No far load exists; every element of x crosses the vector L1 (T + 2W) / T = 1.5 times instead of 3.25, independent of
// what survives in an L2; the loads of the window after next fly over the fold of the current tile.  A tile = CH_B consecutive
// FULL uniform 128-row blocks (plain or seam, mark_uniform_kernel) of the matrix's most frequent pattern, which must be
// far, near.., far with offsets -Pf .. +Pf, Pf even (build_chain_plan, spmv_dict.hip).  The fold per row is pair_fold
// (spmv_dict_dev.hpp), which spmv_tile_kernel calls too — the per-block kernel's products in the same left-to-right order, seam
// rows under scalar tests — with every operand taken from LDS: y bit-identical.  The 128-row blocks outside the chains (boundary planes, the blocks around boundary lines,
// remainders of runs) are walked by the same launch afterwards (pair2_walk), so a launch writes all of y and one dot partial per
// workgroup.
#include "spmv_dict_dev.hpp"
#include "bicg_fuse.hpp"

namespace sprs {
namespace {

constexpr int CH_ROWS = CH_B * 2 * WAVE;          // 2048 rows per tile
constexpr int CH_W = TILE_W;                      // half-width of a window: near = |col - row| <= CH_W - 2
constexpr int CH_WL = CH_ROWS + 2 * CH_W;         // 3072 doubles per window, three of them: 72 KiB — two workgroups per CU

// UX: the dot operand is the input vector itself (taken from the window).  TRI: the near slots are (.., c - 1, c, c + 1, ..)
// around an even centre offset and all other near offsets are even (every stencil with sorted columns on a grid of even line
// length): 16-byte LDS reads, the centre's pair serves the +-1 columns' inner halves.
// FUSE (bicgstab.hip, "fused SpMV input"): 0 = x is a vector in memory.  2 = x is BiCGStab's s = r + v * (-alpha) (K3 into K4:
// x = r, in1 = v), 3 = its p' = (v * (-beta w) + p * beta) + r (K1 into K2: x = v, in1 = p, in2 = r): `pro` is that update's kernel
// structure — its prologue (the scalars of the recurrence and its convergence / restart / breakdown decisions, taken identically by
// every workgroup from the same partials) runs at the top of this launch, the update itself while a window is staged, with the
// update's own rounding sequence; the updated vector is written for the launch's own rows to `own` and never read back.
// YST = false (K4 of BiCGStab's flow "bicg_k5" 1): y is not stored — the launch is its two dots.
// UPD (bicgstab.hip, knob "bicg_k5"): BiCGStab's K5 on the chains.  FUSE == 2 with `pro` = BicgK5: its prologue (status, alpha, w from K4's
// partials), s staged in the windows as K4 staged it, and per row pair the update of spmv_dict_dev.hpp's bicg_k5_row with t = A s
// either folded again here — the same fold over the same window contents: K4's bits — (UPD 1) or loaded from where K4 stored it (UPD 2,
// which skips the fold); x (pro.x) is updated in place, r' goes to `own`, the two sums to pro.partN / pro.partRho, one partial per
// workgroup, and BicgK5's epilogue writes the state.  x, p, r0 (and t) of a 128-row block are requested while the block before it is
// folded.
struct NoPro { __device__ __forceinline__ bool prologue() { return true; } };
template <int FUSE, class PRO, int DOT, bool UX, int UL, bool TRI, bool YST = true, int UPD = 0>
__global__ __launch_bounds__(BLOCK) void spmv_chain_kernel(const int4 *__restrict__ tiles, const int2 *__restrict__ segs, const int32_t *__restrict__ xstart,
                                                           const BlkDesc *__restrict__ desc, const TilePat pat,
                                                           int n_left, const int32_t *__restrict__ left_order,
                                                           const int32_t *__restrict__ row_ptr, const uint8_t *__restrict__ code,
                                                           const int32_t *__restrict__ off_tab, const double *__restrict__ val_tab,
                                                           const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ u,
                                                           double *__restrict__ part0, double *__restrict__ part1,
                                                           const int *__restrict__ status, int nrows, int ncols, const Fin fin,
                                                           PRO pro, const double *__restrict__ in1, const double *__restrict__ in2,
                                                           double *__restrict__ own) {
    using T = double;
    constexpr int NV = FUSE == 0 ? 1 : FUSE;            // input vectors
    static_assert(FUSE == 0 || (FUSE == 2 && DOT == 2 && UX && UPD == 0) || (FUSE == 3 && DOT == 1 && !UX) ||
                  (FUSE == 2 && DOT == 0 && !UX && !YST && UPD != 0), "fused flavours: K3 into K4, K1 into K2, K5 on the chains");
    static_assert((YST || FUSE == 2) && (UPD == 0 || FUSE == 2), "only BiCGStab's K4 / K5 drop the y store");
    constexpr int W = CH_W, WL = CH_WL;
    constexpr int NW = WL / 2 / BLOCK;                  // 16-byte window pieces per lane (6)
    constexpr int NQ = CH_B / NWAVE;                    // 128-row blocks per wavefront and tile (4)
    constexpr int NN = UL - 2;                          // near slots
    constexpr int TC = NN / 2;                          // TRI: the centre's position among the near slots
    static_assert(WL % (2 * BLOCK) == 0 && CH_B % NWAVE == 0 && NN >= 1 && UL <= 8 && (!TRI || (NN & 1)), "chain shape");
    static_assert(sizeof(T) * WL >= sizeof(uint32_t) * NWAVE * CW2, "the left walk's code slices live in the first window");
    __shared__ __attribute__((aligned(16))) T win[3][WL];
    __shared__ PairEnt<T> s_pair[TAB];
    __shared__ T red[NWAVE];
    const int run_state = status != nullptr ? *status : (int)ST_RUNNING;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    stage_pair(s_pair, tid, off_tab[tid] * 8, val_tab[tid]);                  // BLOCK == TAB (the seam rows' own values; the walk below)
    __syncthreads();
    if (run_state != ST_RUNNING) { fin_idle(fin, DOT == 2); return; }
    [[maybe_unused]] T c0 = 0.0, c1 = 0.0;              // coefficients of the fused update
    [[maybe_unused]] T nw = 0.0;                        // UPD: -w
    if constexpr (FUSE != 0) {
        if (!pro.prologue()) return;                    // converged / restart requested / breakdown: the same decision in every workgroup
        if constexpr (FUSE == 2) c0 = pro.na; else { c0 = pro.a; c1 = pro.beta; }
        if constexpr (UPD != 0) nw = pro.nw;
    }
    T d0 = 0.0, d1 = 0.0;

    const int Pf = pat.off[UL - 1];                     // == -pat.off[0]
    const int xhi = (ncols - 2) & ~1;                   // last (even) index a 16-byte load of x may start at
    const int xcd = blockIdx.x & 7;
    const int sstep = gridDim.x >> 3;
    const int send = xstart[xcd + 1];
    // PF windows are in flight while a tile is folded: the register sets R[0 .. PF).  Two for the plain kernel and K3-in-K4; K1-in-K2
    // holds three vectors per window and keeps one (a second set would spill); K5 keeps one too (a second fits, 239-247 VGPRs, and
    // measures the same: profiles/k5_chain.md §5).
    constexpr int PF = (FUSE == 3 || UPD != 0) ? 1 : 2;
    struct WinRegs { u4v a[NW]; u4v b[NV >= 2 ? NW : 1]; u4v c[NV == 3 ? NW : 1]; };
    WinRegs R0;
    [[maybe_unused]] WinRegs R1;
    // raw window of the tile that starts at row tw: [tw - W, tw + CH_ROWS + W).  The margins of a window at either end of x are
    // clamped piece by piece — what they hold is never folded (every column a tile's rows have is inside x)
    auto issue = [&](int tw, WinRegs &R) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            int g = tw - W + 2 * (tid + i * BLOCK);
            g = g < 0 ? 0 : (g > xhi ? xhi : g);
            R.a[i] = *reinterpret_cast<const u4v *>(x + g);              // (non-temporal window loads, allocating result stores: no difference, profiles/r04_tuning.md §3)
            if constexpr (NV >= 2) R.b[i] = *reinterpret_cast<const u4v *>(in1 + g);
            if constexpr (NV == 3) R.c[i] = *reinterpret_cast<const u4v *>(in2 + g);
        }
    };
    auto stage = [&](int slot, const WinRegs &R) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if constexpr (FUSE == 0) {
                *reinterpret_cast<u4v *>(&win[slot][2 * (tid + i * BLOCK)]) = R.a[i];
            } else {
                D2 a, b, cc{0.0, 0.0};
                __builtin_memcpy(&a, &R.a[i], 16); __builtin_memcpy(&b, &R.b[i], 16);
                if constexpr (NV == 3) __builtin_memcpy(&cc, &R.c[i], 16);
                const D2 o = FUSE == 2 ? D2{comb_k3(a.lo, b.lo, c0), comb_k3(a.hi, b.hi, c0)}
                                       : D2{comb_k1(a.lo, b.lo, cc.lo, c0, c1), comb_k1(a.hi, b.hi, cc.hi, c0, c1)};
                *reinterpret_cast<D2 *>(&win[slot][2 * (tid + i * BLOCK)]) = o;
            }
        }
    };
    for (int s = xstart[xcd] + (blockIdx.x >> 3); s < send; s += sstep) {
        const int2 sg = segs[s];
        const int t0 = __builtin_amdgcn_readfirstlane(sg.x), L = __builtin_amdgcn_readfirstlane(sg.y);
        int4 ent = tiles[t0];
        uint32_t rbw[NQ]; int nnw[NQ];                  // seam words of the tile's blocks (wave-uniform: scalar loads), a tile ahead
#pragma unroll
        for (int q = 0; q < NQ; ++q) { const BlkDesc d = desc[__builtin_amdgcn_readfirstlane(ent.x) + q * NWAVE + wv]; rbw[q] = (uint32_t)d.rb; nnw[q] = d.nn; }
        __syncthreads();                                // the previous segment's windows have been read
        int ts_prev = __builtin_amdgcn_readfirstlane(ent.y) - Pf;      // the segment's first tile takes its -Pf operands from the window at ts - Pf
        int sp = 0, sc = 1, sn = 2;                     // slots of the previous / current / next window
        issue(ts_prev, R0); stage(sp, R0);
        issue(__builtin_amdgcn_readfirstlane(ent.y), R0); stage(sc, R0);
        issue(__builtin_amdgcn_readfirstlane(ent.z), R0);                                        // tile 0's next window
        if constexpr (PF == 2) { if (L > 1) issue(tiles[t0 + 1].z, R1); }                       // tile 1's next window
        // one tile: stage its next window from RS (issued PF tiles ago), then refill RS with the next window of tile k + PF
        auto body = [&](int k, WinRegs &RS) {
            const int ts = __builtin_amdgcn_readfirstlane(ent.y), ts_next = __builtin_amdgcn_readfirstlane(ent.z);
            uint32_t rbc[NQ]; int nnc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) { rbc[q] = rbw[q]; nnc[q] = nnw[q]; }
            stage(sn, RS);                              // the next tile's window (its loads flew over the previous folds)
            __syncthreads();
            if (k + PF < L) issue(tiles[t0 + k + PF].z, RS);
            if (k + 1 < L) {
                ent = tiles[t0 + k + 1];
                const int b1 = __builtin_amdgcn_readfirstlane(ent.x);
#pragma unroll
                for (int q = 0; q < NQ; ++q) { const BlkDesc d = desc[b1 + q * NWAVE + wv]; rbw[q] = (uint32_t)d.rb; nnw[q] = d.nn; }
            }
            // x[r - Pf] sits in the previous window at (r - ts) + W + dlo, x[r + Pf] in the next one at (r - ts) + W + dhi
            const int dlo = ts - Pf - ts_prev, dhi = ts + Pf - ts_next;
            const T *wp = &win[sp][W + dlo], *wc = &win[sc][W], *wn = &win[sn][W + dhi];
            D2 uu[NQ];
            if (DOT != 0 && !UX) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const u4v w4 = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(u + (ts + ((q * NWAVE + wv) << 7) + 2 * lane)));
                    __builtin_memcpy(&uu[q], &w4, 16);
                }
            }
            // UPD: x, p, r0 (and the stored t) of the lane's two rows in block q
            struct UpdRegs { u4v x, p, q, t; };
            [[maybe_unused]] UpdRegs ur[2];
            [[maybe_unused]] auto upd_load = [&](int q, UpdRegs &U) {
                if constexpr (UPD != 0) {
                    const int g = ts + ((q * NWAVE + wv) << 7) + 2 * lane;
                    U.x = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(pro.x + g));
                    U.p = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(pro.y + g));
                    U.q = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(pro.r0 + g));
                    if constexpr (UPD == 2) U.t = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(pro.t + g));
                }
            };
            upd_load(0, ur[0]);
            // operands of block q + 1 are read before block q is folded (the seam branch keeps the compiler from doing it)
            T opl[UL], oph[UL], ux0 = 0.0, ux1 = 0.0;
            auto read_ops = [&](int q) {
                const int l = ((q * NWAVE + wv) << 7) + 2 * lane;
                const D2 f0 = *reinterpret_cast<const D2 *>(wp + l), f1 = *reinterpret_cast<const D2 *>(wn + l);
                opl[0] = f0.lo; oph[0] = f0.hi; opl[UL - 1] = f1.lo; oph[UL - 1] = f1.hi;
                if constexpr (TRI) {
#pragma unroll
                    for (int t = 0; t < NN; ++t) {
                        if (t == TC - 1 || t == TC + 1) continue;
                        const D2 v2 = *reinterpret_cast<const D2 *>(wc + l + pat.off[1 + t]);
                        opl[1 + t] = v2.lo; oph[1 + t] = v2.hi;
                    }
                    if constexpr (NN >= 3) {
                        const int oc = pat.off[1 + TC];
                        opl[TC] = wc[l + oc - 1]; oph[TC] = opl[1 + TC];                 // column c - 1: (x[r0 - 1 + c], x[r0 + c])
                        opl[2 + TC] = oph[1 + TC]; oph[2 + TC] = wc[l + oc + 2];         // column c + 1: (x[r0 + 1 + c], x[r0 + 2 + c])
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < NN; ++t) { opl[1 + t] = wc[l + pat.off[1 + t]]; oph[1 + t] = wc[l + pat.off[1 + t] + 1]; }
                }
                if ((DOT != 0 && UX) || FUSE != 0) { const D2 c2 = *reinterpret_cast<const D2 *>(wc + l); ux0 = c2.lo; ux1 = c2.hi; }
            };
            read_ops(0);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const uint32_t rbq = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbc[q]);
                T pl[UL], ph[UL];
#pragma unroll
                for (int t = 0; t < UL; ++t) { pl[t] = opl[t]; ph[t] = oph[t]; }
                const T u0 = (DOT != 0 && !UX) ? uu[q].lo : ux0, u1 = (DOT != 0 && !UX) ? uu[q].hi : ux1;
                [[maybe_unused]] const D2 mine{ux0, ux1};              // FUSE: the formed vector at the lane's own two rows
                if (q + 1 < NQ) { read_ops(q + 1); upd_load(q + 1, ur[(q + 1) & 1]); }
                T acc0 = 0.0, acc1 = 0.0;
                if constexpr (UPD == 2) {               // t as K4 stored it
                    D2 tt;
                    __builtin_memcpy(&tt, &ur[q & 1].t, 16);
                    acc0 = tt.lo; acc1 = tt.hi;
                } else {
                    pair_fold<UL>(pl, ph, pat.val, rbq, nnc[q], s_pair, lane, acc0, acc1);
                }
                row_pair_out<DOT, YST>(y + (ts + ((q * NWAVE + wv) << 7) + 2 * lane), acc0, acc1, u0, u1, d0, d1);
                if constexpr (UPD != 0) {
                    D2 xx, pp, qq, rr;
                    __builtin_memcpy(&xx, &ur[q & 1].x, 16); __builtin_memcpy(&pp, &ur[q & 1].p, 16); __builtin_memcpy(&qq, &ur[q & 1].q, 16);
                    bicg_k5_row(xx.lo, pp.lo, mine.lo, acc0, qq.lo, c0, nw, rr.lo, d0, d1);
                    bicg_k5_row(xx.hi, pp.hi, mine.hi, acc1, qq.hi, c0, nw, rr.hi, d0, d1);
                    const int g = ts + ((q * NWAVE + wv) << 7) + 2 * lane;
                    u4v xo, ro;
                    __builtin_memcpy(&xo, &xx, 16); __builtin_memcpy(&ro, &rr, 16);
                    __builtin_nontemporal_store(xo, reinterpret_cast<u4v *>(pro.x + g));
                    __builtin_nontemporal_store(ro, reinterpret_cast<u4v *>(own + g));
                }
                if constexpr (FUSE == 3) {          // (K3 in K4 stores nothing: K5 forms s again, bicg_fuse.hpp BicgK5<SV>)
                    u4v ov;
                    __builtin_memcpy(&ov, &mine, 16);
                    __builtin_nontemporal_store(ov, reinterpret_cast<u4v *>(own + (ts + ((q * NWAVE + wv) << 7) + 2 * lane)));
                }
            }
            __syncthreads();                            // the previous window's slot is free for the window after next
            ts_prev = ts;
            const int o = sp; sp = sc; sc = sn; sn = o;
        };
        if constexpr (PF == 2) {
            for (int k = 0; k < L; k += 2) { body(k, R0); if (k + 1 < L) body(k + 1, R1); }
        } else {
            for (int k = 0; k < L; ++k) body(k, R0);
        }
    }
    if (n_left > 0) {
        __syncthreads();
        uint32_t (*s_c)[CW2] = reinterpret_cast<uint32_t (*)[CW2]>(&win[0][0]);
        for (int i = lane; i < CW2; i += WAVE) s_c[wv][i] = 0;                 // (wavefront-private slices: no barrier)
        if constexpr (FUSE == 0)
            pair2_walk<DOT, true>(n_left, 0, desc, left_order, row_ptr, code, XPlain{reinterpret_cast<const char *>(x)}, y, u, nrows, ncols, s_pair, s_c, d0, d1);
        else if constexpr (UPD != 0)
            pair2_walk<0, true, XFused<2>, false, BicgUpd<UPD>>(n_left, 0, desc, left_order, row_ptr, code,
                                                                XFused<2>{reinterpret_cast<const char *>(x), reinterpret_cast<const char *>(in1), nullptr, c0, c1},
                                                                nullptr, nullptr, nrows, ncols, s_pair, s_c, d0, d1, nullptr,
                                                                BicgUpd<UPD>{pro.x, pro.y, pro.r0, pro.t, own, c0, nw});
        else if constexpr (!YST)
            pair2_walk<DOT, true, XFused<NV>, false>(n_left, 0, desc, left_order, row_ptr, code,
                                                     XFused<NV>{reinterpret_cast<const char *>(x), reinterpret_cast<const char *>(in1), reinterpret_cast<const char *>(in2), c0, c1},
                                                     nullptr, UX ? nullptr : u, nrows, ncols, s_pair, s_c, d0, d1, own);
        else
            pair2_walk<DOT, true, XFused<NV>>(n_left, 0, desc, left_order, row_ptr, code,
                                              XFused<NV>{reinterpret_cast<const char *>(x), reinterpret_cast<const char *>(in1), reinterpret_cast<const char *>(in2), c0, c1},
                                              y, UX ? nullptr : u, nrows, ncols, s_pair, s_c, d0, d1, own);
    }
    spmv_dot_epilogue<DOT>(d0, d1, red, part0, part1, fin);
    if constexpr (UPD != 0) {
        pro.accN = d0; pro.accR = d1;
        pro.epilogue();
    }
}

}  // namespace

int chain_rows() { return CH_ROWS; }

// One launch of the chain kernel: the plan's and the pair stream's arguments, which every flavour takes alike, then the flavour's.
// kern(integral_constant UL, bool_constant TRI): the flavour's kernel for the plan's shape.
template <class Kern, class PRO>
int launch_chain(const sprs_csr *A, const SpmvRoute &rt, Kern kern, const double *x, double *y, const double *u, double *part0, double *part1,
                 const int *status, const Fin &fin, const PRO &pro, const double *in1, const double *in2, double *own) {
    sprs_ctx *c = A->ctx;
    const sprs_dict *D = A->dict;
    const sprs_chain_plan &CP = *rt.chain;
    const TilePat tp = tile_pat(CP);
#define SPRS_CSHAPE(U, TR)                                                                                                                 \
    if (CP.ul == U && (CP.tri != 0) == TR)                                                                                                 \
        SPRS_LAUNCH_SPMV(c, kern(std::integral_constant<int, U>{}, std::bool_constant<TR>{}), rt.grid, reinterpret_cast<const int4 *>(CP.tiles), \
                         reinterpret_cast<const int2 *>(CP.segs), CP.xstart, rt.desc, tp, CP.n_left, CP.left, A->row_ptr, D->pair_code, D->pair_off, \
                         reinterpret_cast<const double *>(D->pair_val), x, y, u, part0, part1, status, (int)A->nrows, (int)A->ncols, fin, pro, in1, in2, own);
    SPRS_CHAIN_SHAPES(SPRS_CSHAPE)
#undef SPRS_CSHAPE
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

int launch_chain_pair(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                      double *part0, double *part1, const int *status, const Fin &fin) {
    int rc = SPRS_OK;
    // UX: the dot operand is the input vector; without a dot, one kernel
    with_dot(dot_mode, u == x, [&](auto dm, auto ux) {
        constexpr int DM = decltype(dm)::value;
        constexpr bool UXV = DM != 0 && decltype(ux)::value;
        rc = launch_chain(A, r, [](auto ul, auto tri) { return &spmv_chain_kernel<0, NoPro, DM, UXV, decltype(ul)::value, decltype(tri)::value>; },
                          x, y, u, part0, part1, status, fin, NoPro{}, nullptr, nullptr, nullptr);
    });
    return rc;
}

int launch_chain_k4f(const sprs_csr *A, const SpmvRoute &rt, const BicgK3<double, double, false> &pro, const double *r, const double *v, double *s_out,
                     double *t, double *partTT, double *partTR, const int *status, bool store_t) {
    typedef BicgK3<double, double, false> K3;
    auto go = [&](auto yst) {
        return launch_chain(A, rt, [](auto ul, auto tri) { return &spmv_chain_kernel<2, K3, 2, true, decltype(ul)::value, decltype(tri)::value, decltype(yst)::value>; },
                            r, t, nullptr, partTT, partTR, status, Fin{}, pro, v, nullptr, s_out);
    };
    return store_t ? go(std::true_type{}) : go(std::false_type{});
}

int launch_chain_k5(const sprs_csr *A, const SpmvRoute &rt, const BicgK5<double, false, true> &pro, double *r_out, bool recompute) {
    typedef BicgK5<double, false, true> K5;
    auto go = [&](auto upd) {
        return launch_chain(A, rt, [](auto ul, auto tri) { return &spmv_chain_kernel<2, K5, 0, false, decltype(ul)::value, decltype(tri)::value, false, decltype(upd)::value>; },
                            pro.r, nullptr, nullptr, nullptr, nullptr, &pro.S->status, Fin{}, pro, pro.sv, nullptr, r_out);
    };
    return recompute ? go(std::integral_constant<int, 1>{}) : go(std::integral_constant<int, 2>{});
}

int launch_chain_k2f(const sprs_csr *A, const SpmvRoute &rt, const BicgK1<double, double, false> &pro, const double *v_old, const double *p, const double *r,
                     double *p_out, double *v_out, const double *r0, double *partB, const int *status) {
    typedef BicgK1<double, double, false> K1;
    return launch_chain(A, rt, [](auto ul, auto tri) { return &spmv_chain_kernel<3, K1, 1, false, decltype(ul)::value, decltype(tri)::value>; },
                        v_old, v_out, r0, partB, nullptr, status, Fin{}, pro, p, r, p_out);
}

}  // namespace sprs
