// LDS x-window tiles of the f64 OFFSET-CODE stream (a value per entry; design notes and the tile steps shared with spmv_tile.hip in spmv_dict_dev.hpp, profiles/r03_tuning.md §9).
#include "spmv_dict_dev.hpp"

namespace sprs {
namespace {

// The same tiles for the OFFSET-CODE stream (a value per entry: any stencil or band with variable coefficients).  The 128-row
// descriptors are the offset stream's own (owide_desc: uniform and seam blocks marked on the offset codes).  A full block's
// 128 UL values are consecutive in val[]: the wavefront loads them with 16-byte loads (stream order), passes them through its
// LDS slice one block ahead of the fold and reads them back by row — lane l's rows 2l, 2l + 1 sit at entries (2l) UL and
// (2l + 1) UL behind the block's first one; in a seam block the rows behind the short ones move up by what those lack, and a
// short row steps through its values only on the slots it has.  x as in spmv_tile_kernel.  The 64-row blocks outside the tiles
// go through dict_walk in the same launch.
template <int DOT, bool UX, int UL, int FL, int FH>
__global__ __launch_bounds__(BLOCK) void spmv_tile_off_kernel(const int2 *__restrict__ tile_list, const int32_t *__restrict__ xstart,
                                                              const BlkDesc *__restrict__ desc, const TilePat pat,
                                                              int n_left, const int32_t *__restrict__ left_order, const BlkDesc *__restrict__ desc64,
                                                              const int32_t *__restrict__ row_ptr, const uint8_t *__restrict__ code,
                                                              const int32_t *__restrict__ off_tab, const double *__restrict__ val,
                                                              const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ u,
                                                              double *__restrict__ part0, double *__restrict__ part1,
                                                              const int *__restrict__ status, const Fin fin, const V2d *__restrict__ tail2, int g2_last) {
    using T = double;
    constexpr int TR = TILE_ROWS, W = TILE_W;
    constexpr int NW = (TR + 2 * W) / 2 / BLOCK;        // 16-byte window pieces per lane
    constexpr int NQ = TILE_B / NWAVE;                  // 128-row blocks per wavefront and tile
    constexpr int NN = UL - FL - FH;                    // near slots
    constexpr int VROW = 2 * WAVE * UL;                 // values of a full block
    constexpr int NV = (VROW / 2 + 1 + WAVE - 1) / WAVE;   // 16-byte value loads per lane and block (a block may start on an odd entry)
    constexpr int CAPD = nnz_cap<T>::value;
    constexpr int CWD = (CAPD + 3 + CPAD + 3) / 4;
    constexpr int VS = (VROW + 2 + 15) / 16 * 16 > CAPD + 16 ? (VROW + 2 + 15) / 16 * 16 : CAPD + 16;    // slice stride: the tile phase's block, or dict_walk's
    static_assert((TR + 2 * W) % (2 * BLOCK) == 0 && TILE_B % NWAVE == 0 && NN >= 1 && UL <= 8, "tile shape");
    __shared__ __attribute__((aligned(16))) T win[TR + 2 * W];
    __shared__ __attribute__((aligned(16))) T vsl[NWAVE][VS];
    __shared__ int32_t s_off8[TAB];
    __shared__ uint32_t s_c[NWAVE][CWD];
    __shared__ T red[NWAVE];
    const int run_state = status != nullptr ? *status : (int)ST_RUNNING;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    s_off8[tid] = off_tab[tid] * (int32_t)sizeof(T);                            // BLOCK == TAB
    for (int i = lane; i < CWD; i += WAVE) s_c[wv][i] = 0;
    for (int i = lane; i < VS; i += WAVE) vsl[wv][i] = 0.0;
    __syncthreads();
    if (run_state != ST_RUNNING) { fin_idle(fin, DOT == 2); return; }
    T d0 = 0.0, d1 = 0.0;

    TileCursor cur = tile_cursor(tile_list, xstart);
    // per block its seam words and its first entry: scalar loads a tile ahead
    uint32_t rbw[NQ]; int nnw[NQ], vbw[NQ];
    auto load_words = [&](int b0, int ts) {
        tile_seam_words(desc, b0, wv, rbw, nnw);
#pragma unroll
        for (int q = 0; q < NQ; ++q) vbw[q] = row_ptr[ts + ((q * NWAVE + wv) << 7)];
    };
    load_words(__builtin_amdgcn_readfirstlane(cur.ent.x), __builtin_amdgcn_readfirstlane(cur.ent.y));
    T *vs = vsl[wv];
    for (; cur.s < cur.send; cur.s += cur.sstep) {
        const int ts = tile_cursor_take(cur, tile_list);
        uint32_t rbc[NQ]; int nnc[NQ], vbc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { rbc[q] = rbw[q]; nnc[q] = nnw[q]; vbc[q] = __builtin_amdgcn_readfirstlane(vbw[q]); }
        // ---- loads: the window, the far pairs (and dot operands) of the lane's NQ row pairs, the first block's values, then the
        // next tile's words
        u4v wreg[NW];
        window_load(x + (ts - W), tid, wreg);
        D2 far[NQ][FL + FH > 0 ? FL + FH : 1];
        D2 uu[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) tile_far_loads<DOT, UX, UL, FL, FH>(x, u, pat, ts + ((q * NWAVE + wv) << 7) + 2 * lane, far[q], uu[q]);
        u4v vreg[NV];
        auto load_vals = [&](int vb) {                  // chunks [vb >> 1, (vb >> 1) + VROW / 2]: the block's values from its 16-byte boundary
            const u4v *v2 = reinterpret_cast<const u4v *>(val) + (vb >> 1);
#pragma unroll
            for (int i = 0; i < NV; ++i) vreg[i] = __builtin_nontemporal_load(v2 + min(lane + i * WAVE, VROW / 2));      // read once: 720 -> 674 us (profiles/r03_tuning.md §9)
        };
        load_vals(vbc[0]);
        if (cur.s + cur.sstep < cur.send) load_words(__builtin_amdgcn_readfirstlane(cur.ent.x), __builtin_amdgcn_readfirstlane(cur.ent.y));
        window_stage(win, tid, wreg);
        T npl[NN], nph[NN];                             // the near reads of block q + 1 go out before block q is folded (spmv_tile_kernel)
        tile_read_near(win, W + (wv << 7) + 2 * lane, pat.off + FL, npl, nph);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            // this block's values: registers -> the wavefront's slice (stream order), then the next block's loads go out
#pragma unroll
            for (int i = 0; i < NV; ++i) *reinterpret_cast<u4v *>(&vs[2 * min(lane + i * WAVE, VROW / 2)]) = vreg[i];
            if (q + 1 < NQ) load_vals(vbc[q + 1 < NQ ? q + 1 : q]);
            wave_lds_fence();
            const uint32_t rbq = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbc[q]);
            const bool seam = (rbq & SEAM2) != 0;
            const int shift = vbc[q] & 1;
            const int li = W + ((q * NWAVE + wv) << 7) + 2 * lane;              // window index of x[r0]
            T pl[UL], ph[UL];
            tile_slots<UL, FL, FH>(far[q], npl, nph, pl, ph);
            T ux0 = 0.0, ux1 = 0.0;
            if (DOT != 0 && UX) { ux0 = win[li]; ux1 = win[li + 1]; }
            if (q + 1 < NQ) tile_read_near(win, W + (((q + 1) * NWAVE + wv) << 7) + 2 * lane, pat.off + FL, npl, nph);
            T acc0 = 0.0, acc1 = 0.0;
            if (!seam) {
                const T *v0 = vs + shift + 2 * lane * UL;
#pragma unroll
                for (int t = 0; t < UL; ++t) {
                    acc0 = acc0 + pl[t] * v0[t];
                    acc1 = acc1 + ph[t] * v0[UL + t];
                }
            } else {
                // rows k, k + 1 (local) hold only the slots of their masks: their values are fewer, and the rows behind them
                // start that much earlier in the slice
                const int seam1 = __builtin_amdgcn_readfirstlane(nnc[q]) >> 16, seam2 = (int)(rbq & 0x3ffffffu);
                const int k = seam1 & 127, full = (1 << UL) - 1, maskA = (seam1 >> 7) & full, maskB = seam2 & full;
                const int cA = UL - __builtin_popcount(maskA), cB = UL - __builtin_popcount(maskB);
                const int i0 = 2 * lane, i1 = i0 + 1;
                int p0 = shift + i0 * UL - (i0 > k ? cA : 0) - (i0 > k + 1 ? cB : 0);
                int p1 = shift + i1 * UL - (i1 > k ? cA : 0) - (i1 > k + 1 ? cB : 0);
                const int pm0 = i0 == k ? maskA : (i0 == k + 1 ? maskB : full), pm1 = i1 == k ? maskA : (i1 == k + 1 ? maskB : full);
#pragma unroll
                for (int t = 0; t < UL; ++t) {
                    const T n0 = acc0 + pl[t] * vs[p0], n1 = acc1 + ph[t] * vs[p1];
                    const bool h0 = ((pm0 >> t) & 1) != 0, h1 = ((pm1 >> t) & 1) != 0;
                    acc0 = h0 ? n0 : acc0; p0 += h0 ? 1 : 0;
                    acc1 = h1 ? n1 : acc1; p1 += h1 ? 1 : 0;
                }
            }
            row_pair_out<DOT>(y + (ts + ((q * NWAVE + wv) << 7) + 2 * lane), acc0, acc1, (DOT != 0 && !UX) ? uu[q].lo : ux0,
                              (DOT != 0 && !UX) ? uu[q].hi : ux1, d0, d1);
            wave_lds_fence();                                                   // the slice is free for the next block's values
        }
    }
    if (n_left > 0) {
        __syncthreads();
        dict_walk<T, DOT, false, false, true>(n_left, 0, desc64, left_order, row_ptr, code, val, x, y, u, tail2, g2_last,
                                             (const PairEnt<T> *)nullptr, s_off8, s_c, &vsl[0][0], VS, d0, d1);
    }
    spmv_dot_epilogue<DOT>(d0, d1, red, part0, part1, fin);
}

}  // namespace

int launch_tile_off(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                    double *part0, double *part1, const int *status, const Fin &fin) {
    sprs_ctx *c = A->ctx;
    const sprs_dict *D = A->dict;
    const sprs_tile_plan &TP = *r.tile;
    const BlkDesc *desc64 = r.desc;       // the 64-row blocks outside the tiles
    int g2_last;
    const V2d *tail2 = dict_tail2(A, g2_last);
    const TilePat tp = tile_pat(TP);
    const BlkDesc *owd = reinterpret_cast<const BlkDesc *>(D->owide_desc);
    const double *v = reinterpret_cast<const double *>(A->val);
    // UX: the dot operand is the input vector (mul_vec_dot, MINRES' v.Av, K4 without a preconditioner); without a dot, one kernel
    with_dot(dot_mode, u == x, [&](auto dm, auto ux) {
        constexpr int DM = decltype(dm)::value;
        constexpr bool UXV = DM != 0 && decltype(ux)::value;
#define SPRS_TOSHAPE(U, L, H)                                                                                                             \
    if (TP.ul == U && TP.fl == L && TP.fh == H)                                                                                           \
        SPRS_LAUNCH_SPMV(c, (spmv_tile_off_kernel<DM, UXV, U, L, H>), r.grid, reinterpret_cast<const int2 *>(TP.list), TP.xstart, owd, tp, \
                         TP.n_left, TP.left, desc64, A->row_ptr, D->idx_code, D->off_tab, v, x, y, u, part0, part1, status, fin, tail2, g2_last);
        SPRS_TILE_SHAPES(SPRS_TOSHAPE)
#undef SPRS_TOSHAPE
    });
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

}  // namespace sprs
