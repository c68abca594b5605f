// LDS x-window tiles of the f64 PAIR-CODE stream (knob "spmv_tile"; design notes, the shared tile steps and the row-pair fold
// in spmv_dict_dev.hpp, profiles/r03_tuning.md §8).
#include "spmv_dict_dev.hpp"

namespace sprs {
namespace {

// UX: the dot operand is the input vector itself (mul_vec_dot, MINRES' v.Av, K4 without a preconditioner): taken from the window
template <int DOT, bool UX, int UL, int FL, int FH, int W>
__global__ __launch_bounds__(BLOCK) void spmv_tile_kernel(const int2 *__restrict__ tile_list, const int32_t *__restrict__ xstart,
                                                          const BlkDesc *__restrict__ desc, const TilePat pat,
                                                          int n_left, const int32_t *__restrict__ left_order,
                                                          const int32_t *__restrict__ row_ptr, const uint8_t *__restrict__ code,
                                                          const int32_t *__restrict__ off_tab, const double *__restrict__ val_tab,
                                                          const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ u,
                                                          double *__restrict__ part0, double *__restrict__ part1,
                                                          const int *__restrict__ status, int nrows, int ncols, const Fin fin) {
    using T = double;
    constexpr int TR = TILE_ROWS;                       // W: half-width of the window (TILE_W, or TILE_W_WIDE for line bands up to 1534)
    constexpr int NW = (TR + 2 * W) / 2 / BLOCK;        // 16-byte window pieces per lane
    constexpr int NQ = TILE_B / NWAVE;                  // 128-row blocks per wavefront and tile
    constexpr int NN = UL - FL - FH;                    // near slots
    static_assert((TR + 2 * W) % (2 * BLOCK) == 0 && TILE_B % NWAVE == 0 && NN >= 1 && UL <= 8, "tile shape");
    __shared__ __attribute__((aligned(16))) T win[TR + 2 * W];
    __shared__ PairEnt<T> s_pair[TAB];
    __shared__ __attribute__((aligned(16))) uint32_t s_c[NWAVE][CW2];
    __shared__ T red[NWAVE];
    const int run_state = status != nullptr ? *status : (int)ST_RUNNING;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    stage_pair(s_pair, tid, off_tab[tid] * 8, val_tab[tid]);                  // BLOCK == TAB (the seam rows' own values; the walk below)
    for (int i = lane; i < CW2; i += WAVE) s_c[wv][i] = 0;
    __syncthreads();
    if (run_state != ST_RUNNING) { fin_idle(fin, DOT == 2); return; }
    T d0 = 0.0, d1 = 0.0;

    TileCursor cur = tile_cursor(tile_list, xstart);
    uint32_t rbw[NQ]; int nnw[NQ];
    tile_seam_words(desc, __builtin_amdgcn_readfirstlane(cur.ent.x), wv, rbw, nnw);
    for (; cur.s < cur.send; cur.s += cur.sstep) {
        const int ts = tile_cursor_take(cur, tile_list);
        uint32_t rbc[NQ]; int nnc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { rbc[q] = rbw[q]; nnc[q] = nnw[q]; }
        // ---- loads: the window, then the far pairs (and dot operands) of the lane's NQ row pairs, then the next tile's words
        u4v wreg[NW];
        window_load(x + (ts - W), tid, wreg);
        D2 far[NQ][FL + FH > 0 ? FL + FH : 1];
        D2 uu[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) tile_far_loads<DOT, UX, UL, FL, FH>(x, u, pat, ts + ((q * NWAVE + wv) << 7) + 2 * lane, far[q], uu[q]);
        if (cur.s + cur.sstep < cur.send) tile_seam_words(desc, __builtin_amdgcn_readfirstlane(cur.ent.x), wv, rbw, nnw);
        window_stage(win, tid, wreg);
        // near slots from the window; the reads of block q + 1 are issued before block q is folded (the seam branch
        // of the fold keeps the compiler from doing that itself, and a fold behind an exposed LDS round trip eight times per
        // tile is 10 % of the launch)
        T npl[NN], nph[NN];
        tile_read_near(win, W + (wv << 7) + 2 * lane, pat.off + FL, npl, nph);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const uint32_t rbq = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbc[q]);
            const int li = W + ((q * NWAVE + wv) << 7) + 2 * lane;              // window index of x[r0]
            T pl[UL], ph[UL];
            tile_slots<UL, FL, FH>(far[q], npl, nph, pl, ph);
            T ux0 = 0.0, ux1 = 0.0;
            if (DOT != 0 && UX) { ux0 = win[li]; ux1 = win[li + 1]; }
            if (q + 1 < NQ) tile_read_near(win, W + (((q + 1) * NWAVE + wv) << 7) + 2 * lane, pat.off + FL, npl, nph);
            T acc0 = 0.0, acc1 = 0.0;
            pair_fold<UL>(pl, ph, pat.val, rbq, nnc[q], s_pair, lane, acc0, acc1);
            row_pair_out<DOT>(y + (ts + ((q * NWAVE + wv) << 7) + 2 * lane), acc0, acc1, (DOT != 0 && !UX) ? uu[q].lo : ux0,
                              (DOT != 0 && !UX) ? uu[q].hi : ux1, d0, d1);
        }
    }
    if (n_left > 0) {
        __syncthreads();
        pair2_walk<DOT, true>(n_left, 0, desc, left_order, row_ptr, code, XPlain{reinterpret_cast<const char *>(x)}, y, u, nrows, ncols, s_pair, s_c, d0, d1);
    }
    spmv_dot_epilogue<DOT>(d0, d1, red, part0, part1, fin);
}

}  // namespace

int launch_tile_pair(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                     double *part0, double *part1, const int *status, const Fin &fin) {
    sprs_ctx *c = A->ctx;
    const sprs_dict *D = A->dict;
    const sprs_tile_plan &TP = *r.tile;
    const double *pvd = reinterpret_cast<const double *>(D->pair_val);
    const TilePat tp = tile_pat(TP);
    // UX: the dot operand is the input vector (mul_vec_dot, MINRES' v.Av, K4 without a preconditioner); without a dot, one kernel
    with_dot(dot_mode, u == x, [&](auto dm, auto ux) {
        constexpr int DM = decltype(dm)::value;
        constexpr bool UXV = DM != 0 && decltype(ux)::value;
#define SPRS_TSHAPE(U, L, H)                                                                                                              \
    if (TP.ul == U && TP.fl == L && TP.fh == H)                                                                                           \
        SPRS_LAUNCH_SPMV(c, (spmv_tile_kernel<DM, UXV, U, L, H, SPRS_TW>), r.grid, reinterpret_cast<const int2 *>(TP.list), TP.xstart, r.desc, tp, \
                         TP.n_left, TP.left, A->row_ptr, D->pair_code, D->pair_off, pvd, x, y, u, part0, part1, status, (int)A->nrows, (int)A->ncols, fin);
#define SPRS_TW TILE_W
        if (TP.w == TILE_W) { SPRS_TILE_SHAPES(SPRS_TSHAPE) }
#undef SPRS_TW
#define SPRS_TW TILE_W_WIDE
        if (TP.w == TILE_W_WIDE) { SPRS_TILE_SHAPES_WIDE(SPRS_TSHAPE) }
#undef SPRS_TW
#undef SPRS_TSHAPE
    });
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

}  // namespace sprs
