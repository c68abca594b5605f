// LOBPCG (sprs_lobpcg_*): the kernels that are its own (the solver itself: Lobpcg<T> in lobpcg.hip).  No reference analogue — the
// recurrence is the one stated in the header.  One iteration on the 6 b contiguous vectors [X, P, W | AX, AP, AW]:
//   LobResid  (fused_kernel) r_c = AX_c - theta_c X_c for all b columns, W_c = r_c or dinv r_c, partials of |r_c|^2
//   LobCheck  (one workgroup) the norms, nconv, the events
//   b applications of an applied M in place on W ; b SpMVs AW_c = A W_c
//   LobGram   one pass over the basis and its products: per-workgroup partials of the upper triangles of G = S^H S, K = S^H AS
//   LobReduce the partials summed in double, a wavefront per entry
//   LobRR     (one workgroup) the projected problem in double: scaling, Cholesky, K^ = L^-1 K L^-H, its eigenpairs by cyclic
//             Jacobi in LDS, the order of `which`, the coefficient block [C_X | C_P] rounded once to T ; the [X, W] fallback
//   LzRotate  twice (eigsh_fuse.hpp, coefficients of type T): [X, P] <- [X, P, W] [C_X | C_P] in place, the same on the products
// The conventions are gmres_fuse.hpp's: partials re-reduced in one fixed order by their consumer, no atomics, `status` turns the
// rest of an iteration's blind launches into no-ops, the host reads nothing but the head of the state.
#pragma once
#include <type_traits>

#include "eigsh_fuse.hpp"

namespace sprs {

constexpr int LOB_MAXB = SPRS_LOBPCG_MAX_BLOCK;
constexpr int LOB_MAXM = 3 * LOB_MAXB;
constexpr int LOB_LD = LOB_MAXM + 1;         // LobRR's row stride in LDS (odd: a column walk meets every bank once)
constexpr int LOB_MAX_SWEEPS = 30;
constexpr int LOB_THREADS = 512;             // LobGram's workgroup: 8 wavefronts, one workgroup a CU, up to 256 VGPRs a lane
constexpr int LOB_NW = LOB_THREADS / WAVE;
constexpr int LOB_MAX_WALK = 512;            // the most workgroups that walk the tiles (= partials per entry)
static_assert(LOB_MAXM <= LZ_MAXM, "the coefficient block has LzRotate's leading dimension");

// What the host reads (once per `poll` iterations) ...
template <class T>
struct LobHead {
    int status, nconv;
    int zero, pad;              // zero: never written — the guard of the launches the host enqueues after it has read the state
    int k, which;               // set by the host per solve
    long long matvecs, iters, restarts;
    double anorm, tol;
};
// ... what it reads besides when the solve is over (theta, res) and the rest of the device-resident state
template <class T>
struct LobState {
    LobHead<T> hd;
    double theta[LOB_MAXB], res[LOB_MAXB];
    int lock[LOB_MAXB];                  // LobCheck: column c is soft-locked (res_c <= tol anorm), LobRR leaves P_c and W_c out
    T coef[LOB_MAXM * LZ_MAXM];          // coef[i * LZ_MAXM + c]: [C_X | C_P], 3 b rows and 2 b columns (b and b at the start)
    T ident[LOB_MAXB * LZ_MAXM];         // the identity: LzRotate as the copy of k columns into the caller's vectors
};

// rows of an entry block: a lane does 2 R LDS reads of 16 bytes per R^2 multiply-adds of a pack
template <class T> struct lob_r { static constexpr int value = 4; };
template <> struct lob_r<cplx> { static constexpr int value = 2; };
// the most entry blocks a wavefront may own (R^2 accumulators of T each: 192 VGPRs in f64, 96 in f32 / c32, 160 in c64) ...
template <class T> struct lob_nbw { static constexpr int value = 6; };
template <> struct lob_nbw<cplxf> { static constexpr int value = 3; };
template <> struct lob_nbw<cplx> { static constexpr int value = 10; };
// ... and the small flavour (b <= 2 or so)
template <class T> struct lob_nbw_small { static constexpr int value = 2; };
template <> struct lob_nbw_small<cplx> { static constexpr int value = 3; };

// acc += conj(x) y, every multiply-add fused: the same instruction sequence in both flavours of the kernel
__device__ __forceinline__ void lob_fma(double &a, double x, double y) { a = __builtin_fma(x, y, a); }
__device__ __forceinline__ void lob_fma(float &a, float x, float y) { a = __builtin_fmaf(x, y, a); }
__device__ __forceinline__ void lob_fma(cplx &a, cplx x, cplx y) {
    a.re = __builtin_fma(x.re, y.re, __builtin_fma(x.im, y.im, a.re));
    a.im = __builtin_fma(x.re, y.im, __builtin_fma(-x.im, y.re, a.im));
}
__device__ __forceinline__ void lob_fma(cplxf &a, cplxf x, cplxf y) {
    a.re = __builtin_fmaf(x.re, y.re, __builtin_fmaf(x.im, y.im, a.re));
    a.im = __builtin_fmaf(x.re, y.im, __builtin_fmaf(-x.im, y.re, a.im));
}

// 64 lanes x 16 bytes from per-lane global addresses into LDS at lds_base + 16 lane, asynchronously (counted by vmcnt)
__device__ __forceinline__ void lob_glds16(const void *g, void *lds_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g, (__attribute__((address_space(3))) void *)lds_base, 16, 0, 0);
}

template <class T, int PK>
__device__ __forceinline__ Pack<T, PK> lob_zero_pack() {
    Pack<T, PK> z;
#pragma unroll
    for (int e = 0; e < PK; ++e) z.v[e] = szero<T>();
    return z;
}

// basis vector j of the pass (j < m) -> its slot among [X, P, W]: layout 2 is [X, W]
__device__ __forceinline__ int lob_slot(int j, int b, int layout) { return (layout == 2 && j >= b) ? j + b : j; }
// the upper-triangle index of (i, j), i <= j < m, row-major
__host__ __device__ __forceinline__ int lob_tri(int i, int j, int m) { return i * m - i * (i - 1) / 2 + (j - i); }

// ---- LobGram: part[w][0 .. NE) = walker w's share of G_ij = sum conj(S_i) S_j, part[w][NE .. 2 NE) of K_ij = sum conj(S_i) AS_j,
// i <= j < m, NE = m (m + 1) / 2.  S_j = V + slot(j) vstride, AS_j = S_j + aoff.
// A workgroup takes tiles of 64 packs (as LzRotate) and stages the tile of the m basis vectors and the m products in LDS (1 KiB
// per vector, two buffers: the next tile's loads go straight into the other one while this tile is folded; the last, partial
// tile by coalesced 16-byte loads through registers, non-temporal where NT), then every lane owns pack `lane` of the tile
// and every wavefront its entry blocks: R x R entries of G or K, block t of the workgroup's list going to wavefront t mod 8.
// A lane reads the R + R packs of a block once and keeps the block's R^2 accumulators in registers across all the tiles the
// workgroup walks; the butterflies run once, after the walk.  m is padded to a multiple of R with zero vectors in LDS.
// nsplit = 2 (where one workgroup's registers cannot hold both triangles: c64 beyond m = 16, c32 beyond m = 16): the even
// workgroups own G's blocks and stage the basis alone, the odd ones K's.
template <class T, bool NT, int NBW>
__global__ __launch_bounds__(LOB_THREADS) void lob_gram_kernel(const int *__restrict__ status, const T *V, int64_t vstride, int64_t aoff, int b,
                                                               int layout, int m, int64_t n, int nsplit, T *__restrict__ part) {
    constexpr int PK = pack_width<T>::value, R = lob_r<T>::value, ROWS = WAVE * PK;
    using P = Pack<T, PK>;
    if (*status != ST_RUNNING) return;
    extern __shared__ __align__(16) unsigned char lob_tile_raw[];
    const int MB = (m + R - 1) / R, mp = MB * R;
    P *tS = reinterpret_cast<P *>(lob_tile_raw);          // two buffers of [basis | products], [mp][WAVE] packs each
    const int side = (int)blockIdx.x % nsplit, w = (int)blockIdx.x / nsplit, GW = (int)gridDim.x / nsplit;
    const int nb1 = MB * (MB + 1) / 2, nblk = nsplit == 1 ? 2 * nb1 : nb1;
    const bool needA = nsplit == 1 || side == 1;
    for (int id = m * WAVE + (int)threadIdx.x; id < mp * WAVE; id += LOB_THREADS)       // the padding vectors of both buffers
        for (int u = 0; u < 4; ++u) tS[u * mp * WAVE + id] = lob_zero_pack<T, PK>();
    const int lane = threadIdx.x & (WAVE - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // this wavefront's blocks: (kind, I, J) of block t = wv + s LOB_NW, I <= J < MB
    int bk[NBW], bi[NBW], bj[NBW];
    T acc[NBW][R][R];
#pragma unroll
    for (int s = 0; s < NBW; ++s) {
        const int t = wv + s * LOB_NW;
        int u = nsplit == 1 ? t % nb1 : t, I = 0;
        bk[s] = t >= nblk ? -1 : (nsplit == 1 ? t / nb1 : side);
        while (u >= MB - I && I < MB - 1) { u -= MB - I; ++I; }
        bi[s] = I; bj[s] = min(I + u, MB - 1);
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int c = 0; c < R; ++c) acc[s][a][c] = szero<T>();
    }
    const int64_t ntile = (n + ROWS - 1) / ROWS;
    const int nvec = (needA ? 2 : 1) * m, bufsz = 2 * mp * WAVE;
    // tile t into buffer u.  A whole tile: wavefront wv takes vectors wv, wv + 8, ... and its load of a vector's 64 packs goes
    // straight into LDS (1 KiB, lane-linear), so no register holds a tile while another is folded.  The last, partial tile goes
    // through registers, its rows past n as zeros.
    auto stage = [&](int64_t t, int u) __attribute__((always_inline)) {
        P *dS = tS + u * bufsz, *dA = dS + mp * WAVE;
        const int64_t pack0 = t * WAVE;
        if ((pack0 + WAVE) * PK <= n) {
            for (int jj = wv; jj < nvec; jj += LOB_NW) {
                const int j = jj >= m ? jj - m : jj;
                lob_glds16(V + (int64_t)lob_slot(j, b, layout) * vstride + (jj >= m ? aoff : 0) + (pack0 + lane) * PK, (jj >= m ? dA : dS) + j * WAVE);
            }
        } else {
            for (int id = threadIdx.x; id < nvec * WAVE; id += LOB_THREADS) {
                const int jj = id >> 6, l = id & (WAVE - 1), j = jj >= m ? jj - m : jj;
                const int64_t row = (pack0 + l) * PK;
                P v = lob_zero_pack<T, PK>();
                if (row < n) {
                    v = ldp<T, PK, NT>(V + (int64_t)lob_slot(j, b, layout) * vstride + (jj >= m ? aoff : 0), pack0 + l);   // (the vectors are padded to whole packs)
#pragma unroll
                    for (int e = 1; e < PK; ++e)
                        if (row + e >= n) v.v[e] = szero<T>();
                }
                (jj >= m ? dA : dS)[j * WAVE + l] = v;
            }
        }
    };
    int cur = 0;
    if (w < ntile) stage(w, 0);
    for (int64_t t = w; t < ntile; t += GW) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this tile's loads have landed in LDS ...
        __syncthreads();                                     // ... every wavefront's, and the other buffer's readers are done
        if (t + GW < ntile) stage(t + GW, cur ^ 1);          // the next tile's loads fly while this one is folded
        const P *cS = tS + cur * bufsz, *cA = cS + mp * WAVE;
#pragma unroll
        for (int s = 0; s < NBW; ++s) {
            if (bk[s] < 0) continue;
            const P *xs = cS + bi[s] * R * WAVE + lane, *ys = (bk[s] ? cA : cS) + bj[s] * R * WAVE + lane;
            P x[R], y[R];
#pragma unroll
            for (int a = 0; a < R; ++a) { x[a] = xs[a * WAVE]; y[a] = ys[a * WAVE]; }
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int c = 0; c < R; ++c)
#pragma unroll
                    for (int e = 0; e < PK; ++e) lob_fma(acc[s][a][c], x[a].v[e], y[c].v[e]);
        }
        cur ^= 1;
    }
    const int NE = m * (m + 1) / 2;
    T *mine = part + (size_t)w * 2 * NE;
#pragma unroll
    for (int s = 0; s < NBW; ++s) {
        if (bk[s] < 0) continue;
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const T v = wave_sum(acc[s][a][c]);
                const int gi = bi[s] * R + a, gj = bj[s] * R + c;
                if (lane == 0 && gi <= gj && gj < m) mine[bk[s] * NE + lob_tri(gi, gj, m)] = v;
            }
    }
}

// ---- LobResid: r_c = AX_c - theta_c X_c (theta_c rounded once to T::Real), W_c = r_c or dinv r_c, partials of |r_c|^2 at
// partN[c * MAX_GRID + workgroup], all b columns in one launch
template <class T, class V>
struct LobResid {
    const LobState<T> *S; const T *X; const T *AX; T *W; int64_t vs; int b; const V *dinv; Real<T> *partN;
    Real<T> th[LOB_MAXB], accN[LOB_MAXB];
    __device__ __forceinline__ bool prologue() {
        if (S->hd.status != ST_RUNNING) return false;
#pragma unroll
        for (int c = 0; c < LOB_MAXB; ++c) { th[c] = c < b ? (Real<T>)S->theta[c] : Real<T>(0); accN[c] = 0.0; }
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        Pack<V, PK> dv;
        if (dinv) dv = ldp<V, PK, NT>(dinv, i);
#pragma unroll
        for (int c = 0; c < LOB_MAXB; ++c) {
            if (c < b) {
                const auto xv = ldp<T, PK, NT>(X + c * vs, i), av = ldp<T, PK, NT>(AX + c * vs, i);
                Pack<T, PK> wv;
#pragma unroll
                for (int e = 0; e < PK; ++e) {
                    const T r = ssub(av.v[e], smulr(xv.v[e], th[c]));
                    accN[c] = accN[c] + ssq(r);
                    wv.v[e] = dinv ? smulv(r, dv.v[e]) : r;
                }
                stp<T, PK, NT>(W + c * vs, i, wv);
            }
        }
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<T> smD[NWAVE];
#pragma unroll
        for (int c = 0; c < LOB_MAXB; ++c) {
            if (c < b) {
                const Real<T> sN = block_sum(accN[c], smD);
                if (threadIdx.x == 0) partN[c * MAX_GRID + blockIdx.x] = sN;
            }
        }
    }
};

// ---- LobCheck: res_c = |r_c| from LobResid's partials ; a NaN: breakdown ; lock_c = res_c <= tol anorm for every c < b (soft
// locking: LobRR leaves P_c and W_c out of the projected problem) ; nconv = the leading c < k that are locked ; nconv == k:
// converged (iters stays at the iterations completed)
template <class T>
__global__ __launch_bounds__(BLOCK) void lob_check_kernel(LobState<T> *S, const Real<T> *partN, int P, int b) {
    __shared__ Real<T> smD[NWAVE];
    __shared__ double sres[LOB_MAXB];
    LobHead<T> &H = S->hd;
    if (H.status != ST_RUNNING) return;
    for (int c = 0; c < b; ++c) {
        const Real<T> sN = reduce_partials(partN + c * MAX_GRID, P, smD);
        if (threadIdx.x == 0) sres[c] = (double)ssqrt(sN);
    }
    if (threadIdx.x != 0) return;
    bool nan = false;
    for (int c = 0; c < b; ++c) { S->res[c] = sres[c]; nan = nan || !(sres[c] >= 0.0); }
    if (nan) { H.status = ST_BREAKDOWN; return; }
    for (int c = 0; c < b; ++c) S->lock[c] = sres[c] <= H.tol * H.anorm ? 1 : 0;
    int nc = 0;
    while (nc < H.k && S->lock[nc]) ++nc;
    H.nconv = nc;
    if (nc == H.k) H.status = ST_CONVERGED;
}

// ---- LobRR: the Rayleigh-Ritz step of the header, one workgroup, everything in double (complex double for complex T)
__device__ __forceinline__ double lob_cd(double v) { return v; }
__device__ __forceinline__ double lob_cd(float v) { return (double)v; }
__device__ __forceinline__ cplx lob_cd(cplx v) { return v; }
__device__ __forceinline__ cplx lob_cd(cplxf v) { return cplx{(double)v.re, (double)v.im}; }
__device__ __forceinline__ void lob_round(double v, double &o) { o = v; }
__device__ __forceinline__ void lob_round(double v, float &o) { o = (float)v; }
__device__ __forceinline__ void lob_round(cplx v, cplx &o) { o = v; }
__device__ __forceinline__ void lob_round(cplx v, cplxf &o) { o = cplxf{(float)v.re, (float)v.im}; }
__device__ __forceinline__ double lob_real_only(double v) { return v; }
__device__ __forceinline__ cplx lob_real_only(cplx v) { return cplx{v.re, 0.0}; }
__device__ __forceinline__ double lob_unit(double v, double mag) { return v / mag; }
__device__ __forceinline__ cplx lob_unit(cplx v, double mag) { return cplx{v.re / mag, v.im / mag}; }

template <class T> using LobCD = std::conditional_t<is_complex<T>::value, cplx, double>;

// ---- LobReduce: sums[e] = the sum over the GW walkers of part[w][e], e < NE2, in double.  A wavefront per entry: lane l adds
// walkers l, l + 64, ... in that order, then one butterfly — a fixed order, whatever the grid.
template <class T>
__global__ __launch_bounds__(BLOCK) void lob_reduce_kernel(const int *__restrict__ status, const T *__restrict__ part, int GW, int NE2, LobCD<T> *__restrict__ sums) {
    if (*status != ST_RUNNING) return;
    const int lane = threadIdx.x & (WAVE - 1), e = (int)blockIdx.x * NWAVE + (int)(threadIdx.x >> 6);
    if (e >= NE2) return;
    LobCD<T> acc = szero<LobCD<T>>();
    for (int w = lane; w < GW; w += WAVE) acc = sadd(acc, lob_cd(part[(size_t)w * NE2 + e]));
    acc = wave_sum(acc);
    if (lane == 0) sums[e] = acc;
}

// y <- L^-1 y and y <- L^-H y on a column held in registers (L: ma x ma lower triangular in LDS, row stride LOB_LD; every
// wavefront reads the same L_iq: broadcast reads that do not wait for one another)
template <class CD>
__device__ __forceinline__ void lob_forward(const CD *sL, int ma, CD (&y)[LOB_MAXM]) {
#pragma unroll
    for (int i = 0; i < LOB_MAXM; ++i) {
        if (i < ma) {
            CD v = y[i];
#pragma unroll
            for (int q = 0; q < i; ++q) v = ssub(v, smul(sL[i * LOB_LD + q], y[q]));
            y[i] = smulr(v, 1.0 / sre(sL[i * LOB_LD + i]));
        }
    }
}
template <class CD>
__device__ __forceinline__ void lob_backward(const CD *sL, int ma, CD (&y)[LOB_MAXM]) {
#pragma unroll
    for (int i = LOB_MAXM - 1; i >= 0; --i) {
        if (i < ma) {
            CD v = y[i];
#pragma unroll
            for (int q = i + 1; q < LOB_MAXM; ++q)
                if (q < ma) v = ssub(v, smul(sconj(sL[q * LOB_LD + i]), y[q]));
            y[i] = smulr(v, 1.0 / sre(sL[i * LOB_LD + i]));
        }
    }
}

// Cyclic Jacobi on the Hermitian sA (M x M, M even, row stride LOB_LD) with sV = I: lz_ritz_kernel's round-robin order and
// stopping rule, but not its loop: for a real pivot a_pq < 0 with a_pp == a_qq this one rotates with s = -c (tau from |a_pq|,
// then the phase a_pq / |a_pq| = -1) and lz_ritz_kernel's with s = +c (tau = -0.0 passes its tau >= 0), so one loop for both
// would change the bits of one solver's eigenvectors.  The rotation carries the phase u of its pivot (sc = s u): columns
// x_p' = c x_p - conj(sc) x_q, x_q' = sc x_p + c x_q on A and V, rows row_p' = c row_p - sc row_q,
// row_q' = conj(sc) row_p + c row_q on A, then A_pq = A_qp = 0 and Im A_pp = Im A_qq = 0 exactly.  false: a NaN or the sweep cap.
template <class CD>
__device__ bool lob_jacobi(CD *sA, CD *sV, int M, double *sc, CD *ss, double *smD) {
    const int tid = threadIdx.x;
    double fro = 0.0;
    for (int e = tid; e < M * M; e += BLOCK) {
        const int r = e / M, c = e % M;
        sV[r * LOB_LD + c] = r == c ? sone<CD>() : szero<CD>();
        fro += ssq(sA[r * LOB_LD + c]);
    }
    const double fro2 = block_sum(fro, smD), eps = seps<double>();
    if (!(fro2 >= 0.0) || fro2 > 1.7e308) return false;
    for (int sweeps = 0;; ++sweeps) {
        double off = 0.0;
        for (int e = tid; e < M * M; e += BLOCK) {
            const int r = e / M, c = e % M;
            if (r != c) off += ssq(sA[r * LOB_LD + c]);
        }
        const double off2 = block_sum(off, smD);
        if (off2 <= eps * eps * fro2) return true;
        if (sweeps == LOB_MAX_SWEEPS) return false;
        for (int r = 0; r < M - 1; ++r) {
            if (tid < M / 2) {
                int pp, qq;
                lz_pair(tid, r, M, pp, qq);
                const CD apq = sA[pp * LOB_LD + qq];
                const double mag = sabs(apq);
                double c = 1.0;
                CD s = szero<CD>();
                if (mag != 0.0) {
                    const double tau = (sre(sA[qq * LOB_LD + qq]) - sre(sA[pp * LOB_LD + pp])) / (2.0 * mag);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = smulr(lob_unit(apq, mag), t * c);
                }
                sc[tid] = c; ss[tid] = s;
            }
            __syncthreads();
            for (int e = tid; e < M * (M / 2); e += BLOCK) {       // A <- A J, V <- V J
                const int i = e / M, row = e % M;
                int pp, qq;
                lz_pair(i, r, M, pp, qq);
                const double c = sc[i];
                const CD s = ss[i], sh = sconj(s);
                const CD ap = sA[row * LOB_LD + pp], aq = sA[row * LOB_LD + qq];
                sA[row * LOB_LD + pp] = ssub(smulr(ap, c), smul(sh, aq)); sA[row * LOB_LD + qq] = sadd(smul(s, ap), smulr(aq, c));
                const CD vp = sV[row * LOB_LD + pp], vq = sV[row * LOB_LD + qq];
                sV[row * LOB_LD + pp] = ssub(smulr(vp, c), smul(sh, vq)); sV[row * LOB_LD + qq] = sadd(smul(s, vp), smulr(vq, c));
            }
            __syncthreads();
            for (int e = tid; e < M * (M / 2); e += BLOCK) {       // A <- J^H A
                const int i = e / M, col = e % M;
                int pp, qq;
                lz_pair(i, r, M, pp, qq);
                const double c = sc[i];
                const CD s = ss[i], sh = sconj(s);
                const CD ap = sA[pp * LOB_LD + col], aq = sA[qq * LOB_LD + col];
                CD np = ssub(smulr(ap, c), smul(s, aq)), nq = sadd(smul(sh, ap), smulr(aq, c));
                if (col == pp) { np = lob_real_only(np); nq = szero<CD>(); }       // the rotated entry exactly zero, the diagonal real
                if (col == qq) { np = szero<CD>(); nq = lob_real_only(nq); }
                sA[pp * LOB_LD + col] = np; sA[qq * LOB_LD + col] = nq;
            }
            __syncthreads();
        }
    }
}

// sums: LobReduce's sums of the partials of a pass of m_in vectors in `layout` (1: [X], the start step; 2: [X, W]; 3: [X, P, W]).
// it: the iteration this step completes (0: the start step).  The problem's index set: every X column, then the P columns (layout
// 3, the first attempt) and the W columns of the columns that LobCheck did not lock, ascending ; sidx maps the problem's index to
// the pass's, spos a row of the coefficient block to the problem's index (-1: not in it).  Every element of every matrix is
// written by one thread per phase, with barriers between the phases, and every sum has a fixed order.
template <class T>
__global__ __launch_bounds__(BLOCK) void lob_rr_kernel(LobState<T> *S, const LobCD<T> *__restrict__ sums, int m_in, int layout, int b, long long it) {
    using CD = LobCD<T>;
    __shared__ CD sG[LOB_MAXM * LOB_LD], sK[LOB_MAXM * LOB_LD], sL[LOB_MAXM * LOB_LD], sA[LOB_MAXM * LOB_LD], sV[LOB_MAXM * LOB_LD];
    __shared__ CD srot[LOB_MAXM / 2];
    __shared__ double ssc[LOB_MAXM], sth[LOB_MAXM], scs[LOB_MAXM / 2], smD[NWAVE];
    __shared__ int sperm[LOB_MAXM], sidx[LOB_MAXM], spos[LOB_MAXM], sma, sfail;
    LobHead<T> &H = S->hd;
    if (H.status != ST_RUNNING) return;
    const int tid = threadIdx.x, which = H.which;
    const int NE = m_in * (m_in + 1) / 2;
    // (1) LobReduce's sums ; the lower triangles are the conjugates of the upper, the diagonals real
    for (int e = tid; e < 2 * NE; e += BLOCK) {
        const int kind = e / NE;
        int u = e % NE, i = 0;
        while (u >= m_in - i) { u -= m_in - i; ++i; }
        const int j = i + u;
        const CD acc = sums[e];
        CD *dst = kind ? sK : sG;
        if (i == j) dst[i * LOB_LD + i] = lob_real_only(acc);
        else { dst[i * LOB_LD + j] = acc; dst[j * LOB_LD + i] = sconj(acc); }
    }
    if (tid == 0) sfail = 0;
    __syncthreads();
    const double epsR = (double)seps<Real<T>>();
    int attempt = 0, ma = m_in;
    auto act = [&](int i) { return sidx[i]; };
    for (;; ++attempt) {
        // the problem's index i -> the pass's index: the second attempt leaves the P block out, both the locked columns' P and W
        if (tid == 0) {
            int na = 0;
            for (int c = 0; c < b; ++c) sidx[na++] = c;
            if (layout == 3 && attempt == 0)
                for (int c = 0; c < b; ++c)
                    if (!S->lock[c]) sidx[na++] = b + c;
            if (layout != 1)
                for (int c = 0; c < b; ++c)
                    if (!S->lock[c]) sidx[na++] = (layout == 3 ? 2 * b : b) + c;
            sma = na;
        }
        __syncthreads();
        ma = sma;
        // (2) the scaling
        if (tid < ma) {
            const double g = sre(sG[act(tid) * LOB_LD + act(tid)]);
            if (!(g > 0.0) || g > 1.7e308) sfail = 1;
            ssc[tid] = 1.0 / sqrt(g);
        }
        __syncthreads();
        bool fail = sfail != 0;
        if (!fail) {
            // (3) Cholesky of the scaled G, column by column in the lower triangle of sL
            for (int e = tid; e < ma * ma; e += BLOCK) {
                const int r = e / ma, c = e % ma;
                sL[r * LOB_LD + c] = smulr(sG[act(r) * LOB_LD + act(c)], ssc[r] * ssc[c]);
            }
            __syncthreads();
            for (int j = 0; j < ma; ++j) {
                if (tid == 0) {
                    double piv = sre(sL[j * LOB_LD + j]);
                    for (int q = 0; q < j; ++q) piv -= ssq(sL[j * LOB_LD + q]);
                    if (!(piv > 64.0 * ma * epsR)) sfail = 1;
                    sL[j * LOB_LD + j] = sfromr<CD>(sqrt(piv));
                }
                __syncthreads();
                if (sfail) break;
                if (tid > j && tid < ma) {
                    CD v = sL[tid * LOB_LD + j];
                    for (int q = 0; q < j; ++q) v = ssub(v, smul(sL[tid * LOB_LD + q], sconj(sL[j * LOB_LD + q])));
                    sL[tid * LOB_LD + j] = smulr(v, 1.0 / sre(sL[j * LOB_LD + j]));
                }
                __syncthreads();
            }
            fail = sfail != 0;
        }
        if (!fail) break;
        // (4) P in the basis: once more without it ; else a breakdown
        __syncthreads();
        if (attempt == 0 && layout == 3) {
            if (tid == 0) { sfail = 0; H.restarts += 1; }
            __syncthreads();
            continue;
        }
        if (tid == 0) { H.matvecs += b; H.status = ST_BREAKDOWN; }
        return;
    }
    const int M = (ma + 1) & ~1;
    // (5) K^ = L^-1 (s K s) L^-H: a thread per column, then a thread per row, forward substitutions in place in sA
    for (int e = tid; e < M * M; e += BLOCK) {
        const int r = e / M, c = e % M;
        sA[r * LOB_LD + c] = (r < ma && c < ma) ? smulr(sK[act(r) * LOB_LD + act(c)], ssc[r] * ssc[c]) : szero<CD>();
    }
    __syncthreads();
    CD y[LOB_MAXM];
    if (tid < ma) {
#pragma unroll
        for (int i = 0; i < LOB_MAXM; ++i) y[i] = i < ma ? sA[i * LOB_LD + tid] : szero<CD>();
        lob_forward<CD>(sL, ma, y);
#pragma unroll
        for (int i = 0; i < LOB_MAXM; ++i)
            if (i < ma) sA[i * LOB_LD + tid] = y[i];
    }
    __syncthreads();
    if (tid < ma) {     // row tid of M1 L^-H: y = L^-1 conj(row), the row's new entries its conjugates
#pragma unroll
        for (int i = 0; i < LOB_MAXM; ++i) y[i] = i < ma ? sconj(sA[tid * LOB_LD + i]) : szero<CD>();
        lob_forward<CD>(sL, ma, y);
#pragma unroll
        for (int i = 0; i < LOB_MAXM; ++i)
            if (i < ma) sA[tid * LOB_LD + i] = sconj(y[i]);
    }
    __syncthreads();
    for (int e = tid; e < ma * ma; e += BLOCK) {       // Hermitian from the upper triangle, a real diagonal
        const int r = e / ma, c = e % ma;
        if (r == c) sA[r * LOB_LD + r] = lob_real_only(sA[r * LOB_LD + r]);
        else if (r > c) sA[r * LOB_LD + c] = sconj(sA[c * LOB_LD + r]);
    }
    __syncthreads();
    // (6) its eigenpairs
    if (!lob_jacobi<CD>(sA, sV, M, scs, srot, smD)) {
        if (tid == 0) { H.matvecs += b; H.status = ST_BREAKDOWN; }
        return;
    }
    // (7) the order of `which`: rank by value, ties by index
    lz_rank(ma, which == SPRS_EIGSH_LARGEST, [&](int j) { return sre(sA[j * LOB_LD + j]); }, sperm);
    if (tid < ma) sth[tid] = sre(sA[tid * LOB_LD + tid]);
    __syncthreads();
    // (8) C = diag(s) L^-H Z: a thread per column, back substitution in place in sV
    if (tid < ma) {
#pragma unroll
        for (int i = 0; i < LOB_MAXM; ++i) y[i] = i < ma ? sV[i * LOB_LD + tid] : szero<CD>();
        lob_backward<CD>(sL, ma, y);
#pragma unroll
        for (int i = 0; i < LOB_MAXM; ++i)
            if (i < ma) sV[i * LOB_LD + tid] = y[i];
    }
    __syncthreads();
    // the coefficient block: rows in the order [X, P, W] (the rows of a block that was left out are zero), columns C_X then C_P
    // (= C_X with the X rows zero) ; at the start b rows and C_X alone
    const int rows = layout == 1 ? b : 3 * b, cols = layout == 1 ? b : 2 * b;
    if (tid < rows) spos[tid] = -1;
    __syncthreads();
    if (tid < ma) spos[(layout == 2 && sidx[tid] >= b) ? sidx[tid] + b : sidx[tid]] = tid;
    __syncthreads();
    for (int e = tid; e < rows * cols; e += BLOCK) {
        const int r3 = e / cols, c = e % cols, cx = c % b;
        const int i = spos[r3];                            // the problem's index of row r3, -1: not in it
        CD v = szero<CD>();
        if (i >= 0 && !(c >= b && r3 < b)) v = smulr(sV[i * LOB_LD + sperm[cx]], ssc[i]);
        lob_round(v, S->coef[r3 * LZ_MAXM + c]);
    }
    if (tid < b) S->theta[tid] = sth[sperm[tid]];
    if (tid == 0) {
        double an = H.anorm;                               // the Rayleigh quotients of the problem's X and W columns: each <= |A|_2
        for (int i = 0; i < ma; ++i) {
            const int pi = sidx[i];
            if (layout == 3 && pi >= b && pi < 2 * b) continue;
            an = fmax(an, fabs(sre(sK[pi * LOB_LD + pi])) / sre(sG[pi * LOB_LD + pi]));
        }
        H.anorm = an; H.matvecs += b; H.iters = it;
    }
}

}  // namespace sprs
