// Thick-restart Lanczos (sprs_eigsh_*): the kernels that are its own (the solver itself: Eigsh<T> in eigsh.hip).  No reference
// analogue — the recurrence is the one stated in the header.  One Lanczos step j of a cycle:
//   SpMV      w = A v_j                                                   (KrylovBase::spmv, any route, no fused dot)
//   launch_cgs2                                                           (gmres_fuse.hpp, on LzState: CGS2 against v_0 .. v_j,
//                                                                          w - sum v_i c_i into the slot of v_{j+1}, partials of its norm)
//   LzStep    (one workgroup) T_jj, beta, the invariant-subspace threshold, T_{j+1,j}, the count of products ; sets `skip`
//   GmScale   v_{j+1} *= 1 / beta
// per cycle LzRitz (one workgroup: the eigenpairs of T by cyclic Jacobi in LDS, their order, res, anorm, nconv, the events, the
// coefficient block S rounded to T::Real, the restarted T) and, where the host restarts, LzRotate (V[:, :p] <- V[:, :m] S[:, :p]
// in place) ; per solve LzNrm + LzStart + GmScale before the first cycle and LzRotate once more for the eigenvectors.
// The conventions are gmres_fuse.hpp's: partials re-reduced in the same order by every consumer, `status` ends the solve and
// `skip` the rest of a cycle's blind launches, the host reads nothing but the head of the state (once a cycle).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "gmres_fuse.hpp"

namespace sprs {

constexpr int LZ_MAXM = SPRS_EIGSH_MAX_NCV;
static_assert(LZ_MAXM <= GM_MAXM, "GmUpdate stages one coefficient per basis vector in an array of GM_MAXM");
constexpr int LZ_LD = LZ_MAXM + 1;          // LzRitz's row stride in LDS (odd: a column walk meets every bank once)
constexpr int LZ_MAX_SWEEPS = 30;

// What the host reads (once a cycle) of a thick-restart solve: this one's, and the truncated SVD's (svds_fuse.hpp) ...
template <class T>
struct LzHead {
    int status, skip;
    int nconv, m_eff;           // m_eff: rows of the projected problem (m, or j + 1 of the step that met an invariant subspace)
    int invariant;
    int k, which;               // set by the host per solve
    long long matvecs, cycle;   // products that ran ; the cycle of the last step that ran (0: none)
    Real<T> scale;              // 1 / |v0|, or the reciprocal of a step's norm, for GmScale
    double beta, anorm, pscale, tol;     // pscale: the largest entry of the projected matrix (T, the SVD's B) so far
};
// ... what it reads besides when the solve is over (theta, res: everything before h) and the rest of the device-resident state.
// T is real symmetric whatever the scalar type, and is kept in double.
template <class T>
struct LzState {
    LzHead<T> hd;
    double theta[LZ_MAXM], res[LZ_MAXM];     // the Ritz values in the order of `which` and their residual estimates
    T h[LZ_MAXM];                            // GmUpdate's running column of CGS2 coefficients
    double Tm[LZ_MAXM * LZ_MAXM];            // row-major, leading dimension LZ_MAXM
    Real<T> coef[LZ_MAXM * LZ_MAXM];         // coef[i * LZ_MAXM + c] = S[i, c] rounded once to T::Real, columns in the order of `which`
};

// ---- LzNrm: partials of |v|^2 (the start vector, already in the slot of v_0)
template <class T>
struct LzNrm {
    const T *v; Real<T> *partN;
    Real<T> accN;
    __device__ __forceinline__ bool prologue() { accN = 0.0; return true; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        const auto xv = ldp<T, PK, NT>(v, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) accN = accN + ssq(xv.v[e]);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<T> smD[NWAVE];
        const Real<T> sN = block_sum(accN, smD);
        if (threadIdx.x == 0) partN[blockIdx.x] = sN;
    }
};

// LzStart: beta0 = |v0| from LzNrm's partials ; NaN or 0: breakdown ; scale = 1 / beta0 and the first cycle may run
// (St: LzState<T>, or SvState<T> of svds_fuse.hpp)
template <class T, class St>
__global__ __launch_bounds__(BLOCK) void lz_start_kernel(St *S, const Real<T> *partN, int P) {
    __shared__ Real<T> smD[NWAVE];
    LzHead<T> &H = S->hd;
    const Real<T> sN = reduce_partials(partN, P, smD);
    if (threadIdx.x != 0) return;
    const Real<T> beta0 = ssqrt(sN);
    if (!(beta0 > Real<T>(0))) { H.skip = 1; H.status = ST_BREAKDOWN; return; }
    H.scale = Real<T>(1) / beta0;
    H.skip = 0;
}

// LzStep: step j of cycle `cycle`.  beta from GmUpdate<SECOND>'s partials, T_jj = Re(h_j), the threshold, the sub-diagonal.
template <class T>
__global__ __launch_bounds__(BLOCK) void lz_step_kernel(LzState<T> *S, const Real<T> *partN, int P, int j, int m, long long cycle) {
    __shared__ Real<T> smD[NWAVE];
    LzHead<T> &H = S->hd;
    const int skip = H.skip;
    const Real<T> sN = reduce_partials(partN, P, smD);
    if (skip != 0 || threadIdx.x != 0) return;
    const double beta = (double)ssqrt(sN), tjj = (double)sre(S->h[j]);
    H.matvecs += 1; H.cycle = cycle;
    if (!(beta >= 0.0)) { H.skip = 1; H.status = ST_BREAKDOWN; return; }
    S->Tm[j * LZ_MAXM + j] = tjj;
    double sc = fmax(H.pscale, fabs(tjj));
    H.beta = beta;
    if (beta <= 64.0 * (double)seps<Real<T>>() * sc) {      // an invariant subspace: v_{j+1} is not formed
        H.pscale = sc; H.m_eff = j + 1; H.invariant = 1; H.skip = 1;
        return;
    }
    sc = fmax(sc, beta);
    H.pscale = sc;
    if (j + 1 < m) { S->Tm[(j + 1) * LZ_MAXM + j] = beta; S->Tm[j * LZ_MAXM + j + 1] = beta; }
    else H.m_eff = m;
    H.scale = Real<T>(1) / ssqrt(sN);
}

// Round r of the round-robin pairing of M (even) indices: pair 0 is (M - 1, r), pair i is ((r + i) mod (M - 1),
// (r - i) mod (M - 1)) — M / 2 disjoint pairs a round, every pair once in M - 1 rounds.  Returned with p < q.
__device__ __forceinline__ void lz_pair(int i, int r, int M, int &p, int &q) {
    int a, b;
    if (i == 0) { a = M - 1; b = r; }
    else { a = (r + i) % (M - 1); b = (r - i + (M - 1)) % (M - 1); }
    p = a < b ? a : b; q = a < b ? b : a;
}

// The order of `which` of me values: thread tid < me ranks value(tid) — those strictly before it (larger where `largest`, else
// smaller), ties by lower index — and records sperm[rank] = tid.  The caller's barrier stands between this and a read of sperm.
template <class F>
__device__ __forceinline__ void lz_rank(int me, bool largest, F value, int *sperm) {
    const int tid = threadIdx.x;
    if (tid >= me) return;
    const double ti = value(tid);
    int rank = 0;
    for (int j = 0; j < me; ++j) {
        const double tj = value(j);
        const bool first = largest ? tj > ti : tj < ti;
        rank += (first || (tj == ti && j < tid)) ? 1 : 0;
    }
    sperm[rank] = tid;
}

// The verdict of a thick-restart cycle (one thread): anorm = the largest |value| seen so far ; nconv = the leading pairs, in the
// order of sperm, with beta |last[sperm[i]]| <= tol anorm (last: the last row of the projected problem's vectors) ; then an
// invariant subspace ends the solve (converged where it holds k pairs, else a breakdown) and a running one ends at nconv == k.
template <class T>
__device__ __forceinline__ void lz_verdict(LzHead<T> &H, const double *vals, const double *last, const int *sperm, int me, int k, double beta,
                                           int invariant) {
    double an = H.anorm;
    for (int i = 0; i < me; ++i) an = fmax(an, fabs(vals[i]));
    int nc = 0;
    const int kk = k < me ? k : me;
    while (nc < kk && beta * fabs(last[sperm[nc]]) <= H.tol * an) ++nc;
    H.anorm = an;
    if (invariant) {
        if (me >= k) { H.nconv = k; H.status = ST_CONVERGED; }
        else { H.nconv = nc; H.skip = 1; H.status = ST_BREAKDOWN; }
    } else {
        H.nconv = nc;
        if (nc == k) { H.skip = 1; H.status = ST_CONVERGED; }
    }
}

// LzRitz: (theta, S) of T[:m_eff, :m_eff] by cyclic Jacobi (round-robin order, the rotated entry set to exactly zero; stop at
// off(T) <= eps |T|_F, LZ_MAX_SWEEPS sweeps at most, the cap being a breakdown), theta sorted for `which`, res, anorm, nconv,
// the events, the coefficient block, the restarted T (p kept pairs + the arrow row).  Every element of T and S is updated by one
// thread per phase and every sum has a fixed order: the result does not depend on timing.
template <class T>
__global__ __launch_bounds__(BLOCK) void lz_ritz_kernel(LzState<T> *S, int m, int p) {
    __shared__ double sA[LZ_MAXM * LZ_LD], sV[LZ_MAXM * LZ_LD];
    __shared__ double sc[LZ_MAXM / 2], ss[LZ_MAXM / 2], sth[LZ_MAXM], smD[NWAVE];
    __shared__ int sperm[LZ_MAXM];
    LzHead<T> &H = S->hd;
    if (H.status != ST_RUNNING) return;
    const int tid = threadIdx.x, me = H.m_eff, M = (me + 1) & ~1;
    const int k = H.k, which = H.which, invariant = H.invariant;
    const double beta = H.beta;
    double fro = 0.0;
    for (int e = tid; e < M * M; e += BLOCK) {
        const int r = e / M, c = e % M;
        const double a = (r < me && c < me) ? S->Tm[r * LZ_MAXM + c] : 0.0;     // (an odd m_eff: one idle index)
        sA[r * LZ_LD + c] = a; sV[r * LZ_LD + c] = r == c ? 1.0 : 0.0;
        fro += a * a;
    }
    const double fro2 = block_sum(fro, smD), eps = seps<double>();
    int sweeps = 0;
    bool conv = false;
    for (;;) {
        double off = 0.0;
        for (int e = tid; e < M * M; e += BLOCK) {
            const int r = e / M, c = e % M;
            const double a = sA[r * LZ_LD + c];
            if (r != c) off += a * a;
        }
        const double off2 = block_sum(off, smD);
        if (off2 <= eps * eps * fro2) { conv = true; break; }
        if (sweeps == LZ_MAX_SWEEPS) break;
        for (int r = 0; r < M - 1; ++r) {
            if (tid < M / 2) {
                int pp, qq;
                lz_pair(tid, r, M, pp, qq);
                const double apq = sA[pp * LZ_LD + qq];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double tau = (sA[qq * LZ_LD + qq] - sA[pp * LZ_LD + pp]) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t); s = t * c;
                }
                sc[tid] = c; ss[tid] = s;
            }
            __syncthreads();
            for (int e = tid; e < M * (M / 2); e += BLOCK) {       // T <- T J, S <- S J
                const int i = e / M, row = e % M;
                int pp, qq;
                lz_pair(i, r, M, pp, qq);
                const double c = sc[i], s = ss[i];
                const double ap = sA[row * LZ_LD + pp], aq = sA[row * LZ_LD + qq];
                sA[row * LZ_LD + pp] = c * ap - s * aq; sA[row * LZ_LD + qq] = s * ap + c * aq;
                const double vp = sV[row * LZ_LD + pp], vq = sV[row * LZ_LD + qq];
                sV[row * LZ_LD + pp] = c * vp - s * vq; sV[row * LZ_LD + qq] = s * vp + c * vq;
            }
            __syncthreads();
            for (int e = tid; e < M * (M / 2); e += BLOCK) {       // T <- J^T T
                const int i = e / M, col = e % M;
                int pp, qq;
                lz_pair(i, r, M, pp, qq);
                const double c = sc[i], s = ss[i];
                const double ap = sA[pp * LZ_LD + col], aq = sA[qq * LZ_LD + col];
                sA[pp * LZ_LD + col] = c * ap - s * aq; sA[qq * LZ_LD + col] = s * ap + c * aq;
            }
            __syncthreads();
            if (tid < M / 2) {
                int pp, qq;
                lz_pair(tid, r, M, pp, qq);
                sA[pp * LZ_LD + qq] = 0.0; sA[qq * LZ_LD + pp] = 0.0;
            }
            __syncthreads();
        }
        ++sweeps;
    }
    if (!conv) {
        if (tid == 0) { H.skip = 1; H.status = ST_BREAKDOWN; }
        return;
    }
    lz_rank(me, which == SPRS_EIGSH_LARGEST, [&](int j) { return sA[j * LZ_LD + j]; }, sperm);
    __syncthreads();
    if (tid < me) {
        const int i = sperm[tid];
        const double th = sA[i * LZ_LD + i], rs = beta * fabs(sV[(me - 1) * LZ_LD + i]);
        sth[tid] = th;
        S->theta[tid] = th; S->res[tid] = rs;
    }
    __syncthreads();
    for (int e = tid; e < me * me; e += BLOCK) {
        const int i = e / me, c = e % me;
        S->coef[i * LZ_MAXM + c] = (Real<T>)sV[i * LZ_LD + sperm[c]];
    }
    if (!invariant) {
        // T <- diag(theta_0 .. theta_{p-1}), T_{p,i} = T_{i,p} = beta S[m-1, i] (i < p), zero elsewhere
        for (int e = tid; e < me * me; e += BLOCK) {
            const int r = e / me, c = e % me;
            double v = 0.0;
            if (r == c && r < p) v = sth[r];
            else if (r == p && c < p) v = beta * sV[(me - 1) * LZ_LD + sperm[c]];
            else if (c == p && r < p) v = beta * sV[(me - 1) * LZ_LD + sperm[r]];
            S->Tm[r * LZ_MAXM + c] = v;
        }
    }
    if (tid == 0) lz_verdict(H, sth, sV + (me - 1) * LZ_LD, sperm, me, k, beta, invariant);
}

// ---- LzRotate: out[:, c] = sum_{i < me} V[:, i] coef[i, c] for c < q, from zero, i ascending; out may be V itself.
// A workgroup stages the me x q coefficient block in LDS once, then takes tiles of 64 packs (16 bytes each: 64 rows of c64, 128
// of f64 / c32, 256 of f32): it stages the tile of all me basis vectors in LDS (me KiB; coalesced 16-byte loads, non-temporal
// where NT, all of a thread's loads in flight together) and only then, behind a barrier, forms and stores the q outputs — the
// tile's rows are read by this workgroup alone, so no row of V is written before it has been read.  Lane l of every wavefront
// owns pack l of the tile; wavefront w forms columns CB w .. CB w + CB - 1, CB (w + 4) .. : CB accumulator packs on one LDS
// read of the tile, the coefficients read wave-uniformly (one broadcast LDS read per CB columns).  CB = 2 for q <= 8 (all four
// wavefronts have columns), 4 beyond.
// CF: the coefficients' type, T::Real (Lanczos: S is real for complex A too) or T (LOBPCG, lobpcg_fuse.hpp).  Guard: nothing, or
// one `const int *` to a status word — a launch enqueued blind returns at once unless it reads ST_RUNNING.
template <class T, bool NT, int CB, class CF = Real<T>, class... Guard>
__global__ __launch_bounds__(BLOCK) void lz_rotate_kernel(const CF *__restrict__ cf, const T *V, int64_t vstride, int64_t n, int me, int q,
                                                          T *out, int64_t ostride, int packed_out, Guard... guard) {
    constexpr int PK = pack_width<T>::value, R = WAVE * PK;
    if constexpr (sizeof...(Guard) != 0) {
        const int *const g[] = {guard...};
        if (*g[0] != ST_RUNNING) return;
    }
    extern __shared__ __align__(16) unsigned char lz_tile_raw[];
    Pack<T, PK> *tile = reinterpret_cast<Pack<T, PK> *>(lz_tile_raw);                           // [me][WAVE] packs
    CF *cfs = reinterpret_cast<CF *>(lz_tile_raw + (size_t)me * WAVE * 16);                     // [me][qp], columns q .. qp - 1 zero
    const int qp = (q + CB - 1) / CB * CB;
    for (int e = threadIdx.x; e < me * qp; e += BLOCK) {
        const int i = e / qp, c = e % qp;
        cfs[e] = c < q ? cf[i * LZ_MAXM + c] : CF{};
    }
    const int lane = threadIdx.x & (WAVE - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ntile = (n + R - 1) / R;
    for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
        const int64_t pack0 = t * WAVE;
#pragma unroll 8
        for (int id = threadIdx.x; id < me * WAVE; id += BLOCK) {
            const int i = id >> 6, l = id & (WAVE - 1);
            Pack<T, PK> v;
#pragma unroll
            for (int e = 0; e < PK; ++e) v.v[e] = szero<T>();
            if ((pack0 + l) * PK < n) v = ldp<T, PK, NT>(V + (int64_t)i * vstride, pack0 + l);    // (the basis is padded to whole packs)
            tile[id] = v;
        }
        __syncthreads();
        const int64_t row = (pack0 + lane) * PK;
        for (int c0 = wv * CB; c0 < q; c0 += NWAVE * CB) {
            Pack<T, PK> acc[CB];
#pragma unroll
            for (int b = 0; b < CB; ++b)
#pragma unroll
                for (int e = 0; e < PK; ++e) acc[b].v[e] = szero<T>();
#pragma unroll 4
            for (int i = 0; i < me; ++i) {
                const Pack<T, PK> v = tile[i * WAVE + lane];
                const CF *s = cfs + i * qp + c0;
#pragma unroll
                for (int b = 0; b < CB; ++b) {
                    const CF sb = s[b];
#pragma unroll
                    for (int e = 0; e < PK; ++e) acc[b].v[e] = sadd(acc[b].v[e], smulv(v.v[e], sb));
                }
            }
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                if (c0 + b >= q) break;
                T *o = out + (int64_t)(c0 + b) * ostride;
                if (packed_out && row + PK <= n) stp<T, PK, NT>(o, pack0 + lane, acc[b]);
                else {
#pragma unroll
                    for (int e = 0; e < PK; ++e)
                        if (row + e < n) o[row + e] = acc[b].v[e];
                }
            }
        }
        __syncthreads();     // the tile is overwritten by the next one
    }
}

// One LzRotate launch on the context's stream: out[:, c] = sum_{i < me} V[:, i] cf[i * LZ_MAXM + c], c < q.  LDS a workgroup: me KiB
// of tile + the coefficient block.
template <class T, class CF, class... Guard>
static int launch_lz_rotate(sprs_ctx *c, const CF *cf, const T *V, int64_t vstride, int64_t n, int me, int q, T *out, int64_t ostride, Guard... guard) {
    constexpr int PK = pack_width<T>::value;
    const int64_t ntile = (n + WAVE * PK - 1) / (WAVE * PK);
    const int cb = q <= 8 ? 2 : 4, qp = (q + cb - 1) / cb * cb;
    const size_t lds = (size_t)me * WAVE * 16 + (size_t)me * qp * sizeof(CF);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, ((size_t)160 << 10) / lds));    // workgroups a CU's 160 KiB of LDS holds
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ntile, (int64_t)c->num_cu * per_cu));
    const int packed = (aligned16(out) && (ostride * (int64_t)sizeof(T)) % 16 == 0) ? 1 : 0;
    const bool nt = stream_loads_nt(c, (size_t)n * sizeof(T));
    hipError_t attr = hipSuccess;
    auto launch = [&](auto kernel) {
        // more dynamic LDS than the default 64 KiB limit of a launch (ncv near 64): raise the kernel's limit first
        if (lds > ((size_t)64 << 10)) attr = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
        if (attr != hipSuccess) return;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, c->stream, cf, V, vstride, n, me, q, out, ostride, packed, guard...);
    };
    if (cb == 2) { if (nt) launch(lz_rotate_kernel<T, true, 2, CF, Guard...>); else launch(lz_rotate_kernel<T, false, 2, CF, Guard...>); }
    else { if (nt) launch(lz_rotate_kernel<T, true, 4, CF, Guard...>); else launch(lz_rotate_kernel<T, false, 4, CF, Guard...>); }
    SPRS_HIP_TRY(c, attr);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

// ======================================================================= the frame of a thick-restart solve (Eigsh, Svds)
// Before the first launch: the device state zeroed, the head's status / skip / k / which / tol set and pushed.
// (Block: the solver's StateBlock of LzState<T> or SvState<T>, krylov.hpp)
template <class Block, class R>
static int lz_begin(Block &state, size_t k, int which, R tol) {
    using St = std::remove_pointer_t<decltype(state.host)>;
    SPRS_HIP_TRY(state.ctx, hipMemsetAsync(state.dev, 0, sizeof(St), state.ctx->stream));
    memset(state.host, 0, offsetof(St, h));
    auto &H = state.host->hd;
    H.status = ST_RUNNING; H.skip = 1; H.k = (int)k; H.which = which; H.tol = (double)tol;
    return state.push(sizeof(H));
}
// Behind the last cycle: everything before h fetched, the counters and the k values (vals: the state's theta or sigma) and
// residual estimates copied out.  Returns what the solve returns once its vectors are out; SPRS_BREAKDOWN: there are none.
template <class Block, class R>
static int lz_results(Block &state, size_t k, const double *vals, R *vals_out, R *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out) {
    using St = std::remove_pointer_t<decltype(state.host)>;
    SPRS_TRY(state.fetch(offsetof(St, h)));
    const auto &H = state.host->hd;
    *nconv_out = (size_t)H.nconv; *restarts_out = (size_t)H.cycle; *matvecs_out = (size_t)H.matvecs;
    for (size_t i = 0; i < k; ++i) { vals_out[i] = (R)vals[i]; res_out[i] = (R)state.host->res[i]; }
    if (H.status == ST_BREAKDOWN) return SPRS_BREAKDOWN;
    return H.status == ST_CONVERGED ? SPRS_OK : SPRS_INSUFFICIENT_ITER;
}

}  // namespace sprs
