// Restarted GMRES' vector kernels and its single-workgroup scalar kernel (the solver itself: Gmres<T> in gmres.hip).  No
// reference analogue — the recurrence is the one stated in the header (sprs_gmres_*).  One Arnoldi step j of a fused cycle:
//   [GmPrec   z = M^-1 v_j]                                              (Jacobi only)
//   SpMV      w = A z                                                    (KrylovBase::spmv, any route)
//   launch_cgs2 (below: the one host sequence of every solver that orthogonalises against a basis), cnt = j + 1:
//     GmDots    partials of conj(v_i).w, i <= j: B = gm_b<T> basis vectors per launch, ceil((j + 1) / B) launches, ONE read of w each
//     GmUpdate  h_i from the partials (every workgroup, same order) ; w -= sum v_i h_i in one pass over w
//     GmDots    the same on the updated w (CGS2's second pass)
//     GmUpdate  c_i ; h_i += c_i ; w -= sum v_i c_i written straight into the slot of v_{j+1} ; partials of |w|^2
//   GmStep    (one workgroup) hn = |w| ; the rotations ; g ; its ; the step's events ; at a cycle's end the back substitution
//   GmScale   v_{j+1} *= 1 / hn
// and per cycle  SpMV (A x), GmResid (v_0 = rhs - A x, partials of its norm), GmStart (beta, convergence, g_0), GmScale before
// the steps and GmXUpdate (x += [M^-1] sum v_i y_i, one pass over x) after them: 5 + 2 ceil((j + 1) / B) launches a step (one
// more with Jacobi) and 5 a cycle, none per basis vector.
// The conventions are BicgK1 / K3 / K5's and CgKB / KC's: a consumer re-reduces its producer's partials in its prologue (same
// partials, same order in every workgroup => the same bits everywhere), workgroup 0 records the scalars, a state field is never
// read by a launch one of whose OTHER workgroups writes it, and the host reads nothing but the head of the state.  Two words
// steer the launches the host enqueues blind: `status` (the solve is over: every later kernel returns at its first
// instruction) and `skip` (the rest of this cycle's steps are over: set with status, and by a cycle that left its loop early;
// cleared by the next cycle's GmStart).  The x update is keyed on the cycle number its GmStep recorded, so it runs exactly
// once per cycle that made a step, the event's cycle included.
#pragma once
#include <algorithm>

#include "fused_launch.hpp"

namespace sprs {

constexpr int GM_MAXM = SPRS_GMRES_MAX_RESTART;
// basis vectors per GmDots launch = accumulators and 16-byte loads in flight per lane: 8, and 4 for Complex<f64> (a 16-byte
// accumulator each; 8 of them spill to scratch) — the figures per scalar type are in DESIGN §4c
template <class T> struct gm_b { static constexpr int value = 8; };
template <> struct gm_b<cplx> { static constexpr int value = 4; };
constexpr int ST_MAX_ITER = 6;   // status word: its reached max_iter (the other values: internal.hpp)

// What the host reads (every poll_interval() steps) ...
template <class T>
struct GmresHead {
    long long its, max_iter;
    int status, skip;
    int j;                      // the running step of the cycle
    int kx;                     // columns of the x update of cycle x_cycle
    long long x_cycle;          // -1: none yet
    Real<T> r_norm, tol2, scale;   // scale: 1 / beta or 1 / hn for GmScale
    Real<T> tr_g, tr_hn, tr_c;  // the last step's trace row
    T tr_r, tr_s;
};
// ... and the rest of the device-resident scalar state
template <class T>
struct GmresState {
    GmresHead<T> hd;
    T h[GM_MAXM + 1];           // the running Hessenberg column
    T g[GM_MAXM + 1], s[GM_MAXM], y[GM_MAXM];
    Real<T> c[GM_MAXM];
    T R[GM_MAXM * (GM_MAXM + 1) / 2];   // packed upper triangle, column by column: R_ij at j (j + 1) / 2 + i
};

// cnt coefficients, each the sum of P partials at part[i * pstride ..]: wavefront w reduces coefficients w, w + 4, ... (lane l
// adds partials l, l + 64, ... in order, then the butterfly) — a fixed order, no barrier per coefficient
template <class T>
__device__ __forceinline__ void reduce_coefs(const T *__restrict__ part, int64_t pstride, int P, int cnt, T *out) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
    for (int i = wv; i < cnt; i += NWAVE) {
        T acc = szero<T>();
        for (int p = lane; p < P; p += WAVE) acc = sadd(acc, part[i * pstride + p]);
        acc = wave_sum(acc);
        if (lane == 0) out[i] = acc;
    }
    __syncthreads();
}

// ---- GmDots: partials of conj(v_{i0 + b}).w for b < nb <= B, one pass over w and the nb basis vectors
// (H: the head that carries `skip` — GMRES's, or the Lanczos eigensolver's LzHead of eigsh_fuse.hpp)
template <class T, int B, class H = GmresHead<T>>
struct GmDots {
    const H *S; const T *V; int64_t vstride; int i0, nb; const T *w; T *part; int pstride;
    T acc[B];
    __device__ __forceinline__ bool prologue() {
        if (S->skip != 0) return false;
#pragma unroll
        for (int b = 0; b < B; ++b) acc[b] = szero<T>();
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        const auto wv = ldp<T, PK, NT>(w, i);
        Pack<T, PK> vv[B];
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (b < nb) vv[b] = ldp<T, PK, NT>(V + (int64_t)(i0 + b) * vstride, i);
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (b < nb) {
#pragma unroll
                for (int e = 0; e < PK; ++e) acc[b] = sadd(acc[b], smul(sconj(vv[b].v[e]), wv.v[e]));
            }
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ T smT[NWAVE];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (b < nb) {                                            // (nb is uniform: every thread meets the same barriers)
                const T s = block_sum(acc[b], smT);
                if (threadIdx.x == 0) part[(int64_t)(i0 + b) * pstride + blockIdx.x] = s;
            }
        }
    }
};

// ---- GmUpdate: the j + 1 coefficients from their partials, then out = w - sum v_i coef_i in one pass.
// SECOND: pass 2 — h_i += c_i in the state, out is the slot of v_{j+1}, partials of |out|^2 for GmStep.
// (St: the state that carries hd.skip and the column h — GMRES's, or LzState of eigsh_fuse.hpp)
template <class T, bool SECOND, class St = GmresState<T>>
struct GmUpdate {
    St *S; const T *part; int64_t pstride; int P; int j;
    const T *V; int64_t vstride; const T *w; T *out; Real<T> *partN; Fin fin;
    T *cf; Real<T> accN;
    __device__ __forceinline__ bool prologue() {
        __shared__ T coef[GM_MAXM];
        const int skip = S->hd.skip;
        reduce_coefs(part, pstride, P, j + 1, coef);
        if (skip != 0) { if (SECOND) fin_idle(fin, false); return false; }
        if (blockIdx.x == 0)
            for (int i = threadIdx.x; i <= j; i += BLOCK) S->h[i] = SECOND ? sadd(S->h[i], coef[i]) : coef[i];
        __syncthreads();
        if (threadIdx.x <= j) coef[threadIdx.x] = sneg(coef[threadIdx.x]);
        __syncthreads();
        cf = coef; accN = 0.0;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto wv = ldp<T, PK, NT>(w, i);
        int c = 0;
        for (; c + 4 <= j + 1; c += 4) {                             // four basis loads in flight
            Pack<T, PK> vv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) vv[u] = ldp<T, PK, NT>(V + (int64_t)(c + u) * vstride, i);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T nh = cf[c + u];
#pragma unroll
                for (int e = 0; e < PK; ++e) wv.v[e] = sadd(wv.v[e], smul(vv[u].v[e], nh));      // axpy(-h_i, v_i, w), i ascending
            }
        }
        for (; c <= j; ++c) {
            const auto vv = ldp<T, PK, NT>(V + (int64_t)c * vstride, i);
            const T nh = cf[c];
#pragma unroll
            for (int e = 0; e < PK; ++e) wv.v[e] = sadd(wv.v[e], smul(vv.v[e], nh));
        }
        if (SECOND) {
#pragma unroll
            for (int e = 0; e < PK; ++e) accN = accN + ssq(wv.v[e]);
        }
        stp<T, PK, NT>(out, i, wv);
    }
    __device__ __forceinline__ void epilogue() {
        if (!SECOND) return;
        __shared__ Real<T> smD[NWAVE];
        const Real<T> sN = block_sum(accN, smD);
        if (threadIdx.x == 0) st_partial(fin, partN + blockIdx.x, sN);
        if (fin.counter) finalize_last_block<Real<T>, Real<T>>(fin, false, smD, smD);
    }
};

// Where a GmUpdate finds the coefficients of the GmDots pass before it: cnt sums of P partials at part[i * pstride ..].
template <class T> struct GmCoefs { const T *part; int64_t pstride; int P; };
// launch_cgs2's hook after each GmDots pass: the partials stay where GmDots left them
struct GmDotsInPlace { template <class T> int operator()(int, GmCoefs<T> *) const { return SPRS_OK; } };

// CGS2 of w (len entries) against the cnt >= 1 vectors of `basis`, every solver's one Gram-Schmidt sequence: ceil(cnt / gm_b<T>)
// GmDots (i0 ascending), GmUpdate in place on w, the same GmDots again, GmUpdate<SECOND> into `out` with the partials of |out|^2
// in partN (reduced in the launch where `fin` says so).  St: the state that carries hd.skip and the column h.  dots: cnt x grid
// partials (DotsBuf of krylov.hpp).  after_dots(cnt, &cf) runs behind each GmDots pass and may move the coefficients (GMRES on a
// distributed operator: reduced and all-reduced into one value each); it is called before the GmUpdate that reads them is built.
template <class T, class St, class After = GmDotsInPlace>
static int launch_cgs2(sprs_ctx *c, size_t len, int grid, int cw, St *d_state, const T *basis, int64_t bs, int cnt, T *w, T *out, Real<T> *partN,
                       T *dots, Fin fin = Fin{}, After after_dots = After{}) {
    constexpr int B = gm_b<T>::value;
    using Hd = decltype(St::hd);
    GmCoefs<T> cf{dots, grid, grid};
    auto multi_dot = [&]() -> int {
        for (int i0 = 0; i0 < cnt; i0 += B)
            SPRS_TRY(launch_fused<T>(c, len, grid, cw, GmDots<T, B, Hd>{&d_state->hd, basis, bs, i0, std::min(B, cnt - i0), w, dots, grid, {}}));
        return after_dots(cnt, &cf);
    };
    SPRS_TRY(multi_dot());
    SPRS_TRY(launch_fused<T>(c, len, grid, cw, GmUpdate<T, false, St>{d_state, cf.part, cf.pstride, cf.P, cnt - 1, basis, bs, w, w, nullptr, Fin{}, nullptr, 0.0}));
    SPRS_TRY(multi_dot());
    return launch_fused<T>(c, len, grid, cw, GmUpdate<T, true, St>{d_state, cf.part, cf.pstride, cf.P, cnt - 1, basis, bs, w, out, partN, fin, nullptr, 0.0});
}

// ---- GmResid: v_0 = rhs*1 + v_0*(-1) (v_0 holds A x) + partials of its norm for GmStart
template <class T>
struct GmResid {
    const GmresHead<T> *S; const T *rhs; T *v0; Real<T> *partN; Fin fin;
    T one, mone; Real<T> accN;
    __device__ __forceinline__ bool prologue() {
        if (S->status != ST_RUNNING) { fin_idle(fin, false); return false; }
        one = sone<T>(); mone = sneg(sone<T>()); accN = 0.0;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        const auto bv = ldp<T, PK, NT>(rhs, i); auto rv = ldp<T, PK, NT>(v0, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            rv.v[e] = sadd(smul(bv.v[e], one), smul(rv.v[e], mone));      // axpby(1, rhs, -1, v_0)
            accN = accN + ssq(rv.v[e]);
        }
        stp<T, PK, NT>(v0, i, rv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<T> smD[NWAVE];
        const Real<T> sN = block_sum(accN, smD);
        if (threadIdx.x == 0) st_partial(fin, partN + blockIdx.x, sN);
        if (fin.counter) finalize_last_block<Real<T>, Real<T>>(fin, false, smD, smD);
    }
};

// ---- GmScale: v *= scale (1 / beta, 1 / hn: recorded by GmStart / GmStep, launches of their own)
template <class T, class H = GmresHead<T>>
struct GmScale {
    const H *S; T *v;
    Real<T> a;
    __device__ __forceinline__ bool prologue() {
        const int skip = S->skip;
        a = S->scale;
        return skip == 0;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto xv = ldp<T, PK, NT>(v, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) xv.v[e] = smulr(xv.v[e], a);
        stp<T, PK, NT>(v, i, xv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ---- GmPrec: z = M^-1 v_j
template <class T, class V>
struct GmPrec {
    const GmresHead<T> *S; const V *dinv; const T *v; T *z;
    __device__ __forceinline__ bool prologue() const { return S->skip == 0; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto xv = ldp<T, PK, NT>(v, i); const auto dv = ldp<V, PK, NT>(dinv, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) xv.v[e] = smulv(xv.v[e], dv.v[e]);
        stp<T, PK, NT>(z, i, xv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ---- GmXUpdate: u = sum_{i < k} v_i y_i (from zero, i ascending) ; [u = M^-1 u] ; x += u*1 — for the cycle GmStep recorded
template <class T, class V, bool PC>
struct GmXUpdate {
    const GmresState<T> *S; long long cycle; const T *Vb; int64_t vstride; const V *dinv; T *x;
    const T *yv; int k;
    __device__ __forceinline__ bool prologue() {
        __shared__ T ys[GM_MAXM];
        const long long xc = S->hd.x_cycle;
        k = S->hd.kx;
        if (threadIdx.x < GM_MAXM) ys[threadIdx.x] = S->y[threadIdx.x];
        __syncthreads();
        yv = ys;
        return xc == cycle && k > 0;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto xv = ldp<T, PK, NT>(x, i);
        [[maybe_unused]] Pack<V, PK> dv;
        if (PC) dv = ldp<V, PK, NT>(dinv, i);
        Pack<T, PK> u;
#pragma unroll
        for (int e = 0; e < PK; ++e) u.v[e] = szero<T>();
        int c = 0;
        for (; c + 4 <= k; c += 4) {
            Pack<T, PK> vv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) vv[q] = ldp<T, PK, NT>(Vb + (int64_t)(c + q) * vstride, i);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const T yy = yv[c + q];
#pragma unroll
                for (int e = 0; e < PK; ++e) u.v[e] = sadd(u.v[e], smul(vv[q].v[e], yy));         // axpy(y_i, v_i, u)
            }
        }
        for (; c < k; ++c) {
            const auto vv = ldp<T, PK, NT>(Vb + (int64_t)c * vstride, i);
            const T yy = yv[c];
#pragma unroll
            for (int e = 0; e < PK; ++e) u.v[e] = sadd(u.v[e], smul(vv.v[e], yy));
        }
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            T uu = u.v[e];
            if (PC) uu = smulv(uu, dv.v[e]);
            xv.v[e] = sadd(xv.v[e], smul(uu, sone<T>()));                                        // axpy(1, u, x)
        }
        stp<T, PK, NT>(x, i, xv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ---- GmUForm / GmXAdd (applied preconditioners only: ILU(0), AMG): GmXUpdate in two halves around u = P u, both keyed on the
// cycle GmStep recorded.  GmUForm: u = sum_{i < k} v_i y_i (from zero, i ascending).  GmXAdd: x += u*1.
template <class T>
struct GmUForm {
    const GmresState<T> *S; long long cycle; const T *Vb; int64_t vstride; T *u;
    const T *yv; int k;
    __device__ __forceinline__ bool prologue() {
        __shared__ T ys[GM_MAXM];
        const long long xc = S->hd.x_cycle;
        k = S->hd.kx;
        if (threadIdx.x < GM_MAXM) ys[threadIdx.x] = S->y[threadIdx.x];
        __syncthreads();
        yv = ys;
        return xc == cycle && k > 0;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        Pack<T, PK> uv;
#pragma unroll
        for (int e = 0; e < PK; ++e) uv.v[e] = szero<T>();
        for (int c = 0; c < k; ++c) {
            const auto vv = ldp<T, PK, NT>(Vb + (int64_t)c * vstride, i);
            const T yy = yv[c];
#pragma unroll
            for (int e = 0; e < PK; ++e) uv.v[e] = sadd(uv.v[e], smul(vv.v[e], yy));             // axpy(y_i, v_i, u)
        }
        stp<T, PK, NT>(u, i, uv);
    }
    __device__ __forceinline__ void epilogue() const {}
};
template <class T>
struct GmXAdd {
    const GmresState<T> *S; long long cycle; const T *u; T *x;
    __device__ __forceinline__ bool prologue() const { return S->hd.x_cycle == cycle && S->hd.kx > 0; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto xv = ldp<T, PK, NT>(x, i); const auto uv = ldp<T, PK, NT>(u, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) xv.v[e] = sadd(xv.v[e], smul(uv.v[e], sone<T>()));          // axpy(1, u, x)
        stp<T, PK, NT>(x, i, xv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ======================================================================= the O(m) scalar work: one workgroup, thread 0
// The header's scalar lines, shared by the kernel and the literal mode's host loop (same operations, same order).
// Rotations 0 .. j-1 on the column h[0 .. j], rotation j from (h[j], hn), g; R's column j.  Returns |g_{j+1}|.
template <class T>
SPRS_HD Real<T> gm_rotate(int j, T *h, Real<T> hn, Real<T> *c, T *s, T *g, T *Rcol) {
    for (int i = 0; i < j; ++i) {
        const T t = sadd(smulr(h[i], c[i]), smul(s[i], h[i + 1]));
        h[i + 1] = sadd(smul(sneg(sconj(s[i])), h[i]), smulr(h[i + 1], c[i]));
        h[i] = t;
    }
    const T a = h[j];
    const Real<T> aa = sabs(a);
    const Real<T> d = ssqrt(aa * aa + hn * hn);
    if (aa == Real<T>(0)) { c[j] = Real<T>(0); s[j] = sone<T>(); }
    else { c[j] = aa / d; s[j] = smulr(a, (hn / d) / aa); }
    h[j] = sadd(smulr(a, c[j]), smulr(s[j], hn));
    for (int i = 0; i <= j; ++i) Rcol[i] = h[i];
    g[j + 1] = smul(sneg(sconj(s[j])), g[j]);
    g[j] = smulr(g[j], c[j]);
    return sabs(g[j + 1]);
}
// back substitution on the packed R (k columns)
template <class T>
SPRS_HD void gm_backsub(int k, const T *R, const T *g, T *y) {
    for (int i = k - 1; i >= 0; --i) {
        T t = g[i];
        for (int l = i + 1; l < k; ++l) t = ssub(t, smul(R[l * (l + 1) / 2 + i], y[l]));
        y[i] = sdiv(t, R[i * (i + 1) / 2 + i]);
    }
}

// GmStart: beta = |v_0| from GmResid's partials ; converged ? ; its == max_iter ? ; g_0 = beta, scale = 1 / beta, a new cycle
template <class T>
__global__ __launch_bounds__(BLOCK) void gm_start_kernel(GmresState<T> *S, const Real<T> *partN, int P) {
    __shared__ Real<T> smD[NWAVE];
    GmresHead<T> &H = S->hd;
    const int status = H.status;
    const Real<T> sN = reduce_partials(partN, P, smD);
    if (status != ST_RUNNING || threadIdx.x != 0) return;
    const Real<T> beta = ssqrt(sN);
    if (beta <= H.tol2) { H.r_norm = beta; H.skip = 1; H.status = ST_CONVERGED; return; }
    if (H.its >= H.max_iter) { H.skip = 1; H.status = ST_MAX_ITER; return; }
    S->g[0] = sfromr<T>(beta);
    H.scale = Real<T>(1) / beta;
    H.j = 0; H.skip = 0;
}

// GmStep: step j of the cycle.  hn from GmUpdate<SECOND>'s partials, the rotations, g, its, the events; where the cycle's loop
// is left, k, the back substitution and the cycle number for GmXUpdate.  The column, the rotations, g and the earlier columns
// of R are staged in LDS by the whole workgroup; thread 0 does the (serial, fixed-order) arithmetic there.
template <class T>
__global__ __launch_bounds__(BLOCK) void gm_step_kernel(GmresState<T> *S, const Real<T> *partN, int P, int j, int m, long long cycle) {
    __shared__ Real<T> smD[NWAVE];
    __shared__ T sR[GM_MAXM * (GM_MAXM + 1) / 2];
    __shared__ T sh[GM_MAXM + 1], sg[GM_MAXM + 1], ss[GM_MAXM], sy[GM_MAXM];
    __shared__ Real<T> sc[GM_MAXM];
    __shared__ int s_k;         // 0: the loop goes on ; k: it was left with k columns ; -1: breakdown
    GmresHead<T> &H = S->hd;
    const int skip = H.skip;
    const Real<T> sN = reduce_partials(partN, P, smD);
    if (skip != 0) return;
    const int k = j + 1, col = j * (j + 1) / 2;
    for (int e = threadIdx.x; e < col; e += BLOCK) sR[e] = S->R[e];
    if ((int)threadIdx.x <= j) { sh[threadIdx.x] = S->h[threadIdx.x]; sg[threadIdx.x] = S->g[threadIdx.x]; }
    if ((int)threadIdx.x < j) { sc[threadIdx.x] = S->c[threadIdx.x]; ss[threadIdx.x] = S->s[threadIdx.x]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s_k = 0;
        const Real<T> hn = ssqrt(sN);
        if (!(hn >= Real<T>(0))) { H.skip = 1; H.status = ST_BREAKDOWN; s_k = -1; }
        else {
            const Real<T> gabs = gm_rotate<T>(j, sh, hn, sc, ss, sg, sR + col);
            const long long its = H.its + 1;
            H.its = its; H.j = k;
            H.tr_g = gabs; H.tr_hn = hn; H.tr_r = sR[col + j]; H.tr_c = sc[j]; H.tr_s = ss[j];
            const bool conv = gabs <= H.tol2, last = its >= H.max_iter;
            if (conv || hn == Real<T>(0) || last || k == m) {
                gm_backsub<T>(k, sR, sg, sy);
                s_k = k;
                H.kx = k; H.x_cycle = cycle;
                H.skip = 1;
                if (conv) { H.r_norm = gabs; H.status = ST_CONVERGED; }
                else if (last) H.status = ST_MAX_ITER;
            } else {
                H.scale = Real<T>(1) / hn;
            }
        }
    }
    __syncthreads();
    if (s_k < 0) return;
    if ((int)threadIdx.x <= j) S->R[col + threadIdx.x] = sR[col + threadIdx.x];
    if (threadIdx.x == 0) { S->c[j] = sc[j]; S->s[j] = ss[j]; S->g[j] = sg[j]; S->g[j + 1] = sg[j + 1]; }
    if ((int)threadIdx.x < s_k) S->y[threadIdx.x] = sy[threadIdx.x];
}

// distributed operators: this rank's cnt coefficients from their [cnt][P] partials into out[0 .. cnt), for the all-reduce
template <class T>
__global__ __launch_bounds__(BLOCK) void gm_reduce_kernel(const GmresHead<T> *S, const T *part, int64_t pstride, int P, int cnt, T *out) {
    __shared__ T coef[GM_MAXM];
    const int skip = S->skip;
    reduce_coefs(part, pstride, P, cnt, coef);
    if ((int)threadIdx.x < cnt) out[threadIdx.x] = skip != 0 ? szero<T>() : coef[threadIdx.x];
}

}  // namespace sprs
