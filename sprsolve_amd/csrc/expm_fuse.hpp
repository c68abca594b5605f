// The Krylov propagator w = exp(tA) v (sprs_expm_*): the kernels that are its own (the solver itself: Expm<T> in expm.hip).  No
// reference analogue — the recurrence is the one stated in the header.  One sub-step:
//   ExStart   (one workgroup) beta from the partials of |w|^2, the zero / NaN rules, hump, H = 0 ; clears `skip`
//   GmScale   v_0 *= 1 / beta                                             (w lives in the slot of v_0 between sub-steps)
//   m times:  SpMV  p = A v_j                                             (KrylovBase::spmv, any route, no fused dot)
//             launch_cgs2                                                 (gmres_fuse.hpp, on ExState: CGS2 against v_0 .. v_j,
//                                                                          p - sum v_i c_i into the slot of v_{j+1}, partials of its norm)
//             ExArnoldiStep (one workgroup) column j of H, hn, the happy-breakdown rule, the count of products ; sets `skip`
//             GmScale   v_{j+1} *= 1 / hn
//   SpMV + LzNrm   partials of |A v_m|^2                                  (idle after a happy breakdown)
//   ExStep    (one workgroup) avnorm, anorm and the first tau, the reject loop around smallexp in LDS, the coefficient column
//             rounded to T, the next tau, t_now, the counters, the end-of-solve statuses
//   ExCombine out = sum_i v_i c_i in one pass, in place into the slot of v_0 (the access is element-wise) or, on the sub-step that
//             ends the solve, into the caller's w ; partials of |out|^2 for the next ExStart
// The conventions are gmres_fuse.hpp's: partials re-reduced in the same order by every consumer, `status` ends the solve and
// `skip` the rest of a sub-step's Arnoldi launches, the host reads nothing but the head of the state (once a sub-step).
// Every loop of ExStep has a fixed bound — EX_HORNER Horner steps, EX_MAX_SQ squarings, EX_MAX_REJECT rejections, 330 steps of
// round2 — and what decides a trip count is tested for being finite first: the kernel cannot spin.
#pragma once
#include <type_traits>

#include "eigsh_fuse.hpp"

namespace sprs {

constexpr int EX_MAXM = SPRS_EXPM_MAX_NCV;
static_assert(EX_MAXM + 1 <= GM_MAXM, "GmUpdate stages one coefficient per basis vector in an array of GM_MAXM");
constexpr int EX_MAXH = EX_MAXM + 2;        // H and F are (m + 2) x (m + 2)
constexpr int EX_LD = EX_MAXM + 3;          // ExStep's row stride in LDS (odd: a column walk meets every bank once)
constexpr int EX_HORNER = 18, EX_MAX_SQ = 64, EX_MAX_REJECT = 10;
constexpr double EX_GAMMA = 0.9, EX_DELTA = 1.2;

// the projected matrix's scalar: double for real T, complex double for complex T
template <class T> using ExH = std::conditional_t<is_complex<T>::value, cplx, double>;
SPRS_HD double ex_wide(double a) { return a; }
SPRS_HD double ex_wide(float a) { return (double)a; }
SPRS_HD cplx ex_wide(cplx a) { return a; }
SPRS_HD cplx ex_wide(cplxf a) { return cplx{(double)a.re, (double)a.im}; }
template <class T> SPRS_HD T ex_narrow(ExH<T> a);
template <> SPRS_HD double ex_narrow<double>(double a) { return a; }
template <> SPRS_HD float ex_narrow<float>(double a) { return (float)a; }
template <> SPRS_HD cplx ex_narrow<cplx>(cplx a) { return a; }
template <> SPRS_HD cplxf ex_narrow<cplxf>(cplx a) { return cplxf{(float)a.re, (float)a.im}; }
SPRS_HD double ex_divr(double a, double q) { return a / q; }
SPRS_HD cplx ex_divr(cplx a, double q) { return cplx{a.re / q, a.im / q}; }

// What the host reads (once a sub-step) ...
template <class T>
struct ExHead {
    int status, skip;
    int combine;                // ExCombine: 0 nothing to do, 1 into the slot of v_0, 2 into the caller's w (the solve is over)
    int ncoef;                  // terms of the combination: m_eff after a happy breakdown, else m + 1
    int happy, m_eff;
    int zero, pad;              // zero: beta == 0, the answer is w = 0
    long long matvecs, steps, rejects, max_steps;
    Real<T> scale;              // 1 / beta or 1 / hn for GmScale
    double beta, hscale;        // hscale: the happy-breakdown rule's running scale
    double tau, t_now, t_out, sgn, tol, err_sum, hump;      // tau: the next sub-step's proposal (0: not set yet)
};
// ... and the rest of the device-resident state
template <class T>
struct ExState {
    ExHead<T> hd;
    T h[EX_MAXM];                            // GmUpdate's running column of CGS2 coefficients
    T c[EX_MAXM + 1];                        // beta F[:, 0] rounded once to T
    ExH<T> H[EX_MAXH * EX_MAXH];             // row-major, leading dimension EX_MAXH
};

// x to two significant decimal digits, as Expokit rounds its step sizes (the header's round2, operation by operation)
SPRS_HD double ex_round2(double x) {
    if (!(x > 0.0) || !(x < HUGE_VAL)) return x;
    double y = x;
    int u = 0;
    for (int i = 0; i < 330 && y >= 100.0; ++i) { y = y / 10.0; ++u; }
    for (int i = 0; i < 330 && y < 10.0; ++i) { y = y * 10.0; --u; }
    double r = floor(y + 0.55);
    for (int i = 0; i < u; ++i) r = r * 10.0;
    for (int i = 0; i < -u; ++i) r = r / 10.0;
    return r;
}

// ExStart: beta = |w| from the partials of LzNrm (the first sub-step) or ExCombine ; NaN: breakdown ; 0: the answer is zero ;
// hump, scale = 1 / beta, H = 0 and the sub-step's Arnoldi launches may run
template <class T>
__global__ __launch_bounds__(BLOCK) void ex_start_kernel(ExState<T> *S, const Real<T> *partN, int P, int m) {
    __shared__ Real<T> smD[NWAVE];
    ExHead<T> &H = S->hd;
    const int status = H.status;
    const Real<T> sN = reduce_partials(partN, P, smD);
    if (status != ST_RUNNING) return;
    const int M = m + 2;
    for (int e = threadIdx.x; e < M * M; e += BLOCK) S->H[(e / M) * EX_MAXH + e % M] = szero<ExH<T>>();
    if (threadIdx.x != 0) return;
    H.combine = 0;
    const Real<T> beta = ssqrt(sN);
    if (!(beta >= Real<T>(0))) { H.skip = 1; H.status = ST_BREAKDOWN; return; }
    if (beta == Real<T>(0)) { H.skip = 1; H.zero = 1; H.status = ST_CONVERGED; return; }
    H.beta = (double)beta;
    H.hump = fmax(H.hump, (double)beta);
    H.scale = Real<T>(1) / beta;
    H.hscale = 0.0; H.happy = 0; H.m_eff = m;
    H.skip = 0;
}

// ExArnoldiStep: step j of the sub-step.  hn from GmUpdate<SECOND>'s partials, column j of H from the state's h, the
// happy-breakdown rule, the sub-diagonal entry and the scale for GmScale.  (j < 64: the column sits in the first wavefront.)
template <class T>
__global__ __launch_bounds__(BLOCK) void ex_arnoldi_step_kernel(ExState<T> *S, const Real<T> *partN, int P, int j) {
    __shared__ Real<T> smD[NWAVE];
    ExHead<T> &H = S->hd;
    const int skip = H.skip, tid = threadIdx.x;
    const Real<T> sN = reduce_partials(partN, P, smD);
    if (skip != 0 || tid >= WAVE) return;
    double a = 0.0;
    if (tid <= j) {
        const ExH<T> hv = ex_wide(S->h[tid]);
        S->H[tid * EX_MAXH + j] = hv;
        a = sabs(hv);
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) a = fmax(a, __shfl_xor(a, off, WAVE));
    if (tid != 0) return;
    const double hn = (double)ssqrt(sN);
    H.matvecs += 1;
    if (!(hn >= 0.0)) { H.skip = 1; H.status = ST_BREAKDOWN; return; }
    double sc = fmax(H.hscale, a);
    if (hn <= 64.0 * (double)seps<Real<T>>() * sc) {         // a happy breakdown: v_{j+1} is not formed
        H.hscale = sc; H.m_eff = j + 1; H.happy = 1; H.skip = 1;
        return;
    }
    sc = fmax(sc, hn);
    H.hscale = sc;
    S->H[(j + 1) * EX_MAXH + j] = ex_wide(sfromr<T>(ssqrt(sN)));
    H.scale = Real<T>(1) / ssqrt(sN);
}

// One product of the small exponential: out[i, k] = diag (i == k) + (sum_j A[i, j] B[j, k]) / q for the M x M matrices in LDS,
// j ascending, one product and one sum per term, one thread per entry.
template <class HT>
__device__ __forceinline__ void ex_matmul(const HT *A, const HT *B, HT *out, int M, double diag, double q) {
    for (int e = threadIdx.x; e < M * M; e += BLOCK) {
        const int i = e / M, k = e % M;
        HT acc = szero<HT>();
        for (int j = 0; j < M; ++j) acc = sadd(acc, smul(A[i * EX_LD + j], B[j * EX_LD + k]));
        acc = ex_divr(acc, q);
        if (i == k) acc = sadd(acc, sfromr<HT>(diag));
        out[i * EX_LD + k] = acc;
    }
    __syncthreads();
}

// ExStep: everything of a sub-step after its Arnoldi loop (the header's lines from `happy:` on).  Three M x EX_LD matrices in
// dynamic LDS: Y = sgn tau_s H 2^-s and the two sides of the Horner / squaring ping-pong.  Thread 0 does the scalar control and
// hands its verdict over in LDS; the products are spread over the workgroup.  No atomics, every sum in a fixed order.
template <class T>
__global__ __launch_bounds__(BLOCK) void ex_step_kernel(ExState<T> *S, const Real<T> *partN, int P, int m) {
    using HT = ExH<T>;
    extern __shared__ __align__(16) unsigned char ex_lds_raw[];
    __shared__ Real<T> smD[NWAVE];
    __shared__ double s_sum[EX_MAXH];
    __shared__ double s_tau;                 // tau_s of the running attempt
    __shared__ int s_verdict;                // 0: the attempt is accepted ; 1: rejected, s_tau holds the next one ; 2: breakdown
    ExHead<T> &H = S->hd;
    const int status = H.status, happy = H.happy, tid = threadIdx.x;
    const Real<T> sA = reduce_partials(partN, P, smD);
    if (status != ST_RUNNING) return;
    const int M = happy ? H.m_eff : m + 2;
    HT *Y = reinterpret_cast<HT *>(ex_lds_raw), *Ea = Y + (size_t)(m + 2) * EX_LD, *Eb = Ea + (size_t)(m + 2) * EX_LD;
    const double beta = H.beta, tol = H.tol, sgn = H.sgn, rem = H.t_out - H.t_now, avnorm = (double)ssqrt(sA);
    const double tau_old = H.tau;
    if (!happy) {
        // anorm: the largest row sum of |H[:m+1, :m]| (used where tau is not set yet)
        if (tid <= m) {
            double r = 0.0;
            for (int c = 0; c < m; ++c) r = r + sabs(S->H[tid * EX_MAXH + c]);
            s_sum[tid] = r;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double tau_s = rem;
        if (!happy) {
            H.matvecs += 1;
            double tau = tau_old;
            if (tau == 0.0) {
                double anorm = 0.0;
                for (int r = 0; r <= m; ++r) anorm = fmax(anorm, s_sum[r]);
                const double m1 = (double)(m + 1);
                const double fact = pow(m1 / 2.718281828459045, m1) * sqrt(2.0 * 3.141592653589793 * m1);
                tau = ex_round2((1.0 / anorm) * pow((fact * tol) / (4.0 * beta * anorm), 1.0 / (double)m));
            }
            tau_s = tau < rem ? tau : rem;
        }
        s_tau = tau_s;
    }
    __syncthreads();
    double err = 0.0, xm = 0.0, tau_s = 0.0;
    const HT *F = Ea;
    for (int rej = 0;; ++rej) {              // EX_MAX_REJECT attempts at the most: the verdict of attempt EX_MAX_REJECT - 1 is 0 or 2
        tau_s = s_tau;
        const double f = sgn * tau_s;
        for (int e = tid; e < M * M; e += BLOCK) {
            const int i = e / M, k = e % M;
            const HT hv = (!happy && i == m + 1 && k == m) ? sfromr<HT>(1.0) : S->H[i * EX_MAXH + k];       // H[m+1, m] = 1
            Y[i * EX_LD + k] = smulr(hv, f);
        }
        __syncthreads();
        if (tid < M) {
            double cs = 0.0;
            for (int i = 0; i < M; ++i) cs = cs + sabs(Y[i * EX_LD + tid]);
            s_sum[tid] = cs;
        }
        __syncthreads();
        double nrm = 0.0;
        bool finite = true;
        for (int k = 0; k < M; ++k) {
            const double cs = s_sum[k];
            finite = finite && cs < HUGE_VAL;        // (false for a NaN too)
            nrm = fmax(nrm, cs);
        }
        double x = nrm, g = 1.0;
        int s = 0;
        if (finite)
            for (; s < EX_MAX_SQ && x > 0.5; ++s) { x = x * 0.5; g = g * 0.5; }
        if (!finite || x > 0.5) {            // (uniform: every thread holds the same sums)
            if (tid == 0) { H.skip = 1; H.status = ST_BREAKDOWN; }
            return;
        }
        for (int e = tid; e < M * M; e += BLOCK) {
            const int i = e / M, k = e % M;
            Y[i * EX_LD + k] = smulr(Y[i * EX_LD + k], g);
            Ea[i * EX_LD + k] = i == k ? sfromr<HT>(1.0) : szero<HT>();
        }
        __syncthreads();
        HT *src = Ea, *dst = Eb;
        for (int q = EX_HORNER; q >= 1; --q) {               // E = I + (Y E) / q
            ex_matmul<HT>(Y, src, dst, M, 1.0, (double)q);
            HT *t = src; src = dst; dst = t;
        }
        for (int i = 0; i < s; ++i) {                        // E = E E
            ex_matmul<HT>(src, src, dst, M, 0.0, 1.0);
            HT *t = src; src = dst; dst = t;
        }
        F = src;
        if (happy) break;                                    // err = 0: the Krylov space is invariant
        if (tid == 0) {
            const double e1 = beta * sabs(F[m * EX_LD]), e2 = beta * sabs(F[(m + 1) * EX_LD]) * avnorm;
            if (e1 > 10.0 * e2) { err = e2; xm = 1.0 / (double)m; }
            else if (e1 > e2) { err = e1 * e2 / (e1 - e2); xm = 1.0 / (double)m; }
            else { err = e1; xm = 1.0 / (double)(m - 1); }
            int verdict = 1;
            if (err != err) verdict = 2;
            else if (err <= EX_DELTA * tau_s * tol) verdict = 0;
            else if (rej == EX_MAX_REJECT - 1) verdict = 2;
            else {
                const double next = ex_round2(EX_GAMMA * tau_s * pow(tau_s * tol / err, xm));
                if (!(next > 0.0) || !(next < HUGE_VAL)) verdict = 2;
                else { s_tau = next; H.rejects += 1; }
            }
            s_verdict = verdict;
        }
        __syncthreads();
        const int verdict = s_verdict;
        if (verdict == 2) {
            if (tid == 0) { H.skip = 1; H.status = ST_BREAKDOWN; }
            return;
        }
        if (verdict == 0) break;
    }
    const int ncoef = happy ? M : m + 1;
    if (tid < ncoef) S->c[tid] = ex_narrow<T>(smulr(F[tid * EX_LD], beta));
    if (tid != 0) return;
    if (!happy) H.tau = ex_round2(EX_GAMMA * tau_s * pow(tau_s * tol / fmax(err, 2.2250738585072014e-308), xm));
    const double t_now = tau_s == rem ? H.t_out : H.t_now + tau_s;
    const long long steps = H.steps + 1;
    H.t_now = t_now; H.err_sum += err; H.steps = steps; H.ncoef = ncoef;
    H.skip = 1;
    if (t_now >= H.t_out) { H.combine = 2; H.status = ST_CONVERGED; }
    else if (steps == H.max_steps) { H.combine = 2; H.status = ST_MAX_ITER; }
    else H.combine = 1;
}

// ---- ExCombine: out = sum_{i < ncoef} v_i c_i (from zero, i ascending) in one pass, where ExStep asked for it: in place into the
// slot of v_0 — element i of every v is read by the thread that writes element i, so nothing is overwritten before it is read
// — or, on the sub-step that ends the solve, into `last`.  Partials of |out|^2 for the next ExStart.
template <class T>
struct ExCombine {
    const ExState<T> *S; const T *V; int64_t vstride; T *next, *last; Real<T> *partN;
    const T *cf; T *out; int k; Real<T> accN;
    __device__ __forceinline__ bool prologue() {
        __shared__ T cs[EX_MAXM + 1];
        const int mode = S->hd.combine;
        k = S->hd.ncoef;
        if (threadIdx.x <= EX_MAXM) cs[threadIdx.x] = S->c[threadIdx.x];
        __syncthreads();
        cf = cs; out = mode == 2 ? last : next; accN = 0.0;
        return mode != 0;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        Pack<T, PK> u;
#pragma unroll
        for (int e = 0; e < PK; ++e) u.v[e] = szero<T>();
        int c = 0;
        for (; c + 4 <= k; c += 4) {                                 // four basis loads in flight
            Pack<T, PK> vv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) vv[q] = ldp<T, PK, NT>(V + (int64_t)(c + q) * vstride, i);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const T cc = cf[c + q];
#pragma unroll
                for (int e = 0; e < PK; ++e) u.v[e] = sadd(u.v[e], smul(vv[q].v[e], cc));
            }
        }
        for (; c < k; ++c) {
            const auto vv = ldp<T, PK, NT>(V + (int64_t)c * vstride, i);
            const T cc = cf[c];
#pragma unroll
            for (int e = 0; e < PK; ++e) u.v[e] = sadd(u.v[e], smul(vv.v[e], cc));
        }
#pragma unroll
        for (int e = 0; e < PK; ++e) accN = accN + ssq(u.v[e]);
        stp<T, PK, NT>(out, i, u);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<T> smD[NWAVE];
        const Real<T> sN = block_sum(accN, smD);
        if (threadIdx.x == 0) partN[blockIdx.x] = sN;
    }
};

}  // namespace sprs
