// Thick-restart Lanczos bidiagonalisation (sprs_svds_*): the kernels that are its own (the solver itself: Svds<T> in svds.hip).
// No reference analogue — the recurrence is the one stated in the header.  Op is M x N with M >= N (A, or A^H where A is wide);
// p_0 .. p_l span the small space, q_0 .. q_{l-1} the large one.  One step j of a cycle:
//   SpMV      w = Op p_j
//   launch_cgs2                                     (gmres_fuse.hpp, on SvState: CGS2 against q_0 .. q_{j-1}, into the slot of q_j)
//   SvNorm<false>  (one workgroup) alpha = B_jj, the rank-deficiency threshold, 1 / alpha, the count of products ; sets `skip`
//   GmScale   q_j *= 1 / alpha
//   SpMV      w' = Op^H q_j
//   launch_cgs2                                     (CGS2 against p_0 .. p_j, into the slot of p_{j+1})
//   SvNorm<true>   (one workgroup) beta, the invariant-subspace threshold, B_{j,j+1}, 1 / beta, the count, m_eff ; sets `skip`
//   GmScale   p_{j+1} *= 1 / beta
// per cycle SvSvd (one workgroup: B = X Sigma Y^T by one-sided Jacobi in LDS, the order, res, anorm, nconv, the events, both
// coefficient blocks rounded to T::Real, the restarted B) and, where the host restarts, LzRotate twice (eigsh_fuse.hpp) ; per
// solve LzNrm + LzStart + GmScale before the first cycle and LzRotate twice more for the singular vectors.  At j = 0 of the
// first cycle there is nothing to orthogonalise Op p_0 against: the SpMV writes the slot of q_0 and LzNrm forms the partials.
// The conventions are gmres_fuse.hpp's and eigsh_fuse.hpp's: partials re-reduced in the same order by every consumer, `status`
// ends the solve and `skip` the rest of a cycle's blind launches, the host reads nothing but the head of the state (once a cycle).
#pragma once
#include "eigsh_fuse.hpp"

namespace sprs {

static_assert(SPRS_SVDS_MAX_NCV == LZ_MAXM, "LzRotate reads the coefficient blocks with leading dimension LZ_MAXM");
constexpr int SV_MAX_SWEEPS = 30;
constexpr int SV_TP = 8;                    // SvSvd: threads per column pair (32 pairs at M = 64: all 256 threads)

// What the host reads once a cycle is LzHead (matvecs: products with either operator ; pscale: the largest entry of B so far) ;
// what it reads besides when the solve is over (sigma, res: everything before h) and the rest of the device-resident state.
// B is real upper triangular whatever the scalar type, and is kept in double.
template <class T>
struct SvState {
    LzHead<T> hd;
    double sigma[LZ_MAXM], res[LZ_MAXM];     // the singular values in the order of `which` and their residual estimates
    T h[LZ_MAXM];                            // GmUpdate's running column of CGS2 coefficients
    double Bm[LZ_MAXM * LZ_MAXM];            // row-major, leading dimension LZ_MAXM
    Real<T> coefY[LZ_MAXM * LZ_MAXM];        // coefY[i * LZ_MAXM + c] = Y[i, c] rounded once to T::Real, columns in the order of `which`
    Real<T> coefX[LZ_MAXM * LZ_MAXM];        // the same of X
};

// SvNorm: half-step j of cycle `cycle`, the norm from GmUpdate<SECOND>'s (at j = 0 of the first cycle: LzNrm's) partials.
// BETA = false: alpha = |w| = B_jj ; at or under the threshold Op is rank-deficient along the basis: breakdown.
// BETA = true:  beta = |w'| ; at or under the threshold an invariant subspace (p_{j+1} is not formed) ; else B_{j,j+1}.
template <class T, bool BETA>
__global__ __launch_bounds__(BLOCK) void sv_norm_kernel(SvState<T> *S, const Real<T> *partN, int P, int j, int m, long long cycle) {
    __shared__ Real<T> smD[NWAVE];
    LzHead<T> &H = S->hd;
    const int skip = H.skip;
    const Real<T> sN = reduce_partials(partN, P, smD);
    if (skip != 0 || threadIdx.x != 0) return;
    const double v = (double)ssqrt(sN), sc = H.pscale;
    H.matvecs += 1; H.cycle = cycle;
    if (!(v >= 0.0)) { H.skip = 1; H.status = ST_BREAKDOWN; return; }
    const bool small = v <= 64.0 * (double)seps<Real<T>>() * sc;
    if (!BETA) {
        if (small) { H.skip = 1; H.status = ST_BREAKDOWN; return; }
        S->Bm[j * LZ_MAXM + j] = v;
    } else {
        if (small) {                                        // the residuals are zero
            H.beta = 0.0; H.m_eff = j + 1; H.invariant = 1; H.skip = 1;
            return;
        }
        H.beta = v;
        if (j + 1 < m) S->Bm[j * LZ_MAXM + j + 1] = v;
        else H.m_eff = m;
    }
    H.pscale = fmax(sc, v);
    H.scale = Real<T>(1) / ssqrt(sN);
}

// SvSvd: B[:m_eff, :m_eff] = X Sigma Y^T by one-sided (Hestenes) Jacobi on the columns of G = B with Y = I, both in LDS in
// double (row stride LZ_LD: a column walk meets every bank once).  m_eff is rounded up to an even M (an odd m_eff carries one
// zero column, which never rotates).  A sweep is M - 1 rounds in the round-robin order of lz_pair; per round, for each of the
// M / 2 disjoint pairs (p, q): a = |g_p|^2, b = |g_q|^2, c = g_p.g_q — SV_TP threads a pair, thread t summing rows t, t + SV_TP, ..
// in order, the SV_TP partial sums added in order — and, only where |c| > eps sqrt(a b), the rotation that makes the two columns
// orthogonal, applied to G and Y by one thread per (row, pair).  The Gram matrix is never formed: sigma and X keep relative
// accuracy for the small singular values.  A sweep without a rotation ends the iteration; SV_MAX_SWEEPS sweeps with one is a
// breakdown.  Then sigma_i = |g_i|, x_i = g_i / sigma_i, the order of `which`, res, anorm, nconv, the events, the coefficient
// blocks and the restarted B (p kept triplets + the spike column).  Every element is written by one thread per phase and every
// sum has a fixed order: the result does not depend on timing.
template <class T>
__global__ __launch_bounds__(BLOCK) void sv_svd_kernel(SvState<T> *S, int m, int p) {
    __shared__ double sG[LZ_MAXM * LZ_LD], sY[LZ_MAXM * LZ_LD];
    __shared__ double sa[LZ_MAXM / 2 * SV_TP], sb[LZ_MAXM / 2 * SV_TP], scc[LZ_MAXM / 2 * SV_TP];
    __shared__ double scs[LZ_MAXM / 2], ssn[LZ_MAXM / 2], ssig[LZ_MAXM];
    __shared__ int sperm[LZ_MAXM], srot[LZ_MAXM / 2], sflag[2];
    LzHead<T> &H = S->hd;
    if (H.status != ST_RUNNING) return;
    const int tid = threadIdx.x, me = H.m_eff, M = (me + 1) & ~1, np2 = M / 2;
    const int k = H.k, which = H.which, invariant = H.invariant;
    const double beta = H.beta, eps = seps<double>();
    for (int e = tid; e < M * M; e += BLOCK) {
        const int r = e / M, c = e % M;
        sG[r * LZ_LD + c] = (r < me && c < me) ? S->Bm[r * LZ_MAXM + c] : 0.0;
        sY[r * LZ_LD + c] = r == c ? 1.0 : 0.0;
    }
    if (tid == 0) sflag[0] = 0;
    __syncthreads();
    int sweeps = 0;
    bool conv = false;
    const int pi = tid / SV_TP, pt = tid % SV_TP;           // this thread's pair and its share of the pair's rows
    for (;;) {
        for (int r = 0; r < M - 1; ++r) {
            if (pi < np2) {
                int pp, qq;
                lz_pair(pi, r, M, pp, qq);
                double a = 0.0, b = 0.0, c = 0.0;
                for (int row = pt; row < M; row += SV_TP) {
                    const double gp = sG[row * LZ_LD + pp], gq = sG[row * LZ_LD + qq];
                    a += gp * gp; b += gq * gq; c += gp * gq;
                }
                sa[tid] = a; sb[tid] = b; scc[tid] = c;
            }
            __syncthreads();
            if (tid < np2) {
                double a = 0.0, b = 0.0, c = 0.0;
                for (int t = 0; t < SV_TP; ++t) { a += sa[tid * SV_TP + t]; b += sb[tid * SV_TP + t]; c += scc[tid * SV_TP + t]; }
                double cs = 1.0, sn = 0.0;
                int rot = 0;
                if (fabs(c) > eps * sqrt(a * b)) {
                    const double zeta = (b - a) / (2.0 * c);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    cs = 1.0 / sqrt(1.0 + t * t); sn = cs * t;
                    rot = 1;
                }
                scs[tid] = cs; ssn[tid] = sn; srot[tid] = rot;
            }
            __syncthreads();
            for (int e = tid; e < M * np2; e += BLOCK) {            // G <- G J, Y <- Y J
                const int i = e / M, row = e % M;
                if (srot[i] == 0) continue;
                int pp, qq;
                lz_pair(i, r, M, pp, qq);
                const double cs = scs[i], sn = ssn[i];
                const double gp = sG[row * LZ_LD + pp], gq = sG[row * LZ_LD + qq];
                sG[row * LZ_LD + pp] = cs * gp - sn * gq; sG[row * LZ_LD + qq] = sn * gp + cs * gq;
                const double yp = sY[row * LZ_LD + pp], yq = sY[row * LZ_LD + qq];
                sY[row * LZ_LD + pp] = cs * yp - sn * yq; sY[row * LZ_LD + qq] = sn * yp + cs * yq;
            }
            if (tid < np2 && srot[tid] != 0) sflag[0] = 1;           // (every writer writes the same value)
            __syncthreads();
        }
        const int rotated = sflag[0];
        __syncthreads();
        if (tid == 0) sflag[0] = 0;
        __syncthreads();
        if (rotated == 0) { conv = true; break; }
        if (++sweeps == SV_MAX_SWEEPS) break;
    }
    // sigma_i = |g_i| (rows ascending) ; zero or NaN: breakdown
    if (tid == 0) sflag[1] = 0;
    __syncthreads();
    if (tid < me) {
        double s2 = 0.0;
        for (int row = 0; row < me; ++row) { const double g = sG[row * LZ_LD + tid]; s2 += g * g; }
        const double sg = sqrt(s2);
        ssig[tid] = sg;
        if (!(sg > 0.0)) sflag[1] = 1;
    }
    __syncthreads();
    if (!conv || sflag[1] != 0) {
        if (tid == 0) { H.skip = 1; H.status = ST_BREAKDOWN; }
        return;
    }
    lz_rank(me, which == SPRS_SVDS_LARGEST, [&](int j) { return ssig[j]; }, sperm);
    __syncthreads();
    for (int e = tid; e < me * me; e += BLOCK) {                    // X = G Sigma^-1, in place
        const int row = e / me, c = e % me;
        sG[row * LZ_LD + c] = sG[row * LZ_LD + c] / ssig[c];
    }
    __syncthreads();
    if (tid < me) {
        const int i = sperm[tid];
        S->sigma[tid] = ssig[i]; S->res[tid] = beta * fabs(sG[(me - 1) * LZ_LD + i]);
    }
    for (int e = tid; e < me * me; e += BLOCK) {
        const int i = e / me, c = e % me;
        S->coefY[i * LZ_MAXM + c] = (Real<T>)sY[i * LZ_LD + sperm[c]];
        S->coefX[i * LZ_MAXM + c] = (Real<T>)sG[i * LZ_LD + sperm[c]];
    }
    if (!invariant) {
        // B <- diag(sigma_0 .. sigma_{p-1}), the spike column B_{i,p} = beta X[m-1, i] (i < p), zero elsewhere
        for (int e = tid; e < me * me; e += BLOCK) {
            const int r = e / me, c = e % me;
            double v = 0.0;
            if (r == c && r < p) v = ssig[sperm[r]];
            else if (c == p && r < p) v = beta * sG[(me - 1) * LZ_LD + sperm[r]];
            S->Bm[r * LZ_MAXM + c] = v;
        }
    }
    if (tid == 0) lz_verdict(H, ssig, sG + (me - 1) * LZ_LD, sperm, me, k, beta, invariant);
}

}  // namespace sprs
