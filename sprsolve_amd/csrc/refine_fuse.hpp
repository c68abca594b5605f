// Mixed-precision iterative refinement's vector kernels (the solver itself: Refine<H> in refine.hip).  No reference analogue —
// the recurrence is the one stated in the header (sprs_refine_*).  H is the handle's scalar (f64 / c64), L = Low<H> its
// single-precision sibling.  An outer step is three launches around the host-driven inner solve:
//   SpMV      q = A x, in H                                                   (launch_spmv, any route; q lands in r's buffer)
//   RfResid   r = b 1 + q (-1) ; partials of |r|^2 (step 0: of |b|^2 too)
//   RfDemote  |r|, res = |r| / |b|, the stop decision ; rl = fl_L(r (1 / |r|)) ; e = 0
//   (inner)   A_L e = rl in L                                                 (Cg<L> / Gmres<L>)
//   RfUpdate  x += fl_H(e) |r|
// The kernels follow CgKB / CgKC: the prologue re-reduces the producer's partials in every workgroup (same partials, same order
// => the same bits and the same decision everywhere), workgroup 0 records the scalars, and a launch never reads a state field
// that one of its own workgroups writes (the status word apart: it only ever leaves ST_RUNNING, on a decision every workgroup
// takes alike).  Once the status word has left ST_RUNNING every kernel returns at its first instruction.
// Both sides move 16 bytes per access: one pack of L (4 floats / 2 complex) against two packs of H.
#pragma once
#include "fused_launch.hpp"

namespace sprs {

template <class H> struct low_of;
template <> struct low_of<double> { using type = float; };
template <> struct low_of<cplx> { using type = cplxf; };
template <class H> using Low = typename low_of<H>::type;

// fl_L / fl_H: one rounding to nearest per component / exact
__device__ __forceinline__ float rf_lo(double a) { return (float)a; }
__device__ __forceinline__ cplxf rf_lo(cplx a) { return cplxf{(float)a.re, (float)a.im}; }
__device__ __forceinline__ double rf_hi(float a) { return (double)a; }
__device__ __forceinline__ cplx rf_hi(cplxf a) { return cplx{(double)a.re, (double)a.im}; }
__device__ __forceinline__ bool rf_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }
__device__ __forceinline__ bool rf_finite(float a) { return fabsf(a) <= 3.402823466e+38f; }
__device__ __forceinline__ bool rf_finite(cplx a) { return rf_finite(a.re) && rf_finite(a.im); }
__device__ __forceinline__ bool rf_finite(cplxf a) { return rf_finite(a.re) && rf_finite(a.im); }

// Device-resident scalar state of a refinement solve.  `outer` is the 0-based index of the step the last RfDemote decided on.
template <class H>
struct RfState {
    Real<H> r_norm, b_norm, res, s, tol, pad0;
    long long outer;
    int status, zero_rhs;
};

// PK elements of H starting at element i * PK: PK == 1 the element itself, else 16-byte packs (two of them per pack of L)
template <class H, int PK> struct rf_hpack { static constexpr int EP = PK == 1 ? 1 : pack_width<H>::value, NP = PK / EP; };
template <class H, int PK, bool NT>
__device__ __forceinline__ void rf_ld_h(const H *p, int64_t i, H (&v)[PK]) {
    constexpr int EP = rf_hpack<H, PK>::EP, NP = rf_hpack<H, PK>::NP;
    Pack<H, EP> q[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) q[k] = ldp<H, EP, NT>(p, i * NP + k);
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < EP; ++e) v[k * EP + e] = q[k].v[e];
}
template <class H, int PK, bool NT>
__device__ __forceinline__ void rf_st_h(H *p, int64_t i, const H (&v)[PK]) {
    constexpr int EP = rf_hpack<H, PK>::EP, NP = rf_hpack<H, PK>::NP;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        Pack<H, EP> q;
#pragma unroll
        for (int e = 0; e < EP; ++e) q.v[e] = v[k * EP + e];
        stp<H, EP, NT>(p, i * NP + k, q);
    }
}

// out_j = fl_L(in_j * scale): the product rounded in H::Real, then one rounding to L per component.  ZERO: zero_j = 0 as well.
template <class H, int PK, bool NT, bool ZERO>
__device__ __forceinline__ void rf_demote_run(const H *in, Real<H> scale, Low<H> *out, Low<H> *zero, int64_t i) {
    H v[PK];
    rf_ld_h<H, PK, NT>(in, i, v);
    Pack<Low<H>, PK> o;
#pragma unroll
    for (int e = 0; e < PK; ++e) o.v[e] = rf_lo(smulr(v[e], scale));
    stp<Low<H>, PK, NT>(out, i, o);
    if (ZERO) {
        Pack<Low<H>, PK> z;
#pragma unroll
        for (int e = 0; e < PK; ++e) z.v[e] = szero<Low<H>>();
        stp<Low<H>, PK, NT>(zero, i, z);
    }
}
// x_j = x_j + fl_H(in_j) * alpha: the product rounded, then the sum
template <class H, int PK, bool NT>
__device__ __forceinline__ void rf_update_run(const Low<H> *in, Real<H> alpha, H *x, int64_t i) {
    const Pack<Low<H>, PK> ev = ldp<Low<H>, PK, NT>(in, i);
    H v[PK];
    rf_ld_h<H, PK, NT>(x, i, v);
#pragma unroll
    for (int e = 0; e < PK; ++e) v[e] = sadd(v[e], smulr(rf_hi(ev.v[e]), alpha));
    rf_st_h<H, PK, NT>(x, i, v);
}

// RfResid:  r = b*1 + q*(-1) with q = A x found in r ; partials of norm2(r)^2 for RfDemote, at step 0 of norm2(b)^2 too.
//           Reads b and r, writes r.  Walks packs of H (launch_fused<H>).
template <class H, bool FIRST>
struct RfResid {
    const RfState<H> *S; const H *b; H *r; Real<H> *partR, *partB;
    Fin fin;                    // always empty: a single-GPU solver (kept for st_partial)
    H one, mone;
    Real<H> accR, accB;
    __device__ __forceinline__ bool prologue() {
        if (S->status != ST_RUNNING) return false;
        one = sone<H>(); mone = sneg(one);
        accR = 0.0; accB = 0.0;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto bv = ldp<H, PK, NT>(b, i); auto rv = ldp<H, PK, NT>(r, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            const H rr = sadd(smul(bv.v[e], one), smul(rv.v[e], mone));   // axpby(1, b, -1, r)
            rv.v[e] = rr;
            accR = accR + ssq(rr);
            if (FIRST) accB = accB + ssq(bv.v[e]);
        }
        stp<H, PK, NT>(r, i, rv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<H> smR[NWAVE];
        __shared__ Real<H> smB[NWAVE];
        const Real<H> sR = block_sum(accR, smR);
        Real<H> sB = 0.0;
        if (FIRST) sB = block_sum(accB, smB);
        if (threadIdx.x == 0) {
            st_partial(fin, partR + blockIdx.x, sR);
            if (FIRST) st_partial(fin, partB + blockIdx.x, sB);
        }
    }
};

// RfDemote: r_norm = sqrt(sum |r|^2) ; (step 0: b_norm likewise, zero right-hand side?) ; res = r_norm / b_norm ; converged?
//           finite?  the last step allowed?  s = r_norm ; rl = fl_L(r * (1 / s)) ; e = 0.  Reads r, writes rl and e.
//           Walks packs of L (launch_rf).
template <class H, bool FIRST>
struct RfDemote {
    RfState<H> *S; const Real<H> *partR, *partB; int P;
    long long k; int last;      // the step's index; last: k == max_outer, the decision is recorded and nothing is written
    const H *r; Low<H> *rl, *e;
    Real<H> inv_s;
    __device__ __forceinline__ bool prologue() {
        __shared__ Real<H> smR[NWAVE];
        __shared__ Real<H> smB[NWAVE];
        // only fields that no workgroup of THIS launch writes are read: tol always, b_norm from step 1 on (step 0 writes it)
        const int status = S->status;
        const Real<H> tol = S->tol;
        Real<H> b_norm = 0.0, sR, sB;
        if (FIRST) { reduce_partials2(partR, partB, P, smR, smB, sR, sB); b_norm = ssqrt(sB); }
        else { b_norm = S->b_norm; sR = reduce_partials(partR, P, smR); }
        if (status != ST_RUNNING) return false;
        if (FIRST && b_norm <= seps<Real<H>>()) {                   // the other solvers' zero-rhs rule
            if (first_thread()) { S->b_norm = b_norm; S->zero_rhs = 1; S->outer = 0; S->status = ST_CONVERGED; }
            return false;
        }
        const Real<H> r_norm = ssqrt(sR), res = r_norm / b_norm;
        int st = ST_RUNNING;
        if (res <= tol) st = ST_CONVERGED;
        else if (!rf_finite(r_norm)) st = ST_BREAKDOWN;             // a NaN lands here too
        if (first_thread()) {
            if (FIRST) S->b_norm = b_norm;
            S->r_norm = r_norm; S->res = res; S->s = r_norm; S->outer = k;
            if (st != ST_RUNNING) S->status = st;
        }
        if (st != ST_RUNNING || last) return false;
        inv_s = 1.0 / r_norm;                                       // rounded once
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const { rf_demote_run<H, PK, NT, true>(r, inv_s, rl, e, i); }
    __device__ __forceinline__ void epilogue() const {}
};

// RfUpdate: x += fl_H(e) * s.  Reads e and x, writes x; reads the state, writes none of it.  Walks packs of L.
template <class H>
struct RfUpdate {
    const RfState<H> *S; const Low<H> *e; H *x;
    Real<H> s;
    __device__ __forceinline__ bool prologue() {
        const int status = S->status;
        s = S->s;
        return status == ST_RUNNING;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const { rf_update_run<H, PK, NT>(e, s, x, i); }
    __device__ __forceinline__ void epilogue() const {}
};

// The same element-wise code as stand-alone launches (sprs_demote_scaled_dev_*, sprs_axpy_promoted_dev_*)
template <class H>
struct RfDemoteV {
    const H *in; Real<H> scale; Low<H> *out;
    __device__ __forceinline__ bool prologue() const { return true; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const { rf_demote_run<H, PK, NT, false>(in, scale, out, nullptr, i); }
    __device__ __forceinline__ void epilogue() const {}
};
template <class H>
struct RfUpdateV {
    const Low<H> *in; Real<H> alpha; H *x;
    __device__ __forceinline__ bool prologue() const { return true; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const { rf_update_run<H, PK, NT>(in, alpha, x, i); }
    __device__ __forceinline__ void epilogue() const {}
};

// RfCast: out = fl_L(in) for the operator's values and the preconditioner's diagonal (V = double or cplx).  *flag (may be
// null) is set where a finite value leaves L's range.
template <class V>
struct RfCast {
    const V *in; Low<V> *out; int *flag;
    __device__ __forceinline__ bool prologue() const { return true; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        V v[PK];
        rf_ld_h<V, PK, NT>(in, i, v);
        Pack<Low<V>, PK> o;
        bool bad = false;
#pragma unroll
        for (int e = 0; e < PK; ++e) { o.v[e] = rf_lo(v[e]); bad = bad || (rf_finite(v[e]) && !rf_finite(o.v[e])); }
        stp<Low<V>, PK, NT>(out, i, o);
        if (bad && flag) *flag = 1;                                 // an ordinary vector store; every writer stores the same value
    }
    __device__ __forceinline__ void epilogue() const {}
};

// Workgroups of a kernel that walks n elements in packs of pk
inline int rf_grid(const sprs_ctx *c, size_t n, int pk) { return balanced_grid(c, ((int64_t)n / pk + BLOCK - 1) / BLOCK); }

// Launch of a functor that walks packs of L = Low<H> (two packs of H each); `aligned`: every vector is 16-byte aligned (else
// element by element).  Non-temporal accesses from H vectors of 72 MB on (stream_loads_nt).
template <class H, class F>
static int launch_rf(sprs_ctx *c, size_t n, bool aligned, int chunked_walk, F f) {
    constexpr int PKL = pack_width<Low<H>>::value;
    const int grid = rf_grid(c, n, aligned ? PKL : 1);
    const int chunked = (chunked_walk && grid % 8 == 0 && grid >= 8) ? 1 : 0;
    if (!aligned)
        hipLaunchKernelGGL((fused_kernel<1, false, F>), dim3(grid), dim3(BLOCK), 0, c->stream, (int64_t)n, f, chunked);
    else if (stream_loads_nt(c, n * sizeof(H)))
        hipLaunchKernelGGL((fused_kernel<PKL, true, F>), dim3(grid), dim3(BLOCK), 0, c->stream, (int64_t)n, f, chunked);
    else
        hipLaunchKernelGGL((fused_kernel<PKL, false, F>), dim3(grid), dim3(BLOCK), 0, c->stream, (int64_t)n, f, chunked);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

}  // namespace sprs
