// LSMR (Fong & Saunders) for min |rhs - A x|_2, optionally damped, on any CSR operator A and its adjoint handle.  The
// recurrence (the numbered steps are those of the header's sprs_lsmr_* comment; every scalar real, u kept un-normalised):
//   u = rhs*1 + (A x)*(-1) ; beta = |u| ; v = A^H u ; v *= 1 / beta ; alpha = |v| ; v *= 1 / alpha ; h = v ; hbar = 0
//   loop:  w = A v ; u = w*1 + u*f ; beta = |u| ; [w' = A^H u ; v = w'*(1 / beta) + v*(-beta) ; alpha = |v|]  (beta > 0)
//          ls_step: rotations, g1 g2 g3, norm estimates ; BreakDown unless all finite
//          hbar = h*1 + hbar*g1 ; x += hbar*g2 ; v *= 1 / alpha ; h = v*1 + h*g3
//          Ok(its + 1) if beta = 0 or alpha = 0 or test 1 or test 2 (with |x|)
// Fused: five launches per iteration (lsmr_fuse.hpp) — two SpMVs and 3 of m + 3 + 8 of n vector passes.
#include "krylov.hpp"

#include "lsmr_fuse.hpp"

extern "C" int sprs_csr_adjoint(const sprs_csr *A, int conjugate, sprs_csr **out);

namespace sprs {

template <class T>
int Lsmr<T>::create(const sprs_csr *A, const sprs_csr *AH_or_null) {
    const sprs_csr *H = AH_or_null;
    SPRS_TRY(single_gpu_only(A, "sprs_lsmr", H));
    if (H && (H->dtype != A->dtype || H->ctx != A->ctx)) return SPRS_INVALID_ARGUMENT;
    if (H && (H->nrows != A->ncols || H->ncols != A->nrows)) return SPRS_DIM_MISMATCH;
    if (H) AH = H;
    else {
        SPRS_TRY(sprs_csr_adjoint(A, 1, &own_AH));
        AH = own_AH;
    }
    m = (size_t)A->nrows; nc = (size_t)A->ncols;
    SPRS_TRY(this->init(A, m, 2));                       // u, w
    stride_n = (nc + 31) & ~(size_t)31;
    if (stride_n == 0) stride_n = 32;
    SPRS_HIP_TRY(this->ctx, hipMalloc((void **)&work_n, sizeof(T) * stride_n * 4));   // v, w', h, hbar
    SPRS_HIP_TRY(this->ctx, hipMemsetAsync(work_n, 0, sizeof(T) * stride_n * 4, this->ctx->stream));
    SPRS_HIP_TRY(this->ctx, hipStreamSynchronize(this->ctx->stream));
    return state.create(this->ctx);
}

template <class T>
void Lsmr<T>::destroy() {
    state.destroy();
    if (work_n) (void)hipFree(work_n);
    work_n = nullptr;
    KrylovBase<T>::destroy();
    if (own_AH) (void)sprs_csr_destroy(own_AH);
    own_AH = nullptr; AH = nullptr;
}

template <class T>
int Lsmr<T>::mul(const sprs_csr *M, const T *x, T *y, const int *status) {
    return this->profiled([&]() -> int { return launch_spmv<T>(M, SpmvPart::Whole, x, y, 0, nullptr, nullptr, nullptr, status); }, true);
}

template <class T>
int Lsmr<T>::grid_of(size_t len) const {
    constexpr int PKW = pack_width<T>::value;
    return balanced_grid(this->ctx, ((int64_t)len / PKW + BLOCK - 1) / BLOCK);
}

template <class T>
int Lsmr<T>::start(const T *rhs, T *x, R damp, LsIter<R> *s0, R *normb, bool *done, R *res_out, R *ares_out) {
    sprs_ctx *c = this->ctx;
    T *u = this->vec(0), *v = nvec_(0), *h = nvec_(2), *hbar = nvec_(3);
    *done = true;
    SPRS_TRY(norm2_host<T>(c, m, rhs, normb));
    if (*normb <= seps<R>()) {                                              // KrylovBase::zero_rhs on the two lengths
        SPRS_TRY(dzero(c, x, nc));
        *res_out = *normb;
        return SPRS_OK;
    }
    SPRS_TRY(mul(this->A, x, u, nullptr));                                  // u = A x
    SPRS_TRY(launch_axpby<T>(c, m, sone<T>(), rhs, sneg(sone<T>()), u));    // u = rhs*1 + u*(-1)
    R beta = 0, alpha = 0;
    SPRS_TRY(norm2_host<T>(c, m, u, &beta));
    if (!ls_finite(beta)) return SPRS_BREAKDOWN;
    if (beta == (R)0) return SPRS_OK;                                       // x solves the system exactly
    SPRS_TRY(mul(AH, u, v, nullptr));                                       // v = A^H u
    SPRS_TRY(launch_rscale<T>(c, nc, (R)1 / beta, v));
    SPRS_TRY(norm2_host<T>(c, nc, v, &alpha));
    if (!ls_finite(alpha)) return SPRS_BREAKDOWN;
    *res_out = beta / *normb;
    if (alpha == (R)0) return SPRS_OK;                                      // A^H r = 0: x is a least-squares solution
    SPRS_TRY(launch_rscale<T>(c, nc, (R)1 / alpha, v));
    SPRS_TRY(dcopy(c, h, v, nc));
    SPRS_TRY(dzero(c, hbar, nc));
    LsIter<R> s{};
    s.alpha = alpha; s.beta = beta;
    s.alphabar = alpha; s.zetabar = alpha * beta; s.rho = 1; s.rhobar = 1; s.cbar = 1; s.sbar = 0;
    s.betadd = beta; s.betad = 0; s.rhodold = 1; s.tautildeold = 0; s.thetatilde = 0; s.zeta = 0; s.d = 0;
    s.normA2 = alpha * alpha; s.normA = alpha; s.normr = beta; s.normar = alpha * beta; s.lucky = 0; s.its = 0;
    *s0 = s;
    *ares_out = ls_ares(s);
    *done = false;
    return SPRS_OK;
}

template <class T>
int Lsmr<T>::run(const T *rhs, T *x, R damp, size_t max_iter, R tol, size_t *its_out, R *res_out, R *ares_out) {
    sprs_ctx *c = this->ctx;
    T *u = this->vec(0), *w = this->vec(1), *v = nvec_(0), *wn = nvec_(1), *h = nvec_(2), *hbar = nvec_(3);
    LsDev<R> &H = *state.host;
    LsDev<R> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    R normb = 0;
    bool done;
    SPRS_TRY(start(rhs, x, damp, &H.st[0], &normb, &done, res_out, ares_out));
    if (done) return SPRS_OK;
    H.normb = normb; H.tol = tol; H.damp = damp; H.status = ST_RUNNING;
    SPRS_TRY(state.push());
    const int *d_status = &d_state->status;

    const int Gm = grid_of(m), Gn = grid_of(nc);
    const int cwm = fused_chunked(this->A) ? 1 : 0, cwn = fused_chunked(AH) ? 1 : 0;    // XCD-chunked walks (spmv.hip)
    R *partU = this->dslot(0), *partV = this->dslot(1), *partX = this->dslot(2);
    const Fin nofin{};                                                      // single GPU: the consumers re-reduce the partials

    const bool tracing = this->trace != nullptr;
    const size_t poll = this->poll_interval();
    size_t its = 0, since_poll = 0;
    while (true) {
        const bool done_enqueue = its >= max_iter;
        const int par = (int)(its & 1);
        if (!done_enqueue) {
            SPRS_TRY(mul(this->A, v, w, d_status));
            SPRS_TRY(launch_fused<T>(c, m, Gm, cwm, LsKU<T>{d_state, par, partX, Gn, w, u, partU, nofin, 0, 0}));
            SPRS_TRY(mul(AH, u, wn, d_status));
            SPRS_TRY(launch_fused<T>(c, nc, Gn, cwn, LsKV<T>{d_state, par, partU, Gm, wn, v, partV, nofin, 0, 0, 0}));
            SPRS_TRY(launch_fused<T>(c, nc, Gn, cwn, LsKH<T>{d_state, par, partU, Gm, partV, Gn, v, h, hbar, x, partX, nofin, 0, 0, 0, 0, 0}));
            ++its; ++since_poll;
        }
        if (done_enqueue || since_poll >= poll) {
            since_poll = 0;
            SPRS_TRY(launch_fused<T>(c, 0, 1, 0, LsKT<T>{d_state, (int)(its & 1), partX, Gn}));
            SPRS_TRY(state.fetch());
            const size_t ev = (size_t)H.ev_its;
            if (H.status == ST_CONVERGED && its > ev) this->profile_discard_last(2 * (its - ev) - 1);
            if (H.status == ST_BREAKDOWN && its > ev + 1) this->profile_discard_last(2 * (its - ev - 1));
            if (tracing && !done_enqueue && (H.status == ST_RUNNING || H.status == ST_CONVERGED)) {
                const LsIter<R> &b = H.st[its & 1];
                this->trace_row((double)(its - 1), b.normr, sfromr<T>(b.normar), sfromr<T>(b.alpha), sfromr<T>(b.beta));
            }
            if (H.status == ST_CONVERGED) {
                *its_out = ev; *res_out = H.ev_res; *ares_out = H.ev_ares;
                return SPRS_OK;
            }
            if (H.status == ST_BREAKDOWN) {
                *its_out = ev;
                return SPRS_BREAKDOWN;
            }
            if (done_enqueue) break;
        }
    }
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

// literal mode: the recurrence op by op, one kernel per op, host-consumed scalars
template <class T>
int Lsmr<T>::run_literal(const T *rhs, T *x, R damp, size_t max_iter, R tol, size_t *its_out, R *res_out, R *ares_out) {
    sprs_ctx *c = this->ctx;
    T *u = this->vec(0), *w = this->vec(1), *v = nvec_(0), *wn = nvec_(1), *h = nvec_(2), *hbar = nvec_(3);
    LsIter<R> s{};
    R normb = 0;
    bool done;
    SPRS_TRY(start(rhs, x, damp, &s, &normb, &done, res_out, ares_out));
    if (done) return SPRS_OK;
    const T one = sone<T>();
    for (size_t its = 0; its < max_iter; ++its) {
        R beta = 0, alpha = 0, normx = 0, g1, g2, g3;
        SPRS_TRY(mul(this->A, v, w, nullptr));
        SPRS_TRY(launch_axpby<T>(c, m, one, w, sfromr<T>(-(s.alpha * ((R)1 / s.beta))), u));
        SPRS_TRY(norm2_host<T>(c, m, u, &beta));
        if (!ls_finite(beta)) { *its_out = its; return SPRS_BREAKDOWN; }
        if (beta > (R)0) {
            SPRS_TRY(mul(AH, u, wn, nullptr));
            SPRS_TRY(launch_axpby<T>(c, nc, sfromr<T>((R)1 / beta), wn, sfromr<T>(-beta), v));
            SPRS_TRY(norm2_host<T>(c, nc, v, &alpha));
        }
        LsIter<R> o;
        if (!ls_finite(alpha) || !ls_step(s, damp, beta, alpha, o, g1, g2, g3)) { *its_out = its; return SPRS_BREAKDOWN; }
        SPRS_TRY(launch_axpby<T>(c, nc, one, h, sfromr<T>(g1), hbar));
        SPRS_TRY((launch_axpy<T, R>(c, nc, g2, hbar, x)));
        if (alpha > (R)0) SPRS_TRY(launch_rscale<T>(c, nc, (R)1 / alpha, v));
        SPRS_TRY(launch_axpby<T>(c, nc, one, v, sfromr<T>(g3), h));
        SPRS_TRY(norm2_host<T>(c, nc, x, &normx));
        s = o;
        this->trace_row((double)its, s.normr, sfromr<T>(s.normar), sfromr<T>(s.alpha), sfromr<T>(s.beta));
        if (ls_converged(s, normb, tol, normx)) {
            *its_out = its + 1; *res_out = ls_res(s, normb); *ares_out = ls_ares(s);
            return SPRS_OK;
        }
    }
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

template <class T>
int Lsmr<T>::solve_dev(const T *rhs, size_t rhs_len, T *x, size_t x_len, R damp, size_t max_iter, R tol, size_t *its_out, R *res_out,
                       R *ares_out) {
    size_t its_dummy; R res_dummy, ares_dummy;
    if (!its_out) its_out = &its_dummy;
    if (!res_out) res_out = &res_dummy;
    if (!ares_out) ares_out = &ares_dummy;
    *its_out = 0; *res_out = 0; *ares_out = 0;
    if (rhs_len != m || x_len != nc) return SPRS_DIM_MISMATCH;
    if (!(damp >= (R)0)) return SPRS_INVALID_ARGUMENT;
    SPRS_TRY(this->begin_solve());
    const int st = this->mode == 1 ? run_literal(rhs, x, damp, max_iter, tol, its_out, res_out, ares_out)
                                   : run(rhs, x, damp, max_iter, tol, its_out, res_out, ares_out);
    if (st >= SPRS_ERR_HIP) return st;
    SPRS_TRY(this->end_solve());
    return st;
}

template class Lsmr<double>;
template class Lsmr<float>;
template class Lsmr<cplxf>;
template class Lsmr<cplx>;

}  // namespace sprs
