// Multi-shift conjugate gradients (host side): CgShift<T>.  One CG run on A from x_0 = 0 yields the solutions of
// (A + sigma_j I) x_j = rhs for m <= mmax shifts through a scalar recurrence per shift (the header's sprs_cgshift_* comment):
//   r = rhs ; p = rhs ; rho = conj(r).r ; x_j = 0 ; p_j = rhs ; zeta_j^(-1) = zeta_j^(0) = 1 ; alpha_(-1) = 1 ; beta_(-1) = 0
//   loop:  q = A p ; pq = conj(p).q ; BreakDown unless re(pq) > 0 ; alpha = rho / pq ; zeta_j^(n+1) ; r += q (-alpha) ;
//          beta = |r|^2 / rho ; alpha_j, beta_j ; x_j += p_j alpha_j ; Ok(n + 1) for column j if |zeta_j^(n+1)| |r| <= tol |rhs| ;
//          p_j = r zeta_j^(n+1) + p_j beta_j ; p = r*1 + p*beta
// Three launches per iteration whatever m is (cg_shift_fuse.hpp): one SpMV and 3 + (3 + 4 m_active) vector passes.  The host
// enqueues iterations blind and reads the state every `poll` of them; the results do not depend on `poll`: the device freezes a
// column at its event and stops all work once no column runs.  No preconditioner: a general M destroys the shift invariance.
// Of KrylovBase it uses the work vectors (r, p, q, then mmax columns of P and mmax of X), the partial slots and spmv() — no
// literal mode, trace or profile.
#include "krylov.hpp"

#include <cmath>

#include "cg_shift_fuse.hpp"

namespace sprs {

template <class T>
int CgShift<T>::create(const sprs_csr *A_, size_t size, size_t mmax_) {
    this->A = A_; this->ctx = A_->ctx;
    SPRS_TRY(size_is_rows(A_, size));
    if (mmax_ < 1 || mmax_ > (size_t)CGS_MAXM) return refuse(this->ctx, "sprs_cgshift", "mmax = %zu is outside 1 .. %d", mmax_, CGS_MAXM);
    SPRS_TRY(single_gpu_only(A_, "sprs_cgshift"));
    mmax = (int)mmax_;
    SPRS_TRY(this->init(A_, size, 3 + 2 * mmax));   // r, p, q ; P's columns ; X's columns (used where the caller's x is not aligned)
    return state.create(this->ctx);
}

template <class T>
int CgShift<T>::run(const Real<T> *shifts, int m, const T *rhs, bool host, T *x, size_t max_iter, Real<T> tol, size_t *its_out,
                    Real<T> *res_out, int *status_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n, stride = this->stride;
    T *r = this->vec(0), *p = this->vec(1), *q = this->vec(2), *PB = this->vec(3), *XW = this->vec(3 + mmax);

    // x in place where every column of the caller's block is a 16-byte aligned device vector; else a work block, copied out once
    const bool in_place = !host && aligned16(x) && (n * sizeof(T)) % 16 == 0;
    T *X = in_place ? x : XW;
    const int64_t xs = in_place ? (int64_t)n : (int64_t)stride;
    if (n) SPRS_HIP_TRY(c, hipMemcpyAsync(r, rhs, sizeof(T) * n, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    SPRS_TRY(dzero(c, X, (size_t)xs * (size_t)m));                                  // x_j = 0
    auto finish = [&]() -> int {
        if (!in_place && n)
            SPRS_HIP_TRY(c, hipMemcpy2DAsync(x, sizeof(T) * n, XW, sizeof(T) * stride, sizeof(T) * n, (size_t)m,
                                             host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        return SPRS_OK;
    };
    auto report = [&](int j, int st, size_t it, Real<T> res) {
        if (its_out) its_out[j] = it;
        if (res_out) res_out[j] = res;
        if (status_out) status_out[j] = st;
    };

    Real<T> rhs_norm = 0.0;
    SPRS_TRY(this->norm2(r, &rhs_norm));
    if (rhs_norm <= seps<Real<T>>()) {                                              // a zero right-hand side: x_j = 0, as Cg
        for (int j = 0; j < m; ++j) report(j, SPRS_OK, 0, rhs_norm);
        return finish();
    }
    const Real<T> tol2 = tol * rhs_norm;
    if ((double)rhs_norm <= (double)tol2) {                                         // |zeta_j^(0)| |r| <= tol2 with zeta = 1, r = rhs
        for (int j = 0; j < m; ++j) report(j, SPRS_OK, 0, (Real<T>)((double)rhs_norm / (double)rhs_norm));
        return finish();
    }
    T rho = szero<T>();
    SPRS_TRY(this->cdot(r, r, &rho));                                               // rho = conj(r).r
    SPRS_TRY(dcopy(c, p, r, n));                                                    // p = r
    for (int j = 0; j < m; ++j) SPRS_TRY(dcopy(c, PB + (size_t)j * stride, r, n));  // p_j = r

    CgShiftState<T> &H = *state.host;
    CgShiftState<T> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    H.rho = rho; H.rho_prev = rho; H.r_norm = rhs_norm; H.tol2 = tol2; H.rhs_norm = rhs_norm;
    H.a_prev = 1.0; H.b_prev = 0.0;
    for (int j = 0; j < CGS_MAXM; ++j) {
        H.sigma[j] = j < m ? (double)shifts[j] : 0.0;
        H.zeta[0][j] = 1.0; H.zeta[2][j] = 1.0;                                     // zeta^(0) and zeta^(-1) (row -1 mod 3)
        H.col_status[j] = j < m ? (int)ST_RUNNING : (int)CGS_UNUSED;
    }
    H.act_it = -1;
    H.status = ST_RUNNING; H.run_mask = (1 << m) - 1;
    SPRS_TRY(state.push());
    const int *d_status = &d_state->status;

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;
    const int GS = spmv_num_partials(this->A);
    Real<T> *partN = this->dslot(0);
    T *partPQ = this->pslot(1);

    const size_t poll = sprs::poll_interval(c);
    size_t its = 0, since_poll = 0;
    while (true) {
        const bool done_enqueue = its >= max_iter;
        if (!done_enqueue) {
            const long long it = (long long)its;
            SPRS_TRY(this->spmv(p, q, 1, p, partPQ, nullptr, d_status));            // CA: q = A p ; conj(p).q
            SPRS_TRY(launch_fused<T>(c, n, G, cw, CgShiftSB<T>{d_state, partPQ, GS, m, it, q, r, partN, T(), 0.0}));
            SPRS_TRY(launch_fused<T>(c, n, G, cw, CgShiftSC<T>{d_state, partN, G, m, it, r, p, X, PB, xs, (int64_t)stride, 0, 0, T(), T(), {}, {}, {}}));
            ++its; ++since_poll;
        }
        if (done_enqueue || since_poll >= poll) {
            since_poll = 0;
            SPRS_TRY(state.fetch());
            if (done_enqueue || H.status != ST_RUNNING) break;
        }
    }
    SPRS_TRY(finish());

    int ret = SPRS_OK;
    for (int j = 0; j < m; ++j) {
        int st = SPRS_OK; size_t it = (size_t)H.its[j]; Real<T> res = 0.0;
        switch (H.col_status[j]) {
            case ST_CONVERGED: res = H.res[j]; break;
            case ST_BREAKDOWN: st = SPRS_BREAKDOWN; break;
            default: st = SPRS_INSUFFICIENT_ITER; it = max_iter; break;             // still running after max_iter iterations
        }
        report(j, st, it, res);
        if (ret == SPRS_OK && st != SPRS_OK) ret = st;
    }
    return ret;
}

template <class T>
int CgShift<T>::solve(const Real<T> *shifts, size_t m, const T *rhs, size_t rhs_len, bool host, T *x, size_t x_len, size_t max_iter,
                      Real<T> tol, size_t *its_out, Real<T> *res_out, int *status_out) {
    if (!shifts || m < 1 || m > (size_t)mmax) {
        snprintf(this->ctx->err, sizeof(this->ctx->err), "sprs_cgshift: %zu shifts on a handle created for 1 .. %d", shifts ? m : (size_t)0, mmax);
        return SPRS_INVALID_ARGUMENT;
    }
    for (size_t j = 0; j < m; ++j) {
        if (!(shifts[j] >= 0) || !std::isfinite((double)shifts[j])) {
            snprintf(this->ctx->err, sizeof(this->ctx->err), "sprs_cgshift: shift %zu is negative or not finite (shifts must be real, finite and >= 0)", j);
            return SPRS_INVALID_ARGUMENT;
        }
    }
    if (rhs_len != this->n) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (x_len != this->n * m) return SPRS_INCOMPATIBLE_X_SIZE;
    CtxLock lock(this->ctx);   // one solve at a time per context (its stream, its scratch)
    SPRS_HIP_TRY(this->ctx, hipSetDevice(this->ctx->device));
    return run(shifts, (int)m, rhs, host, x, max_iter, tol, its_out, res_out, status_out);
}

template class CgShift<double>;
template class CgShift<float>;
template class CgShift<cplxf>;
template class CgShift<cplx>;

}  // namespace sprs
