// Conjugate gradients for Hermitian positive-definite A, optionally preconditioned: by a diagonal (Jacobi) or by an applied
// handle (ILU(0), AMG), on one host path (Prec<T, V>, krylov.hpp).  The recurrence (the numbered steps are those of the
// header's sprs_cg_* comment):
//   r = rhs*1 + (A x)*(-1) ; z = M^-1 r ; p = z ; rho = conj(r).z
//   loop:  q = A p ; pq = conj(p).q ; BreakDown unless re(pq) > 0 ; alpha = rho / pq ; x += p alpha ; r += q (-alpha) ;
//          Ok(its + 1) if |r| <= tol |rhs| ; z = M^-1 r ; rho_new = conj(r).z ; InvalidPreconditioner unless re(rho_new) > 0 ;
//          beta = rho_new / rho ; p = z*1 + p*beta
// Fused: three launches per iteration (cg_fuse.hpp) — one SpMV and 6 + 3 vector passes (8 + 3 with Jacobi, whose M^-1 is read
// inside CgKB); an applied M adds its own launches and CgRZ between CgKB and CgKC.
#include "krylov.hpp"

#include "cg_fuse.hpp"

namespace sprs {

template <class T>
int Cg<T>::create(const sprs_csr *A, size_t size) {
    SPRS_TRY(size_is_rows(A, size));
    SPRS_TRY(this->init(A, size, 4));   // r, p, q, z (z only with a preconditioner)
    this->no_p2p = true;                // hand-offs through fin_for + handoff + the all-reduce only
    return state.create(this->ctx);
}

template <class T>
template <class V>
int Cg<T>::start(const Prec<T, V> &M, const T *rhs, T *x, Real<T> tol, Real<T> *rhs_norm, Real<T> *tol2, T *rho, bool *done, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    T *r = this->vec(0), *p = this->vec(1), *z = M.any() ? this->vec(3) : r;
    SPRS_TRY(this->zero_rhs(rhs, x, rhs_norm, res_out, done));
    if (*done) return SPRS_OK;
    *done = true;
    *tol2 = tol * *rhs_norm;
    SPRS_TRY(this->spmv(x, r, 0, nullptr, nullptr, nullptr, nullptr));      // r = A x
    SPRS_TRY(launch_axpby<T>(c, n, sone<T>(), rhs, sneg(sone<T>()), r));    // r = rhs*1 + r*(-1)
    Real<T> r_norm = 0.0;
    SPRS_TRY(this->norm2(r, &r_norm));
    if (r_norm <= *tol2) { *res_out = r_norm / *rhs_norm; return SPRS_OK; }
    if (M.any()) SPRS_TRY(M.apply(r, z));                                   // z = M^-1 r
    SPRS_TRY(dcopy(c, p, z, n));                                            // p = z
    SPRS_TRY(this->cdot(r, z, rho));                                        // rho = conj(r).z
    *done = false;
    return SPRS_OK;
}

template <class T>
template <class V>
int Cg<T>::run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const V *dinv = M.dinv;
    const bool pc = M.any(), applied = M.applied.h != nullptr;
    *its_out = 0; *res_out = 0.0;
    T *r = this->vec(0), *p = this->vec(1), *q = this->vec(2), *z = pc ? this->vec(3) : r;

    Real<T> rhs_norm = 0.0, tol2 = 0.0;
    T rho = szero<T>();
    bool done;
    SPRS_TRY(start<V>(M, rhs, x, tol, &rhs_norm, &tol2, &rho, &done, res_out));
    if (done) return SPRS_OK;

    CgState<T> &H = *state.host;
    CgState<T> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    H.rho = rho; H.rho_prev = rho; H.tol2 = tol2;
    H.its = 0; H.status = ST_RUNNING;
    SPRS_TRY(state.push());
    const int *d_status = &d_state->status;

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;      // XCD-chunked walk of the vector kernels (spmv.hip)
    const int GS = spmv_num_partials(this->A);
    Real<T> *partN = this->dslot(0);
    T *partRZ = this->pslot(0), *partPQ = this->pslot(1);
    Part<T> qPQ{partPQ, GS}, qRZ{partRZ, G};
    Part<Real<T>> qN{partN, G};

    auto CA = [&]() -> int {                                                // q = A p ; conj(p).q
        const Fin f = this->fin_for(0, partPQ, nullptr, GS);
        SPRS_TRY(this->spmv(p, q, 1, p, partPQ, nullptr, d_status, false, &f));
        return this->handoff(0, GS, partPQ, &qPQ);
    };
    auto KB = [&]() -> int {                                                // M^-1 a diagonal: z and conj(r).z are formed here too
        const Fin f = this->fin_for(1, partN, partRZ, G);
        SPRS_TRY(dispatch_bool(dinv != nullptr, [&](auto pc_tag) {
            return launch_fused<T>(c, n, G, cw, CgKB<T, V, decltype(pc_tag)::value>{d_state, qPQ.p, qPQ.P, p, q, x, r, dinv, dinv ? z : r, partN, partRZ, f, T(), T(), 0.0, T()});
        }));
        return this->handoff(1, G, partN, &qN, partRZ, &qRZ);
    };
    // An applied M: z = M r is a chain of launches of the handle's own (internal.hpp, AppliedPrec: ILU(0)'s two triangular
    // solves, AMG's cycle), then CgRZ forms the partials of conj(r).z — no host wait inside an iteration.  Once the status
    // word has left ST_RUNNING the solves still run: they read r and write only z and the handle's scratch, never x, r or p.
    auto RZ = [&]() -> int {
        SPRS_TRY(M.apply(r, z));
        return launch_fused<T>(c, n, G, cw, CgRZ<T>{d_state, r, z, partRZ, T()});
    };
    auto KC = [&]() -> int {
        return dispatch_bool(pc, [&](auto pc_tag) {
            return launch_fused<T>(c, n, G, cw, CgKC<T, decltype(pc_tag)::value>{d_state, qN.p, qRZ.p, qN.P, z, p, T(), T()});
        });
    };

    const bool tracing = this->trace != nullptr;
    const size_t poll = this->poll_interval();
    size_t its = 0, since_poll = 0;
    while (true) {
        const bool done_enqueue = its >= max_iter;
        if (!done_enqueue) {
            SPRS_TRY(CA()); SPRS_TRY(KB());
            if (applied) SPRS_TRY(RZ());
            SPRS_TRY(KC());
            ++its; ++since_poll;
        }
        if (done_enqueue || since_poll >= poll) {
            since_poll = 0;
            SPRS_TRY(state.fetch());
            if (H.status != ST_RUNNING && its > (size_t)H.its) this->profile_discard_last(its - (size_t)H.its - (H.status == ST_CONVERGED ? 0 : 1));
            if (H.status == ST_CONVERGED) {
                *its_out = (size_t)H.its; *res_out = H.r_norm / rhs_norm;
                return SPRS_OK;
            }
            if (H.status == ST_BREAKDOWN) {
                *its_out = (size_t)H.its;
                return SPRS_BREAKDOWN;
            }
            if (H.status == ST_INVALID_PC) {
                *its_out = (size_t)H.its; *res_out = H.pc_re;
                return SPRS_INVALID_PRECOND;
            }
            if (tracing && !done_enqueue) this->trace_row((double)(H.its - 1), H.r_norm, H.rho, H.alpha, H.beta);
            if (done_enqueue) break;
        }
    }
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

// literal mode: the recurrence op by op, one kernel per op, host-consumed scalars
template <class T>
template <class V>
int Cg<T>::run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const bool pc = M.any();
    *its_out = 0; *res_out = 0.0;
    T *r = this->vec(0), *p = this->vec(1), *q = this->vec(2), *z = pc ? this->vec(3) : r;
    Real<T> rhs_norm = 0.0, tol2 = 0.0;
    T rho = szero<T>();
    bool done;
    SPRS_TRY(start<V>(M, rhs, x, tol, &rhs_norm, &tol2, &rho, &done, res_out));
    if (done) return SPRS_OK;
    for (size_t its = 0; its < max_iter; ++its) {
        SPRS_TRY(this->spmv(p, q, 0, nullptr, nullptr, nullptr, nullptr));
        T pq;
        SPRS_TRY(this->cdot(p, q, &pq));
        if (!(sre(pq) > 0.0)) { *its_out = its; return SPRS_BREAKDOWN; }
        const T alpha = sdiv(rho, pq);
        SPRS_TRY((launch_axpy<T, T>(c, n, alpha, p, x)));
        SPRS_TRY((launch_axpy<T, T>(c, n, sneg(alpha), q, r)));
        Real<T> r_norm = 0.0;
        SPRS_TRY(this->norm2(r, &r_norm));
        if (r_norm <= tol2) { *its_out = its + 1; *res_out = r_norm / rhs_norm; return SPRS_OK; }
        if (pc) SPRS_TRY(M.apply(r, z));
        T rho_new;
        SPRS_TRY(this->cdot(r, z, &rho_new));
        if (pc && !(sre(rho_new) > 0.0)) { *its_out = its; *res_out = sre(rho_new); return SPRS_INVALID_PRECOND; }
        const T beta = sdiv(rho_new, rho);
        rho = rho_new;
        SPRS_TRY(launch_axpby<T>(c, n, sone<T>(), z, beta, p));
        this->trace_row((double)its, r_norm, rho, alpha, beta);
    }
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

template <class T>
int Cg<T>::solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                     size_t *its_out, Real<T> *res_out) {
    return KrylovBase<T>::solve(*this, false, P, rhs, rhs_len, x, x_len, max_iter, tol, its_out, res_out);
}

template class Cg<double>;
template class Cg<float>;
template class Cg<cplxf>;
template class Cg<cplx>;

}  // namespace sprs
