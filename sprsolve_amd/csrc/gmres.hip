// Restarted GMRES(m), right-preconditioned (a diagonal, or an applied ILU(0) / AMG handle: one host path, Prec<T, V> of
// krylov.hpp), CGS2, Givens rotations: the recurrence of the header's sprs_gmres_* comment.
// Fused (gmres_fuse.hpp): the host enqueues whole cycles blind — per cycle SpMV, GmResid, GmStart, GmScale, the steps, GmXUpdate
// (an applied M: GmUForm, its launches, GmXAdd); per step [GmPrec, or an applied M's launches], SpMV,
// launch_cgs2 against v_0 .. v_j, GmStep, GmScale — and reads the head of the state every poll_interval() steps.
// Distributed operators: the norms travel through fin_for + handoff; the j + 1 coefficients of each of launch_cgs2's GmDots passes
// are reduced by one more single-workgroup launch into `coefs` and all-reduced there (red's cells hold two values a slot).
#include "krylov.hpp"

#include <cmath>

#include "gmres_fuse.hpp"

namespace sprs {

template <class T>
int Gmres<T>::create(const sprs_csr *A, size_t size, size_t restart) {
    if (restart > (size_t)GM_MAXM) return SPRS_INVALID_ARGUMENT;
    SPRS_TRY(size_is_rows(A, size));
    m = restart == 0 ? 30 : (int)restart;
    SPRS_TRY(this->init(A, size, m + 4));   // v_0 .. v_m, w, z, u
    this->no_p2p = true;                    // hand-offs through fin_for + handoff + the all-reduce only
    sprs_ctx *c = this->ctx;
    SPRS_TRY(state.create(c));
    SPRS_HIP_TRY(c, hipMemsetAsync(state.dev, 0, sizeof(GmresState<T>), c->stream));
    if (A->dist) {
        SPRS_HIP_TRY(c, hipMalloc((void **)&coefs, sizeof(T) * (GM_MAXM + 2)));
        SPRS_HIP_TRY(c, hipMemsetAsync(coefs, 0, sizeof(T) * (GM_MAXM + 2), c->stream));
    }
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
void Gmres<T>::destroy() {
    state.destroy();
    dots.destroy();
    if (coefs) (void)hipFree(coefs);
    coefs = nullptr;
    KrylovBase<T>::destroy();
}

template <class T>
void Gmres<T>::trace_step(double its, double g, double hn, T r, double c, T s) {
    if (!this->trace || this->trace_rows >= this->trace_cap) return;
    double *t = this->trace + 8 * this->trace_rows;
    t[0] = its; t[1] = g; t[2] = hn; t[3] = sre(r); t[4] = sim(r); t[5] = c; t[6] = sre(s); t[7] = sim(s);
    ++this->trace_rows;
}

template <class T>
template <class V>
int Gmres<T>::run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const V *dinv = M.dinv;
    const bool pc = M.any(), applied = M.applied.h != nullptr;
    *its_out = 0; *res_out = 0.0;

    Real<T> rhs_norm = 0.0;
    bool zero;
    SPRS_TRY(this->zero_rhs(rhs, x, &rhs_norm, res_out, &zero));
    if (zero) return SPRS_OK;

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;      // XCD-chunked walk of the vector kernels (spmv.hip)
    SPRS_TRY(dots.ensure(c, GM_MAXM, G));

    GmresHead<T> &H = state.host->hd;
    GmresState<T> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    H.its = 0; H.max_iter = (long long)max_iter; H.status = ST_RUNNING; H.skip = 1; H.x_cycle = -1;
    H.tol2 = tol * rhs_norm;
    auto push_head = [&]() -> int { return state.push(sizeof(GmresHead<T>)); };
    auto fetch_head = [&]() -> int { return state.fetch(sizeof(GmresHead<T>)); };
    SPRS_TRY(push_head());
    const GmresHead<T> *d_head = &d_state->hd;
    const int *d_status = &d_state->hd.status, *d_skip = &d_state->hd.skip;

    T *Vb = basis(0), *w = wvec(), *z = zvec(), *u = uvec();
    const int64_t vs = (int64_t)this->stride;
    Real<T> *partN = this->dslot(0), *partR = this->dslot(1);
    const bool dist = this->A->dist != nullptr;

    // distributed: the cnt coefficients of a Gram-Schmidt pass reduced into `coefs` and all-reduced there, one value each
    auto reduce_dots = [&](int cnt, GmCoefs<T> *cf) -> int {
        if (!dist) return SPRS_OK;
        SPRS_TRY(launch_small(c, gm_reduce_kernel<T>, 0, d_head, (const T *)dots.p, (int64_t)G, G, cnt, coefs));
        SPRS_TRY(allreduce_sum(this->comm(), coefs, (size_t)cnt * (sizeof(T) / sizeof(Real<T>)), sizeof(Real<T>) == 4));
        *cf = GmCoefs<T>{coefs, 1, 1};
        return SPRS_OK;
    };
    auto cycle_begin = [&]() -> int {
        SPRS_TRY(this->spmv(x, Vb, 0, nullptr, nullptr, nullptr, d_status));                        // v_0 = A x
        const Fin f = this->fin_for(1, partR, nullptr, G);
        SPRS_TRY(launch_fused<T>(c, n, G, cw, GmResid<T>{d_head, rhs, Vb, partR, f, T(), T(), 0.0}));
        Part<Real<T>> qR{partR, G};
        SPRS_TRY((this->template handoff<Real<T>, Real<T>>(1, G, partR, &qR)));
        SPRS_TRY(launch_small(c, gm_start_kernel<T>, 0, d_state, qR.p, qR.P));
        return launch_fused<T>(c, n, G, cw, GmScale<T>{d_head, Vb, 0.0});
    };
    auto step = [&](int j, long long cycle) -> int {
        T *vj = Vb + (size_t)j * this->stride, *vn = Vb + (size_t)(j + 1) * this->stride;
        // z = M v_j.  An applied M is a chain of launches of the handle's own (internal.hpp, AppliedPrec: ILU(0)'s two triangular
        // solves, AMG's cycle); they are not keyed on `skip` or the cycle: z and u are scratch, and neither x nor the basis is
        // touched by them.
        if (applied) SPRS_TRY(M.apply(vj, z));
        else if (pc) SPRS_TRY(launch_fused<T>(c, n, G, cw, GmPrec<T, V>{d_head, dinv, vj, z}));
        SPRS_TRY(this->spmv(pc ? z : vj, w, 0, nullptr, nullptr, nullptr, d_skip));                 // w = A z
        SPRS_TRY(launch_cgs2<T>(c, n, G, cw, d_state, Vb, vs, j + 1, w, vn, partN, dots.p, this->fin_for(0, partN, nullptr, G), reduce_dots));
        Part<Real<T>> qN{partN, G};
        SPRS_TRY((this->template handoff<Real<T>, Real<T>>(0, G, partN, &qN)));
        SPRS_TRY(launch_small(c, gm_step_kernel<T>, 0, d_state, qN.p, qN.P, j, m, cycle));
        return launch_fused<T>(c, n, G, cw, GmScale<T>{d_head, vn, 0.0});
    };
    auto cycle_end = [&](long long cycle) -> int {
        if (applied) {      // GmXUpdate in three: the solves in place on u stand between forming it and adding it
            SPRS_TRY(launch_fused<T>(c, n, G, cw, GmUForm<T>{d_state, cycle, Vb, vs, u, nullptr, 0}));          // u = sum v_i y_i
            SPRS_TRY(M.apply(u, u));                                                                    // u = M u
            return launch_fused<T>(c, n, G, cw, GmXAdd<T>{d_state, cycle, u, x});                       // x += u*1
        }
        return dispatch_bool(pc, [&](auto pc_tag) {
            return launch_fused<T>(c, n, G, cw, GmXUpdate<T, V, decltype(pc_tag)::value>{d_state, cycle, Vb, vs, dinv, x, nullptr, 0});
        });
    };

    const bool tracing = this->trace != nullptr;
    const size_t poll = this->poll_interval();
    size_t enq = 0, since_poll = 0;
    long long traced = 0;
    bool over = false;
    for (long long cycle = 0; !over; ++cycle) {
        SPRS_TRY(cycle_begin());
        for (int j = 0; j < m && enq < max_iter && !over; ++j) {
            SPRS_TRY(step(j, cycle));
            ++enq;
            if (++since_poll >= poll) {
                since_poll = 0;
                SPRS_TRY(fetch_head());
                if (tracing && H.its > traced) {
                    traced = H.its;
                    trace_step((double)H.its, H.tr_g, H.tr_hn, H.tr_r, H.tr_c, H.tr_s);
                }
                over = H.status != ST_RUNNING;
            }
        }
        SPRS_TRY(cycle_end(cycle));     // (keyed on the cycle its GmStep recorded: a no-op where that cycle made no step)
        if (!over && enq >= max_iter) {
            SPRS_TRY(fetch_head());
            over = H.status != ST_RUNNING;
            enq = (size_t)H.its;        // still running: cycles that exhausted their Krylov space made fewer steps than were enqueued
        }
    }
    SPRS_TRY(fetch_head());             // (behind the last x update)
    if (H.status == ST_CONVERGED) {
        *its_out = (size_t)H.its; *res_out = H.r_norm / rhs_norm;
        return SPRS_OK;
    }
    if (H.status == ST_BREAKDOWN) {
        *its_out = (size_t)H.its;
        return SPRS_BREAKDOWN;
    }
    if (H.status == ST_COMM_TIMEOUT) return this->comm_timeout();
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

// literal mode: the recurrence op by op, one existing BLAS-1 entry per op, scalars consumed on the host
template <class T>
template <class V>
int Gmres<T>::run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const bool pc = M.any();
    *its_out = 0; *res_out = 0.0;
    Real<T> rhs_norm = 0.0;
    bool zero;
    SPRS_TRY(this->zero_rhs(rhs, x, &rhs_norm, res_out, &zero));
    if (zero) return SPRS_OK;
    const Real<T> tol2 = tol * rhs_norm;
    T *w = wvec(), *z = zvec(), *u = uvec();
    std::vector<T> h(GM_MAXM + 1), g(GM_MAXM + 1), s(GM_MAXM), y(GM_MAXM), R(GM_MAXM * (GM_MAXM + 1) / 2), c2(GM_MAXM);
    std::vector<Real<T>> cs(GM_MAXM);
    auto axpy = [&](T a, const T *xx, T *yy) { return launch_axpy<T, T>(c, n, a, xx, yy); };
    size_t its = 0;
    while (true) {
        T *v0 = basis(0);
        SPRS_TRY(this->spmv(x, v0, 0, nullptr, nullptr, nullptr, nullptr));
        SPRS_TRY(launch_axpby<T>(c, n, sone<T>(), rhs, sneg(sone<T>()), v0));
        Real<T> beta = 0.0;
        SPRS_TRY(this->norm2(v0, &beta));
        if (beta <= tol2) { *its_out = its; *res_out = beta / rhs_norm; return SPRS_OK; }
        if (its >= max_iter) { *its_out = max_iter; return SPRS_INSUFFICIENT_ITER; }
        SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta, v0));
        g[0] = sfromr<T>(beta);
        int k = m;
        Real<T> gabs = 0.0;
        for (int j = 0; j < m; ++j) {
            T *vj = basis(j);
            if (pc) SPRS_TRY(M.apply(vj, z));
            SPRS_TRY(this->spmv(pc ? z : vj, w, 0, nullptr, nullptr, nullptr, nullptr));
            for (int i = 0; i <= j; ++i) SPRS_TRY(this->cdot(basis(i), w, &h[i]));
            for (int i = 0; i <= j; ++i) SPRS_TRY(axpy(sneg(h[i]), basis(i), w));
            for (int i = 0; i <= j; ++i) SPRS_TRY(this->cdot(basis(i), w, &c2[i]));
            for (int i = 0; i <= j; ++i) SPRS_TRY(axpy(sneg(c2[i]), basis(i), w));
            for (int i = 0; i <= j; ++i) h[i] = sadd(h[i], c2[i]);
            Real<T> hn = 0.0;
            SPRS_TRY(this->norm2(w, &hn));
            if (!(hn >= Real<T>(0))) { *its_out = its; return SPRS_BREAKDOWN; }
            gabs = gm_rotate<T>(j, h.data(), hn, cs.data(), s.data(), g.data(), R.data() + j * (j + 1) / 2);
            ++its;
            trace_step((double)its, gabs, hn, R[j * (j + 1) / 2 + j], cs[j], s[j]);
            if (gabs <= tol2 || hn == Real<T>(0) || its >= max_iter) { k = j + 1; break; }
            SPRS_TRY(dcopy(c, basis(j + 1), w, n));
            SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / hn, basis(j + 1)));
        }
        gm_backsub<T>(k, R.data(), g.data(), y.data());
        SPRS_TRY(dzero(c, u, n));
        for (int i = 0; i < k; ++i) SPRS_TRY(axpy(y[i], basis(i), u));
        if (pc) SPRS_TRY(M.apply(u, u));
        SPRS_TRY(axpy(sone<T>(), u, x));
        gabs = sabs(g[k]);
        if (gabs <= tol2) { *its_out = its; *res_out = gabs / rhs_norm; return SPRS_OK; }
        if (its >= max_iter) { *its_out = max_iter; return SPRS_INSUFFICIENT_ITER; }
    }
}

template <class T>
int Gmres<T>::solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                        size_t *its_out, Real<T> *res_out) {
    return KrylovBase<T>::solve(*this, false, P, rhs, rhs_len, x, x_len, max_iter, tol, its_out, res_out);
}

template class Gmres<double>;
template class Gmres<float>;
template class Gmres<cplxf>;
template class Gmres<cplx>;

}  // namespace sprs
