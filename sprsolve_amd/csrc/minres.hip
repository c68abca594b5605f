// MINRES / CSMINRES (host side).  Reference: src/minres.rs:31-341, src/cs_minres.rs:29-158.  Kernels: minres_fuse.hpp, and
// spmv_dict.hip for the deferred M3.
#include "krylov.hpp"

#include <utility>

#include "minres_fuse.hpp"

namespace sprs {

template <class T>
int MinRes<T>::create(const sprs_csr *A, size_t size, bool saunders_) {
    saunders = saunders_;
    SPRS_TRY(size_is_rows(A, size));
    SPRS_TRY(this->init(A, size, 8));   // minres.rs:24 workspace 8n (cs_minres.rs:22 uses 7n)
    return state.create(this->ctx);
}

template <class T>
template <class V>
int MinRes<T>::run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const V *dinv = M.dinv;
    const bool pc = M.any(), applied = M.applied.h != nullptr;
    const bool sau = saunders && is_complex<T>::value;   // conj() is the identity on real data
    *its_out = 0; *res_out = 0.0;

    Real<T> rhs_norm = 0.0;
    bool zero;
    SPRS_TRY(this->zero_rhs(rhs, x, &rhs_norm, res_out, &zero));            // :51-56
    if (zero) return SPRS_OK;
    const Real<T> threshold = tol * rhs_norm;                                // :57

    T *v_old = this->vec(0), *v_new = this->vec(1), *v = this->vec(2);      // :68-70
    T *p_old = this->vec(3), *p_oold = this->vec(4), *p = this->vec(5);     // :71-73
    T *w = this->vec(6), *w_new = this->vec(7);                             // :222-223

    SPRS_TRY(dcopy(c, v_new, rhs, n));                                      // :77
    SPRS_TRY(this->spmv(x, v_old, 0, nullptr, nullptr, nullptr, nullptr));  // :78
    SPRS_TRY((launch_axpy<T, T>(c, n, sneg(sone<T>()), v_old, v_new)));     // :80
    Real<T> res_norm = 0.0;
    SPRS_TRY(this->norm2(v_new, &res_norm));                        // :81
    Real<T> beta_new;
    if (pc) {
        SPRS_TRY(M.apply(v_new, w_new));                                    // :233
        T b2;
        SPRS_TRY(this->cdot(v_new, w_new, &b2));               // :235
        if (sre(b2) < seps<Real<T>>() || sim(b2) > seps<Real<T>>() * sre(b2)) {                     // :236-244
            *its_out = 0; *res_out = sre(b2);
            return SPRS_INVALID_PRECOND;
        }
        beta_new = ssqrt(sre(b2));                                           // :245
        const Real<T> ts = Real<T>(1) / beta_new;                                   // :248
        SPRS_TRY(launch_rscale<T>(c, n, ts, v_new));                        // :249
        SPRS_TRY(launch_rscale<T>(c, n, ts, w_new));                        // :250
    } else {
        beta_new = res_norm;                                                // :82
        SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta_new, v_new));            // :84
    }
    SPRS_TRY(dzero(c, v, n)); SPRS_TRY(dzero(c, p_old, n)); SPRS_TRY(dzero(c, p, n));   // :86-88

    MinresDev<T> &H = *state.host;
    MinresDev<T> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    MinresState<T> &S0 = H.st[0];
    S0.c = sone<T>(); S0.c_old = sone<T>(); S0.eta = sone<T>(); S0.alpha = szero<T>();   // :60-64
    S0.s = 0.0; S0.s_old = 0.0;
    S0.beta = beta_new; S0.beta_one = beta_new;                             // :82-83
    S0.res_norm = res_norm; S0.threshold = threshold;
    H.st[1] = S0;
    H.its = 0; H.status = ST_RUNNING;
    SPRS_TRY(state.push());
    const int *d_status = &d_state->status;

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;      // XCD-chunked walk of the vector kernels (spmv.hip)
    const int GS = spmv_num_partials(this->A);
    T *partAlpha = this->pslot(0), *partBeta2 = this->pslot(1);

    const bool tracing = this->trace != nullptr;
    const size_t poll = this->poll_interval();
    size_t since_poll = 0;

    // ---- M3 deferred (no preconditioner, one GPU, the lane-per-row kernels of the compressed streams — cfg 3, cfg 4; knob
    // "spmv_fuse"; minres_fuse.hpp): M3 of iteration k — beta_new, the normalisation of v_new, the Givens rotation, p, x, the
    // convergence event — is not launched after M2.  Iteration k + 1 then runs TWO launches: the SpMV on the un-normalised v_new
    // (its prologue gets 1 / beta_new, its gathers multiply by it: spmv_dict_scaled_kernel) and MinresM23 = M3 (k) + M2 (k + 1) in
    // one pass (9 vector passes instead of 8 + 4).  The normalised v_new is never stored: the vector that is "v" of iteration
    // k + 1 and "v_old" of k + 2 stays raw in memory and every reader applies the factor (v_raw / vold_raw below).  Every scalar and
    // element is bit-identical to the three-launch iteration.  M3 is launched on its own where nothing follows it in time — on the
    // last iteration, before a poll of the status word (a convergence is seen as early as without the deferral), while tracing —
    // and then also writes back the normalised form of a raw v, so that the plain kernels find what they expect.
    bool m3_fusable = false;
    if constexpr (std::is_same<T, double>::value || std::is_same<T, cplx>::value)
        m3_fusable = !pc && !this->A->dist && c->spmv_fuse != 0 &&
                     spmv_route(this->A, SpmvPart::Whole, false).kernel == (is_complex<T>::value ? SpmvKernel::Dict : SpmvKernel::DictWide);
    Real<T> *pbeta[2] = {this->dslot(0), this->dslot(1)};     // |v_new|^2 partials: MinresM23 reads one array while it writes the other
    int cur_pb = 0;
    bool deferred = false, v_raw = false, vold_raw = false;
    const T *m3_p_old = nullptr, *m3_p_oold = nullptr; T *m3_p = nullptr;

    for (size_t its = 0;; ++its) {                                          // :90
        const bool done_enqueue = its >= max_iter;
        if (!done_enqueue) {
            const int par = (int)(its & 1);
            { T *tp = v_old; v_old = v; v = v_new; v_new = tp; }             // :92-96
            vold_raw = v_raw; v_raw = deferred;
            const bool will_defer = m3_fusable && !tracing && its + 1 < max_iter && since_poll + 1 < poll;     // M3 of THIS iteration
            if (pc) { T *tp = w; w = w_new; w_new = tp; }                    // :259,264-265
            const T *q = pc ? w : v;                                         // operand of A and source of p
            // M1: v_new = A q (CSMINRES: A conj(q)) ; alpha = conj(q).v_new   (:116 / :271 / cs:99-103)
            const Fin fA = this->fin_for(0, partAlpha, nullptr, GS);
            Part<T> qA, qB2{partBeta2, G};
            Part<Real<T>> qBt{pbeta[cur_pb], G};
            bool iteration_done = false;
            if constexpr (std::is_same<T, double>::value || std::is_same<T, cplx>::value) {
                if (deferred) {
                    // v is the raw v_new of iteration its - 1, v_old = v (its - 1) (raw too unless that iteration began after a flush)
                    deferred = false;
                    auto two_launches = [&](auto sau_tag) -> int {
                        constexpr bool SAU = decltype(sau_tag)::value;
                        MinresM3<T, false, SAU> m3{d_state, par ^ 1, (long long)its - 1, pbeta[cur_pb], partBeta2, G, nullptr, nullptr, v_old, m3_p_old, m3_p_oold, m3_p, x,
                                                   0.0, 0.0, 0.0, 0.0, T(), T(), T(), T()};
                        m3.q_raw = vold_raw ? 1 : 0;
                        SPRS_TRY(this->profiled([&]() -> int { return launch_spmv_scaled<T, SAU>(this->A, m3, v, v_new, partAlpha); }, true));
                        this->stats.fused_k2 += 1;                  // (counted with BiCGStab's fused K2: an SpMV launch that formed its input)
                        this->mark_step(2);
                        return launch_fused<T>(c, n, G, cw, MinresM23<T, SAU>{m3, partAlpha, GS, v, v_new, pbeta[cur_pb ^ 1], T(), T(), T(), 0.0});
                    };
                    if constexpr (is_complex<T>::value) SPRS_TRY(dispatch_bool(sau, two_launches));
                    else SPRS_TRY(two_launches(std::false_type{}));      // (sau is false on real data, which has no conjugating kernels)
                    cur_pb ^= 1;
                    qBt = Part<Real<T>>{pbeta[cur_pb], G};
                    iteration_done = true;
                }
            }
            if (!iteration_done) {
                SPRS_TRY(this->spmv(q, v_new, 1, q, partAlpha, nullptr, d_status, sau, &fA));
                SPRS_TRY(this->handoff(0, GS, partAlpha, &qA));
                // beta_new^2 comes from conj(v_new).w_new (partBeta2) with a preconditioner, else from |v_new|^2 (pbeta)
                const Fin fB = this->fin_for(1, pc ? (const void *)partBeta2 : (const void *)pbeta[cur_pb], nullptr, G);
                // An applied M (ILU(0), AMG): M2 runs without a preconditioner and updates v_new only (its |v_new|^2 partials go to
                // pbeta and are not consumed), w_new = M v_new is a chain of launches of the handle's own (internal.hpp,
                // AppliedPrec), then MinresVW forms the partials of conj(v_new).w_new that M3 expects: 3 launches + 1 application
                // + MinresVW per iteration, no host wait inside one.  Once the status word has left ST_RUNNING the handle's launches
                // still run until the next poll: they read v_new and write only w_new and the handle's scratch, never x, p, v or
                // the state.
                SPRS_TRY(dispatch_bool(dinv != nullptr, [&](auto pc_tag) {
                    return launch_fused<T>(c, n, G, cw, MinresM2<T, V, decltype(pc_tag)::value>{d_state, par, qA.p, qA.P, v_old, v, v_new, dinv, w_new, pbeta[cur_pb], partBeta2, fB, T(), T(), 0.0, T(), qA.tag, this->mb_timeout()});
                }));
                if (applied) {
                    SPRS_TRY(M.apply(v_new, w_new));                                                     // :276
                    SPRS_TRY(launch_fused<T>(c, n, G, cw, MinresVW<T>{d_state, v_new, w_new, partBeta2, T()}));   // :278
                }
                SPRS_TRY(pc ? this->handoff(1, G, partBeta2, &qB2) : this->handoff(1, G, pbeta[cur_pb], &qBt));
            }
            { T *tp = p_oold; p_oold = p_old; p_old = p; p = tp; }           // :151-154
            if (will_defer) {
                // done by the next iteration's two launches (above); the p names as they are now
                deferred = true;
                m3_p_old = p_old; m3_p_oold = p_oold; m3_p = p;
            } else {
                auto m3_alone = [&](auto pc_tag, auto sau_tag) -> int {
                    constexpr bool PCF = decltype(pc_tag)::value, SAF = decltype(sau_tag)::value;
                    MinresM3<T, PCF, SAF> m3{d_state, par, (long long)its, qBt.p, qB2.p, pc ? qB2.P : qBt.P, v_new, w_new, q, p_old, p_oold, p, x,
                                             0.0, 0.0, 0.0, 0.0, T(), T(), T(), T(), pc ? qB2.tag : qBt.tag, this->mb_timeout()};
                    if (!PCF && v_raw) { m3.q_raw = 1; m3.q_back = v; }     // a raw v: used scaled, and left normalised for the plain kernels
                    return launch_fused<T>(c, n, G, cw, m3);
                };
                if (pc) SPRS_TRY(m3_alone(std::true_type{}, std::false_type{}));        // (CSMINRES takes no preconditioner)
                else SPRS_TRY(dispatch_bool(sau, [&](auto sau_tag) { return m3_alone(std::false_type{}, sau_tag); }));
                v_raw = false;
            }
            ++since_poll;
        }
        if (done_enqueue || since_poll >= poll) {
            since_poll = 0;
            SPRS_TRY(state.fetch());
            if ((H.status & 15) == ST_CONVERGED) {                          // :165-167 (0-based its; the word carries the iteration, MinresM3)
                *its_out = (size_t)H.its;
                *res_out = H.st[(H.its + 1) & 1].res_norm / rhs_norm;
                if (tracing) {
                    const MinresState<T> &N = H.st[(H.its + 1) & 1];
                    this->trace_row((double)H.its, N.beta, H.st[H.its & 1].alpha, N.c, sfromr<T>(N.s));
                    if (this->trace_rows) this->trace[8 * (this->trace_rows - 1) + 7] = N.res_norm;
                }
                return SPRS_OK;
            }
            if (H.status == ST_INVALID_PC) {                                // :279-287
                *its_out = (size_t)H.its; *res_out = H.st[H.its & 1].pc_re;
                return SPRS_INVALID_PRECOND;
            }
            if (H.status == ST_COMM_TIMEOUT) return this->comm_timeout();
            if (done_enqueue) break;
            if (tracing) {
                const MinresState<T> &N = H.st[(its + 1) & 1];
                this->trace_row((double)its, N.beta, H.st[its & 1].alpha, N.c, sfromr<T>(N.s));
                if (this->trace_rows) this->trace[8 * (this->trace_rows - 1) + 7] = N.res_norm;
            }
        }
    }
    *its_out = max_iter;                                                    // :171
    return SPRS_INSUFFICIENT_ITER;
}

template <class T>
template <class V>
int MinRes<T>::run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out,
                           Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const bool pc = M.any();
    const bool sau = saunders;
    *its_out = 0; *res_out = 0.0;
    Real<T> rhs_norm = 0.0;
    bool zero;
    SPRS_TRY(this->zero_rhs(rhs, x, &rhs_norm, res_out, &zero));
    if (zero) return SPRS_OK;
    const Real<T> threshold = tol * rhs_norm;
    T cc = sone<T>(), c_old = sone<T>(), eta = sone<T>();
    Real<T> s = 0.0, s_old = 0.0;
    T *v_old = this->vec(0), *v_new = this->vec(1), *v = this->vec(2);
    T *p_old = this->vec(3), *p_oold = this->vec(4), *p = this->vec(5);
    T *w = this->vec(6), *w_new = this->vec(7), *tvec = this->vec(6);
    auto mv = [&](const T *in, T *out) { return this->spmv(in, out, 0, nullptr, nullptr, nullptr, nullptr); };
    auto axpy = [&](T a, const T *xx, T *yy) { return launch_axpy<T, T>(c, n, a, xx, yy); };
    SPRS_TRY(dcopy(c, v_new, rhs, n));
    SPRS_TRY(mv(x, v_old));
    SPRS_TRY(axpy(sneg(sone<T>()), v_old, v_new));
    Real<T> res_norm = 0.0;
    SPRS_TRY(this->norm2(v_new, &res_norm));
    Real<T> beta_new, beta_one;
    if (pc) {
        SPRS_TRY(M.apply(v_new, w_new));
        T b2;
        SPRS_TRY(this->cdot(v_new, w_new, &b2));
        if (sre(b2) < seps<Real<T>>() || sim(b2) > seps<Real<T>>() * sre(b2)) { *res_out = sre(b2); return SPRS_INVALID_PRECOND; }
        beta_new = ssqrt(sre(b2)); beta_one = beta_new;
        SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta_new, v_new));
        SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta_new, w_new));
    } else {
        beta_new = res_norm; beta_one = beta_new;
        SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta_new, v_new));
    }
    SPRS_TRY(dzero(c, v, n)); SPRS_TRY(dzero(c, p_old, n)); SPRS_TRY(dzero(c, p, n));
    for (size_t its = 0; its < max_iter; ++its) {
        const Real<T> beta = beta_new;
        { T *tp = v_old; v_old = v; v = v_new; v_new = tp; }
        T alpha;
        const T *q;
        if (pc) {
            { T *tp = w; w = w_new; w_new = tp; }
            SPRS_TRY(mv(w, v_new));
            SPRS_TRY(this->cdot(w, v_new, &alpha));
            q = w;
        } else if (sau) {
            SPRS_TRY(launch_conj<T>(c, n, v, tvec));
            SPRS_TRY(mv(tvec, v_new));
            SPRS_TRY(this->cdot(v, v_new, &alpha));
            q = tvec;
        } else {
            SPRS_TRY(mv(v, v_new));
            SPRS_TRY(this->cdot(v, v_new, &alpha));
            q = v;
        }
        SPRS_TRY(axpy(sfromr<T>(-beta), v_old, v_new));
        SPRS_TRY(axpy(sneg(alpha), v, v_new));
        if (pc) {
            SPRS_TRY(M.apply(v_new, w_new));
            T b2;
            SPRS_TRY(this->cdot(v_new, w_new, &b2));
            if (sre(b2) < seps<Real<T>>() || sim(b2) > seps<Real<T>>() * sre(b2)) { *its_out = its; *res_out = sre(b2); return SPRS_INVALID_PRECOND; }
            beta_new = ssqrt(sre(b2));
            SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta_new, v_new));
            SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta_new, w_new));
        } else {
            SPRS_TRY(this->norm2(v_new, &beta_new));
            SPRS_TRY(launch_rscale<T>(c, n, Real<T>(1) / beta_new, v_new));
        }
        const Real<T> r3 = s_old * beta;
        const T tr = smulr(sau ? sconj(c_old) : c_old, beta);
        const T r2 = sadd(smulr(alpha, s), smul(cc, tr));
        const T r1_hat = ssub(smul(sau ? sconj(cc) : cc, alpha), smulr(tr, s));
        const Real<T> r1_inv = Real<T>(1) / ssqrt(ssq(r1_hat) + beta_new * beta_new);
        c_old = cc; s_old = s;
        cc = smulr(sau ? sconj(r1_hat) : r1_hat, r1_inv);
        s = beta_new * r1_inv;
        { T *tp = p_oold; p_oold = p_old; p_old = p; p = tp; }
        SPRS_TRY(dcopy(c, p, q, n));
        SPRS_TRY(axpy(sneg(r2), p_old, p));
        SPRS_TRY(axpy(sfromr<T>(-r3), p_oold, p));
        SPRS_TRY(launch_rscale<T>(c, n, r1_inv, p));
        SPRS_TRY(axpy(smulr(smul(cc, eta), beta_one), p, x));
        res_norm *= sabs(s);
        this->trace_row((double)its, beta_new, alpha, cc, sfromr<T>(s));
        if (this->trace && this->trace_rows) this->trace[8 * (this->trace_rows - 1) + 7] = res_norm;
        if (res_norm < threshold) { *its_out = its; *res_out = res_norm / rhs_norm; return SPRS_OK; }
        eta = smulr(eta, -s);
    }
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

template <class T>
int MinRes<T>::solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter,
                         Real<T> tol, size_t *its_out, Real<T> *res_out) {
    return KrylovBase<T>::solve(*this, saunders, P, rhs, rhs_len, x, x_len, max_iter, tol, its_out, res_out);
}

template class MinRes<double>;
template class MinRes<float>;
template class MinRes<cplxf>;
template class MinRes<cplx>;

}  // namespace sprs
