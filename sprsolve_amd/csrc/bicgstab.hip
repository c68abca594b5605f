// BiCGStab (host side).  Reference: src/bicg_stab.rs:35-366.  Kernels: bicg_fuse.hpp, and spmv_chain.hip for the fused SpMV input.
#include "krylov.hpp"

#include <utility>

#include "bicg_fuse.hpp"

namespace sprs {

template <class T>
int BicgStab<T>::create(const sprs_csr *A, size_t size) {
    SPRS_TRY(size_is_rows(A, size));
    SPRS_TRY(this->init(A, size, 7));   // bicg_stab.rs:28 workspace 7n
    return state.create(this->ctx);
}

template <class T>
template <class V>
int BicgStab<T>::run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const V *dinv = M.dinv;
    const bool pc = M.any(), applied = M.applied.h != nullptr;   // the 7-vector layout serves a diagonal and an applied M alike
    *its_out = 0; *res_out = 0.0;

    Real<T> rhs_norm = 0.0;
    bool zero;
    SPRS_TRY(this->zero_rhs(rhs, x, &rhs_norm, res_out, &zero));            // :55-60
    if (zero) return SPRS_OK;
    const Real<T> tol2 = tol * rhs_norm;                             // :61

    // :64-69 / :234-241
    T *r = this->vec(0), *r0 = this->vec(1), *y = this->vec(2);
    T *p = pc ? this->vec(3) : y;
    T *v = pc ? this->vec(4) : this->vec(3);
    T *t = pc ? this->vec(5) : this->vec(4);
    T *z = pc ? this->vec(6) : nullptr;
    // ---- fused SpMV input (f64, no preconditioner, one GPU, plane-streaming chains; knob "spmv_fuse"): the two vector updates
    // whose results are SpMV inputs are formed INSIDE those SpMVs (spmv_chain.hip, FUSE) — K3 (r -= alpha v, :172) in K4, K1
    // (p = (v (-beta w) + p beta) + r, :155-156) in K2 — with K3's / K1's own prologues (bicg_fuse.hpp) and rounding sequence, so
    // every scalar, every element and every dot partial is bit-identical to the five-launch iteration; an iteration is three
    // launches.  K4 does not even store s: K5 forms it again from r and v (BicgK5<SV>) and writes r' = s - w t over r.  A tile reads
    // its operands' windows while other tiles are still reading them, so K2 writes p' to ANOTHER buffer: p alternates with a work
    // vector the unpreconditioned solve leaves unused (:28 allocates seven), and v and t swap roles every iteration (t is dead when K2
    // writes v', v when K4 writes t).
    const SpmvRoute route = spmv_route(this->A, SpmvPart::Whole, false);     // the chains' plan and grid
    bool fuse = false;
    if constexpr (std::is_same<T, double>::value && std::is_same<V, double>::value)
        fuse = !pc && c->spmv_fuse != 0 && route.kernel == SpmvKernel::Chain;
    T *palt = fuse ? this->vec(5) : nullptr;
    // ---- K5 on the chains (knob "bicg_k5", only where the fused input runs): K5 walks the chains as K4 did, with s in its windows, so
    // t = A s need not travel through memory: K4 keeps its two dots and stores nothing, K5 folds t again for its own rows — K4's bits
    // (1) — or, to pin that flow bit for bit, loads the t that K4 stored (2).  Its two dots are grouped by the chain walk, one partial per
    // workgroup of the SpMV grid, so the scalars differ from the vector kernel's K5 (0) in summation order.  r' cannot be written over r
    // (other workgroups still read r's windows): r alternates with the last work vector, as p does with palt.
    // Automatic (-1) selects it only while "spmv_fuse" is automatic too: a caller who sets spmv_fuse = 1 asks for the flow that is
    // bit-identical to spmv_fuse = 0, and that is flavour 0.
    const int k5_knob = c->bicg_k5 >= 0 ? c->bicg_k5 : (c->spmv_fuse < 0 ? BICG_K5_DEFAULT : 0);
    const int k5_chain = fuse ? k5_knob : 0;
    T *ralt = k5_chain ? this->vec(6) : nullptr;
    int pend_k1 = -1, pend_k3 = -1;          // fused: the mode / breakdown flag of the update that the next SpMV forms
    bool s_pending = false;                  // fused: K4 formed s without storing it (K5 forms it again)

    SPRS_TRY(this->spmv(x, r, 0, nullptr, nullptr, nullptr, nullptr));      // :73
    SPRS_TRY((launch_axpy<T, T>(c, n, sneg(sone<T>()), rhs, r)));           // :75
    SPRS_TRY(dcopy(c, r0, r, n));                                           // :78
    Real<T> r0_norm = 0.0;
    SPRS_TRY(this->norm2(r0, &r0_norm));                                    // :80
    if (r0_norm <= tol2) {                                                  // :81-83
        *its_out = 0; *res_out = r0_norm / rhs_norm;
        return SPRS_OK;
    }
    Real<T> r0_norm_tol = r0_norm * seps<Real<T>>();                                     // :84
    r0_norm_tol = r0_norm_tol * r0_norm_tol;                                // :85

    BicgState<T> &H = *state.host;
    BicgState<T> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    H.rho = sfromr<T>(r0_norm * r0_norm);                                   // :88
    H.rho_old = H.rho;
    H.r_norm = r0_norm; H.r0_norm_tol = r0_norm_tol; H.tol2 = tol2;
    H.its = 0; H.status = ST_RUNNING;
    SPRS_TRY(state.push());
    const int *d_status = &d_state->status;

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;      // XCD-chunked walk of the vector kernels (spmv.hip)
    const int GS = spmv_num_partials(this->A);
    Real<T> *partN = this->dslot(0);
    T *partRho = this->pslot(0), *partB = this->pslot(1), *partTT = this->pslot(2), *partTR = this->pslot(3);

    Part<T> qB{partB, GS}, qTT{partTT, GS}, qTR{partTR, GS}, qRho{partRho, G};
    Part<Real<T>> qN{partN, G};
    auto K2 = [&]() -> int {                                                                 // :93/:160  v = A y ; r0.v
        const Fin f = this->fin_for(0, partB, nullptr, GS);
        if constexpr (std::is_same<T, double>::value && std::is_same<V, double>::value) {
            if (fuse && pend_k1 >= 0) {
                const BicgK1<double, double, false> k1{d_state, qN.p, qRho.p, qN.P, pend_k1, v, r, p, nullptr, y, 0.0, 0.0};
                pend_k1 = -1;
                SPRS_TRY(this->profiled([&]() -> int { return launch_chain_k2f(this->A, route, k1, v, p, r, palt, t, r0, partB, d_status); }, true));
                this->stats.fused_k2 += 1;
                this->mark_step(2 | 1);      // (its dot operand is r0)
                std::swap(p, palt); y = p;   // p' lives in the other buffer
                std::swap(v, t);             // v' was written where t was
                return this->handoff(0, GS, partB, &qB);
            }
        }
        SPRS_TRY(this->spmv(y, v, 1, r0, partB, nullptr, d_status, false, &f));
        return this->handoff(0, GS, partB, &qB);
    };
    // An applied M (ILU(0), AMG; right preconditioning as with a diagonal): K1 and K3 run without a preconditioner — K1 writes p
    // only, K3 turns r into s — and y = M p, z = M s are chains of launches of the handle's own (internal.hpp, AppliedPrec)
    // after them: 5 launches + 2 applications per iteration, no host wait inside one.  Once the status word has left ST_RUNNING
    // the handle's launches still run until the next poll: they read p / r and write only y, z and the handle's scratch, never
    // x, r, p, v or the state.  A restart (below) re-enters with K1(mode 1), so p, then y, then z are all rewritten before K5
    // reads them.
    auto K3 = [&](int check) -> int {
        if (fuse) { pend_k3 = check; return (int)SPRS_OK; }     // formed by the next K4
        SPRS_TRY(dispatch_bool(dinv != nullptr, [&](auto pc_tag) {
            return launch_fused<T>(c, n, G, cw, BicgK3<T, V, decltype(pc_tag)::value>{d_state, qB.p, qB.P, check, v, r, dinv, z, T(), qB.tag, this->mb_timeout()});
        }));
        return applied ? M.apply(r, z) : (int)SPRS_OK;                                       // :343
    };
    auto K4 = [&]() -> int {                                                                 // :104/:175 t = A s ; t.t, t.r
        const Fin f = this->fin_for(1, partTT, partTR, GS);
        if constexpr (std::is_same<T, double>::value && std::is_same<V, double>::value) {
            if (fuse && pend_k3 >= 0) {
                const BicgK3<double, double, false> k3{d_state, qB.p, qB.P, pend_k3, v, r, nullptr, nullptr, 0.0};
                pend_k3 = -1;
                SPRS_TRY(this->profiled([&]() -> int { return launch_chain_k4f(this->A, route, k3, r, v, nullptr, t, partTT, partTR, d_status, k5_chain != 1); }, true));
                this->stats.fused_k4 += 1;
                this->mark_step(4);
                s_pending = true;            // s was formed on the fly and not stored: K5 forms it again from r and v
                return this->handoff(1, GS, partTT, &qTT, partTR, &qTR);
            }
        }
        SPRS_TRY(this->spmv(pc ? z : r, t, 2, r, partTT, partTR, d_status, false, &f));
        return this->handoff(1, GS, partTT, &qTT, partTR, &qTR);
    };
    auto K5 = [&]() -> int {
        if constexpr (std::is_same<T, double>::value && std::is_same<V, double>::value) {
            if (k5_chain && s_pending) {     // (not an SpMV launch for the profile: neither timed nor counted as one)
                const BicgK5<double, false, true> k5{d_state, qTT.p, qTR.p, qTT.P, y, nullptr, t, r0, x, r, partN, partRho, Fin{}, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, v};
                SPRS_TRY(launch_chain_k5(this->A, route, k5, ralt, k5_chain == 1));
                this->stats.chain_k5 += 1;
                s_pending = false;
                std::swap(r, ralt);          // r' lives in the other buffer
                return this->handoff(3, GS, partN, &qN, partRho, &qRho);
            }
        }
        const Fin f = this->fin_for(3, partN, partRho, G);
        auto k5 = [&](auto pc_tag, auto sv_tag) {
            constexpr bool PC = decltype(pc_tag)::value, SV = decltype(sv_tag)::value;
            return launch_fused<T>(c, n, G, cw, BicgK5<T, PC, SV>{d_state, qTT.p, qTR.p, qTT.P, y, z, t, r0, x, r, partN, partRho, f, T(), T(), T(), 0.0, T(), qTT.tag, this->mb_timeout(), SV ? v : nullptr});
        };
        if (s_pending) SPRS_TRY(k5(std::false_type{}, std::true_type{}));      // (only ever without a preconditioner)
        else SPRS_TRY(dispatch_bool(pc, [&](auto pc_tag) { return k5(pc_tag, std::false_type{}); }));
        s_pending = false;
        return this->handoff(3, G, partN, &qN, partRho, &qRho);
    };
    auto K1 = [&](int mode) -> int {
        if (fuse) { pend_k1 = mode; return (int)SPRS_OK; }      // formed by the next K2
        SPRS_TRY(dispatch_bool(dinv != nullptr, [&](auto pc_tag) {
            return launch_fused<T>(c, n, G, cw, BicgK1<T, V, decltype(pc_tag)::value>{d_state, qN.p, qRho.p, qN.P, mode, v, r, p, dinv, y, T(), T(), qN.tag, this->mb_timeout()});
        }));
        return applied ? M.apply(p, y) : (int)SPRS_OK;                                       // :328
    };

    // ---- unrolled first iteration (:87-120 / :258-293)
    if (pc) {
        SPRS_TRY(dcopy(c, p, r, n));                                        // :261
        SPRS_TRY(M.apply(p, y));                                            // :262
    } else {
        SPRS_TRY(dcopy(c, y, r, n));                                        // :91
    }
    SPRS_TRY(K2()); SPRS_TRY(K3(0)); SPRS_TRY(K4()); SPRS_TRY(K5());
    const bool tracing = this->trace != nullptr;
    if (tracing) {
        SPRS_TRY(state.fetch());
        this->trace_row(0.0, r0_norm, H.rho, H.alpha, H.w);
    }

    // ---- main loop (:122-197)
    const size_t poll = this->poll_interval();
    size_t its = 1, since_poll = 0;
    int resume_mode = 0;
    while (true) {
        const bool done_enqueue = its >= max_iter;
        if (!done_enqueue) {
            SPRS_TRY(K1(resume_mode)); resume_mode = 0;
            SPRS_TRY(K2()); SPRS_TRY(K3(1)); SPRS_TRY(K4()); SPRS_TRY(K5());
            ++its; ++since_poll;
        }
        if (done_enqueue || since_poll >= poll) {
            since_poll = 0;
            SPRS_TRY(state.fetch());
            if (H.status == ST_CONVERGED) {                                 // :124-126
                *its_out = (size_t)H.its; *res_out = H.r_norm / rhs_norm;
                return SPRS_OK;
            }
            if (H.status == ST_BREAKDOWN) {                                 // :164-167
                *its_out = (size_t)H.its;
                return SPRS_BREAKDOWN;
            }
            if (H.status == ST_COMM_TIMEOUT) return this->comm_timeout();
            if (H.status == ST_RESTART) {                                   // :131-145, executed at iteration H.its
                // K2 / K4 of the iterations enqueued from the requesting one on returned at their first instruction
                this->profile_discard_last(2 * (its - (size_t)H.its));
                if (fuse && ((its - (size_t)H.its) & 1)) {
                    // ... but the host rotated the buffers once for each of them as it enqueued: an odd number of idle iterations
                    // leaves every pair of names exchanged against what the last EXECUTED launches wrote
                    std::swap(p, palt); y = p; std::swap(v, t);
                    if (k5_chain) std::swap(r, ralt);
                }
                SPRS_TRY(this->spmv(x, r, 0, nullptr, nullptr, nullptr, nullptr));  // :134
                SPRS_TRY((launch_axpy<T, T>(c, n, sneg(sone<T>()), rhs, r)));       // :137
                SPRS_TRY(dcopy(c, r0, r, n));                                       // :140
                Real<T> rn = 0.0;
                SPRS_TRY(this->norm2(r, &rn));                                      // :142
                H.rho = sfromr<T>(rn * rn);                                         // :143
                H.r0_norm_tol = sre(H.rho) * seps<Real<T>>() * seps<Real<T>>();                             // :144
                H.status = ST_RUNNING;
                SPRS_TRY(state.push());
                its = (size_t)H.its;       // every kernel after the request was a no-op: redo from here
                resume_mode = 1;
                continue;
            }
            if (tracing && !done_enqueue) this->trace_row((double)(H.its - 1), H.r_norm, H.rho, H.alpha, H.w);
            if (done_enqueue) break;
        }
    }
    *its_out = max_iter;                                                    // :199
    return SPRS_INSUFFICIENT_ITER;
}

// literal mode: the reference's op list, one kernel per op, host-consumed scalars
template <class T>
template <class V>
int BicgStab<T>::run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out,
                             Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const bool pc = M.any();
    *its_out = 0; *res_out = 0.0;
    Real<T> rhs_norm = 0.0;
    bool zero;
    SPRS_TRY(this->zero_rhs(rhs, x, &rhs_norm, res_out, &zero));
    if (zero) return SPRS_OK;
    const Real<T> tol2 = tol * rhs_norm;
    T *r = this->vec(0), *r0 = this->vec(1), *y = this->vec(2);
    T *p = pc ? this->vec(3) : y;
    T *v = pc ? this->vec(4) : this->vec(3);
    T *t = pc ? this->vec(5) : this->vec(4);
    T *z = pc ? this->vec(6) : nullptr;
    const T *sz = pc ? z : r;
    auto mv = [&](const T *in, T *out) { return this->spmv(in, out, 0, nullptr, nullptr, nullptr, nullptr); };
    auto cdot = [&](const T *a, const T *b, T *o) { return this->cdot(a, b, o); };
    auto axpy = [&](T a, const T *xx, T *yy) { return launch_axpy<T, T>(c, n, a, xx, yy); };

    SPRS_TRY(mv(x, r));
    SPRS_TRY(axpy(sneg(sone<T>()), rhs, r));
    SPRS_TRY(dcopy(c, r0, r, n));
    Real<T> r0_norm = 0.0;
    SPRS_TRY(this->norm2(r0, &r0_norm));
    if (r0_norm <= tol2) { *res_out = r0_norm / rhs_norm; return SPRS_OK; }
    Real<T> r0_norm_tol = r0_norm * seps<Real<T>>();
    r0_norm_tol = r0_norm_tol * r0_norm_tol;
    T rho = sfromr<T>(r0_norm * r0_norm);
    if (pc) { SPRS_TRY(dcopy(c, p, r, n)); SPRS_TRY(M.apply(p, y)); }
    else SPRS_TRY(dcopy(c, y, r, n));
    SPRS_TRY(mv(y, v));
    T tmp;
    SPRS_TRY(cdot(r0, v, &tmp));
    T alpha = sdiv(rho, tmp);
    SPRS_TRY(axpy(sneg(alpha), v, r));
    if (pc) SPRS_TRY(M.apply(r, z));
    SPRS_TRY(mv(sz, t));
    SPRS_TRY(cdot(t, t, &tmp));
    T w = szero<T>();
    if (sre(tmp) > 0.0) { T tr; SPRS_TRY(cdot(t, r, &tr)); w = sdiv(tr, tmp); }
    SPRS_TRY(axpy(sneg(alpha), y, x));
    SPRS_TRY(axpy(sneg(w), sz, x));
    SPRS_TRY(axpy(sneg(w), t, r));
    this->trace_row(0.0, r0_norm, rho, alpha, w);
    for (size_t its = 1; its < max_iter; ++its) {
        Real<T> r_norm = 0.0;
        SPRS_TRY(this->norm2(r, &r_norm));
        if (r_norm <= tol2) { *its_out = its; *res_out = r_norm / rhs_norm; return SPRS_OK; }
        const T rho_old = rho;
        SPRS_TRY(cdot(r0, r, &rho));
        if (sabs(rho) < r0_norm_tol) {
            SPRS_TRY(mv(x, r));
            SPRS_TRY(axpy(sneg(sone<T>()), rhs, r));
            SPRS_TRY(dcopy(c, r0, r, n));
            Real<T> rn = 0.0;
            SPRS_TRY(this->norm2(r, &rn));
            rho = sfromr<T>(rn * rn);
            r0_norm_tol = sre(rho) * seps<Real<T>>() * seps<Real<T>>();
        }
        const T beta = smul(sdiv(rho, rho_old), sdiv(alpha, w));
        SPRS_TRY(launch_axpby<T>(c, n, smul(sneg(beta), w), v, beta, p));
        SPRS_TRY(axpy(sone<T>(), r, p));
        if (pc) SPRS_TRY(M.apply(p, y));
        SPRS_TRY(mv(y, v));
        SPRS_TRY(cdot(r0, v, &tmp));
        if (sabs(tmp) <= 0.0) { *its_out = its; return SPRS_BREAKDOWN; }
        alpha = sdiv(rho, tmp);
        SPRS_TRY(axpy(sneg(alpha), v, r));
        if (pc) SPRS_TRY(M.apply(r, z));
        SPRS_TRY(mv(sz, t));
        SPRS_TRY(cdot(t, t, &tmp));
        if (sre(tmp) > 0.0) { T tr; SPRS_TRY(cdot(t, r, &tr)); w = sdiv(tr, tmp); }
        else w = szero<T>();
        SPRS_TRY(axpy(sneg(alpha), y, x));
        SPRS_TRY(axpy(sneg(w), sz, x));
        SPRS_TRY(axpy(sneg(w), t, r));
        this->trace_row((double)its, r_norm, rho, alpha, w);
    }
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

template <class T>
int BicgStab<T>::solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter,
                           Real<T> tol, size_t *its_out, Real<T> *res_out) {
    return KrylovBase<T>::solve(*this, false, P, rhs, rhs_len, x, x_len, max_iter, tol, its_out, res_out);
}

template class BicgStab<double>;
template class BicgStab<float>;
template class BicgStab<cplxf>;
template class BicgStab<cplx>;

}  // namespace sprs
