// IDR(s) (host side): Idrs<T>, the bi-orthogonal IDR(s) of the header's sprs_idrs_* comment, right-preconditioned by nothing, a
// diagonal or an applied ILU(0) / AMG / FSAI handle (one host path, Prec<T, V> of krylov.hpp).
// Fused only (idrs_fuse.hpp): the host enqueues products blind — an inner step k is IdrsA [an applied M: IdrsA<2>, its launches,
// IdrsA2], SpMV, IdrsDots, IdrsB; the omega step is idrs_check, [IdrsPrec, or an applied M's launches], SpMV with its two dots
// [f32 / c32: SpMV, IdrsDots], IdrsW [complex T: and IdrsDots for the next f] — and reads the head of the state every poll_interval() products.  The
// results do not depend on `poll`: after an event every later launch returns at its first instruction.
// Of KrylovBase it uses the work vectors (r, v, vh, t, then s columns each of G, U and P), the partial slots, spmv() and the
// trace — no literal mode or profile.  The shadow space P is built once at creation: gen_uniform's streams 200 + .., CGS2
// against the earlier columns and a real scale by 1 / norm2, in double on the host, rounded to T.
#include "krylov.hpp"

#include <cmath>
#include <vector>

#include "idrs_fuse.hpp"

namespace sprs {

template <class T>
int Idrs<T>::create(const sprs_csr *A_, size_t size, size_t s_dim) {
    this->A = A_; this->ctx = A_->ctx;
    sprs_ctx *c = this->ctx;
    SPRS_TRY(size_is_rows(A_, size));
    if (s_dim > (size_t)IDRS_MAXS) return refuse(c, "sprs_idrs", "s = %zu is larger than SPRS_IDRS_MAX_S = %d", s_dim, IDRS_MAXS);
    s = s_dim == 0 ? 4 : (int)s_dim;
    if ((size_t)s > size) return refuse(c, "sprs_idrs", "s = %d is larger than the system (%zu rows)", s, size);
    SPRS_TRY(single_gpu_only(A_, "sprs_idrs"));
    SPRS_TRY(this->init(A_, size, 4 + 3 * s));          // r, v, vh, t ; G's, U's and P's columns
    SPRS_TRY(state.create(c));

    // The shadow space: column col holds gen_uniform's stream 200 + 2 col (imaginary parts: 201 + 2 col) rounded to T.  The
    // columns are orthonormalised here, once, in double (CGS2 against the earlier columns: both passes take all their dot
    // products on the same w, then subtract in ascending order; a real scale by 1 / norm2) and rounded to T at the end, so that
    // P is the same to the last bit wherever the same statement is evaluated in double (tests/_idrs_ref.py does).
    using D = Dbl<T>;
    const size_t n = this->n;
    std::vector<D> Pd((size_t)s * n);
    for (int cl = 0; cl < s; ++cl) {
        D *w = Pd.data() + (size_t)cl * n;
        for (size_t i = 0; i < n; ++i) {
            T v = sfromr<T>((Real<T>)gen_uniform(200 + 2 * (uint64_t)cl, i));
            if constexpr (is_complex<T>::value) v.im = (Real<T>)gen_uniform(201 + 2 * (uint64_t)cl, i);
            w[i] = to_dbl(v);
        }
        for (int pass = 0; pass < (cl > 0 ? 2 : 0); ++pass) {
            D h[IDRS_MAXS];
            for (int b = 0; b < cl; ++b) {
                const D *pb = Pd.data() + (size_t)b * n;
                D acc = szero<D>();
                for (size_t i = 0; i < n; ++i) acc = sadd(acc, smul(sconj(pb[i]), w[i]));
                h[b] = acc;
            }
            for (int b = 0; b < cl; ++b) {
                const D *pb = Pd.data() + (size_t)b * n;
                const D nh = sneg(h[b]);
                for (size_t i = 0; i < n; ++i) w[i] = sadd(w[i], smul(pb[i], nh));
            }
        }
        double nn = 0.0;
        for (size_t i = 0; i < n; ++i) nn += dbl_sq(w[i]);
        const double nrm = std::sqrt(nn);
        if (!(nrm > 0.0) || !std::isfinite(nrm)) {
            snprintf(c->err, sizeof(c->err), "sprs_idrs: column %d of the shadow space depends on the earlier ones", cl);
            return SPRS_INVALID_ARGUMENT;
        }
        const double sc = 1.0 / nrm;
        for (size_t i = 0; i < n; ++i) w[i] = smulr(w[i], sc);
    }
    std::vector<T> col(n);
    for (int cl = 0; cl < s; ++cl) {
        for (size_t i = 0; i < n; ++i) col[i] = from_dbl<T>(Pd[(size_t)cl * n + i]);
        SPRS_HIP_TRY(c, hipMemcpyAsync(pvec(cl), col.data(), sizeof(T) * n, hipMemcpyHostToDevice, c->stream));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));           // (`col` is refilled)
    }
    return SPRS_OK;
}

template <class T>
template <class V>
int Idrs<T>::run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out) {
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const V *dinv = M.dinv;
    const bool pc = M.any(), applied = M.applied.h != nullptr;
    *its_out = 0; *res_out = 0.0;

    Real<T> rhs_norm = 0.0;
    bool zero;
    SPRS_TRY(this->zero_rhs(rhs, x, &rhs_norm, res_out, &zero));
    if (zero) return SPRS_OK;
    const Real<T> tol2 = tol * rhs_norm;

    T *r = this->vec(0), *v = this->vec(1), *vh = this->vec(2), *t = this->vec(3);
    T *Gb = gvec(0), *Ub = uvec(0), *Pb = pvec(0);
    const int64_t vs = (int64_t)this->stride;
    SPRS_TRY(this->spmv(x, r, 0, nullptr, nullptr, nullptr, nullptr));              // r = A x
    SPRS_TRY(launch_axpby<T>(c, n, sone<T>(), rhs, sneg(sone<T>()), r));            // r = rhs*1 + r*(-1)
    Real<T> r0_norm = 0.0;
    SPRS_TRY(this->norm2(r, &r0_norm));
    if (r0_norm <= tol2) {
        *res_out = r0_norm / rhs_norm;
        return SPRS_OK;
    }
    SPRS_TRY(dzero(c, Gb, (size_t)vs * (size_t)(2 * s)));                           // G = U = 0

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;      // XCD-chunked walk of the vector kernels (spmv.hip)
    const int GS = spmv_num_partials(this->A);
    // the partials, all of the small quantities' type: [s][G] for q and for f, one row for |r|^2 (doubles), two for conj(r).t, conj(t).t
    using D = Dbl<T>;
    constexpr bool WIDE = sizeof(Real<T>) == 8;         // T is its own wide type: the SpMV's fused dots are the recurrence's
    SPRS_TRY(dots.ensure(c, 2 * IDRS_MAXS + 3, G));
    D *partQ = dots.p, *partF = dots.p + (size_t)IDRS_MAXS * (size_t)G;
    double *partN = reinterpret_cast<double *>(dots.p + (size_t)(2 * IDRS_MAXS) * (size_t)G);
    D *partRT = dots.p + (size_t)(2 * IDRS_MAXS + 1) * (size_t)G;

    IdrsState<T> &H = *state.host;
    IdrsState<T> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    H.hd.max_iter = (long long)max_iter; H.hd.status = ST_RUNNING;
    H.hd.r_norm = (double)r0_norm; H.hd.tol2 = (double)tol2; H.hd.r0sq = (double)r0_norm * (double)r0_norm;
    H.omega = to_dbl(sone<T>());
    for (int i = 0; i < IDRS_MAXS; ++i) H.M[i][i] = to_dbl(sone<T>());
    SPRS_TRY(state.push());
    auto fetch_head = [&]() -> int { return state.fetch(sizeof(IdrsHead<T>)); };
    const IdrsHead<T> *d_head = &d_state->hd;
    const int *d_status = &d_state->hd.status;

    constexpr int B = idrs_b<T>::value;
    constexpr bool FUSE_F = idrs_fuse_f<T>::value;
    auto multi_dot = [&](const T *w, D *part) -> int {                              // partials of conj(p_b).w, b < s
        for (int i0 = 0; i0 < s; i0 += B)
            SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsDots<T, B>{d_head, Pb + (int64_t)i0 * vs, vs, std::min(B, s - i0), w, part + (size_t)i0 * (size_t)G, G, {}}));
        return SPRS_OK;
    };
    int PN = 0;                                         // 0 until a step has left the partials of |r|^2
    auto inner = [&](int k, long long it) -> int {
        T *uk = Ub + (size_t)k * this->stride, *gk = Gb + (size_t)k * this->stride;
        const D *pf = k == 0 ? partF : nullptr;
        if (applied) {
            SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsA<T, V, 2>{d_state, partN, PN, pf, G, G, s, k, it, r, Gb, Ub, vs, nullptr, v, nullptr, T()}));
            SPRS_TRY(M.apply(v, vh));                                               // vh = M v
            SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsA2<T>{d_state, s, k, vh, Ub, vs, nullptr, T()}));
        } else if (pc) {
            SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsA<T, V, 1>{d_state, partN, PN, pf, G, G, s, k, it, r, Gb, Ub, vs, dinv, uk, nullptr, T()}));
        } else {
            SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsA<T, V, 0>{d_state, partN, PN, pf, G, G, s, k, it, r, Gb, Ub, vs, nullptr, uk, nullptr, T()}));
        }
        SPRS_TRY(this->spmv(uk, gk, 0, nullptr, nullptr, nullptr, d_status));       // g_k = A u_k
        SPRS_TRY(multi_dot(gk, partQ));                                             // q = P^H g_k
        SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsB<T>{d_state, partQ, G, G, s, k, it, Gb, Ub, vs, r, x, partN, nullptr, T(), T(), 0.0}));
        PN = G;
        return SPRS_OK;
    };
    auto omega_step = [&](long long it) -> int {
        SPRS_TRY(launch_small(c, idrs_check_kernel<T>, 0, d_state, (const double *)partN, PN, it));
        if (applied) SPRS_TRY(M.apply(r, vh));                                      // vh = M r
        else if (pc) SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsPrec<T, V>{d_head, dinv, r, vh}));
        const D *pTT, *pTR; int PT;
        if constexpr (WIDE) {
            T *partTT = this->pslot(0), *partTR = this->pslot(1);
            SPRS_TRY(this->spmv(pc ? vh : r, t, 2, r, partTT, partTR, d_status));   // t = A vh ; conj(t).t, conj(t).r
            pTT = partTT; pTR = partTR; PT = GS;
        } else {
            // f32 / c32: the SpMV's fused dots are summed in T — conj(r).t and conj(t).t in double from one more read of t
            // (r = vec(0) and t = vec(3): two "columns" three strides apart)
            SPRS_TRY(this->spmv(pc ? vh : r, t, 0, nullptr, nullptr, nullptr, d_status));
            SPRS_TRY(launch_fused<T>(c, n, G, cw, IdrsDots<T, B>{d_head, r, 3 * vs, 2, t, partRT, G, {}}));
            pTR = partRT; pTT = partRT + G; PT = G;
        }
        SPRS_TRY(dispatch_bool(pc, [&](auto pc_tag) {
            return launch_fused<T>(c, n, G, cw, IdrsW<T, decltype(pc_tag)::value, FUSE_F, !WIDE>{d_state, pTT, pTR, PT, s, it, vh, t, Pb, vs, x, r, partN, partF, G, T(), T(), 0.0, {}});
        }));
        PN = G;
        if (!FUSE_F) SPRS_TRY(multi_dot(r, partF));                                 // f = P^H r, a launch of its own
        return SPRS_OK;
    };

    SPRS_TRY(multi_dot(r, partF));                                                  // the first cycle's f

    const bool tracing = this->trace != nullptr;
    const size_t poll = this->poll_interval();
    size_t enq = 0, since_poll = 0;
    long long traced = 0;
    int k = 0;
    bool closed = false;
    while (true) {
        const bool done_enqueue = enq >= max_iter;
        if (!done_enqueue) {
            if (k < s) SPRS_TRY(inner(k, (long long)enq));
            else SPRS_TRY(omega_step((long long)enq));
            k = k == s ? 0 : k + 1;
            ++enq; ++since_poll;
        } else if (!closed) {                                                       // the events of the last product
            SPRS_TRY(launch_small(c, idrs_check_kernel<T>, 0, d_state, (const double *)partN, PN, (long long)enq));
            closed = true;
        }
        if (done_enqueue || since_poll >= poll) {
            since_poll = 0;
            SPRS_TRY(fetch_head());
            if (tracing && H.hd.its > traced && H.hd.status != ST_BREAKDOWN) {
                traced = H.hd.its;
                if (this->trace_rows < this->trace_cap) {
                    double *row = this->trace + 8 * this->trace_rows;
                    row[0] = (double)H.hd.its; row[1] = H.hd.r_norm;
                    row[2] = H.hd.tr[0]; row[3] = H.hd.tr[1]; row[4] = H.hd.tr[2]; row[5] = H.hd.tr[3];
                    row[6] = (double)H.hd.kind; row[7] = 0.0;
                    ++this->trace_rows;
                }
            }
            if (done_enqueue || H.hd.status != ST_RUNNING) break;
        }
    }
    if (H.hd.status == ST_CONVERGED) {
        *its_out = (size_t)H.hd.its; *res_out = (Real<T>)(H.hd.r_norm / (double)rhs_norm);
        return SPRS_OK;
    }
    if (H.hd.status == ST_BREAKDOWN) {
        *its_out = (size_t)H.hd.its;
        return SPRS_BREAKDOWN;
    }
    *its_out = max_iter;
    return SPRS_INSUFFICIENT_ITER;
}

template <class T>
int Idrs<T>::solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                       size_t *its_out, Real<T> *res_out) {
    return KrylovBase<T>::solve(*this, false, P, rhs, rhs_len, x, x_len, max_iter, tol, its_out, res_out);
}

template class Idrs<double>;
template class Idrs<float>;
template class Idrs<cplxf>;
template class Idrs<cplx>;

}  // namespace sprs
