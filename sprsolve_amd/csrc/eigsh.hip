// Thick-restart Lanczos (Wu & Simon; = Hermitian Krylov-Schur) with full reorthogonalisation by CGS2: the recurrence of the
// header's sprs_eigsh_* comment.  The host enqueues whole cycles blind — per step SpMV, launch_cgs2 against v_0 .. v_j, LzStep,
// GmScale; per cycle LzRitz — and reads the head of the state once a cycle, to choose between the restart
// (LzRotate in place + one copy) and the end (LzRotate into the caller's vectors).  Kernels: eigsh_fuse.hpp, gmres_fuse.hpp.
#include "krylov.hpp"

#include <algorithm>

#include "eigsh_fuse.hpp"

namespace sprs {

template <class T>
int Eigsh<T>::create(const sprs_csr *A, size_t size, size_t ncv) {
    SPRS_TRY(single_gpu_only(A, "sprs_eigsh"));
    if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
    if ((int64_t)size != A->nrows) return SPRS_DIM_MISMATCH;
    if (ncv == 0) ncv = std::min<size_t>(32, size);
    if (ncv < 3 || ncv > std::min<size_t>(SPRS_EIGSH_MAX_NCV, size))
        return refuse(A->ctx, "sprs_eigsh", "ncv = %zu is outside 3 .. min(%d, n = %zu)", ncv, SPRS_EIGSH_MAX_NCV, size);
    m = (int)ncv;
    SPRS_TRY(this->init(A, size, m + 2));   // v_0 .. v_m, w
    sprs_ctx *c = this->ctx;
    SPRS_TRY(state.create(c));
    SPRS_HIP_TRY(c, hipMemsetAsync(state.dev, 0, sizeof(LzState<T>), c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
void Eigsh<T>::destroy() {
    state.destroy();
    dots.destroy();
    KrylovBase<T>::destroy();
}

// out[:, c] = sum_i V[:, i] S[i, c], c < q, i < me: one LzRotate launch
template <class T>
int Eigsh<T>::rotate(int me, int q, T *out, int64_t ostride) {
    return launch_lz_rotate<T, Real<T>>(this->ctx, (const Real<T> *)state.dev->coef, (const T *)basis(0), (int64_t)this->stride, (int64_t)this->n, me, q, out, ostride);
}

template <class T>
int Eigsh<T>::solve(size_t k, int which, const T *v0, bool v0_host, size_t max_restarts, Real<T> tol, Real<T> *vals_out, T *vecs, bool vecs_host,
                    Real<T> *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out) {
    using St = LzState<T>;
    using Hd = LzHead<T>;
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    SPRS_TRY(this->begin_solve());

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;
    SPRS_TRY(dots.ensure(c, LZ_MAXM, G));

    Hd &H = state.host->hd;
    St *const d_state = state.dev;
    SPRS_TRY(lz_begin(state, k, which, tol));                               // T = 0, anorm = 0, scale = 0, the counters
    const Hd *d_head = &d_state->hd;
    const int *d_skip = &d_state->hd.skip;

    T *Vb = basis(0), *w = wvec();
    const int64_t vs = (int64_t)this->stride;
    Real<T> *partN = this->dslot(0);
    auto step = [&](int j, long long cycle) -> int {
        T *vj = Vb + (size_t)j * this->stride, *vn = Vb + (size_t)(j + 1) * this->stride;
        SPRS_TRY(this->spmv(vj, w, 0, nullptr, nullptr, nullptr, d_skip));                          // w = A v_j
        SPRS_TRY(launch_cgs2<T>(c, n, G, cw, d_state, Vb, vs, j + 1, w, vn, partN, dots.p));            // against v_0 .. v_j
        SPRS_TRY(launch_small(c, lz_step_kernel<T>, 0, d_state, (const Real<T> *)partN, G, j, m, cycle));
        return launch_fused<T>(c, n, G, cw, GmScale<T, Hd>{d_head, vn, 0.0});
    };

    // v_0 = v0 / |v0|
    SPRS_HIP_TRY(c, hipMemcpyAsync(Vb, v0, sizeof(T) * n, v0_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    SPRS_TRY(launch_fused<T>(c, n, G, cw, LzNrm<T>{Vb, partN, 0.0}));
    SPRS_TRY(launch_small(c, lz_start_kernel<T, St>, 0, d_state, (const Real<T> *)partN, G));
    SPRS_TRY(launch_fused<T>(c, n, G, cw, GmScale<T, Hd>{d_head, Vb, 0.0}));

    const int p = std::min((int)k + std::max((int)k, 4), m - 2);
    int j0 = 0;
    for (long long cycle = 1;; ++cycle) {
        for (int j = j0; j < m; ++j) SPRS_TRY(step(j, cycle));
        SPRS_TRY(launch_small(c, lz_ritz_kernel<T>, 0, d_state, m, p));
        SPRS_TRY(state.fetch(sizeof(Hd)));
        if (H.status != ST_RUNNING || (size_t)cycle >= max_restarts) break;
        SPRS_TRY(rotate(m, p, Vb, vs));                                                             // V[:, :p] <- V[:, :m] S[:, :p]
        SPRS_TRY(dcopy(c, basis(p), (const T *)basis(m), n));                                       // v_p <- v_m
        j0 = p;
    }

    const int rc = lz_results(state, k, state.host->theta, vals_out, res_out, nconv_out, restarts_out, matvecs_out);
    if (rc != SPRS_OK && rc != SPRS_INSUFFICIENT_ITER) return rc;           // a breakdown: no vectors
    if (vecs) {     // X = V[:, :m_eff] S[:, :k]
        if (vecs_host) {
            SPRS_TRY(rotate(H.m_eff, (int)k, Vb, vs));
            for (size_t i = 0; i < k; ++i)
                SPRS_HIP_TRY(c, hipMemcpyAsync(vecs + i * n, basis((int)i), sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
        } else {
            SPRS_TRY(rotate(H.m_eff, (int)k, vecs, (int64_t)n));
        }
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    SPRS_TRY(this->end_solve());
    return rc;
}

template class Eigsh<double>;
template class Eigsh<float>;
template class Eigsh<cplxf>;
template class Eigsh<cplx>;

}  // namespace sprs
