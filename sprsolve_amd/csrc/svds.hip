// Thick-restart Lanczos bidiagonalisation (Golub-Kahan; Baglama & Reichel's restart with plain Ritz vectors) with full
// reorthogonalisation of both bases by CGS2: the recurrence of the header's sprs_svds_* comment.  The host enqueues whole cycles
// blind — per step SpMV, launch_cgs2 against q_0 .. q_{j-1}, SvNorm<alpha>, GmScale, SpMV, launch_cgs2 against p_0 .. p_j,
// SvNorm<beta>, GmScale; per cycle SvSvd — and reads the head of the state once a cycle, to choose between
// the restart (LzRotate in place on both bases + one copy) and the end (LzRotate into the caller's vectors).  Kernels:
// svds_fuse.hpp, eigsh_fuse.hpp, gmres_fuse.hpp.
#include "krylov.hpp"

#include <algorithm>

#include "svds_fuse.hpp"

extern "C" int sprs_csr_adjoint(const sprs_csr *A, int conjugate, sprs_csr **out);

namespace sprs {

template <class T>
int Svds<T>::create(const sprs_csr *A, const sprs_csr *AH_or_null, size_t ncv) {
    const sprs_csr *H = AH_or_null;
    SPRS_TRY(single_gpu_only(A, "sprs_svds", H));
    if (H && (H->dtype != A->dtype || H->ctx != A->ctx)) return refuse(A->ctx, "sprs_svds", "the adjoint handle holds another scalar type or context");
    if (H && (H->nrows != A->ncols || H->ncols != A->nrows)) return refuse(A->ctx, "sprs_svds", "the adjoint handle is not cols x rows");
    const size_t small = (size_t)std::min(A->nrows, A->ncols);
    if (ncv == 0) ncv = std::min<size_t>(32, small);
    if (ncv < 3 || ncv > std::min<size_t>(SPRS_SVDS_MAX_NCV, small))
        return refuse(A->ctx, "sprs_svds", "ncv = %zu is outside 3 .. min(%d, min(rows, cols) = %zu)", ncv, SPRS_SVDS_MAX_NCV, small);
    if (H) AH = H;
    else {
        SPRS_TRY(sprs_csr_adjoint(A, 1, &own_AH));
        AH = own_AH;
    }
    m = (int)ncv;
    rows = (size_t)A->nrows; cols = (size_t)A->ncols;
    swapped = rows < cols;
    Op = swapped ? AH : A; OpH = swapped ? A : AH;
    lenM = std::max(rows, cols); lenN = std::min(rows, cols);
    SPRS_TRY(this->init(A, lenM, m + 1));                // q_0 .. q_{m-1}, w
    sprs_ctx *c = this->ctx;
    stride_n = (lenN + 31) & ~(size_t)31;
    SPRS_HIP_TRY(c, hipMalloc((void **)&work_n, sizeof(T) * stride_n * (size_t)(m + 2)));   // p_0 .. p_m, w'
    SPRS_HIP_TRY(c, hipMemsetAsync(work_n, 0, sizeof(T) * stride_n * (size_t)(m + 2), c->stream));
    SPRS_TRY(state.create(c));
    SPRS_HIP_TRY(c, hipMemsetAsync(state.dev, 0, sizeof(SvState<T>), c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
void Svds<T>::destroy() {
    state.destroy();
    dots.destroy();
    if (work_n) (void)hipFree(work_n);
    work_n = nullptr;
    KrylovBase<T>::destroy();
    if (own_AH) (void)sprs_csr_destroy(own_AH);
    own_AH = nullptr; AH = Op = OpH = nullptr;
}

template <class T>
int Svds<T>::grid_of(size_t len) const {
    constexpr int PKW = pack_width<T>::value;
    return balanced_grid(this->ctx, ((int64_t)len / PKW + BLOCK - 1) / BLOCK);
}

template <class T>
int Svds<T>::solve(size_t k, int which, const T *v0, bool host, size_t max_restarts, R tol, R *vals_out, T *u, T *v, R *res_out,
                   size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out) {
    using St = SvState<T>;
    using Hd = LzHead<T>;
    sprs_ctx *c = this->ctx;
    const size_t M = lenM, N = lenN;
    SPRS_TRY(this->begin_solve());

    const int GM = grid_of(M), GN = grid_of(N), G = std::max(GM, GN);
    const int cwM = fused_chunked(Op) ? 1 : 0, cwN = fused_chunked(OpH) ? 1 : 0;    // (a handle's rows are its output's length)
    SPRS_TRY(dots.ensure(c, LZ_MAXM, G));

    Hd &H = state.host->hd;
    St *const d_state = state.dev;
    SPRS_TRY(lz_begin(state, k, which, tol));                               // B = 0, anorm = 0, pscale = 0, the counters
    const Hd *d_head = &d_state->hd;
    const int *d_skip = &d_state->hd.skip;

    T *Pb = pvec(0), *Qb = qvec(0), *wN = pvec(m + 1), *wM = qvec(m);
    const int64_t ps = (int64_t)stride_n, qs = (int64_t)this->stride;
    R *partN = this->dslot(0);
    auto step = [&](int j, long long cycle) -> int {
        T *pj = Pb + (size_t)j * stride_n, *pn = Pb + (size_t)(j + 1) * stride_n, *qj = Qb + (size_t)j * this->stride;
        if (j == 0) {                                                                               // nothing to orthogonalise against
            SPRS_TRY(launch_spmv<T>(Op, SpmvPart::Whole, pj, qj, 0, nullptr, nullptr, nullptr, d_skip));
            SPRS_TRY(launch_fused<T>(c, M, GM, cwM, LzNrm<T>{qj, partN, 0.0}));
        } else {
            SPRS_TRY(launch_spmv<T>(Op, SpmvPart::Whole, pj, wM, 0, nullptr, nullptr, nullptr, d_skip));     // w = Op p_j
            SPRS_TRY(launch_cgs2<T>(c, M, GM, cwM, d_state, Qb, qs, j, wM, qj, partN, dots.p));
        }
        SPRS_TRY(launch_small(c, sv_norm_kernel<T, false>, 0, d_state, (const R *)partN, GM, j, m, cycle));
        SPRS_TRY(launch_fused<T>(c, M, GM, cwM, GmScale<T, Hd>{d_head, qj, 0.0}));
        SPRS_TRY(launch_spmv<T>(OpH, SpmvPart::Whole, qj, wN, 0, nullptr, nullptr, nullptr, d_skip));        // w' = Op^H q_j
        SPRS_TRY(launch_cgs2<T>(c, N, GN, cwN, d_state, Pb, ps, j + 1, wN, pn, partN, dots.p));
        SPRS_TRY(launch_small(c, sv_norm_kernel<T, true>, 0, d_state, (const R *)partN, GN, j, m, cycle));
        return launch_fused<T>(c, N, GN, cwN, GmScale<T, Hd>{d_head, pn, 0.0});
    };
    auto rotate_p = [&](int me, int q, T *out, int64_t os) { return launch_lz_rotate<T, R>(c, (const R *)d_state->coefY, (const T *)Pb, ps, (int64_t)N, me, q, out, os); };
    auto rotate_q = [&](int me, int q, T *out, int64_t os) { return launch_lz_rotate<T, R>(c, (const R *)d_state->coefX, (const T *)Qb, qs, (int64_t)M, me, q, out, os); };

    // p_0 = v0 / |v0|
    SPRS_HIP_TRY(c, hipMemcpyAsync(Pb, v0, sizeof(T) * N, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    SPRS_TRY(launch_fused<T>(c, N, GN, cwN, LzNrm<T>{Pb, partN, 0.0}));
    SPRS_TRY(launch_small(c, lz_start_kernel<T, St>, 0, d_state, (const R *)partN, GN));
    SPRS_TRY(launch_fused<T>(c, N, GN, cwN, GmScale<T, Hd>{d_head, Pb, 0.0}));

    const int p = std::min((int)k + std::max((int)k, 4), m - 2);
    int j0 = 0;
    for (long long cycle = 1;; ++cycle) {
        for (int j = j0; j < m; ++j) SPRS_TRY(step(j, cycle));
        SPRS_TRY(launch_small(c, sv_svd_kernel<T>, 0, d_state, m, p));
        SPRS_TRY(state.fetch(sizeof(Hd)));
        if (H.status != ST_RUNNING || (size_t)cycle >= max_restarts) break;
        SPRS_TRY(rotate_p(m, p, Pb, ps));                                                           // P[:, :p] <- P[:, :m] Y[:, :p]
        SPRS_TRY(rotate_q(m, p, Qb, qs));                                                           // Q[:, :p] <- Q[:, :m] X[:, :p]
        SPRS_TRY(dcopy(c, pvec(p), (const T *)pvec(m), N));                                         // p_p <- p_m
        j0 = p;
    }

    const int rc = lz_results(state, k, state.host->sigma, vals_out, res_out, nconv_out, restarts_out, matvecs_out);
    if (rc != SPRS_OK && rc != SPRS_INSUFFICIENT_ITER) return rc;           // a breakdown: no vectors
    if (u && v) {     // P[:, :m_eff] Y[:, :k] and Q[:, :m_eff] X[:, :k]: V and U, or U and V where Op is A^H
        T *outN = swapped ? u : v, *outM = swapped ? v : u;
        if (host) {
            SPRS_TRY(rotate_p(H.m_eff, (int)k, Pb, ps));
            SPRS_TRY(rotate_q(H.m_eff, (int)k, Qb, qs));
            for (size_t i = 0; i < k; ++i) {
                SPRS_HIP_TRY(c, hipMemcpyAsync(outN + i * N, pvec((int)i), sizeof(T) * N, hipMemcpyDeviceToHost, c->stream));
                SPRS_HIP_TRY(c, hipMemcpyAsync(outM + i * M, qvec((int)i), sizeof(T) * M, hipMemcpyDeviceToHost, c->stream));
            }
        } else {
            SPRS_TRY(rotate_p(H.m_eff, (int)k, outN, (int64_t)N));
            SPRS_TRY(rotate_q(H.m_eff, (int)k, outM, (int64_t)M));
        }
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    SPRS_TRY(this->end_solve());
    return rc;
}

template class Svds<double>;
template class Svds<float>;
template class Svds<cplxf>;
template class Svds<cplx>;

}  // namespace sprs
