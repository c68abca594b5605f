// LOBPCG (Knyazev's locally optimal block preconditioned conjugate gradients) for the extreme eigenpairs of a Hermitian A: the
// recurrence of the header's sprs_lobpcg_* comment.  The host enqueues whole iterations blind — LobResid, LobCheck, b applications
// of an applied preconditioner, b SpMVs, LobGram, LobReduce, LobRR, LzRotate twice — and reads the head of the state once per `poll`
// iterations.  Kernels: lobpcg_fuse.hpp, eigsh_fuse.hpp (the rotation).
#include "krylov.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "lobpcg_fuse.hpp"

namespace sprs {

template <class T>
int Lobpcg<T>::create(const sprs_csr *A, size_t size, size_t block) {
    SPRS_TRY(single_gpu_only(A, "sprs_lobpcg"));
    if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
    if ((int64_t)size != A->nrows) return SPRS_DIM_MISMATCH;
    if (block == 0) block = std::min<size_t>(SPRS_LOBPCG_MAX_BLOCK, size / 6);
    if (block < 1 || block > SPRS_LOBPCG_MAX_BLOCK || 6 * block > size)
        return refuse(A->ctx, "sprs_lobpcg", "block = %zu is outside 1 .. min(%d, n / 6 = %zu)", block, SPRS_LOBPCG_MAX_BLOCK, size / 6);
    b = (int)block;
    SPRS_TRY(this->init(A, size, 6 * b));   // X, P, W, AX, AP, AW: b vectors each
    sprs_ctx *c = this->ctx;
    SPRS_TRY(state.create(c));
    const size_t m = 3 * (size_t)b;
    SPRS_HIP_TRY(c, hipMalloc((void **)&gpart, sizeof(T) * (size_t)LOB_MAX_WALK * m * (m + 1)));
    SPRS_HIP_TRY(c, hipMalloc((void **)&rpart, sizeof(Real<T>) * (size_t)LOB_MAXB * MAX_GRID));
    SPRS_HIP_TRY(c, hipMalloc((void **)&gsum, sizeof(cplx) * m * (m + 1)));
    SPRS_HIP_TRY(c, hipMemsetAsync(gsum, 0, sizeof(cplx) * m * (m + 1), c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(gpart, 0, sizeof(T) * (size_t)LOB_MAX_WALK * m * (m + 1), c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(rpart, 0, sizeof(Real<T>) * (size_t)LOB_MAXB * MAX_GRID, c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(state.dev, 0, sizeof(LobState<T>), c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
void Lobpcg<T>::destroy() {
    state.destroy();
    if (gpart) (void)hipFree(gpart);
    if (rpart) (void)hipFree(rpart);
    if (gsum) (void)hipFree(gsum);
    gpart = nullptr; rpart = nullptr; gsum = nullptr;
    KrylovBase<T>::destroy();
}

// LobGram on the m vectors of `layout` and their products, then LobReduce: the m (m + 1) sums in double in gsum
template <class T>
int Lobpcg<T>::gram(int layout, int m) {
    sprs_ctx *c = this->ctx;
    constexpr int PK = pack_width<T>::value, R = lob_r<T>::value, NBL = lob_nbw<T>::value, NBS = lob_nbw_small<T>::value;
    const int64_t n = (int64_t)this->n, ntile = (n + WAVE * PK - 1) / (WAVE * PK);
    const int MB = (m + R - 1) / R, nb1 = MB * (MB + 1) / 2;
    const int nsplit = (2 * nb1 + LOB_NW - 1) / LOB_NW <= NBL ? 1 : 2;
    const int need = ((nsplit == 1 ? 2 * nb1 : nb1) + LOB_NW - 1) / LOB_NW;
    const size_t lds = (size_t)2 * 2 * MB * R * WAVE * 16;      // two buffers of 2 m KiB (m rounded up to whole blocks)
    const int per_cu = need <= NBS ? 2 : 1;
    const int GW = (int)std::max<int64_t>(1, std::min<int64_t>({ntile, (int64_t)c->num_cu * per_cu / nsplit, (int64_t)LOB_MAX_WALK}));
    const bool nt = stream_loads_nt(c, this->n * sizeof(T));
    const int *d_status = &state.dev->hd.status;
    hipError_t attr = hipSuccess;
    auto launch = [&](auto kernel) {
        if (lds > ((size_t)64 << 10)) attr = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
        if (attr != hipSuccess) return;
        hipLaunchKernelGGL(kernel, dim3(GW * nsplit), dim3(LOB_THREADS), lds, c->stream, d_status, (const T *)this->vec(0), (int64_t)this->stride,
                           (int64_t)(3 * b) * (int64_t)this->stride, b, layout, m, n, nsplit, gpart);
    };
    if (need <= NBS) { if (nt) launch(lob_gram_kernel<T, true, NBS>); else launch(lob_gram_kernel<T, false, NBS>); }
    else { if (nt) launch(lob_gram_kernel<T, true, NBL>); else launch(lob_gram_kernel<T, false, NBL>); }
    SPRS_HIP_TRY(c, attr);
    SPRS_HIP_TRY(c, hipGetLastError());
    const int NE2 = m * (m + 1);
    hipLaunchKernelGGL(lob_reduce_kernel<T>, dim3((NE2 + NWAVE - 1) / NWAVE), dim3(BLOCK), 0, c->stream, d_status, (const T *)gpart, GW, NE2, (LobCD<T> *)gsum);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

template <class T>
template <class V>
int Lobpcg<T>::run(const Prec<T, V> &M, size_t k, int which, const T *X0, bool x0_host, size_t max_iter, Real<T> tol, Real<T> *vals_out,
                   T *vecs, bool vecs_host, Real<T> *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out) {
    using St = LobState<T>;
    using Hd = LobHead<T>;
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    const int64_t vs = (int64_t)this->stride;
    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;

    St *const d_state = state.dev;
    Hd &H = state.host->hd;
    memset(state.host, 0, sizeof(St));
    H.status = ST_RUNNING; H.k = (int)k; H.which = which; H.tol = (double)tol;
    for (int i = 0; i < LOB_MAXB; ++i) state.host->ident[i * LZ_MAXM + i] = sone<T>();
    SPRS_TRY(state.push());
    const int *d_status = &d_state->hd.status, *d_zero = &d_state->hd.zero;
    const T *d_coef = d_state->coef;

    T *X = this->vec(0), *P = this->vec(b), *W = this->vec(2 * b), *AX = this->vec(3 * b), *AW = this->vec(5 * b);
    // [S] <- [S] C and [AS] <- [AS] C in place: me rows, q columns of the coefficient block
    auto rotate2 = [&](int me, int q) -> int {
        SPRS_TRY((launch_lz_rotate<T, T>(c, d_coef, (const T *)X, vs, (int64_t)n, me, q, X, vs, d_status)));
        return launch_lz_rotate<T, T>(c, d_coef, (const T *)AX, vs, (int64_t)n, me, q, AX, vs, d_status);
    };

    // the start: X = X0, P = AP = 0, AX = A X, one Rayleigh-Ritz step on [X]
    SPRS_TRY(dzero(c, this->work, (size_t)6 * b * this->stride));
    for (int j = 0; j < b; ++j)
        SPRS_HIP_TRY(c, hipMemcpyAsync(X + (size_t)j * this->stride, X0 + (size_t)j * n, sizeof(T) * n, x0_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    for (int j = 0; j < b; ++j) SPRS_TRY(this->spmv(X + (size_t)j * this->stride, AX + (size_t)j * this->stride, 0, nullptr, nullptr, nullptr, d_status));
    SPRS_TRY(gram(1, b));
    SPRS_TRY(launch_small(c, lob_rr_kernel<T>, 0, d_state, (const LobCD<T> *)gsum, b, 1, b, 0LL));
    SPRS_TRY(rotate2(b, b));

    const size_t poll = sprs::poll_interval(c);
    for (size_t it = 1;; ++it) {
        SPRS_TRY(launch_fused<T>(c, n, G, cw, LobResid<T, V>{d_state, X, AX, W, vs, b, M.dinv, rpart, {}, {}}));
        SPRS_TRY(launch_small(c, lob_check_kernel<T>, 0, d_state, (const Real<T> *)rpart, G, b));
        if (it > max_iter) break;
        if (M.applied.h)
            for (int j = 0; j < b; ++j) SPRS_TRY(M.applied.apply(W + (size_t)j * this->stride, W + (size_t)j * this->stride));
        for (int j = 0; j < b; ++j) SPRS_TRY(this->spmv(W + (size_t)j * this->stride, AW + (size_t)j * this->stride, 0, nullptr, nullptr, nullptr, d_status));
        const int layout = it == 1 ? 2 : 3;
        SPRS_TRY(gram(layout, layout * b));
        SPRS_TRY(launch_small(c, lob_rr_kernel<T>, 0, d_state, (const LobCD<T> *)gsum, layout * b, layout, b, (long long)it));
        SPRS_TRY(rotate2(3 * b, 2 * b));
        if (it % poll == 0) {
            SPRS_TRY(state.fetch(sizeof(Hd)));
            if (H.status != ST_RUNNING) break;
        }
    }
    (void)P;

    SPRS_TRY(state.fetch(offsetof(St, coef)));
    *nconv_out = (size_t)H.nconv; *iters_out = (size_t)H.iters; *restarts_out = (size_t)H.restarts; *matvecs_out = (size_t)H.matvecs;
    for (size_t i = 0; i < k; ++i) { vals_out[i] = (Real<T>)state.host->theta[i]; res_out[i] = (Real<T>)state.host->res[i]; }
    if (H.status == ST_BREAKDOWN) return SPRS_BREAKDOWN;
    if (vecs) {     // the first k columns of X: LzRotate with the identity for its coefficients writes them at any alignment
        if (vecs_host) {
            for (size_t i = 0; i < k; ++i)
                SPRS_HIP_TRY(c, hipMemcpyAsync(vecs + i * n, X + i * this->stride, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
        } else {
            SPRS_TRY((launch_lz_rotate<T, T>(c, (const T *)d_state->ident, (const T *)X, vs, (int64_t)n, (int)k, (int)k, vecs, (int64_t)n, d_zero)));
        }
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return H.status == ST_CONVERGED ? SPRS_OK : SPRS_INSUFFICIENT_ITER;
}

template <class T>
int Lobpcg<T>::solve_dev(const Precond<T> &Pc, size_t k, int which, const T *X0, bool x0_host, size_t max_iter, Real<T> tol, Real<T> *vals_out,
                         T *vecs, bool vecs_host, Real<T> *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out) {
    return with_prec<T>(Pc, *this, [&](const auto &M) -> int {
        using V = std::remove_cv_t<std::remove_pointer_t<decltype(M.dinv)>>;
        SPRS_TRY(this->begin_solve());
        const int st = this->template run<V>(M, k, which, X0, x0_host, max_iter, tol, vals_out, vecs, vecs_host, res_out, nconv_out, iters_out,
                                             restarts_out, matvecs_out);
        if (st >= SPRS_ERR_HIP) return st;
        SPRS_TRY(this->end_solve());
        return st;
    });
}

template class Lobpcg<double>;
template class Lobpcg<float>;
template class Lobpcg<cplxf>;
template class Lobpcg<cplx>;

}  // namespace sprs
