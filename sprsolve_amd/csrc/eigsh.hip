// Thick-restart Lanczos (Wu & Simon; = Hermitian Krylov-Schur) with full reorthogonalisation by CGS2: the recurrence of the
// header's sprs_eigsh_* comment.  The host enqueues whole cycles blind — per step SpMV, 2 x (ceil((j + 1) / gm_b<T>) GmDots +
// GmUpdate), LzStep, GmScale; per cycle LzRitz — and reads the head of the state once a cycle, to choose between the restart
// (LzRotate in place + one copy) and the end (LzRotate into the caller's vectors).  Kernels: eigsh_fuse.hpp, gmres_fuse.hpp.
#include "krylov.hpp"

#include <algorithm>
#include <cstddef>

#include "eigsh_fuse.hpp"

namespace sprs {

template <class T>
int Eigsh<T>::create(const sprs_csr *A, size_t size, size_t ncv) {
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
    if (dots) (void)hipFree(dots);
    dots = nullptr; dots_grid = 0;
    KrylovBase<T>::destroy();
}

// out[:, c] = sum_i V[:, i] S[i, c], c < q, i < me: one LzRotate launch; LDS a workgroup: me KiB of tile + the coefficient block
template <class T>
int Eigsh<T>::rotate(int me, int q, T *out, int64_t ostride) {
    sprs_ctx *c = this->ctx;
    constexpr int PK = pack_width<T>::value;
    const int64_t n = (int64_t)this->n, ntile = (n + WAVE * PK - 1) / (WAVE * PK);
    const int cb = q <= 8 ? 2 : 4, qp = (q + cb - 1) / cb * cb;
    const size_t lds = (size_t)me * WAVE * 16 + (size_t)me * qp * sizeof(Real<T>);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, ((size_t)160 << 10) / lds));    // workgroups a CU's 160 KiB of LDS holds
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ntile, (int64_t)c->num_cu * per_cu));
    const int packed = (aligned16(out) && (ostride * (int64_t)sizeof(T)) % 16 == 0) ? 1 : 0;
    const Real<T> *cf = state.dev->coef;
    const bool nt = stream_loads_nt(c, this->n * sizeof(T));
    hipError_t attr = hipSuccess;
    auto launch = [&](auto kernel) {
        // more dynamic LDS than the default 64 KiB limit of a launch (ncv near 64): raise the kernel's limit first
        if (lds > ((size_t)64 << 10)) attr = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
        if (attr != hipSuccess) return;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, c->stream, cf, (const T *)basis(0), (int64_t)this->stride, n, me, q, out, ostride, packed);
    };
    if (cb == 2) { if (nt) launch(lz_rotate_kernel<T, true, 2>); else launch(lz_rotate_kernel<T, false, 2>); }
    else { if (nt) launch(lz_rotate_kernel<T, true, 4>); else launch(lz_rotate_kernel<T, false, 4>); }
    SPRS_HIP_TRY(c, attr);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
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
    if (dots_grid < G) {                                // (the "grid" knob may have grown since the last solve)
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (dots) SPRS_HIP_TRY(c, hipFree(dots));
        dots = nullptr; dots_grid = 0;
        SPRS_HIP_TRY(c, hipMalloc((void **)&dots, sizeof(T) * (size_t)LZ_MAXM * (size_t)G));
        SPRS_HIP_TRY(c, hipMemsetAsync(dots, 0, sizeof(T) * (size_t)LZ_MAXM * (size_t)G, c->stream));
        dots_grid = G;
    }

    Hd &H = state.host->hd;
    St *const d_state = state.dev;
    SPRS_HIP_TRY(c, hipMemsetAsync(d_state, 0, sizeof(St), c->stream));     // T = 0, anorm = 0, scale = 0, the counters
    memset(state.host, 0, offsetof(St, h));
    H.status = ST_RUNNING; H.skip = 1; H.k = (int)k; H.which = which; H.tol = (double)tol;
    SPRS_TRY(state.push(sizeof(Hd)));
    const Hd *d_head = &d_state->hd;
    const int *d_skip = &d_state->hd.skip;

    T *Vb = basis(0), *w = wvec();
    const int64_t vs = (int64_t)this->stride;
    Real<T> *partN = this->dslot(0);
    auto small = [&](auto kernel, auto... args) -> int {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(BLOCK), 0, c->stream, args...);
        SPRS_HIP_TRY(c, hipGetLastError());
        return SPRS_OK;
    };
    auto multi_dot = [&](int j) -> int {
        constexpr int B = gm_b<T>::value;
        for (int i0 = 0; i0 <= j; i0 += B)
            SPRS_TRY(launch_fused<T>(c, n, G, cw, GmDots<T, B, Hd>{d_head, Vb, vs, i0, std::min(B, j + 1 - i0), w, dots, G, {}}));
        return SPRS_OK;
    };
    auto step = [&](int j, long long cycle) -> int {
        T *vj = Vb + (size_t)j * this->stride, *vn = Vb + (size_t)(j + 1) * this->stride;
        SPRS_TRY(this->spmv(vj, w, 0, nullptr, nullptr, nullptr, d_skip));                          // w = A v_j
        SPRS_TRY(multi_dot(j));
        SPRS_TRY(launch_fused<T>(c, n, G, cw, GmUpdate<T, false, St>{d_state, dots, G, G, j, Vb, vs, w, w, nullptr, Fin{}, nullptr, 0.0}));
        SPRS_TRY(multi_dot(j));
        SPRS_TRY(launch_fused<T>(c, n, G, cw, GmUpdate<T, true, St>{d_state, dots, G, G, j, Vb, vs, w, vn, partN, Fin{}, nullptr, 0.0}));
        SPRS_TRY(small(lz_step_kernel<T>, d_state, (const Real<T> *)partN, G, j, m, cycle));
        return launch_fused<T>(c, n, G, cw, GmScale<T, Hd>{d_head, vn, 0.0});
    };

    // v_0 = v0 / |v0|
    SPRS_HIP_TRY(c, hipMemcpyAsync(Vb, v0, sizeof(T) * n, v0_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    SPRS_TRY(launch_fused<T>(c, n, G, cw, LzNrm<T>{Vb, partN, 0.0}));
    SPRS_TRY(small(lz_start_kernel<T>, d_state, (const Real<T> *)partN, G));
    SPRS_TRY(launch_fused<T>(c, n, G, cw, GmScale<T, Hd>{d_head, Vb, 0.0}));

    const int p = std::min((int)k + std::max((int)k, 4), m - 2);
    int j0 = 0;
    for (long long cycle = 1;; ++cycle) {
        for (int j = j0; j < m; ++j) SPRS_TRY(step(j, cycle));
        SPRS_TRY(small(lz_ritz_kernel<T>, d_state, m, p));
        SPRS_TRY(state.fetch(sizeof(Hd)));
        if (H.status != ST_RUNNING || (size_t)cycle >= max_restarts) break;
        SPRS_TRY(rotate(m, p, Vb, vs));                                                             // V[:, :p] <- V[:, :m] S[:, :p]
        SPRS_TRY(dcopy(c, basis(p), (const T *)basis(m), n));                                       // v_p <- v_m
        j0 = p;
    }

    SPRS_TRY(state.fetch(offsetof(St, h)));
    *nconv_out = (size_t)H.nconv; *restarts_out = (size_t)H.cycle; *matvecs_out = (size_t)H.matvecs;
    for (size_t i = 0; i < k; ++i) { vals_out[i] = (Real<T>)state.host->theta[i]; res_out[i] = (Real<T>)state.host->res[i]; }
    if (H.status == ST_BREAKDOWN) return SPRS_BREAKDOWN;
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
    return H.status == ST_CONVERGED ? SPRS_OK : SPRS_INSUFFICIENT_ITER;
}

template class Eigsh<double>;
template class Eigsh<float>;
template class Eigsh<cplxf>;
template class Eigsh<cplx>;

}  // namespace sprs
