// w = exp(tA) v by Krylov projection with Expokit's error-controlled sub-stepping: the recurrence of the header's sprs_expm_*
// comment.  The host enqueues one sub-step blind — ExStart, GmScale, m Arnoldi steps (SpMV, launch_cgs2 against v_0 .. v_j,
// ExArnoldiStep, GmScale), the SpMV and LzNrm of avnorm, ExStep, ExCombine — and reads the head of the state once a
// sub-step.  Kernels: expm_fuse.hpp, gmres_fuse.hpp, eigsh_fuse.hpp (LzNrm).
#include "krylov.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "expm_fuse.hpp"

namespace sprs {

template <class T>
int Expm<T>::create(const sprs_csr *A, size_t size, size_t ncv) {
    SPRS_TRY(single_gpu_only(A, "sprs_expm"));
    if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
    if ((int64_t)size != A->nrows) return SPRS_DIM_MISMATCH;
    if (ncv == 0) ncv = std::min<size_t>(30, size);
    if (ncv < 3 || ncv > std::min<size_t>(SPRS_EXPM_MAX_NCV, size))
        return refuse(A->ctx, "sprs_expm", "ncv = %zu is outside 3 .. min(%d, n = %zu)", ncv, SPRS_EXPM_MAX_NCV, size);
    m = (int)ncv;
    SPRS_TRY(this->init(A, size, m + 3));   // v_0 .. v_m, p, the staging vector of the result
    sprs_ctx *c = this->ctx;
    SPRS_TRY(state.create(c));
    SPRS_HIP_TRY(c, hipMemsetAsync(state.dev, 0, sizeof(ExState<T>), c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
void Expm<T>::destroy() {
    state.destroy();
    dots.destroy();
    KrylovBase<T>::destroy();
}

template <class T>
int Expm<T>::apply(Real<T> t, const T *v, bool host, Real<T> tol, size_t max_steps, Real<T> tau0, T *w, Real<T> *err_out, Real<T> *hump_out,
                   Real<T> *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out) {
    using St = ExState<T>;
    using Hd = ExHead<T>;
    sprs_ctx *c = this->ctx;
    const size_t n = this->n;
    SPRS_TRY(this->begin_solve());
    *err_out = 0; *hump_out = 0; *t_done_out = 0; *steps_out = 0; *rejects_out = 0; *matvecs_out = 0;
    const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (t == Real<T>(0)) {                              // w = v bit for bit
        if (w != v) {
            if (host) memmove(w, v, sizeof(T) * n);
            else SPRS_HIP_TRY(c, hipMemcpyAsync(w, v, sizeof(T) * n, hipMemcpyDeviceToDevice, c->stream));
        }
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        return this->end_solve();
    }

    const int G = this->ew_grid();
    const int cw = fused_chunked(this->A) ? 1 : 0;
    SPRS_TRY(dots.ensure(c, EX_MAXM, G));

    Hd &H = state.host->hd;
    St *const d_state = state.dev;
    SPRS_HIP_TRY(c, hipMemsetAsync(d_state, 0, sizeof(St), c->stream));
    memset(state.host, 0, sizeof(Hd));
    H.status = ST_RUNNING; H.skip = 1;
    H.max_steps = (long long)std::min<size_t>(max_steps, (size_t)1 << 62);
    H.tau = (double)tau0; H.t_out = std::fabs((double)t); H.sgn = t < Real<T>(0) ? -1.0 : 1.0;
    H.tol = tol == Real<T>(0) ? (double)ssqrt(seps<Real<T>>()) : (double)tol;
    SPRS_TRY(state.push(sizeof(Hd)));
    const Hd *d_head = &d_state->hd;
    const int *d_skip = &d_state->hd.skip;

    T *Vb = basis(0), *p = pvec();
    T *last = (host || !aligned16(w)) ? stage() : w;    // where the sub-step that ends the solve writes
    const int64_t vs = (int64_t)this->stride;
    Real<T> *partN = this->dslot(0), *partB = this->dslot(1);      // |p|^2 of a step and |A v_m|^2 ; |w|^2
    const size_t lds = (size_t)3 * (size_t)(m + 2) * EX_LD * sizeof(ExH<T>);
    // more dynamic LDS than the default 64 KiB limit of a launch (complex types, ncv above 24): raise the kernel's limit first, to
    // what this launch needs (the kernel's few static words count against the 160 KiB too)
    if (lds > ((size_t)64 << 10))
        SPRS_HIP_TRY(c, hipFuncSetAttribute((const void *)ex_step_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto step = [&](int j) -> int {
        T *vj = Vb + (size_t)j * this->stride, *vn = Vb + (size_t)(j + 1) * this->stride;
        SPRS_TRY(this->spmv(vj, p, 0, nullptr, nullptr, nullptr, d_skip));                          // p = A v_j
        SPRS_TRY(launch_cgs2<T>(c, n, G, cw, d_state, Vb, vs, j + 1, p, vn, partN, dots.p));            // against v_0 .. v_j
        SPRS_TRY(launch_small(c, ex_arnoldi_step_kernel<T>, 0, d_state, (const Real<T> *)partN, G, j));
        return launch_fused<T>(c, n, G, cw, GmScale<T, Hd>{d_head, vn, 0.0});
    };

    // w = v in the slot of v_0, and the partials of its norm
    SPRS_HIP_TRY(c, hipMemcpyAsync(Vb, v, sizeof(T) * n, in, c->stream));
    SPRS_TRY(launch_fused<T>(c, n, G, cw, LzNrm<T>{Vb, partB, 0.0}));
    for (size_t s = 0; s < max_steps; ++s) {
        SPRS_TRY(launch_small(c, ex_start_kernel<T>, 0, d_state, (const Real<T> *)partB, G, m));
        SPRS_TRY(launch_fused<T>(c, n, G, cw, GmScale<T, Hd>{d_head, Vb, 0.0}));
        for (int j = 0; j < m; ++j) SPRS_TRY(step(j));
        SPRS_TRY(this->spmv(basis(m), p, 0, nullptr, nullptr, nullptr, d_skip));                    // avnorm = |A v_m|
        SPRS_TRY(launch_fused<T>(c, n, G, cw, LzNrm<T>{p, partN, 0.0}));
        SPRS_TRY(launch_small(c, ex_step_kernel<T>, lds, d_state, (const Real<T> *)partN, G, m));
        SPRS_TRY(launch_fused<T>(c, n, G, cw, ExCombine<T>{d_state, Vb, vs, Vb, last, partB, nullptr, nullptr, 0, 0.0}));
        SPRS_TRY(state.fetch(sizeof(Hd)));
        if (H.status != ST_RUNNING) break;
    }

    *err_out = (Real<T>)H.err_sum; *hump_out = (Real<T>)H.hump; *t_done_out = (Real<T>)(H.sgn * H.t_now);
    *steps_out = (size_t)H.steps; *rejects_out = (size_t)H.rejects; *matvecs_out = (size_t)H.matvecs;
    if (H.status != ST_CONVERGED && H.status != ST_MAX_ITER) return SPRS_BREAKDOWN;                 // w is not written
    if (H.zero) SPRS_TRY(dzero(c, last, n));
    if (last != w) SPRS_HIP_TRY(c, hipMemcpyAsync(w, last, sizeof(T) * n, out, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    SPRS_TRY(this->end_solve());
    return H.status == ST_CONVERGED ? SPRS_OK : SPRS_INSUFFICIENT_ITER;
}

template class Expm<double>;
template class Expm<float>;
template class Expm<cplxf>;
template class Expm<cplx>;

}  // namespace sprs
