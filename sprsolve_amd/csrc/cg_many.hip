// Batched conjugate gradients (host side): CgMany<T>.  One solve carries k <= kmax right-hand sides through the three
// launches per iteration of cg_many_fuse.hpp; the host enqueues iterations blind and reads the state every `poll` of them.
// The results do not depend on `poll`: the device freezes a column at its event and stops all work once no column runs.
#include "krylov.hpp"

#include <algorithm>

#include "cg_many_fuse.hpp"

namespace sprs {

template <class T>
int CgMany<T>::create(const sprs_csr *A_, size_t size, size_t k) {
    A = A_; ctx = A_->ctx; n = size;
    if (k < 1 || k > (size_t)CGM_MAXK) return SPRS_INVALID_ARGUMENT;
    SPRS_TRY(size_is_rows(A, size));
    SPRS_TRY(single_gpu_only(A, "sprs_cgmany"));
    kmax = (int)k;
    kp = 1; lg = 0;
    while (kp < kmax) { kp <<= 1; ++lg; }
    n_pad = (n + 3) & ~(size_t)3;
    if (n_pad == 0) n_pad = 4;
    CtxLock lock(ctx);
    SPRS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t blk_elems = n_pad * (size_t)kp;
    SPRS_HIP_TRY(ctx, hipMalloc((void **)&work, sizeof(T) * blk_elems * 5));
    SPRS_HIP_TRY(ctx, hipMemsetAsync(work, 0, sizeof(T) * blk_elems * 5, ctx->stream));
    SPRS_HIP_TRY(ctx, hipMalloc((void **)&partPQ, sizeof(T) * MAX_GRID * CGM_MAXK));
    SPRS_HIP_TRY(ctx, hipMalloc((void **)&partRZ, sizeof(T) * MAX_GRID * CGM_MAXK));
    SPRS_HIP_TRY(ctx, hipMalloc((void **)&partN, sizeof(Real<T>) * MAX_GRID * CGM_MAXK));
    SPRS_HIP_TRY(ctx, hipMemsetAsync(partPQ, 0, sizeof(T) * MAX_GRID * CGM_MAXK, ctx->stream));
    SPRS_HIP_TRY(ctx, hipMemsetAsync(partRZ, 0, sizeof(T) * MAX_GRID * CGM_MAXK, ctx->stream));
    SPRS_HIP_TRY(ctx, hipMemsetAsync(partN, 0, sizeof(Real<T>) * MAX_GRID * CGM_MAXK, ctx->stream));
    SPRS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return state.create(ctx);
}

template <class T>
void CgMany<T>::destroy() {
    state.destroy();
    if (work) (void)hipFree(work);
    if (rhs_buf) (void)hipFree(rhs_buf);
    if (x_buf) (void)hipFree(x_buf);
    if (partPQ) (void)hipFree(partPQ);
    if (partRZ) (void)hipFree(partRZ);
    if (partN) (void)hipFree(partN);
    work = rhs_buf = x_buf = partPQ = partRZ = nullptr; partN = nullptr;
}

template <class T>
template <class V>
int CgMany<T>::run(const V *dinv, const T *rhs, T *x, int k, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out, int *status_out) {
    sprs_ctx *c = ctx;
    constexpr int PKW = pack_width<T>::value;
    const bool pc = dinv != nullptr;
    const int64_t rows = (int64_t)n, elems = (int64_t)n_pad << lg, np = elems / PKW;
    T *X = blk(0), *r = blk(1), *p = blk(2), *q = blk(3), *z = pc ? blk(4) : r;

    const int G = balanced_grid(c, (np + BLOCK - 1) / BLOCK);
    const int GS = spmm_grid(A);
    const int cw = fused_chunked(A) ? 1 : 0;
    const int gcopy = (int)std::min<int64_t>((elems + BLOCK - 1) / BLOCK, 2048);
    hipLaunchKernelGGL(cg_many_to_block<T>, dim3(gcopy), dim3(BLOCK), 0, c->stream, rows, (int64_t)n_pad, k, lg, rhs, r);
    hipLaunchKernelGGL(cg_many_to_block<T>, dim3(gcopy), dim3(BLOCK), 0, c->stream, rows, (int64_t)n_pad, k, lg, (const T *)x, X);
    SPRS_HIP_TRY(c, hipGetLastError());

    CgManyState<T> &H = *state.host;
    CgManyState<T> *const d_state = state.dev;
    memset(&H, 0, sizeof(H));
    for (int j = 0; j < CGM_MAXK; ++j) H.status[j] = CGM_UNUSED;
    SPRS_TRY(state.push());
    const int *d_running = &d_state->running;

    Real<T> *partRhs = reinterpret_cast<Real<T> *>(partPQ);     // S1 reads these while it writes partN: another array (idle until the first SpMM)
    // start: |rhs_c| ; r = rhs - A x ; z ; p ; rho_c ; which columns iterate
    SPRS_TRY(launch_fused<T>(c, (size_t)elems, G, cw, CgManyS0<T>{r, partRhs, kp, lg, rows, {}}));
    SPRS_TRY(launch_spmm<T>(A, X, q, kp, kp, 0, nullptr, nullptr, nullptr));
    SPRS_TRY(dispatch_bool(pc, [&](auto pc_tag) {
        return launch_fused<T>(c, (size_t)elems, G, cw, CgManyS1<T, V, decltype(pc_tag)::value>{d_state, partRhs, G, tol, q, X, r, p, dinv, z, partN, partRZ, kp, lg, rows, {}, {}});
    }));
    SPRS_TRY(launch_fused<T>(c, 0, 1, 0, CgManyS2<T>{d_state, partN, partRZ, G, kp}));

    auto CA = [&]() -> int { return launch_spmm<T>(A, p, q, kp, kp, 1, p, partPQ, d_running); };   // Q = A P ; conj(p_c).q_c
    auto KB = [&]() -> int {
        return dispatch_bool(pc, [&](auto pc_tag) {
            return launch_fused<T>(c, (size_t)elems, G, cw, CgManyKB<T, V, decltype(pc_tag)::value>{d_state, partPQ, GS, GS, p, q, X, r, dinv, z, partN, partRZ, kp, lg, rows, {}, {}, {}});
        });
    };
    auto KC = [&]() -> int {
        return dispatch_bool(pc, [&](auto pc_tag) {
            return launch_fused<T>(c, (size_t)elems, G, cw, CgManyKC<T, decltype(pc_tag)::value>{d_state, partN, partRZ, G, z, p, kp, lg, rows, {}, {}});
        });
    };

    const size_t poll = poll_interval(c);
    size_t its = 0, since_poll = 0;
    while (true) {
        const bool done_enqueue = its >= max_iter;
        if (!done_enqueue) {
            SPRS_TRY(CA()); SPRS_TRY(KB()); SPRS_TRY(KC());
            ++its; ++since_poll;
        }
        if (done_enqueue || since_poll >= poll) {
            since_poll = 0;
            SPRS_TRY(state.fetch());
            if (done_enqueue || H.running == 0) break;
        }
    }
    hipLaunchKernelGGL(cg_many_from_block<T>, dim3(gcopy), dim3(BLOCK), 0, c->stream, rows, k, lg, (const T *)X, x);
    SPRS_HIP_TRY(c, hipGetLastError());
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));

    int ret = SPRS_OK;
    for (int j = 0; j < k; ++j) {
        int st = SPRS_OK; size_t it = (size_t)H.its[j]; Real<T> res = 0.0;
        switch (H.status[j]) {
            case CGM_ZERO_RHS: it = 0; res = H.rhs_norm[j]; break;
            case ST_CONVERGED: res = H.r_norm[j] / H.rhs_norm[j]; break;
            case ST_BREAKDOWN: st = SPRS_BREAKDOWN; break;
            case ST_INVALID_PC: st = SPRS_INVALID_PRECOND; res = H.pc_re[j]; break;
            default: st = SPRS_INSUFFICIENT_ITER; it = max_iter; break;             // still running after max_iter iterations
        }
        if (its_out) its_out[j] = it;
        if (res_out) res_out[j] = res;
        if (status_out) status_out[j] = st;
        if (ret == SPRS_OK && st != SPRS_OK) ret = st;
    }
    return ret;
}

template <class T>
int CgMany<T>::solve_dev(const sprs_diag *P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t k, size_t max_iter, Real<T> tol,
                         size_t *its_out, Real<T> *res_out, int *status_out) {
    if (k < 1 || k > (size_t)kmax) return SPRS_INVALID_ARGUMENT;
    if (rhs_len != n * k) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (x_len != n * k) return SPRS_INCOMPATIBLE_X_SIZE;
    return with_prec<T>(P, *this, [&](const auto &M) -> int {
        SPRS_HIP_TRY(ctx, hipSetDevice(ctx->device));
        return run(M.dinv, rhs, x, (int)k, max_iter, tol, its_out, res_out, status_out);
    });
}

template class CgMany<double>;
template class CgMany<float>;
template class CgMany<cplxf>;
template class CgMany<cplx>;

}  // namespace sprs
