// KrylovBase<T>: what the solvers' hosts share that is no template of theirs (krylov.hpp has the rest).
#include "krylov.hpp"

#include <algorithm>

#include "fused_launch.hpp"

namespace sprs {

template <class T>
int KrylovBase<T>::init(const sprs_csr *A_, size_t size, int nvec_) {
    A = A_; ctx = A_->ctx; n = size; nvec = nvec_;
    // distributed: every work vector carries the halo tail (sparse halo) or is padded to the all-gather slice
    const size_t nx = !A->dist ? n : (A->dist->ag_slice > 0 ? std::max<size_t>(n, (size_t)A->dist->ag_slice) : (size_t)A->ncols);
    stride = (nx + 31) & ~(size_t)31;
    if (stride == 0) stride = 32;
    SPRS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    SPRS_HIP_TRY(ctx, hipMalloc((void **)&work, sizeof(T) * stride * (size_t)nvec));
    SPRS_HIP_TRY(ctx, hipMemsetAsync(work, 0, sizeof(T) * stride * (size_t)nvec, ctx->stream));   // vec![T::zero(); size*7]
    SPRS_HIP_TRY(ctx, hipMalloc((void **)&part, sizeof(T) * MAX_GRID * 8));
    SPRS_HIP_TRY(ctx, hipMalloc((void **)&partD, sizeof(Real<T>) * MAX_GRID * 4));
    SPRS_HIP_TRY(ctx, hipMemsetAsync(part, 0, sizeof(T) * MAX_GRID * 8, ctx->stream));
    SPRS_HIP_TRY(ctx, hipMemsetAsync(partD, 0, sizeof(Real<T>) * MAX_GRID * 4, ctx->stream));
    if (A->dist) {
        SPRS_HIP_TRY(ctx, hipMalloc((void **)&red, sizeof(double) * 32));
        SPRS_HIP_TRY(ctx, hipMemsetAsync(red, 0, sizeof(double) * 32, ctx->stream));
        SPRS_HIP_TRY(ctx, hipMalloc((void **)&fin_counter, sizeof(unsigned int) * 64));      // one arrival counter per hand-off slot, 64 B apart
        SPRS_HIP_TRY(ctx, hipMemsetAsync(fin_counter, 0, sizeof(unsigned int) * 64, ctx->stream));
        SPRS_HIP_TRY(ctx, hipMalloc((void **)&xext, sizeof(T) * stride));
    }
    SPRS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SPRS_OK;
}

template <class T>
void KrylovBase<T>::destroy() {
    if (work) (void)hipFree(work);
    if (rhs_buf) (void)hipFree(rhs_buf);
    if (x_buf) (void)hipFree(x_buf);
    if (part) (void)hipFree(part);
    if (partD) (void)hipFree(partD);
    if (red) (void)hipFree(red);
    if (fin_counter) (void)hipFree(fin_counter);
    if (xext) (void)hipFree(xext);
    red = nullptr; xext = nullptr; fin_counter = nullptr;
    for (auto e : ev) (void)hipEventDestroy(e);
    ev.clear();
    work = rhs_buf = x_buf = part = nullptr; partD = nullptr;
}

template <class T>
int KrylovBase<T>::ew_grid() const {
    constexpr int PKW = pack_width<T>::value;
    int64_t workb = ((int64_t)n / PKW + BLOCK - 1) / BLOCK;
    return balanced_grid(ctx, workb);
}

// Hand-offs of the distributed case.  The producing launch's last-arriving workgroup has already reduced the partials
// into `red` (struct Fin / finalize_last_block): all that is left per hand-off is ONE stream operation, the all-reduce — or
// NONE where the communicator has peer-to-peer mailboxes (knob "p2p_allreduce"): that workgroup also posts the
// values into every rank's mailbox and the consumer kernels of all ranks sum the `world` entries in rank order (device.hpp).
template <class T>
Fin KrylovBase<T>::fin_for(int slot, const void *base0, const void *base1, int P) const {
    if (!A->dist) return Fin{};
    Fin f;
    f.counter = fin_counter + 16 * slot;
    f.base0 = base0; f.base1 = base1;
    f.out0 = red + 2 * slot; f.out1 = red + 2 * slot + 2;
    f.P = P;
    if (use_p2p()) {
        // one more hand-off on this slot: its tag and the half of the slot it uses.  A fast rank can be at most one hand-off of
        // a slot ahead of a slow one (to post hand-off h + 2 it must have consumed h + 1, which the slow rank posts only after
        // all its workgroups consumed h), so two halves suffice.
        sprs_comm *cm = A->dist->comm;
        const unsigned int h = ++cm->seq[slot];
        f.box = cm->d_box; f.tag = h; f.mb_off = (unsigned int)mb_offset(slot, (int)(h & 1u));
    }
    return f;
}
template <class T>
const void *KrylovBase<T>::mbox_entries(int slot) const {
    const sprs_comm *cm = A->dist->comm;
    return reinterpret_cast<const char *>(cm->mbox) + mb_offset(slot, (int)(cm->seq[slot] & 1u));
}

template <class T>
int KrylovBase<T>::spmv(const T *x, T *y, int dot, const T *u, T *p0, T *p1, const int *status, bool conj_x, const Fin *fin) {
    if (A->dist) {
        // the SpMV input needs its halo tail filled: work vectors have room for it, a caller's
        // vector (initial residual, restart) is staged through `xext`
        T *xe = const_cast<T *>(x);
        const bool is_work = x >= work && x < work + stride * (size_t)nvec;
        if (!is_work) {
            SPRS_HIP_TRY(ctx, hipMemcpyAsync(xext, x, sizeof(T) * n, hipMemcpyDeviceToDevice, ctx->stream));
            xe = xext;
        }
        x = xe;
    }
    const T *x_caller = x;
    const int st = profiled([&]() -> int {
        if (A->dist) return dist_spmv<T>(A, const_cast<T *>(x), y, dot, u, p0, p1, status, conj_x, fin);
        return launch_spmv<T>(A, SpmvPart::Whole, x, y, dot, u, p0, p1, status, conj_x, fin);
    }, !A->dist);
    if (profile && dot != 0 && u != x_caller) mark_step(1);
    return st;
}

template <class T>
void KrylovBase<T>::profile_discard_last(size_t launches) {
    if (!profile) return;
    // the last `launches` STEPS were no-ops: the event pairs among them (all of them, or the sampled ones)
    const size_t first_noop = prof_calls > launches ? prof_calls - launches : 0;
    for (size_t k = ev_used / 2; k > 1 && ev_pair[k - 1].call >= first_noop; --k) ev_pair[k - 1].noop = true;     // pair 0 brackets the solve
}

template <class T>
int KrylovBase<T>::begin_solve() {
    SPRS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    trace_rows = 0;
    stats = SolverStats();
    if (profile) {
        if (ev.size() < 2) {
            for (int k = 0; k < 2; ++k) {
                hipEvent_t e;
                SPRS_HIP_TRY(ctx, hipEventCreate(&e));
                ev.push_back(e);
            }
        }
        ev_used = 2;  // ev[0], ev[1] bracket the whole solve
        prof_calls = 0;
        ev_pair.assign(1, EvPair{});
        last_pair = -1;
        SPRS_HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
    }
    return SPRS_OK;
}

template <class T>
int KrylovBase<T>::end_solve() {
    if (!profile) return SPRS_OK;
    SPRS_HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
    SPRS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    SPRS_HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    stats.solve_ms = ms;
    for (size_t k = 2; k + 1 < ev_used; k += 2) {
        const EvPair &p = ev_pair[k / 2];
        if (p.noop) continue;
        SPRS_HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        stats.spmv_ms += ms;
        stats.spmv_launches += 1;
        stats.timed_dot_other += (p.kind & 1) != 0;
        stats.timed_fused_k2 += (p.kind & 2) != 0;
        stats.timed_fused_k4 += (p.kind & 4) != 0;
    }
    stats.steps = (int64_t)prof_calls;
    return SPRS_OK;
}

template <class T>
void KrylovBase<T>::trace_row(double a0, double a1, T b, T c, T d) {
    if (!trace || trace_rows >= trace_cap) return;
    double *t = trace + 8 * trace_rows;
    t[0] = a0; t[1] = a1;
    t[2] = sre(b); t[3] = sim(b); t[4] = sre(c); t[5] = sim(c); t[6] = sre(d); t[7] = sim(d);
    ++trace_rows;
}

// ======================================================================= what the solvers' hosts share
template <class T>
int KrylovBase<T>::zero_rhs(const T *rhs, T *x, Real<T> *rhs_norm, Real<T> *res_out, bool *zero) {
    SPRS_TRY(norm2(rhs, rhs_norm));                                         // bicg_stab.rs:55, minres.rs:51
    *zero = *rhs_norm <= seps<Real<T>>();                                   // bicg_stab.rs:56-60, minres.rs:52-56
    if (*zero) {
        SPRS_TRY(dzero(ctx, x, n));
        *res_out = *rhs_norm;
    }
    return SPRS_OK;
}

template <class T>
int KrylovBase<T>::comm_timeout() {
    snprintf(ctx->err, sizeof(ctx->err), "a peer's hand-off did not reach this rank's mailbox within %d ms (p2p_timeout_ms)", ctx->p2p_timeout_ms);
    return SPRS_ERR_RCCL;
}

template class KrylovBase<double>;
template class KrylovBase<float>;
template class KrylovBase<cplxf>;
template class KrylovBase<cplx>;

}  // namespace sprs
