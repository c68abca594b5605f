// Mixed-precision iterative refinement: the residual and the solution in H (f64 / c64), every correction from an inner Krylov
// solve in L (f32 / c32) on a demoted copy of the operator.  The recurrence (the header's sprs_refine_* comment):
//   |b| <= eps: x = 0, Ok, outer = 0
//   for k = 0, 1, ..:  r = b*1 + (A x)*(-1) ; res = |r| / |b| ; Ok(outer = k) if res <= tol ; BreakDown unless |r| is finite ;
//          InsufficientIterNum if k == max_outer ; s = |r| ; rl = fl_L(r (1 / s)) ; e = 0 ; inner solve A_L e = rl ;
//          x += fl_H(e) s
// Three launches and one SpMV in H per outer step (refine_fuse.hpp) around the inner solver, which is Cg<L> or Gmres<L> as it
// stands; the host reads the state once per outer step, between RfDemote and the inner solve.
#include "krylov.hpp"

#include "refine_fuse.hpp"

struct sprs_refine : sprs_solver_handle {};

namespace sprs {

// the C entry points that differ by L's suffix
static int low_csr_create(sprs_ctx *c, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci, const float *v, sprs_csr **out) {
    return sprs_csr_create_dev_s(c, n, n, nnz, rp, ci, v, 1, out);
}
static int low_csr_create(sprs_ctx *c, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci, const cplxf *v, sprs_csr **out) {
    return sprs_csr_create_dev_c(c, n, n, nnz, rp, ci, (const sprs_c32 *)v, 1, out);
}

template <class H>
class Refine {
   public:
    using L = Low<H>;
    sprs_ctx *ctx = nullptr;
    const sprs_csr *A = nullptr;
    size_t n = 0, stride = 0;
    int inner = SPRS_INNER_CG;
    L *val_lo = nullptr;            // A's values in L; A_lo adopts them with A's own row_ptr / col_idx
    sprs_csr *A_lo = nullptr;
    sprs_diag *P_lo = nullptr;      // the caller's Jacobi preconditioner in L (null: none)
    Cg<L> *cg = nullptr;
    Gmres<L> *gmres = nullptr;
    H *r = nullptr;                 // q = A x, then the residual
    H *rhs_buf = nullptr, *x_buf = nullptr;     // staging of host slices and of device vectors that are not 16-byte aligned
    L *rl = nullptr, *e = nullptr;
    Real<H> *partR = nullptr, *partB = nullptr;
    int *flag = nullptr;            // device: a finite value of A left L's range
    StateBlock<RfState<H>> state;

    int create(const sprs_csr *A_, size_t size, const sprs_diag *P, int inner_, size_t restart);
    void destroy();
    int solve_dev(const H *rhs, H *x, size_t max_outer, Real<H> tol, size_t inner_max_iter, Real<H> inner_tol, size_t *outer_out,
                  size_t *inner_its_out, Real<H> *res_out);

   private:
    int demote_precond(const sprs_diag *P);
    template <class V> int demote_dinv(const sprs_diag *P);
};

template <class H>
int Refine<H>::create(const sprs_csr *A_, size_t size, const sprs_diag *P, int inner_, size_t restart) {
    A = A_; ctx = A_->ctx; n = size; inner = inner_;
    sprs_ctx *c = ctx;
    stride = (n + 31) & ~(size_t)31;
    if (stride == 0) stride = 32;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    // the operator in L: one pass over the values, then a handle like any other (compressed streams included)
    const size_t nnz = (size_t)A->nnz;
    SPRS_HIP_TRY(c, hipMalloc((void **)&val_lo, sizeof(L) * (nnz ? nnz : 1)));
    SPRS_HIP_TRY(c, hipMalloc((void **)&flag, sizeof(int)));
    SPRS_HIP_TRY(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    if (nnz) SPRS_TRY((launch_rf<H>(c, nnz, aligned16(A->val), 0, RfCast<H>{(const H *)A->val, val_lo, flag})));
    int h_flag = 0;
    SPRS_HIP_TRY(c, hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_flag) {
        snprintf(c->err, sizeof(c->err), "sprs_refine_create: a finite value of the matrix is outside single precision's range");
        return SPRS_INVALID_ARGUMENT;
    }
    SPRS_TRY(low_csr_create(c, A->nrows, A->nnz, A->row_ptr, A->col_idx, val_lo, &A_lo));
    if (P) SPRS_TRY(demote_precond(P));
    if (inner == SPRS_INNER_CG) { cg = new Cg<L>(); SPRS_TRY(cg->create(A_lo, n)); }
    else { gmres = new Gmres<L>(); SPRS_TRY(gmres->create(A_lo, n, restart)); }
    SPRS_HIP_TRY(c, hipMalloc((void **)&r, sizeof(H) * stride));
    SPRS_HIP_TRY(c, hipMalloc((void **)&rl, sizeof(L) * stride));
    SPRS_HIP_TRY(c, hipMalloc((void **)&e, sizeof(L) * stride));
    SPRS_HIP_TRY(c, hipMalloc((void **)&partR, sizeof(Real<H>) * MAX_GRID));
    SPRS_HIP_TRY(c, hipMalloc((void **)&partB, sizeof(Real<H>) * MAX_GRID));
    SPRS_HIP_TRY(c, hipMemsetAsync(r, 0, sizeof(H) * stride, c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(rl, 0, sizeof(L) * stride, c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(e, 0, sizeof(L) * stride, c->stream));
    SPRS_TRY(state.create(c));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class H>
template <class V>
int Refine<H>::demote_dinv(const sprs_diag *P) {
    sprs_ctx *c = ctx;
    const size_t np = ((n + 31) & ~(size_t)31) + 32;      // diag_create's padding
    SPRS_HIP_TRY(c, hipMalloc(&P_lo->dinv, sizeof(Low<V>) * np));
    SPRS_HIP_TRY(c, hipMemsetAsync(P_lo->dinv, 0, sizeof(Low<V>) * np, c->stream));
    if (n) SPRS_TRY((launch_rf<V>(c, n, aligned16(P->dinv), 0, RfCast<V>{(const V *)P->dinv, (Low<V> *)P_lo->dinv, nullptr})));
    return SPRS_OK;
}

template <class H>
int Refine<H>::demote_precond(const sprs_diag *P) {
    if (P->n != n) return SPRS_DIM_MISMATCH;
    if (P->t_dtype != dtype_of<H>::value) return SPRS_INVALID_ARGUMENT;
    P_lo = new sprs_diag();
    P_lo->ctx = ctx; P_lo->n = n; P_lo->t_dtype = dtype_of<L>::value; P_lo->v_complex = P->v_complex;
    if (P->v_complex) {
        if constexpr (is_complex<H>::value) return demote_dinv<H>(P);
        else return SPRS_INVALID_ARGUMENT;
    }
    return demote_dinv<Real<H>>(P);
}

template <class H>
void Refine<H>::destroy() {
    if (cg) { cg->destroy(); delete cg; cg = nullptr; }
    if (gmres) { gmres->destroy(); delete gmres; gmres = nullptr; }
    if (P_lo) { (void)sprs_diag_precond_destroy(P_lo); P_lo = nullptr; }
    if (A_lo) { (void)sprs_csr_destroy(A_lo); A_lo = nullptr; }
    for (void *q : {(void *)val_lo, (void *)flag, (void *)r, (void *)rhs_buf, (void *)x_buf, (void *)rl, (void *)e, (void *)partR, (void *)partB})
        if (q) (void)hipFree(q);
    val_lo = nullptr; flag = nullptr; r = rhs_buf = x_buf = nullptr; rl = e = nullptr; partR = partB = nullptr;
    state.destroy();
}

template <class H>
int Refine<H>::solve_dev(const H *rhs, H *x, size_t max_outer, Real<H> tol, size_t inner_max_iter, Real<H> inner_tol,
                         size_t *outer_out, size_t *inner_its_out, Real<H> *res_out) {
    sprs_ctx *c = ctx;
    *outer_out = 0; *inner_its_out = 0; *res_out = 0.0;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));

    RfState<H> &S = *state.host;
    RfState<H> *const d_state = state.dev;
    memset(&S, 0, sizeof(S));
    S.tol = tol; S.status = ST_RUNNING;
    SPRS_TRY(state.push());

    const int G = rf_grid(c, n, pack_width<H>::value);          // RfResid's workgroups = the partials RfDemote re-reduces
    const int cw = fused_chunked(A_lo) ? 1 : 0;                  // the walk of the inner solver's vector kernels
    size_t inner_its = 0;
    for (size_t k = 0;; ++k) {
        const bool first = k == 0, last = k == max_outer;
        SPRS_TRY(launch_spmv<H>(A, SpmvPart::Whole, x, r, 0, nullptr, nullptr, nullptr, nullptr));      // q = A x
        SPRS_TRY(dispatch_bool(first, [&](auto f_tag) {
            constexpr bool F = decltype(f_tag)::value;
            SPRS_TRY(launch_fused<H>(c, n, G, cw, RfResid<H, F>{d_state, rhs, r, partR, partB, Fin{}, H(), H(), 0.0, 0.0}));
            return launch_rf<H>(c, n, true, cw, RfDemote<H, F>{d_state, partR, partB, G, (long long)k, last ? 1 : 0, r, rl, e, 0.0});
        }));
        SPRS_TRY(state.fetch());
        *inner_its_out = inner_its; *res_out = S.res;
        if (S.status == ST_CONVERGED) {
            if (S.zero_rhs) {
                SPRS_TRY(dzero(c, x, n));
                SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
                *res_out = S.b_norm;
                return SPRS_OK;
            }
            *outer_out = k;
            return SPRS_OK;
        }
        *outer_out = k;
        if (S.status == ST_BREAKDOWN) return SPRS_BREAKDOWN;
        if (last) return SPRS_INSUFFICIENT_ITER;
        // A_L e = rl, e = 0 on entry; |rl| = 1, so inner_tol means the same at every step
        size_t its = 0; Real<L> ires = 0;
        const int st = cg ? cg->solve_dev(P_lo, rl, n, e, n, inner_max_iter, (Real<L>)inner_tol, &its, &ires)
                          : gmres->solve_dev(P_lo, rl, n, e, n, inner_max_iter, (Real<L>)inner_tol, &its, &ires);
        inner_its += its; *inner_its_out = inner_its;
        if (st != SPRS_OK && st != SPRS_INSUFFICIENT_ITER) return st;       // x is what it was before this step
        SPRS_TRY(launch_rf<H>(c, n, true, cw, RfUpdate<H>{d_state, e, x, 0.0}));
    }
}

template <class H>
static int refine_create(const sprs_csr *A, size_t n, const sprs_diag *P, int inner, size_t restart, sprs_refine **out) {
    if (!A || !out) return SPRS_INVALID_ARGUMENT;
    *out = nullptr;
    if (A->dtype != dtype_of<H>::value) return SPRS_INVALID_ARGUMENT;
    if (inner != SPRS_INNER_CG && inner != SPRS_INNER_GMRES) return SPRS_INVALID_ARGUMENT;
    if (inner == SPRS_INNER_GMRES && restart > SPRS_GMRES_MAX_RESTART) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    c->err[0] = 0;                  // an SPRS_INVALID_ARGUMENT of this call that has a text is told from one that has none
    SPRS_TRY(single_gpu_only(A, "sprs_refine_create"));
    if ((int64_t)n != A->nrows || (int64_t)n != A->ncols) return SPRS_DIM_MISMATCH;
    auto *s = new Refine<H>();
    const int st = s->create(A, n, P, inner, restart);
    if (st != SPRS_OK) { s->destroy(); delete s; return st; }
    sprs_refine *h = new sprs_refine();
    h->dtype = dtype_of<H>::value; h->impl = s;
    *out = h;
    return SPRS_OK;
}

template <class H>
static Refine<H> *refine_of(sprs_refine *h) { return (h && h->dtype == dtype_of<H>::value) ? (Refine<H> *)h->impl : nullptr; }

// One solve.  Host slices, and device vectors that are not 16-byte aligned, go through the handle's aligned staging buffers.
template <class H>
static int refine_solve(sprs_refine *h, bool host, const H *rhs, size_t rl, H *x, size_t xl, size_t max_outer, double tol,
                        size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out) {
    Refine<H> *s = refine_of<H>(h);
    if (!s || !rhs || !x) return SPRS_INVALID_ARGUMENT;
    if (rl != s->n) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (xl != s->n) return SPRS_INCOMPATIBLE_X_SIZE;
    size_t o_dummy, i_dummy; double r_dummy;
    if (!outer_out) outer_out = &o_dummy;
    if (!inner_its_out) inner_its_out = &i_dummy;
    if (!res_out) res_out = &r_dummy;
    sprs_ctx *c = s->ctx;
    CtxLock lock(c);
    if (!host && aligned16(rhs) && aligned16(x))
        return s->solve_dev(rhs, x, max_outer, tol, inner_max_iter, inner_tol, outer_out, inner_its_out, res_out);
    const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (!s->rhs_buf) SPRS_HIP_TRY(c, hipMalloc((void **)&s->rhs_buf, sizeof(H) * s->stride));
    if (!s->x_buf) SPRS_HIP_TRY(c, hipMalloc((void **)&s->x_buf, sizeof(H) * s->stride));
    SPRS_HIP_TRY(c, hipMemcpyAsync(s->rhs_buf, rhs, sizeof(H) * rl, in, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(s->x_buf, x, sizeof(H) * xl, in, c->stream));
    const int st = s->solve_dev(s->rhs_buf, s->x_buf, max_outer, tol, inner_max_iter, inner_tol, outer_out, inner_its_out, res_out);
    if (st >= SPRS_ERR_HIP) return st;
    SPRS_HIP_TRY(c, hipMemcpyAsync(x, s->x_buf, sizeof(H) * xl, out, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return st;
}

template <class H>
static int demote_scaled(sprs_ctx *c, size_t n, const H *in, double scale, Low<H> *out) {
    if (!c || (n && (!in || !out))) return SPRS_INVALID_ARGUMENT;
    if (n == 0) return SPRS_OK;
    return launch_rf<H>(c, n, aligned16(in) && aligned16(out), 0, RfDemoteV<H>{in, scale, out});
}
template <class H>
static int axpy_promoted(sprs_ctx *c, size_t n, double alpha, const Low<H> *in, H *x) {
    if (!c || (n && (!in || !x))) return SPRS_INVALID_ARGUMENT;
    if (n == 0) return SPRS_OK;
    return launch_rf<H>(c, n, aligned16(in) && aligned16(x), 0, RfUpdateV<H>{in, alpha, x});
}

}  // namespace sprs

using namespace sprs;

#define SPRS_G(...) try { __VA_ARGS__ } catch (...) { return SPRS_ERR_HIP; }

extern "C" {

int sprs_refine_create_d(const sprs_csr *A, size_t n, const sprs_diag *P, int inner, size_t restart, sprs_refine **out) {
    SPRS_G(return refine_create<double>(A, n, P, inner, restart, out);)
}
int sprs_refine_create_z(const sprs_csr *A, size_t n, const sprs_diag *P, int inner, size_t restart, sprs_refine **out) {
    SPRS_G(return refine_create<cplx>(A, n, P, inner, restart, out);)
}
int sprs_refine_destroy(sprs_refine *R) {
    if (!R) return SPRS_OK;
    auto drop = [](auto *s) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); s->destroy(); delete s; };
    if (R->dtype == DT_D) drop((Refine<double> *)R->impl); else drop((Refine<cplx> *)R->impl);
    delete R;
    return SPRS_OK;
}
const sprs_csr *sprs_refine_low_csr(const sprs_refine *R) {
    if (!R) return nullptr;
    return R->dtype == DT_D ? ((const Refine<double> *)R->impl)->A_lo : ((const Refine<cplx> *)R->impl)->A_lo;
}
int sprs_refine_solve_d(sprs_refine *R, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_outer, double tol,
                        size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out) {
    SPRS_G(return refine_solve<double>(R, true, rhs, rhs_len, x, x_len, max_outer, tol, inner_max_iter, inner_tol, outer_out, inner_its_out, res_out);)
}
int sprs_refine_solve_z(sprs_refine *R, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_outer, double tol,
                        size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out) {
    SPRS_G(return refine_solve<cplx>(R, true, (const cplx *)rhs, rhs_len, (cplx *)x, x_len, max_outer, tol, inner_max_iter, inner_tol, outer_out, inner_its_out, res_out);)
}
int sprs_refine_solve_dev_d(sprs_refine *R, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_outer, double tol,
                            size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out) {
    SPRS_G(return refine_solve<double>(R, false, rhs, rhs_len, x, x_len, max_outer, tol, inner_max_iter, inner_tol, outer_out, inner_its_out, res_out);)
}
int sprs_refine_solve_dev_z(sprs_refine *R, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_outer, double tol,
                            size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out) {
    SPRS_G(return refine_solve<cplx>(R, false, (const cplx *)rhs, rhs_len, (cplx *)x, x_len, max_outer, tol, inner_max_iter, inner_tol, outer_out, inner_its_out, res_out);)
}

int sprs_demote_scaled_dev_d(sprs_ctx *c, size_t n, const double *in, double scale, float *out) { return demote_scaled<double>(c, n, in, scale, out); }
int sprs_demote_scaled_dev_z(sprs_ctx *c, size_t n, const sprs_c64 *in, double scale, sprs_c32 *out) { return demote_scaled<cplx>(c, n, (const cplx *)in, scale, (cplxf *)out); }
int sprs_axpy_promoted_dev_d(sprs_ctx *c, size_t n, double alpha, const float *in, double *x) { return axpy_promoted<double>(c, n, alpha, in, x); }
int sprs_axpy_promoted_dev_z(sprs_ctx *c, size_t n, double alpha, const sprs_c32 *in, sprs_c64 *x) { return axpy_promoted<cplx>(c, n, alpha, (const cplxf *)in, (cplx *)x); }

}  // extern "C"
