// Krylov recurrences (host side, C++) over device-resident vectors and scalars: the solver objects behind sprs_bicgstab,
// sprs_minres / sprs_csminres, sprs_cg, sprs_gmres, sprs_cg_many, sprs_cg_shift, sprs_idrs, sprs_lsmr, sprs_eigsh, sprs_lobpcg, sprs_svds and sprs_expm.  One translation unit per solver (bicgstab.hip,
// minres.hip, cg.hip, gmres.hip, cg_many.hip, cg_shift.hip, idrs.hip, lsmr.hip, eigsh.hip, lobpcg.hip, svds.hip, expm.hip), each with its recurrence comment; its kernels are the functors of its *_fuse.hpp, all run by
// fused_kernel (fused_launch.hpp).  BiCGStab and MINRES / CSMINRES follow the reference (src/bicg_stab.rs, src/minres.rs,
// src/cs_minres.rs); CG, GMRES, the batched and the multi-shift CG, LSMR, the two eigensolvers, the truncated SVD and the exponential propagator have no reference analogue: include/sprsolve_hip.h
// states their recurrences.
//
// Two execution modes per solver (sprs_solver_set_mode; the batched CG is fused only):
//  * fused (default): the full-vector passes of an iteration are regrouped into a few kernels (BiCGStab 13 passes -> 5 kernels,
//    MINRES 11 -> 3, CG and GMRES: cg_fuse.hpp, gmres_fuse.hpp).  Every scalar of the recurrence lives in HBM: a kernel that
//    needs the result of a dot product re-reduces that product's per-workgroup partials in its prologue (same partials, same
//    order in every workgroup => bit-identical scalars everywhere) and workgroup 0 records the scalar for later kernels.  The
//    host never waits for a scalar; it polls a status word every `poll` iterations.  After convergence / breakdown / restart
//    request every later kernel returns at its first instruction, so x, r and the iteration number are exactly those at the
//    moment of the event.  The arithmetic of every element keeps the reference's rounding sequence (e.g.
//    y = (v*(-beta*w) + y*beta) + r*1, bicg_stab.rs:155-156); only the summation order of the dot products / norms differs.
//  * literal: one kernel per reference op, scalars consumed on the host where the reference consumes them.  Slow (5 host syncs
//    per iteration); kept as the on-GPU cross-check.
//
// What the hosts share is written once: KrylovBase (below; krylov_base.hip) with solve(), handoff() (a producer's partials to
// their consumer: single GPU / mailbox / all-reduce), zero_rhs(), poll_interval(), comm_timeout(); StateBlock (the device +
// pinned-host pair of the scalar state); DotsBuf (the partials of launch_cgs2 of gmres_fuse.hpp, the one Gram-Schmidt sequence
// of GMRES, Eigsh, Svds and Expm); launch_small (fused_launch.hpp: the one-workgroup scalar kernels); with_prec() (the
// preconditioner's checks, its element type and the Prec<T, V> a run receives: none, Jacobi, or an applied ILU(0) / AMG
// handle).  Eigsh and Svds also share the frame of a thick-restart solve (lz_begin / lz_results of eigsh_fuse.hpp) around their
// own cycle loops.  The main loops stay apart: BiCGStab's restart, MINRES's deferred
// M3, CG's accounting of idle launches and GMRES's cycles have nothing in common.  Each solver has ONE run and ONE run_literal,
// whatever it is preconditioned with.
//
// Handles: every S<T> here has create(...) and destroy().  create holds ALL checks of the operator and of the creation parameters,
// in the order that decides the status when two are wrong: single_gpu_only(), square, size against the rows (size_is_rows() for
// the linear solvers), the parameter's range and default, the adjoint handle; a refusal with a reason goes through refuse()
// (internal.hpp).  destroy is safe on an object whose create returned early.  capi.hip adds only what belongs to the ABI, once, in
// solver_create: null pointers, *out, the handle's scalar type, the context lock, the allocation and the unwind.  A new solver
// writes there its entry points' signatures and one solver_create call.
#pragma once
#include "internal.hpp"

namespace sprs {

// Device-resident scalar state of a BiCGStab solve (bicg_stab.rs:84-88,127-186 locals).
template <class T>
struct BicgState {
    T rho, rho_old, alpha, w, beta;
    Real<T> r_norm, r0_norm_tol, tol2, pad0;
    long long its;
    int status, pad1;
};

// Device-resident scalar state of a MINRES / CSMINRES solve (minres.rs:60-64,81-83 locals).
// Two copies, indexed by iteration parity: kernels of iteration k read st[k&1], workgroup 0 of
// the last kernel writes st[(k+1)&1] — no workgroup ever reads a word another one is writing.
template <class T>
struct MinresState {
    T c, c_old, eta, alpha;
    Real<T> s, s_old, beta, beta_one, res_norm, threshold, pc_re, pad0;
};
template <class T>
struct MinresDev {
    MinresState<T> st[2];
    long long its;   // 0-based iteration index of the event recorded in `status`
    int status, pad;
};

template <class T> struct CgState;   // cg_fuse.hpp
template <class T> struct GmresState;   // gmres_fuse.hpp
template <class R> struct LsDev;       // lsmr_fuse.hpp
template <class R> struct LsIter;

struct SolverStats {
    double spmv_ms = 0.0, solve_ms = 0.0;
    int64_t spmv_launches = 0;
    int64_t fused_k2 = 0, fused_k4 = 0;   // of those (enqueued, profiled or not): chain launches that formed their input on the fly (K1 into K2 / K3 into K4)
    int64_t chain_k5 = 0;                 // BiCGStab: launches of K5 on the chains (knob "bicg_k5"; not SpMV launches: neither timed nor counted above)
    // among the TIMED launches (spmv_launches): how many read a dot operand that is not their input vector, how many were fused K2 / K4
    int64_t timed_dot_other = 0, timed_fused_k2 = 0, timed_fused_k4 = 0;
    int64_t steps = 0;                    // SpMV-class steps of the solve, timed or not
};

// A solver's scalar state: the kernels' copy in HBM and the host's view of it in pinned memory.
template <class S>
struct StateBlock {
    sprs_ctx *ctx = nullptr;
    S *dev = nullptr, *host = nullptr;
    int create(sprs_ctx *c) {
        ctx = c;
        SPRS_HIP_TRY(ctx, hipMalloc((void **)&dev, sizeof(S)));
        SPRS_HIP_TRY(ctx, hipHostMalloc((void **)&host, sizeof(S), hipHostMallocDefault));
        return SPRS_OK;
    }
    void destroy() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr;
    }
    // `bytes`: only the leading part of S travels (GMRES polls the head of a state that also holds the packed R)
    int push(size_t bytes = sizeof(S)) {    // host -> device, in stream order
        SPRS_HIP_TRY(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        return SPRS_OK;
    }
    int fetch(size_t bytes = sizeof(S)) {   // device -> host, and wait for it
        SPRS_HIP_TRY(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        SPRS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return SPRS_OK;
    }
};

// The [maxm][grid] partials of launch_cgs2's multi-dots (gmres_fuse.hpp), held by GMRES, Eigsh, Svds and Expm.
template <class T>
struct DotsBuf {
    T *p = nullptr;
    int grid = 0;
    // before a solve enqueues: room for maxm x G partials (the "grid" knob may have grown since the last solve)
    int ensure(sprs_ctx *c, int maxm, int G) {
        if (grid >= G) return SPRS_OK;
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (p) SPRS_HIP_TRY(c, hipFree(p));
        p = nullptr; grid = 0;
        SPRS_HIP_TRY(c, hipMalloc((void **)&p, sizeof(T) * (size_t)maxm * (size_t)G));
        SPRS_HIP_TRY(c, hipMemsetAsync(p, 0, sizeof(T) * (size_t)maxm * (size_t)G, c->stream));
        grid = G;
        return SPRS_OK;
    }
    void destroy() {
        if (p) (void)hipFree(p);
        p = nullptr; grid = 0;
    }
};

// The preconditioner as a run receives it (with_prec() below has checked it).  dinv: M^-1's diagonal, of V = T (a complex
// diagonal) or Real<T>; it is read inside the solvers' own fused kernels.  applied (applied.h != null): z = M r is a chain of
// launches of the handle's own; V is Real<T> then.  Both null: no preconditioner.
template <class T, class V>
struct Prec {
    sprs_ctx *ctx = nullptr;
    size_t n = 0;
    const V *dinv = nullptr;
    AppliedPrec<T> applied;
    bool any() const { return dinv || applied.h; }
    // out = M in as launches of its own: CG's start, the literal modes, and every application of an applied one
    int apply(const T *in, T *out) const { return applied.h ? applied.apply(in, out) : launch_diag_apply<T, V>(ctx, n, dinv, in, out); }
    operator const V *() const { return dinv; }   // the batched CG takes no applied one and keeps its `const V *dinv` run
};

// The partials of one reduction as their consumer kernel finds them (KrylovBase::handoff).
template <class U>
struct Part { const U *p; int P; unsigned int tag = 0; };   // tag != 0: p = this rank's mailbox entries of the hand-off, P = world

// One profiled SpMV-class step (a pair of events).  Pair 0 brackets the whole solve.
struct EvPair {
    size_t call = 0;            // the step it brackets
    unsigned char kind = 0;     // 1 = dot operand is not the input vector, 2 = fused K2, 4 = fused K4
    bool noop = false;          // launched after a restart request, i.e. returned at once — not a measurement
};

// iterations between two reads of the status word (knob "poll")
inline size_t poll_interval(const sprs_ctx *c) { return (size_t)(c->poll < 1 ? 1 : c->poll); }

template <class T>
class KrylovBase {
   public:
    sprs_ctx *ctx = nullptr;
    const sprs_csr *A = nullptr;
    size_t n = 0, stride = 0;
    int nvec = 0;
    T *work = nullptr;           // nvec * stride
    T *rhs_buf = nullptr, *x_buf = nullptr;
    T *part = nullptr;           // NSLOT * MAX_GRID partials of T
    Real<T> *partD = nullptr;    // NSLOT * MAX_GRID real partials
    int mode = 0;
    double *trace = nullptr;
    size_t trace_cap = 0, trace_rows = 0;
    int profile = 0;             // 0 off; 1: every SpMV launch between HIP events; k >= 2: one pair of consecutive launches in k (a sample:
                                 // the events cost ~6 us per launch, profiled() below)
    size_t prof_calls = 0;       // SpMV-class steps of this solve so far (sampled or not)
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    std::vector<EvPair> ev_pair; // one per pair of events in use: ev_pair[k] describes ev[2k], ev[2k + 1]
    long last_pair = -1;         // the event pair of the last step (-1: it carried none)
    void mark_step(unsigned char kind) { if (last_pair >= 0) ev_pair[(size_t)last_pair].kind |= kind; }
    SolverStats stats;
    // distributed operator (A->dist): all-reduced scalars live in `red`, 16-byte slots
    double *red = nullptr;       // device, 32 doubles
    unsigned int *fin_counter = nullptr;   // device: arrival counters of the in-launch finalizes (struct Fin), one per slot
    T *xext = nullptr;           // extended copy of a caller vector that has no halo tail

    int init(const sprs_csr *A_, size_t size, int nvec_);
    void destroy();
    __attribute__((noinline)) ~KrylovBase() = default;   // (the two vectors) one copy, not one per kind in solver_create's unwind and solver_destroy
    T *vec(int i) { return work + (size_t)i * stride; }
    T *pslot(int s) { return part + (size_t)s * MAX_GRID; }
    Real<T> *dslot(int s) { return partD + (size_t)s * MAX_GRID; }
    int spmv(const T *x, T *y, int dot, const T *u, T *p0, T *p1, const int *status, bool conj_x = false, const sprs::Fin *fin = nullptr);
    // distributed: descriptor that makes the producing launch reduce its partials into red[2*slot ..] (empty otherwise)
    sprs::Fin fin_for(int slot, const void *base0, const void *base1, int P) const;
    template <class F> int profiled(F &&run, bool one_kernel);   // run() = one SpMV-class step, bracketed by the profile's events when a profile is taken
    void profile_discard_last(size_t launches);   // the last `launches` profiled SpMVs were no-ops (status word set): keep them out of the mean
    int begin_solve();
    int end_solve();
    void trace_row(double a0, double a1, T b, T c, T d);
    // What the solvers' solve_dev share: argument defaults, size checks, the preconditioner's checks and element type, the
    // literal-or-fused choice.  S supplies run<V> / run_literal<V>, which receive a Prec<T, V>; no_precond: S takes no
    // preconditioner (CSMINRES).
    template <class S>
    static int solve(S &s, bool no_precond, const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter,
                     Real<T> tol, size_t *its_out, Real<T> *res_out);
    // |rhs|; a zero right-hand side answers x = 0 (*zero = true: the solve is over, *res_out holds the norm)
    int zero_rhs(const T *rhs, T *x, Real<T> *rhs_norm, Real<T> *res_out, bool *zero);
    size_t poll_interval() const { return trace ? 1 : sprs::poll_interval(ctx); }   // a trace reads the state every iteration
    int comm_timeout();          // ST_COMM_TIMEOUT as the caller sees it: the error text and SPRS_ERR_RCCL
    int ew_grid() const;  // workgroups used by the fused element-wise kernels for this n
    sprs_comm *comm() const { return A->dist ? A->dist->comm : nullptr; }
    // Hand a producer's partials to its consumer kernel.  Single GPU: the consumer re-reduces the
    // P partials itself.  Distributed: the producer's last workgroup has reduced them into `red`
    // (fixed order; fin_for), these all-reduce over the ranks, and the consumer reads one value.
    // `slot` picks a 16-byte cell of `red`; a second value (b) travels in the cell after it.
    bool no_p2p = false;         // this solver's hand-offs always take the all-reduce (CG: it has no mailbox consumers)
    bool use_p2p() const { return !no_p2p && A->dist && A->dist->comm->p2p && ctx->p2p_allreduce != 0; }
    unsigned long long mb_timeout() const { return (unsigned long long)(ctx->p2p_timeout_ms < 1 ? 1 : ctx->p2p_timeout_ms) * 100000ull; }   // ticks of the 100 MHz wall clock
    const void *mbox_entries(int slot) const;    // this rank's mailbox at the CURRENT hand-off of `slot`
    template <class U, class W = U>
    int handoff(int slot, int P, const U *a, Part<U> *oa, const W *b = nullptr, Part<W> *ob = nullptr);
    int norm2(const T *x, Real<T> *out) { return norm2_host<T>(ctx, n, x, out, comm()); }
    int cdot(const T *x, const T *y, T *out) { return dot_host<T>(ctx, n, x, y, true, out, comm()); }
};

template <class T>
class BicgStab : public KrylovBase<T> {
   public:
    StateBlock<BicgState<T>> state;
    int create(const sprs_csr *A, size_t size);
    void destroy() { state.destroy(); KrylovBase<T>::destroy(); }
    // P: nothing, a diagonal (a `const sprs_diag *` converts) or an applied ILU(0) / AMG handle
    int solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                  size_t *its_out, Real<T> *res_out);

   private:
    friend class KrylovBase<T>;
    template <class V>
    int run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
    template <class V>
    int run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
};

template <class T>
class MinRes : public KrylovBase<T> {
   public:
    StateBlock<MinresDev<T>> state;
    bool saunders = false;  // CSMINRES
    int create(const sprs_csr *A, size_t size, bool saunders_);
    void destroy() { state.destroy(); KrylovBase<T>::destroy(); }
    // P: nothing, a diagonal (a `const sprs_diag *` converts) or an applied ILU(0) / AMG handle
    int solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                  size_t *its_out, Real<T> *res_out);

   private:
    friend class KrylovBase<T>;
    template <class V>
    int run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
    template <class V>
    int run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
};

// Conjugate gradients for Hermitian positive-definite A (recurrence: include/sprsolve_hip.h, sprs_cg_*; kernels: cg_fuse.hpp)
template <class T>
class Cg : public KrylovBase<T> {
   public:
    StateBlock<CgState<T>> state;
    int create(const sprs_csr *A, size_t size);
    void destroy() { state.destroy(); KrylovBase<T>::destroy(); }
    int solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                  size_t *its_out, Real<T> *res_out);

   private:
    friend class KrylovBase<T>;
    // the part both modes share: zero rhs, initial residual, z = M^-1 r, p = z, rho = conj(r).z; done = 1: answered already
    template <class V>
    int start(const Prec<T, V> &M, const T *rhs, T *x, Real<T> tol, Real<T> *rhs_norm, Real<T> *tol2, T *rho, bool *done, Real<T> *res_out);
    template <class V>
    int run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
    template <class V>
    int run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
};

// Restarted GMRES for any non-singular A (recurrence: include/sprsolve_hip.h, sprs_gmres_*; kernels and launch_cgs2: gmres_fuse.hpp)
template <class T>
class Gmres : public KrylovBase<T> {
   public:
    StateBlock<GmresState<T>> state;     // the host pushes and polls only its head (GmresHead)
    int m = 30;                  // restart length
    DotsBuf<T> dots;             // [GM_MAXM][grid] partials of the multi-dots
    T *coefs = nullptr;          // distributed: the m reduced coefficients of a pass, all-reduced in place
    int create(const sprs_csr *A, size_t size, size_t restart);
    void destroy();
    int solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                  size_t *its_out, Real<T> *res_out);

   private:
    friend class KrylovBase<T>;
    T *basis(int i) { return this->vec(i); }                 // v_0 .. v_m
    T *wvec() { return this->vec(m + 1); }
    T *zvec() { return this->vec(m + 2); }
    T *uvec() { return this->vec(m + 3); }                   // literal mode's x update
    void trace_step(double its, double g, double hn, T r, double c, T s);
    template <class V>
    int run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
    template <class V>
    int run_literal(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
};

// Thick-restart Lanczos for the extreme eigenpairs of a Hermitian A (recurrence: include/sprsolve_hip.h, sprs_eigsh_*; kernels:
// eigsh_fuse.hpp and GMRES's multi-vector Gram-Schmidt through launch_cgs2).  Single GPU, one mode; of KrylovBase it uses the
// work vectors, the partial slots and spmv() — no literal mode, trace or profile.
template <class T> struct LzState;      // eigsh_fuse.hpp
template <class T>
class Eigsh : public KrylovBase<T> {
   public:
    StateBlock<LzState<T>> state;        // the host pushes its head and reads the head once a cycle
    int m = 32;                          // ncv: the basis size
    DotsBuf<T> dots;                     // [LZ_MAXM][grid] partials of the multi-dots
    int create(const sprs_csr *A, size_t size, size_t ncv);
    void destroy();
    // v0: n entries (host where v0_host); vecs: k contiguous vectors of n entries or null (host where vecs_host: the basis is
    // rotated in place and copied out; device: LzRotate writes them, any alignment); vals / res / the counters: host
    int solve(size_t k, int which, const T *v0, bool v0_host, size_t max_restarts, Real<T> tol, Real<T> *vals_out, T *vecs, bool vecs_host,
              Real<T> *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);

   private:
    T *basis(int i) { return this->vec(i); }                 // v_0 .. v_m
    T *wvec() { return this->vec(m + 1); }
    int rotate(int me, int q, T *out, int64_t ostride);      // out[:, :q] = V[:, :me] S[:, :q]
};

// w = exp(tA) v for any square A: Arnoldi projection with Expokit's error-controlled sub-stepping (recurrence:
// include/sprsolve_hip.h, sprs_expm_*; kernels: expm_fuse.hpp, launch_cgs2 of gmres_fuse.hpp and the Lanczos norm).  Single
// GPU, one mode; of KrylovBase it uses the work vectors, the partial slots and spmv() — no literal mode, trace or profile.
template <class T> struct ExState;      // expm_fuse.hpp
template <class T>
class Expm : public KrylovBase<T> {
   public:
    StateBlock<ExState<T>> state;        // the host pushes its head and reads the head once a sub-step
    int m = 30;                          // ncv: the basis size
    DotsBuf<T> dots;                     // [EX_MAXM][grid] partials of the multi-dots
    int create(const sprs_csr *A, size_t size, size_t ncv);
    void destroy();
    // v, w: n entries each, on the host where `host` (w may be v); the six outputs: host
    int apply(Real<T> t, const T *v, bool host, Real<T> tol, size_t max_steps, Real<T> tau0, T *w, Real<T> *err_out, Real<T> *hump_out,
              Real<T> *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);

   private:
    T *basis(int i) { return this->vec(i); }                 // v_0 .. v_m
    T *pvec() { return this->vec(m + 1); }
    T *stage() { return this->vec(m + 2); }                  // the result of a host call or of an unaligned device w
};

// LOBPCG for the extreme eigenpairs of a Hermitian A, with any of the preconditioners (recurrence: include/sprsolve_hip.h,
// sprs_lobpcg_*; kernels: lobpcg_fuse.hpp and the Lanczos rotation).  Single GPU, one mode; of KrylovBase it uses the work vectors
// and spmv() — no literal mode, trace or profile.
template <class T> struct LobState;     // lobpcg_fuse.hpp
template <class T>
class Lobpcg : public KrylovBase<T> {
   public:
    StateBlock<LobState<T>> state;       // the host pushes it per solve and reads its head once per `poll` iterations
    int b = 0;                           // the block size: work holds X, P, W, AX, AP, AW, b contiguous vectors each
    T *gpart = nullptr;                  // [walker][G's upper triangle, K's upper triangle] partials of LobGram
    Real<T> *rpart = nullptr;            // [column][MAX_GRID] partials of the residual norms
    void *gsum = nullptr;                // G's and K's upper triangles summed in double (complex double for complex T)
    int create(const sprs_csr *A, size_t size, size_t block);
    void destroy();
    // X0: b contiguous vectors of n entries (host where x0_host); vecs: k contiguous vectors of n entries or null (host where
    // vecs_host; device: the rotation kernel writes them, any alignment); vals / res / the counters: host
    int solve_dev(const Precond<T> &P, size_t k, int which, const T *X0, bool x0_host, size_t max_iter, Real<T> tol, Real<T> *vals_out, T *vecs,
                  bool vecs_host, Real<T> *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);

   private:
    int gram(int layout, int m);
    template <class V>
    int run(const Prec<T, V> &M, size_t k, int which, const T *X0, bool x0_host, size_t max_iter, Real<T> tol, Real<T> *vals_out, T *vecs,
            bool vecs_host, Real<T> *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
};

// LSMR for min |rhs - A x|_2 (+ damping) on any A, rectangular included (recurrence: include/sprsolve_hip.h, sprs_lsmr_*; kernels:
// lsmr_fuse.hpp).  Two operators and two vector lengths: KrylovBase carries A, the m = rows side (u, w) and everything that
// is not tied to a length (context, poll, trace, profile, partial slots); the n = cols side (v, w', h, hbar) is held here.
template <class T>
class Lsmr : public KrylovBase<T> {
   public:
    using R = Real<T>;
    StateBlock<LsDev<R>> state;
    const sprs_csr *AH = nullptr;   // the adjoint handle: the caller's, or built here (own_AH)
    sprs_csr *own_AH = nullptr;
    size_t m = 0, nc = 0, stride_n = 0;
    T *work_n = nullptr;         // 4 * stride_n
    int create(const sprs_csr *A, const sprs_csr *AH_or_null);
    void destroy();
    // rhs: m entries, x: nc entries, both on the device and 16-byte aligned
    int solve_dev(const T *rhs, size_t rhs_len, T *x, size_t x_len, R damp, size_t max_iter, R tol, size_t *its_out, R *res_out, R *ares_out);

   private:
    T *nvec_(int i) { return work_n + (size_t)i * stride_n; }
    int mul(const sprs_csr *M, const T *x, T *y, const int *status);          // y = M x, profiled like KrylovBase::spmv
    int grid_of(size_t len) const;
    // what both modes share: |rhs|, u = rhs - A x, beta, v = A^H u / beta, alpha, h = v, hbar = 0; done: answered already
    int start(const T *rhs, T *x, R damp, LsIter<R> *s0, R *normb, bool *done, R *res_out, R *ares_out);
    int run(const T *rhs, T *x, R damp, size_t max_iter, R tol, size_t *its_out, R *res_out, R *ares_out);
    int run_literal(const T *rhs, T *x, R damp, size_t max_iter, R tol, size_t *its_out, R *res_out, R *ares_out);
};

// Thick-restart Lanczos bidiagonalisation for the extreme singular triplets of any A, rectangular included (recurrence:
// include/sprsolve_hip.h, sprs_svds_*; kernels: svds_fuse.hpp, launch_cgs2 of gmres_fuse.hpp, the Lanczos rotation, start kernel,
// head and solve frame (lz_begin / lz_results of eigsh_fuse.hpp).  Two
// operators and two vector lengths, as LSMR: Op = A and OpH = A^H where rows >= cols, else the other way round, so that Op is
// M x N with M >= N.  KrylovBase carries the M side (q_0 .. q_{l-1}, w) and the partial slots; the N side (p_0 .. p_l, w') is
// held here.  Single GPU, one mode — no literal mode, trace or profile.
template <class T> struct SvState;      // svds_fuse.hpp
template <class T>
class Svds : public KrylovBase<T> {
   public:
    using R = Real<T>;
    StateBlock<SvState<T>> state;        // the host pushes its head and reads the head once a cycle
    const sprs_csr *AH = nullptr;        // the adjoint handle: the caller's, or built here (own_AH)
    sprs_csr *own_AH = nullptr;
    const sprs_csr *Op = nullptr, *OpH = nullptr;
    bool swapped = false;                // Op = A^H: U and V change places on output
    int m = 32;                          // ncv: the basis size l
    size_t rows = 0, cols = 0, lenM = 0, lenN = 0, stride_n = 0;
    T *work_n = nullptr;                 // (m + 2) * stride_n
    DotsBuf<T> dots;                     // [LZ_MAXM][grid] partials of the multi-dots, grid = the larger side's
    int create(const sprs_csr *A, const sprs_csr *AH_or_null, size_t ncv);
    void destroy();
    // v0: min(rows, cols) entries (host where host); u / v: k contiguous vectors of rows / cols entries, both or neither (host:
    // the bases are rotated in place and copied out; device: LzRotate writes them, any alignment); vals / res / the counters: host
    int solve(size_t k, int which, const T *v0, bool host, size_t max_restarts, R tol, R *vals_out, T *u, T *v, R *res_out, size_t *nconv_out,
              size_t *restarts_out, size_t *matvecs_out);

   private:
    T *pvec(int i) { return work_n + (size_t)i * stride_n; }     // p_0 .. p_m, then w'
    T *qvec(int i) { return this->vec(i); }                      // q_0 .. q_{m-1}, then w
    int grid_of(size_t len) const;
};

// Conjugate gradients on a block of up to kmax <= 8 right-hand sides at once (cg_many.hip; kernels: spmm.hip, cg_many_fuse.hpp).
// Every column runs Cg<T>'s recurrence on its own scalars and stops on its own events.  Single GPU, fused mode only.
template <class T> struct CgManyState;   // cg_many_fuse.hpp
template <class T>
class CgMany {
   public:
    sprs_ctx *ctx = nullptr;
    const sprs_csr *A = nullptr;
    size_t n = 0, n_pad = 0;     // rows; rows of the work blocks (a multiple of 4)
    int kmax = 0, kp = 0, lg = 0;   // the most columns a solve may carry; the blocks' column stride (a power of two) and its log2
    T *work = nullptr;           // x, r, p, q, z: five n_pad x kp blocks
    T *rhs_buf = nullptr, *x_buf = nullptr;   // staging of the host entry points (n x kmax)
    T *partPQ = nullptr, *partRZ = nullptr;   // [column][workgroup] partials
    Real<T> *partN = nullptr;
    StateBlock<CgManyState<T>> state;
    int create(const sprs_csr *A, size_t size, size_t k);
    void destroy();
    T *blk(int i) { return work + (size_t)i * n_pad * (size_t)kp; }
    // rhs, x: device, n x k row-major.  its_out / res_out / status_out: host arrays of k entries (each may be null)
    int solve_dev(const sprs_diag *P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t k, size_t max_iter, Real<T> tol,
                  size_t *its_out, Real<T> *res_out, int *status_out);

   private:
    template <class V>
    int run(const V *dinv, const T *rhs, T *x, int k, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out, int *status_out);
};

// Multi-shift conjugate gradients: (A + sigma_j I) x_j = rhs for up to mmax <= 8 real shifts sigma_j >= 0 in ONE Krylov run on A
// (recurrence: include/sprsolve_hip.h, sprs_cgshift_*; cg_shift.hip; kernels: cg_shift_fuse.hpp).  Single GPU, one mode, no
// preconditioner; of KrylovBase it uses the work vectors, the partial slots and spmv() — no literal mode, trace or profile.
template <class T> struct CgShiftState;  // cg_shift_fuse.hpp
template <class T>
class CgShift : public KrylovBase<T> {
   public:
    StateBlock<CgShiftState<T>> state;
    int mmax = 0;                // the most shifts a solve may carry: work holds r, p, q, then mmax columns of P and mmax of X
    int create(const sprs_csr *A, size_t size, size_t mmax);
    void destroy() { state.destroy(); KrylovBase<T>::destroy(); }
    // shifts: m host values; rhs: n entries, x: m contiguous vectors of n entries (output only), both on the host where `host`;
    // its_out / res_out / status_out: host arrays of m entries (each may be null)
    int solve(const Real<T> *shifts, size_t m, const T *rhs, size_t rhs_len, bool host, T *x, size_t x_len, size_t max_iter, Real<T> tol,
              size_t *its_out, Real<T> *res_out, int *status_out);

   private:
    int run(const Real<T> *shifts, int m, const T *rhs, bool host, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out,
            int *status_out);
};

// IDR(s) for any square non-singular A, with any of the preconditioners (recurrence: include/sprsolve_hip.h, sprs_idrs_*; idrs.hip;
// kernels: idrs_fuse.hpp).  Single GPU, one mode; of KrylovBase it uses the work vectors, the partial
// slots, spmv() and the trace — no literal mode or profile.
template <class T> struct IdrsState;     // idrs_fuse.hpp
template <class T>
class Idrs : public KrylovBase<T> {
   public:
    StateBlock<IdrsState<T>> state;      // the host pushes it per solve and reads its head every poll_interval() products
    int s = 4;                           // the shadow space's dimension: work holds r, v, vh, t, then s columns each of G, U and P
    DotsBuf<std::conditional_t<is_complex<T>::value, cplx, double>> dots;   // partials in double: [8][grid] for q = P^H g_k, [8][grid] for f = P^H r, |r|^2, conj(r).t, conj(t).t
    int create(const sprs_csr *A, size_t size, size_t s_dim);
    void destroy() { state.destroy(); dots.destroy(); KrylovBase<T>::destroy(); }
    // P: nothing, a diagonal (a `const sprs_diag *` converts) or an applied ILU(0) / AMG / FSAI handle
    int solve_dev(const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter, Real<T> tol,
                  size_t *its_out, Real<T> *res_out);

   private:
    friend class KrylovBase<T>;
    T *gvec(int i) { return this->vec(4 + i); }
    T *uvec(int i) { return this->vec(4 + s + i); }
    T *pvec(int i) { return this->vec(4 + 2 * s + i); }
    template <class V>
    int run(const Prec<T, V> &M, const T *rhs, T *x, size_t max_iter, Real<T> tol, size_t *its_out, Real<T> *res_out);
    // (sprs_solver_set_mode refuses mode 1 for this kind: never reached)
    template <class V>
    int run_literal(const Prec<T, V> &, const T *, T *, size_t, Real<T>, size_t *, Real<T> *) { return SPRS_INVALID_ARGUMENT; }
};

// ======================================================================= KrylovBase's member templates
template <class T>
template <class U, class W>
int KrylovBase<T>::handoff(int slot, int P, const U *a, Part<U> *oa, const W *b, Part<W> *ob) {
    if (!A->dist) {
        *oa = Part<U>{a, P};
        if (ob) *ob = Part<W>{b, P};
        return SPRS_OK;
    }
    if (use_p2p()) {    // both values are in the same mailbox entries
        *oa = Part<U>{reinterpret_cast<const U *>(mbox_entries(slot)), comm()->world, comm()->seq[slot]};
        if (ob) *ob = Part<W>{reinterpret_cast<const W *>(mbox_entries(slot)), comm()->world, comm()->seq[slot]};
        return SPRS_OK;
    }
    double *ra = red + 2 * slot, *rb = red + 2 * slot + 2;
    SPRS_TRY(allreduce_sum(comm(), ra, (ob ? 32 : 16) / sizeof(Real<T>), sizeof(Real<T>) == 4));
    *oa = Part<U>{reinterpret_cast<const U *>(ra), 1};
    if (ob) *ob = Part<W>{reinterpret_cast<const W *>(rb), 1};
    return SPRS_OK;
}

template <class T>
template <class F>
int KrylovBase<T>::profiled(F &&run, bool one_kernel) {
    if (!profile) return run();
    // The events are not free: a launch that carries them costs ~6 us more (completion signal + timestamps; measured on the
    // 30-50 us iterations of cfg 2 / 3 / 4, and 11-13 us per cfg-5 iteration = 1 %).  profile = k >= 2 brackets one PAIR of
    // consecutive SpMV-class steps in k (a pair: BiCGStab's K2 and K4 are sampled equally often).
    const size_t call = prof_calls++;
    last_pair = -1;
    if (profile >= 2 && (call >> 1) % (size_t)profile != 0) return run();
    if (ev_used + 2 > ev.size()) {
        for (int k = 0; k < 2; ++k) {
            hipEvent_t e;
            SPRS_HIP_TRY(ctx, hipEventCreate(&e));
            ev.push_back(e);
        }
    }
    int st;
    if (one_kernel) {
        // one kernel per SpMV: the launch records its own begin / end (what rocprofv3 reports as the kernel's duration)
        ctx->prof_start = ev[ev_used]; ctx->prof_stop = ev[ev_used + 1];
        st = run();
        ctx->prof_start = nullptr; ctx->prof_stop = nullptr;
    } else {
        // exchange + two launches: bracket the whole thing (includes the wait for the halo)
        SPRS_HIP_TRY(ctx, hipEventRecord(ev[ev_used], ctx->stream));
        st = run();
        SPRS_HIP_TRY(ctx, hipEventRecord(ev[ev_used + 1], ctx->stream));
    }
    ev_pair.resize(ev_used / 2);
    ev_pair.push_back(EvPair{call});
    last_pair = (long)(ev_used / 2);
    ev_used += 2;
    return st;
}

// The preconditioner as a solve takes it.  An applied handle passes its own check; a diagonal's size and scalar type are
// checked.  Then run(M) is called with M a Prec<T, V> (s: the solver, for its context, A and n): V = T for a complex M^-1
// (complex T only), Real<T> otherwise — for an applied one and for none as well.
template <class T, class S, class F>
int with_prec(const Precond<T> &P, const S &s, F &&run) {
    using R = Real<T>;
    if (P.is_applied) {
        SPRS_TRY(P.applied.check(s.A, s.n));
        return run(Prec<T, R>{s.ctx, s.n, nullptr, P.applied});
    }
    const sprs_diag *D = P.diag;
    if (D && D->n != s.n) return SPRS_DIM_MISMATCH;
    if (D && D->t_dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if (D && D->v_complex) {
        if constexpr (is_complex<T>::value) return run(Prec<T, T>{s.ctx, s.n, (const T *)D->dinv, {}});
        else return SPRS_INVALID_ARGUMENT;
    }
    return run(Prec<T, R>{s.ctx, s.n, D ? (const R *)D->dinv : nullptr, {}});
}

template <class T>
template <class S>
int KrylovBase<T>::solve(S &s, bool no_precond, const Precond<T> &P, const T *rhs, size_t rhs_len, T *x, size_t x_len, size_t max_iter,
                         Real<T> tol, size_t *its_out, Real<T> *res_out) {
    size_t its_dummy; Real<T> res_dummy;
    if (!its_out) its_out = &its_dummy;
    if (!res_out) res_out = &res_dummy;
    if (rhs_len != s.n) return SPRS_INCOMPATIBLE_RHS_SIZE;                  // bicg_stab.rs:44-48, minres.rs:40-44
    if (x_len != s.n) return SPRS_INCOMPATIBLE_X_SIZE;                      // bicg_stab.rs:49-53, minres.rs:45-49
    if (no_precond && P.any()) return SPRS_INVALID_ARGUMENT;                // CSMinRes has no precond_solve
    return with_prec<T>(P, s, [&](const auto &M) -> int {
        using V = std::remove_cv_t<std::remove_pointer_t<decltype(M.dinv)>>;
        SPRS_TRY(s.begin_solve());
        const int st = s.mode == 1 ? s.template run_literal<V>(M, rhs, x, max_iter, tol, its_out, res_out)
                                   : s.template run<V>(M, rhs, x, max_iter, tol, its_out, res_out);
        if (st >= SPRS_ERR_HIP) return st;
        SPRS_TRY(s.end_solve());
        return st;
    });
}

}  // namespace sprs

// opaque C handles: type-erased over T, one layout
struct sprs_solver_handle {
    int dtype;
    void *impl;
};
struct sprs_bicgstab : sprs_solver_handle {};
struct sprs_minres : sprs_solver_handle {};
struct sprs_csminres : sprs_solver_handle {};
struct sprs_cg : sprs_solver_handle {};
struct sprs_gmres : sprs_solver_handle {};
struct sprs_cg_many : sprs_solver_handle {};
struct sprs_cg_shift : sprs_solver_handle {};
struct sprs_idrs : sprs_solver_handle {};
struct sprs_lsmr : sprs_solver_handle {};
struct sprs_eigsh : sprs_solver_handle {};
struct sprs_lobpcg : sprs_solver_handle {};
struct sprs_svds : sprs_solver_handle {};
struct sprs_expm : sprs_solver_handle {};
