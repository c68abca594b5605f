// Smoothed-aggregation algebraic multigrid: the hierarchy (built at creation: the aggregation and the prolongator formula on the
// host, serial; the three sparse products of every level on the device, spgemm.hip, with the bits of the serial loop) and the
// V(1,1) cycle that applies it as a preconditioner.  sprs_amg_create_dev builds the same handle without the host: a parallel
// aggregation rule and every other step of a level in HBM (amg_setup.hpp, included below).  No reference analogue; the rules
// and the order of every sum are stated in the header (sprs_amg_*) and restated by tests/_amg_ref.py and tests/_amg_par_ref.py.
//
// ilu0.hip's two ideas carry the device side:
//  * every operator of the hierarchy (A_l, P_l, R_l) is stored in the sliced-row layout of sell.hpp (position = row) and ONE
//    LANE folds ONE ROW left to right with its sell_fold, so an application has the bits of the serial loop;
//  * everything small is batched: the levels of at most AMG_TAIL_ROWS rows run in ONE launch of ONE workgroup — down, the
//    coarse solve and up — with __syncthreads() between the steps (the barrier orders one step's stores before the next step's
//    loads: all wavefronts of a workgroup share one CU and its L1).  The larger levels take five launches each: the
//    pre-smoothing from zero, the fused residual, the restriction, the prolongation with accumulate and the fused Jacobi sweep.
// No kernel ever waits for another workgroup: stream order between launches is the only inter-workgroup synchronisation.
#include <algorithm>
#include <cmath>
#include <memory>

#include "device.hpp"
#include "sell.hpp"

using namespace sprs;

namespace sprs {
constexpr int AMG_TAIL_ROWS = 1024;      // levels of at most this many rows run inside the tail kernel
constexpr int AMG_COARSE_LIMIT = 1024;   // largest coarse_max: the dense LU is applied by the tail kernel (AMG_COARSE_LIMIT <= AMG_TAIL_ROWS)
constexpr int AMG_COARSE_SWEEPS = 8;     // damped-Jacobi sweeps in place of the LU when the coarsest level has more than coarse_max rows
constexpr int AMG_MAX_LEVELS = 32;
constexpr int AMG_STAGES = 11;           // stages of the device set-up that sprs_amg_setup_stage_ms reports
}  // namespace sprs

namespace {

// ------------------------------------------------------------------------------------------------ host side: the hierarchy
template <class T>
struct HCsr {
    int32_t n = 0, ncols = 0;
    std::vector<int32_t> ip, ix;
    std::vector<T> v;
};

template <class T> inline Real<T> hmod(T a) {   // |a|: fabs, or sqrt(re re + im im) (not hypot: every step is one IEEE operation)
    if constexpr (is_complex<T>::value) return std::sqrt(ssq(a));
    else return std::fabs(a);
}

template <class T>
void transpose_conj(const HCsr<T> &P, HCsr<T> &R) {
    R.n = P.ncols; R.ncols = P.n;
    R.ip.assign((size_t)R.n + 1, 0);
    for (int32_t c : P.ix) R.ip[(size_t)c + 1]++;
    for (int32_t i = 0; i < R.n; ++i) R.ip[i + 1] += R.ip[i];
    R.ix.resize(P.ix.size()); R.v.resize(P.ix.size());
    std::vector<int32_t> fill(R.ip.begin(), R.ip.end() - 1);
    for (int32_t i = 0; i < P.n; ++i)
        for (int32_t p = P.ip[i]; p < P.ip[i + 1]; ++p) {
            const int32_t d = fill[P.ix[p]]++;
            R.ix[d] = i; R.v[d] = sconj(P.v[p]);
        }
}

// the three aggregation passes of the header -> number of aggregates
template <class T>
int32_t aggregate(const HCsr<T> &A, const std::vector<T> &diag, Real<T> theta, std::vector<int32_t> &agg) {
    using R = Real<T>;
    const int32_t n = A.n;
    std::vector<R> md((size_t)n), sq(A.ix.size());
    std::vector<char> strong(A.ix.size(), 0);
    for (int32_t i = 0; i < n; ++i) md[i] = hmod(diag[i]);
    const R th2 = theta * theta;
    for (int32_t i = 0; i < n; ++i)
        for (int32_t p = A.ip[i]; p < A.ip[i + 1]; ++p) {
            const int32_t j = A.ix[p];
            sq[p] = ssq(A.v[p]);
            strong[p] = j != i && sq[p] >= th2 * (md[i] * md[j]);
        }
    agg.assign((size_t)n, -1);
    int32_t count = 0;
    for (int32_t i = 0; i < n; ++i) {                        // pass 1
        if (agg[i] >= 0) continue;
        bool free_nb = true;
        for (int32_t p = A.ip[i]; p < A.ip[i + 1] && free_nb; ++p) if (strong[p] && agg[A.ix[p]] >= 0) free_nb = false;
        if (!free_nb) continue;
        agg[i] = count;
        for (int32_t p = A.ip[i]; p < A.ip[i + 1]; ++p) if (strong[p]) agg[A.ix[p]] = count;
        ++count;
    }
    const std::vector<int32_t> snap(agg);
    for (int32_t i = 0; i < n; ++i) {                        // pass 2
        if (snap[i] >= 0) continue;
        R best = R(-1); int32_t bj = -1;
        for (int32_t p = A.ip[i]; p < A.ip[i + 1]; ++p)
            if (strong[p] && snap[A.ix[p]] >= 0 && sq[p] > best) { best = sq[p]; bj = A.ix[p]; }
        if (bj >= 0) agg[i] = snap[bj];
    }
    for (int32_t i = 0; i < n; ++i) {                        // pass 3 (the header: as the rules stand it finds no row)
        if (agg[i] >= 0) continue;
        agg[i] = count;
        for (int32_t p = A.ip[i]; p < A.ip[i + 1]; ++p) if (strong[p] && agg[A.ix[p]] < 0) agg[A.ix[p]] = count;
        ++count;
    }
    return count;
}

template <class T>
struct HLevel {
    HCsr<T> A, P, R;             // P, R: empty on the coarsest level
    std::vector<T> diag;
    std::vector<int32_t> agg;
    Real<T> omega = 0;
};

// diagonal of A with its checks: -1, or the smallest offending row
template <class T>
int64_t take_diag(const HCsr<T> &A, std::vector<T> &diag) {
    diag.assign((size_t)A.n, szero<T>());
    for (int32_t i = 0; i < A.n; ++i) {
        const int64_t d = diag_pos(A.ip.data(), A.ix.data(), i);
        if (d < 0) return i;
        diag[i] = A.v[(size_t)d];
        if (bad_pivot(diag[i])) return i;
    }
    return -1;
}

// omega = 4 / (3 rho), rho = max_i (sum_j |a_ij|, left to right from zero) / |a_ii|
template <class T>
Real<T> jacobi_omega(const HCsr<T> &A, const std::vector<T> &diag) {
    using R = Real<T>;
    R rho = R(0);
    bool first = true;
    for (int32_t i = 0; i < A.n; ++i) {
        R s = R(0);
        for (int32_t p = A.ip[i]; p < A.ip[i + 1]; ++p) s = s + hmod(A.v[p]);
        const R q = s / hmod(diag[i]);
        if (first || q > rho || q != q) { rho = q; first = false; }
    }
    if (first) rho = R(1);
    return R(4) / (R(3) * rho);
}

// ------------------------------------------------------------------------------------------------ device side
enum : int { OP_MUL = 0, OP_ACC = 1, OP_RESID = 2, OP_JACOBI = 3 };

// One row of one step.  OP_MUL: out = M x.  OP_ACC: out = y + M x (y may be out).  OP_RESID: out = y - M x.
// OP_JACOBI: out = x + (omega (y - M x)) / d (out is not x; y may be out).  M x: sell_fold, left to right from zero.
template <class T, int OP>
__device__ __forceinline__ void amg_row(const SellDev<T> &M, int row, const T *x, const T *y, const T *d, Real<T> omega, T *out) {
    const T sigma = sell_fold<T>(M, row, x);
    if (OP == OP_MUL) out[row] = sigma;
    else if (OP == OP_ACC) out[row] = sadd(y[row], sigma);
    else if (OP == OP_RESID) out[row] = ssub(y[row], sigma);
    else out[row] = sadd(x[row], sdiv(smulr(ssub(y[row], sigma), omega), d[row]));
}

template <class T, int OP>
__global__ __launch_bounds__(BLOCK) void amg_op_kernel(SellDev<T> M, int n, const T *x, const T *y, const T *d, Real<T> omega, T *out) {
    const int row = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (row < n) amg_row<T, OP>(M, row, x, y, d, omega, out);
}

// pre-smoothing from zero: x = (omega b) / d
template <class T>
__global__ __launch_bounds__(BLOCK) void amg_scale_kernel(int n, const T *b, const T *d, Real<T> omega, T *x) {
    const int row = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (row < n) x[row] = sdiv(smulr(b[row], omega), d[row]);
}

template <class T>
struct TailLevel {
    SellDev<T> A, P, R;
    const T *diag;
    Real<T> omega;
    int n;
    T *b, *x, *x2, *r;           // the level's vectors (b: its right-hand side, written by the level above)
};

// Levels [l0, L] in one workgroup: down, the coarse solve on level L, up.  b0 / out0 stand for level l0's right-hand side and
// result (the caller's vectors when the tail is the whole hierarchy; out0 may be b0).  lu: the coarsest level's dense LU,
// column-major, or null: AMG_COARSE_SWEEPS damped-Jacobi sweeps from zero.
template <class T>
__global__ __launch_bounds__(BLOCK) void amg_tail_kernel(const TailLevel<T> *lv, int l0, int L, const T *b0, T *out0, const T *lu) {
    __shared__ T w[AMG_COARSE_LIMIT];
    const int tid = (int)threadIdx.x;
    for (int l = l0; l < L; ++l) {                           // down
        const TailLevel<T> V = lv[l];
        const T *b = l == l0 ? b0 : V.b;
        for (int i = tid; i < V.n; i += BLOCK) V.x[i] = sdiv(smulr(b[i], V.omega), V.diag[i]);
        __syncthreads();
        for (int i = tid; i < V.n; i += BLOCK) amg_row<T, OP_RESID>(V.A, i, V.x, b, nullptr, V.omega, V.r);
        __syncthreads();
        const int nc = lv[l + 1].n;
        T *bc = lv[l + 1].b;
        for (int i = tid; i < nc; i += BLOCK) amg_row<T, OP_MUL>(V.R, i, V.r, nullptr, nullptr, V.omega, bc);
        __syncthreads();
    }
    const T *e;                                              // the result of the level below the one being finished
    {
        const TailLevel<T> V = lv[L];
        const T *b = L == l0 ? b0 : V.b;
        T *res = L == l0 ? out0 : V.x2;
        const int n = V.n;
        if (lu) {
            // w_i = ((b_i - l_i0 w_0) - l_i1 w_1) - ..., then x_j = (((w_j - u_j,n-1 x_n-1) - ...) - u_j,j+1 x_j+1) / u_jj:
            // a column sweep, every row's subtractions in the stated order
            for (int i = tid; i < n; i += BLOCK) w[i] = b[i];
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                const T wj = w[j];
                const T *col = lu + (size_t)j * n;
                for (int i = j + 1 + tid; i < n; i += BLOCK) w[i] = ssub(w[i], smul(col[i], wj));
                __syncthreads();
            }
            for (int j = n - 1; j >= 0; --j) {
                const T *col = lu + (size_t)j * n;
                const T xj = sdiv(w[j], col[j]);
                if (tid == 0) res[j] = xj;
                for (int i = tid; i < j; i += BLOCK) w[i] = ssub(w[i], smul(col[i], xj));
                __syncthreads();
            }
            e = res;
        } else {
            T *cur = V.x, *nxt = V.x2;
            for (int i = tid; i < n; i += BLOCK) cur[i] = sdiv(smulr(b[i], V.omega), V.diag[i]);
            __syncthreads();
            for (int s = 1; s < AMG_COARSE_SWEEPS; ++s) {
                for (int i = tid; i < n; i += BLOCK) amg_row<T, OP_JACOBI>(V.A, i, cur, b, V.diag, V.omega, nxt);
                __syncthreads();
                T *t = cur; cur = nxt; nxt = t;
            }
            if (L == l0) {
                for (int i = tid; i < n; i += BLOCK) out0[i] = cur[i];
                __syncthreads();
            }
            e = cur;
        }
    }
    for (int l = L - 1; l >= l0; --l) {                      // up
        const TailLevel<T> V = lv[l];
        const T *b = l == l0 ? b0 : V.b;
        T *res = l == l0 ? out0 : V.x2;
        for (int i = tid; i < V.n; i += BLOCK) amg_row<T, OP_ACC>(V.P, i, e, V.x, nullptr, V.omega, V.x);
        __syncthreads();
        for (int i = tid; i < V.n; i += BLOCK) amg_row<T, OP_JACOBI>(V.A, i, V.x, b, V.diag, V.omega, res);
        __syncthreads();
        e = res;
    }
}

// A CSR matrix in HBM for the products of the set-up (spgemm.hip): owned, or borrowed from the caller's handle (level 0)
template <class T>
struct DCsr {
    int32_t n = 0, ncols = 0;
    int64_t nnz = 0;
    int32_t *ip = nullptr, *ix = nullptr;
    T *v = nullptr;
    bool own = true;
    DCsr() = default;
    DCsr(const DCsr &) = delete;
    DCsr &operator=(const DCsr &) = delete;
    ~DCsr() { reset(); }
    void reset() {
        if (own) for (void *p : {(void *)ip, (void *)ix, (void *)v}) if (p) (void)hipFree(p);
        ip = nullptr; ix = nullptr; v = nullptr; own = true;
    }
    void take(DCsr &o) {
        reset();
        n = o.n; ncols = o.ncols; nnz = o.nnz; ip = o.ip; ix = o.ix; v = o.v; own = o.own;
        o.ip = nullptr; o.ix = nullptr; o.v = nullptr;
    }
};

template <class T>
bool to_device(const HCsr<T> &M, DCsr<T> &D) {
    D.reset();
    D.n = M.n; D.ncols = M.ncols; D.nnz = (int64_t)M.ix.size();
    return dev_upload(&D.ip, M.ip.data(), M.ip.size()) && dev_upload(&D.ix, M.ix.data(), M.ix.size()) && dev_upload(&D.v, M.v.data(), M.v.size());
}

template <class T>
bool to_host(const DCsr<T> &D, HCsr<T> &M) {
    M.n = D.n; M.ncols = D.ncols;
    M.ip.resize((size_t)D.n + 1); M.ix.resize((size_t)D.nnz); M.v.resize((size_t)D.nnz);
    if (hipMemcpy(M.ip.data(), D.ip, sizeof(int32_t) * M.ip.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (D.nnz == 0) return true;
    return hipMemcpy(M.ix.data(), D.ix, sizeof(int32_t) * M.ix.size(), hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(M.v.data(), D.v, sizeof(T) * M.v.size(), hipMemcpyDeviceToHost) == hipSuccess;
}

// C = A B in Gustavson order on the device: the bits of the serial loop (the contract of sprs_csr_matmul)
template <class T>
int dev_product(sprs_ctx *c, const DCsr<T> &A, const DCsr<T> &B, DCsr<T> &C) {
    C.reset();
    C.n = A.n; C.ncols = B.ncols;
    return spgemm_dev<T>(c, "sprs_amg", A.n, B.n, B.ncols, A.ip, A.ix, A.v, B.ip, B.ix, B.v, &C.ip, &C.ix, &C.v, &C.nnz, nullptr);
}

template <class T>
bool build_sell(SellMat &M, const HCsr<T> &A) {   // position = row
    return M.upload(A.n, sell_pack<T>(A.n, [](size_t p) { return (int32_t)p; }, [&](int32_t i) { return A.ip[i]; }, [&](int32_t i) { return A.ip[i + 1]; },
                                      A.ix.data(), A.v.data()));
}

struct AmgLevel {
    int32_t n = 0;
    int64_t nnz = 0, pnnz = 0;
    SellMat A, P, R;
    void *diag = nullptr;        // device, n of T
    double omega = 0;
    void *b = nullptr, *x = nullptr, *x2 = nullptr, *r = nullptr;   // device, n of T each
    // host copies for sprs_amg_level_read (values as bytes of T): the host set-up's, empty on a device-built handle
    std::vector<int32_t> a_ip, a_ix, p_ip, p_ix, r_ip, r_ix, agg;
    std::vector<char> a_v, p_v, r_v;
    // the device set-up keeps the aggregates in HBM (n of int32; null on the coarsest level) and unpacks A, P, R on demand
    int32_t *agg_dev = nullptr;
    int64_t rounds = 0;          // pass-1 rounds of the device aggregation
};

}  // namespace

struct sprs_amg {
    sprs_ctx *ctx = nullptr;
    int dtype = 0;
    int64_t n = 0;
    std::vector<AmgLevel> lv;
    int tail = 0;                // first level that runs inside the tail kernel (== levels: no tail)
    int lu_n = 0;                // rows of the dense LU of the coarsest level (0: Jacobi sweeps)
    void *lu = nullptr;          // device, lu_n * lu_n of T, column-major
    void *tail_desc = nullptr;   // device, levels of TailLevel<T>
    int64_t launches = 0;
    void *in_tmp = nullptr, *out_tmp = nullptr;   // staging of the host entry points (lazily allocated)
    int setup = 0;               // 0: built by sprs_amg_create (host), 1: by sprs_amg_create_dev
    double stage_ms[AMG_STAGES] = {0};            // device set-up under SPRS_CREATE_TRACE: host clock per stage (SetupClock); zeros otherwise
};

namespace {

template <class T>
void keep_host(const HCsr<T> &M, std::vector<int32_t> &ip, std::vector<int32_t> &ix, std::vector<char> &v) {
    ip = M.ip; ix = M.ix;
    v.resize(sizeof(T) * M.v.size());
    if (!M.v.empty()) memcpy(v.data(), M.v.data(), v.size());
}

// the coarse solve: dense no-pivot LU of Ac in the k-i-j order, kept column-major -> -1, or the row of a pivot nobody may divide by
template <class T>
int64_t dense_lu(const HCsr<T> &Ac, std::vector<T> &lu) {
    const size_t m = (size_t)Ac.n;
    lu.assign(m * m, szero<T>());
    for (int32_t i = 0; i < Ac.n; ++i)
        for (int32_t p = Ac.ip[i]; p < Ac.ip[i + 1]; ++p) lu[(size_t)Ac.ix[p] * m + i] = Ac.v[p];
    for (size_t k = 0; k < m; ++k) {
        const T piv = lu[k * m + k];
        if (bad_pivot(piv)) return (int64_t)k;
        for (size_t i = k + 1; i < m; ++i) lu[k * m + i] = sdiv(lu[k * m + i], piv);
        for (size_t j = k + 1; j < m; ++j) {                 // (the j loop outside: column-major; each entry sees the same one update)
            const T ukj = lu[j * m + k];
            for (size_t i = k + 1; i < m; ++i) lu[j * m + i] = ssub(lu[j * m + i], smul(lu[k * m + i], ukj));
        }
    }
    return -1;
}

// What both set-ups end with, once every level's operators, diagonal and vectors are in place: the tail and the launch count.
template <class T>
int finish_handle(sprs_amg *P) {
    using R = Real<T>;
    const int nlev = (int)P->lv.size();
    // the tail: every level of at most AMG_TAIL_ROWS rows (levels only shrink)
    P->tail = nlev;
    for (int l = nlev - 1; l >= 0 && P->lv[l].n <= AMG_TAIL_ROWS; --l) P->tail = l;
    std::vector<TailLevel<T>> td((size_t)nlev);
    for (int l = 0; l < nlev; ++l) {
        const AmgLevel &D = P->lv[l];
        td[l] = TailLevel<T>{D.A.dev<T>(), D.P.dev<T>(), D.R.dev<T>(), (const T *)D.diag, (R)D.omega, D.n, (T *)D.b, (T *)D.x, (T *)D.x2, (T *)D.r};
    }
    TailLevel<T> *dt = nullptr;
    if (!dev_upload(&dt, td.data(), td.size())) { P->tail_desc = dt; return SPRS_ERR_HIP; }
    P->tail_desc = dt;
    // launches of one application: five per level above the tail (three down, two up), the tail's one, and where the
    // coarsest level is above the tail its Jacobi sweeps
    const int upper = std::min(P->tail, nlev - 1);
    P->launches = 5 * (int64_t)upper + (P->tail < nlev ? 1 : AMG_COARSE_SWEEPS);
    return SPRS_OK;
}

template <class T>
int amg_create(const sprs_csr *A, double theta_d, int64_t coarse_max, int64_t max_levels, sprs_amg **out, int64_t *row_out) {
    using R = Real<T>;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (A->nnz > (int64_t)INT32_MAX) {
        snprintf(c->err, sizeof(c->err), "sprs_amg: more than 2^31 - 1 stored entries");
        return SPRS_INVALID_ARGUMENT;
    }
    // one host copy of the pattern and the values
    std::vector<HLevel<T>> H(1);
    HCsr<T> &A0 = H[0].A;
    A0.n = A0.ncols = (int32_t)A->nrows;
    A0.v.resize((size_t)A->nnz);
    SPRS_TRY(host_pattern(A, "sprs_amg", A0.ip, A0.ix, A0.v.data()));
    // the hierarchy
    const R theta = (R)theta_d;
    DCsr<T> dA;                                              // the level's operator in HBM: level 0 reads the handle's own arrays
    dA.own = false; dA.n = dA.ncols = A0.n; dA.nnz = A->nnz;
    dA.ip = A->row_ptr; dA.ix = A->col_idx; dA.v = (T *)A->val;
    while (true) {
        const int l = (int)H.size() - 1;
        HLevel<T> &Lh = H[l];
        const int64_t bad = take_diag(Lh.A, Lh.diag);
        if (bad >= 0) { if (row_out) *row_out = bad; return SPRS_ZERO_DIAGONAL; }
        Lh.omega = jacobi_omega(Lh.A, Lh.diag);
        const int32_t n = Lh.A.n;
        if (n <= coarse_max || l + 1 >= max_levels) break;
        const int32_t nc = aggregate(Lh.A, Lh.diag, (R)(theta * std::ldexp(R(1), -l)), Lh.agg);
        if (2 * (int64_t)nc > n) { Lh.agg.clear(); break; }    // the half-rows stop: this level is the coarsest
        HCsr<T> Tm, AT, Ac;
        Tm.n = n; Tm.ncols = nc; Tm.ip.resize((size_t)n + 1); Tm.ix = Lh.agg; Tm.v.assign((size_t)n, sone<T>());
        for (int32_t i = 0; i <= n; ++i) Tm.ip[i] = i;
        // the three products run on the device (spgemm.hip); A T and A_c come back for the host steps, A P never leaves HBM
        DCsr<T> dT, dAT, dP, dR, dAP, dAc;
        if (!to_device(Tm, dT)) return SPRS_ERR_HIP;
        SPRS_TRY(dev_product(c, dA, dT, dAT));
        if (!to_host(dAT, AT)) return SPRS_ERR_HIP;
        dT.reset(); dAT.reset();
        Lh.P = AT;
        for (int32_t i = 0; i < n; ++i)                      // p_ic = t_ic - (omega (A T)_ic) / d_i
            for (int32_t p = AT.ip[i]; p < AT.ip[i + 1]; ++p) {
                const T t = AT.ix[p] == Lh.agg[i] ? sone<T>() : szero<T>();
                Lh.P.v[p] = ssub(t, sdiv(smulr(AT.v[p], Lh.omega), Lh.diag[i]));
            }
        transpose_conj(Lh.P, Lh.R);
        if (!to_device(Lh.P, dP) || !to_device(Lh.R, dR)) return SPRS_ERR_HIP;
        SPRS_TRY(dev_product(c, dA, dP, dAP));
        SPRS_TRY(dev_product(c, dR, dAP, dAc));
        if (!to_host(dAc, Ac)) return SPRS_ERR_HIP;
        dA.take(dAc);                                        // the next level's operator stays where it was formed
        H.emplace_back();
        H.back().A = std::move(Ac);
    }
    const int nlev = (int)H.size();
    const HCsr<T> &Ac = H[nlev - 1].A;
    std::vector<T> lu;
    int lu_n = 0;
    if (Ac.n <= coarse_max) {
        lu_n = Ac.n;
        const int64_t bad = dense_lu(Ac, lu);
        if (bad >= 0) { if (row_out) *row_out = bad; return SPRS_ZERO_DIAGONAL; }
    }

    // the device side
    std::unique_ptr<sprs_amg, int (*)(sprs_amg *)> guard(new sprs_amg(), sprs_amg_destroy);   // freed on every early exit, a throwing allocation included
    sprs_amg *P = guard.get();
    P->ctx = c; P->dtype = A->dtype; P->n = A->nrows; P->lu_n = lu_n;
    P->lv.resize((size_t)nlev);
    for (int l = 0; l < nlev; ++l) {
        AmgLevel &D = P->lv[l];
        HLevel<T> &Lh = H[l];
        D.n = Lh.A.n; D.nnz = (int64_t)Lh.A.ix.size(); D.pnnz = (int64_t)Lh.P.ix.size(); D.omega = (double)Lh.omega;
        bool ok = build_sell<T>(D.A, Lh.A);
        if (ok && l + 1 < nlev) ok = build_sell<T>(D.P, Lh.P) && build_sell<T>(D.R, Lh.R);
        T *dd = nullptr;
        ok = ok && dev_upload(&dd, Lh.diag.data(), Lh.diag.size());
        D.diag = dd;
        for (void **v : {&D.b, &D.x, &D.x2, &D.r}) ok = ok && hipMalloc(v, sizeof(T) * ((size_t)D.n + 2)) == hipSuccess;
        if (!ok) return SPRS_ERR_HIP;
        keep_host(Lh.A, D.a_ip, D.a_ix, D.a_v);
        if (l + 1 < nlev) { keep_host(Lh.P, D.p_ip, D.p_ix, D.p_v); keep_host(Lh.R, D.r_ip, D.r_ix, D.r_v); D.agg = Lh.agg; }
        Lh = HLevel<T>();                                    // (the host copy lives in D now)
    }
    if (lu_n) {
        T *dl = nullptr;
        if (!dev_upload(&dl, lu.data(), lu.size())) { P->lu = dl; return SPRS_ERR_HIP; }
        P->lu = dl;
    }
    SPRS_TRY(finish_handle<T>(P));
    *out = guard.release();
    return SPRS_OK;
}

// host clock of the device set-up's stages, a diagnostic like CreateTrace and behind the same switch: with SPRS_CREATE_TRACE set,
// lap() drains the stream and books the time since the last lap; without it lap() does nothing and creation pays no drain
struct SetupClock {
    bool on;
    double *ms, t0;
    explicit SetupClock(double *stage_ms) : on(getenv("SPRS_CREATE_TRACE") != nullptr), ms(stage_ms), t0(CreateTrace::now()) {}
    int lap(sprs_ctx *c, int stage) {
        if (!on) return SPRS_OK;
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        const double t = CreateTrace::now();
        ms[stage] += t - t0; t0 = t;
        return SPRS_OK;
    }
};

}  // namespace

#include "amg_setup.hpp"

namespace {

template <class T, int OP>
void launch_op(sprs_ctx *c, const SellMat &M, const T *x, const T *y, const T *d, Real<T> omega, T *o) {
    hipLaunchKernelGGL((amg_op_kernel<T, OP>), dim3((M.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, M.dev<T>(), (int)M.n, x, y, d, omega, o);
}

template <class T>
int amg_cycle(const sprs_amg *P, const T *in, T *out) {
    using R = Real<T>;
    sprs_ctx *c = P->ctx;
    const int nlev = (int)P->lv.size();
    const int upper = std::min(P->tail, nlev - 1);           // levels [0, upper) run the multi-workgroup kernels down and up
    auto rhs_of = [&](int l) { return l == 0 ? in : (const T *)P->lv[l].b; };
    auto res_of = [&](int l) { return l == 0 ? out : (T *)P->lv[l].x2; };
    for (int l = 0; l < upper; ++l) {
        const AmgLevel &D = P->lv[l];
        const T *b = rhs_of(l);
        hipLaunchKernelGGL((amg_scale_kernel<T>), dim3((D.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, (int)D.n, b, (const T *)D.diag, (R)D.omega, (T *)D.x);
        launch_op<T, OP_RESID>(c, D.A, (const T *)D.x, b, nullptr, (R)D.omega, (T *)D.r);
        launch_op<T, OP_MUL>(c, D.R, (const T *)D.r, nullptr, nullptr, (R)D.omega, (T *)P->lv[l + 1].b);
    }
    if (P->tail < nlev) {
        hipLaunchKernelGGL((amg_tail_kernel<T>), dim3(1), dim3(BLOCK), 0, c->stream, (const TailLevel<T> *)P->tail_desc, upper, nlev - 1,
                           rhs_of(upper), res_of(upper), (const T *)P->lu);
    } else {                                                 // a coarsest level above the tail (the half-rows stop fired early): Jacobi sweeps
        const AmgLevel &D = P->lv[upper];
        const T *b = rhs_of(upper);
        T *cur = (T *)D.x, *nxt = (T *)D.r;                   // (x2 may be the result: it is written by the last sweep only)
        hipLaunchKernelGGL((amg_scale_kernel<T>), dim3((D.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, (int)D.n, b, (const T *)D.diag, (R)D.omega, cur);
        for (int s = 1; s < AMG_COARSE_SWEEPS; ++s) {
            T *dst = s == AMG_COARSE_SWEEPS - 1 ? res_of(upper) : nxt;
            launch_op<T, OP_JACOBI>(c, D.A, (const T *)cur, b, (const T *)D.diag, (R)D.omega, dst);
            nxt = cur; cur = dst;
        }
    }
    for (int l = upper - 1; l >= 0; --l) {
        const AmgLevel &D = P->lv[l];
        launch_op<T, OP_ACC>(c, D.P, (const T *)res_of(l + 1), (const T *)D.x, nullptr, (R)D.omega, (T *)D.x);
        launch_op<T, OP_JACOBI>(c, D.A, (const T *)D.x, rhs_of(l), (const T *)D.diag, (R)D.omega, res_of(l));
    }
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

template <class T>
int amg_apply_host(const sprs_amg *Pc, const T *in, size_t in_len, T *out, size_t out_len) {
    if (!Pc || !in || !out || Pc->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if (in_len != (size_t)Pc->n || out_len != (size_t)Pc->n) return SPRS_DIM_MISMATCH;
    return staged_apply<T>(Pc, in, out, [&](const T *din, T *dout) { return amg_apply<T>(Pc, din, dout); });
}

template <class T> int amg_view_check(const void *h, const sprs_csr *A, int dtype, size_t n) { return amg_check((const sprs_amg *)h, A, dtype, n); }
template <class T> int amg_view_apply(const void *h, const T *in, T *out) { return amg_apply<T>((const sprs_amg *)h, in, out); }

}  // namespace

namespace sprs {

int amg_check(const sprs_amg *P, const sprs_csr *A, int dtype, size_t n) { return applied_check(P, A, dtype, n); }

template <class T>
int amg_apply(const sprs_amg *P, const T *in, T *out) {
    if (!P || !in || !out || P->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = P->ctx;
    CtxLock lock(c);   // the level vectors are per-handle scratch
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (P->n == 0) return SPRS_OK;
    return amg_cycle<T>(P, in, out);
}
template int amg_apply<double>(const sprs_amg *, const double *, double *);
template int amg_apply<cplx>(const sprs_amg *, const cplx *, cplx *);
template int amg_apply<float>(const sprs_amg *, const float *, float *);
template int amg_apply<cplxf>(const sprs_amg *, const cplxf *, cplxf *);

template <class T>
AppliedPrec<T> amg_prec(const sprs_amg *P) { return AppliedPrec<T>{P, amg_view_check<T>, amg_view_apply<T>}; }
template AppliedPrec<double> amg_prec<double>(const sprs_amg *);
template AppliedPrec<cplx> amg_prec<cplx>(const sprs_amg *);
template AppliedPrec<float> amg_prec<float>(const sprs_amg *);
template AppliedPrec<cplxf> amg_prec<cplxf>(const sprs_amg *);

}  // namespace sprs

#define SPRS_G(...) try { __VA_ARGS__ } catch (...) { return SPRS_ERR_HIP; }

extern "C" {

// the refusals both creations share, in this order
static int amg_create_args(const sprs_csr *A, double theta, int64_t coarse_max, int64_t max_levels, sprs_amg **out, int64_t *row_out) {
    if (!A || !out) return SPRS_INVALID_ARGUMENT;
    *out = nullptr;
    if (row_out) *row_out = -1;
    SPRS_TRY(single_gpu_only(A, "sprs_amg"));   // (before the shape: a row block with a halo has more columns than rows)
    if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
    if (!(theta >= 0.0) || coarse_max < 1 || coarse_max > AMG_COARSE_LIMIT || max_levels < 1 || max_levels > AMG_MAX_LEVELS) {
        snprintf(A->ctx->err, sizeof(A->ctx->err), "sprs_amg: theta >= 0, 1 <= coarse_max <= %d and 1 <= max_levels <= %d are required",
                 AMG_COARSE_LIMIT, AMG_MAX_LEVELS);
        return SPRS_INVALID_ARGUMENT;
    }
    return SPRS_OK;
}

int sprs_amg_create(const sprs_csr *A, double theta, int64_t coarse_max, int64_t max_levels, sprs_amg **out, int64_t *row_out) {
    SPRS_G(
        SPRS_TRY(amg_create_args(A, theta, coarse_max, max_levels, out, row_out));
        switch (A->dtype) {
            case DT_D: return amg_create<double>(A, theta, coarse_max, max_levels, out, row_out);
            case DT_Z: return amg_create<cplx>(A, theta, coarse_max, max_levels, out, row_out);
            case DT_S: return amg_create<float>(A, theta, coarse_max, max_levels, out, row_out);
            case DT_C: return amg_create<cplxf>(A, theta, coarse_max, max_levels, out, row_out);
        }
        return SPRS_INVALID_ARGUMENT;)
}

int sprs_amg_create_dev(const sprs_csr *A, double theta, int64_t coarse_max, int64_t max_levels, uint64_t seed, sprs_amg **out, int64_t *row_out) {
    SPRS_G(
        SPRS_TRY(amg_create_args(A, theta, coarse_max, max_levels, out, row_out));
        switch (A->dtype) {
            case DT_D: return amg_create_dev<double>(A, theta, coarse_max, max_levels, seed, out, row_out);
            case DT_Z: return amg_create_dev<cplx>(A, theta, coarse_max, max_levels, seed, out, row_out);
            case DT_S: return amg_create_dev<float>(A, theta, coarse_max, max_levels, seed, out, row_out);
            case DT_C: return amg_create_dev<cplxf>(A, theta, coarse_max, max_levels, seed, out, row_out);
        }
        return SPRS_INVALID_ARGUMENT;)
}

int sprs_amg_setup_info(const sprs_amg *P, int64_t *setup, int64_t *rounds, size_t rounds_len) {
    if (!P || (!rounds && rounds_len)) return SPRS_INVALID_ARGUMENT;
    if (setup) *setup = P->setup;
    for (size_t l = 0; l < rounds_len; ++l) rounds[l] = l < P->lv.size() ? P->lv[l].rounds : 0;
    return SPRS_OK;
}

int sprs_amg_setup_stage_ms(const sprs_amg *P, double *ms, size_t ms_len) {
    if (!P || (!ms && ms_len)) return SPRS_INVALID_ARGUMENT;
    for (size_t s = 0; s < ms_len; ++s) ms[s] = s < (size_t)AMG_STAGES ? P->stage_ms[s] : 0.0;
    return SPRS_OK;
}

int sprs_amg_destroy(sprs_amg *P) {
    if (!P) return SPRS_OK;
    if (P->ctx) { (void)hipSetDevice(P->ctx->device); (void)hipStreamSynchronize(P->ctx->stream); }
    for (AmgLevel &D : P->lv) {
        D.A.release(); D.P.release(); D.R.release();
        for (void *p : {D.diag, D.b, D.x, D.x2, D.r, (void *)D.agg_dev}) if (p) (void)hipFree(p);
    }
    for (void *p : {P->lu, P->tail_desc, P->in_tmp, P->out_tmp}) if (p) (void)hipFree(p);
    delete P;
    return SPRS_OK;
}

int sprs_amg_info(const sprs_amg *P, int64_t *levels, int64_t *launches, int64_t *tail_level, int64_t *lu_rows) {
    if (!P) return SPRS_INVALID_ARGUMENT;
    if (levels) *levels = (int64_t)P->lv.size();
    if (launches) *launches = P->launches;
    if (tail_level) *tail_level = P->tail;
    if (lu_rows) *lu_rows = P->lu_n;
    return SPRS_OK;
}

int sprs_amg_level_info(const sprs_amg *P, int64_t level, int64_t *rows, int64_t *nnz, int64_t *p_nnz, double *omega) {
    if (!P || level < 0 || level >= (int64_t)P->lv.size()) return SPRS_INVALID_ARGUMENT;
    const AmgLevel &D = P->lv[(size_t)level];
    if (rows) *rows = D.n;
    if (nnz) *nnz = D.nnz;
    if (p_nnz) *p_nnz = D.pnnz;
    if (omega) *omega = D.omega;
    return SPRS_OK;
}

int sprs_amg_level_read(const sprs_amg *P, int64_t level, int which, int32_t *row_ptr, int32_t *col_idx, void *val, int32_t *agg) {
    if (!P || level < 0 || level >= (int64_t)P->lv.size() || which < 0 || which > 2) return SPRS_INVALID_ARGUMENT;
    const AmgLevel &D = P->lv[(size_t)level];
    if (P->setup == 1) {                                                // device-built: nothing was kept for this call
        SPRS_G(
            sprs_ctx *c = P->ctx;
            const bool last = level + 1 == (int64_t)P->lv.size();
            if (last && (which != 0 || (agg && D.n))) return SPRS_INVALID_ARGUMENT;   // the coarsest level has no P, R or aggregates
            CtxLock lock(c);
            SPRS_HIP_TRY(c, hipSetDevice(c->device));
            SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (row_ptr || col_idx || val)
                SPRS_TRY(sell_unpack_host(c, which == 0 ? D.A : which == 1 ? D.P : D.R, dtype_size(P->dtype), row_ptr, col_idx, val));
            if (agg && D.n) SPRS_HIP_TRY(c, hipMemcpy(agg, D.agg_dev, sizeof(int32_t) * (size_t)D.n, hipMemcpyDeviceToHost));
            return SPRS_OK;)
    }
    const std::vector<int32_t> &ip = which == 0 ? D.a_ip : which == 1 ? D.p_ip : D.r_ip, &ix = which == 0 ? D.a_ix : which == 1 ? D.p_ix : D.r_ix;
    const std::vector<char> &v = which == 0 ? D.a_v : which == 1 ? D.p_v : D.r_v;
    if (which != 0 && ip.empty()) return SPRS_INVALID_ARGUMENT;       // the coarsest level has no P, R or aggregates
    if (row_ptr) memcpy(row_ptr, ip.data(), sizeof(int32_t) * ip.size());
    if (col_idx && !ix.empty()) memcpy(col_idx, ix.data(), sizeof(int32_t) * ix.size());
    if (val && !v.empty()) memcpy(val, v.data(), v.size());
    if (agg) {
        if (D.agg.empty() && D.n && level + 1 == (int64_t)P->lv.size()) return SPRS_INVALID_ARGUMENT;
        if (!D.agg.empty()) memcpy(agg, D.agg.data(), sizeof(int32_t) * D.agg.size());
    }
    return SPRS_OK;
}

#define SPRS_AMG_API(X, T, CT)                                                                                          \
    int sprs_amg_mul_vec_dev_##X(const sprs_amg *P, const CT *in, CT *out) {                                            \
        SPRS_G(return amg_apply<T>(P, (const T *)in, (T *)out);)                                                        \
    }                                                                                                                   \
    int sprs_amg_mul_vec_##X(const sprs_amg *P, const CT *in, size_t il, CT *out, size_t ol) {                          \
        SPRS_G(return amg_apply_host<T>(P, (const T *)in, il, (T *)out, ol);)                                           \
    }
SPRS_AMG_API(d, double, double)
SPRS_AMG_API(z, cplx, sprs_c64)
SPRS_AMG_API(s, float, float)
SPRS_AMG_API(c, cplxf, sprs_c32)

}  // extern "C"
