// extern "C" surface of libsprsolve_hip.so — see include/sprsolve_hip.h for the contract and
// the reference interface each entry point replaces.  Nothing here throws.
#include <sys/mman.h>

#include <cstdlib>
#include <memory>
#include <new>
#include <string>

#include "krylov.hpp"

using namespace sprs;

static_assert(sizeof(sprs_c64) == sizeof(cplx), "Complex<f64> layout");
static_assert(sizeof(sprs_c32) == sizeof(cplxf), "Complex<f32> layout");

#define SPRS_GUARD_BEGIN try {
#define SPRS_GUARD_END                         \
    }                                          \
    catch (const std::bad_alloc &) {           \
        return SPRS_ERR_HIP;                   \
    }                                          \
    catch (...) {                              \
        return SPRS_ERR_HIP;                   \
    }

// ------------------------------------------------------------------------------ knobs
// sprs_ctx_set / sprs_ctx_get: every knob once.  What a set stores: TRI -1 (any negative) / 0 / 1 (any other); BOOL 0 / 1; INT a value
// of lo .. hi, anything else refused, rounded down to a multiple of 8 where round8; AUTO_OR_INT -1 for any negative, else as INT;
// AT_LEAST the value, raised to lo; GET_ONLY is refused.
namespace {
struct Knob {
    const char *name;
    int sprs_ctx::*field;
    enum Kind { TRI, BOOL, INT, AUTO_OR_INT, AT_LEAST, GET_ONLY } kind;
    int64_t lo, hi;
    bool round8;
};
const Knob KNOBS[] = {
    {"grid", &sprs_ctx::grid, Knob::INT, 8, MAX_GRID, true},
    {"spmv_grid", &sprs_ctx::spmv_grid, Knob::AUTO_OR_INT, 8, MAX_GRID / 2, true},
    {"xcd_chunk", &sprs_ctx::xcd_chunk, Knob::TRI, 0, 0, false},
    {"spmv_dict", &sprs_ctx::spmv_dict, Knob::INT, -1, 2, false},
    {"spmv_wide", &sprs_ctx::spmv_wide, Knob::TRI, 0, 0, false},
    {"spmv_uniform", &sprs_ctx::spmv_uniform, Knob::TRI, 0, 0, false},
    {"spmv_period", &sprs_ctx::spmv_period, Knob::TRI, 0, 0, false},
    {"spmv_triple", &sprs_ctx::spmv_triple, Knob::TRI, 0, 0, false},
    {"spmv_seam", &sprs_ctx::spmv_seam, Knob::TRI, 0, 0, false},
    {"spmv_tile", &sprs_ctx::spmv_tile, Knob::TRI, 0, 0, false},
    {"spmv_chain", &sprs_ctx::spmv_chain, Knob::TRI, 0, 0, false},
    {"spmv_fuse", &sprs_ctx::spmv_fuse, Knob::TRI, 0, 0, false},
    {"bicg_k5", &sprs_ctx::bicg_k5, Knob::AUTO_OR_INT, 0, 2, false},
    {"p2p_allreduce", &sprs_ctx::p2p_allreduce, Knob::TRI, 0, 0, false},
    {"p2p_timeout_ms", &sprs_ctx::p2p_timeout_ms, Knob::AT_LEAST, 1, 0, false},
    {"ew_chunk", &sprs_ctx::ew_chunk, Knob::TRI, 0, 0, false},
    {"stream_nt", &sprs_ctx::stream_nt, Knob::TRI, 0, 0, false},
    {"spmv_eqrows", &sprs_ctx::spmv_eqrows, Knob::TRI, 0, 0, false},
    {"spmv_wideload", &sprs_ctx::spmv_wideload, Knob::TRI, 0, 0, false},
    {"halo_overlap", &sprs_ctx::halo_overlap, Knob::BOOL, 0, 0, false},
    {"gs_graph", &sprs_ctx::gs_graph, Knob::BOOL, 0, 0, false},
    {"poll", &sprs_ctx::poll, Knob::INT, 1, INT64_MAX, false},
    {"num_cu", &sprs_ctx::num_cu, Knob::GET_ONLY, 0, 0, false},
    {"device", &sprs_ctx::device, Knob::GET_ONLY, 0, 0, false},
};
const Knob *find_knob(const char *key) {
    for (const Knob &k : KNOBS)
        if (strcmp(k.name, key) == 0) return &k;
    return nullptr;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ context
int sprs_version(void) { return 100; }

const char *sprs_status_str(int s) {
    switch (s) {
        case SPRS_OK: return "Ok";
        case SPRS_INCOMPATIBLE_RHS_SIZE: return "Incompatible input matrix format: Input vec dimension doesn't match the matrix size";
        case SPRS_INCOMPATIBLE_X_SIZE: return "Incompatible input matrix format: Input and output vec dimension do not match";
        case SPRS_INSUFFICIENT_ITER: return "Insufficient interation #";
        case SPRS_BREAKDOWN: return "Solver break down";
        case SPRS_INVALID_PRECOND: return "Invalid preconditioner";
        case SPRS_DIM_MISMATCH: return "Dimension mismatch";
        case SPRS_INVALID_ARGUMENT: return "Invalid argument";
        case SPRS_ZERO_DIAGONAL: return "Matrix has zero diagonal element";
        case SPRS_NOT_SQUARE: return "Incompatible input matrix format: Not a square matrix";
        case SPRS_NOT_CSR: return "Incompatible input matrix format: Not in CSR format";
        case SPRS_ERR_HIP: return "HIP runtime error";
        case SPRS_ERR_RCCL: return "RCCL error";
        case SPRS_ERR_NO_DEVICE: return "No usable GPU device";
        default: return "Unknown status";
    }
}

int sprs_ctx_create(int device, void *stream, sprs_ctx **out) {
    SPRS_GUARD_BEGIN
    if (!out) return SPRS_INVALID_ARGUMENT;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SPRS_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return SPRS_ERR_NO_DEVICE;
    sprs_ctx *c = new sprs_ctx();
    c->device = device;
    auto fail = [&](int st) { delete c; return st; };
    if (hipSetDevice(device) != hipSuccess) return fail(SPRS_ERR_NO_DEVICE);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return fail(SPRS_ERR_HIP);
        c->own_stream = true;
    }
    // 4 workgroups of 256 lanes per CU: enough loads in flight to saturate HBM while the
    // number of reduction partials (== grid) stays small enough for the fused prologues
    // streaming / reduction kernels: 2 workgroups per CU (measured on the cfg-5 solve: 256 -> 1.99, 384 -> 1.90,
    // 512 -> 1.86, 768 -> 1.86, 1024 -> 2.00, 2048 -> 2.06 ms per BiCGStab iteration; profiles/r01_tuning.md)
    c->grid = ((c->num_cu * 2 + 7) / 8) * 8;
    if (c->grid > MAX_GRID) c->grid = MAX_GRID;
    if (hipMalloc((void **)&c->d_part, sizeof(double) * 2 * MAX_GRID) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipMalloc((void **)&c->d_scal, 256) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipHostMalloc((void **)&c->h_scal, 256, hipHostMallocDefault) != hipSuccess) return fail(SPRS_ERR_HIP);
    *out = c;
    return SPRS_OK;
    SPRS_GUARD_END
}

int sprs_ctx_destroy(sprs_ctx *c) {
    if (!c) return SPRS_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->d_part) (void)hipFree(c->d_part);
    if (c->d_scal) (void)hipFree(c->d_scal);
    if (c->h_scal) (void)hipHostFree(c->h_scal);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return SPRS_OK;
}

int sprs_ctx_sync(sprs_ctx *c) {
    if (!c) return SPRS_INVALID_ARGUMENT;
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

const char *sprs_last_error(const sprs_ctx *c) { return c ? c->err : "null context"; }

int sprs_ctx_set(sprs_ctx *c, const char *key, int64_t value) {
    if (!c || !key) return SPRS_INVALID_ARGUMENT;
    const Knob *k = find_knob(key);
    if (!k) return SPRS_INVALID_ARGUMENT;
    switch (k->kind) {
        case Knob::GET_ONLY: return SPRS_INVALID_ARGUMENT;
        case Knob::TRI: value = value < 0 ? -1 : (value ? 1 : 0); break;
        case Knob::BOOL: value = value ? 1 : 0; break;
        case Knob::AT_LEAST: value = std::max(value, k->lo); break;
        case Knob::AUTO_OR_INT:
        case Knob::INT:
            if (k->kind == Knob::AUTO_OR_INT && value < 0) { value = -1; break; }
            if (value < k->lo || value > k->hi) return SPRS_INVALID_ARGUMENT;
            if (k->round8) value &= ~(int64_t)7;
            break;
    }
    c->*(k->field) = (int)value;
    return SPRS_OK;
}
int64_t sprs_ctx_get(const sprs_ctx *c, const char *key) {
    if (!c || !key) return -1;
    const Knob *k = find_knob(key);
    return k ? c->*(k->field) : -1;
}

int sprs_malloc(sprs_ctx *c, size_t bytes, void **dev_out) {
    if (!c || !dev_out) return SPRS_INVALID_ARGUMENT;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    SPRS_HIP_TRY(c, hipMalloc(dev_out, bytes ? bytes : 16));
    return SPRS_OK;
}
int sprs_free(sprs_ctx *c, void *dev) {
    if (!c) return SPRS_INVALID_ARGUMENT;
    if (!dev) return SPRS_OK;
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    SPRS_HIP_TRY(c, hipFree(dev));
    return SPRS_OK;
}
int sprs_memcpy_h2d(sprs_ctx *c, void *d, const void *h, size_t bytes) {
    if (!c) return SPRS_INVALID_ARGUMENT;
    SPRS_HIP_TRY(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}
int sprs_memcpy_d2h(sprs_ctx *c, void *h, const void *d, size_t bytes) {
    if (!c) return SPRS_INVALID_ARGUMENT;
    SPRS_HIP_TRY(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}
int sprs_memcpy_d2d(sprs_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return SPRS_INVALID_ARGUMENT;
    SPRS_HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return SPRS_OK;
}
int sprs_memset_zero(sprs_ctx *c, void *d, size_t bytes) {
    if (!c) return SPRS_INVALID_ARGUMENT;
    SPRS_HIP_TRY(c, hipMemsetAsync(d, 0, bytes, c->stream));
    return SPRS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------ CSR operator
namespace {

template <class I>
bool narrow_check(const I *a, int64_t n, int64_t lo, int64_t hi) {
    for (int64_t i = 0; i < n; ++i)
        if ((int64_t)a[i] < lo || (int64_t)a[i] > hi) return false;
    return true;
}

// Build the device CSR from host arrays (CSR or CSC, any integer index type).
template <class T, class I>
int csr_create_host(sprs_ctx *c, int64_t nrows, int64_t ncols, int64_t nnz, const I *ptr, const I *idx, const T *val,
                    int storage_csc, sprs_csr **out) {
    if (!c || !out || nrows < 0 || ncols < 0 || nnz < 0) return SPRS_INVALID_ARGUMENT;
    if (!ptr || (nnz > 0 && (!idx || !val))) return SPRS_INVALID_ARGUMENT;
    CtxLock lock(c);
    *out = nullptr;
    if (nrows >= INT32_MAX || ncols >= INT32_MAX || nnz >= INT32_MAX) return SPRS_INVALID_ARGUMENT;
    const int64_t nouter = storage_csc ? ncols : nrows, ninner = storage_csc ? nrows : ncols;
    // validate: the kernels index x and y with these arrays
    if ((int64_t)ptr[0] != 0 || (int64_t)ptr[nouter] != nnz) return SPRS_INVALID_ARGUMENT;
    for (int64_t i = 0; i < nouter; ++i)
        if ((int64_t)ptr[i + 1] < (int64_t)ptr[i]) return SPRS_INVALID_ARGUMENT;
    if (!narrow_check(idx, nnz, 0, ninner - 1)) return SPRS_INVALID_ARGUMENT;

    std::vector<int32_t> rp((size_t)nrows + 1), ci((size_t)nnz);
    std::vector<T> vv;
    const T *vsrc = val;
    if (!storage_csc) {
        for (int64_t i = 0; i <= nrows; ++i) rp[i] = (int32_t)ptr[i];
        for (int64_t k = 0; k < nnz; ++k) ci[k] = (int32_t)idx[k];
    } else {
        // CSC -> CSR, stable in column order: per row the terms keep the order in which the
        // reference's serial scatter (mat.rs:135-141) adds them, so y has the same bits.
        vv.resize((size_t)nnz);
        std::fill(rp.begin(), rp.end(), 0);
        for (int64_t k = 0; k < nnz; ++k) rp[(size_t)idx[k] + 1]++;
        for (int64_t i = 0; i < nrows; ++i) rp[i + 1] += rp[i];
        std::vector<int32_t> fill(rp.begin(), rp.end() - 1);
        for (int64_t col = 0; col < ncols; ++col)
            for (int64_t k = (int64_t)ptr[col]; k < (int64_t)ptr[col + 1]; ++k) {
                int32_t dst = fill[(size_t)idx[k]]++;
                ci[dst] = (int32_t)col;
                vv[dst] = val[k];
            }
        vsrc = vv.data();
    }
    sprs_csr *A = new sprs_csr();
    A->ctx = c; A->dtype = dtype_of<T>::value;
    A->nrows = nrows; A->ncols = ncols; A->nnz = nnz; A->owns_arrays = true; A->was_csc = storage_csc != 0;
    auto fail = [&](int st) { sprs_csr_destroy(A); return st; };
    if (hipSetDevice(c->device) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipMalloc((void **)&A->row_ptr, sizeof(int32_t) * ((size_t)nrows + 1)) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipMalloc((void **)&A->col_idx, sizeof(int32_t) * (size_t)(nnz ? nnz : 1)) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipMalloc((void **)&A->val, sizeof(T) * (size_t)(nnz ? nnz : 1)) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipMemcpyAsync(A->row_ptr, rp.data(), sizeof(int32_t) * ((size_t)nrows + 1), hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (nnz) {
        if (hipMemcpyAsync(A->col_idx, ci.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
        if (hipMemcpyAsync(A->val, vsrc, sizeof(T) * (size_t)nnz, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    int st = build_rowblocks(A, rp.data());
    if (st != SPRS_OK) return fail(st);
    *out = A;
    return SPRS_OK;
}

template <class T>
int csr_create_dev(sprs_ctx *c, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *d_rp, const int32_t *d_ci,
                   const T *d_val, int adopt, sprs_csr **out) {
    if (!c || !out || !d_rp || nrows < 0 || ncols < 0 || nnz < 0) return SPRS_INVALID_ARGUMENT;
    if (nnz > 0 && (!d_ci || !d_val)) return SPRS_INVALID_ARGUMENT;
    CtxLock lock(c);
    *out = nullptr;
    if (nrows >= INT32_MAX || ncols >= INT32_MAX || nnz >= INT32_MAX) return SPRS_INVALID_ARGUMENT;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    CreateTrace tr;
    // row_ptr stays in HBM: build_rowblocks validates it (and copies it to the host only for irregular matrices)
    sprs_csr *A = new sprs_csr();
    A->ctx = c; A->dtype = dtype_of<T>::value;
    A->nrows = nrows; A->ncols = ncols; A->nnz = nnz;
    auto fail = [&](int st) { sprs_csr_destroy(A); return st; };
    if (adopt) {
        A->owns_arrays = false;
        A->row_ptr = const_cast<int32_t *>(d_rp); A->col_idx = const_cast<int32_t *>(d_ci);
        A->val = const_cast<T *>(d_val);
    } else {
        A->owns_arrays = true;
        if (hipMalloc((void **)&A->row_ptr, sizeof(int32_t) * ((size_t)nrows + 1)) != hipSuccess) return fail(SPRS_ERR_HIP);
        if (hipMalloc((void **)&A->col_idx, sizeof(int32_t) * (size_t)(nnz ? nnz : 1)) != hipSuccess) return fail(SPRS_ERR_HIP);
        if (hipMalloc((void **)&A->val, sizeof(T) * (size_t)(nnz ? nnz : 1)) != hipSuccess) return fail(SPRS_ERR_HIP);
        if (hipMemcpyAsync(A->row_ptr, d_rp, sizeof(int32_t) * ((size_t)nrows + 1), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
        if (nnz) {
            if (hipMemcpyAsync(A->col_idx, d_ci, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
            if (hipMemcpyAsync(A->val, d_val, sizeof(T) * (size_t)nnz, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    }
    int st = validate_cols_device(A);
    if (st != SPRS_OK) return fail(st);
    tr.lap("column range check (device)");
    st = build_rowblocks(A, nullptr);
    if (st != SPRS_OK) return fail(st);
    tr.lap("build_rowblocks total");
    *out = A;
    return SPRS_OK;
}

template <class T>
int ensure_tmp(const sprs_csr *Ac) {
    sprs_csr *A = const_cast<sprs_csr *>(Ac);
    sprs_ctx *c = A->ctx;
    const size_t m = (size_t)(A->nrows > A->ncols ? A->nrows : A->ncols) + 2;
    if (!A->x_tmp) SPRS_HIP_TRY(c, hipMalloc(&A->x_tmp, sizeof(T) * m));
    if (!A->y_tmp) SPRS_HIP_TRY(c, hipMalloc(&A->y_tmp, sizeof(T) * m));
    if (!A->part) SPRS_HIP_TRY(c, hipMalloc((void **)&A->part, sizeof(double) * 2 * MAX_GRID));
    return SPRS_OK;
}

// MatVecMul::mul_vec / mul_vec_dot over host slices (mat.rs:49-64)
template <class T>
int mul_vec_host(const sprs_csr *A, const T *x, size_t x_len, T *y, size_t y_len, T *dot_out) {
    if (!A || !x || !y) return SPRS_INVALID_ARGUMENT;
    if (A->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if ((size_t)A->ncols != x_len || x_len != y_len) return SPRS_DIM_MISMATCH;   // mat.rs:50-52
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);   // x_tmp / y_tmp / part are per-handle staging: `&self` calls from several threads queue here
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    SPRS_TRY(ensure_tmp<T>(A));
    T *dx = (T *)A->x_tmp, *dy = (T *)A->y_tmp;
    SPRS_HIP_TRY(c, hipMemcpyAsync(dx, x, sizeof(T) * x_len, hipMemcpyHostToDevice, c->stream));
    T *part = (T *)A->part;
    SPRS_TRY(launch_spmv<T>(A, SpmvPart::Whole, dx, dy, dot_out ? 1 : 0, dx, part, nullptr, nullptr));
    const size_t ncopy = (size_t)A->nrows < y_len ? (size_t)A->nrows : y_len;
    SPRS_HIP_TRY(c, hipMemcpyAsync(y, dy, sizeof(T) * ncopy, hipMemcpyDeviceToHost, c->stream));
    if (dot_out) SPRS_TRY(reduce_partials_host<T>(c, part, spmv_num_partials(A), dot_out));   // mat.rs:151
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
int mul_vec_dev(const sprs_csr *A, const T *dx, T *dy, T *dot_out) {
    if (!A || !dx || !dy) return SPRS_INVALID_ARGUMENT;
    if (A->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (!dot_out) return launch_spmv<T>(A, SpmvPart::Whole, dx, dy, 0, nullptr, nullptr, nullptr, nullptr);
    SPRS_TRY(ensure_tmp<T>(A));
    T *part = (T *)A->part;
    SPRS_TRY(launch_spmv<T>(A, SpmvPart::Whole, dx, dy, 1, dx, part, nullptr, nullptr));
    return reduce_partials_host<T>(c, part, spmv_num_partials(A), dot_out);
}

// Y = A X for a row-major block of k <= 8 vectors (spmm.hip)
template <class T>
int mul_mat_dev(const sprs_csr *A, const T *dx, T *dy, size_t k) {
    if (!A || !dx || !dy) return SPRS_INVALID_ARGUMENT;
    if (A->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if (k < 1 || k > 8) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_TRY(single_gpu_only(A, "sprs_mul_mat"));
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    return launch_spmm<T>(A, dx, dy, (int)k, (int)k, 0, nullptr, nullptr, nullptr);
}

template <class T>
int mul_mat_host(const sprs_csr *A, const T *x, size_t x_len, T *y, size_t y_len, size_t k) {
    if (!A || !x || !y) return SPRS_INVALID_ARGUMENT;
    if (A->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if (k < 1 || k > 8) return SPRS_INVALID_ARGUMENT;
    if ((size_t)A->ncols * k != x_len || (size_t)A->nrows * k != y_len) return SPRS_DIM_MISMATCH;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_TRY(single_gpu_only(A, "sprs_mul_mat"));
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    T *dx = nullptr, *dy = nullptr;
    struct Free { T *&a, *&b; ~Free() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); } } guard{dx, dy};   // every return path
    SPRS_HIP_TRY(c, hipMalloc((void **)&dx, sizeof(T) * (x_len ? x_len : 1)));
    SPRS_HIP_TRY(c, hipMalloc((void **)&dy, sizeof(T) * (y_len ? y_len : 1)));
    SPRS_HIP_TRY(c, hipMemcpyAsync(dx, x, sizeof(T) * x_len, hipMemcpyHostToDevice, c->stream));
    SPRS_TRY(launch_spmm<T>(A, dx, dy, (int)k, (int)k, 0, nullptr, nullptr, nullptr));
    SPRS_HIP_TRY(c, hipMemcpyAsync(y, dy, sizeof(T) * y_len, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
int mul_vec_timed(const sprs_csr *A, const T *dx, T *dy, int reps, double *ms) {
    if (!A || !dx || !dy || !ms || reps < 1) return SPRS_INVALID_ARGUMENT;
    if (A->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = A->ctx;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    CtxLock lock(c);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Ev { hipEvent_t &a, &b; ~Ev() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } guard{e0, e1};   // every return path
    SPRS_HIP_TRY(c, hipEventCreate(&e0));
    SPRS_HIP_TRY(c, hipEventCreate(&e1));
    SPRS_HIP_TRY(c, hipEventRecord(e0, c->stream));
    for (int i = 0; i < reps; ++i) SPRS_TRY(launch_spmv<T>(A, SpmvPart::Whole, dx, dy, 0, nullptr, nullptr, nullptr, nullptr));
    SPRS_HIP_TRY(c, hipEventRecord(e1, c->stream));
    SPRS_HIP_TRY(c, hipEventSynchronize(e1));
    float t = 0.f;
    SPRS_HIP_TRY(c, hipEventElapsedTime(&t, e0, e1));
    *ms = (double)t / reps;
    return SPRS_OK;
}

}  // namespace

// ------------------------------------------------------------------------------ Jacobi preconditioner
namespace {
template <class V>
int diag_create(sprs_ctx *c, size_t n, const V *diag_host, int t_dtype, sprs_diag **out) {
    if (!c || !out || (!diag_host && n)) return SPRS_INVALID_ARGUMENT;
    CtxLock lock(c);
    *out = nullptr;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    sprs_diag *P = new sprs_diag();
    P->ctx = c; P->n = n; P->t_dtype = t_dtype; P->v_complex = is_complex<V>::value ? 1 : 0;
    auto fail = [&](int st) { sprs_diag_precond_destroy(P); return st; };
    V *tmp = nullptr;
    const size_t np = ((n + 31) & ~(size_t)31) + 32;
    if (hipMalloc(&P->dinv, sizeof(V) * np) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipMalloc((void **)&tmp, sizeof(V) * np) != hipSuccess) return fail(SPRS_ERR_HIP);
    int st = SPRS_OK;
    if (hipMemcpyAsync(tmp, diag_host, sizeof(V) * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) st = SPRS_ERR_HIP;
    if (st == SPRS_OK) st = launch_diag_inv<V>(c, n, tmp, (V *)P->dinv);   // precond.rs:22-24
    if (st == SPRS_OK && hipStreamSynchronize(c->stream) != hipSuccess) st = SPRS_ERR_HIP;
    (void)hipFree(tmp);
    if (st != SPRS_OK) return fail(st);
    *out = P;
    return SPRS_OK;
}

template <class T>
int diag_apply_dev(const sprs_diag *P, const T *in, T *out) {
    if (!P || !in || !out) return SPRS_INVALID_ARGUMENT;
    if (P->t_dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if (P->v_complex) {
        if constexpr (is_complex<T>::value) return launch_diag_apply<T, T>(P->ctx, P->n, (const T *)P->dinv, in, out);
        else return SPRS_INVALID_ARGUMENT;
    }
    return launch_diag_apply<T, Real<T>>(P->ctx, P->n, (const Real<T> *)P->dinv, in, out);
}

template <class T>
int diag_apply_host(const sprs_diag *Pc, const T *in, size_t in_len, T *out, size_t out_len) {
    if (!Pc || !in || !out) return SPRS_INVALID_ARGUMENT;
    if (Pc->n != in_len || Pc->n != out_len) return SPRS_DIM_MISMATCH;     // precond.rs:39-41
    return staged_apply<T>(Pc, in, out, [&](const T *din, T *dout) { return diag_apply_dev<T>(Pc, din, dout); });
}

// ------------------------------------------------------------------------------ solver handles
// one opaque handle layout for every solver kind: sprs_solver_handle { dtype, impl }
template <template <class> class S, class F>
int with_solver(int dtype, void *impl, F &&f) {
    switch (dtype) {
        case DT_D: return f((S<double> *)impl);
        case DT_Z: return f((S<cplx> *)impl);
        case DT_S: return f((S<float> *)impl);
        case DT_C: return f((S<cplxf> *)impl);
    }
    return SPRS_INVALID_ARGUMENT;
}

// The one way a solver handle of any kind comes to be.  This holds what belongs to the ABI: the null checks, *out zeroed, the
// handle's scalar type against T, the context lock (the allocations go to the context's stream; recursive, so Lsmr / Svds::create
// -> sprs_csr_adjoint take it again), an S<T> behind an H, and the unwind.  mk(s) is S<T>::create, which holds every check of the
// operator and of the creation parameters (krylov.hpp).  entry: "sprs_<name>", as the refusals' texts begin.
template <class T, class H, template <class> class S, class Mk>
int solver_create(const char *entry, const sprs_csr *A, H **out, Mk mk) {
    if (out) *out = nullptr;
    if (!A || !out) return SPRS_INVALID_ARGUMENT;
    if (A->dtype != dtype_of<T>::value) return refuse(A->ctx, entry, "the operator holds another scalar type");
    CtxLock lock(A->ctx);
    H *h = new H();
    h->dtype = dtype_of<T>::value;
    auto *s = new S<T>();
    h->impl = s;
    const int st = mk(s);
    if (st != SPRS_OK) { s->destroy(); delete s; delete h; return st; }
    *out = h;
    return SPRS_OK;
}

template <template <class> class S>
int solver_destroy(sprs_solver_handle *h) {
    if (!h) return SPRS_OK;
    with_solver<S>(h->dtype, h->impl, [](auto *s) { (void)hipStreamSynchronize(s->ctx->stream); s->destroy(); delete s; return (int)SPRS_OK; });
    delete h;
    return SPRS_OK;
}

// Where one solve's vectors live.  Host slices (host = true), and device vectors that are not 16-byte aligned, go through the
// solver's aligned rhs_buf / x_buf of rcap / xcap entries; other device vectors are used in place.  run(rhs, x) is
// SolverT::solve_dev on the pointers chosen.  The callers have checked rl and xl: nothing is copied on a mismatch.
template <class T, class SolverT, class Run>
int staged_solve(SolverT *s, bool host, const T *rhs, size_t rl, size_t rcap, T *x, size_t xl, size_t xcap, Run run) {
    sprs_ctx *c = s->ctx;
    CtxLock lock(c);   // one solve at a time per context (its stream, its scratch)
    if (!host && ((reinterpret_cast<uintptr_t>(rhs) | reinterpret_cast<uintptr_t>(x)) & 15) == 0) return run(rhs, x);
    const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (!s->rhs_buf) SPRS_HIP_TRY(c, hipMalloc((void **)&s->rhs_buf, sizeof(T) * rcap));
    if (!s->x_buf) SPRS_HIP_TRY(c, hipMalloc((void **)&s->x_buf, sizeof(T) * xcap));
    SPRS_HIP_TRY(c, hipMemcpyAsync(s->rhs_buf, rhs, sizeof(T) * rl, in, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(s->x_buf, x, sizeof(T) * xl, in, c->stream));
    const int st = run((const T *)s->rhs_buf, s->x_buf);
    if (st >= SPRS_ERR_HIP) return st;
    // x is in/out in the reference and is left modified on Err as well: it is copied back on a solver event too
    SPRS_HIP_TRY(c, hipMemcpyAsync(x, s->x_buf, sizeof(T) * xl, out, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return st;
}

// One solve of a square system.  P: what SolverT::solve_dev takes — a sprs_diag (or null), or an ILU(0), AMG or FSAI handle's
// AppliedPrec view (sprs_ilu0_cg_*, sprs_amg_bicgstab_*, ...).
template <class T, class SolverT, class P>
int solve(SolverT *s, bool host, const P &prec, const T *rhs, size_t rl, T *x, size_t xl, size_t max_iter, Real<T> tol,
          size_t *its, Real<T> *res) {
    const Precond<T> M(prec);
    if (!s || (M.is_applied && !M.applied.h) || !rhs || !x) return SPRS_INVALID_ARGUMENT;
    // size checks first (bicg_stab.rs:44-53): nothing is copied on a mismatch, nor where an applied handle is refused
    if (rl != s->n) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (xl != s->n) return SPRS_INCOMPATIBLE_X_SIZE;
    if (M.is_applied) SPRS_TRY(M.applied.check(s->A, s->n));
    return staged_solve<T>(s, host, rhs, rl, s->stride, x, xl, s->stride,
                           [&](const T *b, T *y) { return s->solve_dev(prec, b, rl, y, xl, max_iter, tol, its, res); });
}

// One LSMR solve: rhs of nrows, x of ncols entries.
template <class T>
int lsmr_solve(Lsmr<T> *s, bool host, const T *rhs, size_t rl, T *x, size_t xl, Real<T> damp, size_t max_iter, Real<T> tol, size_t *its,
               Real<T> *res, Real<T> *ares) {
    if (!s || !rhs || !x) return SPRS_INVALID_ARGUMENT;
    if (rl != s->m || xl != s->nc) return SPRS_DIM_MISMATCH;
    if (!(damp >= (Real<T>)0)) return SPRS_INVALID_ARGUMENT;
    return staged_solve<T>(s, host, rhs, rl, s->stride, x, xl, s->stride_n,
                           [&](const T *b, T *y) { return s->solve_dev(b, rl, y, xl, damp, max_iter, tol, its, res, ares); });
}

// One batched CG solve (n x k row-major blocks).  Host slices go through the solver's staging buffers; device blocks are
// read and written in place (the solver copies them into its padded work blocks, so no alignment is asked of them).
// Apart from staged_solve: no alignment test, one capacity of n kmax + 1, and argument statuses that skip the copy-back too.
template <class T>
int solve_many(CgMany<T> *s, bool host, const sprs_diag *P, const T *rhs, size_t rl, T *x, size_t xl, size_t k, size_t max_iter,
               Real<T> tol, size_t *its, Real<T> *res, int *status) {
    if (!s || !rhs || !x) return SPRS_INVALID_ARGUMENT;
    if (k < 1 || k > (size_t)s->kmax) return SPRS_INVALID_ARGUMENT;
    if (rl != s->n * k) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (xl != s->n * k) return SPRS_INCOMPATIBLE_X_SIZE;
    sprs_ctx *c = s->ctx;
    CtxLock lock(c);
    if (!host) return s->solve_dev(P, rhs, rl, x, xl, k, max_iter, tol, its, res, status);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    const size_t cap = (s->n * (size_t)s->kmax) + 1;
    if (!s->rhs_buf) SPRS_HIP_TRY(c, hipMalloc((void **)&s->rhs_buf, sizeof(T) * cap));
    if (!s->x_buf) SPRS_HIP_TRY(c, hipMalloc((void **)&s->x_buf, sizeof(T) * cap));
    SPRS_HIP_TRY(c, hipMemcpyAsync(s->rhs_buf, rhs, sizeof(T) * rl, hipMemcpyHostToDevice, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(s->x_buf, x, sizeof(T) * xl, hipMemcpyHostToDevice, c->stream));
    int st = s->solve_dev(P, s->rhs_buf, rl, s->x_buf, xl, k, max_iter, tol, its, res, status);
    if (st >= SPRS_ERR_HIP || st == SPRS_DIM_MISMATCH || st == SPRS_INVALID_ARGUMENT) return st;
    SPRS_HIP_TRY(c, hipMemcpyAsync(x, s->x_buf, sizeof(T) * xl, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return st;
}

// One multi-shift CG solve.  rhs (n entries) is copied into the solver's residual and x (m contiguous vectors of n, output only)
// is written in place where it is an aligned device block, else copied out of the solver's own: nothing is staged here.
template <class T>
int solve_shift(CgShift<T> *s, bool host, const Real<T> *shifts, size_t m, const T *rhs, size_t rl, T *x, size_t xl, size_t max_iter,
                Real<T> tol, size_t *its, Real<T> *res, int *status) {
    if (!s || !rhs || !x) return SPRS_INVALID_ARGUMENT;
    return s->solve(shifts, m, rhs, rl, host, x, xl, max_iter, tol, its, res, status);
}

// a caller's out-pointer, or a slot of the entry point's own where it is null
template <class V>
V *or_dummy(V *p, V *slot) { return p ? p : slot; }

// One eigensolve.  v0 is copied into the basis and the vectors are written by the rotation kernel (device) or copied out of
// the basis (host), so no alignment is asked of either.
template <class T>
int eigsh_solve(Eigsh<T> *s, bool host, size_t k, int which, const T *v0, size_t v0_len, size_t max_restarts, Real<T> tol, Real<T> *vals,
                T *vecs, size_t vecs_len, Real<T> *res, size_t *nconv, size_t *restarts, size_t *matvecs) {
    if (!s || !v0 || !vals || !res) return SPRS_INVALID_ARGUMENT;
    if (k < 1 || k + 2 > (size_t)s->m || (which != SPRS_EIGSH_LARGEST && which != SPRS_EIGSH_SMALLEST) || max_restarts < 1)
        return SPRS_INVALID_ARGUMENT;
    if (v0_len != s->n) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (vecs && vecs_len != k * s->n) return SPRS_INCOMPATIBLE_X_SIZE;
    size_t d[3];
    CtxLock lock(s->ctx);
    return s->solve(k, which, v0, host, max_restarts, tol, vals, vecs, host, res, or_dummy(nconv, d), or_dummy(restarts, d + 1), or_dummy(matvecs, d + 2));
}

// One propagation.  v is copied into the basis and w is written by the combination kernel (an aligned device w) or copied out of
// the staging vector, so no alignment is asked of either and w may be v.
template <class T>
int expm_apply(Expm<T> *s, bool host, Real<T> t, const T *v, size_t v_len, Real<T> tol, size_t max_steps, Real<T> tau0, T *w, size_t w_len,
               Real<T> *err, Real<T> *hump, Real<T> *t_done, size_t *steps, size_t *rejects, size_t *matvecs) {
    if (!s || !v || !w) return SPRS_INVALID_ARGUMENT;
    if (!std::isfinite(t) || !(tol >= Real<T>(0)) || !std::isfinite(tol) || !(tau0 >= Real<T>(0)) || !std::isfinite(tau0) || max_steps < 1)
        return SPRS_INVALID_ARGUMENT;
    if (v_len != s->n) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (w_len != s->n) return SPRS_INCOMPATIBLE_X_SIZE;
    size_t d[3];
    Real<T> rd[3];
    CtxLock lock(s->ctx);
    return s->apply(t, v, host, tol, max_steps, tau0, w, or_dummy(err, rd), or_dummy(hump, rd + 1), or_dummy(t_done, rd + 2), or_dummy(steps, d),
                    or_dummy(rejects, d + 1), or_dummy(matvecs, d + 2));
}

// One truncated SVD.  v0 is copied into the basis and the vectors are written by the rotation kernel (device) or copied out of
// the bases (host), so no alignment is asked of either.
template <class T>
int svds_solve(Svds<T> *s, bool host, size_t k, int which, const T *v0, size_t v0_len, size_t max_restarts, Real<T> tol, Real<T> *vals, T *u,
               size_t u_len, T *v, size_t v_len, Real<T> *res, size_t *nconv, size_t *restarts, size_t *matvecs) {
    if (!s || !v0 || !vals || !res || (u == nullptr) != (v == nullptr)) return SPRS_INVALID_ARGUMENT;
    if (k < 1 || k + 2 > (size_t)s->m || (which != SPRS_SVDS_LARGEST && which != SPRS_SVDS_SMALLEST) || max_restarts < 1)
        return SPRS_INVALID_ARGUMENT;
    if (v0_len != s->lenN) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (u && (u_len != k * s->rows || v_len != k * s->cols)) return SPRS_INCOMPATIBLE_X_SIZE;
    size_t d[3];
    CtxLock lock(s->ctx);
    return s->solve(k, which, v0, host, max_restarts, tol, vals, u, v, res, or_dummy(nconv, d), or_dummy(restarts, d + 1), or_dummy(matvecs, d + 2));
}

// The default start block: column c holds gen_uniform's values (internal.hpp) of stream 100 + 2 c (the imaginary parts: stream
// 101 + 2 c), rounded to T.
template <class T>
void lobpcg_default_x0(size_t n, int b, std::vector<T> &X0) {
    X0.resize(n * (size_t)b);
    for (int c = 0; c < b; ++c)
        for (size_t i = 0; i < n; ++i) {
            T v = sfromr<T>((Real<T>)gen_uniform(100 + 2 * (uint64_t)c, i));
            if constexpr (is_complex<T>::value) v.im = (Real<T>)gen_uniform(101 + 2 * (uint64_t)c, i);
            X0[(size_t)c * n + i] = v;
        }
}

// One LOBPCG solve.  X0 is copied into the work block and the vectors are written by the rotation kernel (device) or copied out
// of the work block (host), so no alignment is asked of either.  prec: a sprs_diag (or null) or an applied handle's view.
template <class T, class P>
int lobpcg_solve(Lobpcg<T> *s, bool host, const P &prec, size_t k, int which, const T *X0, size_t x0_len, size_t max_iter, Real<T> tol,
                 Real<T> *vals, T *vecs, size_t vecs_len, Real<T> *res, size_t *nconv, size_t *iters, size_t *restarts, size_t *matvecs) {
    const Precond<T> M(prec);
    if (!s || (M.is_applied && !M.applied.h) || !vals || !res) return SPRS_INVALID_ARGUMENT;
    if (k < 1 || k > (size_t)s->b || (which != SPRS_EIGSH_LARGEST && which != SPRS_EIGSH_SMALLEST) || max_iter < 1) return SPRS_INVALID_ARGUMENT;
    if (X0 && x0_len != (size_t)s->b * s->n) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (vecs && vecs_len != k * s->n) return SPRS_INCOMPATIBLE_X_SIZE;
    size_t d[4];
    std::vector<T> def;
    bool x0_host = host;
    if (!X0) { lobpcg_default_x0<T>(s->n, s->b, def); X0 = def.data(); x0_host = true; }
    CtxLock lock(s->ctx);
    return s->solve_dev(M, k, which, X0, x0_host, max_iter, tol, vals, vecs, host, res, or_dummy(nconv, d), or_dummy(iters, d + 1),
                        or_dummy(restarts, d + 2), or_dummy(matvecs, d + 3));
}

// the S<T> behind a handle, or null where the handle holds another scalar type
template <template <class> class S, class T>
S<T> *impl_of(sprs_solver_handle *h) { return (h && h->dtype == dtype_of<T>::value) ? (S<T> *)h->impl : nullptr; }

}  // namespace

// every solver impl derives from KrylovBase<T>
template <class F>
static int with_base(void *solver, int kind, F &&f) {
    auto *h = (sprs_solver_handle *)solver;
    if (!h) return SPRS_INVALID_ARGUMENT;
    switch (kind) {
        case SPRS_SOLVER_BICGSTAB: return with_solver<BicgStab>(h->dtype, h->impl, f);
        case SPRS_SOLVER_CG: return with_solver<Cg>(h->dtype, h->impl, f);
        case SPRS_SOLVER_GMRES: return with_solver<Gmres>(h->dtype, h->impl, f);
        case SPRS_SOLVER_LSMR: return with_solver<Lsmr>(h->dtype, h->impl, f);
        case SPRS_SOLVER_IDRS: return with_solver<Idrs>(h->dtype, h->impl, f);
        case SPRS_SOLVER_MINRES:
        case SPRS_SOLVER_CSMINRES: return with_solver<MinRes>(h->dtype, h->impl, f);
    }
    return SPRS_INVALID_ARGUMENT;
}


#define SPRS_CHK(c) do { if (!(c)) return SPRS_INVALID_ARGUMENT; } while (0)
#define SPRS_G(...) try { __VA_ARGS__ } catch (...) { return SPRS_ERR_HIP; }

extern "C" {

int sprs_csr_destroy(sprs_csr *A) {
    if (!A) return SPRS_OK;
    if (A->ctx) { (void)hipSetDevice(A->ctx->device); (void)hipStreamSynchronize(A->ctx->stream); }
    if (A->owns_arrays) {
        if (A->row_ptr) (void)hipFree(A->row_ptr);
        if (A->col_idx) (void)hipFree(A->col_idx);
        if (A->val) (void)hipFree(A->val);
    }
    if (A->rowblk) (void)hipFree(A->rowblk);
    if (A->blk_desc) (void)hipFree(A->blk_desc);
    if (A->blk_desc_eq) (void)hipFree(A->blk_desc_eq);
    if (A->tail) (void)hipFree(A->tail);
    free_dict(A);
    if (A->x_tmp) (void)hipFree(A->x_tmp);
    if (A->y_tmp) (void)hipFree(A->y_tmp);
    if (A->part) (void)hipFree(A->part);
    if (A->dist) {
        if (A->dist->send_idx) (void)hipFree(A->dist->send_idx);
        if (A->dist->send_buf) (void)hipFree(A->dist->send_buf);
        if (A->dist->ag_buf) (void)hipFree(A->dist->ag_buf);
        if (A->dist->order_int) (void)hipFree(A->dist->order_int);
        if (A->dist->order_bnd) (void)hipFree(A->dist->order_bnd);
        for (void *q : {(void *)A->dist->tile_int.list, (void *)A->dist->tile_int.xstart, (void *)A->dist->tile_int.left}) if (q) (void)hipFree(q);
        if (A->dist->order_int_w) (void)hipFree(A->dist->order_int_w);
        if (A->dist->order_bnd_w) (void)hipFree(A->dist->order_bnd_w);
        if (A->dist->ev_pack) (void)hipEventDestroy(A->dist->ev_pack);
        if (A->dist->ev_halo) (void)hipEventDestroy(A->dist->ev_halo);
        if (A->dist->comm_stream) (void)hipStreamDestroy(A->dist->comm_stream);
        delete A->dist;
    }
    delete A;
    return SPRS_OK;
}
int64_t sprs_csr_rows(const sprs_csr *A) { return A ? A->nrows : -1; }
int64_t sprs_csr_cols(const sprs_csr *A) { return A ? A->ncols : -1; }
int64_t sprs_csr_nnz(const sprs_csr *A) { return A ? A->nnz : -1; }
// The handle's CSR arrays copied to the host (any pointer may be NULL): row_ptr nrows + 1 and col_idx nnz entries of i32, val nnz
// entries of the handle's scalar type.
int sprs_csr_read(const sprs_csr *A, int32_t *row_ptr_host, int32_t *col_idx_host, void *val_host) {
    if (!A) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (row_ptr_host) SPRS_HIP_TRY(c, hipMemcpyAsync(row_ptr_host, A->row_ptr, sizeof(int32_t) * ((size_t)A->nrows + 1), hipMemcpyDeviceToHost, c->stream));
    if (col_idx_host && A->nnz) SPRS_HIP_TRY(c, hipMemcpyAsync(col_idx_host, A->col_idx, sizeof(int32_t) * (size_t)A->nnz, hipMemcpyDeviceToHost, c->stream));
    if (val_host && A->nnz) SPRS_HIP_TRY(c, hipMemcpyAsync(val_host, A->val, dtype_size(A->dtype) * (size_t)A->nnz, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}
int sprs_csr_wide_blocks(const sprs_csr *A, int64_t *n_blocks, int64_t *n_uniform) {
    if (!A || !n_blocks || !n_uniform) return SPRS_INVALID_ARGUMENT;
    *n_blocks = 0; *n_uniform = 0;
    const SpmvRoute r = spmv_route(A, SpmvPart::Whole, false);
    if (r.format == 0) {       // plain CSR stream: the 64-row blocks; "uniform" = equal-length blocks, which read no row_ptr
        *n_blocks = A->n_rowblk; *n_uniform = A->blk_desc_eq ? A->n_eq_blocks : 0;
        return SPRS_OK;
    }
    // the descriptors the SpMV of this handle walks: 128-row blocks of the f64 pair-code stream, else the 64-row
    // blocks of the offset-code stream (the 64-row pair-code kernel walks the plain descriptors: no uniform blocks)
    const sprs_dict *D = A->dict;
    // (as always reported: a matrix of one row or column has its 128-row descriptors counted though the Pair2 guard walks it by 64-row blocks)
    const bool one_line = r.format == 2 && D->wide_desc && (A->nrows < 2 || A->ncols < 2) && A->ctx->spmv_wide != 0;
    const bool wide = (D->wide_desc && r.desc == D->wide_desc) || one_line;
    const void *src = wide ? D->wide_desc : (D->off_desc && r.desc == D->off_desc ? D->off_desc : nullptr);
    const int64_t nb = wide ? D->n_wide : (src ? A->n_rowblk : 0);
    if (!src || nb == 0) return SPRS_OK;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    std::vector<int32_t> d((size_t)nb * 4);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    SPRS_HIP_TRY(c, hipMemcpyAsync(d.data(), src, d.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_blocks = nb;
    for (int64_t j = 0; j < nb; ++j) *n_uniform += ((uint32_t)d[(size_t)j * 4 + 1] & sprs::UNI2) != 0;
    return SPRS_OK;
}
int sprs_csr_tile_plan(const sprs_csr *A, int64_t *n_tiles, int64_t *n_tile_blocks, int64_t *n_other_blocks) {
    if (!A || !n_tiles || !n_tile_blocks || !n_other_blocks) return SPRS_INVALID_ARGUMENT;
    *n_tiles = 0; *n_tile_blocks = 0; *n_other_blocks = 0;
    // a distributed operator with an interior / boundary split: the interior launch's plan (boundary blocks are walked singly)
    const bool split = A->dist && A->dist->order_int;
    const SpmvRoute r = spmv_route(A, split ? SpmvPart::Interior : SpmvPart::Whole, false);
    if (r.kernel != SpmvKernel::TilePair && r.kernel != SpmvKernel::TileOff) return SPRS_OK;
    const sprs_tile_plan &TP = *r.tile;
    *n_tiles = TP.n_tile; *n_tile_blocks = (int64_t)TP.n_tile * sprs::tile_blocks();
    // the other blocks in 128-row units (the offset stream walks them as 64-row blocks)
    if (split) *n_other_blocks = (A->n_rowblk + 1) / 2 - *n_tile_blocks;
    else *n_other_blocks = r.kernel == SpmvKernel::TilePair ? TP.n_left : (TP.n_left + 1) / 2;
    return SPRS_OK;
}
int sprs_csr_chain_plan(const sprs_csr *A, int64_t *n_tiles, int64_t *n_segments, int64_t *n_chains, int64_t *n_other_blocks) {
    if (!A || !n_tiles || !n_segments || !n_chains || !n_other_blocks) return SPRS_INVALID_ARGUMENT;
    *n_tiles = 0; *n_segments = 0; *n_chains = 0; *n_other_blocks = 0;
    const SpmvRoute r = spmv_route(A, SpmvPart::Whole, false);
    if (r.kernel != SpmvKernel::Chain) return SPRS_OK;
    *n_tiles = r.chain->n_tile; *n_segments = r.chain->n_seg; *n_chains = r.chain->n_chain; *n_other_blocks = r.chain->n_left;
    return SPRS_OK;
}
int sprs_csr_spmv_route(const sprs_csr *A, int part, int conj_x, int *kernel, int *format, int *grid, int64_t *n_blocks,
                        int *ordered, int *y_nt) {
    if (!A || part < 0 || part > 2 || !kernel || !format || !grid || !n_blocks || !ordered || !y_nt) return SPRS_INVALID_ARGUMENT;
    *kernel = -1; *format = 0; *grid = 0; *n_blocks = 0; *ordered = 0; *y_nt = 0;
    if (part != 0 && !(A->dist && A->dist->order_int)) return SPRS_OK;          // no interior / boundary split
    const SpmvRoute r = spmv_route(A, part == 0 ? SpmvPart::Whole : part == 1 ? SpmvPart::Interior : SpmvPart::Boundary, conj_x != 0);
    *kernel = (int)r.kernel; *format = r.format; *grid = r.grid; *n_blocks = r.count; *ordered = r.order ? 1 : 0; *y_nt = r.y_nt ? 1 : 0;
    return SPRS_OK;
}
int sprs_csr_stream_format(const sprs_csr *A, int *n_offsets, int *n_values) {
    if (!A) return -1;
    if (n_offsets) *n_offsets = A->dict ? A->dict->n_off : 0;
    if (n_values) *n_values = A->dict ? (A->dict->n_pair ? A->dict->n_pair : 0) : 0;
    return spmv_route(A, SpmvPart::Whole, false).format;
}

int sprs_diag_precond_destroy(sprs_diag *P) {
    if (!P) return SPRS_OK;
    if (P->ctx) { (void)hipSetDevice(P->ctx->device); (void)hipStreamSynchronize(P->ctx->stream); }
    if (P->dinv) (void)hipFree(P->dinv);
    if (P->in_tmp) (void)hipFree(P->in_tmp);
    if (P->out_tmp) (void)hipFree(P->out_tmp);
    delete P;
    return SPRS_OK;
}
int sprs_bicgstab_destroy(sprs_bicgstab *S) { return solver_destroy<BicgStab>(S); }
int sprs_minres_destroy(sprs_minres *S) { return solver_destroy<MinRes>(S); }
int sprs_csminres_destroy(sprs_csminres *S) { return solver_destroy<MinRes>(S); }
int sprs_cg_destroy(sprs_cg *S) { return solver_destroy<Cg>(S); }
int sprs_gmres_destroy(sprs_gmres *S) { return solver_destroy<Gmres>(S); }
int sprs_cgmany_destroy(sprs_cg_many *S) { return solver_destroy<CgMany>(S); }
int sprs_cgshift_destroy(sprs_cg_shift *S) { return solver_destroy<CgShift>(S); }
int sprs_idrs_destroy(sprs_idrs *S) { return solver_destroy<Idrs>(S); }
int sprs_lsmr_destroy(sprs_lsmr *S) { return solver_destroy<Lsmr>(S); }
int sprs_eigsh_destroy(sprs_eigsh *S) { return solver_destroy<Eigsh>(S); }
int sprs_lobpcg_destroy(sprs_lobpcg *S) { return solver_destroy<Lobpcg>(S); }
int sprs_svds_destroy(sprs_svds *S) { return solver_destroy<Svds>(S); }
int sprs_expm_destroy(sprs_expm *S) { return solver_destroy<Expm>(S); }

// ---- a solver's entry points per scalar type.  NAME = the handle is sprs_NAME, S = its class, CREATE = the arguments of S<T>::create
#define SPRS_SOLVER_SOLVES(X, T, CT, R, NAME, S)                                                                       \
    int sprs_##NAME##_solve_##X(sprs_##NAME *h, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res) { \
        SPRS_G(return solve<T>(impl_of<S, T>(h), true, nullptr, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res);)   \
    }                                                                                                                  \
    int sprs_##NAME##_precond_solve_##X(sprs_##NAME *h, const sprs_diag *P, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res) { \
        SPRS_G(if (!P) return SPRS_INVALID_ARGUMENT; return solve<T>(impl_of<S, T>(h), true, P, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res);) \
    }                                                                                                                  \
    int sprs_##NAME##_solve_dev_##X(sprs_##NAME *h, const sprs_diag *P, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res) { \
        SPRS_G(return solve<T>(impl_of<S, T>(h), false, P, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res);)        \
    }
#define SPRS_SOLVER_API(X, T, CT, R, NAME, S, CREATE)                                                                  \
    int sprs_##NAME##_create_##X(const sprs_csr *A, size_t n, sprs_##NAME **out) {                                     \
        SPRS_G(return (solver_create<T, sprs_##NAME, S>("sprs_" #NAME, A, out, [&](auto *s) { return s->create CREATE; }));) \
    }                                                                                                                  \
    SPRS_SOLVER_SOLVES(X, T, CT, R, NAME, S)

// ---- everything that exists once per scalar type.  X = suffix, T = device scalar, CT = C-ABI scalar
// (passed by value / pointer), R = T::Real
#define SPRS_API(X, T, CT, R)                                                                                          \
    int sprs_csr_create_##X(sprs_ctx *c, int64_t nr, int64_t nc, int64_t nnz, const int32_t *rp, const int32_t *ci,    \
                            const CT *v, int csc, sprs_csr **out) {                                                    \
        SPRS_G(return csr_create_host<T, int32_t>(c, nr, nc, nnz, rp, ci, (const T *)v, csc, out);)                    \
    }                                                                                                                  \
    int sprs_csr_create_i64_##X(sprs_ctx *c, int64_t nr, int64_t nc, int64_t nnz, const int64_t *rp,                   \
                                const int64_t *ci, const CT *v, int csc, sprs_csr **out) {                             \
        SPRS_G(return csr_create_host<T, int64_t>(c, nr, nc, nnz, rp, ci, (const T *)v, csc, out);)                    \
    }                                                                                                                  \
    int sprs_csr_create_dev_##X(sprs_ctx *c, int64_t nr, int64_t nc, int64_t nnz, const int32_t *rp,                   \
                                const int32_t *ci, const CT *v, int adopt, sprs_csr **out) {                           \
        SPRS_G(return csr_create_dev<T>(c, nr, nc, nnz, rp, ci, (const T *)v, adopt, out);)                            \
    }                                                                                                                  \
    int sprs_mul_vec_##X(const sprs_csr *A, const CT *x, size_t xl, CT *y, size_t yl) {                                \
        SPRS_G(return mul_vec_host<T>(A, (const T *)x, xl, (T *)y, yl, nullptr);)                                      \
    }                                                                                                                  \
    int sprs_mul_vec_dot_##X(const sprs_csr *A, const CT *x, size_t xl, CT *y, size_t yl, CT *d) {                     \
        SPRS_G(if (!d) return SPRS_INVALID_ARGUMENT; return mul_vec_host<T>(A, (const T *)x, xl, (T *)y, yl, (T *)d);) \
    }                                                                                                                  \
    int sprs_mul_vec_dev_##X(const sprs_csr *A, const CT *x, CT *y) { return mul_vec_dev<T>(A, (const T *)x, (T *)y, nullptr); } \
    int sprs_mul_vec_dot_dev_##X(const sprs_csr *A, const CT *x, CT *y, CT *d) {                                       \
        if (!d) return SPRS_INVALID_ARGUMENT;                                                                          \
        return mul_vec_dev<T>(A, (const T *)x, (T *)y, (T *)d);                                                        \
    }                                                                                                                  \
    int sprs_mul_vec_dev_timed_##X(const sprs_csr *A, const CT *x, CT *y, int reps, double *ms) {                      \
        return mul_vec_timed<T>(A, (const T *)x, (T *)y, reps, ms);                                                    \
    }                                                                                                                  \
    int sprs_mul_mat_##X(const sprs_csr *A, const CT *x, size_t xl, CT *y, size_t yl, size_t k) {                      \
        SPRS_G(return mul_mat_host<T>(A, (const T *)x, xl, (T *)y, yl, k);)                                            \
    }                                                                                                                  \
    int sprs_mul_mat_dev_##X(const sprs_csr *A, const CT *x, CT *y, size_t k) { return mul_mat_dev<T>(A, (const T *)x, (T *)y, k); } \
    /* batched CG: k = the most columns a solve may carry */                                                           \
    int sprs_cgmany_create_##X(const sprs_csr *A, size_t n, size_t k, sprs_cg_many **out) {                           \
        SPRS_G(return (solver_create<T, sprs_cg_many, CgMany>("sprs_cgmany", A, out, [&](auto *s) { return s->create(A, n, k); }));) \
    }                                                                                                                  \
    int sprs_cgmany_solve_##X(sprs_cg_many *h, const sprs_diag *P, const CT *rhs, size_t rl, CT *x, size_t xl, size_t k, size_t mi, R tol, \
                               size_t *its, R *res, int *status) {                                                     \
        SPRS_G(return solve_many<T>(impl_of<CgMany, T>(h), true, P, (const T *)rhs, rl, (T *)x, xl, k, mi, tol, its, res, status);) \
    }                                                                                                                  \
    int sprs_cgmany_solve_dev_##X(sprs_cg_many *h, const sprs_diag *P, const CT *rhs, size_t rl, CT *x, size_t xl, size_t k, size_t mi, R tol, \
                                   size_t *its, R *res, int *status) {                                                 \
        SPRS_G(return solve_many<T>(impl_of<CgMany, T>(h), false, P, (const T *)rhs, rl, (T *)x, xl, k, mi, tol, its, res, status);) \
    }                                                                                                                  \
    /* multi-shift CG: mmax = the most shifts a solve may carry; x = m contiguous vectors of n, output only */          \
    int sprs_cgshift_create_##X(const sprs_csr *A, size_t n, size_t mmax, sprs_cg_shift **out) {                       \
        SPRS_G(return (solver_create<T, sprs_cg_shift, CgShift>("sprs_cgshift", A, out, [&](auto *s) { return s->create(A, n, mmax); }));) \
    }                                                                                                                  \
    int sprs_cgshift_solve_##X(sprs_cg_shift *h, const R *shifts, size_t m, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, \
                               size_t *its, R *res, int *status) {                                                     \
        SPRS_G(return solve_shift<T>(impl_of<CgShift, T>(h), true, shifts, m, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res, status);) \
    }                                                                                                                  \
    int sprs_cgshift_solve_dev_##X(sprs_cg_shift *h, const R *shifts, size_t m, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, \
                                   size_t *its, R *res, int *status) {                                                 \
        SPRS_G(return solve_shift<T>(impl_of<CgShift, T>(h), false, shifts, m, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res, status);) \
    }                                                                                                                  \
    /* LSMR: A of any shape and its adjoint handle (NULL: built and owned by the solver) */                            \
    int sprs_lsmr_create_##X(const sprs_csr *A, const sprs_csr *AH, sprs_lsmr **out) {                                 \
        SPRS_G(return (solver_create<T, sprs_lsmr, Lsmr>("sprs_lsmr", A, out, [&](auto *s) { return s->create(A, AH); }));) \
    }                                                                                                                  \
    int sprs_lsmr_solve_##X(sprs_lsmr *h, const CT *rhs, size_t rl, CT *x, size_t xl, R damp, size_t mi, R tol, size_t *its, R *res, R *ares) { \
        SPRS_G(return lsmr_solve<T>(impl_of<Lsmr, T>(h), true, (const T *)rhs, rl, (T *)x, xl, damp, mi, tol, its, res, ares);) \
    }                                                                                                                  \
    int sprs_lsmr_solve_dev_##X(sprs_lsmr *h, const CT *rhs, size_t rl, CT *x, size_t xl, R damp, size_t mi, R tol, size_t *its, R *res, R *ares) { \
        SPRS_G(return lsmr_solve<T>(impl_of<Lsmr, T>(h), false, (const T *)rhs, rl, (T *)x, xl, damp, mi, tol, its, res, ares);) \
    }                                                                                                                  \
    /* thick-restart Lanczos: ncv = the basis size (0 = min(32, n)) */                                                 \
    int sprs_eigsh_create_##X(const sprs_csr *A, size_t n, size_t ncv, sprs_eigsh **out) {                             \
        SPRS_G(return (solver_create<T, sprs_eigsh, Eigsh>("sprs_eigsh", A, out, [&](auto *s) { return s->create(A, n, ncv); }));) \
    }                                                                                                                  \
    int sprs_eigsh_solve_##X(sprs_eigsh *h, size_t k, int which, const CT *v0, size_t vl, size_t mr, R tol, R *vals, CT *vecs, size_t xl, \
                             R *res, size_t *nconv, size_t *restarts, size_t *matvecs) {                               \
        SPRS_G(return eigsh_solve<T>(impl_of<Eigsh, T>(h), true, k, which, (const T *)v0, vl, mr, tol, vals, (T *)vecs, xl, res, nconv, restarts, matvecs);) \
    }                                                                                                                  \
    int sprs_eigsh_solve_dev_##X(sprs_eigsh *h, size_t k, int which, const CT *v0, size_t vl, size_t mr, R tol, R *vals, CT *vecs, size_t xl, \
                                 R *res, size_t *nconv, size_t *restarts, size_t *matvecs) {                           \
        SPRS_G(return eigsh_solve<T>(impl_of<Eigsh, T>(h), false, k, which, (const T *)v0, vl, mr, tol, vals, (T *)vecs, xl, res, nconv, restarts, matvecs);) \
    }                                                                                                                  \
    /* truncated SVD: A of any shape and its adjoint handle (NULL: built and owned), ncv = the basis size (0 = min(32, min(rows, cols))) */ \
    int sprs_svds_create_##X(const sprs_csr *A, const sprs_csr *AH, size_t ncv, sprs_svds **out) {                     \
        SPRS_G(return (solver_create<T, sprs_svds, Svds>("sprs_svds", A, out, [&](auto *s) { return s->create(A, AH, ncv); }));) \
    }                                                                                                                  \
    int sprs_svds_solve_##X(sprs_svds *h, size_t k, int which, const CT *v0, size_t vl, size_t mr, R tol, R *vals, CT *u, size_t ul, CT *v, size_t vvl, \
                            R *res, size_t *nconv, size_t *restarts, size_t *matvecs) {                                \
        SPRS_G(return svds_solve<T>(impl_of<Svds, T>(h), true, k, which, (const T *)v0, vl, mr, tol, vals, (T *)u, ul, (T *)v, vvl, res, nconv, restarts, matvecs);) \
    }                                                                                                                  \
    int sprs_svds_solve_dev_##X(sprs_svds *h, size_t k, int which, const CT *v0, size_t vl, size_t mr, R tol, R *vals, CT *u, size_t ul, CT *v, size_t vvl, \
                                R *res, size_t *nconv, size_t *restarts, size_t *matvecs) {                            \
        SPRS_G(return svds_solve<T>(impl_of<Svds, T>(h), false, k, which, (const T *)v0, vl, mr, tol, vals, (T *)u, ul, (T *)v, vvl, res, nconv, restarts, matvecs);) \
    }                                                                                                                  \
    /* exp(tA) v: ncv = the basis size (0 = min(30, n)) */                                                             \
    int sprs_expm_create_##X(const sprs_csr *A, size_t n, size_t ncv, sprs_expm **out) {                               \
        SPRS_G(return (solver_create<T, sprs_expm, Expm>("sprs_expm", A, out, [&](auto *s) { return s->create(A, n, ncv); }));) \
    }                                                                                                                  \
    int sprs_expm_apply_##X(sprs_expm *h, R t, const CT *v, size_t vl, R tol, size_t ms, R tau0, CT *w, size_t wl, R *err, R *hump, R *t_done, \
                            size_t *steps, size_t *rejects, size_t *matvecs) {                                         \
        SPRS_G(return expm_apply<T>(impl_of<Expm, T>(h), true, t, (const T *)v, vl, tol, ms, tau0, (T *)w, wl, err, hump, t_done, steps, rejects, matvecs);) \
    }                                                                                                                  \
    int sprs_expm_apply_dev_##X(sprs_expm *h, R t, const CT *v, size_t vl, R tol, size_t ms, R tau0, CT *w, size_t wl, R *err, R *hump, R *t_done, \
                                size_t *steps, size_t *rejects, size_t *matvecs) {                                     \
        SPRS_G(return expm_apply<T>(impl_of<Expm, T>(h), false, t, (const T *)v, vl, tol, ms, tau0, (T *)w, wl, err, hump, t_done, steps, rejects, matvecs);) \
    }                                                                                                                  \
    /* LOBPCG: block = the block size (0 = min(8, n / 6)) */                                                           \
    int sprs_lobpcg_create_##X(const sprs_csr *A, size_t n, size_t block, sprs_lobpcg **out) {                         \
        SPRS_G(return (solver_create<T, sprs_lobpcg, Lobpcg>("sprs_lobpcg", A, out, [&](auto *s) { return s->create(A, n, block); }));) \
    }                                                                                                                  \
    int sprs_lobpcg_solve_##X(sprs_lobpcg *h, const sprs_diag *P, size_t k, int which, const CT *x0, size_t x0l, size_t mi, R tol, R *vals, CT *vecs, \
                              size_t xl, R *res, size_t *nconv, size_t *iters, size_t *restarts, size_t *matvecs) {    \
        SPRS_G(return lobpcg_solve<T>(impl_of<Lobpcg, T>(h), true, P, k, which, (const T *)x0, x0l, mi, tol, vals, (T *)vecs, xl, res, nconv, iters, restarts, matvecs);) \
    }                                                                                                                  \
    int sprs_lobpcg_solve_dev_##X(sprs_lobpcg *h, const sprs_diag *P, size_t k, int which, const CT *x0, size_t x0l, size_t mi, R tol, R *vals, CT *vecs, \
                                  size_t xl, R *res, size_t *nconv, size_t *iters, size_t *restarts, size_t *matvecs) { \
        SPRS_G(return lobpcg_solve<T>(impl_of<Lobpcg, T>(h), false, P, k, which, (const T *)x0, x0l, mi, tol, vals, (T *)vecs, xl, res, nconv, iters, restarts, matvecs);) \
    }                                                                                                                  \
    int sprs_dot_##X(sprs_ctx *c, size_t n, const CT *x, const CT *y, CT *o) { SPRS_CHK(c && o); return dot_host<T>(c, n, (const T *)x, (const T *)y, false, (T *)o); } \
    int sprs_conj_dot_##X(sprs_ctx *c, size_t n, const CT *x, const CT *y, CT *o) { SPRS_CHK(c && o); return dot_host<T>(c, n, (const T *)x, (const T *)y, true, (T *)o); } \
    int sprs_norm2_##X(sprs_ctx *c, size_t n, const CT *x, R *o) { SPRS_CHK(c && o); return norm2_host<T>(c, n, (const T *)x, o); } \
    int sprs_scale_##X(sprs_ctx *c, size_t n, CT a, CT *x) { SPRS_CHK(c); T aa; memcpy(&aa, &a, sizeof(T)); return launch_scale<T>(c, n, aa, (T *)x); } \
    int sprs_rscale_##X(sprs_ctx *c, size_t n, R a, CT *x) { SPRS_CHK(c); return launch_rscale<T>(c, n, a, (T *)x); }  \
    int sprs_conj_##X(sprs_ctx *c, size_t n, const CT *in, CT *out) { SPRS_CHK(c); return launch_conj<T>(c, n, (const T *)in, (T *)out); } \
    int sprs_axpy_##X(sprs_ctx *c, size_t n, CT a, const CT *x, CT *y) { SPRS_CHK(c); T aa; memcpy(&aa, &a, sizeof(T)); return launch_axpy<T, T>(c, n, aa, (const T *)x, (T *)y); } \
    int sprs_axpby_##X(sprs_ctx *c, size_t n, CT a, const CT *x, CT b, CT *y) {                                        \
        SPRS_CHK(c); T aa, bb; memcpy(&aa, &a, sizeof(T)); memcpy(&bb, &b, sizeof(T));                                 \
        return launch_axpby<T>(c, n, aa, (const T *)x, bb, (T *)y);                                                    \
    }                                                                                                                  \
    int sprs_diag_mul_vec_##X(const sprs_diag *P, const CT *in, size_t il, CT *out, size_t ol) {                       \
        SPRS_G(return diag_apply_host<T>(P, (const T *)in, il, (T *)out, ol);)                                         \
    }                                                                                                                  \
    int sprs_diag_mul_vec_dev_##X(const sprs_diag *P, const CT *in, CT *out) { return diag_apply_dev<T>(P, (const T *)in, (T *)out); } \
    SPRS_SOLVER_API(X, T, CT, R, bicgstab, BicgStab, (A, n))                                                           \
    SPRS_SOLVER_API(X, T, CT, R, minres, MinRes, (A, n, false))                                                        \
    SPRS_SOLVER_API(X, T, CT, R, cg, Cg, (A, n))                                                                       \
    /* GMRES' create takes the restart length (0 = 30) */                                                              \
    int sprs_gmres_create_##X(const sprs_csr *A, size_t n, size_t restart, sprs_gmres **out) {                         \
        SPRS_G(return (solver_create<T, sprs_gmres, Gmres>("sprs_gmres", A, out, [&](auto *s) { return s->create(A, n, restart); }));) \
    }                                                                                                                  \
    SPRS_SOLVER_SOLVES(X, T, CT, R, gmres, Gmres)                                                                      \
    /* IDR(s)'s create takes s (0 = 4); the class refuses s > SPRS_IDRS_MAX_S, s > n and a distributed operator with a text */ \
    int sprs_idrs_create_##X(const sprs_csr *A, size_t n, size_t s_dim, sprs_idrs **out) {                             \
        SPRS_G(return (solver_create<T, sprs_idrs, Idrs>("sprs_idrs", A, out, [&](auto *s) { return s->create(A, n, s_dim); }));) \
    }                                                                                                                  \
    SPRS_SOLVER_SOLVES(X, T, CT, R, idrs, Idrs)                                                                        \
    /* CSMinRes has no precond_solve (cs_minres.rs) */                                                                  \
    int sprs_csminres_create_##X(const sprs_csr *A, size_t n, sprs_csminres **out) {                                   \
        SPRS_G(return (solver_create<T, sprs_csminres, MinRes>("sprs_csminres", A, out, [&](auto *s) { return s->create(A, n, true); }));) \
    }                                                                                                                  \
    int sprs_csminres_solve_##X(sprs_csminres *h, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res) { \
        SPRS_G(return solve<T>(impl_of<MinRes, T>(h), true, nullptr, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res);) \
    }                                                                                                                  \
    int sprs_csminres_solve_dev_##X(sprs_csminres *h, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res) { \
        SPRS_G(return solve<T>(impl_of<MinRes, T>(h), false, nullptr, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res);) \
    }

SPRS_API(d, double, double, double)
SPRS_API(z, cplx, sprs_c64, double)
SPRS_API(s, float, float, float)
SPRS_API(c, cplxf, sprs_c32, float)

// BiCGStab, MINRES, CG and GMRES preconditioned by an ILU(0) handle (ilu0.hip), an AMG handle (amg.hip), an FSAI handle (fsai.hip) or a block-Jacobi handle (bjacobi.hip): one path, the handle's AppliedPrec view
#define SPRS_APPLIED_SOLVES(X, T, CT, R, NAME, S, PFX)                                                                 \
    int sprs_##PFX##_##NAME##_solve_##X(sprs_##NAME *h, const sprs_##PFX *P, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res) { \
        SPRS_G(return solve<T>(impl_of<S, T>(h), true, PFX##_prec<T>(P), (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res);)  \
    }                                                                                                                  \
    int sprs_##PFX##_##NAME##_solve_dev_##X(sprs_##NAME *h, const sprs_##PFX *P, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res) { \
        SPRS_G(return solve<T>(impl_of<S, T>(h), false, PFX##_prec<T>(P), (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res);) \
    }
// LOBPCG preconditioned by such a handle: the device entry only
#define SPRS_APPLIED_LOBPCG(X, T, CT, R, PFX)                                                                          \
    int sprs_##PFX##_lobpcg_solve_dev_##X(sprs_lobpcg *h, const sprs_##PFX *P, size_t k, int which, const CT *x0, size_t x0l, size_t mi, R tol, R *vals, \
                                          CT *vecs, size_t xl, R *res, size_t *nconv, size_t *iters, size_t *restarts, size_t *matvecs) { \
        SPRS_G(return lobpcg_solve<T>(impl_of<Lobpcg, T>(h), false, PFX##_prec<T>(P), k, which, (const T *)x0, x0l, mi, tol, vals, (T *)vecs, xl, res, nconv, iters, restarts, matvecs);) \
    }
#define SPRS_APPLIED_API(X, T, CT, R)                                                                 \
    SPRS_APPLIED_SOLVES(X, T, CT, R, cg, Cg, ilu0) SPRS_APPLIED_SOLVES(X, T, CT, R, gmres, Gmres, ilu0) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, cg, Cg, amg) SPRS_APPLIED_SOLVES(X, T, CT, R, gmres, Gmres, amg) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, bicgstab, BicgStab, ilu0) SPRS_APPLIED_SOLVES(X, T, CT, R, minres, MinRes, ilu0) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, bicgstab, BicgStab, amg) SPRS_APPLIED_SOLVES(X, T, CT, R, minres, MinRes, amg) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, cg, Cg, fsai) SPRS_APPLIED_SOLVES(X, T, CT, R, gmres, Gmres, fsai) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, bicgstab, BicgStab, fsai) SPRS_APPLIED_SOLVES(X, T, CT, R, minres, MinRes, fsai) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, idrs, Idrs, ilu0) SPRS_APPLIED_SOLVES(X, T, CT, R, idrs, Idrs, amg) SPRS_APPLIED_SOLVES(X, T, CT, R, idrs, Idrs, fsai) \
    SPRS_APPLIED_LOBPCG(X, T, CT, R, ilu0) SPRS_APPLIED_LOBPCG(X, T, CT, R, amg) SPRS_APPLIED_LOBPCG(X, T, CT, R, fsai) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, cg, Cg, bjacobi) SPRS_APPLIED_SOLVES(X, T, CT, R, gmres, Gmres, bjacobi) \
    SPRS_APPLIED_SOLVES(X, T, CT, R, bicgstab, BicgStab, bjacobi) SPRS_APPLIED_SOLVES(X, T, CT, R, minres, MinRes, bjacobi)
SPRS_APPLIED_API(d, double, double, double)
SPRS_APPLIED_API(z, cplx, sprs_c64, double)
SPRS_APPLIED_API(s, float, float, float)
SPRS_APPLIED_API(c, cplxf, sprs_c32, float)

// complex vector, real scalar (S = Real, T = Complex; vecalg.rs:746-757)
int sprs_axpy_zd(sprs_ctx *c, size_t n, double a, const sprs_c64 *x, sprs_c64 *y) { SPRS_CHK(c); return launch_axpy<cplx, double>(c, n, a, (const cplx *)x, (cplx *)y); }
int sprs_axpy_cs(sprs_ctx *c, size_t n, float a, const sprs_c32 *x, sprs_c32 *y) { SPRS_CHK(c); return launch_axpy<cplxf, float>(c, n, a, (const cplxf *)x, (cplxf *)y); }

// DiagPrecond<T, V>::new  (precond.rs:20-29)
int sprs_diag_precond_create_d(sprs_ctx *c, size_t n, const double *d, sprs_diag **out) { SPRS_G(return diag_create<double>(c, n, d, DT_D, out);) }
int sprs_diag_precond_create_zd(sprs_ctx *c, size_t n, const double *d, sprs_diag **out) { SPRS_G(return diag_create<double>(c, n, d, DT_Z, out);) }
int sprs_diag_precond_create_z(sprs_ctx *c, size_t n, const sprs_c64 *d, sprs_diag **out) { SPRS_G(return diag_create<cplx>(c, n, (const cplx *)d, DT_Z, out);) }
int sprs_diag_precond_create_s(sprs_ctx *c, size_t n, const float *d, sprs_diag **out) { SPRS_G(return diag_create<float>(c, n, d, DT_S, out);) }
int sprs_diag_precond_create_cs(sprs_ctx *c, size_t n, const float *d, sprs_diag **out) { SPRS_G(return diag_create<float>(c, n, d, DT_C, out);) }
int sprs_diag_precond_create_c(sprs_ctx *c, size_t n, const sprs_c32 *d, sprs_diag **out) { SPRS_G(return diag_create<cplxf>(c, n, (const cplxf *)d, DT_C, out);) }

// ------------------------------------------------------------------------------ options / instrumentation
int sprs_solver_set_mode(void *solver, int kind, int mode) {
    if (mode != 0 && mode != 1) return SPRS_INVALID_ARGUMENT;
    if (kind == SPRS_SOLVER_IDRS && mode != 0) return SPRS_INVALID_ARGUMENT;   // IDR(s) has one mode
    return with_base(solver, kind, [&](auto *b) { b->mode = mode; return (int)SPRS_OK; });
}
int sprs_solver_set_trace(void *solver, int kind, double *trace_host, size_t cap) {
    return with_base(solver, kind, [&](auto *b) { b->trace = trace_host; b->trace_cap = trace_host ? cap : 0; b->trace_rows = 0; return (int)SPRS_OK; });
}
int sprs_solver_trace_rows(const void *solver, int kind, size_t *rows_out) {
    if (!rows_out) return SPRS_INVALID_ARGUMENT;
    return with_base(const_cast<void *>(solver), kind, [&](auto *b) { *rows_out = b->trace_rows; return (int)SPRS_OK; });
}
int sprs_solver_set_profile(void *solver, int kind, int enable) {
    return with_base(solver, kind, [&](auto *b) { b->profile = enable < 0 ? 0 : enable; return (int)SPRS_OK; });
}
int sprs_solver_get_profile(const void *solver, int kind, double *spmv_ms, int64_t *launches, double *solve_ms) {
    return with_base(const_cast<void *>(solver), kind, [&](auto *b) {
        if (spmv_ms) *spmv_ms = b->stats.spmv_ms;
        if (launches) *launches = b->stats.spmv_launches;
        if (solve_ms) *solve_ms = b->stats.solve_ms;
        return (int)SPRS_OK;
    });
}

int sprs_solver_get_profile_counts(const void *solver, int kind, int64_t *steps, int64_t *timed_dot_other, int64_t *timed_k2_fused,
                                   int64_t *timed_k4_fused) {
    return with_base(const_cast<void *>(solver), kind, [&](auto *b) {
        if (steps) *steps = b->stats.steps;
        if (timed_dot_other) *timed_dot_other = b->stats.timed_dot_other;
        if (timed_k2_fused) *timed_k2_fused = b->stats.timed_fused_k2;
        if (timed_k4_fused) *timed_k4_fused = b->stats.timed_fused_k4;
        return (int)SPRS_OK;
    });
}

int sprs_solver_get_fused_launches(const void *solver, int kind, int64_t *k2_fused, int64_t *k4_fused) {
    return with_base(const_cast<void *>(solver), kind, [&](auto *b) {
        if (k2_fused) *k2_fused = b->stats.fused_k2;
        if (k4_fused) *k4_fused = b->stats.fused_k4;
        return (int)SPRS_OK;
    });
}

int sprs_solver_get_chain_k5_launches(const void *solver, int kind, int64_t *launches) {
    return with_base(const_cast<void *>(solver), kind, [&](auto *b) {
        if (launches) *launches = b->stats.chain_k5;
        return (int)SPRS_OK;
    });
}

}  // extern "C"
