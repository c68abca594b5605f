// The adjoint of a CSR operator as an ordinary handle of its own, built in HBM (sprs_csr_adjoint).
// Row j of the result holds the entries of column j of A in ascending entry index, i.e. in ascending original row with the
// stored order of one row kept (duplicates included): the arrays of the stable CSC -> CSR conversion of csr_create_host
// (capi.hip) given A's arrays as the CSC of the result.  Three passes over the entries:
//   count   per-column entry counts (integer atomics: the counts do not depend on the order of arrival)
//   scan    rocprim::exclusive_scan of the counts = the result's row_ptr
//   fill    a STABLE radix sort of (column, entry index) pairs on the column's significant bits — rocprim::radix_sort_pairs,
//           whose result is a function of its input alone — then one gather that writes col_idx (the source row, found by
//           bisection in A's row_ptr) and val (conjugated on request) of every entry at its sorted position
// No slot is handed out by an atomic counter, so two constructions give the same arrays.  The finished arrays go through
// sprs_csr_create_dev_* like any matrix built in HBM (row blocks, dictionary streams, tile and chain plans) and are then owned
// by the new handle.  adjoint_dev (internal.hpp) is the same three passes on raw arrays without the handle: the AMG set-up
// forms R = P^H with it (amg_setup.hpp).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "internal.hpp"

using namespace sprs;

namespace {

__global__ __launch_bounds__(BLOCK) void adj_count_kernel(int64_t nnz, int64_t ncols, const int32_t *__restrict__ col_idx,
                                                          int32_t *__restrict__ cnt, int32_t *__restrict__ key, int32_t *__restrict__ ent) {
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * BLOCK) {
        const int32_t c = col_idx[k];
        key[k] = c; ent[k] = (int32_t)k;
        if (c >= 0 && (int64_t)c < ncols) atomicAdd(cnt + c, 1);          // (creation validated the columns; an adopted array may have changed since)
    }
}

template <class T> __device__ __forceinline__ T adj_value(T v, int) { return v; }
template <> __device__ __forceinline__ cplx adj_value<cplx>(cplx v, int conj) { return conj ? cplx{v.re, -v.im} : v; }
template <> __device__ __forceinline__ cplxf adj_value<cplxf>(cplxf v, int conj) { return conj ? cplxf{v.re, -v.im} : v; }

// entry j of the result = entry ent[j] of A: its column is the source row, the largest r with row_ptr[r] <= ent[j]
template <class T>
__global__ __launch_bounds__(BLOCK) void adj_fill_kernel(int64_t nnz, int64_t nrows, int conj, const int32_t *__restrict__ row_ptr,
                                                         const int32_t *__restrict__ ent, const T *__restrict__ val,
                                                         int32_t *__restrict__ col_out, T *__restrict__ val_out) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * BLOCK) {
        const int32_t k = ent[j];
        int64_t lo = 0, hi = nrows - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (row_ptr[mid] <= k) lo = mid; else hi = mid - 1;
        }
        col_out[j] = (int32_t)lo;
        val_out[j] = adj_value<T>(val[k], conj);
    }
}

// the three passes on raw arrays (internal.hpp, adjoint_dev)
template <class T>
int adjoint_arrays(sprs_ctx *c, const char *who, int64_t nr, int64_t nc, int64_t nnz, const int32_t *a_rp, const int32_t *a_ci, const T *a_v, int conj,
                   int32_t **rp_out, int32_t **ci_out, T **v_out) {
    *rp_out = nullptr; *ci_out = nullptr; *v_out = nullptr;
    const int grid = (int)std::min<int64_t>(std::max<int64_t>((nnz + BLOCK - 1) / BLOCK, 1), 4 * (int64_t)grid_for(c));
    DevBufs tmp;
    int32_t *cnt, *rp, *ci, *key, *ent, *key_s, *ent_s;
    T *vv;
    SPRS_TRY(tmp.alloc(c, &cnt, (size_t)nc + 1));
    SPRS_TRY(tmp.alloc(c, &rp, (size_t)nc + 1));
    SPRS_TRY(tmp.alloc(c, &ci, (size_t)nnz));
    SPRS_TRY(tmp.alloc(c, &vv, (size_t)nnz));
    SPRS_TRY(tmp.alloc(c, &key, (size_t)nnz));
    SPRS_TRY(tmp.alloc(c, &ent, (size_t)nnz));
    SPRS_TRY(tmp.alloc(c, &key_s, (size_t)nnz));
    SPRS_TRY(tmp.alloc(c, &ent_s, (size_t)nnz));
    // count
    SPRS_HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)nc + 1), c->stream));
    if (nnz > 0) {
        hipLaunchKernelGGL(adj_count_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, nnz, nc, a_ci, cnt, key, ent);
        SPRS_HIP_TRY(c, hipGetLastError());
    }
    // scan: row_ptr of the result (nc + 1 entries, the last one = nnz)
    size_t scan_bytes = 0, sort_bytes = 0;
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, cnt, rp, (int32_t)0, (size_t)nc + 1, rocprim::plus<int32_t>(), c->stream));
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) < nc) ++bits;              // the columns' significant bits
    if (nnz > 0)
        SPRS_HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, key, key_s, ent, ent_s, (size_t)nnz, 0u, (unsigned int)bits, c->stream));
    char *scratch;
    SPRS_TRY(tmp.alloc(c, &scratch, std::max(scan_bytes, sort_bytes)));
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, scan_bytes, cnt, rp, (int32_t)0, (size_t)nc + 1, rocprim::plus<int32_t>(), c->stream));
    int32_t total = -1;
    SPRS_HIP_TRY(c, hipMemcpyAsync(&total, rp + nc, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((int64_t)total != nnz) {
        snprintf(c->err, sizeof(c->err), "%s: %lld of %lld column indices are outside [0, %lld)", who, (long long)(nnz - total), (long long)nnz, (long long)nc);
        return SPRS_INVALID_ARGUMENT;
    }
    // fill
    if (nnz > 0) {
        SPRS_HIP_TRY(c, rocprim::radix_sort_pairs(scratch, sort_bytes, key, key_s, ent, ent_s, (size_t)nnz, 0u, (unsigned int)bits, c->stream));
        hipLaunchKernelGGL((adj_fill_kernel<T>), dim3(grid), dim3(BLOCK), 0, c->stream, nnz, nr, conj, a_rp, ent_s, a_v, ci, vv);
        SPRS_HIP_TRY(c, hipGetLastError());
    }
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    tmp.release(rp); tmp.release(ci); tmp.release(vv);                 // (the sort's 16 bytes per entry, the counts and rocprim's scratch go here)
    *rp_out = rp; *ci_out = ci; *v_out = vv;
    return SPRS_OK;
}

template <class T, class CT>
int adjoint_typed(const sprs_csr *A, int conj, int (*create_dev)(sprs_ctx *, int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const CT *, int, sprs_csr **),
                  sprs_csr **out) {
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    const int64_t nr = A->nrows, nc = A->ncols, nnz = A->nnz;
    int32_t *rp, *ci;
    T *vv;
    SPRS_TRY(adjoint_arrays<T>(c, "sprs_csr_adjoint", nr, nc, nnz, A->row_ptr, A->col_idx, reinterpret_cast<const T *>(A->val), conj, &rp, &ci, &vv));
    DevBufs own;                                                       // released if creation fails
    own.p = {(void *)rp, (void *)ci, (void *)vv};
    sprs_csr *H = nullptr;
    SPRS_TRY(create_dev(c, nc, nr, nnz, rp, ci, reinterpret_cast<const CT *>(vv), 1, &H));
    H->owns_arrays = true;                                             // adopted, and from here on released with the handle
    own.p.clear();
    *out = H;
    return SPRS_OK;
}

}  // namespace

namespace sprs {

template <class T>
int adjoint_dev(sprs_ctx *c, const char *who, int64_t nr, int64_t nc, int64_t nnz, const int32_t *a_rp, const int32_t *a_ci, const T *a_v, int conj,
                int32_t **rp_out, int32_t **ci_out, T **v_out) {
    return adjoint_arrays<T>(c, who, nr, nc, nnz, a_rp, a_ci, a_v, conj, rp_out, ci_out, v_out);
}
#define SPRS_ADJOINT_INST(T)                                                                                                              \
    template int adjoint_dev<T>(sprs_ctx *, const char *, int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const T *, int, \
                                int32_t **, int32_t **, T **);
SPRS_ADJOINT_INST(double)
SPRS_ADJOINT_INST(cplx)
SPRS_ADJOINT_INST(float)
SPRS_ADJOINT_INST(cplxf)

}  // namespace sprs

extern "C" {

int sprs_csr_adjoint(const sprs_csr *A, int conjugate, sprs_csr **out) {
    if (!A || !out) return SPRS_INVALID_ARGUMENT;
    *out = nullptr;
    SPRS_TRY(single_gpu_only(A, "sprs_csr_adjoint"));
    try {
        switch (A->dtype) {
            case DT_D: return adjoint_typed<double, double>(A, 0, sprs_csr_create_dev_d, out);
            case DT_Z: return adjoint_typed<cplx, sprs_c64>(A, conjugate != 0, sprs_csr_create_dev_z, out);
            case DT_S: return adjoint_typed<float, float>(A, 0, sprs_csr_create_dev_s, out);
            case DT_C: return adjoint_typed<cplxf, sprs_c32>(A, conjugate != 0, sprs_csr_create_dev_c, out);
        }
    } catch (...) { return SPRS_ERR_HIP; }
    return SPRS_INVALID_ARGUMENT;
}

}  // extern "C"
