/* sprsolve_hip.h — C ABI of the MI355X (gfx950) backend for sprsolve's Krylov hot path.
 *
 * This is the drop-in boundary.  It exports exactly what a Rust FFI for the
 * path would bind: an opaque device CSR operator that implements the `MatVecMul` trait
 * (reference src/mat.rs:12-37; in-tree precedent for an opaque backend handle:
 * src/mkl_mat.rs:15-149,322-333), the BLAS-1 kernels of src/vecalg.rs on device vectors, the
 * Jacobi preconditioner of src/precond.rs, and the three solver objects with the reference's
 * `new` / `solve` / `precond_solve` signatures (src/bicg_stab.rs:25,35,204; src/minres.rs:21,31,
 * 178; src/cs_minres.rs:19,29).  Plain pointers and sizes only; nothing throws or aborts
 * across this boundary.  The reference-side binding is shown in INTEGRATION.md.
 *
 * Suffix convention:  _d = f64,  _z = Complex<f64> (layout {re, im} = num_complex::Complex<f64>
 * repr(C) = double2),  _zd = complex vector with a real scalar/diagonal;  _s / _c / _cs are the same
 * for f32 / Complex<f32> (declared in one block further down).
 * "host" pointers are ordinary CPU memory; "dev" pointers are HIP device memory on the
 * context's GPU.  All calls are blocking from the caller's view unless stated otherwise.
 */
#ifndef SPRSOLVE_HIP_H
#define SPRSOLVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double re, im; } sprs_c64;   /* Complex<f64> */
typedef struct { float re, im; } sprs_c32;    /* Complex<f32> */

/* Status codes. 1..5 map 1:1 onto reference src/error.rs:7-22 `SolverError`; 6 is the
 * `panic!("Dimension mismatch")` of src/mat.rs:50-52,58-60 and src/precond.rs:39-41. */
enum {
    SPRS_OK = 0,
    SPRS_INCOMPATIBLE_RHS_SIZE = 1, /* IncompatibleMatrixFormat("Input vec dimension doesn't match the matrix size") bicg_stab.rs:44-48 */
    SPRS_INCOMPATIBLE_X_SIZE = 2,   /* IncompatibleMatrixFormat("Input and output vec dimension do not match")       bicg_stab.rs:49-53 */
    SPRS_INSUFFICIENT_ITER = 3,     /* InsufficientIterNum(max_iter)  bicg_stab.rs:199  (*its_out = max_iter) */
    SPRS_BREAKDOWN = 4,             /* BreakDown(its)                 bicg_stab.rs:164-167 (*its_out = its) */
    SPRS_INVALID_PRECOND = 5,       /* InvalidPreconditioner(..)      minres.rs:236-244,279-287 (*its_out = its, *res_out = re(beta^2)) */
    SPRS_DIM_MISMATCH = 6,          /* panic!("Dimension mismatch")   mat.rs:50-52 */
    SPRS_INVALID_ARGUMENT = 7,      /* null handle, index out of i32 range, malformed CSR */
    SPRS_ZERO_DIAGONAL = 8,         /* ZeorDiagonalElem(row)          gauss_seidel.rs:72-78 (*its_out = row) */
    SPRS_NOT_SQUARE = 9,            /* IncompatibleMatrixFormat("Not a square matrix")  gauss_seidel.rs:16-20 */
    SPRS_NOT_CSR = 10,              /* IncompatibleMatrixFormat("Not in CSR format")    gauss_seidel.rs:22-26 */
    SPRS_ERR_HIP = 100,             /* a HIP runtime call failed; see sprs_last_error() */
    SPRS_ERR_RCCL = 101,            /* an RCCL call failed */
    SPRS_ERR_NO_DEVICE = 102        /* no usable gfx950 device */
};

typedef struct sprs_ctx sprs_ctx;           /* one GPU + one HIP stream + reduction scratch */
typedef struct sprs_csr sprs_csr;           /* device CSR operator: impl MatVecMul (mat.rs:47-153) */
typedef struct sprs_diag sprs_diag;         /* DiagPrecond<T,V>              (precond.rs:6-63)  */
typedef struct sprs_bicgstab sprs_bicgstab; /* BiCGStab<T,M>                 (bicg_stab.rs:17-31) */
typedef struct sprs_minres sprs_minres;     /* MinRes<T,M>                   (minres.rs:13-27)    */
typedef struct sprs_csminres sprs_csminres; /* CSMinRes<T,M>                 (cs_minres.rs:11-25) */
typedef struct sprs_cg sprs_cg;             /* conjugate gradients (no reference analogue; "conjugate gradients" below) */
typedef struct sprs_lsmr sprs_lsmr;         /* LSMR least squares on any A, rectangular included ("LSMR" below) */
typedef struct sprs_cg_many sprs_cg_many;   /* conjugate gradients on several right-hand sides at once ("several right-hand sides" below) */
typedef struct sprs_cg_shift sprs_cg_shift; /* conjugate gradients on (A + sigma_j I) x_j = rhs for several shifts at once ("shifted systems" below) */
typedef struct sprs_gmres sprs_gmres;       /* restarted GMRES (no reference analogue; "restarted GMRES" below) */
typedef struct sprs_idrs sprs_idrs;         /* IDR(s) for non-symmetric systems (no reference analogue; "IDR(s)" below) */
typedef struct sprs_comm sprs_comm;        /* RCCL communicator of this rank (multi-GPU section)  */
typedef struct sprs_gauss_seidel sprs_gauss_seidel; /* GaussSeidel<T>        (gauss_seidel.rs:8-31) */
/* sprs_ilu0, the ILU(0) preconditioner handle, is declared with its section ("ILU(0) preconditioner" below) */

/* ---------------------------------------------------------------- context */
/* device: HIP device ordinal.  stream: an existing hipStream_t to run on (e.g. the caller's
 * framework stream), or NULL to create a private one. */
int sprs_ctx_create(int device, void *stream, sprs_ctx **out);
int sprs_ctx_destroy(sprs_ctx *ctx);               /* NULL is a no-op */
int sprs_ctx_sync(sprs_ctx *ctx);
const char *sprs_last_error(const sprs_ctx *ctx);  /* text of the last SPRS_ERR_* on this ctx, and of a SPRS_INVALID_ARGUMENT that
                                                      says why ("sprs_<entry>: <text>"; every sprs_*_create_* of a solver says so
                                                      where the operator holds another scalar type than its suffix) */
const char *sprs_status_str(int status);
int sprs_version(void);
/* Tuning knobs.  Defaults are the measured best on MI355X (profiles/r0*_tuning.md); none changes a result except through
 * the summation order of the fused reductions' partials (y of every SpMV is bit-identical under all of them).
 * -1 = automatic where noted.  Knobs marked (creation) are read when a matrix handle is created.
 *   "grid"          workgroups of the streaming (BLAS-1 / fused recurrence) kernels, 8..4096, multiple of 8
 *   "spmv_grid"     workgroups of the SpMV kernels (-1: 4 per CU)
 *   "poll"          iterations between two host looks at the device-side status word (>= 1)
 *   "stream_nt"     fused recurrence kernels read and write their vectors, and the pair-code SpMV writes y, with
 *                   non-temporal accesses: -1 automatic (vectors of 72 MB and more), 0 / 1
 *   "xcd_chunk"     1: one contiguous chunk of row blocks per XCD (-1: automatic — cache-resident matrices only)
 *   "ew_chunk"      fused recurrence kernels walk one contiguous eighth of the vectors per XCD, the eighth whose rows
 *                   that XCD multiplies: -1 automatic (cache-resident matrices whose far band is at most 1/32 of
 *                   the rows), 0 / 1
 *   "spmv_dict"     SpMV stream: -1 auto / 0 plain CSR / 1 offset codes / 2 (offset, value) pair codes
 *                   (sprs_csr_stream_format reports what a handle got)                                   (creation)
 *   "spmv_wide"     f64 pair codes: two rows per lane, 128-row blocks (-1 / 1 on, 0 off)
 *   "spmv_uniform"  blocks whose rows repeat one code sequence are multiplied from that pattern          (creation)
 *   "spmv_triple"   ... and read columns c - 1, c + 1 of a column triple from column c's loads           (creation)
 *   "spmv_seam"     ... and so are blocks that are uniform but for one row, or two adjacent ones, holding only
 *                   part of the pattern or one entry of their own (line seams of truncated / Dirichlet grids) (creation)
 *   "spmv_tile"     f64 compressed streams: runs of 4096 rows of one stencil pattern are multiplied from an x window
 *                   staged in LDS (near columns) + per-row-pair far loads, one launch with the remaining blocks:
 *                   -1 automatic = vectors of 44 MiB and more, 1 = every matrix with such runs, 0 = off
 *                   (sprs_csr_tile_plan reports what a handle got)                       (creation; 0 also at launch)
 *   "spmv_chain"    f64 pair codes, patterns with one far slot a side at -P / +P (3-D stencils): a workgroup walks a
 *                   column of 2048-row tiles plane by plane with the x windows of three consecutive tiles in LDS — no far
 *                   load at all: -1 automatic = wherever "spmv_tile" applies and the chains fill the chip, 1 = wherever
 *                   chains exist, 0 = off (sprs_csr_chain_plan reports what a handle got)  (creation; 0 also at launch)
 *   "spmv_fuse"     BiCGStab, f64, no preconditioner, one GPU, SpMV through chains: the vector updates that produce an SpMV's
 *                   input (r -= alpha v before t = A r; p = (v (-beta w) + p beta) + r before v = A p) are formed inside that
 *                   SpMV — three launches per iteration instead of five, every scalar and element bit-identical; 0 = off (per solve).
 *                   MINRES / CSMINRES, no preconditioner, one GPU, SpMV through the lane-per-row kernel of a compressed stream
 *                   (f64 offset codes, complex offset / pair codes): the third kernel of an iteration (normalisation, Givens
 *                   rotation, p, x, convergence test) is not launched — the next SpMV multiplies by the un-normalised vector
 *                   scaled in its gathers and the element-wise work rides with the next iteration's second kernel: two launches
 *                   instead of three, fewer vector passes, bit-identical
 *   "bicg_k5"       BiCGStab where "spmv_fuse" applies: the last update of an iteration (x, r' = s - w t, |r'|^2, r0.r') walks the
 *                   chains as the SpMV before it did, with s in its windows.  1 = that SpMV (t = A s) keeps its two dots and stores
 *                   nothing, the update folds t again for its own rows (the same bits); 2 = t is stored and loaded as before, the update
 *                   walks the chains all the same (the two agree bit for bit); 0 = the update is the vector kernel.  With 1 and 2 the
 *                   update's two dots are grouped by the chain walk: scalars and x differ from 0's in summation order only.
 *                   -1 automatic = 1 while "spmv_fuse" is automatic too, 0 once "spmv_fuse" has been set (1 there means the flow
 *                   that is bit-identical to 0) (per solve)
 *   "p2p_allreduce" distributed solves: the scalar hand-offs go through peer-to-peer mailboxes (no stream operation) instead of
 *                   ncclAllReduce: -1 / 1 wherever the communicator has them (sprs_comm_p2p), 0 = RCCL
 *                   (communicator creation: 0 sets none up; per solve)
 *   "p2p_timeout_ms" how long a consumer kernel polls its mailbox before the solve fails with SPRS_ERR_RCCL (default 20000)
 *   "spmv_eqrows"   plain CSR: blocks of equal-length rows do not read row_ptr                           (creation)
 *   "spmv_wideload" plain CSR, f64: 16-byte stream loads (4 entries per lane), 3 workgroups per CU on HBM-sized
 *                   matrices; 0 = the kernel with 4- / 8-byte loads                                      (creation)
 *   "spmv_period"   XCD-period walk of the compressed streams' blocks for matrices with a far band (rows r and
 *                   r +- band on one XCD): -1 automatic = the f64 pair-code stream (cfg 5: SpMV -2.3 %),
 *                   1 = the offset-code stream too (measured slower), 0 = off                            (creation)
 *   "halo_overlap"  distributed SpMV: 1 (default) multiplies the interior rows while the halo travels
 *   "gs_graph"      1: Gauss-Seidel replays a sweep's level launches from a hipGraph (default 0)
 * sprs_ctx_get also answers "num_cu" and "device".  Unknown key: SPRS_INVALID_ARGUMENT / -1. */
int sprs_ctx_set(sprs_ctx *ctx, const char *key, int64_t value);
int64_t sprs_ctx_get(const sprs_ctx *ctx, const char *key);

/* device memory for callers that have no HIP of their own (a Rust host) */
int sprs_malloc(sprs_ctx *ctx, size_t bytes, void **dev_out);
int sprs_free(sprs_ctx *ctx, void *dev);
int sprs_memcpy_h2d(sprs_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int sprs_memcpy_d2h(sprs_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
int sprs_memcpy_d2d(sprs_ctx *ctx, void *dev_dst, const void *dev_src, size_t bytes); /* ptr::copy_nonoverlapping, bicg_stab.rs:78 */
int sprs_memset_zero(sprs_ctx *ctx, void *dev, size_t bytes);                          /* iter_mut().for_each(zero), minres.rs:86-88 */

/* ---------------------------------------------------------------- CSR operator (MatVecMul) */
/* Create from host arrays (copied to HBM; the caller keeps its own copy — cf. MklMat::new,
 * mkl_mat.rs:32-74).  Index types of mat.rs:196-199: i32 natively; i64 covers u32/u64/usize by
 * narrowing with a range check (SPRS_INVALID_ARGUMENT if anything exceeds i32).
 * `storage_csc` != 0: the arrays are CSC (mat.rs:130-142); converted to CSR once at creation. */
int sprs_csr_create_d(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *row_ptr,
                      const int32_t *col_idx, const double *val, int storage_csc, sprs_csr **out);
int sprs_csr_create_z(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *row_ptr,
                      const int32_t *col_idx, const sprs_c64 *val, int storage_csc, sprs_csr **out);
int sprs_csr_create_i64_d(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t *row_ptr,
                          const int64_t *col_idx, const double *val, int storage_csc, sprs_csr **out);
int sprs_csr_create_i64_z(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t *row_ptr,
                          const int64_t *col_idx, const sprs_c64 *val, int storage_csc, sprs_csr **out);
/* Create from arrays already resident in HBM (CSR, i32).  adopt == 0: copied; adopt != 0: the
 * handle references the caller's arrays, which must outlive it (no copy of multi-GB matrices) and must not
 * be modified while the handle lives: like mkl_sparse_optimize (mkl_mat.rs:81-148), creation analyses the
 * matrix once and keeps what it derived (row blocks, the compressed code stream of sprs_csr_stream_format). */
int sprs_csr_create_dev_d(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *dev_row_ptr,
                          const int32_t *dev_col_idx, const double *dev_val, int adopt, sprs_csr **out);
int sprs_csr_create_dev_z(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *dev_row_ptr,
                          const int32_t *dev_col_idx, const sprs_c64 *dev_val, int adopt, sprs_csr **out);
int sprs_csr_destroy(sprs_csr *A); /* Drop, mkl_mat.rs:322-333; NULL is a no-op */
int64_t sprs_csr_rows(const sprs_csr *A);
int64_t sprs_csr_cols(const sprs_csr *A);
int64_t sprs_csr_nnz(const sprs_csr *A);
/* Which stream the SpMV of this handle reads (backend detail, csrc/spmv_dict.hip): 0 = plain CSR (12 B/nnz for
 * f64), 1 = one-byte column-offset codes + the values (9 B/nnz), 2 = one-byte codes of the (offset, value) pairs
 * (1 B/nnz).  The compressed streams are built at creation when the matrix has <= 256 distinct (col - row) offsets
 * (and, for real scalars, <= 256 distinct values and pairs; for complex scalars <= 255 distinct (offset, value) pairs
 * among the entries OFF the diagonal — the offset-0 entries are kept one per row, 16 B per row for Complex<f64>) and
 * the ctx knob "spmv_dict" allows it; y is bit-identical in all three.  Automatic policy: pair codes where they
 * exist; else offset codes for real scalars and the plain stream for complex ones.  n_offsets / n_pairs (may be
 * NULL) receive the table sizes (0 = table absent; complex pair codes count the row-value slot as one pair). */
int sprs_csr_stream_format(const sprs_csr *A, int *n_offsets, int *n_pairs);
/* Diagnostics of the compressed streams: the number of row blocks the SpMV of this handle walks (128-row blocks of
 * the f64 pair-code stream, 64-row blocks of the offset-code stream) and how many of them are "uniform" (all rows
 * repeat one code sequence: multiplied from a scalar pattern, no code bytes and no row_ptr read).  Plain stream: its
 * 64-row blocks and how many of them hold rows of equal length (row extents from the descriptor, no row_ptr read).
 * Copies the descriptors to the host: not for hot paths. */
int sprs_csr_wide_blocks(const sprs_csr *A, int64_t *n_blocks, int64_t *n_uniform);
/* Diagnostics of the f64 pair-code stream's LDS-window tiles (ctx knob "spmv_tile", csrc/spmv_dict.hip): how many tiles
 * the SpMV of this handle multiplies from an x window staged in LDS, how many 128-row blocks they cover, and how many
 * 128-row blocks the same launch walks one by one.  All zero when the handle has no tile plan (other streams, matrices
 * without long runs of one stencil pattern, cache-resident matrices under the automatic policy). */
int sprs_csr_tile_plan(const sprs_csr *A, int64_t *n_tiles, int64_t *n_tile_blocks, int64_t *n_other_blocks);
/* ... and of its plane-streaming chains (ctx knob "spmv_chain", csrc/spmv_chain.hip), which take precedence over the tiles
 * where a handle has both (sprs_csr_tile_plan then reports zeros): chain tiles (2048 rows each), chain segments (the work
 * items, about one per workgroup), chains, and the 128-row blocks the same launch walks one by one.  All zero otherwise. */
int sprs_csr_chain_plan(const sprs_csr *A, int64_t *n_tiles, int64_t *n_segments, int64_t *n_chains, int64_t *n_other_blocks);
/* Diagnostics: the kernel the next SpMV launch of this handle takes, as csrc/spmv.hip's routing function decides it now
 * (the launch-time ctx knobs are read at the call).  part 0: the whole matrix; 1 / 2: the interior / boundary launch of a
 * distributed operator that was split at creation — *kernel = -1 (and zeros) when the handle has no such split.
 * *kernel: 0 Csr, 1 CsrWide, 2 Dict, 3 DictWide, 4 Pair2, 5 TilePair, 6 TileOff, 7 Chain (the order of SpmvKernel in
 * csrc/internal.hpp); *format: 0 plain, 1 offset codes, 2 pair codes; *grid: workgroups = dot partials of the launch;
 * *n_blocks: row blocks it walks; *ordered: 1 when it walks them through an order list (XCD-period order, the subsets of
 * a split operator); *y_nt: 1 when the route asks for non-temporal y stores (CsrWide and Pair2 honour it). */
int sprs_csr_spmv_route(const sprs_csr *A, int part, int conj_x, int *kernel, int *format, int *grid, int64_t *n_blocks,
                        int *ordered, int *y_nt);

/* MatVecMul::mul_vec / mul_vec_dot (mat.rs:49-64): host slices, checked — returns
 * SPRS_DIM_MISMATCH where the reference panics.  y = A x ; *dot_out = conj(x) . y
 * Thread-safety (bicg_stab.rs:17-18 `T: Send + Sync`, `A: &M` shared): the handle is immutable after creation and
 * every entry point that uses per-context or per-handle scratch — the host-slice mul_vec / mul_vec_dot (staging
 * buffers), everything that returns a scalar, handle creation, all solves — takes the context's mutex, so concurrent
 * `&self` calls on one handle from several host threads are safe: they queue (one context = one stream; use one
 * context per thread for concurrency).  tests/test_gpu_threads.py.  The asynchronous device-pointer entry points
 * (sprs_mul_vec_dev_*, element-wise vecalg) touch no shared scratch; sprs_last_error is last-writer-wins. */
int sprs_mul_vec_d(const sprs_csr *A, const double *x_host, size_t x_len, double *y_host, size_t y_len);
int sprs_mul_vec_z(const sprs_csr *A, const sprs_c64 *x_host, size_t x_len, sprs_c64 *y_host, size_t y_len);
int sprs_mul_vec_dot_d(const sprs_csr *A, const double *x_host, size_t x_len, double *y_host, size_t y_len, double *dot_out);
int sprs_mul_vec_dot_z(const sprs_csr *A, const sprs_c64 *x_host, size_t x_len, sprs_c64 *y_host, size_t y_len, sprs_c64 *dot_out);
/* MatVecMul::mul_vec_unchecked / mul_vec_dot_unchecked (mat.rs:68-152) on device vectors:
 * no dimension check, no PCIe traffic.  x_dev has ncols elements, y_dev nrows.  sprs_mul_vec_dev_* and the
 * element-wise vecalg entry points below are ASYNCHRONOUS on the context's stream (sprs_ctx_sync to wait);
 * entry points that return a scalar, and all solves, block. */
int sprs_mul_vec_dev_d(const sprs_csr *A, const double *x_dev, double *y_dev);
int sprs_mul_vec_dev_z(const sprs_csr *A, const sprs_c64 *x_dev, sprs_c64 *y_dev);
int sprs_mul_vec_dot_dev_d(const sprs_csr *A, const double *x_dev, double *y_dev, double *dot_out);
int sprs_mul_vec_dot_dev_z(const sprs_csr *A, const sprs_c64 *x_dev, sprs_c64 *y_dev, sprs_c64 *dot_out);
/* Launch `reps` back-to-back SpMVs bracketed by HIP events on the context's stream and
 * return the mean device time of one launch in milliseconds (roofline measurement). */
int sprs_mul_vec_dev_timed_d(const sprs_csr *A, const double *x_dev, double *y_dev, int reps, double *ms_per_launch);
int sprs_mul_vec_dev_timed_z(const sprs_csr *A, const sprs_c64 *x_dev, sprs_c64 *y_dev, int reps, double *ms_per_launch);

/* ---------------------------------------------------------------- vecalg (src/vecalg.rs) on device vectors */
int sprs_dot_d(sprs_ctx *ctx, size_t n, const double *x, const double *y, double *out);            /* vecalg.rs:24,556  sum x*y (no conj) */
int sprs_dot_z(sprs_ctx *ctx, size_t n, const sprs_c64 *x, const sprs_c64 *y, sprs_c64 *out);
int sprs_conj_dot_d(sprs_ctx *ctx, size_t n, const double *x, const double *y, double *out);       /* vecalg.rs:51,563  sum conj(x)*y */
int sprs_conj_dot_z(sprs_ctx *ctx, size_t n, const sprs_c64 *x, const sprs_c64 *y, sprs_c64 *out);
int sprs_norm2_d(sprs_ctx *ctx, size_t n, const double *x, double *out);                           /* vecalg.rs:63,601  sqrt(sum |x|^2), unscaled */
int sprs_norm2_z(sprs_ctx *ctx, size_t n, const sprs_c64 *x, double *out);
int sprs_scale_d(sprs_ctx *ctx, size_t n, double a, double *x);                                    /* vecalg.rs:74,592  x *= a */
int sprs_scale_z(sprs_ctx *ctx, size_t n, sprs_c64 a, sprs_c64 *x);
int sprs_rscale_d(sprs_ctx *ctx, size_t n, double a, double *x);                                   /* vecalg.rs:86,596  x = x.mul_real(a) */
int sprs_rscale_z(sprs_ctx *ctx, size_t n, double a, sprs_c64 *x);
int sprs_conj_d(sprs_ctx *ctx, size_t n, const double *in, double *out);                           /* vecalg.rs:96,577  out = conj(in) */
int sprs_conj_z(sprs_ctx *ctx, size_t n, const sprs_c64 *in, sprs_c64 *out);
int sprs_axpy_d(sprs_ctx *ctx, size_t n, double a, const double *x, double *y);                    /* vecalg.rs:109,570 y += x*a */
int sprs_axpy_z(sprs_ctx *ctx, size_t n, sprs_c64 a, const sprs_c64 *x, sprs_c64 *y);
int sprs_axpy_zd(sprs_ctx *ctx, size_t n, double a, const sprs_c64 *x, sprs_c64 *y);               /* S = f64, T = Complex<f64> (vecalg.rs:746-757) */
int sprs_axpby_d(sprs_ctx *ctx, size_t n, double a, const double *x, double b, double *y);         /* vecalg.rs:135,585 y = x*a + y*b */
int sprs_axpby_z(sprs_ctx *ctx, size_t n, sprs_c64 a, const sprs_c64 *x, sprs_c64 b, sprs_c64 *y);

/* ---------------------------------------------------------------- Jacobi preconditioner (src/precond.rs) */
/* DiagPrecond::new(diag): stores 1/diag (precond.rs:20-29; no zero check, as in the reference). */
int sprs_diag_precond_create_d(sprs_ctx *ctx, size_t n, const double *diag_host, sprs_diag **out);    /* DiagPrecond<f64,f64> */
int sprs_diag_precond_create_zd(sprs_ctx *ctx, size_t n, const double *diag_host, sprs_diag **out);   /* DiagPrecond<Complex64,f64>       (tests/test_complex_solve.rs:44) */
int sprs_diag_precond_create_z(sprs_ctx *ctx, size_t n, const sprs_c64 *diag_host, sprs_diag **out);  /* DiagPrecond<Complex64,Complex64> (tests/test_complex_solve2.rs:10) */
int sprs_diag_precond_destroy(sprs_diag *P);
/* MatVecMul::mul_vec for DiagPrecond (precond.rs:37-52): host slices, checked */
int sprs_diag_mul_vec_d(const sprs_diag *P, const double *in_host, size_t in_len, double *out_host, size_t out_len);
int sprs_diag_mul_vec_z(const sprs_diag *P, const sprs_c64 *in_host, size_t in_len, sprs_c64 *out_host, size_t out_len);
/* mul_vec_unchecked on device vectors */
int sprs_diag_mul_vec_dev_d(const sprs_diag *P, const double *in_dev, double *out_dev);
int sprs_diag_mul_vec_dev_z(const sprs_diag *P, const sprs_c64 *in_dev, sprs_c64 *out_dev);

/* ---------------------------------------------------------------- solvers */
/* Common contract (bicg_stab.rs:35-41):  rhs read-only, x in/out (initial guess -> solution),
 * returns a status; on SPRS_OK (*its_out, *res_out) is the reference's Ok((iters, rel_residual)).
 * `*_solve_*`      : rhs/x are host slices (one H2D + one D2H per solve, all iteration state in HBM).
 * `*_solve_dev_*`  : rhs/x are device vectors (nothing crosses PCIe).
 * The solver borrows A (and the preconditioner) — they must outlive it (bicg_stab.rs:18) — and
 * owns its 7n/8n-element workspace, reused across solves (bicg_stab.rs:28).  One in-flight solve
 * per solver handle (`&mut self`). */
int sprs_bicgstab_create_d(const sprs_csr *A, size_t size, sprs_bicgstab **out);   /* BiCGStab::new  bicg_stab.rs:25 */
int sprs_bicgstab_create_z(const sprs_csr *A, size_t size, sprs_bicgstab **out);
int sprs_bicgstab_destroy(sprs_bicgstab *S);
int sprs_bicgstab_solve_d(sprs_bicgstab *S, const double *rhs, size_t rhs_len, double *x, size_t x_len,
                          size_t max_iter, double tol, size_t *its_out, double *res_out);            /* bicg_stab.rs:35-200 */
int sprs_bicgstab_solve_z(sprs_bicgstab *S, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len,
                          size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bicgstab_precond_solve_d(sprs_bicgstab *S, const sprs_diag *P, const double *rhs, size_t rhs_len, double *x,
                                  size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out); /* bicg_stab.rs:204-366 */
int sprs_bicgstab_precond_solve_z(sprs_bicgstab *S, const sprs_diag *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x,
                                  size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bicgstab_solve_dev_d(sprs_bicgstab *S, const sprs_diag *P_or_null, const double *rhs_dev, size_t rhs_len,
                              double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bicgstab_solve_dev_z(sprs_bicgstab *S, const sprs_diag *P_or_null, const sprs_c64 *rhs_dev, size_t rhs_len,
                              sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);

int sprs_minres_create_d(const sprs_csr *A, size_t size, sprs_minres **out);       /* MinRes::new  minres.rs:21 */
int sprs_minres_create_z(const sprs_csr *A, size_t size, sprs_minres **out);
int sprs_minres_destroy(sprs_minres *S);
int sprs_minres_solve_d(sprs_minres *S, const double *rhs, size_t rhs_len, double *x, size_t x_len,
                        size_t max_iter, double tol, size_t *its_out, double *res_out);              /* minres.rs:31-172 */
int sprs_minres_solve_z(sprs_minres *S, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len,
                        size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_minres_precond_solve_d(sprs_minres *S, const sprs_diag *P, const double *rhs, size_t rhs_len, double *x,
                                size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out); /* minres.rs:178-341 */
int sprs_minres_precond_solve_z(sprs_minres *S, const sprs_diag *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x,
                                size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_minres_solve_dev_d(sprs_minres *S, const sprs_diag *P_or_null, const double *rhs_dev, size_t rhs_len,
                            double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_minres_solve_dev_z(sprs_minres *S, const sprs_diag *P_or_null, const sprs_c64 *rhs_dev, size_t rhs_len,
                            sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);

int sprs_csminres_create_z(const sprs_csr *A, size_t size, sprs_csminres **out);   /* CSMinRes::new  cs_minres.rs:19 */
int sprs_csminres_create_d(const sprs_csr *A, size_t size, sprs_csminres **out);   /* generic over T: real T degenerates to MINRES arithmetic */
int sprs_csminres_destroy(sprs_csminres *S);
int sprs_csminres_solve_z(sprs_csminres *S, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len,
                          size_t max_iter, double tol, size_t *its_out, double *res_out);            /* cs_minres.rs:29-158 */
int sprs_csminres_solve_d(sprs_csminres *S, const double *rhs, size_t rhs_len, double *x, size_t x_len,
                          size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_csminres_solve_dev_z(sprs_csminres *S, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len,
                              size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_csminres_solve_dev_d(sprs_csminres *S, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len,
                              size_t max_iter, double tol, size_t *its_out, double *res_out);

/* ---------------------------------------------------------------- Gauss-Seidel (src/gauss_seidel.rs)
 * `GaussSeidel::new(A.view())` / `::solve(rhs, x, max_iter, eps)`; real scalars only (the reference bounds
 * T: PartialOrd).  The serial sweep is made data-parallel by dependency levels (rows of one level per launch)
 * without changing its arithmetic: x after k sweeps is bit-identical to the reference's.  On SPRS_OK
 * (*its_out, *res_out) = Ok((iters, ABSOLUTE residual norm)) exactly as gauss_seidel.rs:107,136 return them.
 * create: SPRS_NOT_SQUARE / SPRS_NOT_CSR (the handle was built from CSC arrays) as the reference's `new`. */
int sprs_gauss_seidel_create(const sprs_csr *A, sprs_gauss_seidel **out);
int sprs_gauss_seidel_destroy(sprs_gauss_seidel *G);
int64_t sprs_gauss_seidel_levels(const sprs_gauss_seidel *G);   /* number of dependency levels (launches per sweep) */
int sprs_gauss_seidel_solve_d(sprs_gauss_seidel *G, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double eps, size_t *its_out, double *res_out);
int sprs_gauss_seidel_solve_s(sprs_gauss_seidel *G, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float eps, size_t *its_out, float *res_out);
int sprs_gauss_seidel_solve_dev_d(sprs_gauss_seidel *G, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double eps, size_t *its_out, double *res_out);
int sprs_gauss_seidel_solve_dev_s(sprs_gauss_seidel *G, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float eps, size_t *its_out, float *res_out);

/* ---------------------------------------------------------------- conjugate gradients
 * For Hermitian positive-definite A (A == A^H, x^H A x > 0); neither property is checked — on another matrix the solve
 * ends in SPRS_BREAKDOWN, SPRS_INSUFFICIENT_ITER or a wrong answer.  The reference has no such solver; the conventions are its
 * BiCGStab's: relative residual against |rhs|, a zero right-hand side answers x = 0, x is in/out and is left modified on
 * error.  One SpMV and two dot products per iteration; the handle holds 4n of workspace (3n are used without a preconditioner).  P is the Jacobi
 * preconditioner (any of its (T, V) pairs); its size / scalar type are checked as for the other solvers.
 * All scalars are of type T, sign tests use the real part, conj_dot(a, b) = sum conj(a_i) b_i:
 *     rhs_norm = norm2(rhs);  if rhs_norm <= eps: x = 0, return SPRS_OK with *its_out = 0, *res_out = rhs_norm
 *     r = rhs*1 + (A x)*(-1);  if norm2(r) <= tol * rhs_norm: return SPRS_OK with *its_out = 0
 *     z = P r (z is r itself without P);  p = z;  rho = conj_dot(r, z)
 *     for its = 0 .. max_iter - 1:
 *         q = A p;  pq = conj_dot(p, q);  unless re(pq) > 0: SPRS_BREAKDOWN, *its_out = its  (also where pq is NaN)
 *         alpha = rho / pq;  x += p*alpha;  r += q*(-alpha)
 *         if norm2(r) <= tol * rhs_norm: SPRS_OK, *its_out = its + 1, *res_out = norm2(r) / rhs_norm
 *         z = P r;  rho_new = conj_dot(r, z);  with P, unless re(rho_new) > 0: SPRS_INVALID_PRECOND, *its_out = its,
 *                                                                               *res_out = re(rho_new)
 *         beta = rho_new / rho;  rho = rho_new;  p = z*1 + p*beta
 *     SPRS_INSUFFICIENT_ITER, *its_out = max_iter
 * So *its_out of SPRS_OK counts the SpMVs of the loop; of an error it is the 0-based iteration of the event.
 * SPRS_INCOMPATIBLE_RHS_SIZE / SPRS_INCOMPATIBLE_X_SIZE as for BiCGStab.  Trace row (sprs_solver_set_trace), one per iteration
 * that reached the p update: [its, r_norm, re(rho), im(rho), re(alpha), im(alpha), re(beta), im(beta)], rho = rho_new. */
int sprs_cg_create_d(const sprs_csr *A, size_t size, sprs_cg **out);
int sprs_cg_create_z(const sprs_csr *A, size_t size, sprs_cg **out);
int sprs_cg_destroy(sprs_cg *S);               /* NULL is a no-op */
int sprs_cg_solve_d(sprs_cg *S, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_cg_solve_z(sprs_cg *S, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_cg_precond_solve_d(sprs_cg *S, const sprs_diag *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_cg_precond_solve_z(sprs_cg *S, const sprs_diag *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
/* the same on device vectors (16-byte aligned ones are used in place) */
int sprs_cg_solve_dev_d(sprs_cg *S, const sprs_diag *P_or_null, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_cg_solve_dev_z(sprs_cg *S, const sprs_diag *P_or_null, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);

/* ---------------------------------------------------------------- the adjoint of an operator
 * sprs_csr_adjoint builds A^T (conjugate = 0) or A^H (conjugate != 0; the flag is ignored for real scalars) as an ordinary,
 * independent handle of shape ncols x nrows: it owns its arrays, outlives A, and every sprs_mul_vec_* / sprs_mul_mat_* / solver
 * entry point takes it like any other handle (it gets its row blocks, dictionary streams, tile and chain plans at creation).
 * Row j of the result holds the entries of column j of A in ascending original row; the entries of one row of A keep their
 * stored order, duplicates included; conjugation flips the sign of the imaginary part and nothing else.  These are exactly the
 * arrays sprs_csr_create_* builds from A's (row_ptr, col_idx, conjugated val) passed with storage_csc = 1 and the dimensions
 * swapped, so an SpMV through either handle has the same bits on every route.  The construction runs on the device only (count,
 * scan, stable key sort + gather: csrc/transpose.hip), so a matrix adopted in HBM never crosses PCIe; temporary device memory:
 * 16 bytes per entry + the result.  A distributed A: SPRS_INVALID_ARGUMENT (text in sprs_last_error). */
int sprs_csr_adjoint(const sprs_csr *A, int conjugate, sprs_csr **out);
/* The handle's CSR arrays copied to host memory (any pointer may be NULL): row_ptr nrows + 1 and col_idx nnz entries of int32_t,
 * val nnz entries of the handle's scalar type. */
int sprs_csr_read(const sprs_csr *A, int32_t *row_ptr_host, int32_t *col_idx_host, void *val_host);

/* ---------------------------------------------------------------- the product of two operators
 * sprs_csr_matmul builds C = A B as an ordinary, independent handle of shape A.nrows x B.ncols: it owns its arrays, outlives A
 * and B, and every sprs_mul_vec_* / sprs_mul_mat_* / solver entry point, sprs_csr_adjoint, sprs_csr_matmul itself and
 * sprs_amg_create take it like any other handle.  The construction runs on the device only (csrc/spgemm.hip).
 * The contract is the serial row-by-row loop, and the result has its bits in f64, c64, f32 and c32:
 *   - row i of C comes from one accumulator per column, each starting at zero (+0);
 *   - the stored entries a_ik of row i of A are walked in stored order, and for each the stored entries b_kj of row k of B in
 *     stored order; each pair does acc_j = acc_j + a_ik * b_kj, two separately rounded operations (complex numbers by
 *     components with the naive product formula).  No accumulator is initialised with its first product: 0 + (-0.0) is +0.0;
 *   - the stored pattern is the structural one: an entry whose terms cancel to exactly zero stays stored;
 *   - the columns of every row of C are strictly ascending;
 *   - two calls on the same operands give the same bytes.
 * Operands: single-GPU handles of one context and one scalar type (otherwise SPRS_INVALID_ARGUMENT, text in sprs_last_error);
 * A.ncols != B.nrows: SPRS_DIM_MISMATCH.  The rows of A may be stored in any order and may hold duplicate columns (their
 * contributions are folded in stored order).  The rows of B must be strictly ascending: checked on the device,
 * SPRS_INVALID_ARGUMENT with the smallest offending row in the text.  A == B is allowed.  A product of more than 2^31 - 1
 * stored entries: SPRS_INVALID_ARGUMENT.  Empty rows of A give empty rows of C, empty rows of B contribute nothing.
 * Each row of A is dealt to one of three kernels by u_i = the sum of nnz(B row k) over its stored entries a_ik, an upper bound
 * of its products: u_i <= 64 several rows per wavefront, small tables in LDS; u_i <= 1024 (2048 in f32) one workgroup per row
 * and a hash table in LDS sized for twice that; larger rows one workgroup per row with a dense accumulator of B.ncols entries
 * in device scratch.  At most 1024 such workgroups run, and no more than fit 256 MiB: the scratch of a call is bounded by
 * max(256 MiB, B.ncols * (sizeof(scalar) + 4)) bytes whatever the matrices.  Further temporary device memory: 29 bytes per row
 * of A + the result.
 * info (may be NULL) receives 5 values: [0..2] the rows of A taken by the short / table / dense kernel, [3] the largest u_i of
 * the short kernel, [4] the largest u_i of the table kernel for this scalar type. */
int sprs_csr_matmul(const sprs_csr *A, const sprs_csr *B, sprs_csr **out, int64_t *info);

/* ---------------------------------------------------------------- orderings: graph colouring and the symmetric permutation
 * For square, single-GPU handles (SPRS_NOT_SQUARE; a distributed A is SPRS_INVALID_ARGUMENT, text in sprs_last_error).  The
 * reference has neither.  sprs_ilu0_create_ordered (below) is built from both.
 *
 * sprs_csr_color colours the graph of A's pattern: the vertices are the rows, and i ~ j iff i != j and A stores (i, j) or
 * (j, i).  Explicit zeros count, the pattern may be non-symmetric, values are never read (the colours do not depend on the
 * scalar type).  The priority of vertex i is w(i), 64 unsigned bits computed from the seed and i alone:
 *     z = seed + (i + 1) * 0x9E3779B97F4A7C15            (all arithmetic modulo 2^64)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     w(i) = z ^ (z >> 31)
 * and the colouring is greedy first-fit in decreasing order of the pair (w(i), i):
 *     colour[i] = -1 for all i
 *     for i in decreasing (w(i), i):  colour[i] = the smallest c >= 0 that no neighbour j of i with colour[j] >= 0 has
 * The device computes exactly this colouring by Jones-Plassmann rounds, one kernel launch each:
 *     repeat until no vertex is uncoloured:
 *         S = the uncoloured i whose (w(i), i) exceeds that of every uncoloured neighbour     (an independent set)
 *         for i in S, in any order:  colour[i] = the smallest c >= 0 no coloured neighbour of i has
 * (no neighbour of a vertex of S is written in its round, so the round runs in place and its result does not depend on the
 * launch geometry; the largest uncoloured vertex is always in S, so at most n rounds run).  colors_host receives n values in
 * 0 .. *ncolors_out - 1; *ncolors_out is the largest colour + 1 and *rounds_out the number of rounds (both may be NULL).
 * n = 0: zero colours, zero rounds.  Sorting the rows by colour (stably) gives a permutation under which every colour is a
 * diagonal block of P A P^T, and the dependency levels of its triangles are at most the colours.
 * Temporary device memory: 4 bytes per entry + 16 per row.
 *
 * sprs_csr_permute builds B = P A P^T as an ordinary, independent handle: it owns its arrays, outlives A, gets whatever
 * stream format its creation finds, and every entry point takes it.  perm_host[p] is the row of A that becomes row p of B
 * (new -> old):
 *     B[p, q] = A[perm[p], perm[q]]
 *     row p of B:  for each stored (perm[p], j, v) of A:  store (inv[j], v), inv the inverse of perm;  then sort the row by column
 *                  with a STABLE sort
 * The columns of every row of B ascend.  The rows of A may be stored in any order and may hold duplicate columns: duplicates
 * stay duplicates, in their stored order (as in sprs_csr_adjoint), so B's columns ascend strictly exactly where A's rows hold
 * none.  The values are bit copies.  perm must have A.nrows entries, each in [0, nrows), none twice: otherwise SPRS_INVALID_ARGUMENT with
 * the offending entry in sprs_last_error.  The construction runs on the device (inverse, row-length gather and scan, one
 * wavefront per row: csrc/order.hip); only perm crosses PCIe. */
int sprs_csr_color(const sprs_csr *A, uint64_t seed, int32_t *colors_host, int64_t *ncolors_out, int64_t *rounds_out);
int sprs_csr_permute(const sprs_csr *A, const int32_t *perm_host, size_t perm_len, sprs_csr **out);

/* ---------------------------------------------------------------- LSMR
 * Fong & Saunders' LSMR: x minimises |rhs - A x|_2, or with damp > 0 |[A; damp I] x - [rhs; 0]|_2, for A of ANY shape (m rows,
 * n columns; rank-deficient and inconsistent systems included; on an under-determined system started from x = 0 the minimum-norm
 * solution).  It runs on the Golub-Kahan bidiagonalisation and is MINRES on the normal equations in exact arithmetic.  Two SpMVs
 * per iteration, one by A and one by its adjoint handle AH (shape n x m, the same scalar type and context; sprs_csr_adjoint(A, 1)):
 * create borrows the caller's AH (SPRS_DIM_MISMATCH / SPRS_INVALID_ARGUMENT where shape / type do not fit) or, given NULL, builds
 * and owns one.  The handle holds 2m + 4n of workspace.  A distributed A: SPRS_INVALID_ARGUMENT (text in sprs_last_error).
 * x is in/out (n entries): a non-zero x is an initial guess, the recurrence runs on the correction; rhs has m entries.  Wrong
 * lengths: SPRS_DIM_MISMATCH; damp < 0 (or NaN): SPRS_INVALID_ARGUMENT.
 * EVERY recurrence scalar is of type T::Real, also for complex T (norms and plane rotations); only the vectors are complex.
 * In the vector updates below a*s is the element times the real s, one rounding per real operation, and + is one addition:
 * axpby(a, p, b, q) is q = sadd(smul(p, a), smul(q, b)).  u is kept UN-NORMALISED: in memory u = beta u_k, readers apply 1/beta.
 * symortho(a, b) -> (c, s, r) with c a + s b = r, -s a + c b = 0:   b == 0: (sign a, 0, |a|);   a == 0: (0, sign b, |b|);
 *     |b| > |a|: tau = a / b, s = sign(b) / sqrt(1 + tau tau), c = s tau, r = b / s;   else: tau = b / a, c = sign(a) / sqrt(1 + tau tau),
 *     s = c tau, r = a / c        (sign 0 = 0)
 *     normb = norm2(rhs);  if normb <= eps: x = 0, return SPRS_OK with *its_out = 0, *res_out = normb, *ares_out = 0
 *     u = rhs*1 + (A x)*(-1);  beta = norm2(u);  not finite: SPRS_BREAKDOWN (its 0);  beta == 0: SPRS_OK, its 0, res 0, ares 0
 *     v = AH u;  v = v*(1/beta);  alpha = norm2(v);  not finite: SPRS_BREAKDOWN;  alpha == 0: SPRS_OK, its 0, res = beta / normb, ares 0
 *     v = v*(1/alpha);  h = v;  hbar = 0
 *     alphabar = alpha; zetabar = alpha beta; rho = rhobar = cbar = 1; sbar = 0; betadd = beta; betad = 0; rhodold = 1;
 *     tautildeold = thetatilde = zeta = d = 0; normA2 = alpha alpha
 *     for its = 0 .. max_iter - 1:
 *         V1  w = A v;  u = w*1 + u*f with f = -(alpha (1/beta))             [axpby(1, w, f, u)]
 *         V2  beta = norm2(u);  not finite: SPRS_BREAKDOWN, *its_out = its
 *         V3  if beta > 0:  w' = AH u;  v = w'*(1/beta) + v*(-beta)  [axpby(1/beta, w', -beta, v)];  alpha = norm2(v);  not finite:
 *             SPRS_BREAKDOWN;   if beta == 0:  alpha = 0 and v is left alone
 *         S1  (chat, shat, alphahat) = symortho(alphabar, damp);  rhoold = rho;  (c, s, rho) = symortho(alphahat, beta)
 *         S2  thetanew = s alpha;  alphabar = c alpha;  rhobarold = rhobar;  zetaold = zeta;  thetabar = sbar rho
 *         S3  (cbar, sbar, rhobar) = symortho(cbar rho, thetanew)  [the old cbar];  zeta = cbar zetabar;  zetabar = -sbar zetabar
 *         S4  g1 = -(thetabar rho / (rhoold rhobarold));  g2 = zeta / (rho rhobar);  g3 = -(thetanew / rho)
 *         S5  betaacute = chat betadd;  betacheck = -shat betadd;  betahat = c betaacute;  betadd = -s betaacute
 *         S6  thetatildeold = thetatilde;  (ct, st, rt) = symortho(rhodold, thetabar);  thetatilde = st rhobar;  rhodold = ct rhobar;
 *             betad = -st betad + ct betahat;  tautildeold = (zetaold - thetatildeold tautildeold) / rt;
 *             taud = (zeta - thetatilde tautildeold) / rhodold;  d = d + betacheck betacheck
 *         S7  normr = sqrt(d + (betad - taud)^2 + betadd betadd);  normA2 += beta beta;  normA = sqrt(normA2);  normA2 += alpha alpha;
 *             normar = |zetabar|
 *         S8  unless g1, g2, g3, normr, normA, normar are all finite: SPRS_BREAKDOWN, *its_out = its  (x as after its iterations)
 *         V4  hbar = h*1 + hbar*g1  [axpby(1, h, g1, hbar)];  x = x + hbar*g2  [axpy(g2, hbar, x)];  if alpha > 0: v = v*(1/alpha);
 *             h = v*1 + h*g3  [axpby(1, v, g3, h)]
 *         T   normx = norm2(x);  SPRS_OK with *its_out = its + 1 if beta == 0 or alpha == 0 (the exact solution has been reached),
 *             or normr <= tol normb + tol normA normx   (test 1),   or normar <= tol normA normr   (test 2)
 *     SPRS_INSUFFICIENT_ITER, *its_out = max_iter
 * On SPRS_OK from the loop *res_out = normr / normb and *ares_out = normar / (normA normr) (0 where that product is 0): the
 * recurrence's estimates of |r| / |rhs| and |A^H r| / (|A|_F |r|), r = rhs - A x; no extra pass is made for them.  No condition-
 * number limit is applied.  The fused mode (default; five launches per iteration, csrc/lsmr_fuse.hpp) evaluates T in the launch
 * after V4 — same values, same event, whatever the context's `poll`; the literal mode runs the steps one kernel per operation.
 * Solver kind SPRS_SOLVER_LSMR for sprs_solver_set_mode / set_trace / the profile getters.  Trace row, one per iteration that
 * reached T: [its, normr, normar, 0, alpha, 0, beta, 0]. */
int sprs_lsmr_destroy(sprs_lsmr *S);           /* NULL is a no-op */
int sprs_lsmr_create_d(const sprs_csr *A, const sprs_csr *AH_or_null, sprs_lsmr **out);
int sprs_lsmr_solve_d(sprs_lsmr *S, const double *rhs, size_t rhs_len, double *x, size_t x_len, double damp, size_t max_iter, double tol, size_t *its_out, double *res_out, double *ares_out);
int sprs_lsmr_solve_dev_d(sprs_lsmr *S, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, double damp, size_t max_iter, double tol, size_t *its_out, double *res_out, double *ares_out);
int sprs_lsmr_create_z(const sprs_csr *A, const sprs_csr *AH_or_null, sprs_lsmr **out);
int sprs_lsmr_solve_z(sprs_lsmr *S, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, double damp, size_t max_iter, double tol, size_t *its_out, double *res_out, double *ares_out);
int sprs_lsmr_solve_dev_z(sprs_lsmr *S, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, double damp, size_t max_iter, double tol, size_t *its_out, double *res_out, double *ares_out);

/* ---------------------------------------------------------------- several right-hand sides at once: SpMM and batched CG
 * A block of k vectors (1 <= k <= 8) is an n x k ROW-MAJOR array: the k values of row i are contiguous (numpy's C order
 * of an (n, k) array).  Single GPU: a distributed operator is refused with SPRS_INVALID_ARGUMENT (text in sprs_last_error).
 *
 * sprs_mul_mat_*: Y = A X on the plain CSR arrays, one pass over the matrix for all k columns.  Column c of Y is bit-identical
 * to sprs_mul_vec_dev_* on column c of X.  The host entries check x_len == ncols * k and y_len == nrows * k
 * (SPRS_DIM_MISMATCH); k outside 1..8, a null handle and a handle of another scalar type are SPRS_INVALID_ARGUMENT.
 *
 * sprs_cgmany_* on a sprs_cg_many handle (the functions carry no `sprs_cg_` prefix: that one names the single-vector solver's
 * entry points): conjugate gradients ("conjugate gradients" above) on k right-hand sides in three launches per iteration
 * whatever k is.  Column j runs exactly that recurrence on its own rho, alpha, beta, |r| and tol * |rhs_j|, with its own
 * zero-right-hand-side and converged-at-the-start rules, and stops on its own event; from then on its x is not written.
 * create's k is the most columns a solve may carry; a solve takes any 1 <= k <= that (else SPRS_INVALID_ARGUMENT) and
 * rhs_len == x_len == size * k (SPRS_INCOMPATIBLE_RHS_SIZE / SPRS_INCOMPATIBLE_X_SIZE).  its_out[j], res_out[j] are what
 * sprs_cg_solve_* reports for column j's event and status_out[j] is that event's status code (each array: k entries, or
 * NULL).  Returns SPRS_OK if every column did, else the status of the lowest-numbered column that did not.  Argument and
 * size errors return at once and write nothing.  The handle holds 5 blocks of size x k' (k' = k rounded up to a power of
 * two).  No literal mode, trace or profile. */
int sprs_cgmany_destroy(sprs_cg_many *S);     /* NULL is a no-op */
int sprs_mul_mat_d(const sprs_csr *A, const double *x_host, size_t x_len, double *y_host, size_t y_len, size_t k);
int sprs_mul_mat_dev_d(const sprs_csr *A, const double *x_dev, double *y_dev, size_t k);
int sprs_cgmany_create_d(const sprs_csr *A, size_t size, size_t k, sprs_cg_many **out);
int sprs_cgmany_solve_d(sprs_cg_many *S, const sprs_diag *P_or_null, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t k, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_cgmany_solve_dev_d(sprs_cg_many *S, const sprs_diag *P_or_null, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t k, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_mul_mat_z(const sprs_csr *A, const sprs_c64 *x_host, size_t x_len, sprs_c64 *y_host, size_t y_len, size_t k);
int sprs_mul_mat_dev_z(const sprs_csr *A, const sprs_c64 *x_dev, sprs_c64 *y_dev, size_t k);
int sprs_cgmany_create_z(const sprs_csr *A, size_t size, size_t k, sprs_cg_many **out);
int sprs_cgmany_solve_z(sprs_cg_many *S, const sprs_diag *P_or_null, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t k, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_cgmany_solve_dev_z(sprs_cg_many *S, const sprs_diag *P_or_null, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t k, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);

/* ---------------------------------------------------------------- shifted systems: multi-shift conjugate gradients
 * sprs_cgshift_* on a sprs_cg_shift handle: the solutions of (A + sigma_j I) x_j = rhs, j = 0 .. m - 1, for a Hermitian positive-
 * definite A and m real shifts (finite, >= 0, 1 <= m <= mmax <= 8), in ONE Krylov run on A: one SpMV and three launches per
 * iteration whatever m is.  A Krylov space does not change under a shift; started from x = 0, every shifted residual stays
 * collinear with the residual of CG on A (the "seed"), r_j = zeta_j r, and column j follows from a scalar recurrence
 * (Jegerlehner's CG-M, in the convention of "conjugate gradients" above: alpha is the step, beta = rho_new / rho).  In exact
 * arithmetic x_j is CG's own iterate on A + sigma_j I, so each column needs the iterations it would need alone.
 * The zero start is part of the method: x is OUTPUT ONLY, m contiguous vectors of n entries (numpy's C order of an (m, n) array;
 * each x_j is an ordinary vector), its contents on entry are ignored.  There is no preconditioner and no precond_solve: a general
 * M destroys the shift invariance.  Out of scope: negative shifts, complex shifts, a non-zero start, distributed operators
 * (refused at creation with SPRS_INVALID_ARGUMENT, text in sprs_last_error).
 * Vectors are of type T; rho, alpha, beta are T; the norms are T::Real; zeta_j, a, b and the column coefficients are DOUBLES
 * whatever T is.  Every line is one library operation per element, each arithmetic operation rounded once:
 *     rhs_norm = norm2(rhs);  if rhs_norm <= eps: every x_j = 0, return SPRS_OK with its_out[j] = 0, res_out[j] = rhs_norm
 *     tol2 = tol * rhs_norm;  r = rhs;  if |r| <= tol2 (tol >= 1): every x_j = 0, SPRS_OK, its_out[j] = 0, res_out[j] = 1
 *     p = r;  rho = conj_dot(r, r);  x_j = 0;  p_j = r;  zeta_j^(-1) = zeta_j^(0) = 1;  a_old = 1;  b_old = 0;  all columns run
 *     for n = 0 .. max_iter - 1:
 *         q = A p;  pq = conj_dot(p, q);  unless re(pq) > 0: every running column ends with SPRS_BREAKDOWN, its_out[j] = n
 *         alpha = rho / pq;  a = re(alpha)
 *         for every running column, with z = zeta_j^(n), zp = zeta_j^(n-1), s = sigma_j:
 *             den = a*b_old*(zp - z) + zp*a_old*(1 + s*a);  zn = z*zp*a_old / den
 *             if den == 0 or zn is not finite: that column alone ends with SPRS_BREAKDOWN, its_out[j] = n (x_j as after n iterations)
 *             zeta_j^(n+1) = zn
 *         r += q*(-alpha);  r_norm = sqrt(sum |r_i|^2);  rho_new = sum |r_i|^2;  beta = rho_new / rho;  b = re(beta)
 *         for every column that still runs:  t = zn / z;  alpha_j = a*t;  beta_j = b*(t*t)
 *             x_j += p_j*alpha_j                                   [alpha_j rounded to T::Real; a real times T, as the Jacobi product]
 *             if |zn| * r_norm <= tol2:  column j ends with SPRS_OK, its_out[j] = n + 1, res_out[j] = |zn| * r_norm / rhs_norm;
 *                 from then on it is frozen: x_j, p_j and zeta_j are neither read nor written
 *             else  p_j = r*zn + p_j*beta_j                        [zn, beta_j rounded to T::Real]
 *         p = r*1 + p*beta;  rho = rho_new;  a_old = a;  b_old = b
 *         if no column runs: the solve is over
 *     columns still running: SPRS_INSUFFICIENT_ITER, its_out[j] = max_iter
 * res_out[j] is the recurrence's |r_j| / |rhs| (0 with an error status).  its_out, res_out, status_out: m entries each, or NULL.
 * Returns SPRS_OK if every column did, else the status of the lowest-numbered column that did not.
 * create's mmax is the most shifts a solve may carry (mmax = 0 or > 8: SPRS_INVALID_ARGUMENT); the handle holds 3 + 2 mmax
 * vectors.  Argument errors return at once and write nothing: m = 0 or m > mmax, a null shifts / rhs / x, a shift that is
 * negative or not finite (text in sprs_last_error): SPRS_INVALID_ARGUMENT; rhs_len != size: SPRS_INCOMPATIBLE_RHS_SIZE;
 * x_len != size * m: SPRS_INCOMPATIBLE_X_SIZE.  shifts is a host array in both entry points.  The iterations are enqueued
 * blind and the device-side state is read every `poll` of them: results do not depend on `poll`, and column j's bits do not
 * depend on m or on the other shifts.  No literal mode, trace or profile. */
int sprs_cgshift_destroy(sprs_cg_shift *S);   /* NULL is a no-op */
int sprs_cgshift_create_d(const sprs_csr *A, size_t size, size_t mmax, sprs_cg_shift **out);
int sprs_cgshift_solve_d(sprs_cg_shift *S, const double *shifts, size_t m, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_cgshift_solve_dev_d(sprs_cg_shift *S, const double *shifts, size_t m, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_cgshift_create_z(const sprs_csr *A, size_t size, size_t mmax, sprs_cg_shift **out);
int sprs_cgshift_solve_z(sprs_cg_shift *S, const double *shifts, size_t m, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_cgshift_solve_dev_z(sprs_cg_shift *S, const double *shifts, size_t m, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_cgshift_create_s(const sprs_csr *A, size_t size, size_t mmax, sprs_cg_shift **out);
int sprs_cgshift_solve_s(sprs_cg_shift *S, const float *shifts, size_t m, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_cgshift_solve_dev_s(sprs_cg_shift *S, const float *shifts, size_t m, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_cgshift_create_c(const sprs_csr *A, size_t size, size_t mmax, sprs_cg_shift **out);
int sprs_cgshift_solve_c(sprs_cg_shift *S, const float *shifts, size_t m, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_cgshift_solve_dev_c(sprs_cg_shift *S, const float *shifts, size_t m, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);

/* ---------------------------------------------------------------- restarted GMRES
 * GMRES(m) for any non-singular A: right-preconditioned (Jacobi P, or none), the Arnoldi vector orthogonalised by classical
 * Gram-Schmidt applied twice (CGS2), Givens rotations on the Hessenberg column.  The reference has no such solver; the
 * conventions are its BiCGStab's: relative residual against |rhs|, a zero right-hand side answers x = 0, x is in/out and is
 * left modified on error, the same status codes.  The residual estimate never increases and the method cannot break down
 * before it has the solution.  The handle holds (m + 4) n of workspace.  `restart` = m, 0 means 30, at most
 * SPRS_GMRES_MAX_RESTART; a larger one, or a null A, is SPRS_INVALID_ARGUMENT.
 * Vectors v_0 .. v_m, w, z, u are of type T; h_i, c_i (pass 2), g_i, s_i, y_i and the entries of R are T; hn, beta, cs_i, d, aa
 * are T::Real.  conj_dot(a, b) = sum conj(a_i) b_i.  Every line below is one library operation per element (axpy: y += x*a;
 * axpby: y = x*a + y*b), each arithmetic operation rounded once:
 *     rhs_norm = norm2(rhs);  if rhs_norm <= eps: x = 0, return SPRS_OK with *its_out = 0, *res_out = rhs_norm
 *     tol2 = tol * rhs_norm;  its = 0
 *     cycle:
 *         v_0 = A x;  v_0 = rhs*1 + v_0*(-1);  beta = norm2(v_0)
 *         if beta <= tol2: SPRS_OK, *its_out = its, *res_out = beta / rhs_norm
 *         v_0 = v_0 * (1 / beta)  (real scale);  g_0 = beta
 *         for j = 0 .. m - 1:
 *             z = P v_j (z is v_j itself without P);  w = A z
 *             pass 1:  h_i = conj_dot(v_i, w) for i = 0 .. j, all on the same w;  then for i = 0 .. j in order: w += v_i*(-h_i)
 *             pass 2:  c_i = conj_dot(v_i, w) for i = 0 .. j, all on the same w;  then for i = 0 .. j in order: w += v_i*(-c_i);
 *                      h_i = h_i + c_i
 *             hn = norm2(w);  unless hn >= 0 (NaN): SPRS_BREAKDOWN, *its_out = its
 *             for i = 0 .. j - 1 in order (the earlier rotations on the new column):
 *                 t = h_i*cs_i + s_i*h_{i+1};  h_{i+1} = (-conj(s_i))*h_i + h_{i+1}*cs_i;  h_i = t
 *             rotation j from a = h_j and the real hn:  aa = |a|;  d = sqrt(aa*aa + hn*hn)
 *                 aa == 0:  cs_j = 0, s_j = 1          else:  cs_j = aa / d,  s_j = a * ((hn / d) / aa)   (real c, complex s)
 *                 R_jj = a*cs_j + s_j*hn  (it keeps the phase of a);  R_ij = h_i for i < j
 *                 g_{j+1} = (-conj(s_j))*g_j;  g_j = g_j*cs_j
 *             its += 1
 *             if |g_{j+1}| <= tol2, or hn == 0 (the Krylov space is exhausted), or its == max_iter: k = j + 1, leave the loop
 *             v_{j+1} = w * (1 / hn)  (real scale)
 *         (k = m where the loop ran out)
 *         back substitution, for i = k - 1 .. 0:  t = g_i;  for l = i + 1 .. k - 1 in order: t = t - R_il*y_l;  y_i = t / R_ii
 *         u = 0;  for i = 0 .. k - 1 in order: u += v_i*y_i;  u = P u;  x += u*1
 *         if |g_k| <= tol2: SPRS_OK, *its_out = its, *res_out = |g_k| / rhs_norm
 *         if its == max_iter: SPRS_INSUFFICIENT_ITER, *its_out = max_iter  (x holds the partial cycle's update)
 *         else the next cycle
 * max_iter == 0: SPRS_INSUFFICIENT_ITER after the first cycle's beta test, x untouched.
 * `its` counts Arnoldi steps = the SpMVs inside the cycles (each cycle costs one more for its residual); |.| of a complex
 * number is hypot.  Fused and literal modes differ only in the summation order of the dot products and norms.
 * Trace row (sprs_solver_set_trace), one per Arnoldi step: [its (after the step), |g_{j+1}|, hn, re(R_jj), im(R_jj), cs_j,
 * re(s_j), im(s_j)]. */
#define SPRS_GMRES_MAX_RESTART 64
int sprs_gmres_create_d(const sprs_csr *A, size_t size, size_t restart, sprs_gmres **out);
int sprs_gmres_create_z(const sprs_csr *A, size_t size, size_t restart, sprs_gmres **out);
int sprs_gmres_destroy(sprs_gmres *S);         /* NULL is a no-op */
int sprs_gmres_solve_d(sprs_gmres *S, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_gmres_solve_z(sprs_gmres *S, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_gmres_precond_solve_d(sprs_gmres *S, const sprs_diag *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_gmres_precond_solve_z(sprs_gmres *S, const sprs_diag *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
/* the same on device vectors (16-byte aligned ones are used in place) */
int sprs_gmres_solve_dev_d(sprs_gmres *S, const sprs_diag *P_or_null, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_gmres_solve_dev_z(sprs_gmres *S, const sprs_diag *P_or_null, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);

/* ---------------------------------------------------------------- IDR(s)
 * IDR(s) for any square non-singular A (Sonneveld & van Gijzen 2008; the bi-orthogonal variant of van Gijzen & Sonneveld, ACM
 * TOMS 38(1), 2011): a short-recurrence solver on 3 s + 4 vectors with a fixed cost per product with A and no restart; IDR(1)
 * is mathematically BiCGStab.  Right-preconditioned by nothing, a diagonal, or an applied handle (sprs_ilu0_idrs_*,
 * sprs_amg_idrs_*, sprs_fsai_idrs_*).  The conventions are BiCGStab's: relative residual against |rhs|, a zero right-hand side
 * answers x = 0, x is in/out (a non-zero start is honoured) and is left modified on error, the same status codes.  `s` = 0
 * means 4; s > SPRS_IDRS_MAX_S or s > size is SPRS_INVALID_ARGUMENT with a text (sprs_last_error), and so is a distributed
 * operator.  One (fused) mode: sprs_solver_set_mode(.., SPRS_SOLVER_IDRS, 1) is SPRS_INVALID_ARGUMENT.
 *
 * Shadow space: column c of P holds the U[-1, 1) values of the generators' counter-based stream 200 + 2 c (sprs_lobpcg_*'s
 * default start block uses streams 100 + ..; the imaginary parts of a complex T: stream 201 + 2 c), rounded to T; the columns
 * are orthonormalised once at creation, in D (CGS2 against the earlier columns: each pass takes its dot products on the same
 * vector, then subtracts in ascending order; then a real scale by 1 / norm2), and rounded to T at the end.
 *
 * Vectors r, v, vh, t, g_i, u_i, p_i are of type T.  D = double for a real T and complex double for a complex T: M (s x s, the
 * identity at the start), f, c, alpha, beta, q and omega (1 at the start) are kept and computed in D for every T, in the order
 * written, and rounded to T only where they multiply a vector.  G = [g_i] and U = [u_i] start at zero.  conj_dot(a, b) =
 * sum conj(a_i) b_i and norm2 inside the cycles are computed in D too: the operands are widened, so for a single-precision T
 * every product is exact and only the sum rounds, and the scalars do not depend on the summation order beyond 1e-16 (the
 * first rn is the library's norm2 in T).  P v is the preconditioner (v itself without one).  kappa = 0.7.
 *     rhs_norm = norm2(rhs);  if rhs_norm <= eps: x = 0, return SPRS_OK with *its_out = 0, *res_out = rhs_norm
 *     tol2 = tol * rhs_norm;  r = A x;  r = rhs*1 + r*(-1);  rn = norm2(r);  its = 0
 *     if rn <= tol2: SPRS_OK, *its_out = 0, *res_out = rn / rhs_norm
 *     cycle:
 *         f_i = conj_dot(p_i, r) for i = 0 .. s - 1, all on the same r
 *         for k = 0 .. s - 1:
 *             for i = k .. s - 1 in order:  t = f_i;  for j = k .. i - 1 in order: t = t - M_ij*c_j;  c_i = t / M_ii
 *             v = r;  for i = k .. s - 1 in order: v += g_i*(-c_i);  vh = P v
 *             w = 0;  for i = k .. s - 1 in order: w += u_i*c_i;  u_k = vh*omega + w
 *             g_k = A u_k;  its += 1
 *             q_i = conj_dot(p_i, g_k) for i = 0 .. s - 1, all on the same g_k
 *             for i = 0 .. k - 1 in order:  t = q_i;  for j = 0 .. i - 1 in order: t = t - M_ij*alpha_j;  alpha_i = t / M_ii
 *             for i = 0 .. k - 1 in order: g_k += g_i*(-alpha_i);  for i = 0 .. k - 1 in order: u_k += u_i*(-alpha_i)
 *             for i = k .. s - 1:  m = q_i;  for j = 0 .. k - 1 in order: m = m - M_ij*alpha_j;  M_ik = m
 *             unless M_kk is finite and not 0: SPRS_BREAKDOWN, *its_out = its (x and r are those before this step)
 *             beta = f_k / M_kk;  r += g_k*(-beta);  x += u_k*beta;  for i = k + 1 .. s - 1: f_i = f_i - beta*M_ik
 *             rn = norm2(r);  if rn <= tol2: SPRS_OK, *its_out = its, *res_out = rn / rhs_norm
 *             if its == max_iter: SPRS_INSUFFICIENT_ITER, *its_out = max_iter
 *         vh = P r;  t = A vh;  its += 1;  tt = re(conj_dot(t, t));  tr = conj_dot(t, r)
 *         rho = |tr| / (sqrt(tt) * rn);  omega = tr*(1 / tt);  if rho < kappa: omega = omega * (kappa / rho)
 *         unless tt > 0 and tt and omega are finite and omega is not 0: SPRS_BREAKDOWN, *its_out = its
 *         x += vh*omega;  r += t*(-omega);  rn = norm2(r);  the two tests on rn and its as above
 * max_iter == 0: SPRS_INSUFFICIENT_ITER after the initial residual's test, x untouched.  `its` counts the products with A after
 * the initial residual; the reported residual is the recursive one.  The k sequential projections of the textbook step are one
 * multi-dot and a k x k forward solve here, because P^H [g_0 .. g_{k-1}] is lower triangular.
 * Solver kind SPRS_SOLVER_IDRS for sprs_solver_set_trace / sprs_solver_trace_rows.  Trace row, one per product with A: [its
 * (after the product), rn before the step, re, im of the step's coefficient (beta, or omega), re, im of its pivot (M_kk, or tt),
 * k (s for the omega step), 0]. */
#define SPRS_IDRS_MAX_S 8
int sprs_idrs_destroy(sprs_idrs *S);           /* NULL is a no-op */
int sprs_idrs_create_d(const sprs_csr *A, size_t size, size_t s, sprs_idrs **out);
int sprs_idrs_create_z(const sprs_csr *A, size_t size, size_t s, sprs_idrs **out);
int sprs_idrs_create_s(const sprs_csr *A, size_t size, size_t s, sprs_idrs **out);
int sprs_idrs_create_c(const sprs_csr *A, size_t size, size_t s, sprs_idrs **out);
int sprs_idrs_solve_d(sprs_idrs *S, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_idrs_solve_z(sprs_idrs *S, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_idrs_solve_s(sprs_idrs *S, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_idrs_solve_c(sprs_idrs *S, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_idrs_precond_solve_d(sprs_idrs *S, const sprs_diag *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_idrs_precond_solve_z(sprs_idrs *S, const sprs_diag *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_idrs_precond_solve_s(sprs_idrs *S, const sprs_diag *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_idrs_precond_solve_c(sprs_idrs *S, const sprs_diag *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
/* the same on device vectors (16-byte aligned ones are used in place) */
int sprs_idrs_solve_dev_d(sprs_idrs *S, const sprs_diag *P_or_null, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_idrs_solve_dev_z(sprs_idrs *S, const sprs_diag *P_or_null, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_idrs_solve_dev_s(sprs_idrs *S, const sprs_diag *P_or_null, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_idrs_solve_dev_c(sprs_idrs *S, const sprs_diag *P_or_null, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);

/* ---------------------------------------------------------------- mixed-precision iterative refinement
 * An answer of H precision (H = f64 for _d, Complex<f64> for _z) at the byte cost of L iterations (L = f32 / Complex<f32>):
 * the residual and the solution stay in H, every correction comes from an inner Krylov solve in L on a copy of A whose values
 * were rounded to L once, at creation.  The reference has no such solver; conventions are the other solvers'.  Single GPU: a
 * distributed A is refused with SPRS_INVALID_ARGUMENT (text in sprs_last_error).  Every line is one library operation per
 * element, each arithmetic operation rounded once; fl_L rounds an H value to L (to nearest, per component), fl_H is exact:
 *     the sums of |b|^2 and of the first |r|^2 are formed in one pass;  if norm2(b) <= eps(H::Real): x = 0, SPRS_OK,
 *                                                                   *outer_out = 0, *res_out = norm2(b)
 *     for k = 0, 1, ...:
 *         r = b*1 + (A x)*(-1)                in H, the SpMV of the handle A (any route)
 *         res = norm2(r) / norm2(b);  if res <= tol: SPRS_OK, *outer_out = k, *res_out = res
 *         unless norm2(r) is finite: SPRS_BREAKDOWN, *outer_out = k
 *         if k == max_outer: SPRS_INSUFFICIENT_ITER, *outer_out = max_outer, *res_out = res  (x is the last iterate)
 *         s = norm2(r);  rl_i = fl_L(r_i * (1 / s))       1 / s rounded once in H::Real; a real scale (mul_real)
 *         e = 0;  inner solve of A_L e = rl in L: sprs_cg_* or sprs_gmres_* as stated above with max_iter = inner_max_iter,
 *                 tol = fl(inner_tol), P_L (P's stored 1 / diag rounded to L) or no preconditioner
 *             SPRS_OK or SPRS_INSUFFICIENT_ITER: the correction is used
 *             any other status is returned as this solve's, *outer_out = k, x unchanged by this step
 *         x_i = x_i + fl_H(e_i) * s                       the product rounded (a real scale), then the sum
 * Every inner right-hand side has norm 1, so no residual underflows in L and inner_tol means the same at every step.
 * *inner_its_out is the sum of the inner solves' *its_out; x is in/out and is left modified on error.
 * create: `inner` picks the inner solver, `restart` is GMRES' m (0 = 30; ignored by CG).  SPRS_INVALID_ARGUMENT (with a text)
 * if a finite value of A leaves L's range; P's size / scalar type are checked as for the other solvers.  The handle borrows A
 * (A's row_ptr / col_idx are shared with the L operator) and copies P; it owns the L operator (sprs_refine_low_csr returns it,
 * borrowed: any sprs_mul_vec_*_s / _c call applies), the inner solver, one H vector, two L vectors, and two more H vectors once a
 * solve was given host slices.  An outer step costs one SpMV in H and three launches besides its inner iterations. */
typedef struct sprs_refine sprs_refine;
enum { SPRS_INNER_CG = 0, SPRS_INNER_GMRES = 1 };
int sprs_refine_create_d(const sprs_csr *A, size_t size, const sprs_diag *P_or_null, int inner, size_t restart, sprs_refine **out);
int sprs_refine_create_z(const sprs_csr *A, size_t size, const sprs_diag *P_or_null, int inner, size_t restart, sprs_refine **out);
int sprs_refine_destroy(sprs_refine *R);       /* NULL is a no-op */
const sprs_csr *sprs_refine_low_csr(const sprs_refine *R);
int sprs_refine_solve_d(sprs_refine *R, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_outer, double tol, size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out);
int sprs_refine_solve_z(sprs_refine *R, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_outer, double tol, size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out);
/* the same on device vectors (16-byte aligned ones are used in place) */
int sprs_refine_solve_dev_d(sprs_refine *R, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_outer, double tol, size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out);
int sprs_refine_solve_dev_z(sprs_refine *R, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_outer, double tol, size_t inner_max_iter, double inner_tol, size_t *outer_out, size_t *inner_its_out, double *res_out);
/* The two mixed-precision vector operations of the recurrence on device vectors, asynchronous on the context's stream like the
 * vecalg entry points; the scalars are real (H::Real):  out_i = fl_L(in_i * scale)  and  x_i = x_i + fl_H(in_i) * alpha. */
int sprs_demote_scaled_dev_d(sprs_ctx *ctx, size_t n, const double *in_dev, double scale, float *out_dev);
int sprs_demote_scaled_dev_z(sprs_ctx *ctx, size_t n, const sprs_c64 *in_dev, double scale, sprs_c32 *out_dev);
int sprs_axpy_promoted_dev_d(sprs_ctx *ctx, size_t n, double alpha, const float *in_dev, double *x_dev);
int sprs_axpy_promoted_dev_z(sprs_ctx *ctx, size_t n, double alpha, const sprs_c32 *in_dev, sprs_c64 *x_dev);

/* ---------------------------------------------------------------- f32 / Complex<f32>
 * The reference is generic over cauchy::Scalar = {f32, f64, c32, c64} and its unit tests exercise f32 / c32
 * BLAS-1 (src/vecalg.rs:647-658,669-677,771-798,816-830).  Every typed entry point above exists again with
 * suffix _s (f32), _c (Complex<f32> = sprs_c32) and _cs (complex vector, real scalar/diagonal); T::Real
 * quantities (tol, residual, norm2, rscale factor) are float. */
int sprs_csr_create_s(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const float *val, int storage_csc, sprs_csr **out);
int sprs_csr_create_c(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const sprs_c32 *val, int storage_csc, sprs_csr **out);
int sprs_csr_create_i64_s(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t *row_ptr, const int64_t *col_idx, const float *val, int storage_csc, sprs_csr **out);
int sprs_csr_create_i64_c(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t *row_ptr, const int64_t *col_idx, const sprs_c32 *val, int storage_csc, sprs_csr **out);
int sprs_csr_create_dev_s(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx, const float *dev_val, int adopt, sprs_csr **out);
int sprs_csr_create_dev_c(sprs_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx, const sprs_c32 *dev_val, int adopt, sprs_csr **out);
int sprs_mul_vec_s(const sprs_csr *A, const float *x_host, size_t x_len, float *y_host, size_t y_len);
int sprs_mul_vec_c(const sprs_csr *A, const sprs_c32 *x_host, size_t x_len, sprs_c32 *y_host, size_t y_len);
int sprs_mul_vec_dot_s(const sprs_csr *A, const float *x_host, size_t x_len, float *y_host, size_t y_len, float *dot_out);
int sprs_mul_vec_dot_c(const sprs_csr *A, const sprs_c32 *x_host, size_t x_len, sprs_c32 *y_host, size_t y_len, sprs_c32 *dot_out);
int sprs_mul_vec_dev_s(const sprs_csr *A, const float *x_dev, float *y_dev);
int sprs_mul_vec_dev_c(const sprs_csr *A, const sprs_c32 *x_dev, sprs_c32 *y_dev);
int sprs_mul_vec_dot_dev_s(const sprs_csr *A, const float *x_dev, float *y_dev, float *dot_out);
int sprs_mul_vec_dot_dev_c(const sprs_csr *A, const sprs_c32 *x_dev, sprs_c32 *y_dev, sprs_c32 *dot_out);
int sprs_mul_vec_dev_timed_s(const sprs_csr *A, const float *x_dev, float *y_dev, int reps, double *ms_per_launch);
int sprs_mul_vec_dev_timed_c(const sprs_csr *A, const sprs_c32 *x_dev, sprs_c32 *y_dev, int reps, double *ms_per_launch);
int sprs_dot_s(sprs_ctx *ctx, size_t n, const float *x, const float *y, float *out);
int sprs_dot_c(sprs_ctx *ctx, size_t n, const sprs_c32 *x, const sprs_c32 *y, sprs_c32 *out);
int sprs_conj_dot_s(sprs_ctx *ctx, size_t n, const float *x, const float *y, float *out);
int sprs_conj_dot_c(sprs_ctx *ctx, size_t n, const sprs_c32 *x, const sprs_c32 *y, sprs_c32 *out);
int sprs_norm2_s(sprs_ctx *ctx, size_t n, const float *x, float *out);
int sprs_norm2_c(sprs_ctx *ctx, size_t n, const sprs_c32 *x, float *out);
int sprs_scale_s(sprs_ctx *ctx, size_t n, float a, float *x);
int sprs_scale_c(sprs_ctx *ctx, size_t n, sprs_c32 a, sprs_c32 *x);
int sprs_rscale_s(sprs_ctx *ctx, size_t n, float a, float *x);
int sprs_rscale_c(sprs_ctx *ctx, size_t n, float a, sprs_c32 *x);
int sprs_conj_s(sprs_ctx *ctx, size_t n, const float *in, float *out);
int sprs_conj_c(sprs_ctx *ctx, size_t n, const sprs_c32 *in, sprs_c32 *out);
int sprs_axpy_s(sprs_ctx *ctx, size_t n, float a, const float *x, float *y);
int sprs_axpy_c(sprs_ctx *ctx, size_t n, sprs_c32 a, const sprs_c32 *x, sprs_c32 *y);
int sprs_axpy_cs(sprs_ctx *ctx, size_t n, float a, const sprs_c32 *x, sprs_c32 *y);
int sprs_axpby_s(sprs_ctx *ctx, size_t n, float a, const float *x, float b, float *y);
int sprs_axpby_c(sprs_ctx *ctx, size_t n, sprs_c32 a, const sprs_c32 *x, sprs_c32 b, sprs_c32 *y);
int sprs_diag_precond_create_s(sprs_ctx *ctx, size_t n, const float *diag_host, sprs_diag **out);
int sprs_diag_precond_create_cs(sprs_ctx *ctx, size_t n, const float *diag_host, sprs_diag **out);
int sprs_diag_precond_create_c(sprs_ctx *ctx, size_t n, const sprs_c32 *diag_host, sprs_diag **out);
int sprs_diag_mul_vec_s(const sprs_diag *P, const float *in_host, size_t in_len, float *out_host, size_t out_len);
int sprs_diag_mul_vec_c(const sprs_diag *P, const sprs_c32 *in_host, size_t in_len, sprs_c32 *out_host, size_t out_len);
int sprs_diag_mul_vec_dev_s(const sprs_diag *P, const float *in_dev, float *out_dev);
int sprs_diag_mul_vec_dev_c(const sprs_diag *P, const sprs_c32 *in_dev, sprs_c32 *out_dev);
int sprs_bicgstab_create_s(const sprs_csr *A, size_t size, sprs_bicgstab **out);
int sprs_bicgstab_create_c(const sprs_csr *A, size_t size, sprs_bicgstab **out);
int sprs_bicgstab_solve_s(sprs_bicgstab *S, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bicgstab_solve_c(sprs_bicgstab *S, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bicgstab_precond_solve_s(sprs_bicgstab *S, const sprs_diag *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bicgstab_precond_solve_c(sprs_bicgstab *S, const sprs_diag *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bicgstab_solve_dev_s(sprs_bicgstab *S, const sprs_diag *P_or_null, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bicgstab_solve_dev_c(sprs_bicgstab *S, const sprs_diag *P_or_null, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_minres_create_s(const sprs_csr *A, size_t size, sprs_minres **out);
int sprs_minres_create_c(const sprs_csr *A, size_t size, sprs_minres **out);
int sprs_minres_solve_s(sprs_minres *S, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_minres_solve_c(sprs_minres *S, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_minres_precond_solve_s(sprs_minres *S, const sprs_diag *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_minres_precond_solve_c(sprs_minres *S, const sprs_diag *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_minres_solve_dev_s(sprs_minres *S, const sprs_diag *P_or_null, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_minres_solve_dev_c(sprs_minres *S, const sprs_diag *P_or_null, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_csminres_create_c(const sprs_csr *A, size_t size, sprs_csminres **out);
int sprs_csminres_create_s(const sprs_csr *A, size_t size, sprs_csminres **out);
int sprs_csminres_solve_c(sprs_csminres *S, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_csminres_solve_s(sprs_csminres *S, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_csminres_solve_dev_c(sprs_csminres *S, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_csminres_solve_dev_s(sprs_csminres *S, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_cg_create_s(const sprs_csr *A, size_t size, sprs_cg **out);
int sprs_cg_create_c(const sprs_csr *A, size_t size, sprs_cg **out);
int sprs_cg_solve_s(sprs_cg *S, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_cg_solve_c(sprs_cg *S, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_cg_precond_solve_s(sprs_cg *S, const sprs_diag *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_cg_precond_solve_c(sprs_cg *S, const sprs_diag *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_cg_solve_dev_s(sprs_cg *S, const sprs_diag *P_or_null, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_cg_solve_dev_c(sprs_cg *S, const sprs_diag *P_or_null, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_mul_mat_s(const sprs_csr *A, const float *x_host, size_t x_len, float *y_host, size_t y_len, size_t k);
int sprs_mul_mat_dev_s(const sprs_csr *A, const float *x_dev, float *y_dev, size_t k);
int sprs_cgmany_create_s(const sprs_csr *A, size_t size, size_t k, sprs_cg_many **out);
int sprs_cgmany_solve_s(sprs_cg_many *S, const sprs_diag *P_or_null, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t k, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_cgmany_solve_dev_s(sprs_cg_many *S, const sprs_diag *P_or_null, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t k, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_mul_mat_c(const sprs_csr *A, const sprs_c32 *x_host, size_t x_len, sprs_c32 *y_host, size_t y_len, size_t k);
int sprs_mul_mat_dev_c(const sprs_csr *A, const sprs_c32 *x_dev, sprs_c32 *y_dev, size_t k);
int sprs_cgmany_create_c(const sprs_csr *A, size_t size, size_t k, sprs_cg_many **out);
int sprs_cgmany_solve_c(sprs_cg_many *S, const sprs_diag *P_or_null, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t k, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_cgmany_solve_dev_c(sprs_cg_many *S, const sprs_diag *P_or_null, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t k, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_lsmr_create_s(const sprs_csr *A, const sprs_csr *AH_or_null, sprs_lsmr **out);
int sprs_lsmr_solve_s(sprs_lsmr *S, const float *rhs, size_t rhs_len, float *x, size_t x_len, float damp, size_t max_iter, float tol, size_t *its_out, float *res_out, float *ares_out);
int sprs_lsmr_solve_dev_s(sprs_lsmr *S, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, float damp, size_t max_iter, float tol, size_t *its_out, float *res_out, float *ares_out);
int sprs_lsmr_create_c(const sprs_csr *A, const sprs_csr *AH_or_null, sprs_lsmr **out);
int sprs_lsmr_solve_c(sprs_lsmr *S, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, float damp, size_t max_iter, float tol, size_t *its_out, float *res_out, float *ares_out);
int sprs_lsmr_solve_dev_c(sprs_lsmr *S, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, float damp, size_t max_iter, float tol, size_t *its_out, float *res_out, float *ares_out);
int sprs_gmres_create_s(const sprs_csr *A, size_t size, size_t restart, sprs_gmres **out);
int sprs_gmres_create_c(const sprs_csr *A, size_t size, size_t restart, sprs_gmres **out);
int sprs_gmres_solve_s(sprs_gmres *S, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_gmres_solve_c(sprs_gmres *S, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_gmres_precond_solve_s(sprs_gmres *S, const sprs_diag *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_gmres_precond_solve_c(sprs_gmres *S, const sprs_diag *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_gmres_solve_dev_s(sprs_gmres *S, const sprs_diag *P_or_null, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_gmres_solve_dev_c(sprs_gmres *S, const sprs_diag *P_or_null, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_dist_csr_create_dev_s(sprs_comm *comm, int64_t n_local, int64_t n_ext, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx_ext, const float *dev_val, int adopt, int n_peers, const int32_t *peer_rank, const int64_t *send_off, const int32_t *send_idx_dev, const int64_t *recv_off, sprs_csr **out);
int sprs_dist_csr_create_dev_c(sprs_comm *comm, int64_t n_local, int64_t n_ext, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx_ext, const sprs_c32 *dev_val, int adopt, int n_peers, const int32_t *peer_rank, const int64_t *send_off, const int32_t *send_idx_dev, const int64_t *recv_off, sprs_csr **out);
int sprs_dist_mul_vec_dev_s(const sprs_csr *A, float *x_ext_dev, float *y_local_dev);
int sprs_dist_mul_vec_dev_c(const sprs_csr *A, sprs_c32 *x_ext_dev, sprs_c32 *y_local_dev);

/* ---------------------------------------------------------------- ILU(0) preconditioner
 * The incomplete LU factorisation of a square, single-GPU CSR handle on A's own pattern (any of the four scalar types, taken
 * from A), and the two triangular solves that apply it: z = U^-1 (L^-1 r), L unit lower.  The reference has no such
 * preconditioner.  The handle owns everything it derives and borrows nothing from A after creation.
 * create:  SPRS_NOT_SQUARE;  SPRS_INVALID_ARGUMENT (text in sprs_last_error) for a distributed A and for a row whose column
 * indices are not strictly ascending (unsorted or duplicate);  SPRS_ZERO_DIAGONAL with *row_out = the smallest row that stores
 * no diagonal entry.  A handle created from CSC arrays is accepted (it is CSR by then).  *row_out is -1 otherwise.
 * The factorisation, in place on a copy of A's values (sdiv, ssub, smul: one scalar operation each, rounded once, complex
 * ones by the naive formulas; nothing is fused):
 *     for i = 0 .. n - 1 in order:
 *         for each stored entry of row i with column k < i, ascending:
 *             l = a_ik / u_kk;  a_ik = l
 *             for each stored entry of row i with column j > k, ascending:  if row k stores column j:  a_ij = a_ij - l*u_kj
 * After all rows: if a pivot u_ii is exactly zero or not finite, SPRS_ZERO_DIAGONAL with *row_out = the smallest such row and
 * no handle (rows downstream of that row simply carry the inf or NaN).
 * Levels: level(i) = 1 + max level(k) over the stored k < i (0 without one); for the upper solve ulevel(i) = 1 + max ulevel(j)
 * over the stored j > i, from the last row down.  The rows of one level are independent in the factorisation and in the
 * solves; the device runs level after level, one lane per row, so factors and solves have the bits of the serial loops.
 * The solves (which = 1: out = L^-1 in, 2: out = U^-1 in, 0: out = U^-1 (L^-1 in); another value is SPRS_INVALID_ARGUMENT):
 *     forward,  i = 0 .. n - 1:  sigma = 0;  for stored k < i ascending: sigma = sigma + l_ik*y_k;  y_i = r_i - sigma
 *     backward, i = n - 1 .. 0:  sigma = 0;  for stored j > i ascending: sigma = sigma + u_ij*z_j;  z_i = (y_i - sigma) / u_ii
 * (a division, not a stored reciprocal).  The factors are kept level by level in 64-row slices, slice-column-major, so a
 * wavefront's loads are coalesced; a run of consecutive levels of at most 256 rows each (at most 128 levels) is one launch of
 * one workgroup, a larger level one launch: sprs_ilu0_levels reports the levels and the launches of one solve of each kind.
 * The _dev solves are asynchronous on the context's stream; in == out is allowed; the handle owns the intermediate y of a
 * which = 0 solve, so calls on one context serialise.  Host slices of the wrong length: SPRS_DIM_MISMATCH.
 * sprs_ilu0_read: the nnz factor values at A's CSR positions, l_ik below the diagonal, u_ij on and above it.
 * Solvers: a handle of another scalar type or context than the solver's A, a distributed A, or a NULL P is
 * SPRS_INVALID_ARGUMENT; another size is SPRS_DIM_MISMATCH.  z = P r, z = P v_j and u = P u of the recurrences are the
 * which = 0 solve; everything else (events, *its_out / *res_out, trace rows, both modes) is as stated for the solvers.
 *
 * Jacobi-sweep solves.  sprs_ilu0_create_sweeps(A, sweeps, ...) fixes a handle's mode at creation: sweeps = 0 is
 * sprs_ilu0_create itself; sweeps < 0 or > SPRS_ILU0_MAX_SWEEPS is SPRS_INVALID_ARGUMENT; every other creation error is as
 * above.  The factors are those of sprs_ilu0_create (sprs_ilu0_read returns the same values).  With sweeps = k >= 1 the three
 * solves are replaced by k Jacobi sweeps from zero on each triangular system (a triangular matrix is its diagonal plus a
 * nilpotent part, so the sweeps converge for every factor).  The same scalar operations as above; every sigma is folded from
 * +0 over the row's stored entries in ascending column order, sigma = sigma + a_ij*x_j:
 *     lower (which = 1):  y(1) = in;  y(m+1)_i = in_i - sigma_i, sigma_i over l_ij, j < i, reading y(m);  out = y(k)
 *     upper (which = 2):  z(1)_i = in_i / u_ii;  z(m+1)_i = (in_i - sigma_i) / u_ii, sigma_i over u_ij, j > i, reading z(m);
 *                         out = z(k)
 *     application (which = 0):  the upper sweeps on the output of the lower sweeps.
 * Every sweep reads only the previous sweep's vector (the handle owns the vectors the sweeps alternate between; never in
 * place), so the result does not depend on the launch geometry and is the same bytes on every call.  The fold is the exact
 * solve's own expression, so a row of level l holds its final bits from sweep l + 1 on: with k >= lower_levels (upper_levels)
 * the sweeps return the exact solve bit for bit.  For Hermitian positive-definite A the k-sweep application is Hermitian
 * positive definite up to rounding, so CG may take it.
 * A sweep is one launch over the whole factor, one lane per row, the factors kept in natural row order in 64-row slices,
 * slice-column-major (no level-major copy is kept).  Lower sweep 1 is no pass; upper sweep 1 of an application is stored by
 * the last lower launch.  Launches: which = 1: k - 1 (k = 1: one device copy, nothing when in == out; k = 2 with in == out:
 * one device copy more); which = 2: k; which = 0: 2k - 2, one for k = 1.  sprs_ilu0_levels reports the level counts of the
 * pattern as for an exact handle and k - 1 / k as the two launch counts.  in == out is allowed for every `which`; `in` is
 * never written unless it is `out`.  sprs_ilu0_sweeps: k, 0 for an exact handle, -1 for NULL.  Everything that takes a
 * sprs_ilu0 (the solves, sprs_ilu0_cg_*, sprs_ilu0_gmres_*, sprs_ilu0_bicgstab_*, sprs_ilu0_minres_*) takes either kind.
 *
 * Ordered ILU(0).  sprs_ilu0_create_ordered(A, sweeps, order, perm_host, perm_len, ...) factorises B = P A P^T in place of A
 * (the orderings section above): order = SPRS_ORDER_NATURAL is sprs_ilu0_create_sweeps itself (perm ignored);
 * SPRS_ORDER_MULTICOLOR takes the stable sort of the rows by sprs_csr_color's colours with seed 0 (perm ignored);
 * SPRS_ORDER_PERM takes perm_host (new -> old, checked as by sprs_csr_permute).  With ord = the inverse of perm:
 *     B[p, q] = A[perm[p], perm[q]];   L U ~ B by the factorisation loop above, run on B
 *     which = 0:  out = P^T U^-1 L^-1 P in:   t_p = in[perm[p]];  y = L^-1 t;  z = U^-1 y  (the loops above on B's rows);  out[perm[p]] = z_p
 *     which = 1:  out = P^T L^-1 P in;   which = 2:  out = P^T U^-1 P in   (the same with one solve)
 * Vectors go in and come out in A's numbering; in == out is allowed.  The gather is the lower solve's own load and the scatter
 * the upper solve's own store, so an application costs the launches of the two solves and nothing else; the handle owns one
 * n-vector in B's numbering.  sprs_ilu0_read returns the values at A's CSR positions: entry (i, j) is l where ord(j) < ord(i)
 * and u otherwise.  sprs_ilu0_levels reports the levels and launches of B's triangles (at most the number of colours for the
 * multicolour ordering).  *row_out of SPRS_ZERO_DIAGONAL is given in A's numbering: perm[p] of the smallest offending row p of B.
 * An ordering together with sweeps != 0 is SPRS_INVALID_ARGUMENT (text in sprs_last_error): with few levels the sweeps have no
 * purpose.  sprs_ilu0_order: 1 and the n entries of perm in perm_host (may be NULL) for an ordered handle, 0 for a natural one,
 * -1 for NULL.  The solvers take an ordered handle like any other; it is checked against A, not B. */
#define SPRS_ILU0_MAX_SWEEPS 4096
#define SPRS_ORDER_NATURAL 0
#define SPRS_ORDER_MULTICOLOR 1
#define SPRS_ORDER_PERM 2
typedef struct sprs_ilu0 sprs_ilu0;
int sprs_ilu0_create(const sprs_csr *A, sprs_ilu0 **out, int64_t *row_out);   /* row_out may be NULL */
int sprs_ilu0_create_sweeps(const sprs_csr *A, int sweeps, sprs_ilu0 **out, int64_t *row_out);   /* row_out may be NULL */
int sprs_ilu0_sweeps(const sprs_ilu0 *P);
int sprs_ilu0_create_ordered(const sprs_csr *A, int sweeps, int order, const int32_t *perm_host, size_t perm_len, sprs_ilu0 **out, int64_t *row_out);   /* perm_host, row_out may be NULL */
int sprs_ilu0_order(const sprs_ilu0 *P, int32_t *perm_host);
int sprs_ilu0_destroy(sprs_ilu0 *P);           /* NULL is a no-op */
int sprs_ilu0_levels(const sprs_ilu0 *P, int64_t *lower_levels, int64_t *upper_levels, int64_t *lower_launches, int64_t *upper_launches);   /* any pointer may be NULL */
int sprs_ilu0_read(const sprs_ilu0 *P, void *val_host);
int sprs_ilu0_solve_dev_d(const sprs_ilu0 *P, int which, const double *in_dev, double *out_dev);
int sprs_ilu0_solve_dev_z(const sprs_ilu0 *P, int which, const sprs_c64 *in_dev, sprs_c64 *out_dev);
int sprs_ilu0_solve_dev_s(const sprs_ilu0 *P, int which, const float *in_dev, float *out_dev);
int sprs_ilu0_solve_dev_c(const sprs_ilu0 *P, int which, const sprs_c32 *in_dev, sprs_c32 *out_dev);
int sprs_ilu0_solve_d(const sprs_ilu0 *P, int which, const double *in_host, size_t in_len, double *out_host, size_t out_len);
int sprs_ilu0_solve_z(const sprs_ilu0 *P, int which, const sprs_c64 *in_host, size_t in_len, sprs_c64 *out_host, size_t out_len);
int sprs_ilu0_solve_s(const sprs_ilu0 *P, int which, const float *in_host, size_t in_len, float *out_host, size_t out_len);
int sprs_ilu0_solve_c(const sprs_ilu0 *P, int which, const sprs_c32 *in_host, size_t in_len, sprs_c32 *out_host, size_t out_len);
/* CG and GMRES preconditioned by ILU(0): the recurrences of sprs_cg_* and sprs_gmres_* with P = the which = 0 solve */
int sprs_ilu0_cg_solve_d(sprs_cg *S, const sprs_ilu0 *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_cg_solve_z(sprs_cg *S, const sprs_ilu0 *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_cg_solve_s(sprs_cg *S, const sprs_ilu0 *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_cg_solve_c(sprs_cg *S, const sprs_ilu0 *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_cg_solve_dev_d(sprs_cg *S, const sprs_ilu0 *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_cg_solve_dev_z(sprs_cg *S, const sprs_ilu0 *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_cg_solve_dev_s(sprs_cg *S, const sprs_ilu0 *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_cg_solve_dev_c(sprs_cg *S, const sprs_ilu0 *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_gmres_solve_d(sprs_gmres *S, const sprs_ilu0 *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_gmres_solve_z(sprs_gmres *S, const sprs_ilu0 *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_gmres_solve_s(sprs_gmres *S, const sprs_ilu0 *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_gmres_solve_c(sprs_gmres *S, const sprs_ilu0 *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_gmres_solve_dev_d(sprs_gmres *S, const sprs_ilu0 *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_gmres_solve_dev_z(sprs_gmres *S, const sprs_ilu0 *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_gmres_solve_dev_s(sprs_gmres *S, const sprs_ilu0 *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_gmres_solve_dev_c(sprs_gmres *S, const sprs_ilu0 *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
/* BiCGStab and MINRES preconditioned by ILU(0): the recurrences of sprs_bicgstab_precond_solve_* and
 * sprs_minres_precond_solve_* with P = the which = 0 solve wherever those multiply by the diagonal; arguments and status codes
 * as sprs_ilu0_cg_solve_*.
 *   BiCGStab (right preconditioning):  y = P p before v = A y and z = P s before t = A z (s = r - alpha v);
 *     x -= alpha y ; x -= w z ; r = s - w t.  P need not be symmetric.  A fused iteration is five launches of the solver's
 *     plus two applications, without a host wait.
 *   MINRES:  w_new = P v_new after v_new = A w - beta v_old - alpha v, then b2 = conj(v_new).w_new and beta_new = sqrt(re b2).
 *     SPRS_INVALID_PRECOND (its_out = the iteration, res_out = re b2) when re(b2) < eps or im(b2) > eps re(b2) — the rule of
 *     the diagonal solve, unchanged.  P must be Hermitian positive definite: ILU(0) of a Hermitian positive-definite M-matrix
 *     is; with an applied P on complex data im(b2) is rounding noise and no longer an exact zero, so the rule can in principle
 *     fire on a valid P if that noise grows past eps re(b2).  A fused iteration is four launches of the solver's plus one
 *     application.
 * CSMINRES takes no preconditioner; the batched CG takes a diagonal only. */
int sprs_ilu0_bicgstab_solve_d(sprs_bicgstab *S, const sprs_ilu0 *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_bicgstab_solve_z(sprs_bicgstab *S, const sprs_ilu0 *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_bicgstab_solve_s(sprs_bicgstab *S, const sprs_ilu0 *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_bicgstab_solve_c(sprs_bicgstab *S, const sprs_ilu0 *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_bicgstab_solve_dev_d(sprs_bicgstab *S, const sprs_ilu0 *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_bicgstab_solve_dev_z(sprs_bicgstab *S, const sprs_ilu0 *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_bicgstab_solve_dev_s(sprs_bicgstab *S, const sprs_ilu0 *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_bicgstab_solve_dev_c(sprs_bicgstab *S, const sprs_ilu0 *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_minres_solve_d(sprs_minres *S, const sprs_ilu0 *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_minres_solve_z(sprs_minres *S, const sprs_ilu0 *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_minres_solve_s(sprs_minres *S, const sprs_ilu0 *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_minres_solve_c(sprs_minres *S, const sprs_ilu0 *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_minres_solve_dev_d(sprs_minres *S, const sprs_ilu0 *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_minres_solve_dev_z(sprs_minres *S, const sprs_ilu0 *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_minres_solve_dev_s(sprs_minres *S, const sprs_ilu0 *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_minres_solve_dev_c(sprs_minres *S, const sprs_ilu0 *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);

/* ---------------------------------------------------------------- smoothed-aggregation AMG preconditioner
 * An algebraic multigrid hierarchy of a square, single-GPU CSR handle (any of the four scalar types, taken from A) and the
 * V(1,1) cycle that applies it.  The reference has no such preconditioner.  The handle owns everything it derives (host copies
 * of every level included) and borrows nothing from A after creation.
 * create(A, theta, coarse_max, max_levels):  SPRS_NOT_SQUARE;  SPRS_INVALID_ARGUMENT (text in sprs_last_error) for a distributed
 * A, a row whose column indices are not strictly ascending, theta < 0 or NaN, coarse_max outside 1 .. 1024, max_levels outside
 * 1 .. 32;  SPRS_ZERO_DIAGONAL with *row_out = the smallest row OF THE LEVEL BEING BUILT that stores no diagonal entry or whose
 * diagonal is exactly zero or not finite, or the row of a zero or non-finite pivot of the coarse LU.  *row_out is -1 otherwise.
 * The hierarchy is built on the host, serially, from one copy of A; every scalar operation is rounded once, complex ones by
 * the naive formulas, nothing is fused.  |a| is fabs(a), for a complex a sqrt(re*re + im*im); |a|^2 is a*a or re*re + im*im.
 * Level l (A_0 = A), with d_i its diagonal:
 *   omega_l = 4 / (3 * rho),  rho = max_i (s_i / |d_i|),  s_i = sum over the stored j of |a_ij|, left to right from zero.
 *   It is the coarsest level when it has at most coarse_max rows or l + 1 == max_levels.
 *   Strength, theta_l = theta * 2^-l:  a stored j != i is strong for row i when |a_ij|^2 >= (theta_l*theta_l) * (|d_i| * |d_j|).
 *   Aggregation, three passes over the rows in ascending order:
 *     1. an unaggregated row none of whose strong neighbours is aggregated founds the next aggregate with them (a row without
 *        strong neighbours founds a singleton);
 *     2. a row left over joins the aggregate that its strong neighbour of largest |a_ij|^2 had AFTER PASS 1 (pass 2 reads a
 *        snapshot; the first of equal neighbours wins; neighbours unaggregated in the snapshot do not count);
 *     3. a row still left founds the next aggregate with its strong neighbours that are still unaggregated.
 *        (A row is left by pass 1 only because a strong neighbour of its was aggregated by then, and pass 2 places it with one
 *        of those: as the rules stand pass 3 finds no row.  It is kept as the guard that every row ends in an aggregate.)
 *   If the aggregates number more than half the rows, level l is the coarsest after all (the half-rows stop).
 *   Products run row by row in Gustavson order: for a_ik with k ascending, for b_kj with j ascending, acc_j = acc_j + a_ik*b_kj,
 *   acc from zero; the stored pattern is the structural one (exact zeros are kept), columns ascending.
 *   T has a 1 at (i, agg(i)).  P = T - omega D^-1 A T entry by entry on the pattern of the product A T:
 *   p_ic = t_ic - ((A T)_ic * omega_l) / d_i.   R = P^H.   A_{l+1} = R (A P), the inner product first.
 *   (theta_l halves per level, Vanek's rule: DESIGN.md §4h has the level sizes it gives.)
 * Coarse solve.  At most coarse_max rows: the dense no-pivot LU of the coarsest A in the k-i-j order (l_ik = a_ik / a_kk, then
 * a_ij = a_ij - l_ik*a_kj), applied as  w = b;  for j ascending: w_i = w_i - l_ij*w_j (i > j);  then for j descending:
 * x_j = w_j / u_jj, w_i = w_i - u_ij*x_j (i < j).  More rows (the half-rows stop or max_levels ended the coarsening early):
 * eight damped-Jacobi sweeps from zero, i.e. the pre-smoothing formula followed by seven sweeps of the post-smoothing one.
 * The cycle on level l, right-hand side b (sigma = sum over a row's stored entries, left to right from zero):
 *     x_i = (b_i*omega_l) / d_i;   r_i = b_i - sigma_i(A x);   b' = R r (b'_c = sigma_c);   e = cycle(l + 1, b');
 *     x_i = x_i + sigma_i(P e);    result_i = x_i + ((b_i - sigma_i(A x))*omega_l) / d_i.
 * One lane folds one row, so an application has the bits of these loops.  Every operator is kept in 64-row slices,
 * slice-column-major; the levels of at most 1024 rows (AMG_TAIL_ROWS) run in ONE launch of ONE workgroup, down, coarse solve and
 * up; each larger level takes five launches.  sprs_amg_info: the levels, the launches of one application, the first level of
 * the tail (== levels when there is none) and the rows of the coarse LU (0: Jacobi sweeps).  sprs_amg_level_info: rows, nnz(A_l),
 * nnz(P_l) (0 on the coarsest level) and omega_l.  sprs_amg_level_read: the CSR arrays of A_l (which = 0), P_l (1) or R_l (2) and
 * the aggregate of every row of level l, into host arrays; any pointer may be NULL; P, R and aggregates of the coarsest level
 * are SPRS_INVALID_ARGUMENT.
 * mul_vec: out = one cycle on in.  The _dev form is asynchronous on the context's stream; in == out is allowed; the handle
 * owns the level vectors, so calls on one context serialise.  Host slices of the wrong length: SPRS_DIM_MISMATCH.
 * Solvers: as for ILU(0) (same errors); z = P r, z = P v_j and u = P u of the recurrences are one cycle.  The cycle is
 * Hermitian positive definite when A is, so it is a valid CG preconditioner; on an indefinite A, CG ends in
 * SPRS_INVALID_PRECOND as with any preconditioner that is not positive definite.
 *
 * create_dev(A, theta, coarse_max, max_levels, seed) builds the same handle without the host: every step of a
 * level runs in HBM, and the three serial aggregation passes are replaced by a rule that a few parallel rounds reproduce exactly.
 * The refusals, their order and *row_out are create's (unsorted or duplicate columns are looked for on the device: the smallest
 * such row is named).  Everything above holds as it stands — omega, theta_l, the strength test, the products, P, R, the stop
 * rules, the coarse LU (on the host, from a download of the coarsest operator), the cycle — except "Aggregation", which reads:
 *   G:  i ~ j when (i, j) or (j, i) is a strong stored entry; w(i, j) = the largest |a|^2 among those of the two that are strong.
 *   key(i) = (splitmix64(seed, i), i), compared lexicographically; splitmix64 is sprs_csr_color's:
 *     z = seed + (i + 1) * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31.
 *   1. root[.] = -1;  for i in decreasing key(i):
 *          if root[i] < 0 and root[j] < 0 for every j ~ i:   root[i] = i;  root[j] = i for every j ~ i
 *      (a vertex without neighbours is a root on its own).
 *   2. snap = root;  for every i with snap[i] < 0:
 *          j* = the j ~ i with snap[j] >= 0 of largest w(i, j), the smallest such j among equals;   root[i] = snap[j*]
 *      After a maximal pass 1 a free vertex has an aggregated neighbour, so j* exists and there is no pass 3; the device checks
 *      it (a row without j* is SPRS_ERR_HIP, "internal error", never an unplaced row).
 *   3. agg(i) = the number of roots below root[i]: aggregates are numbered by ascending root.
 * The device runs pass 1 as rounds.  Every vertex is undecided at first.  A round: an undecided vertex that is aggregated or has
 * an aggregated neighbour stops being undecided (it can never be a root); if none is undecided pass 1 is over; otherwise the
 * round counts, and every undecided vertex whose key is the largest among the undecided vertices within two edges of it becomes
 * a root and takes its neighbours.  Two winners of a round are more than two edges apart, a root decided earlier lies beyond two
 * edges, and "never a root" is final because aggregation only grows: the rounds give loop 1's root[] whatever the launch geometry.
 * No floating-point atomic is used; integer atomics count and hand out list slots whose order reaches no result.  The same seed
 * gives the same handle, byte for byte; another seed gives other aggregates.  Aggregates are not bounded in size (a hub takes all
 * its neighbours).
 * A device-built handle keeps no host copy and no second device copy of its operators: sprs_amg_level_read unpacks the CSR arrays
 * from the sliced-row layout (which holds every row's length, columns and values in stored order) and reads the aggregates from
 * the 4 bytes a row kept in HBM.  sprs_amg_setup_info: *setup = 0 (create) or 1 (create_dev); rounds[l] = pass 1's rounds on
 * level l for l < rounds_len (0 for the coarsest level, beyond it, and throughout a host-built handle).  sprs_amg_setup_stage_ms:
 * a diagnostic, off unless the environment variable SPRS_CREATE_TRACE is set when create_dev runs (it then drains the stream at
 * every stage boundary; otherwise creation pays no such drain and every entry is 0): host-clock milliseconds per stage, summed
 * over the levels, in the order diagonal and omega, graph, rounds, pass 2 and numbering, A T, prolongator, adjoint, A P, R (A P),
 * packing, coarse download and LU; entries beyond the eleventh and every entry of a host-built handle are 0. */
typedef struct sprs_amg sprs_amg;
int sprs_amg_create(const sprs_csr *A, double theta, int64_t coarse_max, int64_t max_levels, sprs_amg **out, int64_t *row_out);   /* row_out may be NULL */
int sprs_amg_create_dev(const sprs_csr *A, double theta, int64_t coarse_max, int64_t max_levels, uint64_t seed, sprs_amg **out, int64_t *row_out);   /* row_out may be NULL */
int sprs_amg_setup_info(const sprs_amg *P, int64_t *setup, int64_t *rounds, size_t rounds_len);   /* setup may be NULL; rounds may be NULL when rounds_len is 0 */
int sprs_amg_setup_stage_ms(const sprs_amg *P, double *ms, size_t ms_len);
int sprs_amg_destroy(sprs_amg *P);             /* NULL is a no-op */
int sprs_amg_info(const sprs_amg *P, int64_t *levels, int64_t *launches, int64_t *tail_level, int64_t *lu_rows);   /* any pointer may be NULL */
int sprs_amg_level_info(const sprs_amg *P, int64_t level, int64_t *rows, int64_t *nnz, int64_t *p_nnz, double *omega);
int sprs_amg_level_read(const sprs_amg *P, int64_t level, int which, int32_t *row_ptr_host, int32_t *col_idx_host, void *val_host, int32_t *agg_host);
int sprs_amg_mul_vec_dev_d(const sprs_amg *P, const double *in_dev, double *out_dev);
int sprs_amg_mul_vec_dev_z(const sprs_amg *P, const sprs_c64 *in_dev, sprs_c64 *out_dev);
int sprs_amg_mul_vec_dev_s(const sprs_amg *P, const float *in_dev, float *out_dev);
int sprs_amg_mul_vec_dev_c(const sprs_amg *P, const sprs_c32 *in_dev, sprs_c32 *out_dev);
int sprs_amg_mul_vec_d(const sprs_amg *P, const double *in_host, size_t in_len, double *out_host, size_t out_len);
int sprs_amg_mul_vec_z(const sprs_amg *P, const sprs_c64 *in_host, size_t in_len, sprs_c64 *out_host, size_t out_len);
int sprs_amg_mul_vec_s(const sprs_amg *P, const float *in_host, size_t in_len, float *out_host, size_t out_len);
int sprs_amg_mul_vec_c(const sprs_amg *P, const sprs_c32 *in_host, size_t in_len, sprs_c32 *out_host, size_t out_len);
/* CG and GMRES preconditioned by AMG: the recurrences of sprs_cg_* and sprs_gmres_* with P = one cycle */
int sprs_amg_cg_solve_d(sprs_cg *S, const sprs_amg *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_cg_solve_z(sprs_cg *S, const sprs_amg *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_cg_solve_s(sprs_cg *S, const sprs_amg *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_cg_solve_c(sprs_cg *S, const sprs_amg *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_cg_solve_dev_d(sprs_cg *S, const sprs_amg *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_cg_solve_dev_z(sprs_cg *S, const sprs_amg *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_cg_solve_dev_s(sprs_cg *S, const sprs_amg *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_cg_solve_dev_c(sprs_cg *S, const sprs_amg *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_gmres_solve_d(sprs_gmres *S, const sprs_amg *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_gmres_solve_z(sprs_gmres *S, const sprs_amg *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_gmres_solve_s(sprs_gmres *S, const sprs_amg *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_gmres_solve_c(sprs_gmres *S, const sprs_amg *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_gmres_solve_dev_d(sprs_gmres *S, const sprs_amg *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_gmres_solve_dev_z(sprs_gmres *S, const sprs_amg *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_gmres_solve_dev_s(sprs_gmres *S, const sprs_amg *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_gmres_solve_dev_c(sprs_gmres *S, const sprs_amg *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
/* BiCGStab and MINRES preconditioned by AMG: as sprs_ilu0_bicgstab_* / sprs_ilu0_minres_* with P = one cycle (Hermitian
 * positive definite when A is; on an indefinite A, MINRES ends in SPRS_INVALID_PRECOND) */
int sprs_amg_bicgstab_solve_d(sprs_bicgstab *S, const sprs_amg *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_bicgstab_solve_z(sprs_bicgstab *S, const sprs_amg *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_bicgstab_solve_s(sprs_bicgstab *S, const sprs_amg *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_bicgstab_solve_c(sprs_bicgstab *S, const sprs_amg *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_bicgstab_solve_dev_d(sprs_bicgstab *S, const sprs_amg *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_bicgstab_solve_dev_z(sprs_bicgstab *S, const sprs_amg *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_bicgstab_solve_dev_s(sprs_bicgstab *S, const sprs_amg *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_bicgstab_solve_dev_c(sprs_bicgstab *S, const sprs_amg *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_minres_solve_d(sprs_minres *S, const sprs_amg *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_minres_solve_z(sprs_minres *S, const sprs_amg *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_minres_solve_s(sprs_minres *S, const sprs_amg *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_minres_solve_c(sprs_minres *S, const sprs_amg *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_minres_solve_dev_d(sprs_minres *S, const sprs_amg *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_minres_solve_dev_z(sprs_minres *S, const sprs_amg *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_minres_solve_dev_s(sprs_minres *S, const sprs_amg *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_minres_solve_dev_c(sprs_minres *S, const sprs_amg *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);

/* ---------------------------------------------------------------- factorised sparse approximate inverse (FSAI) preconditioner
 * M = G^H G, G sparse lower triangular on a pattern fixed up front, for a square single-GPU CSR handle of any of the four
 * scalar types that is Hermitian positive definite.  The reference has no such preconditioner.  Applying M is two ordinary
 * SpMVs, so there are no dependent launches and no levels; M is Hermitian positive definite by construction, so CG and MINRES
 * never end in SPRS_INVALID_PRECOND with it.  The handle owns everything it derives and borrows nothing from A after creation.
 * A is TAKEN as Hermitian: only stored entries a(r, c) with c <= r are ever read, and nothing checks the upper triangle.
 * create(A, power):  SPRS_NOT_SQUARE;  SPRS_INVALID_ARGUMENT (text in sprs_last_error) for a distributed A, power other than
 * 1 or 2, a row whose column indices are not strictly ascending, and a row of G above the cap (below).  *row_out is -1 unless
 * stated.  Every scalar operation is in the handle's scalar type and rounded once, complex products are (ac - bd, ad + bc),
 * sqrt and / are correctly rounded, nothing is fused.
 * 1. Pattern.  P = pattern(A) for power 1; for power 2 the structural pattern of A A: row i is the union of the patterns of
 *    the rows k of A over the stored columns k of row i (an entry that cancels to zero stays).  Row i of G has the columns
 *    J_i = { j in P_i : j <= i }, ascending: j_0 < ... < j_{m-1}.  If i is not in J_i, or a(i, i) is not stored:
 *    SPRS_ZERO_DIAGONAL with *row_out = the smallest such row.  Else if m > SPRS_FSAI_MAX_ROW: SPRS_INVALID_ARGUMENT, and
 *    sprs_last_error names the smallest such row and its length; nothing is truncated.
 * 2. The local matrix.  For q <= p: s_pq = a(j_p, j_q), read from row j_p of A, +0 where that entry is not stored; the
 *    diagonal takes re(a(j_p, j_p)) only.
 * 3. Cholesky S = C C^H, column q = 0 .. m - 1:
 *        d = re(s_qq);  for k = 0 .. q - 1 ascending:  d = d - (re(c_qk)*re(c_qk) + im(c_qk)*im(c_qk))   [real: d - c_qk*c_qk]
 *        d not finite or d <= 0:  A is not positive definite on this pattern: SPRS_INVALID_PRECOND, *row_out = the smallest
 *        such row i (SPRS_ZERO_DIAGONAL wins where both occur);   c_qq = sqrt(d), real
 *        for p > q:  t = s_pq;  for k = 0 .. q - 1 ascending:  t = t - c_pk*conj(c_qk);   c_pq = t / c_qq, component-wise
 * 4. The row of G (the conjugate of C^-H e_last):
 *        g_{m-1} = 1 / c_{m-1,m-1};  for p = m - 2 .. 0:  acc = +0;  for q = m - 1 down to p + 1:  acc = acc + c_qp*g_q
 *        (no conjugate);  g_p = (-acc) / c_pp, component-wise;   G(i, j_p) = g_p.
 *    Every element's updates come in a fixed order, so any loop nest and lane mapping gives the same bits.  diag(G A G^H) = 1
 *    up to rounding; where J_i is the whole lower triangle, G^H G = A^-1.
 * 5. Application.  out = GH (G in): two SpMVs on two ordinary handles, G (adopting the arrays built on the device) and
 *    GH = sprs_csr_adjoint(G, 1), each with whatever stream format its creation found; the result has the bits of the
 *    SpMV's row fold on every route.  The handle owns the intermediate vector, so calls on one context serialise; the _dev
 *    form is asynchronous on the context's stream; in == out is allowed.  Host slices of the wrong length: SPRS_DIM_MISMATCH.
 * Steps 2 to 4 run on the device in one pass over the rows, binned by length (csrc/fsai.hip).
 * sprs_fsai_info: rows, nnz(G), the longest row of G and the power; any pointer may be NULL.  sprs_fsai_factor: a BORROWED
 * handle, which = 0: G, 1: GH (another value is SPRS_INVALID_ARGUMENT); it lives as long as P and is not destroyed by the
 * caller; sprs_csr_read, sprs_csr_stream_format and sprs_mul_vec_* take it like any handle.
 * Solvers: as for ILU(0) (same errors); z = P r, z = P v_j and u = P u of the recurrences are one application. */
#define SPRS_FSAI_MAX_ROW 64
typedef struct sprs_fsai sprs_fsai;
int sprs_fsai_create(const sprs_csr *A, int power, sprs_fsai **out, int64_t *row_out);   /* row_out may be NULL */
int sprs_fsai_destroy(sprs_fsai *P);           /* NULL is a no-op */
int sprs_fsai_info(const sprs_fsai *P, int64_t *n, int64_t *nnz_g, int64_t *max_row, int64_t *power);
int sprs_fsai_factor(const sprs_fsai *P, int which, const sprs_csr **out);
int sprs_fsai_mul_vec_dev_d(const sprs_fsai *P, const double *in_dev, double *out_dev);
int sprs_fsai_mul_vec_dev_z(const sprs_fsai *P, const sprs_c64 *in_dev, sprs_c64 *out_dev);
int sprs_fsai_mul_vec_dev_s(const sprs_fsai *P, const float *in_dev, float *out_dev);
int sprs_fsai_mul_vec_dev_c(const sprs_fsai *P, const sprs_c32 *in_dev, sprs_c32 *out_dev);
int sprs_fsai_mul_vec_d(const sprs_fsai *P, const double *in_host, size_t in_len, double *out_host, size_t out_len);
int sprs_fsai_mul_vec_z(const sprs_fsai *P, const sprs_c64 *in_host, size_t in_len, sprs_c64 *out_host, size_t out_len);
int sprs_fsai_mul_vec_s(const sprs_fsai *P, const float *in_host, size_t in_len, float *out_host, size_t out_len);
int sprs_fsai_mul_vec_c(const sprs_fsai *P, const sprs_c32 *in_host, size_t in_len, sprs_c32 *out_host, size_t out_len);
/* CG, GMRES, BiCGStab and MINRES preconditioned by FSAI: as sprs_ilu0_*_solve_* with P = one application */
int sprs_fsai_cg_solve_d(sprs_cg *S, const sprs_fsai *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_cg_solve_z(sprs_cg *S, const sprs_fsai *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_cg_solve_s(sprs_cg *S, const sprs_fsai *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_cg_solve_c(sprs_cg *S, const sprs_fsai *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_cg_solve_dev_d(sprs_cg *S, const sprs_fsai *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_cg_solve_dev_z(sprs_cg *S, const sprs_fsai *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_cg_solve_dev_s(sprs_cg *S, const sprs_fsai *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_cg_solve_dev_c(sprs_cg *S, const sprs_fsai *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_gmres_solve_d(sprs_gmres *S, const sprs_fsai *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_gmres_solve_z(sprs_gmres *S, const sprs_fsai *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_gmres_solve_s(sprs_gmres *S, const sprs_fsai *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_gmres_solve_c(sprs_gmres *S, const sprs_fsai *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_gmres_solve_dev_d(sprs_gmres *S, const sprs_fsai *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_gmres_solve_dev_z(sprs_gmres *S, const sprs_fsai *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_gmres_solve_dev_s(sprs_gmres *S, const sprs_fsai *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_gmres_solve_dev_c(sprs_gmres *S, const sprs_fsai *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_bicgstab_solve_d(sprs_bicgstab *S, const sprs_fsai *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_bicgstab_solve_z(sprs_bicgstab *S, const sprs_fsai *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_bicgstab_solve_s(sprs_bicgstab *S, const sprs_fsai *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_bicgstab_solve_c(sprs_bicgstab *S, const sprs_fsai *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_bicgstab_solve_dev_d(sprs_bicgstab *S, const sprs_fsai *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_bicgstab_solve_dev_z(sprs_bicgstab *S, const sprs_fsai *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_bicgstab_solve_dev_s(sprs_bicgstab *S, const sprs_fsai *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_bicgstab_solve_dev_c(sprs_bicgstab *S, const sprs_fsai *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_minres_solve_d(sprs_minres *S, const sprs_fsai *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_minres_solve_z(sprs_minres *S, const sprs_fsai *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_minres_solve_s(sprs_minres *S, const sprs_fsai *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_minres_solve_c(sprs_minres *S, const sprs_fsai *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_minres_solve_dev_d(sprs_minres *S, const sprs_fsai *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_minres_solve_dev_z(sprs_minres *S, const sprs_fsai *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_minres_solve_dev_s(sprs_minres *S, const sprs_fsai *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_minres_solve_dev_c(sprs_minres *S, const sprs_fsai *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);

/* IDR(s) preconditioned by ILU(0), AMG or FSAI: the recurrence of sprs_idrs_* with P = the handle's application */
int sprs_ilu0_idrs_solve_d(sprs_idrs *S, const sprs_ilu0 *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_idrs_solve_z(sprs_idrs *S, const sprs_ilu0 *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_idrs_solve_s(sprs_idrs *S, const sprs_ilu0 *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_idrs_solve_c(sprs_idrs *S, const sprs_ilu0 *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_idrs_solve_dev_d(sprs_idrs *S, const sprs_ilu0 *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_idrs_solve_dev_z(sprs_idrs *S, const sprs_ilu0 *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_ilu0_idrs_solve_dev_s(sprs_idrs *S, const sprs_ilu0 *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_ilu0_idrs_solve_dev_c(sprs_idrs *S, const sprs_ilu0 *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_idrs_solve_d(sprs_idrs *S, const sprs_amg *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_idrs_solve_z(sprs_idrs *S, const sprs_amg *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_idrs_solve_s(sprs_idrs *S, const sprs_amg *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_idrs_solve_c(sprs_idrs *S, const sprs_amg *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_idrs_solve_dev_d(sprs_idrs *S, const sprs_amg *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_idrs_solve_dev_z(sprs_idrs *S, const sprs_amg *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_amg_idrs_solve_dev_s(sprs_idrs *S, const sprs_amg *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_amg_idrs_solve_dev_c(sprs_idrs *S, const sprs_amg *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_idrs_solve_d(sprs_idrs *S, const sprs_fsai *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_idrs_solve_z(sprs_idrs *S, const sprs_fsai *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_idrs_solve_s(sprs_idrs *S, const sprs_fsai *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_idrs_solve_c(sprs_idrs *S, const sprs_fsai *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_idrs_solve_dev_d(sprs_idrs *S, const sprs_fsai *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_idrs_solve_dev_z(sprs_idrs *S, const sprs_fsai *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_fsai_idrs_solve_dev_s(sprs_idrs *S, const sprs_fsai *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_fsai_idrs_solve_dev_c(sprs_idrs *S, const sprs_fsai *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);

/* ---------------------------------------------------------------- block-Jacobi preconditioner
 * M = blockdiag(A_bb)^-1 for a square single-GPU CSR handle of any of the four scalar types: the diagonal blocks of A, inverted
 * on the device at creation and stored densely; applying M is one launch of small dense products, with no levels and no
 * dependent launches.  The reference has no such preconditioner.  Block b covers the rows and columns [s_b, e_b),
 * 1 <= m = e_b - s_b <= SPRS_BJACOBI_MAX_BLOCK: several unknowns of one grid node, or one grid line.  The handle owns
 * everything it derives and borrows nothing from A after creation.
 * create(A, block_size, block_ptr, nblocks): the checks, in this order.  SPRS_INVALID_ARGUMENT (text in sprs_last_error) for a
 * distributed A;  SPRS_NOT_SQUARE;  SPRS_INVALID_ARGUMENT (text) unless exactly one of block_size > 0 and block_ptr != NULL is
 * given, for a block_ptr (nblocks + 1 entries) that does not start at 0, does not increase strictly or does not end at n, for a
 * block of more than SPRS_BJACOBI_MAX_BLOCK rows, and for a row of A whose column indices are not strictly ascending (the check
 * of FSAI and ILU(0));  SPRS_INVALID_PRECOND with *row_out = s_b of the lowest singular block (below).  *row_out is -1
 * otherwise, *out is NULL after every failure.  block_size = bs stands for block_ptr = 0, bs, 2 bs, .., n: the last block takes
 * what is left (nblocks is not read then).
 * Every scalar operation is in the handle's scalar type and rounded once, complex products are (ac - bd, ad + bc), the complex
 * quotient a / b is ((re a re b + im a im b) / d, (im a re b - re a im b) / d) with d = re b re b + im b im b, nothing is fused.
 * 1. The local matrix.  W[i][j] = the stored a(s_b + i, s_b + j), +0 where nothing is stored.  A missing diagonal entry is no
 *    error: the elimination pivots.
 * 2. The inverse: Gauss-Jordan on [W | V], V = I, with implicit row pivoting.  For k = 0 .. m - 1:
 *      mag(a) = |re a| + |im a| (one addition; |a| for the real types).  Over the rows i not yet used as a pivot row, ascending:
 *      p = the first of them, and every later one replaces p where mag(W[i][k]) > mag(W[p][k]) (so the lowest row wins a tie and
 *      a NaN never replaces anything).  mag(W[p][k]) zero or not finite: the block is singular.  Else perm[k] = p, piv = W[p][k];
 *      W[p][j] = W[p][j] / piv and V[p][j] = V[p][j] / piv for every j;
 *      for every i != p:  f = W[i][k];  W[i][j] = W[i][j] - f * W[p][j] and V[i][j] = V[i][j] - f * V[p][j] for every j
 *      (one product and one difference per update).
 *    The loops run over ALL j = 0 .. m - 1, structural zeros and the columns already eliminated included: the signs of the zeros
 *    are part of the result.  Every element's updates come in the order of k, so any lane mapping gives the same bits.  Row k of
 *    the inverse is V[perm[k]].
 * 3. Application.  out[s_b + i] = sum_j Minv[i][j] * in[s_b + j], j = 0 .. m - 1 ascending from +0, acc = acc + Minv[i][j] * in[..]
 *    (the row fold of the sliced layouts).  The _dev form is asynchronous on the context's stream; in == out is allowed, and the
 *    device vectors need the alignment of one element only.  Host slices of the wrong length: SPRS_DIM_MISMATCH.
 * Storage (csrc/bjacobi_plan.hpp): the inverse blocks sit in slices of 64 lanes, whole consecutive blocks a slice, entry (i, j) of
 * the block whose row i is at lane l in slot sbase[slice] + 64 j + l; a slice is as wide as its largest block.
 * sprs_bjacobi_info: rows, blocks, the largest block and the slots of that storage; any pointer may be NULL.
 * sprs_bjacobi_block_ptr: the nblocks + 1 block starts.  sprs_bjacobi_inverse_*: every inverse block on the host, row-major, one
 * block after another, sum of m^2 entries (len: what out holds; another length is SPRS_DIM_MISMATCH).
 * Solvers: as for ILU(0) (same errors); z = P r, z = P v_j and u = P u of the recurrences are one application.  M is Hermitian
 * positive definite where A is, up to rounding: CG takes it as it takes FSAI.  MINRES with COMPLEX scalars is wired but not
 * usable in general: its rule for SPRS_INVALID_PRECOND rejects im(conj(v) . M v) > eps * re(..), and with dense complex blocks
 * that imaginary part is rounding noise of just that size (measured 2.7e-16 .. 2.2e-15 against 2.2e-16), so such a solve ends
 * with that status after a few iterations.  The rule is the reference's and is not loosened; use CG there. */
#define SPRS_BJACOBI_MAX_BLOCK 32
typedef struct sprs_bjacobi sprs_bjacobi;
int sprs_bjacobi_create(const sprs_csr *A, int64_t block_size, const int64_t *block_ptr_or_null, int64_t nblocks, sprs_bjacobi **out, int64_t *row_out);   /* row_out may be NULL */
int sprs_bjacobi_destroy(sprs_bjacobi *P);     /* NULL is a no-op */
int sprs_bjacobi_info(const sprs_bjacobi *P, int64_t *n, int64_t *nblocks, int64_t *max_block, int64_t *slots);
int sprs_bjacobi_block_ptr(const sprs_bjacobi *P, int64_t *block_ptr_out);
int sprs_bjacobi_inverse_d(const sprs_bjacobi *P, double *out_host, size_t len);
int sprs_bjacobi_inverse_z(const sprs_bjacobi *P, sprs_c64 *out_host, size_t len);
int sprs_bjacobi_inverse_s(const sprs_bjacobi *P, float *out_host, size_t len);
int sprs_bjacobi_inverse_c(const sprs_bjacobi *P, sprs_c32 *out_host, size_t len);
int sprs_bjacobi_mul_vec_dev_d(const sprs_bjacobi *P, const double *in_dev, double *out_dev);
int sprs_bjacobi_mul_vec_dev_z(const sprs_bjacobi *P, const sprs_c64 *in_dev, sprs_c64 *out_dev);
int sprs_bjacobi_mul_vec_dev_s(const sprs_bjacobi *P, const float *in_dev, float *out_dev);
int sprs_bjacobi_mul_vec_dev_c(const sprs_bjacobi *P, const sprs_c32 *in_dev, sprs_c32 *out_dev);
int sprs_bjacobi_mul_vec_d(const sprs_bjacobi *P, const double *in_host, size_t in_len, double *out_host, size_t out_len);
int sprs_bjacobi_mul_vec_z(const sprs_bjacobi *P, const sprs_c64 *in_host, size_t in_len, sprs_c64 *out_host, size_t out_len);
int sprs_bjacobi_mul_vec_s(const sprs_bjacobi *P, const float *in_host, size_t in_len, float *out_host, size_t out_len);
int sprs_bjacobi_mul_vec_c(const sprs_bjacobi *P, const sprs_c32 *in_host, size_t in_len, sprs_c32 *out_host, size_t out_len);
/* CG, GMRES, BiCGStab and MINRES preconditioned by block-Jacobi: as sprs_ilu0_*_solve_* with P = one application.  IDR(s) and
 * LOBPCG do not take the handle yet. */
int sprs_bjacobi_cg_solve_d(sprs_cg *S, const sprs_bjacobi *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_cg_solve_z(sprs_cg *S, const sprs_bjacobi *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_cg_solve_s(sprs_cg *S, const sprs_bjacobi *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_cg_solve_c(sprs_cg *S, const sprs_bjacobi *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_cg_solve_dev_d(sprs_cg *S, const sprs_bjacobi *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_cg_solve_dev_z(sprs_cg *S, const sprs_bjacobi *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_cg_solve_dev_s(sprs_cg *S, const sprs_bjacobi *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_cg_solve_dev_c(sprs_cg *S, const sprs_bjacobi *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_gmres_solve_d(sprs_gmres *S, const sprs_bjacobi *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_gmres_solve_z(sprs_gmres *S, const sprs_bjacobi *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_gmres_solve_s(sprs_gmres *S, const sprs_bjacobi *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_gmres_solve_c(sprs_gmres *S, const sprs_bjacobi *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_gmres_solve_dev_d(sprs_gmres *S, const sprs_bjacobi *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_gmres_solve_dev_z(sprs_gmres *S, const sprs_bjacobi *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_gmres_solve_dev_s(sprs_gmres *S, const sprs_bjacobi *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_gmres_solve_dev_c(sprs_gmres *S, const sprs_bjacobi *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_bicgstab_solve_d(sprs_bicgstab *S, const sprs_bjacobi *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_bicgstab_solve_z(sprs_bicgstab *S, const sprs_bjacobi *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_bicgstab_solve_s(sprs_bicgstab *S, const sprs_bjacobi *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_bicgstab_solve_c(sprs_bicgstab *S, const sprs_bjacobi *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_bicgstab_solve_dev_d(sprs_bicgstab *S, const sprs_bjacobi *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_bicgstab_solve_dev_z(sprs_bicgstab *S, const sprs_bjacobi *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_bicgstab_solve_dev_s(sprs_bicgstab *S, const sprs_bjacobi *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_bicgstab_solve_dev_c(sprs_bicgstab *S, const sprs_bjacobi *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_minres_solve_d(sprs_minres *S, const sprs_bjacobi *P, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_minres_solve_z(sprs_minres *S, const sprs_bjacobi *P, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_minres_solve_s(sprs_minres *S, const sprs_bjacobi *P, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_minres_solve_c(sprs_minres *S, const sprs_bjacobi *P, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_minres_solve_dev_d(sprs_minres *S, const sprs_bjacobi *P, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_minres_solve_dev_z(sprs_minres *S, const sprs_bjacobi *P, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out);
int sprs_bjacobi_minres_solve_dev_s(sprs_minres *S, const sprs_bjacobi *P, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);
int sprs_bjacobi_minres_solve_dev_c(sprs_minres *S, const sprs_bjacobi *P, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out);

/* ---------------------------------------------------------------- multi-GPU (one process per GPU)
 * No reference analogue: the reference is single-process (rayon).  The matrix is row-partitioned;
 * rank r owns rows [r0, r1) and the matching slices of every vector.  A distributed operator is the
 * local row block with column indices renumbered into the rank's EXTENDED x vector
 * [ owned entries (n_local) | entries received from peer 0 | peer 1 | ... ]  (n_ext elements).
 * Every solver above accepts such an operator (create it with size = n_local): SpMV is preceded by
 * the halo exchange (RCCL send/recv with the owning peers over xGMI), every dot product / norm is
 * followed by an RCCL all-reduce, and rhs / x are the rank's slices.  sprsolve_amd/partition.py
 * derives the exchange plan from global column indices. */
int sprs_comm_unique_id(void *id128_out);  /* rank 0: 128-byte RCCL id to broadcast to the other ranks */
int sprs_comm_create(sprs_ctx *ctx, int world, int rank, const void *id128, sprs_comm **out); /* collective */
int sprs_comm_destroy(sprs_comm *comm);
/* 1 when the ranks of this communicator mapped each other's mailboxes at creation (same node, hipIpc): the distributed solvers'
 * scalar hand-offs then need no stream operation — the producing kernel's last workgroup posts its reduced values into every
 * rank's mailbox, the consumer kernels sum the entries in rank order (ctx knobs "p2p_allreduce", "p2p_timeout_ms"); 0: ncclAllReduce. */
int sprs_comm_p2p(const sprs_comm *comm, int *enabled_out);
int sprs_comm_count(const sprs_comm *comm, int *count_out); /* ncclCommCount: the number of ranks RCCL itself reports */
int sprs_comm_allreduce_sum_f64(sprs_comm *comm, double *dev, size_t count); /* in place; blocking */
/* mean time of `reps` back-to-back in-place all-reduces of `count` doubles on the context's stream (HIP events): the
 * price of one dot-product hand-off of a distributed solve on this communicator; collective */
int sprs_comm_allreduce_timed_f64(sprs_comm *comm, double *dev, size_t count, int reps, double *us_out);
/* peer_rank[n_peers]; send_off/recv_off[n_peers+1] are element offsets; send_idx_dev[send_off[n_peers]]
 * (device, i32) lists the local entries to pack for each peer; entries from peer p land at
 * x_ext[n_local + recv_off[p] ...].  recv_off[n_peers] == n_ext - n_local. */
int sprs_dist_csr_create_dev_d(sprs_comm *comm, int64_t n_local, int64_t n_ext, int64_t nnz,
                               const int32_t *dev_row_ptr, const int32_t *dev_col_idx_ext, const double *dev_val, int adopt,
                               int n_peers, const int32_t *peer_rank, const int64_t *send_off,
                               const int32_t *send_idx_dev, const int64_t *recv_off, sprs_csr **out);
int sprs_dist_csr_create_dev_z(sprs_comm *comm, int64_t n_local, int64_t n_ext, int64_t nnz,
                               const int32_t *dev_row_ptr, const int32_t *dev_col_idx_ext, const sprs_c64 *dev_val, int adopt,
                               int n_peers, const int32_t *peer_rank, const int64_t *send_off,
                               const int32_t *send_idx_dev, const int64_t *recv_off, sprs_csr **out);
/* north_star's literal exchange instead of the sparse halo: before every SpMV an ncclAllGather of all ranks'
 * x slices (each padded to `slice` >= max n_local elements, the same value on every rank).  Column indices
 * address the gathered vector: col = owner_rank * slice + (global_col - first_row_of_owner).  Moves
 * world*slice elements per SpMV (400 MB for cfg 5) — kept for comparison; the sparse halo is the default. */
/* The same operator from GLOBAL column indices — the exchange plan is derived inside the library (device passes +
 * one ncclAllGather of the per-peer counts + one ncclSend/ncclRecv group of the index lists), which is what a host
 * without numpy (the Rust binding) calls.  Collective over comm.  row_starts[world + 1] (host, identical on all ranks):
 * rank r owns rows / x entries [row_starts[r], row_starts[r+1]); dev_col_idx_global (device, i32[nnz]) holds global
 * column numbers and is renumbered IN PLACE into the rank's extended numbering when adopt != 0 (into a private copy
 * otherwise).  exchange: 0 = sparse halo (only the referenced remote entries travel, from the ranks that own them),
 * 1 = north_star's literal ncclAllGather of every rank's x slice.  Temporary device memory: 5 bytes per global column.
 * SPRS_INVALID_ARGUMENT when a column index is outside [0, row_starts[world]). */
int sprs_dist_csr_create_global_dev_d(sprs_comm *comm, const int64_t *row_starts, int64_t nnz, const int32_t *dev_row_ptr, int32_t *dev_col_idx_global, const double *dev_val, int adopt, int exchange, sprs_csr **out);
int sprs_dist_csr_create_global_dev_z(sprs_comm *comm, const int64_t *row_starts, int64_t nnz, const int32_t *dev_row_ptr, int32_t *dev_col_idx_global, const sprs_c64 *dev_val, int adopt, int exchange, sprs_csr **out);
int sprs_dist_csr_create_global_dev_s(sprs_comm *comm, const int64_t *row_starts, int64_t nnz, const int32_t *dev_row_ptr, int32_t *dev_col_idx_global, const float *dev_val, int adopt, int exchange, sprs_csr **out);
int sprs_dist_csr_create_global_dev_c(sprs_comm *comm, const int64_t *row_starts, int64_t nnz, const int32_t *dev_row_ptr, int32_t *dev_col_idx_global, const sprs_c32 *dev_val, int adopt, int exchange, sprs_csr **out);
/* The plan of a distributed operator, read back (tests, bench evidence): sizes; then peer ranks and element offsets
 * (arrays of cap >= n_peers and n_peers + 1 entries); then the local indices this rank packs, grouped by peer. */
int sprs_dist_csr_info(const sprs_csr *A, int64_t *n_local, int64_t *n_ext, int *n_peers, int64_t *send_entries, int64_t *recv_entries);
int sprs_dist_csr_peers(const sprs_csr *A, int cap, int32_t *peer_rank, int64_t *send_off, int64_t *recv_off);
int sprs_dist_csr_send_idx(const sprs_csr *A, int64_t cap, int32_t *send_idx_host);
int sprs_dist_csr_create_allgather_dev_d(sprs_comm *comm, int64_t n_local, int64_t slice, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx_gathered, const double *dev_val, int adopt, sprs_csr **out);
int sprs_dist_csr_create_allgather_dev_z(sprs_comm *comm, int64_t n_local, int64_t slice, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx_gathered, const sprs_c64 *dev_val, int adopt, sprs_csr **out);
int sprs_dist_csr_create_allgather_dev_s(sprs_comm *comm, int64_t n_local, int64_t slice, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx_gathered, const float *dev_val, int adopt, sprs_csr **out);
int sprs_dist_csr_create_allgather_dev_c(sprs_comm *comm, int64_t n_local, int64_t slice, int64_t nnz, const int32_t *dev_row_ptr, const int32_t *dev_col_idx_gathered, const sprs_c32 *dev_val, int adopt, sprs_csr **out);
/* y_local = A_local * x after exchanging the halo tail of x_ext (n_ext elements, owned slice first) */
int sprs_dist_mul_vec_dev_d(const sprs_csr *A, double *x_ext_dev, double *y_local_dev);
int sprs_dist_mul_vec_dev_z(const sprs_csr *A, sprs_c64 *x_ext_dev, sprs_c64 *y_local_dev);

/* ---------------------------------------------------------------- thick-restart Lanczos eigensolver
 * The k algebraically largest or smallest eigenpairs of a square A that is assumed Hermitian (as with CG, that is not checked):
 * thick-restart Lanczos (Wu & Simon; equal to Hermitian Krylov-Schur) with full reorthogonalisation by classical Gram-Schmidt
 * applied twice.  The reference has no such solver.  Single GPU: a distributed A is refused with SPRS_INVALID_ARGUMENT (text in
 * sprs_last_error).  The handle owns ncv + 2 vectors: v_0 .. v_m (m = ncv) and w.
 * Vectors and the CGS2 coefficients h_i, c_i are of type T.  T_ij, theta_i, S, beta, res_i, anorm, scale are double for all four
 * scalar types: the projected matrix is real symmetric for complex A too (its diagonal holds Re(conj_dot(v_j, A v_j)), its
 * sub-diagonal norms, and after a restart Ritz values and real multiples of a real eigenvector matrix).  beta is the square root,
 * taken in T::Real, of a sum of squares formed in T::Real.  conj_dot(a, b) = sum conj(a_i) b_i.
 *     beta0 = norm2(v0);  NaN or 0: SPRS_BREAKDOWN (*matvecs_out = 0, *restarts_out = 0).  v_0 = v0 * (1 / beta0)
 *     T = 0, j0 = 0, anorm = 0, scale = 0
 *     cycle c = 1, 2, ...:
 *         for j = j0 .. m - 1:
 *             w = A v_j
 *             pass 1:  h_i = conj_dot(v_i, w) for i = 0 .. j, all on the same w;  then for i = 0 .. j in order: w += v_i*(-h_i)
 *             pass 2:  c_i = conj_dot(v_i, w) for i = 0 .. j, all on the same w;  then for i = 0 .. j in order: w += v_i*(-c_i);
 *                      h_i = h_i + c_i
 *             T_jj = Re(h_j);  beta = norm2(w);  NaN: SPRS_BREAKDOWN
 *             scale = max(scale, |T_jj|)
 *             if beta <= 64 eps(T::Real) scale: an invariant subspace, m_eff = j + 1, leave the loop (v_{j+1} is not formed)
 *             scale = max(scale, beta);  if j + 1 < m: T_{j+1,j} = T_{j,j+1} = beta;   v_{j+1} = w * (1 / beta)   (also at j = m - 1)
 *         (m_eff = m where the loop ran out)
 *         (theta, S) = the eigendecomposition of T[:m_eff, :m_eff] (below), theta descending (SPRS_EIGSH_LARGEST) or ascending
 *                      (SPRS_EIGSH_SMALLEST), ties by index, the columns of S with it
 *         res_i = beta |S[m_eff - 1, i]|;  anorm = max(anorm, max |theta_i|);  nconv = the number of LEADING i < k with
 *                      res_i <= tol anorm
 *         invariant subspace:  m_eff >= k: SPRS_OK with nconv = k;  else SPRS_BREAKDOWN
 *         nconv == k:          SPRS_OK
 *         c == max_restarts:   SPRS_INSUFFICIENT_ITER (the outputs are the current leading k pairs, nconv as counted)
 *         restart:  p = min(k + max(k, 4), m - 2);  V[:, :p] = V[:, :m] S[:, :p];  v_p = v_m;
 *                   T = diag(theta_0 .. theta_{p-1}),  T_{p,i} = T_{i,p} = beta S[m - 1, i] (i < p);  j0 = p
 *     outputs:  vals_i = theta_i and res_i (absolute) for i < k, rounded to T::Real;  X = V[:, :m_eff] S[:, :k] as k contiguous
 *               vectors of n (vecs may be NULL);  nconv;  restarts = c;  matvecs = the products A v that ran
 * Only T's diagonal, sub-diagonal and the restart's arrow row are kept from a step; the other CGS2 coefficients serve the
 * reorthogonalisation alone.  The coefficients of V S are S rounded once to T::Real, and every output element is summed over
 * i ascending from zero, one real-by-T product and one sum per term, each rounded once.  Eigenvector phases are whatever falls
 * out.  On SPRS_BREAKDOWN vals / res hold the last Ritz values computed (zeros where there were none) and vecs is not written.
 * The eigendecomposition: cyclic Jacobi on T with S = I.  m_eff is rounded up to an even M (an odd m_eff carries one idle
 * index).  A sweep is M - 1 rounds; round r rotates the M / 2 disjoint pairs (M - 1, r) and ((r + i) mod (M - 1),
 * (r - i) mod (M - 1)), i = 1 .. M / 2 - 1, each ordered p < q, all from the same T:  T_pq == 0: nothing;  else
 * tau = (T_qq - T_pp) / (2 T_pq), t = sign(tau) / (|tau| + sqrt(1 + tau^2)) (sign(0) = 1), c = 1 / sqrt(1 + t^2), s = t c;
 * columns: x_p' = c x_p - s x_q, x_q' = s x_p + c x_q on T and S, then the same on T's rows, then T_pq = T_qp = 0 exactly.
 * Before every sweep off(T)^2 = the sum of the squared off-diagonal entries is compared with eps^2 |T|_F^2 (|T|_F of the
 * input): at or below it the diagonal holds theta; after 30 sweeps above it the solve ends in SPRS_BREAKDOWN, never a silent
 * result.
 * create:  ncv = 0 means min(32, n);  SPRS_INVALID_ARGUMENT unless 3 <= ncv <= min(SPRS_EIGSH_MAX_NCV, n);  SPRS_NOT_SQUARE;
 *          SPRS_DIM_MISMATCH for size != rows.
 * solve:   SPRS_INVALID_ARGUMENT unless 1 <= k <= ncv - 2, which is one of the two and max_restarts >= 1;
 *          SPRS_INCOMPATIBLE_RHS_SIZE for v0_len != n;  SPRS_INCOMPATIBLE_X_SIZE for a non-null vecs with vecs_len != k n.
 *          vals_out and res_out hold k entries; the three counters may be NULL.
 * Not provided for this solver: a literal mode, the trace, the profile hooks and a sprs_solver_* kind.
 * Limits: a single start vector finds one copy of a multiple eigenvalue; convergence is governed by the relative gap, so the
 * smallest modes of a large Laplacian take thousands of products; a start vector inside an invariant subspace yields that
 * subspace's extreme pairs, not A's. */
typedef struct sprs_eigsh sprs_eigsh;
#define SPRS_EIGSH_MAX_NCV 64
enum { SPRS_EIGSH_LARGEST = 0, SPRS_EIGSH_SMALLEST = 1 };
int sprs_eigsh_destroy(sprs_eigsh *S);         /* NULL is a no-op */
int sprs_eigsh_create_d(const sprs_csr *A, size_t size, size_t ncv, sprs_eigsh **out);
int sprs_eigsh_create_z(const sprs_csr *A, size_t size, size_t ncv, sprs_eigsh **out);
int sprs_eigsh_create_s(const sprs_csr *A, size_t size, size_t ncv, sprs_eigsh **out);
int sprs_eigsh_create_c(const sprs_csr *A, size_t size, size_t ncv, sprs_eigsh **out);
int sprs_eigsh_solve_d(sprs_eigsh *S, size_t k, int which, const double *v0, size_t v0_len, size_t max_restarts, double tol, double *vals_out, double *vecs_out_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_eigsh_solve_z(sprs_eigsh *S, size_t k, int which, const sprs_c64 *v0, size_t v0_len, size_t max_restarts, double tol, double *vals_out, sprs_c64 *vecs_out_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_eigsh_solve_s(sprs_eigsh *S, size_t k, int which, const float *v0, size_t v0_len, size_t max_restarts, float tol, float *vals_out, float *vecs_out_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_eigsh_solve_c(sprs_eigsh *S, size_t k, int which, const sprs_c32 *v0, size_t v0_len, size_t max_restarts, float tol, float *vals_out, sprs_c32 *vecs_out_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
/* the same with v0 and vecs on the device (any alignment); vals, res and the counters stay on the host */
int sprs_eigsh_solve_dev_d(sprs_eigsh *S, size_t k, int which, const double *v0_dev, size_t v0_len, size_t max_restarts, double tol, double *vals_out, double *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_eigsh_solve_dev_z(sprs_eigsh *S, size_t k, int which, const sprs_c64 *v0_dev, size_t v0_len, size_t max_restarts, double tol, double *vals_out, sprs_c64 *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_eigsh_solve_dev_s(sprs_eigsh *S, size_t k, int which, const float *v0_dev, size_t v0_len, size_t max_restarts, float tol, float *vals_out, float *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_eigsh_solve_dev_c(sprs_eigsh *S, size_t k, int which, const sprs_c32 *v0_dev, size_t v0_len, size_t max_restarts, float tol, float *vals_out, sprs_c32 *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);

/* ---------------------------------------------------------------- preconditioned block eigensolver (LOBPCG)
 * The k algebraically smallest or largest eigenpairs of a square A that is assumed Hermitian (not checked), by locally optimal
 * block preconditioned conjugate gradients (Knyazev) on a block of b vectors, 1 <= b <= SPRS_LOBPCG_MAX_BLOCK and 6 b <= n, with
 * a Rayleigh-Ritz step on [X, P, W] per iteration.  The preconditioner M (Hermitian positive definite, about A^-1 for the
 * smallest pairs) is nothing, a sprs_diag, or an ILU(0), AMG or FSAI handle.  The reference has no such solver.  Single GPU: a
 * distributed A is refused with SPRS_INVALID_ARGUMENT (text in sprs_last_error).  The handle owns 6 b contiguous vectors:
 * X, P, W, AX, AP, AW.  A solve wants the first k <= b pairs in the order of `which` (SPRS_EIGSH_LARGEST / _SMALLEST); the other
 * b - k columns are guard vectors.
 * Vectors, the Gram sums and the coefficients C are of type T; G, K, L, K^, Z, theta, s, res, anorm are double (complex double
 * for complex T) for all four scalar types.  conj_dot(a, b) = sum conj(a_i) b_i.
 *   start:  X = X0 (b vectors);  AX_c = A X_c;  one Rayleigh-Ritz step (below) on S = [X], AS = [AX], m = b:
 *           X = S C, AX = AS C, theta = its b Ritz values;  P = AP = 0
 *   iteration it = 1, 2, ...:
 *     1. r_c = AX_c - theta_c X_c for c < b, theta_c rounded once to T::Real;  res_c = norm2(r_c), the square root taken in
 *        T::Real of a sum of squares formed in T::Real;  a NaN: SPRS_BREAKDOWN
 *     2. column c < b is LOCKED in this iteration when res_c <= tol anorm (anorm: step 5 (8));  nconv = the number of LEADING
 *        c < k that are locked.  nconv == k: SPRS_OK with iters = it - 1.
 *        it > max_iter: SPRS_INSUFFICIENT_ITER with iters = max_iter (the outputs are the current leading k pairs)
 *     3. W_c = M r_c (W_c = r_c without a preconditioner; a diagonal M inside the residual kernel, an applied one in place)
 *     4. AW_c = A W_c
 *     5. Rayleigh-Ritz on S = [X, P, W], AS = [AX, AP, AW];  at it = 1: S = [X, W].  Soft locking: the P_c and W_c of the columns
 *        locked in step 2 are left out of the projected problem (their rows of C are zero; the lock is taken again from the
 *        residuals of every iteration, so a column whose residual grows comes back), m = b + 2 (b - locked), b + (b - locked)
 *        without P.  A converged column's W_c is rounding noise and its P_c the difference of two such: kept in the basis they
 *        make G singular to working precision, and a G that still passes rule (3) then yields Ritz values far outside A's
 *        spectrum
 *        (1) G = S^H S, K = S^H AS from their upper triangles (G_ij = conj_dot(S_i, S_j), K_ij = conj_dot(S_i, AS_j), i <= j,
 *            summed in T), the lower triangles their conjugates, the diagonals real
 *        (2) s_i = G_ii^(-1/2);  G^ = diag(s) G diag(s).  A G_ii that is not a positive finite number: failure
 *        (3) Cholesky G^ = L L^H, column by column.  Failure when a pivot G^_jj - sum_q |L_jq|^2 (= L_jj^2) is not greater than
 *            64 m eps(T::Real)
 *        (4) failure with P in the basis: steps (2) - (8) once more on the [X, W] sub-blocks of G and K, the P rows of C zero,
 *            restarts += 1.  Failure without P: SPRS_BREAKDOWN
 *        (5) K^ = L^-1 diag(s) K diag(s) L^-H, taken Hermitian from its upper triangle with a real diagonal
 *        (6) K^ = Z Theta Z^H by cyclic Jacobi: the order and stopping rule of sprs_eigsh_* (round-robin pairs on m rounded up
 *            to even, off^2 <= eps^2 |K^|_F^2 before every sweep, 30 sweeps, then SPRS_BREAKDOWN).  With u = K^_pq / |K^_pq|,
 *            tau = (K^_qq - K^_pp) / (2 |K^_pq|), t, c, s as there and sc = s u:  columns x_p' = c x_p - conj(sc) x_q,
 *            x_q' = sc x_p + c x_q on K^ and Z;  rows row_p' = c row_p - sc row_q, row_q' = conj(sc) row_p + c row_q on K^;
 *            then K^_pq = K^_qp = 0 and Im K^_pp = Im K^_qq = 0 exactly
 *        (7) Theta ascending (SMALLEST) or descending (LARGEST), ties by index, the columns of Z with it
 *        (8) C = diag(s) L^-H Z;  anorm = max(anorm, max_i |K_ii| / G_ii) over the X and W columns i of the problem solved:
 *            Rayleigh quotients of vectors whose products with A are held, so anorm <= |A|_2 up to the rounding of the Gram
 *            sums whatever the projected problem returns (a Ritz value of an ill-conditioned basis has no such bound)
 *     6. C_X = the first b columns of C, C_P = C_X with its X rows zero, both rounded once to T:
 *        X = S C_X, P = S C_P, AX = AS C_X, AP = AS C_P (every element summed over the rows of C ascending from zero, one product
 *        and one sum per term, each rounded once);  theta = the first b entries of Theta
 * A NaN anywhere ends the solve with SPRS_BREAKDOWN, and so does a zero column of X0 (G_ii = 0 at the start) or a start block of
 * deficient rank (the Cholesky rule).  matvecs = b (iters + 1) on SPRS_OK and SPRS_INSUFFICIENT_ITER.
 * outputs:  vals_i = theta_i and res_i (absolute) for i < k, rounded to T::Real;  X_0 .. X_{k-1} as k contiguous vectors of n
 *           (vecs may be NULL);  nconv, iters, restarts (the [X, W] fallbacks), matvecs.  On SPRS_BREAKDOWN vecs is not written.
 * create:   block = 0 means min(8, n / 6);  SPRS_INVALID_ARGUMENT (text in sprs_last_error) for block > 8, 6 block > n, a
 *           distributed A or another scalar type;  SPRS_NOT_SQUARE;  SPRS_DIM_MISMATCH for size != rows.
 * solve:    SPRS_INVALID_ARGUMENT unless 1 <= k <= block, which is one of the two and max_iter >= 1;  X0 NULL selects the default
 *           block (column c: U[-1, 1) from the library's splitmix64 streams 100 + 2 c, the imaginary parts 101 + 2 c), else
 *           SPRS_INCOMPATIBLE_RHS_SIZE for x0_len != block n;  SPRS_INCOMPATIBLE_X_SIZE for a non-null vecs with
 *           vecs_len != k n.  vals_out and res_out hold k entries; the four counters may be NULL.  A sprs_diag of another size:
 *           SPRS_DIM_MISMATCH, of another scalar type: SPRS_INVALID_ARGUMENT.
 * Not provided for this solver: a literal mode, the trace, the profile hooks and a sprs_solver_* kind.
 * Limits: soft locking is in the projected problem only, locked columns still cost their share of every pass; with k = block
 * (no guard vectors) convergence can take ten times the iterations, so choose block > k; the block is at most 8 wide; the host
 * does not wait inside an iteration, so up to `poll` iterations' launches run as no-ops after the event. */
typedef struct sprs_lobpcg sprs_lobpcg;
#define SPRS_LOBPCG_MAX_BLOCK 8
int sprs_lobpcg_destroy(sprs_lobpcg *S);       /* NULL is a no-op */
int sprs_lobpcg_create_d(const sprs_csr *A, size_t size, size_t block, sprs_lobpcg **out);
int sprs_lobpcg_create_z(const sprs_csr *A, size_t size, size_t block, sprs_lobpcg **out);
int sprs_lobpcg_create_s(const sprs_csr *A, size_t size, size_t block, sprs_lobpcg **out);
int sprs_lobpcg_create_c(const sprs_csr *A, size_t size, size_t block, sprs_lobpcg **out);
int sprs_lobpcg_solve_d(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const double *X0_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, double *vecs_out_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_lobpcg_solve_z(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const sprs_c64 *X0_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, sprs_c64 *vecs_out_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_lobpcg_solve_s(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const float *X0_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, float *vecs_out_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_lobpcg_solve_c(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const sprs_c32 *X0_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, sprs_c32 *vecs_out_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
/* the same with X0 and vecs on the device (any alignment); vals, res and the counters stay on the host */
int sprs_lobpcg_solve_dev_d(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const double *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, double *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_lobpcg_solve_dev_z(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const sprs_c64 *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, sprs_c64 *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_lobpcg_solve_dev_s(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const float *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, float *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_lobpcg_solve_dev_c(sprs_lobpcg *S, const sprs_diag *P_or_null, size_t k, int which, const sprs_c32 *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, sprs_c32 *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
/* ... preconditioned by an ILU(0), AMG or FSAI handle, checked as the Krylov solvers check it: SPRS_INVALID_ARGUMENT for a null handle,
 * another scalar type or context, SPRS_DIM_MISMATCH for another size */
int sprs_ilu0_lobpcg_solve_dev_d(sprs_lobpcg *S, const sprs_ilu0 *P, size_t k, int which, const double *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, double *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_ilu0_lobpcg_solve_dev_z(sprs_lobpcg *S, const sprs_ilu0 *P, size_t k, int which, const sprs_c64 *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, sprs_c64 *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_ilu0_lobpcg_solve_dev_s(sprs_lobpcg *S, const sprs_ilu0 *P, size_t k, int which, const float *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, float *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_ilu0_lobpcg_solve_dev_c(sprs_lobpcg *S, const sprs_ilu0 *P, size_t k, int which, const sprs_c32 *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, sprs_c32 *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_amg_lobpcg_solve_dev_d(sprs_lobpcg *S, const sprs_amg *P, size_t k, int which, const double *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, double *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_amg_lobpcg_solve_dev_z(sprs_lobpcg *S, const sprs_amg *P, size_t k, int which, const sprs_c64 *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, sprs_c64 *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_amg_lobpcg_solve_dev_s(sprs_lobpcg *S, const sprs_amg *P, size_t k, int which, const float *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, float *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_amg_lobpcg_solve_dev_c(sprs_lobpcg *S, const sprs_amg *P, size_t k, int which, const sprs_c32 *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, sprs_c32 *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_fsai_lobpcg_solve_dev_d(sprs_lobpcg *S, const sprs_fsai *P, size_t k, int which, const double *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, double *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_fsai_lobpcg_solve_dev_z(sprs_lobpcg *S, const sprs_fsai *P, size_t k, int which, const sprs_c64 *X0_dev_or_null, size_t x0_len, size_t max_iter, double tol, double *vals_out, sprs_c64 *vecs_dev_or_null, size_t vecs_len, double *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_fsai_lobpcg_solve_dev_s(sprs_lobpcg *S, const sprs_fsai *P, size_t k, int which, const float *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, float *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_fsai_lobpcg_solve_dev_c(sprs_lobpcg *S, const sprs_fsai *P, size_t k, int which, const sprs_c32 *X0_dev_or_null, size_t x0_len, size_t max_iter, float tol, float *vals_out, sprs_c32 *vecs_dev_or_null, size_t vecs_len, float *res_out, size_t *nconv_out, size_t *iters_out, size_t *restarts_out, size_t *matvecs_out);

/* ---------------------------------------------------------------- truncated SVD (thick-restart Lanczos bidiagonalisation)
 * The k largest or smallest singular triplets A v_i = sigma_i u_i, A^H u_i = sigma_i v_i (nothing conjugated) of an r x c matrix A
 * of any shape: Golub-Kahan-Lanczos bidiagonalisation with a thick restart on plain Ritz vectors and full reorthogonalisation
 * of both bases by classical Gram-Schmidt applied twice.  The reference has no such solver.  Single GPU: a distributed A is
 * refused with SPRS_INVALID_ARGUMENT (text in sprs_last_error).  The handle borrows a handle of A^H (sprs_csr_adjoint with
 * conjugate = 1) or builds and owns one.
 * Op = A and OpH = A^H where r >= c; otherwise Op = A^H and OpH = A, and U and V change places on output.  So Op is M x N with
 * M >= N, and the start vector v0 lives in the small space: N = min(r, c) entries (a start vector in the large space would carry
 * a null-space component into B).  The handle owns 2 l + 3 vectors, l = ncv: p_0 .. p_l and w' of N entries, q_0 .. q_{l-1} and
 * w of M entries.
 * Vectors and the CGS2 coefficients are of type T.  B (l x l, upper triangular), sigma_i, X, Y, alpha, beta, res_i, anorm, scale
 * are double for all four scalar types: the projected matrix is real for complex A too (its diagonal and super-diagonal hold
 * norms, and after a restart singular values and real multiples of a real singular-vector matrix).  alpha and beta are square
 * roots, taken in T::Real, of sums of squares formed in T::Real.  conj_dot(a, b) = sum conj(a_i) b_i.
 *     beta0 = norm2(v0);  NaN or 0: SPRS_BREAKDOWN (*matvecs_out = 0, *restarts_out = 0).  p_0 = v0 * (1 / beta0)
 *     B = 0, j0 = 0, anorm = 0, scale = 0
 *     cycle c = 1, 2, ...:
 *         for j = j0 .. l - 1:
 *             w = Op p_j
 *             j > 0:   pass 1:  h_i = conj_dot(q_i, w) for i = 0 .. j - 1, all on the same w;  then for i in order: w += q_i*(-h_i)
 *                      pass 2:  the same once more on the updated w
 *             alpha = norm2(w);  NaN: SPRS_BREAKDOWN;  alpha <= 64 eps(T::Real) scale: Op is numerically rank-deficient along the
 *                      basis, SPRS_BREAKDOWN (a limit, not worked round)
 *             B_jj = alpha;  scale = max(scale, alpha);  q_j = w * (1 / alpha)
 *             w' = OpH q_j
 *             pass 1, pass 2:  the same against p_0 .. p_j
 *             beta = norm2(w');  NaN: SPRS_BREAKDOWN
 *             if beta <= 64 eps(T::Real) scale: an invariant subspace, m_eff = j + 1, beta = 0 (the residuals are zero), leave
 *                      the loop (p_{j+1} is not formed)
 *             scale = max(scale, beta);  if j + 1 < l: B_{j,j+1} = beta;   p_{j+1} = w' * (1 / beta)   (also at j = l - 1)
 *         (m_eff = l where the loop ran out)
 *         B[:m_eff, :m_eff] = X Sigma Y^T (below), sigma descending (SPRS_SVDS_LARGEST) or ascending (SPRS_SVDS_SMALLEST), ties
 *                      by index, the columns of X and Y with it
 *         res_i = beta |X[m_eff - 1, i]|;  anorm = max(anorm, max sigma_i);  nconv = the number of LEADING i < k with
 *                      res_i <= tol anorm
 *         invariant subspace:  m_eff >= k: SPRS_OK with nconv = k;  else SPRS_BREAKDOWN
 *         nconv == k:          SPRS_OK
 *         c == max_restarts:   SPRS_INSUFFICIENT_ITER (the outputs are the current leading k triplets, nconv as counted)
 *         restart:  p = min(k + max(k, 4), l - 2);  P[:, :p] = P[:, :l] Y[:, :p];  Q[:, :p] = Q[:, :l] X[:, :p];  p_p = p_l;
 *                   B = diag(sigma_0 .. sigma_{p-1}) with the spike column B_{i,p} = beta X[l - 1, i] (i < p), zero elsewhere;
 *                   j0 = p  (the next step's first Gram-Schmidt, against q_0 .. q_{p-1}, removes the spike by itself)
 *     outputs:  vals_i = sigma_i and res_i (absolute) for i < k, rounded to T::Real;  V = P[:, :m_eff] Y[:, :k] and
 *               U = Q[:, :m_eff] X[:, :k] (the other way round where Op = A^H) as k contiguous vectors of c and of r entries (both
 *               pointers or neither);  nconv;  restarts = c;  matvecs = the products with either operator that ran: without an
 *               invariant subspace 2 l + 2 (l - p)(restarts - 1)
 * Only alpha and beta are kept from a step; the other entries of B are known from its structure and the CGS2 coefficients serve
 * the reorthogonalisation alone.  The coefficients of P Y and Q X are Y and X rounded once to T::Real, and every output element
 * is summed over i ascending from zero, one real-by-T product and one sum per term, each rounded once.  Phases and signs of the
 * singular vectors are whatever falls out.  On SPRS_BREAKDOWN vals / res hold the last values computed (zeros where there were
 * none) and the vectors are not written.
 * The projected SVD: one-sided (Hestenes) Jacobi on the columns of G = B with Y = I, in double; the Gram matrix B^T B is never
 * formed, so sigma and X keep relative accuracy for the small singular values.  m_eff is rounded up to an even M (an odd m_eff
 * carries one zero column, which never rotates).  A sweep is M - 1 rounds; round r takes the M / 2 disjoint pairs (M - 1, r) and
 * ((r + i) mod (M - 1), (r - i) mod (M - 1)), i = 1 .. M / 2 - 1, each ordered p < q, all from the same G:
 * a = |g_p|^2, b = |g_q|^2, c = g_p.g_q;  |c| <= eps sqrt(a b): nothing;  else zeta = (b - a) / (2 c),
 * t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (sign(0) = 1), cs = 1 / sqrt(1 + t^2), sn = cs t;
 * g_p' = cs g_p - sn g_q, g_q' = sn g_p + cs g_q, and the same on Y.  A sweep without a rotation ends the iteration; 30 sweeps
 * with one end the solve in SPRS_BREAKDOWN, never a silent result.  Then sigma_i = |g_i| (zero or NaN: SPRS_BREAKDOWN) and
 * x_i = g_i / sigma_i.
 * create:  ncv = 0 means min(32, min(r, c));  SPRS_INVALID_ARGUMENT (text in sprs_last_error) unless
 *          3 <= ncv <= min(SPRS_SVDS_MAX_NCV, min(r, c)), for a distributed A and for an AH of another shape, scalar type or context.
 * solve:   SPRS_INVALID_ARGUMENT unless 1 <= k <= ncv - 2, which is one of the two, max_restarts >= 1 and u_out, v_out are both
 *          given or both NULL;  SPRS_INCOMPATIBLE_RHS_SIZE for v0_len != min(r, c);  SPRS_INCOMPATIBLE_X_SIZE for u_len != k r or
 *          v_len != k c where the vectors are given.  vals_out and res_out hold k entries; the three counters may be NULL.
 *          SPRS_INSUFFICIENT_ITER fills everything, SPRS_BREAKDOWN everything but the vectors.
 * Not provided for this solver: a literal mode, the trace, the profile hooks, a sprs_solver_* kind and a Rust binding.
 * Limits: plain Ritz extraction at a restart (no harmonic or refined vectors), so the smallest triplets of an ill-conditioned A
 * converge slowly or not at all within max_restarts; both bases are fully reorthogonalised; a single start vector finds one copy
 * of a multiple singular value; a numerically rank-deficient operator ends in SPRS_BREAKDOWN; the projected SVD runs in one
 * workgroup. */
typedef struct sprs_svds sprs_svds;
#define SPRS_SVDS_MAX_NCV 64
enum { SPRS_SVDS_LARGEST = 0, SPRS_SVDS_SMALLEST = 1 };
int sprs_svds_destroy(sprs_svds *S);           /* NULL is a no-op */
int sprs_svds_create_d(const sprs_csr *A, const sprs_csr *AH_or_null, size_t ncv, sprs_svds **out);
int sprs_svds_create_z(const sprs_csr *A, const sprs_csr *AH_or_null, size_t ncv, sprs_svds **out);
int sprs_svds_create_s(const sprs_csr *A, const sprs_csr *AH_or_null, size_t ncv, sprs_svds **out);
int sprs_svds_create_c(const sprs_csr *A, const sprs_csr *AH_or_null, size_t ncv, sprs_svds **out);
int sprs_svds_solve_d(sprs_svds *S, size_t k, int which, const double *v0, size_t v0_len, size_t max_restarts, double tol, double *vals_out, double *u_out_or_null, size_t u_len, double *v_out_or_null, size_t v_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_svds_solve_z(sprs_svds *S, size_t k, int which, const sprs_c64 *v0, size_t v0_len, size_t max_restarts, double tol, double *vals_out, sprs_c64 *u_out_or_null, size_t u_len, sprs_c64 *v_out_or_null, size_t v_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_svds_solve_s(sprs_svds *S, size_t k, int which, const float *v0, size_t v0_len, size_t max_restarts, float tol, float *vals_out, float *u_out_or_null, size_t u_len, float *v_out_or_null, size_t v_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_svds_solve_c(sprs_svds *S, size_t k, int which, const sprs_c32 *v0, size_t v0_len, size_t max_restarts, float tol, float *vals_out, sprs_c32 *u_out_or_null, size_t u_len, sprs_c32 *v_out_or_null, size_t v_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
/* the same with v0, u and v on the device (any alignment); vals, res and the counters stay on the host */
int sprs_svds_solve_dev_d(sprs_svds *S, size_t k, int which, const double *v0_dev, size_t v0_len, size_t max_restarts, double tol, double *vals_out, double *u_dev_or_null, size_t u_len, double *v_dev_or_null, size_t v_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_svds_solve_dev_z(sprs_svds *S, size_t k, int which, const sprs_c64 *v0_dev, size_t v0_len, size_t max_restarts, double tol, double *vals_out, sprs_c64 *u_dev_or_null, size_t u_len, sprs_c64 *v_dev_or_null, size_t v_len, double *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_svds_solve_dev_s(sprs_svds *S, size_t k, int which, const float *v0_dev, size_t v0_len, size_t max_restarts, float tol, float *vals_out, float *u_dev_or_null, size_t u_len, float *v_dev_or_null, size_t v_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);
int sprs_svds_solve_dev_c(sprs_svds *S, size_t k, int which, const sprs_c32 *v0_dev, size_t v0_len, size_t max_restarts, float tol, float *vals_out, sprs_c32 *u_dev_or_null, size_t u_len, sprs_c32 *v_dev_or_null, size_t v_len, float *res_out, size_t *nconv_out, size_t *restarts_out, size_t *matvecs_out);

/* ---------------------------------------------------------------- matrix exponential propagator
 * w = exp(tA) v for a square A of any kind (non-symmetric, complex) and a finite real t of T::Real, negative or zero included:
 * Arnoldi projection on a Krylov space of m = ncv vectors with the error-controlled sub-stepping of Expokit's expv (Sidje, ACM
 * TOMS 24, 1998), full orthogonalisation by classical Gram-Schmidt applied twice.  The reference has no such operation.  Single
 * GPU: a distributed A is refused with SPRS_INVALID_ARGUMENT (text in sprs_last_error).  The handle owns ncv + 3 vectors:
 * v_0 .. v_m, p and one that stages the result.
 * Vectors and the CGS2 coefficients h_i, c_i are of type T.  The projected matrix H, F, every tau, the error estimates and beta
 * as used in the control are double for real T and complex double / double for complex T (the rule of sprs_eigsh_*).  beta, hn
 * and avnorm are square roots, taken in T::Real, of sums of squares formed in T::Real.  conj_dot(a, b) = sum conj(a_i) b_i.
 *     tol == 0 means sqrt(eps(T::Real));  sgn = sign(t), t_out = |t|, t_now = 0, w = v, tau = tau0 (0: not set yet)
 *     gamma = 0.9, delta = 1.2, at most 10 attempts per sub-step
 *     t_out == 0:  w = v bit for bit, SPRS_OK, all counters 0
 *     sub-step s = 1, 2, ...:
 *         beta = norm2(w);  NaN: SPRS_BREAKDOWN;  0: w = 0, SPRS_OK
 *         hump = max(hump, beta);  v_0 = w * (1 / beta);  H = 0 ((m+2) x (m+2));  scale = 0
 *         for j = 0 .. m - 1:
 *             p = A v_j
 *             pass 1:  h_i = conj_dot(v_i, p) for i = 0 .. j, all on the same p;  then for i = 0 .. j in order: p += v_i*(-h_i)
 *             pass 2:  c_i = conj_dot(v_i, p) for i = 0 .. j, all on the same p;  then for i = 0 .. j in order: p += v_i*(-c_i);
 *                      h_i = h_i + c_i                                     (exactly the passes of sprs_eigsh_*)
 *             H[i, j] = h_i for i <= j;  hn = norm2(p);  NaN: SPRS_BREAKDOWN;  scale = max(scale, max_i |h_i|)
 *             if hn <= 64 eps(T::Real) scale: a happy breakdown, m_eff = j + 1, leave the loop (v_{j+1} is not formed)
 *             scale = max(scale, hn);  H[j+1, j] = hn;  v_{j+1} = p * (1 / hn)          (also at j = m - 1)
 *         rem = t_out - t_now
 *         happy:  tau_s = rem;  F = smallexp(sgn tau_s H[:m_eff, :m_eff]);  c_i = beta F[i, 0] for i < m_eff;  err = 0
 *         else:   avnorm = norm2(A v_m)  (one more product, counted);  H[m+1, m] = 1
 *                 tau not set:  anorm = the largest row sum of |H[:m+1, :m]|;  fact = ((m+1)/e)^(m+1) sqrt(2 pi (m+1));
 *                               tau = round2((1/anorm) ((fact tol) / (4 beta anorm))^(1/m))
 *                 tau_s = tau if tau < rem, else rem
 *                 attempt a = 1, 2, ...:
 *                     F = smallexp(sgn tau_s H)   (all m + 2 rows);  e1 = beta |F[m, 0]|;  e2 = beta |F[m+1, 0]| avnorm
 *                     e1 > 10 e2: err = e2, xm = 1/m;   else e1 > e2: err = e1 e2 / (e1 - e2), xm = 1/m;   else err = e1, xm = 1/(m-1)
 *                     a NaN err: SPRS_BREAKDOWN;  err <= delta tau_s tol: accept, leave the loop
 *                     a == 10 (the tenth rejection of this sub-step): SPRS_BREAKDOWN
 *                     tau_s = round2(gamma tau_s (tau_s tol / err)^xm);  not finite or not > 0: SPRS_BREAKDOWN;  rejects += 1
 *                 c_i = beta F[i, 0] for i <= m;   tau = round2(gamma tau_s (tau_s tol / max(err, DBL_MIN))^xm)
 *         w = sum_i v_i c_i   (c rounded once to T, from zero, i ascending, one product and one sum per term, each rounded once)
 *         t_now = t_out where tau_s == rem, else t_now + tau_s;  err_sum += err;  steps += 1
 *         t_now >= t_out: SPRS_OK;   steps == max_steps: SPRS_INSUFFICIENT_ITER  (w is the state at t_done = sgn t_now)
 *     outputs:  w;  err = err_sum, hump and t_done rounded to T::Real;  steps;  rejects;  matvecs = the products A v that ran
 * round2(x) rounds a finite x > 0 to two significant decimal digits as Expokit does, and returns anything else as it is:
 * y = x, u = 0;  while y >= 100: y = y / 10, u += 1;  while y < 10: y = y * 10, u -= 1  (330 steps each at the most);
 * r = floor(y + 0.55);  then r = r * 10, u times, or r = r / 10, -u times.
 * smallexp(X) for an M x M matrix X, M <= m + 2, is its exponential by Taylor scaling and squaring:  nrm = the largest column sum
 * of |X|, not finite: SPRS_BREAKDOWN;  s = the least integer >= 0 with nrm 2^-s <= 1/2, s > 64: SPRS_BREAKDOWN;  Y = X 2^-s
 * (exact);  E = I, then for q = 18, 17, .., 1: E = I + (Y E) / q;  then s times E = E E.  Every entry of a product is summed over
 * the inner index ascending from zero, one product and one sum per term, by one thread, without atomics: the result does not
 * depend on timing.  |z| of a complex entry is hypot(re, im).
 * Where this departs from Expokit: anorm comes from the first projected matrix, not from the caller; Taylor scaling and squaring
 * of degree 18 stands in for the Pade approximant (three small matrices and no linear solve: it fits one workgroup's local
 * memory); t_now is set to t_out by the sub-step that takes all that remains, so that a rounding of t_now + tau_s cannot ask
 * for one more; a step size that is no longer a positive finite number ends the solve.  As in Expokit beta and the estimates
 * are absolute: the sum of the accepted estimates is at most delta |t| tol.
 * create:  ncv = 0 means min(30, n);  SPRS_INVALID_ARGUMENT unless 3 <= ncv <= min(SPRS_EXPM_MAX_NCV, n);  SPRS_NOT_SQUARE;
 *          SPRS_DIM_MISMATCH for size != rows.
 * apply:   SPRS_INVALID_ARGUMENT unless t, tol >= 0 and tau0 >= 0 are finite and max_steps >= 1;  SPRS_INCOMPATIBLE_RHS_SIZE for
 *          v_len != n;  SPRS_INCOMPATIBLE_X_SIZE for w_len != n.  w may be v.  The six outputs may be NULL.  On SPRS_BREAKDOWN w is
 *          not written.
 * Not provided: phi-functions, several output times in one call, a Lanczos shortcut for Hermitian A, a literal mode, the trace,
 * the profile hooks and a sprs_solver_* kind. */
typedef struct sprs_expm sprs_expm;
#define SPRS_EXPM_MAX_NCV 48
int sprs_expm_destroy(sprs_expm *S);           /* NULL is a no-op */
int sprs_expm_create_d(const sprs_csr *A, size_t size, size_t ncv, sprs_expm **out);
int sprs_expm_create_z(const sprs_csr *A, size_t size, size_t ncv, sprs_expm **out);
int sprs_expm_create_s(const sprs_csr *A, size_t size, size_t ncv, sprs_expm **out);
int sprs_expm_create_c(const sprs_csr *A, size_t size, size_t ncv, sprs_expm **out);
int sprs_expm_apply_d(sprs_expm *S, double t, const double *v, size_t v_len, double tol, size_t max_steps, double tau0, double *w, size_t w_len, double *err_out, double *hump_out, double *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);
int sprs_expm_apply_z(sprs_expm *S, double t, const sprs_c64 *v, size_t v_len, double tol, size_t max_steps, double tau0, sprs_c64 *w, size_t w_len, double *err_out, double *hump_out, double *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);
int sprs_expm_apply_s(sprs_expm *S, float t, const float *v, size_t v_len, float tol, size_t max_steps, float tau0, float *w, size_t w_len, float *err_out, float *hump_out, float *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);
int sprs_expm_apply_c(sprs_expm *S, float t, const sprs_c32 *v, size_t v_len, float tol, size_t max_steps, float tau0, sprs_c32 *w, size_t w_len, float *err_out, float *hump_out, float *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);
/* the same with v and w on the device (any alignment); the six outputs stay on the host */
int sprs_expm_apply_dev_d(sprs_expm *S, double t, const double *v_dev, size_t v_len, double tol, size_t max_steps, double tau0, double *w_dev, size_t w_len, double *err_out, double *hump_out, double *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);
int sprs_expm_apply_dev_z(sprs_expm *S, double t, const sprs_c64 *v_dev, size_t v_len, double tol, size_t max_steps, double tau0, sprs_c64 *w_dev, size_t w_len, double *err_out, double *hump_out, double *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);
int sprs_expm_apply_dev_s(sprs_expm *S, float t, const float *v_dev, size_t v_len, float tol, size_t max_steps, float tau0, float *w_dev, size_t w_len, float *err_out, float *hump_out, float *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);
int sprs_expm_apply_dev_c(sprs_expm *S, float t, const sprs_c32 *v_dev, size_t v_len, float tol, size_t max_steps, float tau0, sprs_c32 *w_dev, size_t w_len, float *err_out, float *hump_out, float *t_done_out, size_t *steps_out, size_t *rejects_out, size_t *matvecs_out);

/* ---------------------------------------------------------------- solver options / instrumentation
 * `solver` is a handle of any of the solver types below, `kind` says which. */
enum { SPRS_SOLVER_BICGSTAB = 1, SPRS_SOLVER_MINRES = 2, SPRS_SOLVER_CSMINRES = 3, SPRS_SOLVER_CG = 4, SPRS_SOLVER_GMRES = 5, SPRS_SOLVER_LSMR = 6, SPRS_SOLVER_IDRS = 7 };
/* mode 0 (default): fused kernels, device-resident scalars, lazy host polling.
 * mode 1: "literal" — the reference's op list one kernel per op, every scalar consumed on the
 *         host exactly where the reference consumes it (bicg_stab.rs:122-197).  IDR(s) has no such mode: mode 1 with
 *         SPRS_SOLVER_IDRS is SPRS_INVALID_ARGUMENT. */
int sprs_solver_set_mode(void *solver, int kind, int mode);
/* Per-iteration scalar trace (8 doubles per row: BiCGStab [its, r_norm, rho, alpha, w]; MINRES [its, beta, alpha, c, s, res_norm];
 * CG [its, r_norm, rho, alpha, beta]; LSMR [its, normr, normar, alpha, beta], each scalar in a (re, im) pair — LSMR's scalars
 * are real, so its imaginary slots hold 0, as the sprs_lsmr_* section says): the solver
 * synchronises every iteration while a trace buffer is set.  rows_out: rows written by the last solve. */
int sprs_solver_set_trace(void *solver, int kind, double *trace_host, size_t capacity_rows);
int sprs_solver_trace_rows(const void *solver, int kind, size_t *rows_out);
/* Device-time profile of the last solve: total milliseconds and launch count of the SpMV
 * kernel measured with HIP events on the solver's stream.  enable: 0 off; 1 every SpMV launch; k >= 2 a SAMPLE — one pair
 * of consecutive SpMV launches in k (a launch that carries events costs ~6 us more: a fifth of a 30 us iteration). */
int sprs_solver_set_profile(void *solver, int kind, int enable);
/* ... and what the timed launches were: `steps` = SpMV launches of the solve (timed or not); among the TIMED ones (the
 * `launches` of sprs_solver_get_profile) how many read a dot operand other than their input vector, how many were K2 / K4
 * launches that formed their input on the fly ("spmv_fuse").  Any pointer may be NULL. */
int sprs_solver_get_profile_counts(const void *solver, int kind, int64_t *steps, int64_t *timed_dot_other, int64_t *timed_k2_fused,
                                   int64_t *timed_k4_fused);
int sprs_solver_get_profile(const void *solver, int kind, double *spmv_ms_total, int64_t *spmv_launches,
                            double *solve_ms_total);
/* How many SpMV launches of the last solve formed their input vector on the fly (ctx knob "spmv_fuse"; MINRES: its SpMV launches that
 * multiplied by the un-normalised vector are reported in k2_fused): BiCGStab's K2 with K1's
 * update p = (v (-beta w) + p beta) + r inside, K4 with K3's r -= alpha v inside (bicg_stab.rs:155-156,172).  Zero for the other
 * solvers (CG among them) and wherever the five-launch iteration ran. */
int sprs_solver_get_fused_launches(const void *solver, int kind, int64_t *k2_fused, int64_t *k4_fused);
/* How many launches of the last solve were BiCGStab's last update walking the chains (ctx knob "bicg_k5" 1 or 2).  They are not SpMV
 * launches: sprs_solver_get_profile neither times nor counts them.  Zero for the other solvers and with "bicg_k5" 0. */
int sprs_solver_get_chain_k5_launches(const void *solver, int kind, int64_t *launches);

/* ---------------------------------------------------------------- on-chip batch solvers: many small systems, one workgroup each
 * (no reference analogue; csrc/batch.hip, csrc/batch_plan.hpp)
 * nbatch systems A_b x_b = rhs_b that share ONE square CSR pattern (n rows, nnz entries, int32 indices, every row's columns
 * strictly ascending) and have their own values: a C-contiguous (nbatch, nnz) block.  Vectors are C-contiguous (nbatch, n) blocks.
 * One workgroup of B(n) threads runs one whole solve with every vector of the recurrence in the CU's LDS; one launch serves the
 * batch; no workgroup waits for another and every loop is bounded by max_iter.  The matrix values stay in HBM / L2, the pattern
 * once and each system's values in the 64-row sliced, slice-column-major layout of csrc/sell.hpp.
 *
 * create / create_dev (the arrays on the host / on the device; both are copied, the handle owns its copies):
 *   SPRS_INVALID_ARGUMENT for a NULL ctx / pattern / out, n < 0, nnz < 0, nbatch < 0, row_ptr[0] != 0, row_ptr[n] != nnz, a row_ptr
 *   that decreases, a column outside [0, n), NULL values while nbatch * nnz > 0, and — with "the column indices of row .. are not
 *   strictly ascending" in sprs_last_error and *row_out = that row — for the lowest such row.  nbatch == 0 or n == 0 is allowed:
 *   every call on such a handle does nothing and returns SPRS_OK.  Whether every row stores its diagonal is recorded (the
 *   smallest row without one); it matters only when Jacobi is asked for.  row_out may be NULL (-1 where no row is to blame).
 * set_values[_dev]: replaces the values of all systems (pattern and plan stay).  read: the values back, (nbatch, nnz).
 * info: n, nnz, nbatch, the threads per workgroup B(n), and the LDS bytes a CG / a BiCGStab workgroup asks for; any pointer may be
 *   NULL.  sprs_batch_max_rows(solver, dtype): the row cap of a solver (SPRS_BATCH_*) for a scalar type (0 f64, 1 c64, 2 f32,
 *   3 c32), -1 for another code.
 * mul_vec[_dev]: y_b = A_b x_b for every system in one launch (any n); lengths other than nbatch * n: SPRS_DIM_MISMATCH.
 *
 * The plan (batch_plan.hpp).  B(n) = min(256, 64 ceil(n / 64)), 64 for n = 0.  CG keeps 5 vectors of n in LDS (x, r, z, p, q),
 * BiCGStab 8 (x, r, r0, y, p, v, t, z), plus 128 bytes of reduction scratch.  With 64 KiB of vectors per workgroup (two workgroups
 * and more per CU) max_rows(solver, T) = floor(65536 / (NV sizeof(T))) rounded down to a multiple of 64: BiCGStab 1024 (f64),
 * 512 (c64), 2048 (f32), 1024 (c32); CG 1600, 768, 3264, 1600.  A solve on a handle with n above the solver's cap is
 * SPRS_INVALID_ARGUMENT with n and the cap in sprs_last_error; nothing is truncated and nothing falls back.
 *
 * solve(B, precond, rhs, rhs_len, x, x_len, max_iter, tol, its_out, res_out, status_out): precond SPRS_BATCH_NONE or
 * SPRS_BATCH_JACOBI (another value: SPRS_INVALID_ARGUMENT); x is in/out; its_out / res_out / status_out are host arrays of
 * nbatch entries (any may be NULL).  rhs_len != nbatch * n: SPRS_INCOMPATIBLE_RHS_SIZE; x_len != nbatch * n:
 * SPRS_INCOMPATIBLE_X_SIZE.  Jacobi on a pattern without a full diagonal: SPRS_ZERO_DIAGONAL for the whole call, nothing is
 * launched, the row in sprs_last_error (and in its_out[0] where its_out is given).  Otherwise the call returns SPRS_OK or the status
 * of the lowest-numbered system that did not return SPRS_OK; solver events are per system and never abort the batch.
 * Jacobi: dinv_i = one / a_ii in T (DiagPrecond::new with V = T), formed by each workgroup from its system's values; a zero value
 * is not checked.  z = r * dinv_i is a product in T.
 * BiCGStab: the recurrence of sprs_bicgstab_solve_* / sprs_bicgstab_precond_solve_* per system, statement for statement (zero
 * right-hand side, early exit, restart, BreakDown, omega = 0, InsufficientIterNum); CG: the recurrence of sprs_cg_* above.  An event
 * other than SPRS_OK reports *res_out = 0 (SPRS_INVALID_PRECOND: re(rho_new)).
 *
 * The arithmetic.  Every scalar operation is in T (T::Real for norms), rounded once, nothing fused; complex products and quotients
 * are the naive formulas.  Row fold: sigma = +0; for the stored j ascending: sigma = sigma + a_ij * x_j.  A sum over rows
 * (conj_dot(a, b) = sum conj(a_i) b_i; norm2 = sqrt of sum |a_i|^2 in T::Real): thread t folds from +0 over i = t, t + B, ..
 * ascending; inside each wavefront of 64 the butterfly v[l] += v[l + off], off = 32 .. 1; then the B / 64 wavefronts left to right
 * from wavefront 0.  Every thread of the workgroup holds the same bits, so every branch on a scalar is workgroup-uniform.  A given
 * input gives the same bytes on every call and for every nbatch.
 * Limits: one pattern per batch; n up to the cap; one system per workgroup (systems far below 64 rows waste lanes); Jacobi only; no
 * mixed precision; single GPU. */
typedef struct sprs_batch sprs_batch;
enum { SPRS_BATCH_BICGSTAB = 0, SPRS_BATCH_CG = 1 };
enum { SPRS_BATCH_NONE = 0, SPRS_BATCH_JACOBI = 1 };
int sprs_batch_destroy(sprs_batch *B);     /* NULL is a no-op */
int sprs_batch_info(const sprs_batch *B, int64_t *n, int64_t *nnz, int64_t *nbatch, int64_t *threads, int64_t *lds_cg, int64_t *lds_bicgstab);
int sprs_batch_max_rows(int solver, int dtype);
int sprs_batch_create_d(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_host, const int32_t *col_idx_host, const double *values_host, sprs_batch **out, int64_t *row_out);
int sprs_batch_create_dev_d(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_dev, const int32_t *col_idx_dev, const double *values_dev, sprs_batch **out, int64_t *row_out);
int sprs_batch_set_values_d(sprs_batch *B, const double *values_host);
int sprs_batch_set_values_dev_d(sprs_batch *B, const double *values_dev);
int sprs_batch_read_d(const sprs_batch *B, double *values_host);
int sprs_batch_mul_vec_d(const sprs_batch *B, const double *x_host, size_t x_len, double *y_host, size_t y_len);
int sprs_batch_mul_vec_dev_d(const sprs_batch *B, const double *x_dev, size_t x_len, double *y_dev, size_t y_len);
int sprs_batch_bicgstab_solve_d(sprs_batch *B, int precond, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_bicgstab_solve_dev_d(sprs_batch *B, int precond, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_cg_solve_d(sprs_batch *B, int precond, const double *rhs, size_t rhs_len, double *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_cg_solve_dev_d(sprs_batch *B, int precond, const double *rhs_dev, size_t rhs_len, double *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_create_z(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_host, const int32_t *col_idx_host, const sprs_c64 *values_host, sprs_batch **out, int64_t *row_out);
int sprs_batch_create_dev_z(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_dev, const int32_t *col_idx_dev, const sprs_c64 *values_dev, sprs_batch **out, int64_t *row_out);
int sprs_batch_set_values_z(sprs_batch *B, const sprs_c64 *values_host);
int sprs_batch_set_values_dev_z(sprs_batch *B, const sprs_c64 *values_dev);
int sprs_batch_read_z(const sprs_batch *B, sprs_c64 *values_host);
int sprs_batch_mul_vec_z(const sprs_batch *B, const sprs_c64 *x_host, size_t x_len, sprs_c64 *y_host, size_t y_len);
int sprs_batch_mul_vec_dev_z(const sprs_batch *B, const sprs_c64 *x_dev, size_t x_len, sprs_c64 *y_dev, size_t y_len);
int sprs_batch_bicgstab_solve_z(sprs_batch *B, int precond, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_bicgstab_solve_dev_z(sprs_batch *B, int precond, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_cg_solve_z(sprs_batch *B, int precond, const sprs_c64 *rhs, size_t rhs_len, sprs_c64 *x, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_cg_solve_dev_z(sprs_batch *B, int precond, const sprs_c64 *rhs_dev, size_t rhs_len, sprs_c64 *x_dev, size_t x_len, size_t max_iter, double tol, size_t *its_out, double *res_out, int *status_out);
int sprs_batch_create_s(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_host, const int32_t *col_idx_host, const float *values_host, sprs_batch **out, int64_t *row_out);
int sprs_batch_create_dev_s(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_dev, const int32_t *col_idx_dev, const float *values_dev, sprs_batch **out, int64_t *row_out);
int sprs_batch_set_values_s(sprs_batch *B, const float *values_host);
int sprs_batch_set_values_dev_s(sprs_batch *B, const float *values_dev);
int sprs_batch_read_s(const sprs_batch *B, float *values_host);
int sprs_batch_mul_vec_s(const sprs_batch *B, const float *x_host, size_t x_len, float *y_host, size_t y_len);
int sprs_batch_mul_vec_dev_s(const sprs_batch *B, const float *x_dev, size_t x_len, float *y_dev, size_t y_len);
int sprs_batch_bicgstab_solve_s(sprs_batch *B, int precond, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_batch_bicgstab_solve_dev_s(sprs_batch *B, int precond, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_batch_cg_solve_s(sprs_batch *B, int precond, const float *rhs, size_t rhs_len, float *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_batch_cg_solve_dev_s(sprs_batch *B, int precond, const float *rhs_dev, size_t rhs_len, float *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_batch_create_c(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_host, const int32_t *col_idx_host, const sprs_c32 *values_host, sprs_batch **out, int64_t *row_out);
int sprs_batch_create_dev_c(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *row_ptr_dev, const int32_t *col_idx_dev, const sprs_c32 *values_dev, sprs_batch **out, int64_t *row_out);
int sprs_batch_set_values_c(sprs_batch *B, const sprs_c32 *values_host);
int sprs_batch_set_values_dev_c(sprs_batch *B, const sprs_c32 *values_dev);
int sprs_batch_read_c(const sprs_batch *B, sprs_c32 *values_host);
int sprs_batch_mul_vec_c(const sprs_batch *B, const sprs_c32 *x_host, size_t x_len, sprs_c32 *y_host, size_t y_len);
int sprs_batch_mul_vec_dev_c(const sprs_batch *B, const sprs_c32 *x_dev, size_t x_len, sprs_c32 *y_dev, size_t y_len);
int sprs_batch_bicgstab_solve_c(sprs_batch *B, int precond, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_batch_bicgstab_solve_dev_c(sprs_batch *B, int precond, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_batch_cg_solve_c(sprs_batch *B, int precond, const sprs_c32 *rhs, size_t rhs_len, sprs_c32 *x, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);
int sprs_batch_cg_solve_dev_c(sprs_batch *B, int precond, const sprs_c32 *rhs_dev, size_t rhs_len, sprs_c32 *x_dev, size_t x_len, size_t max_iter, float tol, size_t *its_out, float *res_out, int *status_out);

#ifdef __cplusplus
}
#endif
#endif /* SPRSOLVE_HIP_H */
