// Internal declarations shared by the translation units of libsprsolve_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <ctime>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/sprsolve_hip.h"
#include "scalar.hpp"

namespace sprs {

constexpr int BLOCK = 256;     // threads per workgroup (4 wavefronts of 64)
constexpr uint32_t UNI2 = 0x40000000u;  // 128-row block descriptors (spmv_dict.hip), rb bit 30: every row has the SAME code sequence
constexpr uint32_t SEAM2 = 0x20000000u; // ... bit 29 (with UNI2, full 128-row blocks): all rows but one or two; rb's low bits then describe those (spmv_dict.hip)
constexpr int BICG_K5_DEFAULT = 1;   // what knob "bicg_k5" = -1 selects (bicgstab.hip).  1: + 5.9-6.3 % iterations/s at cfg 5 against 0, same box (profiles/k5_chain.md)
constexpr int MAX_GRID = 4096; // upper bound of the streaming-kernel grid (= max partials per reduction)

// device-side status word of a running solve
enum : int { ST_RUNNING = 0, ST_CONVERGED = 1, ST_RESTART = 2, ST_BREAKDOWN = 3, ST_INVALID_PC = 4,
             ST_COMM_TIMEOUT = 5 };   // a peer's hand-off never arrived in this rank's mailbox (device.hpp, mbox_sum)

// Hand-off of a fused reduction whose FINAL value is computed inside the producing launch (device.hpp,
// finalize_last_block): the workgroup that arrives last re-reduces all partials in the library's fixed order and writes
// the scalars to out0 / out1.  Used by the distributed solves, whose consumer is an ncclAllReduce of those scalars: one
// stream operation per hand-off instead of a finalize launch plus the collective.  counter == nullptr: no finalize (the
// consumer kernel re-reduces the partials itself, the single-GPU hand-off).
// Peer-to-peer mailboxes of a communicator (dist.hip, p2p_setup; SURVEY §8e's deterministic all-reduce): every rank owns one
// mailbox of MB_BYTES in uncached device memory, mapped into every other rank of the node (hipIpcOpenMemHandle).  A hand-off's
// producer writes its reduced scalars into EVERY rank's mailbox — entry [slot][parity][source rank], eight 8-byte granules
// {32 data bits, 32-bit tag}, each one naturally aligned store, so a granule is seen whole or not at all whatever the link —
// and the consumer kernels of all ranks sum the `world` entries in rank order: bit-identical on every rank, no stream operation.
constexpr int MB_SLOTS = 4, MB_RANKS = 8, MB_GRAN = 8;
constexpr size_t MB_ENTRY = MB_GRAN * 8;                                  // 64 B: two 16-byte cells (out0, out1) as 8 granules
constexpr size_t MB_BYTES = (size_t)MB_SLOTS * 2 * MB_RANKS * MB_ENTRY;   // 4 KiB
inline size_t mb_offset(int slot, int parity) { return ((size_t)slot * 2 + (size_t)parity) * MB_RANKS * MB_ENTRY; }
struct P2pBox {
    unsigned long long peer[MB_RANKS];   // rank q's mailbox as mapped on this device (own rank: the local allocation)
    int world, rank;
};

struct Fin {
    unsigned int *counter = nullptr;   // agent-scope arrival counter, zero between launches
    const void *base0 = nullptr, *base1 = nullptr;   // first partial of the WHOLE reduction (an earlier launch may have written the head)
    void *out0 = nullptr, *out1 = nullptr;           // the reduced values (16-byte slots of the solver's `red` buffer)
    int P = 0;                         // partials of the whole reduction
    // peer-to-peer hand-off: the last workgroup also posts the values into every rank's mailbox (tag != 0)
    const P2pBox *box = nullptr;
    unsigned int tag = 0;              // this hand-off's sequence number on its slot (never 0)
    unsigned int mb_off = 0;           // byte offset of [slot][parity] inside a mailbox
};

}  // namespace sprs

struct sprs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 256;
    int grid = 512;      // blocks launched by streaming / reduction kernels (multiple of 8; 2 per CU, set in sprs_ctx_create)
    int spmv_grid = -1;    // workgroups of the persistent SpMV grid; -1 = auto (4 per CU)
    // SpMV placement: -1 = auto (measured on MI355X, profiles/r01_tuning.md): matrices whose stream fits the 256 MiB
    // Infinity Cache run best with one contiguous chunk of row blocks per XCD (x stays in that XCD's L2); HBM-bound
    // ones run best round-robin (all XCDs sweep the same region, x re-reads are served by the Infinity Cache).
    int xcd_chunk = -1;
    // dictionary-compressed SpMV stream: -1 auto (the most compact the matrix qualifies for), 0 plain CSR,
    // 1 offset codes + values, 2 (offset, value) pair codes.  Read at handle creation (what is built) and at launch (what is used).
    int spmv_dict = -1;
    int spmv_wide = -1;   // f64 pair codes: two rows per lane (16-byte gathers); -1 / 1 on, 0 off
    int spmv_wideload = -1; // plain-CSR stream, f64: 16 bytes per lane per stream load, 3 workgroups per CU on HBM-sized matrices; 0 = the 4/8-byte kernel.  Read at creation and at launch
    int spmv_eqrows = -1; // plain-CSR stream: blocks of equal-length rows take their extents from the descriptor (no row_ptr read); read at creation
    int spmv_period = -1;  // XCD-period walk for matrices with a far band (3-D stencils): -1 automatic = the f64 pair-code stream only, 1 = the offset-code stream too, 0 = off.  Read at creation
    int spmv_triple = -1;  // f64 pair codes, uniform blocks: columns c - 1 and c + 1 read from column c's loads; 0 = off.  Read at creation
    int spmv_seam = -1;    // f64 pair codes: blocks that are uniform but for one or two adjacent rows lacking one slot run the uniform path; 0 = off.  Read at creation
    int spmv_tile = -1;    // f64 compressed streams: LDS x-window tiles for the near columns of uniform stencil runs (spmv_tile_kernel, spmv_tile_off_kernel): -1 automatic = vectors of 44 MiB and more (tile_wanted), 1 = every matrix that has such runs, 0 = off.  Read at creation; 0 also at launch
    int spmv_chain = -1;   // f64 pair codes, 3-D stencils: plane-streaming chains (spmv_chain_kernel): -1 automatic = wherever the tile plan is wanted and the chains fill the chip, 1 = wherever chains exist, 0 = off.  Read at creation; 0 also at launch
    int spmv_fuse = -1;    // BiCGStab (f64, no preconditioner, one GPU) on a handle whose SpMV runs through chains: K3 formed inside K4 and K1 inside K2 (bicgstab.hip, "fused SpMV input"); 0 = off.  Read per solve
    int bicg_k5 = -1;      // ... and there BiCGStab's last update K5 walks the chains too (bicgstab.hip, "K5 on the chains"): 1 = K4 stores no t, K5 folds it again; 2 = K4 stores t, K5 loads it (the same walk: pins 1 bit for bit); 0 = the vector kernel; -1 automatic (BICG_K5_DEFAULT while spmv_fuse is -1 too, else 0).  Read per solve
    int ew_chunk = -1;     // fused recurrence kernels walk one contiguous eighth of the vectors per XCD: -1 automatic (fused_chunked), 0 / 1
    int stream_nt = -1;    // fused recurrence kernels access their vectors with non-temporal loads / stores: -1 auto (by vector size), 0 / 1
    int spmv_uniform = -1; // ... and blocks whose rows all repeat one code sequence read neither codes nor row_ptr; read at creation
    int halo_overlap = 1;  // distributed SpMV: run the halo-free rows while the halo travels
    int gs_graph = 0;    // Gauss-Seidel: 1 = replay a sweep's level launches from a hipGraph (tests/test_gpu_gauss_seidel.py; no gain measured, r01_tuning.md)
    int p2p_allreduce = -1; // distributed hand-offs through the peer-to-peer mailboxes instead of ncclAllReduce: -1 / 1 wherever the communicator has them, 0 = RCCL.  Read at communicator creation (0: no mailboxes are set up) and per solve
    int p2p_timeout_ms = 20000; // a consumer that has polled its mailbox this long gives up (status ST_COMM_TIMEOUT -> SPRS_ERR_RCCL)
    int poll = 16;       // iterations between host polls of the device status word
    double *d_part = nullptr;  // reduction partials for the stand-alone vecalg entry points
    double *d_scal = nullptr;  // small device result buffer
    double *h_scal = nullptr;  // pinned host mirror
    mutable char err[512] = {0};
    // When both are set, the next SpMV kernel launch records them as its OWN begin / end (hipExtLaunchKernelGGL): the
    // solver's profile then times the kernel exactly as rocprofv3 does, without the dispatch gap two hipEventRecord
    // calls around the launch would include (1104 vs 1089 us on the cfg-5 plain stream).  Set and cleared by
    // KrylovBase::spmv under the context mutex.
    hipEvent_t prof_start = nullptr, prof_stop = nullptr;
    // Serialises every entry point that uses per-context or per-handle scratch (reduction partials, the pinned
    // scalar mirror, the host-slice staging buffers) or that must see its own results on the single stream: the
    // reference shares `&M` between threads (bicg_stab.rs:17-18 `T: Send + Sync`, mat.rs:156-161), so concurrent
    // sprs_mul_vec_* / solves on handles of ONE context must be safe.  They are: they queue behind this mutex (the
    // GPU runs one stream anyway); callers that want concurrency create one context per thread.  Recursive because
    // the blocking entry points nest (a solve calls norm2_host, mul_vec_dot calls reduce_partials_host).
    mutable std::recursive_mutex mu;
};
struct CtxLock {
    std::unique_lock<std::recursive_mutex> lk;
    explicit CtxLock(const sprs_ctx *c) { if (c) lk = std::unique_lock<std::recursive_mutex>(c->mu); }
};

#define SPRS_HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) {                                                                    \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,  \
                     hipGetErrorString(e__));                                                       \
            return SPRS_ERR_HIP;                                                                    \
        }                                                                                           \
    } while (0)

// An argument an entry point refuses with a reason: sprs_last_error reads "<entry>: <text>", the status is SPRS_INVALID_ARGUMENT.
__attribute__((format(printf, 3, 4))) static inline int refuse(const sprs_ctx *c, const char *entry, const char *fmt, ...) {
    const int at = snprintf(c->err, sizeof(c->err), "%s: ", entry);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err + at, sizeof(c->err) - (size_t)at, fmt, ap);
    va_end(ap);
    return SPRS_INVALID_ARGUMENT;
}

// Launch of an SpMV kernel on the context's stream; timed by the launch itself when a profile is being taken.
#define SPRS_LAUNCH_SPMV(c, kernel, grid, ...)                                                                            \
    do {                                                                                                                 \
        if ((c)->prof_start && (c)->prof_stop)                                                                           \
            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(sprs::BLOCK), 0, (c)->stream, (c)->prof_start, (c)->prof_stop, 0, __VA_ARGS__); \
        else                                                                                                             \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(sprs::BLOCK), 0, (c)->stream, __VA_ARGS__);                      \
    } while (0)

// SPRS_CREATE_TRACE=1: stage times of handle creation on stderr (diagnostics; profiles/r03_tuning.md §4)
struct CreateTrace {
    bool on; double t0;
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
    CreateTrace() : on(getenv("SPRS_CREATE_TRACE") != nullptr), t0(now()) {}
    void lap(const char *what) { if (!on) return; const double t = now(); fprintf(stderr, "[sprs create] %-28s %8.2f ms\n", what, t - t0); t0 = t; }
};

#define SPRS_TRY(expr)                       \
    do {                                     \
        int s__ = (expr);                    \
        if (s__ != SPRS_OK) return s__;      \
    } while (0)

// RCCL communicator of one rank (dist.hip).  RCCL is resolved with dlopen at first use, so the
// single-GPU library has no link-time dependency on it.
struct sprs_comm {
    sprs_ctx *ctx = nullptr;
    void *nccl = nullptr;   // ncclComm_t
    int world = 1, rank = 0;
    // peer-to-peer mailboxes (sprs::P2pBox): set up collectively at creation when every rank could map every other's
    bool p2p = false;
    void *mbox = nullptr;                 // this rank's mailbox (uncached device memory, MB_BYTES)
    void *peer_map[8] = {nullptr};        // the other ranks' mailboxes as opened here (hipIpcOpenMemHandle); [rank] = mbox
    sprs::P2pBox *d_box = nullptr;        // device copy of the table
    unsigned int seq[4] = {0, 0, 0, 0};   // hand-offs issued per slot: the host recurrences are replicated, so every rank counts alike
};

// Row-partition metadata of a distributed CSR operator: which local x entries each peer needs
// (packed and sent before every SpMV) and where the entries received from each peer land in
// the halo tail [n_local, n_ext) of the extended x vector.
// Runs of TILE_B consecutive full uniform 128-row blocks that share one pattern whose NEAR columns (|col - row| <= TILE_W - 2)
// are taken from an LDS window of x (spmv_dict.hip); the blocks outside those runs stay with the per-block walk (same launch)
struct sprs_tile_plan {
    int32_t *list = nullptr;       // device: {first 128-row block, first row} of each tile, eight per-XCD sections in row order
    int32_t *xstart = nullptr;     // device, 9 entries: section bounds within list
    int32_t *left = nullptr;       // device: the other blocks, in the walk order they had (128-row blocks: pair stream; 64-row blocks: offset stream)
    int n_tile = 0, n_left = 0;
    int ul = 0, fl = 0, fh = 0;    // pattern shape: slots, leading far slots, trailing far slots
    int w = 0;                     // half-width of the x window (512, or 1536 for the pair stream's long-line grids)
    int32_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double val[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // pair stream: the pattern's values
    std::vector<int32_t> h_list, h_xstart;         // host copies of list / xstart (the distributed operator cuts its interior plan from them)
};

// Plane-streaming CHAINS of the f64 pair-code stream (spmv_chain.hip, round 4): a pattern with exactly one far slot a side at
// -Pf / +Pf (a 3-D stencil's plane neighbours).  A chain = tiles of CH_B uniform 128-row blocks at rows ts, ts + Pf, ts + 2 Pf, ...
// (each within 127 rows of that, on the 128-row block grid); a workgroup walks a segment of a chain keeping the x windows of three
// consecutive tiles in LDS, so the +-Pf operands come from the neighbouring tiles' windows: no far load at all.
struct sprs_chain_plan {
    int32_t *tiles = nullptr;      // device, int4 per tile: {first 128-row block, first row, first row of the NEXT window (the chain's next tile, or ts + Pf), 0}; segments contiguous
    int32_t *segs = nullptr;       // device, int2 per segment: {first tile, tiles}
    int32_t *xstart = nullptr;     // device, 9 entries: per-XCD ranges of segs
    int32_t *left = nullptr;       // device: the 128-row blocks outside the chains, in the per-block kernel's walk order
    int n_tile = 0, n_seg = 0, n_chain = 0, n_left = 0;
    int ul = 0, tri = 0;           // pattern slots; tri: the near slots are (.., c - 1, c, c + 1, ..) around an even centre, the others even (16-byte LDS reads)
    int32_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double val[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct sprs_dist_info {
    sprs_comm *comm = nullptr;
    int64_t n_local = 0, n_ext = 0;
    std::vector<int> peer;
    std::vector<int64_t> send_off, recv_off;   // n_peers + 1 each (elements)
    int32_t *send_idx = nullptr;               // device: local indices to pack, grouped by peer
    void *send_buf = nullptr;                  // device: packed values
    // north_star's literal exchange: ncclAllGather of every rank's (padded) x slice into ag_buf, column
    // indices address ag_buf = [rank 0 slice | rank 1 slice | ...]; ag_slice == 0 selects the sparse halo
    int64_t ag_slice = 0;
    void *ag_buf = nullptr;
    // overlap of the halo exchange with the SpMV of the rows that need no halo entry
    int32_t *order_int = nullptr, *order_bnd = nullptr;   // device: interior / boundary row blocks
    int32_t n_int = 0, n_bnd = 0;
    // the same split in units of the 128-row blocks of the two-rows-per-lane kernel (null when it does not apply)
    int32_t *order_int_w = nullptr, *order_bnd_w = nullptr;
    sprs_tile_plan tile_int;       // LDS-window tiles that hold interior rows only + the interior blocks outside them (the interior launch)
    bool tile_int_off = false;     // ... of the offset-code stream (else the pair-code stream)
    int32_t n_int_w = 0, n_bnd_w = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_pack = nullptr, ev_halo = nullptr;
};

// Dictionary-compressed copy of the (col_idx, val) stream (spmv_dict.hip): one byte per nnz indexing the
// table of distinct (col - row) offsets or, for real matrices with few distinct values, the table of distinct
// (offset, value) pairs.  Built at handle creation when the matrix qualifies.
struct sprs_dict {
    uint8_t *idx_code = nullptr;   // device, nnz (+ pad): code of col - row
    uint8_t *pair_code = nullptr;  // device, nnz (+ pad): code of the (col - row, value) pair, or null
    int32_t *off_tab = nullptr;    // device, 256 entries: col - row per offset code
    int32_t *pair_off = nullptr;   // device, 256 entries: col - row per pair code
    void *pair_val = nullptr;      // device, 256 entries of T: value per pair code
    void *rowval = nullptr;        // device, nrows of T (complex scalars only): the value of each row's offset-0 entry — pair code 255 means "this row's value" (spmv_dict.hip, cpair stage)
    int n_off = 0, n_val = 0, n_pair = 0;
    void *wide_desc = nullptr;     // device: descriptors of the 128-row blocks of the two-rows-per-lane kernel (f64 pair codes)
    int n_wide = 0;
    int32_t *wide_order = nullptr; // device: XCD-period schedule of the 128-row blocks (null = natural order)
    int32_t *off_order = nullptr;  // device: the same schedule for the 64-row blocks of the offset-code stream
    int64_t period = 0;            // the far band it folds over (rows)
    int64_t max_off = -1;          // largest |col - row| of the matrix (-1: unknown)
    // tile plans of spmv_tile_kernel (f64, HBM-sized stencil-like matrices): one for the pair-code stream, one for the
    // offset-code stream (values per entry) when that is the stream the handle multiplies with
    sprs_tile_plan tile_pair, tile_off;
    sprs_chain_plan chain_pair;    // plane-streaming chains of the pair-code stream (preferred over tile_pair where it exists; knob "spmv_chain")
    void *owide_desc = nullptr;    // device: 128-row descriptors of the offset-code stream (uniform / seam blocks marked on its codes)
    int n_owide = 0;
    void *off_desc = nullptr;      // device: copy of blk_desc for the offset-code stream with the uniform blocks flagged (bit 30, nn = row length)
    int n_off_uniform = 0;
};

struct sprs_csr {
    sprs_ctx *ctx = nullptr;
    int dtype = 0;               // sprs::DT_D / DT_Z / DT_S / DT_C
    int64_t nrows = 0, ncols = 0, nnz = 0;
    int32_t *row_ptr = nullptr;  // device
    int32_t *col_idx = nullptr;  // device
    void *val = nullptr;         // device, T
    bool owns_arrays = true;
    bool was_csc = false;        // created from CSC arrays (GaussSeidel::new rejects those, gauss_seidel.rs:22-26)
    int32_t *rowblk = nullptr;   // device: n_rowblk+1 row starts, bit31 set on vector-mode blocks
    int32_t n_rowblk = 0;
    void *blk_desc = nullptr;      // device: one 16-byte {ra, rb|flag, pa, nn} descriptor per row block
    void *blk_desc_eq = nullptr;   // device: the plain-CSR kernel's copy, equal-length blocks flagged (rb bit 30, row length in nn >> 16)
    int32_t n_eq_blocks = 0;
    void *tail = nullptr;          // device, 64 B: zero-padded copy of the last 4-entry group of col_idx (16 B) and val (32 B) for spmv_wide_kernel; null = that kernel does not apply       // ... how many are flagged (their row_ptr entries are not read)
    // scratch for the host-slice trait entry points (lazily allocated)
    void *x_tmp = nullptr, *y_tmp = nullptr;
    double *part = nullptr;      // partials for mul_vec_dot
    sprs_dist_info *dist = nullptr;   // non-null: row block of a matrix partitioned over ranks
    sprs_dict *dict = nullptr;        // non-null: dictionary-compressed stream available (spmv_dict.hip)
};

// Entry points that take no distributed operator refuse one (A, or the second handle that comes with it: an adjoint, a product's
// right operand) with this text, on A's context.
static inline int single_gpu_only(const sprs_csr *A, const char *entry, const sprs_csr *B_or_null = nullptr) {
    if (!A->dist && !(B_or_null && B_or_null->dist)) return SPRS_OK;
    return refuse(A->ctx, entry, "distributed operators are not supported (single GPU only)");
}
// The linear solvers multiply size-vectors by A in place.  The reference leaves a mismatch to UB (mul_vec_unchecked); they refuse
// it rather than index out of bounds on the GPU.  A distributed row block carries its halo columns past its rows.
static inline int size_is_rows(const sprs_csr *A, size_t size) {
    const bool fits = (int64_t)size == A->nrows && (A->dist ? A->ncols >= A->nrows : (int64_t)size == A->ncols);
    return fits ? SPRS_OK : SPRS_DIM_MISMATCH;
}

struct sprs_diag {
    sprs_ctx *ctx = nullptr;
    int t_dtype = 0;    // T (sprs::DT_*)
    int v_complex = 0;  // V is complex (same precision as T)
    size_t n = 0;
    void *dinv = nullptr;  // device, V
    void *in_tmp = nullptr, *out_tmp = nullptr;
};

namespace sprs {

// ---- spmv.hip
// Which kernel an SpMV launch takes, its grid and its block walk: spmv_route() is the one place that holds this policy and
// the only code that reads the launch-time SpMV knobs.  It runs at every launch (a knob changed after creation is followed
// by the next launch).  The launches of one operator application: the whole matrix, or the interior and the boundary row
// blocks of a distributed operator split at creation (dist.hip), whose dot partials are concatenated.
enum class SpmvPart { Whole, Interior, Boundary };
enum class SpmvKernel {
    Csr,        // spmv_kernel: plain CSR, 64-row blocks (spmv.hip)
    CsrWide,    // spmv_wide_kernel: f64 plain CSR, 16-byte loads
    Dict,       // spmv_dict_kernel: offset or pair codes, lane per row (spmv_dict.hip)
    DictWide,   // spmv_dict_kernel: f64 offset codes, 16-byte value loads
    Pair2,      // spmv_pair2_kernel: f64 pair codes, two rows per lane, 128-row blocks
    TilePair,   // spmv_tile_kernel: LDS x-window tiles of the f64 pair-code stream (spmv_tile.hip)
    TileOff,    // spmv_tile_off_kernel: ... of the f64 offset-code stream (spmv_tile_off.hip)
    Chain,      // spmv_chain_kernel: plane-streaming chains of the f64 pair-code stream (spmv_chain.hip)
};
struct BlkDesc;
struct SpmvRoute {
    SpmvKernel kernel;
    int format;                     // stream: 0 plain, 1 offset codes, 2 pair codes (offset + value)
    int grid;                       // workgroups == partials this launch writes
    int xcd_chunk;                  // block walk: one contiguous chunk per XCD (1) or round-robin (0)
    const BlkDesc *desc;            // block descriptors the kernel walks
    const int32_t *order;           // ... in this order (null: natural)
    int count;                      // ... this many
    const sprs_tile_plan *tile;     // TilePair / TileOff: the plan
    const sprs_chain_plan *chain;   // Chain: the plan
    bool y_nt;                      // CsrWide / Pair2: non-temporal y stores
};
SpmvRoute spmv_route(const sprs_csr *A, SpmvPart part, bool conj_x);
// y = A x over the row blocks of `part`.  dot_mode 0: none; 1: part0[b] = sum conj(u_i) y_i; 2: part0 = sum conj(y_i) y_i,
// part1 = sum conj(y_i) u_i.  status (device int*, may be null): kernels return immediately when *status != 0.
// conj_x: gather conj(x[col]) instead of x[col] (CSMINRES: A * conj(q), cs_minres.rs:99-101, without materialising conj(q)).
template <class T>
int launch_spmv(const sprs_csr *A, SpmvPart part, const T *x, T *y, int dot_mode, const T *u, T *part0, T *part1,
                const int *status, bool conj_x = false, const Fin *fin = nullptr);
int spmv_num_partials(const sprs_csr *A);  // partials of one operator application (both launches of a split one)
// f(integral_constant<int, dot_mode>, bool_constant<flag>): the launch sites' one instantiation per (dot mode, flag)
template <class F>
inline void with_dot(int dot_mode, bool flag, F &&f) {
    auto go = [&](auto dm) { if (flag) f(dm, std::true_type{}); else f(dm, std::false_type{}); };
    if (dot_mode == 0) go(std::integral_constant<int, 0>{});
    else if (dot_mode == 1) go(std::integral_constant<int, 1>{});
    else go(std::integral_constant<int, 2>{});
}
int tile_blocks();   // 128-row blocks per LDS-window tile (spmv_dict.hip)
int build_rowblocks(sprs_csr *A, const int32_t *host_row_ptr);   // host_row_ptr == null: row_ptr lives in HBM only (summaries first)
int validate_cols_device(const sprs_csr *A);   // SPRS_INVALID_ARGUMENT if any col_idx is outside [0, ncols)
// per-row-block column span (device kernel + D2H): lo/hi sized n_rowblk
int rowblk_spans(const sprs_csr *A, std::vector<int32_t> &lo, std::vector<int32_t> &hi);
// ---- spmv_dict.hip
// SPRS_OK also when the matrix does not qualify (A->dict stays null); blk / blk_pa: the row blocks just built (first row / first entry)
int build_dict(sprs_csr *A, bool has_vector_blocks, const std::vector<int32_t> &blk, const std::vector<int32_t> &blk_pa);
void free_dict(sprs_csr *A);
// Should the fused recurrence kernels of a solve on A give every XCD one contiguous eighth of the vectors (spmv.hip)?
bool fused_chunked(const sprs_csr *A);
// the launches of routes Dict, DictWide (f64) and Pair2 (f64)
template <class T>
int launch_dict(const sprs_csr *A, const SpmvRoute &r, const T *x, T *y, int dot_mode, const T *u, T *part0, T *part1,
                const int *status, bool conj_x, const Fin &fin);
int launch_dict_wide(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                     double *part0, double *part1, const int *status, const Fin &fin);
int launch_pair2(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                 double *part0, double *part1, const int *status, const Fin &fin);
// ... TilePair (spmv_tile.hip), TileOff (spmv_tile_off.hip), Chain (spmv_chain.hip): one launch = the tiles or chains of the
// route's plan + the per-block walk over the blocks outside them
int launch_tile_pair(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                     double *part0, double *part1, const int *status, const Fin &fin);
int launch_tile_off(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                    double *part0, double *part1, const int *status, const Fin &fin);
int launch_chain_pair(const sprs_csr *A, const SpmvRoute &r, const double *x, double *y, int dot_mode, const double *u,
                      double *part0, double *part1, const int *status, const Fin &fin);

// ---- spmm.hip
// Y = A X on the plain CSR arrays for a row-major block of k <= 8 vectors with leading dimension ld >= k (X: ncols x ld,
// Y: nrows x ld); column c of Y has the bits of the SpMV of column c.  dot_mode 1: part[c * spmm_grid(A) + b] = workgroup b's
// partial of sum conj(u_ic) y_ic.  running (device int*, may be null): the launch returns at once when *running == 0.
template <class T>
int launch_spmm(const sprs_csr *A, const T *x, T *y, int ld, int k, int dot_mode, const T *u, T *part, const int *running);
int spmm_grid(const sprs_csr *A);   // workgroups == partials per column of one launch

// ---- transpose.hip / spgemm.hip / amg.hip
struct DevBufs {     // the temporaries of one construction, released on every return path
    std::vector<void *> p;
    ~DevBufs() { for (void *q : p) if (q) (void)hipFree(q); }
    template <class U> int alloc(sprs_ctx *c, U **out, size_t count) {
        *out = nullptr;
        SPRS_HIP_TRY(c, hipMalloc((void **)out, sizeof(U) * (count ? count : 1)));
        p.push_back(*out);
        return SPRS_OK;
    }
    void release(void *q) { for (auto &r : p) if (r == q) r = nullptr; }   // q now belongs to somebody else
    void free(void *q) { for (auto &r : p) if (r == q) { (void)hipFree(q); r = nullptr; } }
};

// ---- spgemm.hip
// C = A B on raw device CSR arrays (the contract of sprs_csr_matmul in the header; A is nrA x nrB, B is nrB x ncB): no handle is
// created and no stream format planned.  On SPRS_OK *c_rp (nrA + 1), *c_ci and *c_v (*c_nnz entries; at least one is allocated)
// are hipMalloc'd arrays that belong to the caller.  Checks on the device that A's columns lie in [0, nrB) and that B's rows are
// strictly ascending in [0, ncB): SPRS_INVALID_ARGUMENT with a text that starts with `who`.  info: as sprs_csr_matmul, may be
// null.  Blocking; the caller holds the context's lock and has set the device.
template <class T>
int spgemm_dev(sprs_ctx *c, const char *who, int64_t nrA, int64_t nrB, int64_t ncB, const int32_t *a_rp, const int32_t *a_ci, const T *a_v,
               const int32_t *b_rp, const int32_t *b_ci, const T *b_v, int32_t **c_rp, int32_t **c_ci, T **c_v, int64_t *c_nnz, int64_t *info);

// ---- transpose.hip
// The conjugate transpose (conj != 0) or transpose of raw device CSR arrays (nr x nc, nnz entries; the contract of sprs_csr_adjoint:
// row j holds column j's entries in ascending source row, stored order kept): no handle is created.  On SPRS_OK *rp (nc + 1), *ci
// and *v (nnz entries; at least one is allocated) are hipMalloc'd arrays that belong to the caller.  A column outside [0, nc):
// SPRS_INVALID_ARGUMENT with a text that starts with `who`.  Blocking; the caller holds the context's lock and has set the device.
template <class T>
int adjoint_dev(sprs_ctx *c, const char *who, int64_t nr, int64_t nc, int64_t nnz, const int32_t *a_rp, const int32_t *a_ci, const T *a_v, int conj,
                int32_t **rp, int32_t **ci, T **v);

// ---- blas1.hip  (all on ctx->stream, asynchronous)
template <class T, class S> int launch_axpy(sprs_ctx *c, size_t n, S a, const T *x, T *y);
template <class T> int launch_axpby(sprs_ctx *c, size_t n, T a, const T *x, T b, T *y);
template <class T> int launch_scale(sprs_ctx *c, size_t n, T a, T *x);
template <class T> int launch_rscale(sprs_ctx *c, size_t n, Real<T> a, T *x);
template <class T> int launch_conj(sprs_ctx *c, size_t n, const T *in, T *out);
template <class T, class V> int launch_diag_apply(sprs_ctx *c, size_t n, const V *dinv, const T *in, T *out);
template <class V> int launch_diag_inv(sprs_ctx *c, size_t n, const V *diag, V *dinv);
// reductions: blocking, result returned to the host
// comm != null: the locally reduced value is all-reduced over the ranks before it is returned
template <class T> int dot_host(sprs_ctx *c, size_t n, const T *x, const T *y, bool conj, T *out, sprs_comm *comm = nullptr);
template <class T> int norm2_host(sprs_ctx *c, size_t n, const T *x, Real<T> *out, sprs_comm *comm = nullptr);
// reduce `P` partials of T (or of double when T_is_real_partials) with the library's fixed order; blocking
template <class T> int reduce_partials_host(sprs_ctx *c, const T *part, int P, T *out, sprs_comm *comm = nullptr);

// ---- what the set-ups and host entry points of the preconditioner handles share (capi.hip's sprs_diag, ilu0.hip, amg.hip, gs.hip)
// hipMalloc'd copy of a host array (two elements more than it holds: an empty one still owns an allocation)
template <class U>
bool dev_upload(U **dst, const U *src, size_t count) {
    if (hipMalloc((void **)dst, sizeof(U) * (count + 2)) != hipSuccess) return false;
    return count == 0 || hipMemcpy(*dst, src, sizeof(U) * count, hipMemcpyHostToDevice) == hipSuccess;
}

// The device arrays of a single-GPU CSR matrix without the handle around them: what a set-up that runs on raw arrays (ILU(0) on a
// permuted copy) is given, so that it cannot read handle state that is not there.
struct CsrView {
    sprs_ctx *ctx;
    int dtype;
    int64_t nrows, ncols, nnz;
    const int32_t *row_ptr, *col_idx;
    const void *val;
};
inline CsrView csr_view(const sprs_csr *A) { return CsrView{A->ctx, A->dtype, A->nrows, A->ncols, A->nnz, A->row_ptr, A->col_idx, A->val}; }

// A's pattern (and, where val_host is given, its nnz values) on the host, with the check that every row's columns ascend
// strictly: SPRS_INVALID_ARGUMENT and a text that starts with `who`.  The caller holds the context's lock and has set the device.
inline int host_pattern(const CsrView &A, const char *who, std::vector<int32_t> &rp, std::vector<int32_t> &ci, void *val_host = nullptr) {
    sprs_ctx *c = A.ctx;
    rp.assign((size_t)A.nrows + 1, 0); ci.resize((size_t)A.nnz);
    SPRS_HIP_TRY(c, hipMemcpyAsync(rp.data(), A.row_ptr, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, c->stream));
    if (A.nnz) SPRS_HIP_TRY(c, hipMemcpyAsync(ci.data(), A.col_idx, sizeof(int32_t) * ci.size(), hipMemcpyDeviceToHost, c->stream));
    if (A.nnz && val_host) SPRS_HIP_TRY(c, hipMemcpyAsync(val_host, A.val, dtype_size(A.dtype) * (size_t)A.nnz, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < A.nrows; ++i)
        for (int32_t k = rp[i] + 1; k < rp[i + 1]; ++k)
            if (ci[k] <= ci[k - 1]) {
                snprintf(c->err, sizeof(c->err), "%s: the column indices of row %lld are not strictly ascending", who, (long long)i);
                return SPRS_INVALID_ARGUMENT;
            }
    return SPRS_OK;
}
inline int host_pattern(const sprs_csr *A, const char *who, std::vector<int32_t> &rp, std::vector<int32_t> &ci, void *val_host = nullptr) {
    return host_pattern(csr_view(A), who, rp, ci, val_host);
}

// position of the diagonal entry of row i in ci (columns strictly ascending), or -1
inline int64_t diag_pos(const int32_t *rp, const int32_t *ci, int64_t i) {
    const int32_t *b = ci + rp[i], *e = ci + rp[i + 1], *d = std::lower_bound(b, e, (int32_t)i);
    return d != e && *d == (int32_t)i ? d - ci : -1;
}

// a pivot nobody may divide by: exactly zero, or not finite
template <class T> SPRS_HD bool bad_pivot(T u) {
    using std::isfinite;
    const Real<T> re = sre(u), im = sim(u);
    return !isfinite(re) || !isfinite(im) || (re == Real<T>(0) && im == Real<T>(0));
}

// rows in level order (ascending inside a level) and the levels' extents
inline void group_by_level(const std::vector<int32_t> &level, int32_t nlev, std::vector<int32_t> &lvl_ptr, std::vector<int32_t> &rows) {
    const size_t n = level.size();
    lvl_ptr.assign((size_t)nlev + 1, 0);
    for (size_t i = 0; i < n; ++i) lvl_ptr[(size_t)level[i] + 1]++;
    for (int32_t l = 0; l < nlev; ++l) lvl_ptr[l + 1] += lvl_ptr[l];
    std::vector<int32_t> fill(lvl_ptr.begin(), lvl_ptr.end() - 1);
    rows.resize(n);
    for (size_t i = 0; i < n; ++i) rows[(size_t)fill[level[i]]++] = (int32_t)i;
}

// The host entry point of a handle H with {ctx, n, in_tmp, out_tmp}: `in` to the handle's staging vector, apply(in_tmp, out_tmp) on
// the stream, the result back to `out`; blocking.  The caller has checked its arguments (n elements each way).
template <class T, class H, class F>
int staged_apply(const H *Pc, const T *in, T *out, F &&apply) {
    H *P = const_cast<H *>(Pc);
    sprs_ctx *c = P->ctx;
    const size_t n = (size_t)P->n;
    CtxLock lock(c);   // in_tmp / out_tmp are per-handle staging
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (!P->in_tmp) SPRS_HIP_TRY(c, hipMalloc(&P->in_tmp, sizeof(T) * (n + 2)));
    if (!P->out_tmp) SPRS_HIP_TRY(c, hipMalloc(&P->out_tmp, sizeof(T) * (n + 2)));
    SPRS_HIP_TRY(c, hipMemcpyAsync(P->in_tmp, in, sizeof(T) * n, hipMemcpyHostToDevice, c->stream));
    SPRS_TRY(apply((const T *)P->in_tmp, (T *)P->out_tmp));
    SPRS_HIP_TRY(c, hipMemcpyAsync(out, P->out_tmp, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

// What the solvers ask of an applied handle H with {ctx, dtype, n} before they use it: SPRS_INVALID_ARGUMENT unless P has the scalar
// type `dtype` and lives on A's context and A is on one GPU, SPRS_DIM_MISMATCH unless it has n rows.
template <class H>
int applied_check(const H *P, const sprs_csr *A, int dtype, size_t n) {
    if (!P || !A || P->dtype != dtype || P->ctx != A->ctx || A->dist) return SPRS_INVALID_ARGUMENT;
    if ((size_t)P->n != n) return SPRS_DIM_MISMATCH;
    return SPRS_OK;
}

// ---- ilu0.hip
// The solvers' view of an ILU(0) handle.  ilu0_check: applied_check.  ilu0_apply: out = U^-1 L^-1 in (which = 0), L^-1 in (1) or
// U^-1 in (2) on device vectors, asynchronous on the context's stream; in == out is allowed.
int ilu0_check(const sprs_ilu0 *P, const sprs_csr *A, int dtype, size_t n);
template <class T> int ilu0_apply(const sprs_ilu0 *P, int which, const T *in, T *out);

// ---- order.hip
// perm (host, new -> old) is a permutation of 0 .. n - 1, or SPRS_INVALID_ARGUMENT with "<who>: ..." in the context's text.
int perm_check(const sprs_ctx *c, const char *who, const int32_t *perm, size_t len, int64_t n);
// The colours of sprs_csr_color on the host (the header's rule); ncolors / rounds may be null.  Blocking; takes the lock itself.
int csr_color_host(const sprs_csr *A, uint64_t seed, std::vector<int32_t> &colors, int64_t *ncolors, int64_t *rounds);
// The stable sort of the rows by colour: perm (new -> old), rows of one colour ascending.
std::vector<int32_t> color_major_perm(const std::vector<int32_t> &colors, int64_t ncolors);
// B = P A P^T on raw device arrays (the contract of sprs_csr_permute; perm_dev a checked permutation): *rp (n + 1), *ci, *val
// (nnz entries of A's scalar type; at least one is allocated) and, where src is not null, *src (per entry of B its position in
// A's arrays) are hipMalloc'd arrays that belong to the caller.  No handle is created.  Blocking; the caller holds the lock and
// has set the device.
int csr_permute_arrays(const sprs_csr *A, const int32_t *perm_dev, int32_t **rp, int32_t **ci, void **val, int32_t **src);

// ---- amg.hip
// The same for an AMG handle: amg_check as ilu0_check, amg_apply: out = one V(1,1) cycle on in; in == out is allowed.
int amg_check(const sprs_amg *P, const sprs_csr *A, int dtype, size_t n);
template <class T> int amg_apply(const sprs_amg *P, const T *in, T *out);

// ---- fsai.hip
// The same for an FSAI handle: fsai_check as ilu0_check, fsai_apply: out = G^H (G in), two launch_spmv calls; in == out is allowed.
int fsai_check(const sprs_fsai *P, const sprs_csr *A, int dtype, size_t n);
template <class T> int fsai_apply(const sprs_fsai *P, const T *in, T *out);
// The lowest row of A whose column indices do not ascend strictly, looked for on the device (the pattern never crosses PCIe):
// SPRS_INVALID_ARGUMENT and "<who>: the column indices of row .. are not strictly ascending".  Blocking; the caller holds the
// context's lock and has set the device.
int sorted_columns_dev(const sprs_csr *A, const char *who);

// ---- bjacobi.hip
// The same for a block-Jacobi handle: bjacobi_check as ilu0_check, bjacobi_apply: out = blockdiag(A_bb)^-1 in, one launch; in == out
// is allowed.
int bjacobi_check(const sprs_bjacobi *P, const sprs_csr *A, int dtype, size_t n);
template <class T> int bjacobi_apply(const sprs_bjacobi *P, const T *in, T *out);

// ---- an applied preconditioner: a handle whose application is a chain of launches of its own (ILU(0)'s triangular solves,
// AMG's cycle, FSAI's two SpMVs, block-Jacobi's one launch), asynchronous on the context's stream.  check: SPRS_INVALID_ARGUMENT for a null handle, another scalar type or
// context, or a distributed A; SPRS_DIM_MISMATCH for another size.  apply: out = M in on device vectors, in == out allowed.
template <class T>
struct AppliedPrec {
    const void *h = nullptr;
    int (*check_fn)(const void *h, const sprs_csr *A, int dtype, size_t n) = nullptr;
    int (*apply_fn)(const void *h, const T *in, T *out) = nullptr;
    int check(const sprs_csr *A, size_t n) const { return h && check_fn ? check_fn(h, A, dtype_of<T>::value, n) : SPRS_INVALID_ARGUMENT; }
    int apply(const T *in, T *out) const { return apply_fn(h, in, out); }
};
template <class T> AppliedPrec<T> ilu0_prec(const sprs_ilu0 *P);   // the which = 0 solve
template <class T> AppliedPrec<T> amg_prec(const sprs_amg *P);
template <class T> AppliedPrec<T> fsai_prec(const sprs_fsai *P);
template <class T> AppliedPrec<T> bjacobi_prec(const sprs_bjacobi *P);

// ---- what a solve is preconditioned with, from the C entry points down: nothing (a null sprs_diag), a diagonal (Jacobi) or
// an applied handle (BiCGStab, MINRES, CG and GMRES; CSMINRES refuses any preconditioner and the batched CG takes a sprs_diag
// only).  with_prec() (krylov.hpp) checks it and
// resolves it into the Prec<T, V> the runs receive.
template <class T>
struct Precond {
    const sprs_diag *diag = nullptr;
    AppliedPrec<T> applied;
    bool is_applied = false;            // (an applied one whose handle is null is still one: it is refused, not ignored)
    Precond(const sprs_diag *d = nullptr) : diag(d) {}
    Precond(const AppliedPrec<T> &a) : applied(a), is_applied(true) {}
    bool any() const { return diag || is_applied; }
};

// ---- dist.hip
// exchange the halo entries of the extended vector x (local part [0,n_local) already in place)
template <class T> int halo_exchange(const sprs_csr *A, T *x_ext);
// split form used for overlap: pack + exchange on the communication stream (returns immediately),
// then make the compute stream wait for the halo
template <class T> int halo_begin(const sprs_csr *A, T *x_ext);
int halo_wait(const sprs_csr *A);
template <class T>
int dist_spmv(const sprs_csr *A, T *x_ext, T *y, int dot_mode, const T *u, T *part0, T *part1, const int *status, bool conj_x,
              const Fin *fin = nullptr);   // fin: handed to the LAST launch of the operator (P and base pointers span all of them)
int allreduce_sum(sprs_comm *comm, void *dev, size_t count, bool f32 = false);   // in place, on the ctx stream; count elements of f64 (or f32)

// sprsolve_amd.gen.uniform's values on the host: a U[-1, 1) double from the top 53 bits of counter-based splitmix64, seed
// "PRSOLVE".  LOBPCG's default start block (streams 100 + ..) and IDR(s)'s shadow space (streams 200 + ..) are made of them.
inline double gen_uniform(uint64_t stream, uint64_t i) {
    uint64_t z = 0x5052534F4C5645ull + stream * 0xD1B54A32D192ED03ull + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return -1.0 + 2.0 * ((double)(z >> 11) * (1.0 / 9007199254740992.0));
}

inline int grid_for(const sprs_ctx *c) {
    int g = c->grid;
    if (g < 8) g = 8;
    if (g > MAX_GRID) g = MAX_GRID;
    return g & ~7;
}

// Non-temporal vector accesses — operand loads and result stores of the fused recurrence kernels, the y stores of the
// pair-code SpMV: knob "stream_nt" (1 / 0), automatic (-1) from the size of one vector.  Measured cross-over: 64 MB
// (-0.9 %; at 50 MB the vectors of a solve live in the 256 MiB Infinity Cache: -3 %) to 80 MB (+3.6 %; 100-200 MB: +11 %),
// profiles/r02_tuning.md §20.
inline bool stream_loads_nt(const sprs_ctx *c, size_t vector_bytes) {
    if (c->stream_nt >= 0) return c->stream_nt != 0;
    return vector_bytes >= (size_t)72 << 20;
}
// the whole stream + three vectors fit the 256 MiB Infinity Cache (spmv.hip: XCD-chunked walks for these, round-robin otherwise)
inline bool is_cache_resident(const sprs_csr *A) {
    const double s = (double)dtype_size(A->dtype);
    return (double)A->nnz * (s + 4) + 3.0 * A->nrows * s < 192.0 * 1024 * 1024;
}

// LDS-window tiles of the compressed-stream SpMVs (spmv_dict.hip): knob "spmv_tile" 1 / 0, automatic (-1) from the size of one
// vector.  Measured cross-over on 500 x 500 x nz slabs (per-block kernel -> tiles, SpMV us in the solve; profiles/r03_tuning.md
// §9): 16 MB 15.6 -> 31.9, 32 MB 22.1 -> 30.3, 50 MB 36.5 -> 33.6, 100 MB 71.8 -> 64.6, 200 MB 139 -> 110, 400 MB 278 -> 213.
inline bool tile_wanted(const sprs_ctx *c, size_t vector_bytes) {
    if (c->spmv_tile >= 0) return c->spmv_tile != 0;
    return vector_bytes >= (size_t)44 << 20;
}

// Grid of a grid-stride streaming pass over `work` tiles: no more workgroups than the context's grid, and as few as make
// every workgroup take the same number of trips (1953 tiles on 512 workgroups are 4 trips for most and 3 for some —
// 496 workgroups take 4 each and the pass ends 5 % sooner; at HBM sizes the difference vanishes).  Multiple of 8 (XCDs).
inline int balanced_grid(const sprs_ctx *c, int64_t work) {
    const int g0 = grid_for(c);
    if (work <= g0) return (int)(work < 1 ? 1 : work);
    const int64_t trips = (work + g0 - 1) / g0;
    int64_t g = (work + trips - 1) / trips;
    g = (g + 7) & ~(int64_t)7;
    return (int)(g > g0 ? g0 : g);
}

}  // namespace sprs
