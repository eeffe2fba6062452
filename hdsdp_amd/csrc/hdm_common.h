// hdm_common.h -- shared declarations for the MI355X (gfx950) HDSDP Schur engine.
// Internal header (C++/HIP). The public C ABI lives in include/hdsdp_mi355x.h.
#pragma once
#include <cstddef>
// Slack (bytes) appended to every device buffer that the role 1-3 GEMM kernels read as an operand: their staging loads
// carry no row mask (gemm_tile.h, SStager::load_nomask), so the last tile of the last matrix in a buffer may read up
// to 127 rows past its end.  `ld` = elements between consecutive rows (K-major) or 1 (M-major).
static inline size_t hdm_operand_pad(long ld) { return (size_t) 128 * (size_t) (ld < 16 ? 16 : ld) * 8 + 4096; }
#define HDM_OPERAND_PAD_DOUBLES 8192   /* the same slack for the [p-block][row][16] congruence output, in doubles */

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// Every device allocation of the engine goes through hdm_malloc: plain hipMalloc, and -- with HDM_POISON=1 in the environment,
// a diagnostic -- the new memory filled with 0xFF bytes (NaN as a double, -1 as an int), so that a kernel that reads what
// nobody has written shows up as NaNs in the results instead of as whatever the allocator recycled (round 4: one run of the
// ingest test read an earlier cone's data out of a fresh buffer and nothing said so).
// The engine's buffers are HdmBuf<T> / HdmPinned<T> (devbuf.h), whose alloc() calls it; the few buffers that live until the process
// ends (gemm_f64.hip, schur.hip: never freed, raw pointers on purpose) call it by name.
hipError_t hdm_malloc(void **p, size_t bytes);   // alloc.cpp
#include "devbuf.h"

#include "gemm_geom.h"   // HDM_TILE / HDM_BK / HDM_SUB, HdmKLimit / HdmEpilogue / HdmRole, skyline storage, and the family's geometry

typedef double hdm_d4 __attribute__((ext_vector_type(4)));

#define HDM_HIP_CHECK(expr)                                                                     \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            fprintf(stderr, "[hdsdp_mi355x] HIP error %s at %s:%d: %s\n", hipGetErrorName(_e),  \
                    __FILE__, __LINE__, hipGetErrorString(_e));                                 \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

// hipMemset on the legacy stream may still be in flight when work is queued on the engine's non-blocking
// stream: always drain it before anyone else touches the buffer.
static inline hipError_t hdm_memset_sync(void *p, int v, size_t bytes) {
    hipError_t e = hipMemset(p, v, bytes);
    if (e != hipSuccess) return e;
    return hipDeviceSynchronize();
}

static inline hipError_t hdm_memcpy_h2d_sync(void *dst, const void *src, size_t bytes) {
    hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    return hipDeviceSynchronize();
}

static inline long hdm_roundup(long x, long q) { return (x + q - 1) / q * q; }

// ---------------------------------------------------------------------------------------------
// GEMM family (gemm_f64.hip).  Everything is column-major fp64.
//   C[M x N] = alpha * A[M x K] * B[N x K]^T + beta * C
// Operand storage is selected per operand:
//   M-major ("N"): element (i,k) at X[i + k*ld]  (rows contiguous: a column-major M x K matrix)
//   K-major ("T"): element (i,k) at X[i*ld + k]  (k contiguous: the transpose is column-major)
// ---------------------------------------------------------------------------------------------
struct HdmGemmArgs {
    const double *A, *B;
    double *C;
    // optional second product accumulated into the same tile (SYR2K form): C = alpha (A B^T + A2 B2^T) + beta C,
    // same shapes, storage classes and K range as the first pair; A2 == nullptr: single product
    const double *A2, *B2;
    long lda2, ldb2, strideA2, strideB2;
    int b_sky;        // congruence step 1: the B operand is a batch of skyline-stored A_L matrices (N = their dimension)
    // roles 1-3 (unmasked tile loads): elements readable from each operand pointer, slack included; checked at launch
    long spanA, spanB, spanA2, spanB2;
    long lda, ldb, ldc;
    long strideA, strideB, strideC;  // batch strides (elements) along blockIdx.z (batch) -- 0 = shared
    int M, N, K;
    int a_kmajor, b_kmajor;
    long a_kblk, b_kblk;  // K-major operands: elements between consecutive 16-deep k blocks (16 for a plain matrix)
    // K-major operands may be cut into row segments (one per source rank after the multi-GPU transpose):
    // element offset += (row / seg_rows) * seg_extra.  seg_rows == 0: one segment.
    long seg_rows, seg_extra;
    int klimit;       // HdmKLimit: triangular operand => shorter K loop for early tiles
    int lower_only;   // only tiles with tile_m >= tile_n are computed (C symmetric / lower)
    unsigned long long tile_col_mask;  // != 0: only tile columns whose bit is set are computed (N <= 64 tiles; multi-GPU
                                       // builds run congruence step 2 by packed-index range, see engine.hip)
    int epilogue;     // HdmEpilogue
    int batch;        // number of batch entries (grid z for STORE/BLOCKED), or #K-splits for SLAB
    int queue_global; // persistent launches: ONE job queue for the whole chip, batch entry (K split) by batch entry in order,
                      // instead of one queue per XCD over the entries x, x + 8, ... (gemm_tile.h: hdm_gemm_persist_kernel)
    double alpha, beta;
    int role;         // HdmRole
    double flops;     // algorithmic flops of this launch (valid data only), for the live roofline
    // BLOCKED epilogue: destination chunk layout  dst[((blk*16 + c_local) * rowStride + row) * 16 + r_local]
    long blk_row_stride;  // = m_pad (number of constraint rows per 16-wide p-block)
    long blk_row0;        // constraint row of batch entry 0
    int nblk;             // n/16: sub-blocks per matrix edge
    // SLAB epilogue / split-K
    long k_chunk;         // K range per split (multiple of HDM_BK)
    long k_base;          // first k of split 0 (a launch may cover a sub-range of the splits; C then points at its first slab)
    long slab_stride;     // elements between slabs
};

int hdm_launch_gemm(const HdmGemmArgs &args, hipStream_t stream);
// while a stream capture is recording the launches (chol.hip), the launcher must not record timing events
void hdm_gemm_capture_mode(int on);
void hdm_gemm_reserve_cus(int cus);   // CUs the persistent GEMM launches leave to concurrent kernels (collectives of a sharded build)
// per-role live timing with HIP events on the launch stream (off by default)
void hdm_timing_enable(int on);
void hdm_set_debug_buffer(unsigned long long *dev, int role);
int hdm_timing_collect(double *ms, double *flops, long *launches, double *issued = nullptr);  // arrays of HDM_NROLES; resets.  issued: flops the launches' MFMA instructions executed (gemm_f64.hip: issued_mfma_flops)

// One kernel handle per translation unit with device code.  The HIP runtime loads a translation unit's code object when its
// first kernel is launched (10 ms for the first HKKTBuildUp of a process, which is a fifth of a whole solve of a 100 x 100
// block); the engine asks for one function attribute per unit on a helper thread when its first context opens instead, beside
// whatever the caller does next (presolve, the other cones' creation).  HDSDP_MI355X_PRELOAD=0: load on first use.
const void *hdm_module_handle_gemm_f64();
const void *hdm_module_handle_gemm_persist();
const void *hdm_module_handle_chol();
const void *hdm_module_handle_schur();
const void *hdm_module_handle_lanczos();
const void *hdm_module_handle_lu();
const void *hdm_module_handle_small();
const void *hdm_module_handle_bsparse();
