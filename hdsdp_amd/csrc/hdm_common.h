// hdm_common.h -- shared declarations for the MI355X (gfx950) HDSDP Schur engine.
// Internal header (C++/HIP). The public C ABI lives in include/hdsdp_mi355x.h.
#pragma once
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
#include "env_switches.h"

#include "gemm_geom.h"   // HDM_TILE / HDM_BK / HDM_SUB, HdmKLimit / HdmEpilogue / HdmRole, skyline storage, and the family's geometry
#include "gemm_calls.h"  // HdmGemmArgs and its call forms; with work_plan.h: the layout, the operand slack and the spans

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

// the GEMM family (gemm_f64.hip): its argument block and the call forms that fill it are gemm_calls.h's
int hdm_launch_gemm(const HdmGemmArgs &args, hipStream_t stream);
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
