// dc_common.h -- shared helpers for the gfx950 kernels (internal; the public
// surface is include/deformcontact.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/deformcontact.h"

namespace dc {

constexpr int kWave = 64;      // CDNA4 wavefront
constexpr int kXcds = 8;       // MI355X: 8 XCDs, each with a private 4 MiB L2

void set_error(const char *fmt, ...);

// launch log (dc_kernel_trace / dc_kernel_trace_dump, dc_core.hip): off unless a test or tool switches it on.
// g_trace_on is a bit set: kTraceLog (the launch log counts) | kTraceCoverage (dc_launch_coverage: the cumulative set
// of launch sites reached), so that a launch pays ONE predictable branch when both are off
constexpr int kTraceLog = 1, kTraceCoverage = 2;
extern int g_trace_on;
void trace_kernel_slow(const char *name);
inline void trace_kernel(const char *name) {
    if (__builtin_expect(g_trace_on, 0)) trace_kernel_slow(name);
}

// One record per launch site, emitted into the link section "dc_sites" by DC_LAUNCH / DC_LAUNCH_SITE: the library
// lists its own launches (dc_launch_sites_dump walks __start_dc_sites .. __stop_dc_sites; host code only, no GPU
// needed).  A templated host launcher yields one record per instantiation, told apart by `where`
// (__PRETTY_FUNCTION__ names the template arguments).
struct Site {
    const char *kernel;   // the kernel expression as written at the site
    const char *where;    // __PRETTY_FUNCTION__ of the enclosing host function
    const char *file;     // __FILE__
};
void trace_site_slow(const Site *site, const char *name);
inline void trace_site(const Site *site, const char *name) {
    if (__builtin_expect(g_trace_on, 0)) trace_site_slow(site, name);
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// An environment switch: its integer value, `dflt` when unset or empty.  The ONE reader of the environment in csrc/ (but
// for dc_core.hip's PYTEST_CURRENT_TEST).  Two read times, chosen at the call site: a switch that tests flip inside one
// process (DC_CSR_BUCKETS*, DC_CSR_BUCKET_SHIFT, DC_DW_BF16_DMA) is read on every call; one that only chooses between
// kernels for a whole process (DC_H2_*, DC_DW_WIDE, DC_DENSE_TRACE; tests set those through child processes) is read
// once, into a function-local `static const int`.
inline int64_t env_int64(const char *name, int64_t dflt) {
    const char *v = getenv(name);
    return (v && *v) ? atoll(v) : dflt;
}
inline int env_int(const char *name, int dflt) { return (int)env_int64(name, dflt); }

inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return DC_ELAUNCH;
    }
    return DC_OK;
}

// XCD-aware block remap (bijective for any grid size).  Workgroups are dealt
// round-robin over the 8 XCDs, so hardware blocks b and b+8 share an L2.  The
// remap hands XCD k the k-th CONTIGUOUS chunk of logical blocks: rows of one
// mesh (block-diagonal batch => its neighbours too) are then gathered through
// one L2 instead of all eight.  Speed only; any placement is correct.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk) {
    const unsigned q = nblk / kXcds, r = nblk % kXcds;
    const unsigned xcd = bid % kXcds, idx = bid / kXcds;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// gcn_norm's deg.pow(-0.5) with inf -> 0 (PyG gcn_conv.py: gcn_norm): ONE definition, so that every kernel that
// forms a weight dis[source] * dis[destination] (dc_csr.hip writes them, dc_hopchain.hip re-forms them) gets the same bits
__device__ __forceinline__ float inv_sqrt_count(int d) {
    return d > 0 ? 1.0f / sqrtf((float)d) : 0.0f;
}

// ReLU of every fused epilogue, torch.threshold's semantics: NaN stays NaN (fmaxf(NaN, 0) is 0 and would hide a
// diverged run), -0.0 -> +0.  ONE definition.  IEEE 754-2019 maximum, which propagates NaN and
// orders -0 below +0: one v_maximum3_f32 on gfx950, where `v <= 0.f ? 0.f : v` is a compare and a select
__device__ __forceinline__ float relu_keep_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }

// one step of the max aggregations' walk (SAGE, EdgeConv / PointNetConv, global_max_pool): the running maximum mx and
// the number ct of candidates that attain it take in n candidates of value a (n > 1: a merged partial result).  Greater:
// the maximum is replaced and the count starts again; equal: n more.  A NaN candidate wins and then stays (NaN > x is
// false for every x), as in torch's scatter_reduce(..., 'amax'); the count of a NaN maximum is the number of NaN
// candidates.  +-Inf are ordinary values: the maximum is a selection
__device__ __forceinline__ void max_step(float a, int n, float &mx, int &ct) {
    const bool a_nan = a != a, take = a > mx || a_nan;
    ct = mx != mx ? (a_nan ? ct + n : ct) : (take ? n : (a == mx ? ct + n : ct));
    mx = take ? a : mx;
}

// ---- primitives with users outside the dense family (dc_spmm.hip, dc_hopchain.hip, dc_attn.hip); the dense
// kernels' own are in dc_dense.h ----
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// an LDS object's 32-bit byte address (for offsets folded by hand)
__device__ __forceinline__ unsigned lds_addr(const void *p) {
    return (unsigned)(uintptr_t)(const void __attribute__((address_space(3))) *)p;
}

// this wave's LDS operations have completed (reads returned, writes landed), then the workgroup meets.  NOT
// __syncthreads(): its fence also waits for vmcnt(0), i.e. for global loads issued ahead on purpose and for stores
// that may keep draining
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// fp32 -> bf16 bits, round to nearest even, NaN kept quiet
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);   // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

}  // namespace dc

// the static record of one launch site (dc::Site), placed in the link section the library walks
#define DC_SITE_RECORD(text) \
    static const dc::Site dc_site_ __attribute__((section("dc_sites"), used)) = {text, __PRETTY_FUNCTION__, __FILE__}

// every kernel launch of the library: the site is on record (DC_SITE_RECORD), and the kernel expression as written
// (template arguments included) goes to the launch log / the site to the reached set when they are on
#define DC_LAUNCH(kernel, ...)                     \
    do {                                           \
        DC_SITE_RECORD(#kernel);                   \
        dc::trace_site(&dc_site_, #kernel);        \
        hipLaunchKernelGGL(kernel, __VA_ARGS__);   \
    } while (0)

// a launch written out by hand (hipLaunchKernelGGL with a name of its own in the launch log): registers the site
// under `name`, which must have static storage and a constant address
#define DC_LAUNCH_SITE(name)                 \
    do {                                     \
        DC_SITE_RECORD(name);                \
        dc::trace_site(&dc_site_, name);     \
    } while (0)

// the global source and the LDS destination of the LDS-DMA builtins (__builtin_amdgcn_global_load_lds,
// __builtin_amdgcn_raw_ptr_buffer_load_lds).  Macros, not functions: called through a __device__ function from a
// kernel template, the host pass silently dropped the template's instantiations (k_fwd_h2: undefined launch stubs)
#define DC_DMA_SRC(p) ((const void __attribute__((address_space(1))) *)(p))
#define DC_DMA_DST(p) ((void __attribute__((address_space(3))) *)(p))

// s_waitcnt vmcnt(n) only: the other counters stay as they are
#define DC_WAITVM(n) __builtin_amdgcn_s_waitcnt(0x0F70 | ((n) & 15) | (((n) >> 4) << 14))

#define DC_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            dc::set_error(__VA_ARGS__);  \
            return DC_EINVAL;            \
        }                                \
    } while (0)
