// dc_segment.h -- the device and host helpers the segment kernels share (dc_gat*.hip, dc_gatv2.hip, dc_transformer.hip,
// dc_sage.hip, dc_gine.hip, dc_edge.hip, dc_gmm.hip, dc_gnn_epi.hip, dc_pointnet.hip).  Internal; not for the dense / hop / attention translation units.
//
// These kernels promise: every sum in a fixed order, products and sums rounded separately, no float atomics - two runs
// give the same bits.  The promise rests on the exact operation order of the helpers below, so each is defined ONCE,
// here; a new layer's kernels include this header instead of copying.  Everything has internal linkage.
#pragma once
#include "dc_common.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }

// compensated running sum: (acc, cmp) += v, in the order of the calls
__device__ __forceinline__ void kahan_add(float &acc, float &cmp, float v) {
    const float y = v - cmp;
    const float t = acc + y;
    cmp = (t - acc) - y;
    acc = t;
}

// ---- VEC columns per lane: one float, or four as a 16-byte access -----------------------------------------------------
template <int VEC> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<4> { using T = float4; };

__device__ __forceinline__ float vec_zero(float) { return 0.0f; }
__device__ __forceinline__ float4 vec_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }

// guarded load: zeros where !ok (p is not dereferenced then)
template <class V>
__device__ __forceinline__ V vec_load(const float *p, bool ok) {
    return ok ? *reinterpret_cast<const V *>(p) : vec_zero(V{});
}

// the same as a register block whose columns can be indexed: per-column state of the kernels that sum per column
// (the float4 is formed here, not through vec_load: the kernels of dc_sage.hip allocate other registers that way)
template <int VEC> struct Cols { float a[VEC]; };
template <int VEC>
__device__ __forceinline__ Cols<VEC> cols_load(const float *p, bool ok) {
    Cols<VEC> r;
    if constexpr (VEC == 4) {
        const float4 v = ok ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
        r.a[0] = v.x, r.a[1] = v.y, r.a[2] = v.z, r.a[3] = v.w;
    } else {
        r.a[0] = ok ? *p : 0.f;
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void cols_store(float *p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// the same for an int32 image (the tie counts of a max: dc_sage.hip, dc_edge.hip); an absent element reads as 1
template <int VEC> struct Ints { int a[VEC]; };
template <int VEC>
__device__ __forceinline__ Ints<VEC> ints_load(const int32_t *p, bool ok) {
    Ints<VEC> r;
    if constexpr (VEC == 4) {
        const int4 v = ok ? *reinterpret_cast<const int4 *>(p) : make_int4(1, 1, 1, 1);
        r.a[0] = v.x, r.a[1] = v.y, r.a[2] = v.z, r.a[3] = v.w;
    } else {
        r.a[0] = ok ? *p : 1;
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void ints_store(int32_t *p, const int (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<int4 *>(p) = make_int4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// the per-column part of the backward of a sum / mean / max of rows gathered by an index (the pool and the PointNetConv
// reduction, dc_pointnet.hip): one output row from the row g of the reduced side.  mode (wave-uniform): 0 a copy of
// g_row; 1 that divided by deg; 2 the even split of the max - (v_row[c] == y_row[c]) ? g_row[c] / float(cnt_row[c]) : 0.
// !ok: a zero row, and no pointer is dereferenced but out_row.  v_row, y_row, cnt_row are read for the max alone.
template <int VEC>
__device__ __forceinline__ void reduce_bwd_cols(int mode, bool ok, float deg, const float *__restrict__ v_row,
                                                const float *__restrict__ y_row, const int32_t *__restrict__ cnt_row,
                                                const float *__restrict__ g_row, float *__restrict__ out_row, int sub,
                                                int L, int C) {
    for (int c = sub * VEC; c < C; c += L * VEC) {
        const Cols<VEC> gv = cols_load<VEC>(g_row + c, ok);
        float out[VEC];
        if (mode == 2) {
            const Cols<VEC> mv = cols_load<VEC>(v_row + c, ok);
            const Cols<VEC> yv = cols_load<VEC>(y_row + c, ok);
            const Ints<VEC> cv = ints_load<VEC>(cnt_row + c, ok);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const bool hit = ok && mv.a[k] == yv.a[k] && cv.a[k] > 0;
                const float share = gv.a[k] / (float)(hit ? cv.a[k] : 1);
                out[k] = hit ? share : 0.f;
            }
        } else if (mode == 1) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) out[k] = ok ? gv.a[k] / deg : 0.f;
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) out[k] = gv.a[k];      // (!ok: loaded as zeros)
        }
        cols_store<VEC>(out_row + c, out);
    }
}

// ---- cross-lane sums: fixed xor butterflies, widest step first; every lane of the group gets the result ---------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}
// over aligned groups of T lanes (T a power of two <= 64, a run-time value)
__device__ __forceinline__ float group_sum(float v, int T) {
    for (int d = T >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}
// the same two sums of double partial sums (dot products that cancel: dc_gmm.hip)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}
__device__ __forceinline__ double group_sum(double v, int T) {
    for (int d = T >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}
// over aligned sub-groups of SUB lanes (the lanes that share a destination segment; SUB is the kernel's choice)
template <int SUB, class T>
__device__ __forceinline__ T sub_sum(T v) {
#pragma unroll
    for (int d = SUB / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}
template <int SUB>
__device__ __forceinline__ float sub_max(float v) {
#pragma unroll
    for (int d = SUB / 2; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, kWave));
    return v;
}
template <int SUB>
__device__ __forceinline__ int sub_max(int v) {
#pragma unroll
    for (int d = SUB / 2; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, kWave));
    return v;
}

// the row this lane works for and its place in the row's lane group (lg = log2 L; WAVE: L = 64, row wave-uniform)
template <bool WAVE>
__device__ __forceinline__ bool seg_row(int lg, int64_t rows, int64_t &row, int &sub, int &L) {
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    if constexpr (WAVE) {
        row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
        sub = threadIdx.x & 63;
        L = kWave;
    } else {
        L = 1 << lg;
        row = (int64_t)lb * (256 >> lg) + (threadIdx.x >> lg);
        sub = threadIdx.x & (L - 1);
    }
    return row < rows;
}

// ---- host-side checks of the entries ------------------------------------------------------------------------------------
// rows x width, and rows x heads x channels per head: what the kernels' int arithmetic holds
inline bool sizes_ok(int64_t rows, int64_t F) { return rows < (int64_t)INT32_MAX / 4 && F < (1 << 24); }
inline bool sizes_ok(int64_t N, int64_t H, int64_t C) {
    return N < (int64_t)INT32_MAX / 4 && H < (1 << 16) && C < (1 << 24) && H * C < (1 << 24);
}
// widths the row-wise column-sum passes take: 4-column quads, a whole number of rows side by side in a workgroup
inline bool colsum_width_ok(int64_t F) { return F >= 4 && F <= 1024 && F % 4 == 0 && 256 % (F / 4) == 0; }
// lanes per head: the power of two >= units, at most one wave
inline int lanes_per_head(int64_t units) {
    int t = 1;
    while (t < kWave && t < units) t <<= 1;
    return t;
}
// log2 of the lanes per row: the power of two >= units within 4..64
inline int log2_lanes(int64_t units) {
    int lg = 2;
    while (lg < 6 && (1 << lg) < units) ++lg;
    return lg;
}

}  // namespace

}  // namespace dc
