// dc_transformer.hip -- TransformerConv (PyG 2.5.2 transformer_conv.py): the scaled dot-product score, its edge softmax
// and both sides of its backward on the sorted adjacency.
//
// With q = lin_query(x), k = lin_key(x), v = lin_value(x) viewed as [N, H, C], for edge p from j into i, head h:
//   e[p,h] = (sum_c q[i,h,c] k[j,h,c]) * scale          (scale = float32(1 / sqrt(C)), given by the caller)
//   alpha[p,h] = softmax of e[.,h] over the edges into i (maximum subtracted, + 1e-16 in the denominator)
// As in dc_gatv2.hip the logit is per edge and head and gathers H*C floats per edge; per-edge vectors are EDGE-MAJOR
// [capacity, H], and the aggregation (dc_spmm_f32_heads_bias_act, of v) and the SDDMM (dc_sddmm_f32_heads: galpha =
// <gm[i], v[j]>) are the ones of dc_gat_heads.hip.  The edge set is taken as given: a destination may have NO edge.
//
// Rules of the segment kernels (the order-defining helpers: see dc_segment.h): destination-sorted segments, every sum
// in a fixed order, products and sums rounded separately, no float atomics, no host read - two runs give the same bits.
// The long sums (a segment's softmax
// denominator, its sum of alpha galpha, the per-column sums over a segment's edges) are compensated (Kahan).  Any
// H >= 1, C >= 1 and in-degree, 0 included, N = 0: no width cap - what a lane cannot hold in registers it reads again
// (forward) or works through in column chunks (backward).
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

// acc += sum over the lane's channels of q * k, channel order
__device__ __forceinline__ void tc_score(float &acc, float q, float k) {
    const float m = q * k;
    acc = acc + m;
}
__device__ __forceinline__ void tc_score(float &acc, const float4 &q, const float4 &k) {
    tc_score(acc, q.x, k.x);
    tc_score(acc, q.y, k.y);
    tc_score(acc, q.z, k.z);
    tc_score(acc, q.w, k.w);
}

// the gradient of the scaled dot product from the softmax's: ONE expression, so that the value the destination side
// stores (gl) and the one it uses for g_q are the same bits
__device__ __forceinline__ float tc_logit_grad(float alpha, float galpha, float dot, float scale) {
    const float d = galpha - dot;
    const float ge = alpha * d;
    return ge * scale;
}

}  // namespace

// ---- forward: score + edge softmax ---------------------------------------------------------------------------------------
// One wave per destination row, the head / lane-group scheme of k_gatv2_softmax_fwd: a head is an aligned group of T
// lanes (T = the power of two >= C / VEC, at most 64); G = 64 / T heads make a pass, lane (grp, sub) owns the channel
// units sub, sub + T, ... of head h0 + grp.  Per pass the lane's part of q[i] sits in registers (the first kRegTc units;
// a wider head reads the rest again), every k[j] element is gathered once, U edges in flight; the head's sum over c:
// the lane's channels in order, then the fixed butterfly, which leaves the logit (and so the running maximum) on every
// lane of the group.  The edges of the segment are dealt round-robin to the lanes of the group: lane `sub` stores
// the raw logits of the edges beg + sub, + T, ... into alpha, turns exactly those into exp(e - max) - its compensated
// sum joins the group's by the butterfly - and then into the weights: a hub's exp / normalise passes run T wide, and
// a lane reads back only what it wrote itself.
constexpr int kRegTc = 4;
constexpr int kEdgesTc = 4;

template <int VEC>
__global__ void __launch_bounds__(256)
k_tconv_softmax_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ q,
                    int64_t ldq, const float *__restrict__ k, int64_t ldk, float scale, float *alpha, int64_t N, int H,
                    int C, int T) {
    using V = typename Vec<VEC>::T;
    constexpr int U = kEdgesTc;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    if (beg >= end) return;                                    // no edge into this row: nothing to write
    const int Cv = C / VEC, G = kWave / T, J = (Cv + T - 1) / T;
    const int sub = lane & (T - 1), grp = lane / T;
    for (int h0 = 0; h0 < H; h0 += G) {
        const int h = h0 + grp;
        const bool hv = h < H;
        const int64_t hcol = (int64_t)h * C;
        V qr[kRegTc];
#pragma unroll
        for (int r = 0; r < kRegTc; ++r) {
            const int cu = sub + T * r;
            qr[r] = vec_load<V>(q + row * ldq + hcol + cu * VEC, hv && cu < Cv);
        }
        float m = -INFINITY;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;                             // wave-uniform
            int64_t s[U];
            float acc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = u < n ? other[p + u] : row;
                acc[u] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < kRegTc; ++r) {
                if (r < J) {                                   // wave-uniform
                    const int cu = sub + T * r;
                    const bool ok = hv && cu < Cv;
                    V kv[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) kv[u] = vec_load<V>(k + s[u] * ldk + hcol + cu * VEC, ok && u < n);
#pragma unroll
                    for (int u = 0; u < U; ++u) tc_score(acc[u], qr[r], kv[u]);
                }
            }
            for (int r = kRegTc; r < J; ++r) {                 // heads wider than the registers hold: q read again
                const int cu = sub + T * r;
                const bool ok = hv && cu < Cv;
                const V qv = vec_load<V>(q + row * ldq + hcol + cu * VEC, ok);
                V kv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) kv[u] = vec_load<V>(k + s[u] * ldk + hcol + cu * VEC, ok && u < n);
#pragma unroll
                for (int u = 0; u < U; ++u) tc_score(acc[u], qv, kv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {                                   // wave-uniform
                    const float e = group_sum(acc[u], T) * scale;
                    m = fmaxf(m, e);
                    if (hv && ((p + u - beg) & (T - 1)) == sub) alpha[(int64_t)(p + u) * H + h] = e;
                }
        }
        // the lane's own edges: exp(e - max) with its compensated sum, the group's sum by the butterfly, the weights
        float sum = 0.f, cmp = 0.f;
        if (hv)
            for (int p = beg + sub; p < end; p += T) {
                float *al = alpha + (int64_t)p * H + h;
                const float ex = expf(*al - m);
                *al = ex;
                kahan_add(sum, cmp, ex);
            }
        const float den = group_sum(sum, T) + 1e-16f;
        if (hv)
            for (int p = beg + sub; p < end; p += T) {
                float *al = alpha + (int64_t)p * H + h;
                *al = *al / den;
            }
    }
}

// ---- backward, destination side ---------------------------------------------------------------------------------------------
// One wave per destination row i, ONE launch, no workspace:
//   dot[h]     = sum over the segment of alpha[p,h] galpha[p,h]    (the 64 lanes take the edges beg + lane, + 64, ...,
//                each a compensated sum in p order, then the fixed butterfly)
//   gl[p,h]    = alpha[p,h] (galpha[p,h] - dot[h]) * scale         (the gradient of <q_i, k_j>; stored for the source side)
//   g_q[i,h,c] = sum over the edges p into i, in p order, of gl[p,h] k[j,h,c]
// Columns as k_gatv2_dst_bwd: lane l owns the column units u0 + l, u0 + 64 + l of a chunk of kRegUTc * 64 units (a
// unit = VEC columns of one head), chunk by chunk.  A chunk needs the dot of the heads its columns lie in: they are
// formed in front of the chunk (a head wider than a chunk: once per chunk it reaches into - H floats per edge against
// the H*C the chunk gathers) and gl of a head is stored by the chunk in which the head begins.  The column sums form
// gl again from alpha, galpha and dot (tc_logit_grad: the same bits) - a lane never reads what another lane stored.
// A row without edges stores zeros.
constexpr int kRegUTc = 2;

template <int VEC>
__global__ void __launch_bounds__(256)
k_tconv_dst_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ alpha,
                const float *__restrict__ galpha, const float *__restrict__ k, int64_t ldk, float scale,
                float *__restrict__ gl, float *__restrict__ g_q, int64_t ldgq, int64_t N, int H, int C) {
    constexpr int R = kRegUTc, U = kEdgesTc;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    const int F = H * C, Fv = F / VEC;
    for (int u0 = 0; u0 < Fv; u0 += R * kWave) {               // wave-uniform
        bool ok[R];
        int col[R], hh[R];
        float dot[R], acc[R][VEC], cmp[R][VEC];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int u = u0 + r * kWave + lane;
            ok[r] = u < Fv;
            col[r] = ok[r] ? u * VEC : 0;
            hh[r] = col[r] / C;
            dot[r] = 0.f;
#pragma unroll
            for (int c = 0; c < VEC; ++c) acc[r][c] = 0.f, cmp[r][c] = 0.f;
        }
        const int64_t c0 = (int64_t)u0 * VEC;
        const int64_t c1 = c0 + (int64_t)R * kWave * VEC < F ? c0 + (int64_t)R * kWave * VEC : F;
        const int h_first = (int)(c0 / C), h_last = (int)((c1 - 1) / C);
        for (int h = h_first; h <= h_last; ++h) {              // wave-uniform
            float d = 0.f, dc = 0.f;
            for (int p = beg + lane; p < end; p += kWave)
                kahan_add(d, dc, alpha[(int64_t)p * H + h] * galpha[(int64_t)p * H + h]);
            d = group_sum(d, kWave);
            if ((int64_t)h * C >= c0)                          // the head begins in this chunk: its gl is stored here
                for (int p = beg + lane; p < end; p += kWave)
                    gl[(int64_t)p * H + h] = tc_logit_grad(alpha[(int64_t)p * H + h], galpha[(int64_t)p * H + h], d, scale);
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (ok[r] && hh[r] == h) dot[r] = d;
        }
        for (int p = beg; p < end; p += U) {
            const int n = end - p;                             // wave-uniform
            int64_t s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = u < n ? other[p + u] : row;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                Cols<VEC> kv[U];
                float g[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool on = ok[r] && u < n;
                    kv[u] = cols_load<VEC>(k + s[u] * ldk + col[r], on);
                    const int64_t x = (int64_t)(p + u) * H + hh[r];
                    g[u] = on ? tc_logit_grad(alpha[x], galpha[x], dot[r], scale) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u < n) {                               // wave-uniform
#pragma unroll
                        for (int c = 0; c < VEC; ++c) kahan_add(acc[r][c], cmp[r][c], g[u] * kv[u].a[c]);
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (ok[r]) cols_store<VEC>(g_q + row * ldgq + col[r], acc[r]);
    }
}

// ---- backward, source side: over the transposed set -----------------------------------------------------------------------
// For source row j and the edges t out of j (to i = other[t]; p = to_fwd[t] its position in the destination-sorted
// order), in t order:  g_k[j,h,c] = sum gl[p,h] q[i,h,c],  g_v[j,h,c] = sum alpha[p,h] gm[i,h,c]  - both in ONE walk
// of the transposed segment: two gathered rows per edge, two compensated per-column sums, two stores per source row.
// One wave per source row, columns in chunks as k_tconv_dst_bwd.
template <int VEC>
__global__ void __launch_bounds__(256)
k_tconv_src_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const int32_t *__restrict__ to_fwd,
                const float *__restrict__ alpha, const float *__restrict__ gl, const float *__restrict__ q, int64_t ldq,
                const float *__restrict__ gm, int64_t ldgm, float *__restrict__ g_k, int64_t ldgk,
                float *__restrict__ g_v, int64_t ldgv, int64_t N, int H, int C) {
    constexpr int R = kRegUTc, U = kEdgesTc;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    const int F = H * C, Fv = F / VEC;
    for (int u0 = 0; u0 < Fv; u0 += R * kWave) {
        bool ok[R];
        int col[R], hh[R];
        float ak[R][VEC], ck[R][VEC], av[R][VEC], cv[R][VEC];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int u = u0 + r * kWave + lane;
            ok[r] = u < Fv;
            col[r] = ok[r] ? u * VEC : 0;
            hh[r] = col[r] / C;
#pragma unroll
            for (int c = 0; c < VEC; ++c) ak[r][c] = 0.f, ck[r][c] = 0.f, av[r][c] = 0.f, cv[r][c] = 0.f;
        }
        for (int p = beg; p < end; p += U) {
            const int n = end - p;                             // wave-uniform
            int64_t s[U], f[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = u < n ? other[p + u] : row;
                f[u] = u < n ? to_fwd[p + u] : 0;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                Cols<VEC> qv[U], gv[U];
                float a[U], g[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool on = ok[r] && u < n;
                    qv[u] = cols_load<VEC>(q + s[u] * ldq + col[r], on);
                    gv[u] = cols_load<VEC>(gm + s[u] * ldgm + col[r], on);
                    a[u] = on ? alpha[f[u] * H + hh[r]] : 0.f;
                    g[u] = on ? gl[f[u] * H + hh[r]] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u < n) {                               // wave-uniform
#pragma unroll
                        for (int c = 0; c < VEC; ++c) {
                            kahan_add(ak[r][c], ck[r][c], g[u] * qv[u].a[c]);
                            kahan_add(av[r][c], cv[r][c], a[u] * gv[u].a[c]);
                        }
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (ok[r]) {
                cols_store<VEC>(g_k + row * ldgk + col[r], ak[r]);
                cols_store<VEC>(g_v + row * ldgv + col[r], av[r]);
            }
    }
}

}  // namespace dc

using namespace dc;

#define DC_TCONV_SHAPE(name, N, H, C)                                                                              \
    DC_REQUIRE((N) >= 0 && (H) >= 1 && (C) >= 1, name ": need N >= 0, H >= 1, C >= 1 (N=%lld H=%lld C=%lld)",     \
               (long long)(N), (long long)(H), (long long)(C));                                                    \
    DC_REQUIRE(sizes_ok(N, H, C), name ": size out of range")

extern "C" int dc_tconv_softmax_fwd(const int32_t *ptr, const int32_t *other, const float *q, int64_t ldq,
                                    const float *k, int64_t ldk, float scale, float *alpha, int64_t N, int64_t H,
                                    int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_TCONV_SHAPE("dc_tconv_softmax_fwd", N, H, C);
    DC_REQUIRE(ldq >= H * C && ldk >= H * C, "dc_tconv_softmax_fwd: leading dimension smaller than H * C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && q && k && alpha, "dc_tconv_softmax_fwd: null pointer");
    const bool v4 = C % 4 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && al16(q) && al16(k);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (v4)
        DC_LAUNCH((k_tconv_softmax_fwd<4>), grid, dim3(256), 0, stream, ptr, other, q, ldq, k, ldk, scale, alpha, N,
                  (int)H, (int)C, lanes_per_head(C / 4));
    else
        DC_LAUNCH((k_tconv_softmax_fwd<1>), grid, dim3(256), 0, stream, ptr, other, q, ldq, k, ldk, scale, alpha, N,
                  (int)H, (int)C, lanes_per_head(C));
    return check_launch("dc_tconv_softmax_fwd");
}

extern "C" int dc_tconv_softmax_bwd(const int32_t *ptr, const int32_t *other, const float *alpha, const float *galpha,
                                    const float *k, int64_t ldk, float scale, float *gl, float *g_q, int64_t ldgq,
                                    int64_t N, int64_t H, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_TCONV_SHAPE("dc_tconv_softmax_bwd", N, H, C);
    DC_REQUIRE(ldk >= H * C && ldgq >= H * C, "dc_tconv_softmax_bwd: leading dimension smaller than H * C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && alpha && galpha && k && gl && g_q, "dc_tconv_softmax_bwd: null pointer");
    DC_REQUIRE(g_q != k && gl != alpha && gl != galpha, "dc_tconv_softmax_bwd: g_q / gl must not alias an input");
    const bool v4 = C % 4 == 0 && ldk % 4 == 0 && ldgq % 4 == 0 && al16(k) && al16(g_q);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (v4)
        DC_LAUNCH((k_tconv_dst_bwd<4>), grid, dim3(256), 0, stream, ptr, other, alpha, galpha, k, ldk, scale, gl, g_q,
                  ldgq, N, (int)H, (int)C);
    else
        DC_LAUNCH((k_tconv_dst_bwd<1>), grid, dim3(256), 0, stream, ptr, other, alpha, galpha, k, ldk, scale, gl, g_q,
                  ldgq, N, (int)H, (int)C);
    return check_launch("dc_tconv_softmax_bwd");
}

extern "C" int dc_tconv_source_bwd(const int32_t *ptr_t, const int32_t *other_t, const int32_t *to_fwd,
                                   const float *alpha, const float *gl, const float *q, int64_t ldq, const float *gm,
                                   int64_t ldgm, float *g_k, int64_t ldgk, float *g_v, int64_t ldgv, int64_t N,
                                   int64_t H, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_TCONV_SHAPE("dc_tconv_source_bwd", N, H, C);
    const int64_t F = H * C;
    DC_REQUIRE(ldq >= F && ldgm >= F && ldgk >= F && ldgv >= F,
               "dc_tconv_source_bwd: leading dimension smaller than H * C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr_t && other_t && to_fwd && alpha && gl && q && gm && g_k && g_v, "dc_tconv_source_bwd: null pointer");
    DC_REQUIRE(g_k != q && g_k != gm && g_v != q && g_v != gm && g_k != g_v,
               "dc_tconv_source_bwd: g_k / g_v must not alias q / gm or each other");
    const bool v4 = C % 4 == 0 && ldq % 4 == 0 && ldgm % 4 == 0 && ldgk % 4 == 0 && ldgv % 4 == 0 && al16(q) &&
                    al16(gm) && al16(g_k) && al16(g_v);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (v4)
        DC_LAUNCH((k_tconv_src_bwd<4>), grid, dim3(256), 0, stream, ptr_t, other_t, to_fwd, alpha, gl, q, ldq, gm, ldgm,
                  g_k, ldgk, g_v, ldgv, N, (int)H, (int)C);
    else
        DC_LAUNCH((k_tconv_src_bwd<1>), grid, dim3(256), 0, stream, ptr_t, other_t, to_fwd, alpha, gl, q, ldq, gm, ldgm,
                  g_k, ldgk, g_v, ldgv, N, (int)H, (int)C);
    return check_launch("dc_tconv_source_bwd");
}
