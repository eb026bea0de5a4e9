// dc_gatv2.hip -- GATv2Conv (PyG 2.5.2 gatv2_conv.py): the dynamic-attention score, its edge softmax and both sides of
// its backward on the sorted adjacency.
//
// With xl = lin_l(x), xr = lin_r(x) viewed as [N, H, C], for edge p from j into i, head k, channel c:
//   s[p,k,c] = xl[j,k,c] + xr[i,k,c]            e[p,k] = sum_c att[k,c] leaky_relu(s[p,k,c])
//   alpha[p,k] = softmax of e[.,k] over the edges into i (maximum subtracted, + 1e-16 in the denominator)
// GATConv's logit a_src[j] + a_dst[i] folds to one scalar per node and head (dc_gat_alpha_heads_fwd); this one is per
// edge, head AND channel - the non-linearity sits in front of the attention vector - so the score and its backward
// gather H*C floats per edge.  Per-edge vectors are EDGE-MAJOR [capacity, H] as in dc_gat_heads.hip, whose aggregation
// (dc_spmm_f32_heads_bias_act) and SDDMM (dc_sddmm_f32_heads) the layer uses unchanged.
//
// Rules of the segment kernels (the order-defining helpers: see dc_segment.h): destination-sorted segments, every sum
// in a fixed order, products and sums rounded separately, no float atomics, no host read - two runs give the same bits.
// The long sums (a segment's softmax
// denominator, the per-column sums over a segment's edges) are compensated (Kahan): a hub with thousands of edges
// costs no more digits than a short segment.  Any H >= 1, C >= 1 and in-degree, N = 0: no width cap - what a lane
// cannot hold in registers it reads again (forward) or works through in column chunks (backward).
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

__device__ __forceinline__ float v2_dlrelu(float v, float slope) { return v > 0.f ? 1.0f : slope; }

// acc += sum over the lane's channels of att * leaky_relu(xl + xr), channel order
__device__ __forceinline__ void v2_score(float &acc, float xl, float xr, float att, float slope) {
    const float m = att * lrelu(xl + xr, slope);
    acc = acc + m;
}
__device__ __forceinline__ void v2_score(float &acc, const float4 &xl, const float4 &xr, const float4 &att, float slope) {
    v2_score(acc, xl.x, xr.x, att.x, slope);
    v2_score(acc, xl.y, xr.y, att.y, slope);
    v2_score(acc, xl.z, xr.z, att.z, slope);
    v2_score(acc, xl.w, xr.w, att.w, slope);
}

}  // namespace

// ---- forward: score + edge softmax ---------------------------------------------------------------------------------------
// One wave per destination row.  A head is an aligned group of T lanes (T = the power of two >= C / VEC, at most 64);
// G = 64 / T heads make a pass, lane (grp, sub) owns the channel units sub, sub + T, ... of head k0 + grp.  Per pass the
// lane's part of xr[i] and of att sits in registers (the first kRegV2 units; a wider head reads the rest again), every
// xl[j] element is gathered once, U edges in flight; the head's sum over c: the lane's channels in order, then the
// fixed butterfly.  alpha holds the raw logits between the passes; the group's first lane, which wrote them, turns
// them into exp(e - max) and then into the weights - it reads back only what it wrote itself.
constexpr int kRegV2 = 4;
constexpr int kEdgesV2 = 4;

template <int VEC>
__global__ void __launch_bounds__(256)
k_gatv2_softmax_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ xl,
                    int64_t ldxl, const float *__restrict__ xr, int64_t ldxr, const float *__restrict__ att, float slope,
                    float *alpha, int64_t N, int H, int C, int T) {
    using V = typename Vec<VEC>::T;
    constexpr int U = kEdgesV2;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    const int Cv = C / VEC, G = kWave / T, J = (Cv + T - 1) / T;
    const int sub = lane & (T - 1), grp = lane / T;
    for (int k0 = 0; k0 < H; k0 += G) {
        const int k = k0 + grp;
        const bool hv = k < H;
        const int64_t hcol = (int64_t)k * C;
        V xrr[kRegV2], atr[kRegV2];
#pragma unroll
        for (int r = 0; r < kRegV2; ++r) {
            const int cu = sub + T * r;
            const bool ok = hv && cu < Cv;
            xrr[r] = vec_load<V>(xr + row * ldxr + hcol + cu * VEC, ok);
            atr[r] = vec_load<V>(att + hcol + cu * VEC, ok);
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
            for (int r = 0; r < kRegV2; ++r) {
                if (r < J) {                                   // wave-uniform
                    const int cu = sub + T * r;
                    const bool ok = hv && cu < Cv;
                    V v[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) v[u] = vec_load<V>(xl + s[u] * ldxl + hcol + cu * VEC, ok && u < n);
#pragma unroll
                    for (int u = 0; u < U; ++u) v2_score(acc[u], v[u], xrr[r], atr[r], slope);
                }
            }
            for (int r = kRegV2; r < J; ++r) {                 // heads wider than the registers hold: xr, att read again
                const int cu = sub + T * r;
                const bool ok = hv && cu < Cv;
                const V xv = vec_load<V>(xr + row * ldxr + hcol + cu * VEC, ok);
                const V av = vec_load<V>(att + hcol + cu * VEC, ok);
                V v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = vec_load<V>(xl + s[u] * ldxl + hcol + cu * VEC, ok && u < n);
#pragma unroll
                for (int u = 0; u < U; ++u) v2_score(acc[u], v[u], xv, av, slope);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {                                   // wave-uniform
                    const float e = group_sum(acc[u], T);
                    m = fmaxf(m, e);
                    if (hv && sub == 0) alpha[(int64_t)(p + u) * H + k] = e;
                }
        }
        if (hv && sub == 0) {
            float sum = 0.f, cmp = 0.f;
            for (int p = beg; p < end; ++p) {
                float *al = alpha + (int64_t)p * H + k;
                const float ex = expf(*al - m);
                *al = ex;
                kahan_add(sum, cmp, ex);
            }
            const float den = sum + 1e-16f;
            for (int p = beg; p < end; ++p) {
                float *al = alpha + (int64_t)p * H + k;
                *al = *al / den;
            }
        }
    }
}

// ---- backward, destination side ---------------------------------------------------------------------------------------------
// ge[p,k] = alpha[p,k] (galpha[p,k] - sum over the segment of alpha galpha): the gradient of the logit e[p,k].  Layout of
// k_gat_softmax_heads_bwd (dc_gat_heads.hip): kSubV2 lanes per segment, lane `sub` walks edges beg + sub, + kSubV2, ...
// with HB heads of each edge in registers.
constexpr int kSubV2 = 8;

template <int HB>
__global__ void __launch_bounds__(256)
k_gatv2_logit_grad(const int32_t *__restrict__ ptr, const float *__restrict__ alpha, const float *__restrict__ galpha,
                   float *__restrict__ ge, int64_t N, int H) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kSubV2;
    const int sub = threadIdx.x % kSubV2;
    const bool live = i < N;
    const int beg = live ? ptr[i] : 0, end = live ? ptr[i + 1] : 0;
    for (int k0 = 0; k0 < H; k0 += HB) {
        float dot[HB], cmp[HB];
#pragma unroll
        for (int b = 0; b < HB; ++b) dot[b] = 0.f, cmp[b] = 0.f;
        for (int p = beg + sub; p < end; p += kSubV2) {
            const float *al = alpha + (int64_t)p * H + k0, *ga = galpha + (int64_t)p * H + k0;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) kahan_add(dot[b], cmp[b], al[b] * ga[b]);
        }
#pragma unroll
        for (int b = 0; b < HB; ++b) dot[b] = sub_sum<kSubV2>(dot[b]);
        for (int p = beg + sub; p < end; p += kSubV2) {
            const float *al = alpha + (int64_t)p * H + k0, *ga = galpha + (int64_t)p * H + k0;
            float *o = ge + (int64_t)p * H + k0;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) o[b] = al[b] * (ga[b] - dot[b]);
        }
    }
}

// g_xr[i,k,c] = sum over the edges p into i of t[p,k,c],  t = ge[p,k] att[k,c] (s[p,k,c] > 0 ? 1 : slope), and the
// workgroup's row of partial sums of g_att[k,c] = sum_p ge[p,k] leaky_relu(s[p,k,c]).  Purely per column: lane l owns
// the column units u0 + l, u0 + 64 + l, ... of a chunk of kRegUV2 * 64 units (a unit = VEC columns of one head), chunk
// by chunk; wave w of workgroup b owns the rows b * kRowsV2 + w, + 4, ...: a row of g_xr is summed by one lane per
// column in p order, and the lane's g_att sums run over its rows in order.  The four waves' sums are added in wave
// order through LDS: one row of the workspace per workgroup, added in index order by k_gatv2_colsum.
constexpr int kRegUV2 = 2;
constexpr int kRowsV2 = DC_GATV2_ROWS;

template <int VEC>
__global__ void __launch_bounds__(256)
k_gatv2_dst_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ ge,
                const float *__restrict__ xl, int64_t ldxl, const float *__restrict__ xr, int64_t ldxr,
                const float *__restrict__ att, float slope, float *__restrict__ g_xr, int64_t ldg,
                float *__restrict__ partial, int64_t N, int H, int C) {
    constexpr int R = kRegUV2, U = kEdgesV2;
    __shared__ float red[4][R * kWave * VEC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = (int64_t)blockIdx.x * kRowsV2;
    const int64_t r1 = r0 + kRowsV2 < N ? r0 + kRowsV2 : N;
    const int F = H * C, Fv = F / VEC;
    for (int u0 = 0; u0 < Fv; u0 += R * kWave) {               // uniform over the workgroup
        bool ok[R];
        int col[R], kk[R];
        Cols<VEC> av[R];
        float ga[R][VEC], gc[R][VEC];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int u = u0 + r * kWave + lane;
            ok[r] = u < Fv;
            col[r] = ok[r] ? u * VEC : 0;
            kk[r] = col[r] / C;
            av[r] = cols_load<VEC>(att + col[r], ok[r]);
#pragma unroll
            for (int q = 0; q < VEC; ++q) ga[r][q] = 0.f, gc[r][q] = 0.f;
        }
        for (int64_t row = r0 + wave; row < r1; row += 4) {
            const int beg = ptr[row], end = ptr[row + 1];
            Cols<VEC> xv[R];
            float acc[R][VEC], cmp[R][VEC];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                xv[r] = cols_load<VEC>(xr + row * ldxr + col[r], ok[r]);
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[r][q] = 0.f, cmp[r][q] = 0.f;
            }
            for (int p = beg; p < end; p += U) {
                const int n = end - p;                         // wave-uniform
                int64_t s[U];
#pragma unroll
                for (int u = 0; u < U; ++u) s[u] = u < n ? other[p + u] : row;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    Cols<VEC> v[U];
                    float g[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const bool on = ok[r] && u < n;
                        v[u] = cols_load<VEC>(xl + s[u] * ldxl + col[r], on);
                        g[u] = on ? ge[(int64_t)(p + u) * H + kk[r]] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (u < n) {                           // wave-uniform
#pragma unroll
                            for (int q = 0; q < VEC; ++q) {
                                const float sv = v[u].a[q] + xv[r].a[q];
                                const float ga_t = g[u] * av[r].a[q];
                                kahan_add(acc[r][q], cmp[r][q], ga_t * v2_dlrelu(sv, slope));
                                kahan_add(ga[r][q], gc[r][q], g[u] * lrelu(sv, slope));
                            }
                        }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (ok[r]) cols_store<VEC>(g_xr + row * ldg + col[r], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < VEC; ++q) red[wave][(r * kWave + lane) * VEC + q] = ga[r][q];
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (ok[r]) {
                    float t[VEC];
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        const int x = (r * kWave + lane) * VEC + q;
                        t[q] = ((red[0][x] + red[1][x]) + red[2][x]) + red[3][x];
                    }
                    cols_store<VEC>(partial + (int64_t)blockIdx.x * F + col[r], t);
                }
        }
        __syncthreads();
    }
}

// out[c] (+)= the rows of partial[nblocks, F] in a fixed order: lane l adds rows l, l + 64, ... in index order, then the
// fixed butterfly (k_colsum_final_heads of dc_gat_heads.hip; any F)
__global__ void __launch_bounds__(256)
k_gatv2_colsum(const float *__restrict__ partial, int64_t nblocks, int F, float *out, int accumulate) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= F) return;
    float s = 0.f;
    for (int64_t b = lane; b < nblocks; b += kWave) s = s + partial[b * F + c];
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) s = s + __shfl_xor(s, q, kWave);
    if (lane == 0) out[c] = accumulate ? out[c] + s : s;
}

// ---- backward, source side: over the transposed set -----------------------------------------------------------------------
// g_xl[j,k,c] = sum over the edges q out of j (to i = other[q]; p = to_fwd[q] its position in the destination-sorted
// order) of alpha[p,k] gm[i,k,c] + t[p,k,c]: both terms in ONE walk of the transposed segment, which gathers gm[i] and
// xr[i] once each; xl[j] and att sit in registers.  One wave per source row, columns in chunks as k_gatv2_dst_bwd; sum
// in q order.
template <int VEC>
__global__ void __launch_bounds__(256)
k_gatv2_src_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const int32_t *__restrict__ to_fwd,
                const float *__restrict__ alpha, const float *__restrict__ ge, const float *__restrict__ gm, int64_t ldgm,
                const float *__restrict__ xl, int64_t ldxl, const float *__restrict__ xr, int64_t ldxr,
                const float *__restrict__ att, float slope, float *__restrict__ g_xl, int64_t ldg, int64_t N, int H,
                int C) {
    constexpr int R = kRegUV2, U = kEdgesV2;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    const int F = H * C, Fv = F / VEC;
    for (int u0 = 0; u0 < Fv; u0 += R * kWave) {
        bool ok[R];
        int col[R], kk[R];
        Cols<VEC> av[R], xv[R];
        float acc[R][VEC], cmp[R][VEC];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int u = u0 + r * kWave + lane;
            ok[r] = u < Fv;
            col[r] = ok[r] ? u * VEC : 0;
            kk[r] = col[r] / C;
            av[r] = cols_load<VEC>(att + col[r], ok[r]);
            xv[r] = cols_load<VEC>(xl + row * ldxl + col[r], ok[r]);
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[r][q] = 0.f, cmp[r][q] = 0.f;
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
                Cols<VEC> g[U], v[U];
                float a[U], e[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool on = ok[r] && u < n;
                    g[u] = cols_load<VEC>(gm + s[u] * ldgm + col[r], on);
                    v[u] = cols_load<VEC>(xr + s[u] * ldxr + col[r], on);
                    a[u] = on ? alpha[f[u] * H + kk[r]] : 0.f;
                    e[u] = on ? ge[f[u] * H + kk[r]] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u < n) {                               // wave-uniform
#pragma unroll
                        for (int q = 0; q < VEC; ++q) {
                            const float sv = xv[r].a[q] + v[u].a[q];
                            const float m = a[u] * g[u].a[q];
                            const float ea = e[u] * av[r].a[q];
                            const float t = ea * v2_dlrelu(sv, slope);
                            kahan_add(acc[r][q], cmp[r][q], m + t);
                        }
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (ok[r]) cols_store<VEC>(g_xl + row * ldg + col[r], acc[r]);
    }
}

}  // namespace dc

using namespace dc;

#define DC_GATV2_SHAPE(name, N, H, C)                                                                              \
    DC_REQUIRE((N) >= 0 && (H) >= 1 && (C) >= 1, name ": need N >= 0, H >= 1, C >= 1 (N=%lld H=%lld C=%lld)",     \
               (long long)(N), (long long)(H), (long long)(C));                                                    \
    DC_REQUIRE(sizes_ok(N, H, C), name ": size out of range")

extern "C" int dc_gatv2_softmax_fwd(const int32_t *ptr, const int32_t *other, const float *xl, int64_t ldxl,
                                    const float *xr, int64_t ldxr, const float *att, float slope, float *alpha, int64_t N,
                                    int64_t H, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GATV2_SHAPE("dc_gatv2_softmax_fwd", N, H, C);
    DC_REQUIRE(ldxl >= H * C && ldxr >= H * C, "dc_gatv2_softmax_fwd: leading dimension smaller than H * C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && xl && xr && att && alpha, "dc_gatv2_softmax_fwd: null pointer");
    const bool v4 = C % 4 == 0 && ldxl % 4 == 0 && ldxr % 4 == 0 && al16(xl) && al16(xr) && al16(att);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (v4)
        DC_LAUNCH((k_gatv2_softmax_fwd<4>), grid, dim3(256), 0, stream, ptr, other, xl, ldxl, xr, ldxr, att, slope, alpha,
                  N, (int)H, (int)C, lanes_per_head(C / 4));
    else
        DC_LAUNCH((k_gatv2_softmax_fwd<1>), grid, dim3(256), 0, stream, ptr, other, xl, ldxl, xr, ldxr, att, slope, alpha,
                  N, (int)H, (int)C, lanes_per_head(C));
    return check_launch("dc_gatv2_softmax_fwd");
}

extern "C" int64_t dc_gatv2_workspace_bytes(int64_t N, int64_t H, int64_t C) {
    if (N < 0 || H < 1 || C < 1 || !sizes_ok(N, H, C)) return -1;
    return (N + kRowsV2 - 1) / kRowsV2 * H * C * (int64_t)sizeof(float);
}

extern "C" int dc_gatv2_softmax_bwd(const int32_t *ptr, const int32_t *other, const float *alpha, const float *galpha,
                                    const float *xl, int64_t ldxl, const float *xr, int64_t ldxr, const float *att,
                                    float slope, float *ge, float *g_xr, int64_t ldg, float *g_att, int accumulate,
                                    void *workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t C,
                                    dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GATV2_SHAPE("dc_gatv2_softmax_bwd", N, H, C);
    const int64_t F = H * C;
    DC_REQUIRE(ldxl >= F && ldxr >= F && ldg >= F, "dc_gatv2_softmax_bwd: leading dimension smaller than H * C");
    DC_REQUIRE(att && g_att, "dc_gatv2_softmax_bwd: null pointer");
    const int64_t nb = (N + kRowsV2 - 1) / kRowsV2;
    DC_REQUIRE(workspace_bytes >= nb * F * (int64_t)sizeof(float) && (workspace || nb == 0),
               "dc_gatv2_softmax_bwd: workspace smaller than dc_gatv2_workspace_bytes(N, H, C)");
    if (N > 0) {
        DC_REQUIRE(ptr && other && alpha && galpha && xl && xr && ge && g_xr, "dc_gatv2_softmax_bwd: null pointer");
        DC_REQUIRE(g_xr != xl && g_xr != xr, "dc_gatv2_softmax_bwd: g_xr must not alias xl / xr");
        const dim3 grid_e((unsigned)((N * kSubV2 + 255) / 256));
        if (H == 1) DC_LAUNCH((k_gatv2_logit_grad<1>), grid_e, dim3(256), 0, stream, ptr, alpha, galpha, ge, N, (int)H);
        else if (H == 2) DC_LAUNCH((k_gatv2_logit_grad<2>), grid_e, dim3(256), 0, stream, ptr, alpha, galpha, ge, N, (int)H);
        else if (H <= 4) DC_LAUNCH((k_gatv2_logit_grad<4>), grid_e, dim3(256), 0, stream, ptr, alpha, galpha, ge, N, (int)H);
        else DC_LAUNCH((k_gatv2_logit_grad<8>), grid_e, dim3(256), 0, stream, ptr, alpha, galpha, ge, N, (int)H);
        const bool v4 = C % 4 == 0 && ldxl % 4 == 0 && ldxr % 4 == 0 && ldg % 4 == 0 && al16(xl) && al16(xr) &&
                        al16(att) && al16(g_xr) && al16(workspace);
        if (v4)
            DC_LAUNCH((k_gatv2_dst_bwd<4>), dim3((unsigned)nb), dim3(256), 0, stream, ptr, other, ge, xl, ldxl, xr, ldxr,
                      att, slope, g_xr, ldg, (float *)workspace, N, (int)H, (int)C);
        else
            DC_LAUNCH((k_gatv2_dst_bwd<1>), dim3((unsigned)nb), dim3(256), 0, stream, ptr, other, ge, xl, ldxl, xr, ldxr,
                      att, slope, g_xr, ldg, (float *)workspace, N, (int)H, (int)C);
    }
    DC_LAUNCH(k_gatv2_colsum, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, stream, (const float *)workspace, nb, (int)F,
              g_att, accumulate);
    return check_launch("dc_gatv2_softmax_bwd");
}

extern "C" int dc_gatv2_source_bwd(const int32_t *ptr_t, const int32_t *other_t, const int32_t *to_fwd,
                                   const float *alpha, const float *ge, const float *gm, int64_t ldgm, const float *xl,
                                   int64_t ldxl, const float *xr, int64_t ldxr, const float *att, float slope,
                                   float *g_xl, int64_t ldg, int64_t N, int64_t H, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GATV2_SHAPE("dc_gatv2_source_bwd", N, H, C);
    const int64_t F = H * C;
    DC_REQUIRE(ldgm >= F && ldxl >= F && ldxr >= F && ldg >= F,
               "dc_gatv2_source_bwd: leading dimension smaller than H * C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr_t && other_t && to_fwd && alpha && ge && gm && xl && xr && att && g_xl,
               "dc_gatv2_source_bwd: null pointer");
    DC_REQUIRE(g_xl != xl && g_xl != xr && g_xl != gm, "dc_gatv2_source_bwd: g_xl must not alias xl / xr / gm");
    const bool v4 = C % 4 == 0 && ldgm % 4 == 0 && ldxl % 4 == 0 && ldxr % 4 == 0 && ldg % 4 == 0 && al16(gm) &&
                    al16(xl) && al16(xr) && al16(att) && al16(g_xl);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (v4)
        DC_LAUNCH((k_gatv2_src_bwd<4>), grid, dim3(256), 0, stream, ptr_t, other_t, to_fwd, alpha, ge, gm, ldgm, xl, ldxl, xr,
                  ldxr, att, slope, g_xl, ldg, N, (int)H, (int)C);
    else
        DC_LAUNCH((k_gatv2_src_bwd<1>), grid, dim3(256), 0, stream, ptr_t, other_t, to_fwd, alpha, ge, gm, ldgm, xl, ldxl, xr,
                  ldxr, att, slope, g_xl, ldg, N, (int)H, (int)C);
    return check_launch("dc_gatv2_source_bwd");
}
