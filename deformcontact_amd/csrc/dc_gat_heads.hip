// dc_gat_heads.hip -- GATConv with several attention heads (heads > 1; concat or mean) on the sorted adjacency.
//
// PyG 2.5.2 gat_conv.py with h = lin(x) viewed as [N, H, C]: per head k the two attention dot products, the edge softmax
// over the incoming edges of i (utils/_softmax.py) and out[i, k, :] = sum_p alpha[p, k] h[other[p], k, :].  The heads = 1
// kernels (dc_gat.hip, dc_gnn_epi.hip, dc_spmm_f32_bias_act) carry ONE scalar per edge; these carry H of them, stored
// EDGE-MAJOR ([capacity, H] in destination-sorted order, [N, H] per node): the H weights of an edge sit together, so one
// read of other[p] and one of the segment bounds serve every head and every neighbour row of H*C floats is gathered
// once.  Same rules as the single-head kernels: destination-sorted segments, sums in p order, products and sums rounded
// separately, no float atomics - two runs give the same bits.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

// kSubH lanes per destination segment, as k_gat_softmax_fwd (dc_gat.hip): lane `sub` walks edges beg + sub,
// beg + sub + kSubH, ... and carries HB heads of each edge in registers - one walk of the segment (one read of
// other[p]) per pass serves HB heads; H > HB repeats the walk per block of heads.  Per head the arithmetic is that of
// the single-head kernel, in the same order.
constexpr int kSubH = 8;

// EDGE (GATConv(edge_dim=...), dc_gat_edge.hip): the logit carries a third, per-edge addend a_edge[p, k] - added to the
// finished a_src + a_dst, so an a_edge of zeros leaves every bit as it is; EDGE = false is the code without the operand.
template <bool EDGE>
__device__ __forceinline__ float logit_h(float as, float ad, const float *__restrict__ ae, int b) {
    const float s = as + ad;
    if constexpr (EDGE) return s + ae[b];
    else return s;
}

template <int HB, bool EDGE = false>
__global__ void __launch_bounds__(256)
k_gat_softmax_heads_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other,
                        const float *__restrict__ a_src, const float *__restrict__ a_dst, float slope,
                        float *__restrict__ alpha, int64_t N, int H, const float *__restrict__ a_edge) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kSubH;
    const int sub = threadIdx.x % kSubH;
    const bool live = i < N;
    const int beg = live ? ptr[i] : 0, end = live ? ptr[i + 1] : 0;
    for (int k0 = 0; k0 < H; k0 += HB) {
        float ad[HB], m[HB], s[HB];
#pragma unroll
        for (int b = 0; b < HB; ++b) {
            ad[b] = (live && k0 + b < H) ? a_dst[i * H + k0 + b] : 0.f;
            m[b] = -INFINITY;
            s[b] = 0.f;
        }
        for (int p = beg + sub; p < end; p += kSubH) {
            const float *as = a_src + (int64_t)other[p] * H + k0;
            const float *ae = EDGE ? a_edge + (int64_t)p * H + k0 : nullptr;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) m[b] = fmaxf(m[b], lrelu(logit_h<EDGE>(as[b], ad[b], ae, b), slope));
        }
#pragma unroll
        for (int b = 0; b < HB; ++b) m[b] = sub_max<kSubH>(m[b]);
        for (int p = beg + sub; p < end; p += kSubH) {
            const float *as = a_src + (int64_t)other[p] * H + k0;
            const float *ae = EDGE ? a_edge + (int64_t)p * H + k0 : nullptr;
            float *al = alpha + (int64_t)p * H + k0;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) {
                    const float ex = expf(lrelu(logit_h<EDGE>(as[b], ad[b], ae, b), slope) - m[b]);
                    al[b] = ex;
                    s[b] += ex;
                }
        }
#pragma unroll
        for (int b = 0; b < HB; ++b) s[b] = sub_sum<kSubH>(s[b]) + 1e-16f;
        for (int p = beg + sub; p < end; p += kSubH) {          // own elements only
            float *al = alpha + (int64_t)p * H + k0;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) al[b] = al[b] / s[b];
        }
    }
}

template <int HB, bool EDGE = false>
__global__ void __launch_bounds__(256)
k_gat_softmax_heads_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other,
                        const float *__restrict__ a_src, const float *__restrict__ a_dst, float slope,
                        const float *__restrict__ alpha, const float *__restrict__ galpha,
                        float *__restrict__ ge, float *__restrict__ g_a_dst, int64_t N, int H,
                        const float *__restrict__ a_edge) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kSubH;
    const int sub = threadIdx.x % kSubH;
    const bool live = i < N;
    const int beg = live ? ptr[i] : 0, end = live ? ptr[i + 1] : 0;
    for (int k0 = 0; k0 < H; k0 += HB) {
        float ad[HB], dot[HB], acc[HB];
#pragma unroll
        for (int b = 0; b < HB; ++b) {
            ad[b] = (live && k0 + b < H) ? a_dst[i * H + k0 + b] : 0.f;
            dot[b] = 0.f;
            acc[b] = 0.f;
        }
        for (int p = beg + sub; p < end; p += kSubH) {
            const float *al = alpha + (int64_t)p * H + k0, *ga = galpha + (int64_t)p * H + k0;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) dot[b] += al[b] * ga[b];
        }
#pragma unroll
        for (int b = 0; b < HB; ++b) dot[b] = sub_sum<kSubH>(dot[b]);
        for (int p = beg + sub; p < end; p += kSubH) {
            const float *as = a_src + (int64_t)other[p] * H + k0;
            const float *al = alpha + (int64_t)p * H + k0, *ga = galpha + (int64_t)p * H + k0;
            const float *ae = EDGE ? a_edge + (int64_t)p * H + k0 : nullptr;
            float *o = ge + (int64_t)p * H + k0;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) {
                    const float s = logit_h<EDGE>(as[b], ad[b], ae, b);
                    const float g = al[b] * (ga[b] - dot[b]) * (s > 0.f ? 1.0f : slope);
                    o[b] = g;
                    acc[b] += g;
                }
        }
#pragma unroll
        for (int b = 0; b < HB; ++b) {
            acc[b] = sub_sum<kSubH>(acc[b]);
            if (live && sub == 0 && k0 + b < H) g_a_dst[i * H + k0 + b] = acc[b];
        }
    }
}

// ---- the aggregation: one wave per destination row, as k_spmm_wave (dc_spmm.hip) --------------------------------------
__device__ __forceinline__ void haxpy(float &acc, float w, float v) {
    const float m = w * v;
    acc = acc + m;
}
__device__ __forceinline__ void haxpy(float4 &acc, float w, const float4 &v) {
    const float mx = w * v.x, my = w * v.y, mz = w * v.z, mw = w * v.w;
    acc.x = acc.x + mx, acc.y = acc.y + my, acc.z = acc.z + mz, acc.w = acc.w + mw;
}
__device__ __forceinline__ void hadd(float &a, float b) { a = a + b; }
__device__ __forceinline__ void hadd(float4 &a, const float4 &b) { a.x = a.x + b.x, a.y = a.y + b.y, a.z = a.z + b.z, a.w = a.w + b.w; }
__device__ __forceinline__ void hdiv(float &a, float d) { a = a / d; }
__device__ __forceinline__ void hdiv(float4 &a, float d) { a.x = a.x / d, a.y = a.y / d, a.z = a.z / d, a.w = a.w / d; }
__device__ __forceinline__ void hrelu(float &a) { a = relu_keep_nan(a); }
__device__ __forceinline__ void hrelu(float4 &a) { a.x = relu_keep_nan(a.x), a.y = relu_keep_nan(a.y), a.z = relu_keep_nan(a.z), a.w = relu_keep_nan(a.w); }

// y[row, c] = act(sum_p alpha[p, c / C] x[other[p], c] + bias[c]) over the H*C columns (MEAN: the C columns of
// (1/H) sum_k sum_p alpha[p, k] x[other[p], k C + c]).  The row index, segment bounds and neighbour ids are
// wave-uniform (scalar loads); a lane's weight is that of the head its columns belong to - with VEC = 4 (C % 4 == 0) a
// lane's four columns never straddle two heads.  U neighbour rows in flight; every element of a neighbour row is
// loaded once.  Sum in p order from zero, bias added to the finished sum: with H = 1 the bits of dc_spmm_f32_bias_act.
template <int VEC, int U, bool MEAN>
__global__ void __launch_bounds__(256)
k_spmm_heads(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ alpha,
             const float *__restrict__ x, int64_t ldx, const float *__restrict__ bias, int relu, float *y,
             int64_t ldy, int64_t N, int H, int C) {
    using V = typename Vec<VEC>::T;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    const int fout = MEAN ? C : H * C;
    for (int c = lane * VEC; c < fout; c += kWave * VEC) {
        V tot = vec_zero(V{});
        const int k0 = MEAN ? 0 : c / C, k1 = MEAN ? H : k0 + 1;
        for (int k = k0; k < k1; ++k) {
            const int col = MEAN ? k * C + c : c;
            V acc = vec_zero(V{});
            for (int p = beg; p < end; p += U) {
                const int n = end - p;   // wave-uniform
                int s[U];
                float ww[U];
                V v[U];
#pragma unroll
                for (int j = 0; j < U; ++j)
                    if (j < n) {
                        s[j] = other[p + j];
                        ww[j] = alpha[(int64_t)(p + j) * H + k];
                    }
#pragma unroll
                for (int j = 0; j < U; ++j)
                    if (j < n) v[j] = *reinterpret_cast<const V *>(x + (int64_t)s[j] * ldx + col);
#pragma unroll
                for (int j = 0; j < U; ++j)
                    if (j < n) haxpy(acc, ww[j], v[j]);
            }
            if (MEAN) hadd(tot, acc);
            else tot = acc;
        }
        if (MEAN) hdiv(tot, (float)H);
        if (bias) hadd(tot, *reinterpret_cast<const V *>(bias + c));
        if (relu) hrelu(tot);
        *reinterpret_cast<V *>(y + row * ldy + c) = tot;
    }
}

// ---- SDDMM: d[p, k] = <g[i, kC:(k+1)C], h[other[p], kC:(k+1)C]> ------------------------------------------------------
// 16-byte form (C % 4 == 0, T = C / 4 a power of two <= 64): one wave per destination row, lane l owns the columns
// 4 l + 256 j; a head is an aligned group of T lanes of one 256-column chunk, reduced with a fixed butterfly.  The row of
// g is held in registers (the first kGRegsH chunks; wider rows re-read it), U neighbour rows are in flight and each is
// read once for all heads.
constexpr int kGRegsH = 2;

template <int U>
__device__ __forceinline__ void sddmm_chunk(const float4 gv, int c0, int F, int T, int H, int C, const int (&s)[U], int n,
                                            int p, const float *__restrict__ h, int64_t ldh, float *__restrict__ d,
                                            int lane) {
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        acc[u] = 0.f;
        if (u < n && c0 < F) {
            const float4 hv = *reinterpret_cast<const float4 *>(h + (int64_t)s[u] * ldh + c0);
            acc[u] = gv.x * hv.x + gv.y * hv.y + gv.z * hv.z + gv.w * hv.w;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (u < n) {                                           // wave-uniform
            const float t = group_sum(acc[u], T);
            if (c0 < F && (lane & (T - 1)) == 0) d[(int64_t)(p + u) * H + c0 / C] = t;
        }
}

template <int U>
__global__ void __launch_bounds__(256)
k_sddmm_heads_v4(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ g,
                 int64_t ldg, const float *__restrict__ h, int64_t ldh, float *__restrict__ d, int64_t N, int H, int C) {
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    const int F = H * C, T = C / 4;
    float4 gr[kGRegsH];
#pragma unroll
    for (int j = 0; j < kGRegsH; ++j) {
        const int c0 = (j * kWave + lane) * 4;
        gr[j] = c0 < F ? *reinterpret_cast<const float4 *>(g + row * ldg + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int p = beg; p < end; p += U) {
        const int n = end - p;
        int s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = u < n ? other[p + u] : 0;
#pragma unroll
        for (int j = 0; j < kGRegsH; ++j)
            if (j * kWave * 4 < F) sddmm_chunk<U>(gr[j], (j * kWave + lane) * 4, F, T, H, C, s, n, p, h, ldh, d, lane);
        for (int j = kGRegsH; j * kWave * 4 < F; ++j) {
            const int c0 = (j * kWave + lane) * 4;
            const float4 gv = c0 < F ? *reinterpret_cast<const float4 *>(g + row * ldg + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
            sddmm_chunk<U>(gv, c0, F, T, H, C, s, n, p, h, ldh, d, lane);
        }
    }
}

// any H, C, alignment: per edge and head the lanes stride the head's C columns, one wave reduction each
__global__ void __launch_bounds__(256)
k_sddmm_heads_any(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ g,
                  int64_t ldg, const float *__restrict__ h, int64_t ldh, float *__restrict__ d, int64_t N, int H, int C) {
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row = __builtin_amdgcn_readfirstlane((int)(lb * 4u + (threadIdx.x >> 6)));
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int beg = ptr[row], end = ptr[row + 1];
    for (int p = beg; p < end; ++p) {
        const int64_t s = other[p];
        for (int k = 0; k < H; ++k) {
            float acc = 0.f;
            for (int c = lane; c < C; c += kWave) acc += g[row * ldg + k * C + c] * h[s * ldh + k * C + c];
            acc = wave_sum(acc);
            if (lane == 0) d[(int64_t)p * H + k] = acc;
        }
    }
}

// ---- per-edge / per-node vectors of width W -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_segment_sum_heads(const int32_t *__restrict__ ptr, const int32_t *__restrict__ map, const float *__restrict__ v,
                    float *__restrict__ out, int64_t N, int W) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * W) return;
    const int64_t i = t / W;
    const int k = (int)(t % W);
    float acc = 0.f;
    for (int p = ptr[i], end = ptr[i + 1]; p < end; ++p) acc += v[(int64_t)(map ? map[p] : p) * W + k];
    out[t] = acc;
}

__global__ void __launch_bounds__(256)
k_gather_heads(const float *__restrict__ v, const int32_t *__restrict__ idx, float *__restrict__ out,
               const int32_t *n_ptr, int64_t cap, int W) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = t / W;
    if (p < cap && p < *n_ptr) out[t] = v[(int64_t)idx[p] * W + t % W];
}

// out[i, k C + c] = g[i, c] / H : the gradient of the mean over heads (concat = False), spread to every head
__global__ void __launch_bounds__(256)
k_spread_heads(const float *__restrict__ g, int64_t ldg, float *__restrict__ out, int64_t ldo, int64_t N, int H, int C) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t F = (int64_t)H * C;
    if (t >= N * F) return;
    const int64_t i = t / F;
    const int c = (int)(t % F);
    out[i * ldo + c] = g[i * ldg + c % C] / (float)H;
}

// ---- the attention dot products for all heads ------------------------------------------------------------------------------
// 16-byte form (as k_sddmm_heads_v4: a head is an aligned group of T = C / 4 lanes): one wave per row, one pass over h
__global__ void __launch_bounds__(256)
k_gat_alpha_heads_fwd_v4(const float *__restrict__ h, int64_t ldh, const float *__restrict__ att_src,
                         const float *__restrict__ att_dst, float *a_src, float *a_dst, int64_t N, int H, int C) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const int F = H * C, T = C / 4;
    for (int base = 0; base < F; base += 4 * kWave) {
        const int c = base + 4 * lane;
        float s = 0.f, d = 0.f;
        if (c < F) {
            const float4 v = *reinterpret_cast<const float4 *>(h + row * ldh + c);
            const float4 as = *reinterpret_cast<const float4 *>(att_src + c), ad = *reinterpret_cast<const float4 *>(att_dst + c);
            s = v.x * as.x + v.y * as.y + v.z * as.z + v.w * as.w;
            d = v.x * ad.x + v.y * ad.y + v.z * ad.z + v.w * ad.w;
        }
        s = group_sum(s, T);
        d = group_sum(d, T);
        if (c < F && (lane & (T - 1)) == 0) a_src[row * H + c / C] = s, a_dst[row * H + c / C] = d;
    }
}

__global__ void __launch_bounds__(256)
k_gat_alpha_heads_fwd_any(const float *__restrict__ h, int64_t ldh, const float *__restrict__ att_src,
                          const float *__restrict__ att_dst, float *a_src, float *a_dst, int64_t N, int H, int C) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    for (int k = 0; k < H; ++k) {
        float s = 0.f, d = 0.f;
        for (int c = k * C + lane; c < (k + 1) * C; c += kWave) {
            const float v = h[row * ldh + c];
            s += v * att_src[c];
            d += v * att_dst[c];
        }
        s = wave_sum(s);
        d = wave_sum(d);
        if (lane == 0) a_src[row * H + k] = s, a_dst[row * H + k] = d;
    }
}

constexpr int kEpiRowsH = 32;                       // rows per block of the column-sum pass (dc_gnn_epi.hip: kEpiRows)

// backward of the dot products, k_gat_alpha_bwd (dc_gnn_epi.hip) with one (ga_src, ga_dst) pair per head: thread t owns
// 4 columns, each with the head it belongs to (C % 4 != 0: the four may belong to different heads)
//   gh[i, c] += ga_src[i, c / C] att_src[c] + ga_dst[i, c / C] att_dst[c]
//   partial[block][0:F] = sum_i ga_src[i, c / C] h[i, c],  partial[block][F:2F] likewise with ga_dst
__global__ void __launch_bounds__(256)
k_gat_alpha_heads_bwd(const float *__restrict__ h, int64_t ldh, const float *__restrict__ ga_src,
                      const float *__restrict__ ga_dst, const float *__restrict__ att_src,
                      const float *__restrict__ att_dst, float *gh, int64_t ldgh, int64_t N, int H, int C,
                      float *__restrict__ partial) {
    __shared__ float red[256 * 8];
    const int F = H * C;
    const int tpr = F / 4, groups = 256 / tpr;
    const int gidx = threadIdx.x / tpr, c = 4 * (threadIdx.x % tpr);
    const int64_t r0 = (int64_t)blockIdx.x * kEpiRowsH;
    float ss[4] = {0.f, 0.f, 0.f, 0.f}, sd[4] = {0.f, 0.f, 0.f, 0.f};
    if (gidx < groups) {
        const float4 as4 = *reinterpret_cast<const float4 *>(att_src + c), ad4 = *reinterpret_cast<const float4 *>(att_dst + c);
        const float as[4] = {as4.x, as4.y, as4.z, as4.w}, ad[4] = {ad4.x, ad4.y, ad4.z, ad4.w};
        const int kk[4] = {c / C, (c + 1) / C, (c + 2) / C, (c + 3) / C};
        for (int64_t r = r0 + gidx; r < r0 + kEpiRowsH && r < N; r += groups) {
            const float4 v4 = *reinterpret_cast<const float4 *>(h + r * ldh + c);
            const float4 o4 = *reinterpret_cast<const float4 *>(gh + r * ldgh + c);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            float o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float gs = ga_src[r * H + kk[q]], gd = ga_dst[r * H + kk[q]];
                o[q] += gs * as[q] + gd * ad[q];
                ss[q] += gs * v[q];
                sd[q] += gd * v[q];
            }
            *reinterpret_cast<float4 *>(gh + r * ldgh + c) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    *reinterpret_cast<float4 *>(&red[8 * threadIdx.x]) = make_float4(ss[0], ss[1], ss[2], ss[3]);
    *reinterpret_cast<float4 *>(&red[8 * threadIdx.x + 4]) = make_float4(sd[0], sd[1], sd[2], sd[3]);
    __syncthreads();
    if (threadIdx.x < tpr) {                               // the row groups of a column quad, in group order
        float4 ts = make_float4(0.f, 0.f, 0.f, 0.f), td = ts;
        for (int q = 0; q < groups; ++q) {
            const float4 a = *reinterpret_cast<const float4 *>(&red[8 * (q * tpr + threadIdx.x)]);
            const float4 b = *reinterpret_cast<const float4 *>(&red[8 * (q * tpr + threadIdx.x) + 4]);
            ts.x += a.x, ts.y += a.y, ts.z += a.z, ts.w += a.w;
            td.x += b.x, td.y += b.y, td.z += b.z, td.w += b.w;
        }
        *reinterpret_cast<float4 *>(partial + (int64_t)blockIdx.x * 2 * F + c) = ts;
        *reinterpret_cast<float4 *>(partial + (int64_t)blockIdx.x * 2 * F + F + c) = td;
    }
}

// out[c] (+)= sum over blocks of partial[b * stride + c], the blocks in a fixed order (k_colsum_final of dc_gnn_epi.hip)
__global__ void __launch_bounds__(256)
k_colsum_final_heads(const float *__restrict__ partial, int64_t nblocks, int64_t stride, int F, float *out, int accumulate) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= F) return;
    float s = 0.f;
    for (int64_t b = lane; b < nblocks; b += 64) s = s + partial[b * stride + c];
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) s = s + __shfl_xor(s, q);
    if (lane == 0) out[c] = accumulate ? out[c] + s : s;
}

static inline bool h_pow2(int64_t v) { return v >= 1 && (v & (v - 1)) == 0; }
// C % 4 == 0 and a head = an aligned group of C / 4 <= 64 lanes
static inline bool h_group_ok(int64_t C) { return C % 4 == 0 && h_pow2(C / 4) && C / 4 <= kWave; }

}  // namespace dc

using namespace dc;

#define DC_HEADS_SHAPE(name, N, H, C)                                                                              \
    DC_REQUIRE((N) >= 0 && (H) >= 1 && (C) >= 1, name ": need N >= 0, H >= 1, C >= 1 (N=%lld H=%lld C=%lld)",     \
               (long long)(N), (long long)(H), (long long)(C));                                                    \
    DC_REQUIRE(sizes_ok(N, H, C), name ": size out of range")

#define DC_HEADS_HB(kernel, H, grid, stream, ...)                                                       \
    do {                                                                                                 \
        if ((H) == 1) DC_LAUNCH((kernel<1>), grid, dim3(256), 0, stream, __VA_ARGS__);                   \
        else if ((H) == 2) DC_LAUNCH((kernel<2>), grid, dim3(256), 0, stream, __VA_ARGS__);              \
        else if ((H) <= 4) DC_LAUNCH((kernel<4>), grid, dim3(256), 0, stream, __VA_ARGS__);              \
        else DC_LAUNCH((kernel<8>), grid, dim3(256), 0, stream, __VA_ARGS__);                            \
    } while (0)
// ... with the per-edge addend of the logit (GATConv(edge_dim=...))
#define DC_HEADS_HB_EDGE(kernel, H, grid, stream, ...)                                                  \
    do {                                                                                                 \
        if ((H) == 1) DC_LAUNCH((kernel<1, true>), grid, dim3(256), 0, stream, __VA_ARGS__);             \
        else if ((H) == 2) DC_LAUNCH((kernel<2, true>), grid, dim3(256), 0, stream, __VA_ARGS__);        \
        else if ((H) <= 4) DC_LAUNCH((kernel<4, true>), grid, dim3(256), 0, stream, __VA_ARGS__);        \
        else DC_LAUNCH((kernel<8, true>), grid, dim3(256), 0, stream, __VA_ARGS__);                      \
    } while (0)

extern "C" int dc_gat_alpha_heads_fwd(const float *h, int64_t ldh, const float *att_src, const float *att_dst,
                                      float *a_src, float *a_dst, int64_t N, int64_t H, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_gat_alpha_heads_fwd", N, H, C);
    DC_REQUIRE(ldh >= H * C, "dc_gat_alpha_heads_fwd: leading dimension smaller than H * C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(h && att_src && att_dst && a_src && a_dst, "dc_gat_alpha_heads_fwd: null pointer");
    const bool v4 = h_group_ok(C) && ldh % 4 == 0 && al16(h) && al16(att_src) && al16(att_dst);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (v4)
        DC_LAUNCH(k_gat_alpha_heads_fwd_v4, grid, dim3(256), 0, stream, h, ldh, att_src, att_dst, a_src, a_dst, N, (int)H,
                  (int)C);
    else
        DC_LAUNCH(k_gat_alpha_heads_fwd_any, grid, dim3(256), 0, stream, h, ldh, att_src, att_dst, a_src, a_dst, N,
                  (int)H, (int)C);
    return check_launch("dc_gat_alpha_heads_fwd");
}

extern "C" int dc_gat_edge_softmax_heads_fwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                                             const float *a_dst, float slope, float *alpha, int64_t N, int64_t H,
                                             dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_gat_edge_softmax_heads_fwd", N, H, 1);
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && a_src && a_dst && alpha, "dc_gat_edge_softmax_heads_fwd: null pointer");
    const dim3 grid((unsigned)((N * kSubH + 255) / 256));
    DC_HEADS_HB(k_gat_softmax_heads_fwd, H, grid, stream, ptr, other, a_src, a_dst, slope, alpha, N, (int)H,
                (const float *)nullptr);
    return check_launch("dc_gat_edge_softmax_heads_fwd");
}

// the two entries of GATConv(edge_dim=...) that share the kernel templates above (the rest: dc_gat_edge.hip)
extern "C" int dc_gat_edge_attr_softmax_fwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                                            const float *a_dst, const float *a_edge, float slope, float *alpha,
                                            int64_t N, int64_t H, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_gat_edge_attr_softmax_fwd", N, H, 1);
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && a_src && a_dst && a_edge && alpha, "dc_gat_edge_attr_softmax_fwd: null pointer");
    const dim3 grid((unsigned)((N * kSubH + 255) / 256));
    DC_HEADS_HB_EDGE(k_gat_softmax_heads_fwd, H, grid, stream, ptr, other, a_src, a_dst, slope, alpha, N, (int)H, a_edge);
    return check_launch("dc_gat_edge_attr_softmax_fwd");
}

extern "C" int dc_gat_edge_attr_softmax_bwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                                            const float *a_dst, const float *a_edge, float slope, const float *alpha,
                                            const float *galpha, float *ge, float *g_a_dst, int64_t N, int64_t H,
                                            dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_gat_edge_attr_softmax_bwd", N, H, 1);
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && a_src && a_dst && a_edge && alpha && galpha && ge && g_a_dst,
               "dc_gat_edge_attr_softmax_bwd: null pointer");
    const dim3 grid((unsigned)((N * kSubH + 255) / 256));
    DC_HEADS_HB_EDGE(k_gat_softmax_heads_bwd, H, grid, stream, ptr, other, a_src, a_dst, slope, alpha, galpha, ge,
                     g_a_dst, N, (int)H, a_edge);
    return check_launch("dc_gat_edge_attr_softmax_bwd");
}

extern "C" int dc_gat_edge_softmax_heads_bwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                                             const float *a_dst, float slope, const float *alpha, const float *galpha,
                                             float *ge, float *g_a_dst, int64_t N, int64_t H, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_gat_edge_softmax_heads_bwd", N, H, 1);
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && a_src && a_dst && alpha && galpha && ge && g_a_dst,
               "dc_gat_edge_softmax_heads_bwd: null pointer");
    const dim3 grid((unsigned)((N * kSubH + 255) / 256));
    DC_HEADS_HB(k_gat_softmax_heads_bwd, H, grid, stream, ptr, other, a_src, a_dst, slope, alpha, galpha, ge, g_a_dst, N,
                (int)H, (const float *)nullptr);
    return check_launch("dc_gat_edge_softmax_heads_bwd");
}

extern "C" int dc_spmm_f32_heads_bias_act(const int32_t *ptr, const int32_t *other, const float *alpha, const float *x,
                                          int64_t ldx, const float *bias, int relu, int mean, float *y, int64_t ldy,
                                          int64_t N, int64_t H, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_spmm_f32_heads_bias_act", N, H, C);
    DC_REQUIRE(ldx >= H * C && ldy >= (mean ? C : H * C), "dc_spmm_f32_heads_bias_act: leading dimension too small");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && alpha && x && y, "dc_spmm_f32_heads_bias_act: null pointer");
    DC_REQUIRE(x != y, "dc_spmm_f32_heads_bias_act: y must not alias x");
    const bool vec4 = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y) && (!bias || al16(bias));
    const dim3 grid((unsigned)((N + 3) / 4));
#define DC_SPMM_HEADS(VEC, MEAN)                                                                                   \
    DC_LAUNCH((k_spmm_heads<VEC, 8, MEAN>), grid, dim3(256), 0, stream, ptr, other, alpha, x, ldx, bias, relu, y, ldy, N, \
              (int)H, (int)C)
    if (vec4 && mean) DC_SPMM_HEADS(4, true);
    else if (vec4) DC_SPMM_HEADS(4, false);
    else if (mean) DC_SPMM_HEADS(1, true);
    else DC_SPMM_HEADS(1, false);
#undef DC_SPMM_HEADS
    return check_launch("dc_spmm_f32_heads_bias_act");
}

extern "C" int dc_sddmm_f32_heads(const int32_t *ptr, const int32_t *other, const float *g, int64_t ldg, const float *h,
                                  int64_t ldh, float *d, int64_t N, int64_t H, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_sddmm_f32_heads", N, H, C);
    DC_REQUIRE(ldg >= H * C && ldh >= H * C, "dc_sddmm_f32_heads: leading dimension smaller than H * C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && g && h && d, "dc_sddmm_f32_heads: null pointer");
    const bool v4 = h_group_ok(C) && ldg % 4 == 0 && ldh % 4 == 0 && al16(g) && al16(h);
    const dim3 grid((unsigned)((N + 3) / 4));
    if (v4)
        DC_LAUNCH((k_sddmm_heads_v4<4>), grid, dim3(256), 0, stream, ptr, other, g, ldg, h, ldh, d, N, (int)H, (int)C);
    else
        DC_LAUNCH(k_sddmm_heads_any, grid, dim3(256), 0, stream, ptr, other, g, ldg, h, ldh, d, N, (int)H, (int)C);
    return check_launch("dc_sddmm_f32_heads");
}

extern "C" int dc_segment_sum_f32_heads(const int32_t *ptr, const int32_t *map, const float *v, float *out, int64_t N,
                                        int64_t W, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_segment_sum_f32_heads", N, W, 1);
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && v && out, "dc_segment_sum_f32_heads: null pointer");
    DC_LAUNCH(k_segment_sum_heads, dim3((unsigned)((N * W + 255) / 256)), dim3(256), 0, stream, ptr, map, v, out, N, (int)W);
    return check_launch("dc_segment_sum_f32_heads");
}

extern "C" int dc_gather_f32_heads(const float *v, const int32_t *idx, float *out, const int32_t *count_ptr, int64_t cap,
                                   int64_t W, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_gather_f32_heads", cap, W, 1);
    if (cap == 0) return DC_OK;
    DC_REQUIRE(v && idx && out && count_ptr, "dc_gather_f32_heads: null pointer");
    DC_LAUNCH(k_gather_heads, dim3((unsigned)((cap * W + 255) / 256)), dim3(256), 0, stream, v, idx, out, count_ptr, cap,
              (int)W);
    return check_launch("dc_gather_f32_heads");
}

extern "C" int dc_spread_heads_f32(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t N, int64_t H, int64_t C,
                                   dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_spread_heads_f32", N, H, C);
    DC_REQUIRE(ldg >= C && ldo >= H * C, "dc_spread_heads_f32: leading dimension too small");
    if (N == 0) return DC_OK;
    DC_REQUIRE(g && out && g != out, "dc_spread_heads_f32: null pointer / aliasing");
    DC_LAUNCH(k_spread_heads, dim3((unsigned)((N * H * C + 255) / 256)), dim3(256), 0, stream, g, ldg, out, ldo, N, (int)H,
              (int)C);
    return check_launch("dc_spread_heads_f32");
}

extern "C" int dc_gat_alpha_heads_bwd(const float *h, int64_t ldh, const float *ga_src, const float *ga_dst,
                                      const float *att_src, const float *att_dst, float *gh, int64_t ldgh, int64_t N,
                                      int64_t H, int64_t C, void *workspace, int64_t workspace_bytes, float *g_att_src,
                                      float *g_att_dst, int accumulate, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_HEADS_SHAPE("dc_gat_alpha_heads_bwd", N, H, C);
    const int64_t F = H * C;
    DC_REQUIRE(colsum_width_ok(F), "dc_gat_alpha_heads_bwd: H * C must be a multiple of 4 that divides 1024 (H*C=%lld)",
               (long long)F);
    DC_REQUIRE(h && ga_src && ga_dst && att_src && att_dst && gh && g_att_src && g_att_dst && ldh >= F && ldgh >= F &&
                   ldh % 4 == 0 && ldgh % 4 == 0 && al16(h) && al16(gh) && al16(att_src) && al16(att_dst),
               "dc_gat_alpha_heads_bwd: null / misaligned operand");
    const int64_t nb = (N + kEpiRowsH - 1) / kEpiRowsH;
    DC_REQUIRE(workspace_bytes >= nb * F * 2 * (int64_t)sizeof(float) && (workspace || nb == 0),
               "dc_gat_alpha_heads_bwd: workspace too small");
    if (nb > 0)
        DC_LAUNCH(k_gat_alpha_heads_bwd, dim3((unsigned)nb), dim3(256), 0, stream, h, ldh, ga_src, ga_dst, att_src, att_dst,
                  gh, ldgh, N, (int)H, (int)C, (float *)workspace);
    const float *ws = (const float *)workspace;
    DC_LAUNCH(k_colsum_final_heads, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, stream, ws, nb, 2 * F, (int)F, g_att_src,
              accumulate);
    DC_LAUNCH(k_colsum_final_heads, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, stream, ws + F, nb, 2 * F, (int)F,
              g_att_dst, accumulate);
    return check_launch("dc_gat_alpha_heads_bwd");
}
