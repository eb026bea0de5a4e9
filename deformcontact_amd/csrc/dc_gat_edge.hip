// dc_gat_edge.hip -- the edge-feature term of GATConv(edge_dim = D) on the sorted adjacency.
//
// PyG 2.5.2 gat_conv.py edge_update with edge_attr: a_edge[p, k] = <lin_edge(edge_attr[p])[k, :], att_edge[k, :]> joins
// the logit of edge p and head k.  The term is linear in edge_attr, so it is formed as edge_attr[p, :] @ M with the folded
// M[d, k] = sum_c lin_edge.weight[k C + c, d] att_edge[k, c] ([D, H] row-major, formed by the caller): [E, H*C] never
// exists.  The appended self loop of node i (edge id E + i) carries fill_value: the mean of the attribute rows of the other
// edges into i, or a constant.  The softmax with the extra addend shares the kernel templates of dc_gat_heads.hip and
// lives there (dc_gat_edge_attr_softmax_fwd / _bwd).  Rules of the segment kernels (helpers: see dc_segment.h):
// destination-sorted segments, sums in p order (the mean) and in d / k order (the products with M), products and sums rounded separately,
// no float atomics - two runs give the same bits.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

constexpr int kSubE = 8;                      // lanes per destination segment, as kSubH of dc_gat_heads.hip
constexpr int kSegsE = 256 / kSubE;           // segments per workgroup
constexpr int kMaxD = DC_GAT_EDGE_MAX_DIM;    // the loop attributes of a workgroup's segments sit in LDS: 32 x 64 floats
constexpr int kGmChunk = 1024;                // sorted edges per workgroup of the gM partial pass

// One group of kSubE lanes per destination segment.  Pass 1, lane = attribute column: the loop attribute of the node, the
// running sum over the segment's input edges in p order divided by their count (or the constant).  Pass 2, lane = edge:
// row perm[p] of edge_attr (the loop: the row of pass 1, from LDS) times M, HB heads per walk of the row.
template <int HB>
__global__ void __launch_bounds__(256)
k_gat_edge_term_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ perm,
                    const float *__restrict__ edge_attr, int64_t lda, const float *__restrict__ m, int fill_mean,
                    float fill_value, float *__restrict__ a_edge, float *__restrict__ loop_attr, int64_t N, int E, int D,
                    int H) {
    __shared__ float la[kSegsE][kMaxD];
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kSubE;
    const int sub = threadIdx.x % kSubE, grp = threadIdx.x / kSubE;
    const bool live = i < N;
    const int beg = live ? ptr[i] : 0, end = live ? ptr[i + 1] : 0;
    for (int d = sub; d < D; d += kSubE) {
        float v = fill_value;
        if (fill_mean) {
            float s = 0.f;
            int cnt = 0;
            for (int p = beg; p < end; ++p) {
                const int e = perm[p];
                if (e < E) {
                    s = s + edge_attr[(int64_t)e * lda + d];
                    ++cnt;
                }
            }
            v = cnt > 0 ? s / (float)cnt : 0.f;
        }
        la[grp][d] = v;
        if (live) loop_attr[i * D + d] = v;
    }
    __syncthreads();
    for (int k0 = 0; k0 < H; k0 += HB) {
        for (int p = beg + sub; p < end; p += kSubE) {
            const int e = perm[p];
            const float *row = e < E ? edge_attr + (int64_t)e * lda : la[grp];
            float acc[HB];
#pragma unroll
            for (int b = 0; b < HB; ++b) acc[b] = 0.f;
            for (int d = 0; d < D; ++d) {
                const float v = row[d];
                const float *mr = m + d * H + k0;
#pragma unroll
                for (int b = 0; b < HB; ++b)
                    if (k0 + b < H) acc[b] = acc[b] + v * mr[b];
            }
            float *o = a_edge + (int64_t)p * H + k0;
#pragma unroll
            for (int b = 0; b < HB; ++b)
                if (k0 + b < H) o[b] = acc[b];
        }
    }
}

// g_edge_attr[perm[p], :] = (ge[p, :] + ge[loop of i, :] / cnt_i) @ M^T (constant fill: ge[p, :] @ M^T) for the input edges
// p of segment i: lane = edge, every input edge written by exactly one thread; H > HB: the later blocks of heads add to
// what the first one stored (same thread).
template <int HB>
__global__ void __launch_bounds__(256)
k_gat_edge_term_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ perm, const float *__restrict__ ge,
                    const float *__restrict__ m, int fill_mean, float *__restrict__ g_edge_attr, int64_t ldg, int64_t N,
                    int E, int D, int H) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kSubE;
    const int sub = threadIdx.x % kSubE;
    const bool live = i < N;
    const int beg = live ? ptr[i] : 0, end = live ? ptr[i + 1] : 0;
    int pl = -1, cnt = 0;
    for (int p = beg + sub; p < end; p += kSubE) {
        if (perm[p] >= E) pl = p;
        else ++cnt;
    }
    pl = sub_max<kSubE>(pl);
    cnt = sub_sum<kSubE>(cnt);
    const bool through_mean = fill_mean && pl >= 0 && cnt > 0;
    for (int k0 = 0; k0 < H; k0 += HB) {
        float gl[HB];
#pragma unroll
        for (int b = 0; b < HB; ++b)
            gl[b] = (through_mean && k0 + b < H) ? ge[(int64_t)pl * H + k0 + b] / (float)cnt : 0.f;
        for (int p = beg + sub; p < end; p += kSubE) {
            const int e = perm[p];
            if (e >= E) continue;
            const float *g = ge + (int64_t)p * H + k0;
            float t[HB];
#pragma unroll
            for (int b = 0; b < HB; ++b) {
                t[b] = k0 + b < H ? g[b] : 0.f;
                if (through_mean) t[b] = t[b] + gl[b];
            }
            float *o = g_edge_attr + (int64_t)e * ldg;
            for (int d = 0; d < D; ++d) {
                const float *mr = m + d * H + k0;
                float acc = 0.f;
#pragma unroll
                for (int b = 0; b < HB; ++b)
                    if (k0 + b < H) acc = acc + t[b] * mr[b];
                o[d] = k0 == 0 ? acc : o[d] + acc;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_gat_edge_zero_rows(float *__restrict__ g, int64_t ldg, int64_t E, int D) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < E * D) g[(t / D) * ldg + t % D] = 0.f;
}

// gM[d, k] = sum_p attr_fwd[p, d] ge[p, k] over the sorted edges (loops with their fill attribute), stage 1: workgroup b
// owns the sorted edges [b kGmChunk, (b + 1) kGmChunk) below the device-side edge count and writes partial[b, 0:D*H].
// D*H < 256: the workgroup's threads form 256 / (D*H) groups, each over a contiguous share of the chunk in p order,
// combined in group order through LDS; else a thread owns the pairs tid, tid + 256, ...
__global__ void __launch_bounds__(256)
k_gat_edge_gm_partial(const int32_t *__restrict__ perm, const int32_t *__restrict__ n_ptr, const float *__restrict__ ge,
                      const float *__restrict__ edge_attr, int64_t lda, const float *__restrict__ loop_attr,
                      float *__restrict__ partial, int64_t cap, int E, int D, int H) {
    __shared__ float red[256];
    const int P = D * H;
    const int64_t ne = min((int64_t)*n_ptr, cap);
    const int64_t c0 = (int64_t)blockIdx.x * kGmChunk, c1 = min(c0 + kGmChunk, ne);
    float *out = partial + (int64_t)blockIdx.x * P;
    if (P >= 256) {
        for (int pair = threadIdx.x; pair < P; pair += 256) {
            const int d = pair / H, k = pair % H;
            float s = 0.f;
            for (int64_t p = c0; p < c1; ++p) {
                const int e = perm[p];
                const float a = e < E ? edge_attr[(int64_t)e * lda + d] : loop_attr[(int64_t)(e - E) * D + d];
                s = s + a * ge[p * H + k];
            }
            out[pair] = s;
        }
        return;
    }
    const int groups = 256 / P, grp = threadIdx.x / P, pair = threadIdx.x % P;
    const int per = (kGmChunk + groups - 1) / groups;
    float s = 0.f;
    if (grp < groups) {
        const int d = pair / H, k = pair % H;
        const int64_t p0 = c0 + (int64_t)grp * per, p1 = min(p0 + per, c1);
        for (int64_t p = p0; p < p1; ++p) {
            const int e = perm[p];
            const float a = e < E ? edge_attr[(int64_t)e * lda + d] : loop_attr[(int64_t)(e - E) * D + d];
            s = s + a * ge[p * H + k];
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < P) {
        float t = 0.f;
        for (int q = 0; q < groups; ++q) t = t + red[q * P + threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// stage 2: out[c] = sum over workgroups of partial[b, c], one wave per column, fixed order (k_colsum_final, dc_gnn_epi.hip)
__global__ void __launch_bounds__(256)
k_gat_edge_gm_final(const float *__restrict__ partial, int64_t nblocks, int P, float *__restrict__ out) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= P) return;
    float s = 0.f;
    for (int64_t b = lane; b < nblocks; b += 64) s = s + partial[b * P + c];
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) s = s + __shfl_xor(s, q);
    if (lane == 0) out[c] = s;
}

static inline bool e_sizes_ok(int64_t N, int64_t E, int64_t D, int64_t H) {
    return N < (int64_t)INT32_MAX / 4 && E + N < (int64_t)INT32_MAX && H < (1 << 16) && D * H < (1 << 20);
}

}  // namespace dc

using namespace dc;

#define DC_EDGE_SHAPE(name, N, E, D, H)                                                                               \
    DC_REQUIRE((N) >= 0 && (E) >= 0 && (D) >= 1 && (H) >= 1, name ": need N >= 0, E >= 0, D >= 1, H >= 1 (N=%lld E=%lld " \
               "D=%lld H=%lld)", (long long)(N), (long long)(E), (long long)(D), (long long)(H));                      \
    DC_REQUIRE((D) <= DC_GAT_EDGE_MAX_DIM, name ": edge_dim %lld over the cap of %d", (long long)(D),                  \
               DC_GAT_EDGE_MAX_DIM);                                                                                   \
    DC_REQUIRE(e_sizes_ok(N, E, D, H), name ": size out of range")

#define DC_EDGE_HB(kernel, H, grid, stream, ...)                                                        \
    do {                                                                                                 \
        if ((H) == 1) DC_LAUNCH((kernel<1>), grid, dim3(256), 0, stream, __VA_ARGS__);                   \
        else if ((H) == 2) DC_LAUNCH((kernel<2>), grid, dim3(256), 0, stream, __VA_ARGS__);              \
        else if ((H) <= 4) DC_LAUNCH((kernel<4>), grid, dim3(256), 0, stream, __VA_ARGS__);              \
        else DC_LAUNCH((kernel<8>), grid, dim3(256), 0, stream, __VA_ARGS__);                            \
    } while (0)

extern "C" int dc_gat_edge_attr_fwd(const int32_t *ptr, const int32_t *perm, const float *edge_attr, int64_t lda,
                                    const float *m, int fill_mean, float fill_value, float *a_edge, float *loop_attr,
                                    int64_t N, int64_t E, int64_t D, int64_t H, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_EDGE_SHAPE("dc_gat_edge_attr_fwd", N, E, D, H);
    DC_REQUIRE(E == 0 || lda >= D, "dc_gat_edge_attr_fwd: leading dimension smaller than D");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && perm && m && a_edge && loop_attr && (edge_attr || E == 0), "dc_gat_edge_attr_fwd: null pointer");
    const dim3 grid((unsigned)((N * kSubE + 255) / 256));
    DC_EDGE_HB(k_gat_edge_term_fwd, H, grid, stream, ptr, perm, edge_attr, lda, m, fill_mean, fill_value, a_edge,
               loop_attr, N, (int)E, (int)D, (int)H);
    return check_launch("dc_gat_edge_attr_fwd");
}

extern "C" int64_t dc_gat_edge_attr_bwd_workspace_bytes(int64_t capacity, int64_t D, int64_t H) {
    if (capacity < 0 || D < 1 || H < 1 || D > DC_GAT_EDGE_MAX_DIM || H >= (1 << 16)) return DC_EINVAL;
    return (capacity + kGmChunk - 1) / kGmChunk * D * H * (int64_t)sizeof(float);
}

extern "C" int dc_gat_edge_attr_bwd(const int32_t *ptr, const int32_t *perm, const float *ge, const float *edge_attr,
                                    int64_t lda, const float *loop_attr, const float *m, int fill_mean,
                                    float *g_edge_attr, int64_t ldg, float *g_m, int64_t N, int64_t E, int64_t D,
                                    int64_t H, int64_t capacity, void *workspace, int64_t workspace_bytes,
                                    dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_EDGE_SHAPE("dc_gat_edge_attr_bwd", N, E, D, H);
    DC_REQUIRE(capacity >= 0 && capacity <= E + N, "dc_gat_edge_attr_bwd: capacity must be within [0, E + N]");
    DC_REQUIRE(E == 0 || (lda >= D && (!g_edge_attr || ldg >= D)), "dc_gat_edge_attr_bwd: leading dimension smaller than D");
    DC_REQUIRE(ptr && perm && ge && m && loop_attr && (edge_attr || E == 0), "dc_gat_edge_attr_bwd: null pointer");
    DC_REQUIRE(g_edge_attr != edge_attr || !edge_attr, "dc_gat_edge_attr_bwd: g_edge_attr must not alias edge_attr");
    const int64_t nb = (capacity + kGmChunk - 1) / kGmChunk;
    DC_REQUIRE(!g_m || (workspace_bytes >= nb * D * H * (int64_t)sizeof(float) && (workspace || nb == 0)),
               "dc_gat_edge_attr_bwd: workspace too small");
    if (g_edge_attr && E > 0) {
        DC_LAUNCH(k_gat_edge_zero_rows, dim3((unsigned)((E * D + 255) / 256)), dim3(256), 0, stream, g_edge_attr, ldg, E,
                  (int)D);
        if (N > 0) {
            const dim3 grid((unsigned)((N * kSubE + 255) / 256));
            DC_EDGE_HB(k_gat_edge_term_bwd, H, grid, stream, ptr, perm, ge, m, fill_mean, g_edge_attr, ldg, N, (int)E,
                       (int)D, (int)H);
        }
    }
    if (g_m) {
        if (nb > 0)
            DC_LAUNCH(k_gat_edge_gm_partial, dim3((unsigned)nb), dim3(256), 0, stream, perm, ptr + N, ge, edge_attr, lda,
                      loop_attr, (float *)workspace, capacity, (int)E, (int)D, (int)H);
        DC_LAUNCH(k_gat_edge_gm_final, dim3((unsigned)((D * H + 3) / 4)), dim3(256), 0, stream, (const float *)workspace, nb,
                  (int)(D * H), g_m);
    }
    return check_launch("dc_gat_edge_attr_bwd");
}
