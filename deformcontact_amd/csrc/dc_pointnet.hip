// dc_pointnet.hip -- the per-edge primitives of PointNet++'s set-abstraction layer (PointNetConv, PyG 2.5.2
// point_conv.py) on a BIPARTITE edge set, and the per-graph pooling that closes a point-cloud model (global_add_pool /
// global_mean_pool / global_max_pool).
//
// Sources are the n_src rows of x_src [n_src, F] / pos_src [n_src, 3], destinations the n_dst rows of pos_dst
// [n_dst, 3]; src / dst are the two int64 rows of the edge list (src_q in [0, n_src), dst_q in [0, n_dst)).  The sorted
// sets come from ONE adjacency over max(n_src, n_dst) rows: by destination ptr / other (= source id) / perm (= input
// edge id), by source ptr_t / other_t (= destination id) / perm_t; rows beyond n_dst (n_src) of the respective set are
// empty for a valid edge list.  With LOOPS (one node set, n_src == n_dst == N, an adjacency built with self loops) the
// edge rows are E' = E + N: the input edges in input order, then the loop of node i at row E + i; the sorted sets then
// hold no input edge with src == dst and name node i's loop, LAST in its group, by the edge id E + i.
//   pair, forward    z[q,c] = x_src[src_q,c] (a copy), c < F;  z[q,F+d] = pos_src[src_q,d] - pos_dst[dst_q,d]   (ONE fp32
//                    subtraction), d < 3;  a loop row E + i: [x_src[i], +0, +0, +0].  An input edge with src_q outside
//                    [0, n_src) or dst_q outside [0, n_dst) gets a zero row.  F = 0 is legal (positions alone).  zpad
//                    (0..3) further columns z[q, F+3 .. F+3+zpad) are written as zeros: the padding of a row stride
//                    rounded up to 4 floats, so that no element of such a buffer stays unwritten.
//   pair, backward   one lane group per node r, compensated sums (kahan_add) in the order of the sorted sets:
//                    g_x_src[r,c]   = sum over t in [ptr_t[r], ptr_t[r+1]) of g_z[perm_t[t],c]       (the loop row included)
//                    g_pos_src[r,d] = the same of g_z[perm_t[t],F+d] over the input edges alone      (perm_t[t] < E)
//                    g_pos_dst[r,d] = -(sum over p in [ptr[r], ptr[r+1]) of g_z[perm[p],F+d], perm[p] < E)
//                    an edge of a sorted set whose other endpoint is outside its node set (the forward wrote it a zero
//                    row) is left out.  Each output may be NULL and is then skipped.
//   reduce, backward the per-row gradient of dc_edge_reduce_fwd's sum / mean / max (dc_edge.hip; the forward walks
//                    m[perm[p]] over E' rows as it stands) for edge rows q < E':  i = dst_q (a loop row: q - E)
//                    sum g_m[q,c] = g_y[i,c];  mean g_y[i,c] / float(ptr[i+1] - ptr[i]) (the loop counts);
//                    max (m[q,c] == y[i,c]) ? g_y[i,c] / float(cnt[i,c]) : 0 - the even split of INTEGRATION.md 1.5.
//                    A zero row for: dst_q outside [0, n_dst), src_q outside [0, n_all) (n_all the adjacency's rows:
//                    edges the sorted set does not hold), and with loops an input edge with src_q == dst_q.
//   pool, forward    one workgroup per (graph g, block of 16 lanes' columns), rows [ptr[g], ptr[g+1]) (ptr NULL: one graph
//                    [0, N)).  The workgroup's 256 lanes form 16 SLOTS of 16 lanes (slots 4w .. 4w+3 in wave w); slot s
//                    takes the rows a + s, a + s + 16, a + s + 32, ... in ascending order:
//                    sum   P_s = 0, then P_s = P_s + x[r,c] (plain fp32); the total is P_0, then + P_1, ..., + P_15 in
//                          slot order through LDS (a slot without rows adds its 0);  mean: that / float(n_g)
//                    max   (mx, ct) per slot by dc_edge.hip's rule (greater: replace, count 1; equal: one more), slots
//                          merged in slot order by the same rule with their counts
//                    a graph without rows gets 0 (cnt 0).
//   pool, backward   one lane group per row r, g = batch[r] (batch NULL: 0): sum g_x[r,c] = g_y[g,c]; mean g_y[g,c] /
//                    float(n_g); max (x[r,c] == y[g,c]) ? g_y[g,c] / float(cnt[g,c]) : 0; g outside [0, B): a zero row.
//
// Rules of the segment kernels (dc_segment.h, dc_edge.hip): fp contract(off), every sum in a fixed order, no float atomics,
// no host read - two runs give the same bits and every entry can be captured.  Any width >= 1 (pair: F >= 0); 16-byte
// accesses where the width % 4 == 0 and every pointer and stride allows it, scalar otherwise; the three position columns
// are always scalar.  Lanes as in dc_edge.hip (seg_row).  Non-finite features and pooled rows follow
// INTEGRATION.md 1.14 (the pools' max walks with max_step: NaN propagates, +-Inf are ordinary values).
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

constexpr int kEdgesPn = 8;        // rows in flight per lane of the walks over a sorted set
constexpr int kPoolSlots = 16;     // row slots of a pooling workgroup
constexpr int kPoolLanes = 16;     // lanes of a slot: 16 * VEC columns per workgroup
constexpr int kPoolRows = 4;       // rows in flight per lane

// the compensated sum of column `col` of the input-edge rows (id < E) of one group of a sorted set, in set order; an
// edge whose other endpoint is outside [0, n_other) is left out
__device__ __forceinline__ float pos_walk(const int32_t *__restrict__ perm, const int32_t *__restrict__ other, int beg,
                                          int end, int64_t n_other, int64_t E, const float *__restrict__ gz,
                                          int64_t ldgz, int col) {
    constexpr int U = kEdgesPn;
    float acc = 0.f, cmp = 0.f;
    for (int p = beg; p < end; p += U) {
        const int n = end - p;
        int64_t q[U];
        bool ok[U];
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            q[u] = u < n ? perm[p + u] : 0;
            const int64_t o = u < n ? other[p + u] : -1;
            ok[u] = u < n && q[u] >= 0 && q[u] < E && o >= 0 && o < n_other;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = ok[u] ? gz[q[u] * ldgz + col] : 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (ok[u]) kahan_add(acc, cmp, v[u]);
    }
    return acc;
}

}  // namespace

// ---- pair, forward: one lane group per edge row q < rows (= E, or E + N with loops) -----------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_pointnet_pair_fwd(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const float *__restrict__ x,
                    int64_t ldx, const float *__restrict__ ps, int64_t ldps, const float *__restrict__ pd, int64_t ldpd,
                    float *__restrict__ z, int64_t ldz, int zpad, int64_t n_src, int64_t n_dst, int64_t E, int64_t rows,
                    int F, int lg) {
    int64_t q;
    int sub, L;
    if (!seg_row<WAVE>(lg, rows, q, sub, L)) return;
    const bool loop = q >= E;
    int64_t j, i;
    bool ok;
    if (loop) {
        j = i = q - E;
        ok = true;
    } else {
        j = src[q], i = dst[q];
        ok = j >= 0 && j < n_src && i >= 0 && i < n_dst;         // (else: a zero row)
    }
    for (int c = sub * VEC; c < F; c += L * VEC) {
        const Cols<VEC> xj = cols_load<VEC>(x + j * ldx + c, ok);
        cols_store<VEC>(z + q * ldz + c, xj.a);
    }
    if (sub < 3) {
        float d = 0.f;
        if (ok && !loop) d = ps[j * ldps + sub] - pd[i * ldpd + sub];
        z[q * ldz + F + sub] = d;
    } else if (sub == 3) {                                       // (a lane group has at least 4 lanes)
        for (int k = 0; k < zpad; ++k) z[q * ldz + F + 3 + k] = 0.f;
    }
}

// ---- pair, backward: one lane group per node of the adjacency ---------------------------------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_pointnet_pair_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const int32_t *__restrict__ perm,
                    const int32_t *__restrict__ ptr_t, const int32_t *__restrict__ other_t,
                    const int32_t *__restrict__ perm_t, const float *__restrict__ gz, int64_t ldgz,
                    float *__restrict__ gx, int64_t ldgx, float *__restrict__ gps, int64_t ldgps,
                    float *__restrict__ gpd, int64_t ldgpd, int64_t n_src, int64_t n_dst, int64_t E, int64_t erows,
                    int64_t rows, int F, int lg) {
    constexpr int U = kEdgesPn;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, rows, row, sub, L)) return;
    if (row < n_src) {
        const int beg_t = ptr_t[row], end_t = ptr_t[row + 1];
        if (gx) {
            for (int c = sub * VEC; c < F; c += L * VEC) {
                float acc[VEC], cmp[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = 0.f, cmp[k] = 0.f;
                for (int t = beg_t; t < end_t; t += U) {
                    const int n = end_t - t;
                    int64_t q[U];
                    bool ok[U];
                    Cols<VEC> v[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        q[u] = u < n ? perm_t[t + u] : 0;
                        const int64_t o = u < n ? other_t[t + u] : -1;
                        ok[u] = u < n && q[u] >= 0 && q[u] < erows && o >= 0 && o < n_dst;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) v[u] = cols_load<VEC>(gz + q[u] * ldgz + c, ok[u]);
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (ok[u]) {
#pragma unroll
                            for (int k = 0; k < VEC; ++k) kahan_add(acc[k], cmp[k], v[u].a[k]);
                        }
                }
                cols_store<VEC>(gx + row * ldgx + c, acc);
            }
        }
        if (gps && sub < 3)
            gps[row * ldgps + sub] = pos_walk(perm_t, other_t, beg_t, end_t, n_dst, E, gz, ldgz, F + sub);
    }
    if (row < n_dst && gpd && sub < 3) {
        const float s = pos_walk(perm, other, ptr[row], ptr[row + 1], n_src, E, gz, ldgz, F + sub);
        gpd[row * ldgpd + sub] = -s;
    }
}

// ---- reduce, backward: one lane group per edge row q < rows; m and g_m stream, the rows of the destination are gathered
// mode (wave-uniform): 0 a copy of g_y[i]; 1 that divided by the in-degree of i; 2 the even split of the max
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_pointnet_reduce_bwd(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const int32_t *__restrict__ ptr,
                      const float *__restrict__ m, int64_t ldm, const float *__restrict__ y, int64_t ldy,
                      const int32_t *__restrict__ cnt, int64_t ldc, const float *__restrict__ gy, int64_t ldgy,
                      float *__restrict__ gm, int64_t ldgm, int mode, int loops, int64_t n_all, int64_t n_dst, int64_t E,
                      int64_t rows, int C, int lg) {
    int64_t q;
    int sub, L;
    if (!seg_row<WAVE>(lg, rows, q, sub, L)) return;
    int64_t i;
    bool ok;
    if (q >= E) {
        i = q - E;                                               // the appended loop of node i
        ok = true;
    } else {
        const int64_t j = src[q];
        i = dst[q];
        ok = j >= 0 && j < n_all && i >= 0 && i < n_dst && !(loops && j == i);
    }
    float deg = 1.f;
    if (mode == 1 && ok) {
        const int d = ptr[i + 1] - ptr[i];
        deg = (float)(d > 0 ? d : 1);
    }
    reduce_bwd_cols<VEC>(mode, ok, deg, m + q * ldm, y + i * ldy, cnt + i * ldc, gy + i * ldgy, gm + q * ldgm, sub, L, C);
}

// ---- pool, forward: one workgroup per (graph, column block); 16 slots of 16 lanes, merged through LDS in slot order -----
template <int VEC>
__global__ void __launch_bounds__(256)
k_pool_fwd(const int64_t *__restrict__ ptr, const float *__restrict__ x, int64_t ldx, float *__restrict__ y, int64_t ldy,
           int32_t *__restrict__ cnt, int64_t ldc, int mode, int64_t N, int C, int ncb) {
    constexpr int U = kPoolRows, W = kPoolLanes * VEC;
    __shared__ float s_v[kPoolSlots][W];
    __shared__ int s_c[kPoolSlots][W];
    const int64_t g = blockIdx.x / (unsigned)ncb;
    const int cb = blockIdx.x % (unsigned)ncb;
    const int sub = threadIdx.x & (kPoolLanes - 1), slot = threadIdx.x >> 4;
    const int c = cb * W + sub * VEC;
    const bool col_ok = c < C;                                   // (VEC = 4: C % 4 == 0, the four columns are all inside)
    int64_t a = 0, b = N;
    if (ptr) {
        a = ptr[g], b = ptr[g + 1];
        a = a < 0 ? 0 : (a > N ? N : a);
        b = b < a ? a : (b > N ? N : b);
    }
    const bool is_max = mode == 2;
    float acc[VEC];
    int ct[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = is_max ? -INFINITY : 0.f, ct[k] = 0;
    for (int64_t r = a + slot; r < b; r += kPoolSlots * U) {
        Cols<VEC> v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t rr = r + (int64_t)kPoolSlots * u;
            v[u] = cols_load<VEC>(x + rr * ldx + c, col_ok && rr < b);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (r + (int64_t)kPoolSlots * u < b) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float e = v[u].a[k];
                    if (is_max) {
                        max_step(e, 1, acc[k], ct[k]);
                    } else {
                        acc[k] = acc[k] + e;
                    }
                }
            }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) s_v[slot][sub * VEC + k] = acc[k], s_c[slot][sub * VEC + k] = ct[k];
    __syncthreads();
    if (slot != 0 || !col_ok) return;
    for (int s = 1; s < kPoolSlots; ++s) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float e = s_v[s][sub * VEC + k];
            if (is_max) {
                max_step(e, s_c[s][sub * VEC + k], acc[k], ct[k]);
            } else {
                acc[k] = acc[k] + e;
            }
        }
    }
    if (b <= a) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f, ct[k] = 0;
    } else if (mode == 1) {
        const float n = (float)(b - a);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = acc[k] / n;
    }
    cols_store<VEC>(y + g * ldy + c, acc);
    if (is_max) ints_store<VEC>(cnt + g * ldc + c, ct);
}

// ---- pool, backward: one lane group per row r; x and g_x stream, the rows of the graph are gathered --------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_pool_bwd(const int64_t *__restrict__ batch, const int64_t *__restrict__ ptr, const float *__restrict__ x, int64_t ldx,
           const float *__restrict__ y, int64_t ldy, const int32_t *__restrict__ cnt, int64_t ldc,
           const float *__restrict__ gy, int64_t ldgy, float *__restrict__ gx, int64_t ldgx, int mode, int64_t B,
           int64_t N, int C, int lg) {
    int64_t r;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, r, sub, L)) return;
    const int64_t g = batch ? batch[r] : 0;
    const bool ok = g >= 0 && g < B;
    float deg = 1.f;
    if (mode == 1 && ok) {
        int64_t a = 0, b = N;
        if (ptr) {
            a = ptr[g], b = ptr[g + 1];
            a = a < 0 ? 0 : (a > N ? N : a);
            b = b < a ? a : (b > N ? N : b);
        }
        deg = (float)(b > a ? b - a : 1);
    }
    reduce_bwd_cols<VEC>(mode, ok, deg, x + r * ldx, y + g * ldy, cnt + g * ldc, gy + g * ldgy, gx + r * ldgx, sub, L, C);
}

}  // namespace dc

using namespace dc;

// the four forms of a lane-group kernel: 16-byte or scalar columns, one wave per row or 64 / L rows per wave.  UNITS: the
// lanes a row can use (its column units, and at least the 3 position lanes where a kernel has them); W: the width passed
#define DC_PN_LAUNCH(kernel, v4, ROWS, UNITS, W, stream, ...)                                                      \
    do {                                                                                                           \
        const int lg_ = log2_lanes(UNITS);                                                                         \
        const int64_t rows_ = 256 >> lg_;                                                                          \
        const dim3 grid_((unsigned)(((ROWS) + rows_ - 1) / rows_));                                                \
        if ((v4) && lg_ == 6) DC_LAUNCH((kernel<4, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(W), lg_); \
        else if (v4) DC_LAUNCH((kernel<4, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(W), lg_);       \
        else if (lg_ == 6) DC_LAUNCH((kernel<1, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(W), lg_);  \
        else DC_LAUNCH((kernel<1, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(W), lg_);               \
    } while (0)

#define DC_PN_MODE(name, mode) \
    DC_REQUIRE((mode) >= 0 && (mode) <= 2, name ": mode must be 0 (sum), 1 (mean) or 2 (max), got %d", mode)

extern "C" int dc_pointnet_pair_fwd(const int64_t *src, const int64_t *dst, const float *x, int64_t ldx,
                                    const float *pos_src, int64_t ldps, const float *pos_dst, int64_t ldpd, float *z,
                                    int64_t ldz, int64_t n_src, int64_t n_dst, int64_t E, int64_t F, int loops,
                                    int zpad, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "dc_pointnet_pair_fwd";
    DC_REQUIRE(n_src >= 0 && n_dst >= 0 && E >= 0 && F >= 0, "%s: need n_src, n_dst, E, F >= 0 (n_src=%lld n_dst=%lld "
               "E=%lld F=%lld)", name, (long long)n_src, (long long)n_dst, (long long)E, (long long)F);
    DC_REQUIRE(!loops || n_src == n_dst, "%s: loops need one node set (n_src == n_dst)", name);
    DC_REQUIRE(sizes_ok(n_src, F + 3) && sizes_ok(n_dst, F + 3) && sizes_ok(E, F + 3) && sizes_ok(E + n_src, F + 3),
               "%s: size out of range", name);
    DC_REQUIRE(zpad >= 0 && zpad <= 3, "%s: zpad must be 0..3 padding columns, got %d", name, zpad);
    DC_REQUIRE((F == 0 || ldx >= F) && ldps >= 3 && ldpd >= 3 && ldz >= F + 3 + zpad,
               "%s: leading dimension smaller than F (x), 3 (pos) or F + 3 + zpad (z)", name);
    const int64_t rows = E + (loops ? n_src : 0);
    if (rows == 0) return DC_OK;
    DC_REQUIRE((E == 0 || (src && dst)) && (F == 0 || x) && pos_src && pos_dst && z, "%s: null pointer", name);
    DC_REQUIRE(z != x && z != pos_src && z != pos_dst, "%s: z must not alias an input", name);
    const bool v4 = F > 0 && F % 4 == 0 && ldx % 4 == 0 && ldz % 4 == 0 && al16(x) && al16(z);
    const int64_t units = v4 ? F / 4 : F;
    DC_PN_LAUNCH(k_pointnet_pair_fwd, v4, rows, units > 3 ? units : 3, F, stream, src, dst, x, ldx, pos_src, ldps,
                 pos_dst, ldpd, z, ldz, zpad, n_src, n_dst, E, rows);
    return check_launch(name);
}

extern "C" int dc_pointnet_pair_bwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const int32_t *ptr_t,
                                    const int32_t *other_t, const int32_t *perm_t, const float *gz, int64_t ldgz,
                                    float *gx, int64_t ldgx, float *gpos_src, int64_t ldgps, float *gpos_dst,
                                    int64_t ldgpd, int64_t n_src, int64_t n_dst, int64_t E, int64_t F, int loops,
                                    dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "dc_pointnet_pair_bwd";
    DC_REQUIRE(n_src >= 0 && n_dst >= 0 && E >= 0 && F >= 0, "%s: need n_src, n_dst, E, F >= 0 (n_src=%lld n_dst=%lld "
               "E=%lld F=%lld)", name, (long long)n_src, (long long)n_dst, (long long)E, (long long)F);
    DC_REQUIRE(!loops || n_src == n_dst, "%s: loops need one node set (n_src == n_dst)", name);
    DC_REQUIRE(sizes_ok(n_src, F + 3) && sizes_ok(n_dst, F + 3) && sizes_ok(E, F + 3) && sizes_ok(E + n_src, F + 3),
               "%s: size out of range", name);
    DC_REQUIRE(ldgz >= F + 3 && (F == 0 || ldgx >= F) && ldgps >= 3 && ldgpd >= 3,
               "%s: leading dimension smaller than F + 3 (gz), F (gx) or 3 (pos)", name);
    const int64_t rows = n_src > n_dst ? n_src : n_dst;
    if (F == 0) gx = nullptr;
    if (rows == 0 || (!gx && !gpos_src && !gpos_dst)) return DC_OK;
    DC_REQUIRE(ptr && other && perm && ptr_t && other_t && perm_t && gz, "%s: null pointer", name);
    DC_REQUIRE(gx != gz && gpos_src != gz && gpos_dst != gz && (!gx || (gx != gpos_src && gx != gpos_dst)) &&
               (!gpos_src || gpos_src != gpos_dst), "%s: an output must not alias gz or another output", name);
    const bool v4 = gx && F % 4 == 0 && ldgz % 4 == 0 && ldgx % 4 == 0 && al16(gz) && al16(gx);
    const int64_t units = v4 ? F / 4 : F;
    DC_PN_LAUNCH(k_pointnet_pair_bwd, v4, rows, units > 3 ? units : 3, F, stream, ptr, other, perm, ptr_t, other_t,
                 perm_t, gz, ldgz, gx, ldgx, gpos_src, ldgps, gpos_dst, ldgpd, n_src, n_dst, E,
                 E + (loops ? n_src : 0), rows);
    return check_launch(name);
}

extern "C" int dc_pointnet_reduce_bwd(const int64_t *src, const int64_t *dst, const int32_t *ptr, const float *m,
                                      int64_t ldm, const float *y, int64_t ldy, const int32_t *cnt, int64_t ldc,
                                      const float *gy, int64_t ldgy, float *gm, int64_t ldgm, int mode, int64_t n_all,
                                      int64_t n_dst, int64_t E, int64_t C, int loops, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "dc_pointnet_reduce_bwd";
    DC_REQUIRE(n_all >= 0 && n_dst >= 0 && n_dst <= n_all && E >= 0 && C >= 1, "%s: need 0 <= n_dst <= n_all, E >= 0, "
               "width >= 1 (n_all=%lld n_dst=%lld E=%lld width=%lld)", name, (long long)n_all, (long long)n_dst,
               (long long)E, (long long)C);
    DC_REQUIRE(!loops || n_all == n_dst, "%s: loops need one node set (n_all == n_dst)", name);
    DC_REQUIRE(sizes_ok(n_all, C) && sizes_ok(E, C) && sizes_ok(E + n_all, C), "%s: size out of range", name);
    DC_PN_MODE("dc_pointnet_reduce_bwd", mode);
    DC_REQUIRE(ldgy >= C && ldgm >= C && (mode != 2 || (ldm >= C && ldy >= C && ldc >= C)),
               "%s: leading dimension smaller than C", name);
    const int64_t rows = E + (loops ? n_dst : 0);
    if (rows == 0) return DC_OK;
    DC_REQUIRE((E == 0 || (src && dst)) && gy && gm && (mode != 1 || ptr) && (mode != 2 || (m && y && cnt)),
               "%s: null pointer", name);
    DC_REQUIRE(gm != gy && (mode != 2 || (gm != m && gm != y && (const void *)gm != (const void *)cnt)),
               "%s: gm must not alias an input", name);
    const bool v4 = C % 4 == 0 && ldgy % 4 == 0 && ldgm % 4 == 0 && al16(gy) && al16(gm) &&
                    (mode != 2 || (ldm % 4 == 0 && ldy % 4 == 0 && ldc % 4 == 0 && al16(m) && al16(y) && al16(cnt)));
    DC_PN_LAUNCH(k_pointnet_reduce_bwd, v4, rows, v4 ? C / 4 : C, C, stream, src, dst, ptr, m, ldm, y, ldy, cnt, ldc, gy,
                 ldgy, gm, ldgm, mode, loops, n_all, n_dst, E, rows);
    return check_launch(name);
}

extern "C" int dc_pool_fwd(const int64_t *ptr, const float *x, int64_t ldx, float *y, int64_t ldy, int32_t *cnt,
                           int64_t ldc, int mode, int64_t N, int64_t B, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "dc_pool_fwd";
    DC_REQUIRE(N >= 0 && B >= 0 && C >= 1, "%s: need N >= 0, B >= 0, width >= 1 (N=%lld B=%lld width=%lld)", name,
               (long long)N, (long long)B, (long long)C);
    DC_REQUIRE(sizes_ok(N, C) && sizes_ok(B, C), "%s: size out of range", name);
    DC_PN_MODE("dc_pool_fwd", mode);
    DC_REQUIRE(ldx >= C && ldy >= C && (mode != 2 || ldc >= C), "%s: leading dimension smaller than C", name);
    if (B == 0) return DC_OK;
    DC_REQUIRE((N == 0 || x) && y, "%s: null pointer", name);
    DC_REQUIRE(ptr || B == 1, "%s: null pointer (ptr may be NULL for one graph only, B=%lld)", name, (long long)B);
    DC_REQUIRE(mode != 2 || cnt, "%s: null pointer (the max needs cnt)", name);
    DC_REQUIRE(mode == 2 || !cnt, "%s: cnt is written by the max only and must be NULL for sum and mean", name);
    DC_REQUIRE(y != x && (!cnt || ((const void *)cnt != (const void *)x && (const void *)cnt != (const void *)y)),
               "%s: y / cnt must not alias x or each other", name);
    const bool v4 = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y) &&
                    (mode != 2 || (ldc % 4 == 0 && al16(cnt)));
    const int64_t w = kPoolLanes * (v4 ? 4 : 1), ncb = (C + w - 1) / w;
    DC_REQUIRE(B * ncb < (int64_t)INT32_MAX, "%s: size out of range (graphs x column blocks)", name);
    const dim3 grid((unsigned)(B * ncb));
    if (v4) DC_LAUNCH((k_pool_fwd<4>), grid, dim3(256), 0, stream, ptr, x, ldx, y, ldy, cnt, ldc, mode, N, (int)C, (int)ncb);
    else DC_LAUNCH((k_pool_fwd<1>), grid, dim3(256), 0, stream, ptr, x, ldx, y, ldy, cnt, ldc, mode, N, (int)C, (int)ncb);
    return check_launch(name);
}

extern "C" int dc_pool_bwd(const int64_t *batch, const int64_t *ptr, const float *x, int64_t ldx, const float *y,
                           int64_t ldy, const int32_t *cnt, int64_t ldc, const float *gy, int64_t ldgy, float *gx,
                           int64_t ldgx, int mode, int64_t N, int64_t B, int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "dc_pool_bwd";
    DC_REQUIRE(N >= 0 && B >= 0 && C >= 1, "%s: need N >= 0, B >= 0, width >= 1 (N=%lld B=%lld width=%lld)", name,
               (long long)N, (long long)B, (long long)C);
    DC_REQUIRE(sizes_ok(N, C) && sizes_ok(B, C), "%s: size out of range", name);
    DC_PN_MODE("dc_pool_bwd", mode);
    DC_REQUIRE(ldgy >= C && ldgx >= C && (mode != 2 || (ldx >= C && ldy >= C && ldc >= C)),
               "%s: leading dimension smaller than C", name);
    if (N == 0) return DC_OK;
    DC_REQUIRE(gy && gx && (mode != 2 || (x && y && cnt)), "%s: null pointer", name);
    DC_REQUIRE((batch && (ptr || mode != 1)) || (!batch && !ptr && B == 1),
               "%s: null pointer (batch and ptr may be NULL for one graph only; the mean reads ptr)", name);
    DC_REQUIRE(gx != gy && (mode != 2 || (gx != x && gx != y && (const void *)gx != (const void *)cnt)),
               "%s: gx must not alias an input", name);
    const bool v4 = C % 4 == 0 && ldgy % 4 == 0 && ldgx % 4 == 0 && al16(gy) && al16(gx) &&
                    (mode != 2 || (ldx % 4 == 0 && ldy % 4 == 0 && ldc % 4 == 0 && al16(x) && al16(y) && al16(cnt)));
    DC_PN_LAUNCH(k_pool_bwd, v4, N, v4 ? C / 4 : C, C, stream, batch, ptr, x, ldx, y, ldy, cnt, ldc, gy, ldgy, gx, ldgx,
                 mode, B, N);
    return check_launch(name);
}
