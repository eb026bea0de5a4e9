// dc_edge.hip -- the two per-edge primitives of the "module per edge" layers (EdgeConv, PyG 2.5.2 edge_conv.py): the
// pair rows [x_i, x_j - x_i] of every edge with their backward, and the reduction of rows that LIVE ON THE EDGES
// (sum / mean / max per destination) with its backward.
//
// x [N, F] (row stride ldx) are the node rows; z [E, 2F], m [E, C] and their gradients are edge rows IN THE ORDER OF
// THE INPUT EDGES (src / dst: the two int64 rows of the edge list the adjacency was built from).  The
// destination-sorted adjacency (ptr [N+1]) carries perm = the input edge id of every sorted position, the transposed
// set (ptr_t / perm_t) likewise.  The edge set is taken as it is given - no self loop is added, duplicates count, a row
// may have no edge.
//   pair, forward    z[q,c]   = x[dst_q,c];  z[q,F+c] = x[src_q,c] - x[dst_q,c]          (one fp32 subtraction)
//   pair, backward   g_x[j,c] = the compensated sum, in this order, of
//                               g_z[perm[p],c] - g_z[perm[p],F+c]  for p in [ptr[j], ptr[j+1])     (the edges into j; the
//                                                                   difference is formed first, in fp32)
//                               g_z[perm_t[t],F+c]                 for t in [ptr_t[j], ptr_t[j+1])  (the edges out of j)
//   reduce, forward  sum   y[i,c] = acc, acc = 0, then acc = acc + m[perm[p],c] in p order: plain fp32 adds
//                    mean  that sum / float(deg_i), deg_i = ptr[i+1] - ptr[i]: a true division
//                    max   y[i,c] = the maximum of m[perm[p],c]; cnt[i,c] = the number of edges of the row that attain it
//                    a row without edges is 0 (cnt 0)
//   reduce, backward sum   g_m[q,c] = g_y[dst_q,c]
//                    mean  g_m[q,c] = g_y[dst_q,c] / float(deg_{dst_q})
//                    max   g_m[q,c] = (m[q,c] == y[dst_q,c]) ? g_y[dst_q,c] / float(cnt[dst_q,c]) : 0
// The max backward splits the gradient EVENLY among all edges that attain the maximum, a duplicate edge counting as an
// edge; the comparison is exact - y is a copy of one of the reduced values.  Non-finite inputs as in dc_sage.hip
// (INTEGRATION.md 1.14): contained sums, a NaN-propagating max forward (max_step) that selects among +-Inf exactly.
//
// The two kernels with one lane group per INPUT edge q (pair forward, reduce backward) stream their edge rows - row q
// in, row q out, every output row written exactly once by one lane group - and gather only node rows (x[src_q],
// x[dst_q]; g_y, y, cnt of dst_q).  An edge with an endpoint outside [0, N) - the build skips and flags those - gets
// a zero row.  The two kernels with one lane group per node (pair backward, reduce forward) walk the sorted sets and
// gather edge rows through perm.
//
// Rules of the segment kernels (helpers: see dc_segment.h): fp contract(off), every sum in a fixed order, no float
// atomics, no host read - two runs give the same bits, and every entry can be captured.  Any width >= 1: 16-byte loads
// where the width % 4 == 0 and every pointer and stride allows it, scalar loads otherwise; no width cap (columns in
// chunks of the lane group); any in-degree.
//
// Lanes as in dc_gine.hip (seg_row, dc_segment.h): a row is served by a group of L lanes, L the power of two >= width /
// VEC within 4..64 (the pair kernels: the width is F, a lane holds column c of both halves of the 2F row); 256 / L rows
// per workgroup; L = 64 is the one-wave-per-row form.  U edge rows are in flight per lane before the first is consumed.
// No lane reads what another lane wrote and there is no cross-lane step.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

constexpr int kEdgesEd = 8;        // rows in flight per lane: one gathered array per edge (reduce forward, out-edges)
constexpr int kEdgesEdPair = 4;    // the in-edges of the pair backward gather two arrays per edge

}  // namespace

// ---- pair, forward: one lane group per INPUT edge q; z streams, x[dst_q] and x[src_q] are gathered --------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_edge_pair_fwd(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const float *__restrict__ x,
                int64_t ldx, float *__restrict__ z, int64_t ldz, int64_t N, int64_t E, int F, int lg) {
    int64_t q;
    int sub, L;
    if (!seg_row<WAVE>(lg, E, q, sub, L)) return;
    const int64_t j = src[q], i = dst[q];
    const bool ok = j >= 0 && j < N && i >= 0 && i < N;          // (an edge the build skipped: a zero row)
    for (int c = sub * VEC; c < F; c += L * VEC) {
        const Cols<VEC> xi = cols_load<VEC>(x + i * ldx + c, ok);
        const Cols<VEC> xj = cols_load<VEC>(x + j * ldx + c, ok);
        float d[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) d[k] = xj.a[k] - xi.a[k];
        cols_store<VEC>(z + q * ldz + c, xi.a);
        cols_store<VEC>(z + q * ldz + F + c, d);
    }
}

// ---- pair, backward: one lane group per node j; first the edges into j (both halves of g_z), then the edges out of j ---
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_edge_pair_bwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ perm, const int32_t *__restrict__ ptr_t,
                const int32_t *__restrict__ perm_t, const float *__restrict__ gz, int64_t ldgz,
                float *__restrict__ gx, int64_t ldgx, int64_t N, int F, int lg) {
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    const int beg_t = ptr_t[row], end_t = ptr_t[row + 1];
    for (int c = sub * VEC; c < F; c += L * VEC) {
        float acc[VEC], cmp[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f, cmp[k] = 0.f;
        {
            constexpr int U = kEdgesEdPair;
            for (int p = beg; p < end; p += U) {
                const int n = end - p;
                int64_t q[U];
                Cols<VEC> a[U], b[U];
#pragma unroll
                for (int u = 0; u < U; ++u) q[u] = u < n ? perm[p + u] : 0;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    a[u] = cols_load<VEC>(gz + q[u] * ldgz + c, u < n);
                    b[u] = cols_load<VEC>(gz + q[u] * ldgz + F + c, u < n);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u < n) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) {
                            const float d = a[u].a[k] - b[u].a[k];
                            kahan_add(acc[k], cmp[k], d);
                        }
                    }
            }
        }
        {
            constexpr int U = kEdgesEd;
            for (int t = beg_t; t < end_t; t += U) {
                const int n = end_t - t;
                int64_t q[U];
                Cols<VEC> b[U];
#pragma unroll
                for (int u = 0; u < U; ++u) q[u] = u < n ? perm_t[t + u] : 0;
#pragma unroll
                for (int u = 0; u < U; ++u) b[u] = cols_load<VEC>(gz + q[u] * ldgz + F + c, u < n);
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (u < n) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) kahan_add(acc[k], cmp[k], b[u].a[k]);
                    }
            }
        }
        cols_store<VEC>(gx + row * ldgx + c, acc);
    }
}

// ---- reduce, forward: sum and mean (the sum divided by the in-degree in the same launch) ------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_edge_sum_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ perm, const float *__restrict__ m,
               int64_t ldm, float *__restrict__ y, int64_t ldy, int mean, int64_t N, int C, int lg) {
    constexpr int U = kEdgesEd;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    const float deg = (float)(end - beg);
    for (int c = sub * VEC; c < C; c += L * VEC) {
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t q[U];
            Cols<VEC> v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) q[u] = u < n ? perm[p + u] : 0;
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = cols_load<VEC>(m + q[u] * ldm + c, u < n);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + v[u].a[k];
                }
        }
        if (mean && end > beg) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] / deg;
        }
        cols_store<VEC>(y + row * ldy + c, acc);
    }
}

// ---- reduce, forward: the maximum and the number of edges that attain it, in one walk ----------------------------------
// greater: the maximum is replaced and the count starts again at 1; equal: one more (k_sage_max_fwd's rule)
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_edge_max_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ perm, const float *__restrict__ m,
               int64_t ldm, float *__restrict__ y, int64_t ldy, int32_t *__restrict__ cnt, int64_t ldc, int64_t N,
               int C, int lg) {
    constexpr int U = kEdgesEd;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    for (int c = sub * VEC; c < C; c += L * VEC) {
        float mx[VEC];
        int ct[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) mx[k] = -INFINITY, ct[k] = 0;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t q[U];
            Cols<VEC> v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) q[u] = u < n ? perm[p + u] : 0;
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = cols_load<VEC>(m + q[u] * ldm + c, u < n);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) max_step(v[u].a[k], 1, mx[k], ct[k]);
                }
        }
        if (end <= beg) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) mx[k] = 0.f;
        }
        cols_store<VEC>(y + row * ldy + c, mx);
        ints_store<VEC>(cnt + row * ldc + c, ct);
    }
}

// ---- reduce, backward: one lane group per INPUT edge q; m and g_m stream, the rows of dst_q are gathered ---------------
// mode (wave-uniform): 0 a copy of g_y[dst_q]; 1 that divided by the in-degree of dst_q; 2 the even split of the max
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_edge_reduce_bwd(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const int32_t *__restrict__ ptr,
                  const float *__restrict__ m, int64_t ldm, const float *__restrict__ y, int64_t ldy,
                  const int32_t *__restrict__ cnt, int64_t ldc, const float *__restrict__ gy, int64_t ldgy,
                  float *__restrict__ gm, int64_t ldgm, int mode, int64_t N, int64_t E, int C, int lg) {
    int64_t q;
    int sub, L;
    if (!seg_row<WAVE>(lg, E, q, sub, L)) return;
    const int64_t j = src[q], i = dst[q];
    const bool ok = j >= 0 && j < N && i >= 0 && i < N;          // (an edge the build skipped: a zero row)
    float deg = 1.f;
    if (mode == 1 && ok) {
        const int d = ptr[i + 1] - ptr[i];
        deg = (float)(d > 0 ? d : 1);
    }
    for (int c = sub * VEC; c < C; c += L * VEC) {
        const Cols<VEC> gv = cols_load<VEC>(gy + i * ldgy + c, ok);
        float out[VEC];
        if (mode == 2) {
            const Cols<VEC> mv = cols_load<VEC>(m + q * ldm + c, ok);
            const Cols<VEC> yv = cols_load<VEC>(y + i * ldy + c, ok);
            const Ints<VEC> cv = ints_load<VEC>(cnt + i * ldc + c, ok);
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
        cols_store<VEC>(gm + q * ldgm + c, out);
    }
}

}  // namespace dc

using namespace dc;

#define DC_EDGE_SHAPE(name, N, F)                                                                                  \
    DC_REQUIRE((N) >= 0 && (F) >= 1, name ": need N >= 0, width >= 1 (N=%lld width=%lld)", (long long)(N),        \
               (long long)(F));                                                                                    \
    DC_REQUIRE(sizes_ok(N, F), name ": size out of range")

// the four forms of a kernel: 16-byte or scalar columns, one wave per row or 64 / L rows per wave (ROWS rows in all)
#define DC_EDGE_LAUNCH(kernel, v4, ROWS, F, stream, ...)                                                           \
    do {                                                                                                           \
        const int lg_ = log2_lanes((v4) ? (F) / 4 : (F));                                                       \
        const int64_t rows_ = 256 >> lg_;                                                                          \
        const dim3 grid_((unsigned)(((ROWS) + rows_ - 1) / rows_));                                                \
        if ((v4) && lg_ == 6) DC_LAUNCH((kernel<4, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_); \
        else if (v4) DC_LAUNCH((kernel<4, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);       \
        else if (lg_ == 6) DC_LAUNCH((kernel<1, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);  \
        else DC_LAUNCH((kernel<1, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);               \
    } while (0)

extern "C" int dc_edge_pair_fwd(const int64_t *src, const int64_t *dst, const float *x, int64_t ldx, float *z,
                                int64_t ldz, int64_t N, int64_t E, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_EDGE_SHAPE("dc_edge_pair_fwd", N, F);
    DC_REQUIRE(E >= 0 && sizes_ok(E, 2 * F), "dc_edge_pair_fwd: E or 2F out of range (E=%lld)", (long long)E);
    DC_REQUIRE(ldx >= F && ldz >= 2 * F, "dc_edge_pair_fwd: leading dimension smaller than F (x) or 2F (z)");
    if (E == 0) return DC_OK;
    DC_REQUIRE(src && dst && x && z, "dc_edge_pair_fwd: null pointer");
    DC_REQUIRE(z != x, "dc_edge_pair_fwd: z must not alias x");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldz % 4 == 0 && al16(x) && al16(z);
    DC_EDGE_LAUNCH(k_edge_pair_fwd, v4, E, F, stream, src, dst, x, ldx, z, ldz, N, E);
    return check_launch("dc_edge_pair_fwd");
}

extern "C" int dc_edge_pair_bwd(const int32_t *ptr, const int32_t *perm, const int32_t *ptr_t, const int32_t *perm_t,
                                const float *gz, int64_t ldgz, float *gx, int64_t ldgx, int64_t N, int64_t F,
                                dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_EDGE_SHAPE("dc_edge_pair_bwd", N, F);
    DC_REQUIRE(2 * F < (1 << 24), "dc_edge_pair_bwd: size out of range");
    DC_REQUIRE(ldgz >= 2 * F && ldgx >= F, "dc_edge_pair_bwd: leading dimension smaller than 2F (gz) or F (gx)");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && perm && ptr_t && perm_t && gz && gx, "dc_edge_pair_bwd: null pointer");
    DC_REQUIRE(gx != gz, "dc_edge_pair_bwd: gx must not alias gz");
    const bool v4 = F % 4 == 0 && ldgz % 4 == 0 && ldgx % 4 == 0 && al16(gz) && al16(gx);
    DC_EDGE_LAUNCH(k_edge_pair_bwd, v4, N, F, stream, ptr, perm, ptr_t, perm_t, gz, ldgz, gx, ldgx, N);
    return check_launch("dc_edge_pair_bwd");
}

extern "C" int dc_edge_reduce_fwd(const int32_t *ptr, const int32_t *perm, const float *m, int64_t ldm, float *y,
                                  int64_t ldy, int32_t *cnt, int64_t ldc, int mode, int64_t N, int64_t C,
                                  dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_EDGE_SHAPE("dc_edge_reduce_fwd", N, C);
    DC_REQUIRE(mode >= 0 && mode <= 2, "dc_edge_reduce_fwd: mode must be 0 (sum), 1 (mean) or 2 (max), got %d", mode);
    DC_REQUIRE(ldm >= C && ldy >= C && (mode != 2 || ldc >= C), "dc_edge_reduce_fwd: leading dimension smaller than C");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && perm && m && y, "dc_edge_reduce_fwd: null pointer");
    DC_REQUIRE(mode != 2 || cnt, "dc_edge_reduce_fwd: null pointer (the max needs cnt)");
    DC_REQUIRE(mode == 2 || !cnt, "dc_edge_reduce_fwd: cnt is written by the max only and must be NULL for sum and mean");
    DC_REQUIRE(y != m && (const void *)cnt != (const void *)m && (const void *)cnt != (const void *)y,
               "dc_edge_reduce_fwd: y / cnt must not alias m or each other");
    if (mode == 2) {
        const bool v4 = C % 4 == 0 && ldm % 4 == 0 && ldy % 4 == 0 && ldc % 4 == 0 && al16(m) && al16(y) && al16(cnt);
        DC_EDGE_LAUNCH(k_edge_max_fwd, v4, N, C, stream, ptr, perm, m, ldm, y, ldy, cnt, ldc, N);
    } else {
        const bool v4 = C % 4 == 0 && ldm % 4 == 0 && ldy % 4 == 0 && al16(m) && al16(y);
        DC_EDGE_LAUNCH(k_edge_sum_fwd, v4, N, C, stream, ptr, perm, m, ldm, y, ldy, mode, N);
    }
    return check_launch("dc_edge_reduce_fwd");
}

extern "C" int dc_edge_reduce_bwd(const int64_t *src, const int64_t *dst, const int32_t *ptr, const float *m,
                                  int64_t ldm, const float *y, int64_t ldy, const int32_t *cnt, int64_t ldc,
                                  const float *gy, int64_t ldgy, float *gm, int64_t ldgm, int mode, int64_t N, int64_t E,
                                  int64_t C, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_EDGE_SHAPE("dc_edge_reduce_bwd", N, C);
    DC_REQUIRE(E >= 0 && sizes_ok(E, C), "dc_edge_reduce_bwd: E out of range (E=%lld)", (long long)E);
    DC_REQUIRE(mode >= 0 && mode <= 2, "dc_edge_reduce_bwd: mode must be 0 (sum), 1 (mean) or 2 (max), got %d", mode);
    DC_REQUIRE(ldgy >= C && ldgm >= C && (mode != 2 || (ldm >= C && ldy >= C && ldc >= C)),
               "dc_edge_reduce_bwd: leading dimension smaller than C");
    if (E == 0) return DC_OK;
    DC_REQUIRE(src && dst && gy && gm && (mode != 1 || ptr) && (mode != 2 || (m && y && cnt)),
               "dc_edge_reduce_bwd: null pointer");
    DC_REQUIRE(gm != gy && (mode != 2 || (gm != m && gm != y && (const void *)gm != (const void *)cnt)),
               "dc_edge_reduce_bwd: gm must not alias an input");
    const bool v4 = C % 4 == 0 && ldgy % 4 == 0 && ldgm % 4 == 0 && al16(gy) && al16(gm) &&
                    (mode != 2 || (ldm % 4 == 0 && ldy % 4 == 0 && ldc % 4 == 0 && al16(m) && al16(y) && al16(cnt)));
    DC_EDGE_LAUNCH(k_edge_reduce_bwd, v4, E, C, stream, src, dst, ptr, m, ldm, y, ldy, cnt, ldc, gy, ldgy, gm, ldgm,
                   mode, N, E);
    return check_launch("dc_edge_reduce_bwd");
}
