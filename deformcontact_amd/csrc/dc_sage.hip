// dc_sage.hip -- SAGEConv (PyG 2.5.2 sage_conv.py): the MEAN and the MAX over a node's in-edges and their backward.
//
// Segment reductions of x [N, F] (row stride ldx) over the destination-sorted adjacency (ptr [N+1], other = source
// ids), the backward over the transposed set (ptr_t / other_t: row j holds the destinations of the edges out of j):
//   mean  y[i,c]   = (sum over the edges p into i, in p order, of x[other[p],c]) / float(deg_i),  deg_i = ptr[i+1]-ptr[i]
//         g_x[j,c] = sum over the edges t out of j, in t order, of g_y[i_t,c] / float(deg_{i_t})
//   max   m[i,c]   = max over the edges into i of x[other[p],c];  cnt[i,c] = number of those edges that attain it
//         g_x[j,c] = sum over the edges t out of j, in t order, of (x[j,c] == m[i_t,c]) g_m[i_t,c] / float(cnt[i_t,c])
// A row without edges is 0 (m = 0, cnt = 0).  The sum is the plain fp32 sum of the unweighted hop (dc_spmm.hip: 1 * v
// added in p order), so mean == hop / deg bit for bit; the division is a true (correctly rounded) division.  The max
// backward splits the gradient EVENLY among all edges that attain the maximum, duplicates each counting as an edge;
// the comparison is exact - m is a copy of one of the gathered values - so no index image is kept.  Non-finite
// inputs (INTEGRATION.md "Non-finite values"): the maximum is a selection, so +-Inf candidates are ordinary values and the
// forward equals scatter_reduce(..., 'amax') exactly; a NaN candidate makes m[i,c] NaN, as there, and cnt[i,c] the number
// of NaN candidates (max_step, dc_common.h).  The sums and the mean carry NaN / Inf as fp32 addition does, into the
// rows and columns that depend on them and no others.  The backward of a non-finite forward is not specified; on a finite
// forward a non-finite g_m[i,c] reaches exactly the edges that attain m[i,c].
//
// Rules of the segment kernels (helpers: see dc_segment.h): every sum in a fixed order (the backward sums compensated), no
// float atomics, no host read - two runs give the same bits.  Any F >= 1: 16-byte loads where F % 4 == 0 and every pointer
// and stride allows it, scalar loads otherwise; no width cap (columns in chunks of the lane group); any in-degree.
//
// Lanes: a row is served by a group of L lanes, L the power of two >= F / VEC within 4..64; 256 / L rows per
// workgroup.  L = 64 is the one-wave-per-row form of the hop (row, segment bounds and ids wave-uniform: scalar loads);
// narrower rows pack 64 / L rows into a wave as k_spmm_sub does.  U edges are in flight per lane before the first is
// consumed.  No lane reads what another lane wrote and there is no cross-lane step.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

constexpr int kEdgesSg = 8;        // rows in flight per lane: one gathered array per edge (mean, max forward)
constexpr int kEdgesSgBwd = 4;     // the max backward gathers three arrays per edge

}  // namespace

// ---- mean, forward ---------------------------------------------------------------------------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_sage_mean_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ x,
                int64_t ldx, float *__restrict__ y, int64_t ldy, int64_t N, int F, int lg) {
    constexpr int U = kEdgesSg;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    const float deg = (float)(end - beg);
    for (int c = sub * VEC; c < F; c += L * VEC) {
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t s[U];
            Cols<VEC> v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = u < n ? other[p + u] : row;
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = cols_load<VEC>(x + s[u] * ldx + c, u < n);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + v[u].a[k];
                }
        }
        if (end > beg) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] / deg;
        }
        cols_store<VEC>(y + row * ldy + c, acc);
    }
}

// ---- mean, backward: over the transposed set, the destination's in-degree from the forward ptr ---------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_sage_mean_bwd(const int32_t *__restrict__ ptr_t, const int32_t *__restrict__ other_t,
                const int32_t *__restrict__ ptr, const float *__restrict__ gy, int64_t ldgy, float *__restrict__ gx,
                int64_t ldgx, int64_t N, int F, int lg) {
    constexpr int U = kEdgesSg;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr_t[row], end = ptr_t[row + 1];
    for (int c = sub * VEC; c < F; c += L * VEC) {
        float acc[VEC], cmp[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f, cmp[k] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t s[U];
            float d[U];
            Cols<VEC> v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = u < n ? other_t[p + u] : row;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = u < n ? (float)(ptr[s[u] + 1] - ptr[s[u]]) : 1.f;
                v[u] = cols_load<VEC>(gy + s[u] * ldgy + c, u < n);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) kahan_add(acc[k], cmp[k], v[u].a[k] / d[u]);
                }
        }
        cols_store<VEC>(gx + row * ldgx + c, acc);
    }
}

// ---- max, forward: maximum and the number of edges that attain it, in one walk ---------------------------------------
// greater: the maximum is replaced and the count starts again at 1; equal: one more.  cnt == nullptr: not stored.
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_sage_max_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ x,
               int64_t ldx, float *__restrict__ m, int64_t ldm, int32_t *__restrict__ cnt, int64_t ldc, int64_t N,
               int F, int lg) {
    constexpr int U = kEdgesSg;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    for (int c = sub * VEC; c < F; c += L * VEC) {
        float mx[VEC];
        int ct[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) mx[k] = -INFINITY, ct[k] = 0;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t s[U];
            Cols<VEC> v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = u < n ? other[p + u] : row;
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = cols_load<VEC>(x + s[u] * ldx + c, u < n);
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
        cols_store<VEC>(m + row * ldm + c, mx);
        if (cnt) ints_store<VEC>(cnt + row * ldc + c, ct);
    }
}

// ---- max, backward: over the transposed set; the even split among the edges that attain the maximum ------------------
// x[j,c] is read once per source row and column; per edge the destination's m, cnt and g_m rows are gathered.  Where
// x[j,c] == m[i,c] the edge j -> i is one of the cnt[i,c] >= 1 that attain it.
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_sage_max_bwd(const int32_t *__restrict__ ptr_t, const int32_t *__restrict__ other_t, const float *__restrict__ x,
               int64_t ldx, const float *__restrict__ m, int64_t ldm, const int32_t *__restrict__ cnt, int64_t ldc,
               const float *__restrict__ gm, int64_t ldgm, float *__restrict__ gx, int64_t ldgx, int64_t N, int F,
               int lg) {
    constexpr int U = kEdgesSgBwd;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr_t[row], end = ptr_t[row + 1];
    for (int c = sub * VEC; c < F; c += L * VEC) {
        const Cols<VEC> xj = cols_load<VEC>(x + row * ldx + c, true);
        float acc[VEC], cmp[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f, cmp[k] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t s[U];
            Cols<VEC> mv[U], gv[U];
            Ints<VEC> cv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = u < n ? other_t[p + u] : row;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                mv[u] = cols_load<VEC>(m + s[u] * ldm + c, u < n);
                cv[u] = ints_load<VEC>(cnt + s[u] * ldc + c, u < n);
                gv[u] = cols_load<VEC>(gm + s[u] * ldgm + c, u < n);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const bool hit = xj.a[k] == mv[u].a[k] && cv[u].a[k] > 0;
                        const float share = gv[u].a[k] / (float)(hit ? cv[u].a[k] : 1);
                        kahan_add(acc[k], cmp[k], hit ? share : 0.f);
                    }
                }
        }
        cols_store<VEC>(gx + row * ldgx + c, acc);
    }
}

}  // namespace dc

using namespace dc;

#define DC_SAGE_SHAPE(name, N, F)                                                                                  \
    DC_REQUIRE((N) >= 0 && (F) >= 1, name ": need N >= 0, F >= 1 (N=%lld F=%lld)", (long long)(N), (long long)(F)); \
    DC_REQUIRE(sizes_ok(N, F), name ": size out of range")

// the four forms of a kernel: 16-byte or scalar columns, one wave per row or 64 / L rows per wave
#define DC_SAGE_LAUNCH(kernel, v4, N, F, stream, ...)                                                              \
    do {                                                                                                           \
        const int lg_ = log2_lanes((v4) ? (F) / 4 : (F));                                                       \
        const int64_t rows_ = 256 >> lg_;                                                                          \
        const dim3 grid_((unsigned)(((N) + rows_ - 1) / rows_));                                                   \
        if ((v4) && lg_ == 6) DC_LAUNCH((kernel<4, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, N, (int)(F), lg_); \
        else if (v4) DC_LAUNCH((kernel<4, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, N, (int)(F), lg_);    \
        else if (lg_ == 6) DC_LAUNCH((kernel<1, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, N, (int)(F), lg_); \
        else DC_LAUNCH((kernel<1, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, N, (int)(F), lg_);            \
    } while (0)

extern "C" int dc_sage_mean_fwd(const int32_t *ptr, const int32_t *other, const float *x, int64_t ldx, float *y,
                                int64_t ldy, int64_t N, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SAGE_SHAPE("dc_sage_mean_fwd", N, F);
    DC_REQUIRE(ldx >= F && ldy >= F, "dc_sage_mean_fwd: leading dimension smaller than F");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && x && y, "dc_sage_mean_fwd: null pointer");
    DC_REQUIRE(y != x, "dc_sage_mean_fwd: y must not alias x");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y);
    DC_SAGE_LAUNCH(k_sage_mean_fwd, v4, N, F, stream, ptr, other, x, ldx, y, ldy);
    return check_launch("dc_sage_mean_fwd");
}

extern "C" int dc_sage_mean_bwd(const int32_t *ptr_t, const int32_t *other_t, const int32_t *ptr, const float *gy,
                                int64_t ldgy, float *gx, int64_t ldgx, int64_t N, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SAGE_SHAPE("dc_sage_mean_bwd", N, F);
    DC_REQUIRE(ldgy >= F && ldgx >= F, "dc_sage_mean_bwd: leading dimension smaller than F");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr_t && other_t && ptr && gy && gx, "dc_sage_mean_bwd: null pointer");
    DC_REQUIRE(gx != gy, "dc_sage_mean_bwd: gx must not alias gy");
    const bool v4 = F % 4 == 0 && ldgy % 4 == 0 && ldgx % 4 == 0 && al16(gy) && al16(gx);
    DC_SAGE_LAUNCH(k_sage_mean_bwd, v4, N, F, stream, ptr_t, other_t, ptr, gy, ldgy, gx, ldgx);
    return check_launch("dc_sage_mean_bwd");
}

extern "C" int dc_sage_max_fwd(const int32_t *ptr, const int32_t *other, const float *x, int64_t ldx, float *m,
                               int64_t ldm, int32_t *cnt, int64_t ldc, int64_t N, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SAGE_SHAPE("dc_sage_max_fwd", N, F);
    DC_REQUIRE(ldx >= F && ldm >= F && (!cnt || ldc >= F), "dc_sage_max_fwd: leading dimension smaller than F");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && x && m, "dc_sage_max_fwd: null pointer");
    DC_REQUIRE(m != x && (const void *)cnt != (const void *)x && (const void *)cnt != (const void *)m,
               "dc_sage_max_fwd: m / cnt must not alias x or each other");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldm % 4 == 0 && al16(x) && al16(m) &&
                    (!cnt || (ldc % 4 == 0 && al16(cnt)));
    DC_SAGE_LAUNCH(k_sage_max_fwd, v4, N, F, stream, ptr, other, x, ldx, m, ldm, cnt, ldc);
    return check_launch("dc_sage_max_fwd");
}

extern "C" int dc_sage_max_bwd(const int32_t *ptr_t, const int32_t *other_t, const float *x, int64_t ldx,
                               const float *m, int64_t ldm, const int32_t *cnt, int64_t ldc, const float *gm,
                               int64_t ldgm, float *gx, int64_t ldgx, int64_t N, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SAGE_SHAPE("dc_sage_max_bwd", N, F);
    DC_REQUIRE(ldx >= F && ldm >= F && ldc >= F && ldgm >= F && ldgx >= F,
               "dc_sage_max_bwd: leading dimension smaller than F");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr_t && other_t && x && m && cnt && gm && gx, "dc_sage_max_bwd: null pointer");
    DC_REQUIRE(gx != x && gx != m && gx != gm && (const void *)gx != (const void *)cnt,
               "dc_sage_max_bwd: gx must not alias an input");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldm % 4 == 0 && ldc % 4 == 0 && ldgm % 4 == 0 && ldgx % 4 == 0 &&
                    al16(x) && al16(m) && al16(cnt) && al16(gm) && al16(gx);
    DC_SAGE_LAUNCH(k_sage_max_bwd, v4, N, F, stream, ptr_t, other_t, x, ldx, m, ldm, cnt, ldc, gm, ldgm, gx, ldgx);
    return check_launch("dc_sage_max_bwd");
}
