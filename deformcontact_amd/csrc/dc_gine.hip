// dc_gine.hip -- GINEConv (PyG 2.5.2 gin_conv.py): the sum over a node's in-edges of relu(x_j + e_ji), the root term
// (1 + eps) x_i, and the backward in x and in e.
//
// x [N, F] (row stride ldx) are the node rows, e [E, F] (row stride lde) the edge rows IN THE ORDER OF THE INPUT EDGES:
// the destination-sorted adjacency (ptr [N+1], other = source ids) carries perm = the input edge id of every sorted
// position, the transposed set (ptr_t / other_t = destination ids / perm_t) likewise.  The edge set is taken as it is
// given - no self loop is added, duplicates count, a row may have no edge - so perm is a bijection over the E input edges.
//   forward   y[i,c]   = (1 + eps) x[i,c] + s,  s = 0, then for p in [ptr[i], ptr[i+1]) in order
//                        s += max(x[other[p],c] + e[perm[p],c], 0): plain fp32 adds; 1 + eps is formed first (fp32), then
//                        the product, then the add of s - a host loop in that order reproduces the bits
//   backward  g_x[j,c] = (1 + eps) g_y[j,c] + sum over the edges t out of j, in t order, of
//                        (x[j,c] + e[perm_t[t],c] > 0) g_y[other_t[t],c]         (the sum compensated)
//             g_e[q,c] = (x[src_q,c] + e[q,c] > 0) g_y[dst_q,c]                  for every input edge q
// The ReLU mask is RECOMPUTED in the backward from the same fp32 add of the same two numbers - the same bits as the
// forward - so nothing is saved but x, e and the graph; relu'(0) = 0.  eps is a DEVICE pointer to one float (a trained
// parameter may change between two replays of a captured step); NULL: no root term (y = s, g_x = the sum).
//
// g_e walks the INPUT order: one lane group per input edge q reads src_q / dst_q from the int64 edge list the
// adjacency was built from, so e and g_e stream (row q in, row q out) and only x[src_q] and g_y[dst_q] are gathered;
// every row of g_e is written exactly once, by one lane group.  An edge with an endpoint outside [0, N) - the build
// skips and flags those - gets a zero row.
//
// Rules of the segment kernels (helpers: see dc_segment.h): fp contract(off), every sum in a fixed order, no float
// atomics, no host read - two runs give the same bits, and every entry can be captured.  Any F >= 1: 16-byte loads
// where F % 4 == 0 and every pointer and stride allows it, scalar loads otherwise; no width cap (columns in chunks of
// the lane group); any in-degree.
//
// Lanes as in dc_sage.hip (seg_row, dc_segment.h): a row (of x, or of e for g_e) is served by a group of L lanes, L the
// power of two >= F / VEC within 4..64; 256 / L rows per workgroup; L = 64 is the one-wave-per-row form (row, segment bounds and ids wave-uniform).
// U edges are in flight per lane before the first is consumed (two gathered rows per edge: U = 4).  No lane reads what
// another lane wrote and there is no cross-lane step.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

constexpr int kEdgesGn = 4;        // edges in flight per lane: two gathered rows per edge (x / g_y and e)

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_gine_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const int32_t *__restrict__ perm,
           const float *__restrict__ x, int64_t ldx, const float *__restrict__ e, int64_t lde,
           const float *__restrict__ eps, float *__restrict__ y, int64_t ldy, int64_t N, int F, int lg) {
    constexpr int U = kEdgesGn;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    const float ope = eps ? 1.f + *eps : 0.f;
    for (int c = sub * VEC; c < F; c += L * VEC) {
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t s[U], q[U];
            Cols<VEC> xv[U], ev[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = u < n ? other[p + u] : row;
                q[u] = u < n ? perm[p + u] : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                xv[u] = cols_load<VEC>(x + s[u] * ldx + c, u < n);
                ev[u] = cols_load<VEC>(e + q[u] * lde + c, u < n);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float m = xv[u].a[k] + ev[u].a[k];
                        acc[k] = acc[k] + relu_keep_nan(m);
                    }
                }
        }
        if (eps) {
            const Cols<VEC> xi = cols_load<VEC>(x + row * ldx + c, true);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float r = ope * xi.a[k];
                acc[k] = r + acc[k];
            }
        }
        cols_store<VEC>(y + row * ldy + c, acc);
    }
}

// ---- backward in x: over the transposed set; x[j,c] is read once per row and column, per edge e's row and g_y's ----------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_gine_bwd_x(const int32_t *__restrict__ ptr_t, const int32_t *__restrict__ other_t, const int32_t *__restrict__ perm_t,
             const float *__restrict__ x, int64_t ldx, const float *__restrict__ e, int64_t lde,
             const float *__restrict__ eps, const float *__restrict__ gy, int64_t ldgy, float *__restrict__ gx,
             int64_t ldgx, int64_t N, int F, int lg) {
    constexpr int U = kEdgesGn;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr_t[row], end = ptr_t[row + 1];
    const float ope = eps ? 1.f + *eps : 0.f;
    for (int c = sub * VEC; c < F; c += L * VEC) {
        const Cols<VEC> xj = cols_load<VEC>(x + row * ldx + c, true);
        float acc[VEC], cmp[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f, cmp[k] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t d[U], q[U];
            Cols<VEC> gv[U], ev[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = u < n ? other_t[p + u] : row;
                q[u] = u < n ? perm_t[p + u] : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                gv[u] = cols_load<VEC>(gy + d[u] * ldgy + c, u < n);
                ev[u] = cols_load<VEC>(e + q[u] * lde + c, u < n);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float m = xj.a[k] + ev[u].a[k];
                        kahan_add(acc[k], cmp[k], m > 0.f ? gv[u].a[k] : 0.f);
                    }
                }
        }
        if (eps) {
            const Cols<VEC> gj = cols_load<VEC>(gy + row * ldgy + c, true);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float r = ope * gj.a[k];
                acc[k] = r + acc[k];
            }
        }
        cols_store<VEC>(gx + row * ldgx + c, acc);
    }
}

// ---- backward in e: one lane group per INPUT edge q; e and g_e stream, x[src_q] and g_y[dst_q] are gathered ---------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_gine_bwd_e(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const float *__restrict__ x, int64_t ldx,
             const float *__restrict__ e, int64_t lde, const float *__restrict__ gy, int64_t ldgy,
             float *__restrict__ ge, int64_t ldge, int64_t N, int64_t E, int F, int lg) {
    int64_t q;
    int sub, L;
    if (!seg_row<WAVE>(lg, E, q, sub, L)) return;
    const int64_t j = src[q], i = dst[q];
    const bool ok = j >= 0 && j < N && i >= 0 && i < N;          // (an edge the build skipped: a zero row)
    for (int c = sub * VEC; c < F; c += L * VEC) {
        const Cols<VEC> xv = cols_load<VEC>(x + j * ldx + c, ok);
        const Cols<VEC> ev = cols_load<VEC>(e + q * lde + c, ok);
        const Cols<VEC> gv = cols_load<VEC>(gy + i * ldgy + c, ok);
        float out[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float m = xv.a[k] + ev.a[k];
            out[k] = ok && m > 0.f ? gv.a[k] : 0.f;
        }
        cols_store<VEC>(ge + q * ldge + c, out);
    }
}

}  // namespace dc

using namespace dc;

#define DC_GINE_SHAPE(name, N, F)                                                                                  \
    DC_REQUIRE((N) >= 0 && (F) >= 1, name ": need N >= 0, F >= 1 (N=%lld F=%lld)", (long long)(N), (long long)(F)); \
    DC_REQUIRE(sizes_ok(N, F), name ": size out of range")

// the four forms of a kernel: 16-byte or scalar columns, one wave per row or 64 / L rows per wave (ROWS rows in all)
#define DC_GINE_LAUNCH(kernel, v4, ROWS, F, stream, ...)                                                           \
    do {                                                                                                           \
        const int lg_ = log2_lanes((v4) ? (F) / 4 : (F));                                                       \
        const int64_t rows_ = 256 >> lg_;                                                                          \
        const dim3 grid_((unsigned)(((ROWS) + rows_ - 1) / rows_));                                                \
        if ((v4) && lg_ == 6) DC_LAUNCH((kernel<4, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_); \
        else if (v4) DC_LAUNCH((kernel<4, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);       \
        else if (lg_ == 6) DC_LAUNCH((kernel<1, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);  \
        else DC_LAUNCH((kernel<1, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);               \
    } while (0)

extern "C" int dc_gine_fwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const float *x, int64_t ldx,
                           const float *e, int64_t lde, const float *eps, float *y, int64_t ldy, int64_t N, int64_t F,
                           dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GINE_SHAPE("dc_gine_fwd", N, F);
    DC_REQUIRE(ldx >= F && lde >= F && ldy >= F, "dc_gine_fwd: leading dimension smaller than F");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && perm && x && e && y, "dc_gine_fwd: null pointer");
    DC_REQUIRE(y != x && y != e, "dc_gine_fwd: y must not alias x or e");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && lde % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(e) && al16(y);
    DC_GINE_LAUNCH(k_gine_fwd, v4, N, F, stream, ptr, other, perm, x, ldx, e, lde, eps, y, ldy, N);
    return check_launch("dc_gine_fwd");
}

extern "C" int dc_gine_bwd_x(const int32_t *ptr_t, const int32_t *other_t, const int32_t *perm_t, const float *x,
                             int64_t ldx, const float *e, int64_t lde, const float *eps, const float *gy, int64_t ldgy,
                             float *gx, int64_t ldgx, int64_t N, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GINE_SHAPE("dc_gine_bwd_x", N, F);
    DC_REQUIRE(ldx >= F && lde >= F && ldgy >= F && ldgx >= F, "dc_gine_bwd_x: leading dimension smaller than F");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr_t && other_t && perm_t && x && e && gy && gx, "dc_gine_bwd_x: null pointer");
    DC_REQUIRE(gx != x && gx != e && gx != gy, "dc_gine_bwd_x: gx must not alias an input");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && lde % 4 == 0 && ldgy % 4 == 0 && ldgx % 4 == 0 && al16(x) &&
                    al16(e) && al16(gy) && al16(gx);
    DC_GINE_LAUNCH(k_gine_bwd_x, v4, N, F, stream, ptr_t, other_t, perm_t, x, ldx, e, lde, eps, gy, ldgy, gx, ldgx, N);
    return check_launch("dc_gine_bwd_x");
}

extern "C" int dc_gine_bwd_e(const int64_t *src, const int64_t *dst, const float *x, int64_t ldx, const float *e,
                             int64_t lde, const float *gy, int64_t ldgy, float *ge, int64_t ldge, int64_t N, int64_t E,
                             int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GINE_SHAPE("dc_gine_bwd_e", N, F);
    DC_REQUIRE(E >= 0 && sizes_ok(E, F), "dc_gine_bwd_e: E out of range (E=%lld)", (long long)E);
    DC_REQUIRE(ldx >= F && lde >= F && ldgy >= F && ldge >= F, "dc_gine_bwd_e: leading dimension smaller than F");
    if (E == 0) return DC_OK;
    DC_REQUIRE(src && dst && x && e && gy && ge, "dc_gine_bwd_e: null pointer");
    DC_REQUIRE(ge != x && ge != e && ge != gy, "dc_gine_bwd_e: ge must not alias an input");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && lde % 4 == 0 && ldgy % 4 == 0 && ldge % 4 == 0 && al16(x) &&
                    al16(e) && al16(gy) && al16(ge);
    DC_GINE_LAUNCH(k_gine_bwd_e, v4, E, F, stream, src, dst, x, ldx, e, lde, gy, ldgy, ge, ldge, N, E);
    return check_launch("dc_gine_bwd_e");
}
