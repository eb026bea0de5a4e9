// dc_spline.hip -- SplineConv (SplineCNN; PyG 2.5.2 spline_conv.py with torch-spline-conv's basis and weighting): an open
// or closed B-spline of degree 1..3 over the D-dimensional pseudo-coordinates of an edge picks S = (degree+1)^D of the K
// column blocks of the source row and weights them.
//
// h [N, K*M] (row stride ldh; column k*M + c is weight matrix k, channel c) are the node rows x @ weight[k], a [E, D]
// (row stride lda) the pseudo-coordinates IN THE ORDER OF THE INPUT EDGES.  ks[d] (the kernel size of dimension d),
// open[d] and degree are HOST values copied into the kernel arguments; nothing of them is read from the device.  The
// destination-sorted adjacency (ptr [N+1], other = source ids) carries perm = the input edge id of every sorted
// position, the transposed set (ptr_t / other_t = destination ids / perm_t) likewise.  The edge set is taken as it is
// given: no self loop is added, duplicates count, a row may have no edge.
//   basis     for slot s in 0..S-1, with k = s, wi = 0, off = 1, bv = 1, for d = 0..D-1 in order:
//               k_mod = k % (degree+1), k /= degree+1;  v = a[q,d] * float(ks[d] - degree*open[d]) (one float32 product)
//               wi += ((floor(v) + k_mod) mod ks[d]) * off, off *= ks[d];  bv *= B_degree(v - floor(v), k_mod)
//             the modulo is the non-negative one of floor(v) clamped to +-2^30 (NaN: 0), so 0 <= wi < K whatever a holds;
//             b [E, S] float32 and wi [E, S] int32 in the order of the input edges, one thread per (q, s)
//   forward   y[i,c]   = acc = 0, then for p in [ptr[i], ptr[i+1]) in order: the edge's message t = 0, for s = 0..S-1 in
//                        order t += b[perm[p],s] * h[other[p], wi[perm[p],s]*M + c] (the product rounded, then the add),
//                        then acc += t - the message first, then the sum over the edges, as the contract writes it; mean:
//                        one division acc / float(deg) where deg = ptr[i+1] - ptr[i] > 0; then acc + base[i,c] (base NULL:
//                        none); then max(acc, 0) with relu - a host loop in that order reproduces the bits
//   backward  gs[i,c]  = gy[i,c] / float(deg_i) (mean; one division per read, deg from the forward ptr), gy[i,c] (add)
//             g_h[j, k*M+c] = sum over the edges t out of j, in t order, and the slots s with wi[perm_t[t],s] == k, in s
//                        order, of b[perm_t[t],s] * gs[other_t[t],c]; a column no slot names is written as 0
//             g_b[q,s] = sum_c gs[dst_q,c] * h[src_q, wi[q,s]*M + c]                     for every input edge q
//             g_a[q,d] = float(ks[d] - degree*open[d]) * sum_s g_b[q,s] B'(f_d, k_mod_d) prod_{d' != d} B(f_d', k_mod_d')
//
// b and wi are formed once per edge and SAVED for the backward (2 E S words).  g_h: a lane owns columns of ONE weight
// matrix k (M % VEC == 0) and scans the S slot indices of each of its row's edges for k; the gradient row of the edge's
// destination is loaded only for an edge with a hit.  g_b walks the INPUT order as dc_gmm_bwd_w does: one lane group per
// input edge, dot products in double (a product of two floats is exact there), the lanes combined by the fixed
// butterflies of dc_segment.h; an edge with an endpoint outside [0, N) gets a zero row.  g_a is a sum of terms of either
// sign: formed in double from the float32 fraction and rounded once.
//
// Rules of the segment kernels (helpers: see dc_segment.h): fp contract(off), every sum in a fixed order, no float
// atomics, no host read - two runs give the same bits, and every entry can be captured.  Any M >= 1: 16-byte loads
// where M % 4 == 0 and every pointer and stride allows it, scalar loads otherwise.
// Caps: 1 <= D <= 4 (DC_SPLINE_MAX_D), S <= 64 (DC_SPLINE_MAX_S), ks[d] >= 1, K <= 1024 (DC_SPLINE_MAX_K), E*S < 2^31,
// N*K*M < 2^31.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

constexpr int kPairsSp = 8;         // (edge, slot) pairs in flight per lane of the forward
constexpr int kSlotsSp = 4;         // slots in flight per lane of g_b

// the host values of a layer, by value in the kernel arguments
struct SplineGeom {
    int ks[DC_SPLINE_MAX_D];
    int mult[DC_SPLINE_MAX_D];      // ks[d] - degree * open[d]
    int D, degree;
};

// B_degree(f, k) and its derivative in f, in T = float (the basis) or double (g_a); the operations in the order written
template <class T>
__device__ __forceinline__ T spline_b(int degree, T f, int k) {
    if (degree == 1) return (((T)1 - f) - (T)k) + (((T)2 * f) * (T)k);
    if (degree == 2) {
        if (k == 0) return (((T)0.5 * f) * f - f) + (T)0.5;
        if (k == 1) return (f - f * f) + (T)0.5;
        return ((T)0.5 * f) * f;
    }
    if (k == 0) {
        const T g = (T)1 - f;
        return ((g * g) * g) / (T)6;
    }
    if (k == 1) return ((((T)3 * f) * f) * f - (((T)6 * f) * f) + (T)4) / (T)6;
    if (k == 2) return (((((T)3 * f) * f - (((T)3 * f) * f) * f) + (T)3 * f) + (T)1) / (T)6;
    return ((f * f) * f) / (T)6;
}
__device__ __forceinline__ double spline_db(int degree, double f, int k) {
    if (degree == 1) return 2.0 * (double)k - 1.0;
    if (degree == 2) return k == 0 ? f - 1.0 : (k == 1 ? 1.0 - 2.0 * f : f);
    if (k == 0) return (2.0 * f - f * f - 1.0) / 2.0;
    if (k == 1) return (3.0 * f * f - 4.0 * f) / 2.0;
    if (k == 2) return (2.0 * f + 1.0 - 3.0 * f * f) / 2.0;
    return f * f / 2.0;
}
// floor(v) as an int the modulo can take: clamped to +-2^30, NaN: 0
__device__ __forceinline__ int spline_cell(float fl) {
    const float lim = 1073741824.f;
    if (!(fl == fl)) return 0;
    return (int)(fl < -lim ? -lim : (fl > lim ? lim : fl));
}

// ---- basis: one thread per (q, s) -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_spline_basis(const float *__restrict__ a, int64_t lda, SplineGeom gm, float *__restrict__ b, int32_t *__restrict__ wi,
               int64_t E, int S) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * S) return;
    const int64_t q = idx / S;
    int k = (int)(idx - q * S);
    const int dp = gm.degree + 1;
    int w = 0, off = 1;
    float bv = 1.f;
    for (int d = 0; d < gm.D; ++d) {
        const int k_mod = k % dp;
        k /= dp;
        const float v = a[q * lda + d] * (float)gm.mult[d];
        const float fl = floorf(v);
        int r = (spline_cell(fl) + k_mod) % gm.ks[d];
        if (r < 0) r += gm.ks[d];
        w += r * off;
        off *= gm.ks[d];
        bv = bv * spline_b<float>(gm.degree, v - fl, k_mod);
    }
    b[idx] = bv;
    wi[idx] = w;
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_spline_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const int32_t *__restrict__ perm,
             const float *__restrict__ b, const int32_t *__restrict__ wi, const float *__restrict__ h, int64_t ldh,
             const float *__restrict__ base, int64_t ldb, float *__restrict__ y, int64_t ldy, int64_t N, int S, int mean,
             int relu, int M, int lg) {
    constexpr int U = kPairsSp;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    const int cnt = (end - beg) * S;                       // (edge, slot) pairs of the row; E * S < 2^31 (entry)
    for (int c = sub * VEC; c < M; c += L * VEC) {
        float acc[VEC], msg[VEC];                          // the row's sum; the message of the edge being walked
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f, msg[v] = 0.f;
        int pp = beg, ss = 0;
        for (int t = 0; t < cnt; t += U) {
            const int n = cnt - t;
            int64_t src[U], bo[U];
            bool last[U];                                  // the edge's last slot: its message joins the row's sum
#pragma unroll
            for (int u = 0; u < U; ++u) {
                src[u] = u < n ? other[pp] : 0;
                const int64_t q = u < n ? perm[pp] : 0;
                bo[u] = q * S + ss;
                last[u] = ss == S - 1;
                if (++ss == S) ss = 0, ++pp;
            }
            float bv[U];
            int64_t ho[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bv[u] = u < n ? b[bo[u]] : 0.f;
                ho[u] = src[u] * ldh + (int64_t)(u < n ? wi[bo[u]] : 0) * M;
            }
            Cols<VEC> hv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) hv[u] = cols_load<VEC>(h + ho[u] + c, u < n);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float m = bv[u] * hv[u].a[v];
                        msg[v] = msg[v] + m;
                        if (last[u]) acc[v] = acc[v] + msg[v], msg[v] = 0.f;
                    }
                }
        }
        if (mean && end > beg) {
            const float deg = (float)(end - beg);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / deg;
        }
        if (base) {
            const Cols<VEC> av = cols_load<VEC>(base + row * ldb + c, true);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + av.a[v];
        }
        if (relu) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = relu_keep_nan(acc[v]);
        }
        cols_store<VEC>(y + row * ldy + c, acc);
    }
}

// ---- backward in h: over the transposed set, a row of width K*M; a lane scans its edges' slots for its own k ---------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_spline_bwd_h(const int32_t *__restrict__ ptr_t, const int32_t *__restrict__ other_t, const int32_t *__restrict__ perm_t,
               const int32_t *__restrict__ ptr, const float *__restrict__ b, const int32_t *__restrict__ wi,
               const float *__restrict__ gy, int64_t ldgy, float *__restrict__ gh, int64_t ldgh, int64_t N, int S, int M,
               int KM, int lg) {
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr_t[row], end = ptr_t[row + 1];
    for (int cc = sub * VEC; cc < KM; cc += L * VEC) {
        const int k = cc / M, c = cc - k * M;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int p = beg; p < end; ++p) {
            const int64_t qs = (int64_t)perm_t[p] * S;
            unsigned long long hit = 0;                    // (S <= 64: one bit per slot)
            for (int s = 0; s < S; ++s) hit |= (unsigned long long)(wi[qs + s] == k) << s;
            if (!hit) continue;
            const int64_t d = other_t[p];
            const Cols<VEC> gv = cols_load<VEC>(gy + d * ldgy + c, true);
            float gs[VEC];
            if (ptr) {
                const float deg = (float)(ptr[d + 1] - ptr[d]);                    // (an edge into d: deg >= 1)
#pragma unroll
                for (int v = 0; v < VEC; ++v) gs[v] = gv.a[v] / deg;
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) gs[v] = gv.a[v];
            }
            for (int s = 0; s < S; ++s)
                if ((hit >> s) & 1ull) {
                    const float bv = b[qs + s];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float m = bv * gs[v];
                        acc[v] = acc[v] + m;
                    }
                }
        }
        cols_store<VEC>(gh + row * ldgh + cc, acc);
    }
}

// ---- backward in b: one lane group per INPUT edge q; S dot products of gs[dst_q] with the named column blocks of h[src_q] --
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_spline_bwd_b(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const int32_t *__restrict__ ptr,
               const int32_t *__restrict__ wi, const float *__restrict__ h, int64_t ldh, const float *__restrict__ gy,
               int64_t ldgy, float *__restrict__ gb, int64_t N, int64_t E, int S, int M, int lg) {
    constexpr int U = kSlotsSp;
    int64_t q;
    int sub, L;
    if (!seg_row<WAVE>(lg, E, q, sub, L)) return;
    const int64_t j = src[q], i = dst[q];
    const bool ok = j >= 0 && j < N && i >= 0 && i < N;          // (an edge the build skipped: a zero row)
    float deg = 1.f;
    if (ptr && ok) {
        const int dg = ptr[i + 1] - ptr[i];
        deg = dg > 0 ? (float)dg : 1.f;
    }
    for (int s0 = 0; s0 < S; s0 += U) {
        double t[U];
        int64_t ho[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            t[u] = 0.0;
            ho[u] = ok && s0 + u < S ? j * ldh + (int64_t)wi[q * S + s0 + u] * M : 0;
        }
        for (int c = sub * VEC; c < M; c += L * VEC) {
            const Cols<VEC> gv = cols_load<VEC>(gy + i * ldgy + c, ok);
            Cols<VEC> hv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) hv[u] = cols_load<VEC>(h + ho[u] + c, ok && s0 + u < S);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const double gs = (double)(ptr ? gv.a[v] / deg : gv.a[v]);           // (the float32 gs of g_h)
#pragma unroll
                for (int u = 0; u < U; ++u) t[u] = t[u] + gs * (double)hv[u].a[v];    // (the product is exact)
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double tot = WAVE ? wave_sum(t[u]) : group_sum(t[u], L);
            if (sub == 0 && s0 + u < S) gb[q * S + s0 + u] = (float)tot;
        }
    }
}

// ---- backward in a: one thread per (q, d) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_spline_bwd_a(const float *__restrict__ gb, const float *__restrict__ a, int64_t lda, SplineGeom gm,
               float *__restrict__ ga, int64_t ldga, int64_t E, int S) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * gm.D) return;
    const int64_t q = idx / gm.D;
    const int d = (int)(idx - q * gm.D);
    const int dp = gm.degree + 1;
    double f[DC_SPLINE_MAX_D];
#pragma unroll
    for (int e = 0; e < DC_SPLINE_MAX_D; ++e) {
        f[e] = 0.0;
        if (e < gm.D) {
            const float v = a[q * lda + e] * (float)gm.mult[e];
            f[e] = (double)(v - floorf(v));                // (the float32 fraction of the basis)
        }
    }
    double tot = 0.0;
    for (int s = 0; s < S; ++s) {
        int k = s;
        double term = (double)gb[q * S + s];
#pragma unroll
        for (int e = 0; e < DC_SPLINE_MAX_D; ++e)
            if (e < gm.D) {
                const int k_mod = k % dp;
                k /= dp;
                term = term * (e == d ? spline_db(gm.degree, f[e], k_mod) : spline_b<double>(gm.degree, f[e], k_mod));
            }
        tot = tot + term;
    }
    double mult = 0.0;
#pragma unroll
    for (int e = 0; e < DC_SPLINE_MAX_D; ++e)
        if (e == d) mult = (double)(float)gm.mult[e];
    ga[q * ldga + d] = (float)(mult * tot);
}

// (degree+1)^D, or 0 where D or degree is out of range
inline int64_t spline_slots(int64_t D, int64_t degree) {
    if (D < 1 || D > DC_SPLINE_MAX_D || degree < 1 || degree > 3) return 0;
    int64_t s = 1;
    for (int64_t d = 0; d < D; ++d) s *= degree + 1;
    return s;
}

}  // namespace dc

using namespace dc;

// D, degree and S; then E
#define DC_SPLINE_DIM(name, D, degree)                                                                               \
    DC_REQUIRE((D) >= 1 && (D) <= DC_SPLINE_MAX_D, name ": need 1 <= D <= %d (D=%lld)", DC_SPLINE_MAX_D,            \
               (long long)(D));                                                                                      \
    DC_REQUIRE((degree) >= 1 && (degree) <= 3, name ": need 1 <= degree <= 3 (degree=%lld)", (long long)(degree));  \
    DC_REQUIRE(spline_slots(D, degree) <= DC_SPLINE_MAX_S, name ": need S = (degree+1)^D <= %d (S=%lld)",            \
               DC_SPLINE_MAX_S, (long long)spline_slots(D, degree))
#define DC_SPLINE_EDGES(name, E, S)                                                                                  \
    DC_REQUIRE((E) >= 0 && (E) < (int64_t)INT32_MAX / 4 && (E) * (S) < (int64_t)INT32_MAX,                         \
               name ": E out of range (E=%lld S=%lld)", (long long)(E), (long long)(S))
#define DC_SPLINE_SHAPE(name, N, S, K, M)                                                                            \
    DC_REQUIRE((N) >= 0 && (M) >= 1, name ": need N >= 0, M >= 1 (N=%lld M=%lld)", (long long)(N), (long long)(M)); \
    DC_REQUIRE((S) >= 1 && (S) <= DC_SPLINE_MAX_S, name ": need 1 <= S <= %d (S=%lld)", DC_SPLINE_MAX_S,            \
               (long long)(S));                                                                                      \
    DC_REQUIRE((K) >= 1 && (K) <= DC_SPLINE_MAX_K, name ": need 1 <= K <= %d (K=%lld)", DC_SPLINE_MAX_K,            \
               (long long)(K));                                                                                      \
    DC_REQUIRE((M) < (1 << 24) && sizes_ok(N, (K) * (M)) && (N) * (K) * (M) < (int64_t)INT32_MAX,                  \
               name ": size out of range (N*K*M must stay below 2^31)")

// the host values of a layer into the kernels' argument; the entries have checked D, degree and the pointers
#define DC_SPLINE_GEOM(name, gm, ks, open, D, degree)                                                                \
    SplineGeom gm;                                                                                                   \
    do {                                                                                                             \
        int64_t K_ = 1;                                                                                              \
        for (int d_ = 0; d_ < DC_SPLINE_MAX_D; ++d_) gm.ks[d_] = 1, gm.mult[d_] = 1;                                 \
        for (int d_ = 0; d_ < (int)(D); ++d_) {                                                                      \
            DC_REQUIRE((ks)[d_] >= 1, name ": need ks[d] >= 1 (ks[%d]=%lld)", d_, (long long)(ks)[d_]);              \
            K_ *= (ks)[d_];                                                                                          \
            DC_REQUIRE(K_ <= DC_SPLINE_MAX_K, name ": need K = prod ks[d] <= %d", DC_SPLINE_MAX_K);                  \
            gm.ks[d_] = (int)(ks)[d_];                                                                               \
            gm.mult[d_] = (int)(ks)[d_] - (int)(degree) * ((open)[d_] ? 1 : 0);                                      \
        }                                                                                                            \
        gm.D = (int)(D), gm.degree = (int)(degree);                                                                  \
    } while (0)

// the four forms of a kernel: 16-byte or scalar columns, one wave per row or 64 / L rows per wave (ROWS rows of width W)
#define DC_SPLINE_LAUNCH(kernel, v4, ROWS, W, stream, ...)                                                         \
    do {                                                                                                           \
        const int lg_ = log2_lanes((v4) ? (W) / 4 : (W));                                                       \
        const int64_t rows_ = 256 >> lg_;                                                                          \
        const dim3 grid_((unsigned)(((ROWS) + rows_ - 1) / rows_));                                                \
        if ((v4) && lg_ == 6) DC_LAUNCH((kernel<4, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);         \
        else if (v4) DC_LAUNCH((kernel<4, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);                 \
        else if (lg_ == 6) DC_LAUNCH((kernel<1, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);            \
        else DC_LAUNCH((kernel<1, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);                         \
    } while (0)

extern "C" int dc_spline_basis(const float *a, int64_t lda, const int64_t *ks, const int32_t *open, int64_t degree,
                               float *b, int32_t *wi, int64_t E, int64_t D, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SPLINE_DIM("dc_spline_basis", D, degree);
    const int64_t S = spline_slots(D, degree);
    DC_SPLINE_EDGES("dc_spline_basis", E, S);
    DC_REQUIRE(lda >= D, "dc_spline_basis: leading dimension smaller than D");
    if (E == 0) return DC_OK;
    DC_REQUIRE(a && ks && open && b && wi, "dc_spline_basis: null pointer");
    DC_SPLINE_GEOM("dc_spline_basis", gm, ks, open, D, degree);
    DC_REQUIRE((const void *)b != a && (const void *)wi != a && (void *)b != (void *)wi,
               "dc_spline_basis: b and wi must not alias a or each other");
    DC_LAUNCH(k_spline_basis, dim3((unsigned)((E * S + 255) / 256)), dim3(256), 0, stream, a, lda, gm, b, wi, E, (int)S);
    return check_launch("dc_spline_basis");
}

extern "C" int dc_spline_fwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const float *b,
                             const int32_t *wi, const float *h, int64_t ldh, const float *base, int64_t ldb, int mean,
                             int relu, float *y, int64_t ldy, int64_t N, int64_t E, int64_t S, int64_t K, int64_t M,
                             dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SPLINE_SHAPE("dc_spline_fwd", N, S, K, M);
    DC_SPLINE_EDGES("dc_spline_fwd", E, S);
    DC_REQUIRE(ldh >= K * M && ldy >= M && (!base || ldb >= M), "dc_spline_fwd: leading dimension smaller than the width");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && perm && h && y && ((b && wi) || E == 0), "dc_spline_fwd: null pointer");
    DC_REQUIRE(y != h && y != b && (const void *)y != wi && y != base, "dc_spline_fwd: y must not alias h, b, wi or base");
    const bool v4 = M % 4 == 0 && ldh % 4 == 0 && ldy % 4 == 0 && al16(h) && al16(y) &&
                    (!base || (ldb % 4 == 0 && al16(base)));
    DC_SPLINE_LAUNCH(k_spline_fwd, v4, N, M, stream, ptr, other, perm, b, wi, h, ldh, base, ldb, y, ldy, N, (int)S, mean,
                     relu, (int)M);
    return check_launch("dc_spline_fwd");
}

extern "C" int dc_spline_bwd_h(const int32_t *ptr_t, const int32_t *other_t, const int32_t *perm_t, const int32_t *ptr,
                               const float *b, const int32_t *wi, const float *gy, int64_t ldgy, float *gh, int64_t ldgh,
                               int64_t N, int64_t E, int64_t S, int64_t K, int64_t M, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SPLINE_SHAPE("dc_spline_bwd_h", N, S, K, M);
    DC_SPLINE_EDGES("dc_spline_bwd_h", E, S);
    DC_REQUIRE(ldgy >= M && ldgh >= K * M, "dc_spline_bwd_h: leading dimension smaller than the width");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr_t && other_t && perm_t && gy && gh && ((b && wi) || E == 0), "dc_spline_bwd_h: null pointer");
    DC_REQUIRE(gh != gy && gh != b && (const void *)gh != wi, "dc_spline_bwd_h: gh must not alias an input");
    const bool v4 = M % 4 == 0 && ldgy % 4 == 0 && ldgh % 4 == 0 && al16(gy) && al16(gh);
    const int64_t KM = K * M;
    DC_SPLINE_LAUNCH(k_spline_bwd_h, v4, N, KM, stream, ptr_t, other_t, perm_t, ptr, b, wi, gy, ldgy, gh, ldgh, N, (int)S,
                     (int)M, (int)KM);
    return check_launch("dc_spline_bwd_h");
}

extern "C" int dc_spline_bwd_b(const int64_t *src, const int64_t *dst, const int32_t *ptr, const int32_t *wi,
                               const float *h, int64_t ldh, const float *gy, int64_t ldgy, float *gb, int64_t N, int64_t E,
                               int64_t S, int64_t K, int64_t M, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SPLINE_SHAPE("dc_spline_bwd_b", N, S, K, M);
    DC_SPLINE_EDGES("dc_spline_bwd_b", E, S);
    DC_REQUIRE(ldh >= K * M && ldgy >= M, "dc_spline_bwd_b: leading dimension smaller than the width");
    if (E == 0) return DC_OK;
    DC_REQUIRE(src && dst && wi && h && gy && gb, "dc_spline_bwd_b: null pointer");
    DC_REQUIRE(gb != h && gb != gy && (const void *)gb != wi, "dc_spline_bwd_b: gb must not alias an input");
    const bool v4 = M % 4 == 0 && ldh % 4 == 0 && ldgy % 4 == 0 && al16(h) && al16(gy);
    DC_SPLINE_LAUNCH(k_spline_bwd_b, v4, E, M, stream, src, dst, ptr, wi, h, ldh, gy, ldgy, gb, N, E, (int)S, (int)M);
    return check_launch("dc_spline_bwd_b");
}

extern "C" int dc_spline_bwd_a(const float *gb, const float *a, int64_t lda, const int64_t *ks, const int32_t *open,
                               int64_t degree, float *ga, int64_t ldga, int64_t E, int64_t D, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_SPLINE_DIM("dc_spline_bwd_a", D, degree);
    const int64_t S = spline_slots(D, degree);
    DC_SPLINE_EDGES("dc_spline_bwd_a", E, S);
    DC_REQUIRE(lda >= D && ldga >= D, "dc_spline_bwd_a: leading dimension smaller than D");
    if (E == 0) return DC_OK;
    DC_REQUIRE(gb && a && ks && open && ga, "dc_spline_bwd_a: null pointer");
    DC_SPLINE_GEOM("dc_spline_bwd_a", gm, ks, open, D, degree);
    DC_REQUIRE(ga != gb && ga != a, "dc_spline_bwd_a: ga must not alias an input");
    DC_LAUNCH(k_spline_bwd_a, dim3((unsigned)((E * D + 255) / 256)), dim3(256), 0, stream, gb, a, lda, gm, ga, ldga, E,
              (int)S);
    return check_launch("dc_spline_bwd_a");
}
