// dc_gmm.hip -- GMMConv (MoNet; PyG 2.5.2 gmm_conv.py, separate_gaussians=False): a mixture of K Gaussians over the
// D-dimensional pseudo-coordinates of an edge weights K column blocks of the source row.
//
// h [N, K*M] (row stride ldh; column k*M + c is kernel k, channel c) are the node rows x @ g, a [E, D] (row stride
// lda) the pseudo-coordinates IN THE ORDER OF THE INPUT EDGES, mu / sigma [K, D] dense DEVICE arrays (trained
// parameters may change between two replays of a captured step).  The destination-sorted adjacency (ptr [N+1],
// other = source ids) carries perm = the input edge id of every sorted position, the transposed set (ptr_t / other_t =
// destination ids / perm_t) likewise.  The edge set is taken as it is given: no self loop is added, duplicates count, a
// row may have no edge.
//   weights   w[q,k]   = exp(e), e = 0, then for d = 0..D-1 in order e += (-0.5 * (t * t)) / (1e-15 + sigma[k,d]^2) with
//                        t = a[q,d] - mu[k,d]: torch's float32 operations in torch's order; one thread per (q, k), w in
//                        the order of the input edges.  sigma = 0 with a != mu: e is a large finite negative, w = 0.
//   forward   y[i,c]   = s = 0, then for p in [ptr[i], ptr[i+1]) in order, for k = 0..K-1 in order
//                        s += w[perm[p],k] * h[other[p], k*M + c] (the product rounded, then the add); mean: one division
//                        s / float(deg) where deg = ptr[i+1] - ptr[i] > 0; then s + base[i,c] (base NULL: none); then
//                        max(s, 0) with relu - a host loop in that order reproduces the bits
//   backward  gs[i,c]  = gy[i,c] / float(deg_i) (mean; one division per read, deg from the forward ptr), gy[i,c] (add)
//             g_h[j, k*M+c] = sum over the edges t out of j, in t order, of w[perm_t[t],k] * gs[other_t[t],c]
//             g_w[q,k] = sum_c gs[dst_q,c] * h[src_q, k*M + c]                          for every input edge q
//             g_mu[k,d] = sum_q t r,  g_sigma[k,d] = (sum_q t r r) sigma[k,d],  g_a[q,d] = -sum_k t r
//                        with t = g_w[q,k] w[q,k], r = (a[q,d] - mu[k,d]) / (1e-15 + sigma[k,d]^2)
//
// w is formed once per edge and SAVED for the backward (E*K floats); nothing else is saved but h, a and the graph.
// g_w walks the INPUT order: one lane group per input edge reads src_q / dst_q from the int64 edge list the adjacency
// was built from, every lane sums its own columns in column order, the lanes are combined by the fixed butterflies of
// dc_segment.h.  An edge with an endpoint outside [0, N) - the build skips and flags those - gets a zero row.
// The [K, D] sums: every workgroup sums a chunk of edges per (k, d) pair - the pair's lanes each a strided slice of the
// chunk, the slices combined in slice order through LDS - into a partial row of the workspace; a second launch adds
// the partial rows in chunk order.  No [E, K, D] temporary.  These sums, g_a and the dot products of g_w CANCEL (terms of
// either sign): they are formed in double - a product of two floats is exact there - and rounded to float32 once.
//
// Rules of the segment kernels (helpers: see dc_segment.h): fp contract(off), every sum in a fixed order, no float
// atomics, no host read - two runs give the same bits, and every entry can be captured.  Any M >= 1: 16-byte loads
// where M % 4 == 0 and every pointer and stride allows it, scalar loads otherwise; no width cap; any in-degree.
// Caps: 1 <= K <= 64 (DC_GMM_MAX_K), 1 <= D <= 16 (DC_GMM_MAX_D).
//
// Lanes as in dc_gine.hip: a row is served by a group of L lanes, L the power of two >= width / VEC within 4..64;
// 256 / L rows per workgroup.  The forward walks the (edge, kernel) pairs of a row as ONE sequence, U = 8 pairs in flight
// per lane (one gathered column block and one broadcast weight each: 8 x VEC + 8 registers) - the order p then k is the
// order of that sequence, whatever K is.  g_h is a row of width K*M: a lane's columns lie in one kernel k (M % VEC == 0),
// so per edge it reads one weight and one column block of gs, U = 4 edges in flight.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

constexpr int kPairsGm = 8;         // (edge, kernel) pairs in flight per lane of the forward
constexpr int kEdgesGm = 4;         // edges in flight per lane of g_h
constexpr int kKernelsGm = 4;       // kernels in flight per lane of g_w
constexpr float kGmmEps = 1e-15f;   // PyG's EPS

// ---- weights: one thread per (q, k) -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_gmm_weights(const float *__restrict__ a, int64_t lda, const float *__restrict__ mu, const float *__restrict__ sigma,
              float *__restrict__ w, int64_t E, int K, int D) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * K) return;
    const int64_t q = idx / K;
    const int k = (int)(idx - q * K);
    float e = 0.f;
    for (int d = 0; d < D; ++d) {
        const float t = a[q * lda + d] - mu[k * D + d];
        const float sg = sigma[k * D + d];
        const float den = kGmmEps + sg * sg;
        const float num = -0.5f * (t * t);
        e = e + num / den;
    }
    w[idx] = expf(e);
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_gmm_fwd(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const int32_t *__restrict__ perm,
          const float *__restrict__ w, const float *__restrict__ h, int64_t ldh, const float *__restrict__ base,
          int64_t ldb, float *__restrict__ y, int64_t ldy, int64_t N, int K, int mean, int relu, int M, int lg) {
    constexpr int U = kPairsGm;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    const int cnt = (end - beg) * K;                       // (edge, kernel) pairs of the row; E * K < 2^31 (entry)
    for (int c = sub * VEC; c < M; c += L * VEC) {
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        int pp = beg, kk = 0;
        for (int t = 0; t < cnt; t += U) {
            const int n = cnt - t;
            int64_t ho[U], wo[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t s = u < n ? other[pp] : 0;
                const int64_t q = u < n ? perm[pp] : 0;
                ho[u] = s * ldh + (int64_t)kk * M;
                wo[u] = q * K + kk;
                if (++kk == K) kk = 0, ++pp;
            }
            Cols<VEC> hv[U];
            float wv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                hv[u] = cols_load<VEC>(h + ho[u] + c, u < n);
                wv[u] = u < n ? w[wo[u]] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float m = wv[u] * hv[u].a[v];
                        acc[v] = acc[v] + m;
                    }
                }
        }
        if (mean && end > beg) {
            const float deg = (float)(end - beg);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / deg;
        }
        if (base) {
            const Cols<VEC> bv = cols_load<VEC>(base + row * ldb + c, true);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + bv.a[v];
        }
        if (relu) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = relu_keep_nan(acc[v]);
        }
        cols_store<VEC>(y + row * ldy + c, acc);
    }
}

// ---- backward in h: over the transposed set, a row of width K*M ------------------------------------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_gmm_bwd_h(const int32_t *__restrict__ ptr_t, const int32_t *__restrict__ other_t, const int32_t *__restrict__ perm_t,
            const int32_t *__restrict__ ptr, const float *__restrict__ w, const float *__restrict__ gy, int64_t ldgy,
            float *__restrict__ gh, int64_t ldgh, int64_t N, int K, int M, int KM, int lg) {
    constexpr int U = kEdgesGm;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr_t[row], end = ptr_t[row + 1];
    for (int cc = sub * VEC; cc < KM; cc += L * VEC) {
        const int k = cc / M, c = cc - k * M;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int64_t d[U], q[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = u < n ? other_t[p + u] : row;
                q[u] = u < n ? perm_t[p + u] : 0;
            }
            Cols<VEC> gv[U];
            float wv[U], deg[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                gv[u] = cols_load<VEC>(gy + d[u] * ldgy + c, u < n);
                wv[u] = u < n ? w[q[u] * K + k] : 0.f;
                deg[u] = ptr && u < n ? (float)(ptr[d[u] + 1] - ptr[d[u]]) : 1.f;     // (an edge into d: deg >= 1)
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float gs = ptr ? gv[u].a[v] / deg[u] : gv[u].a[v];
                        const float m = wv[u] * gs;
                        acc[v] = acc[v] + m;
                    }
                }
        }
        cols_store<VEC>(gh + row * ldgh + cc, acc);
    }
}

// ---- backward in w: one lane group per INPUT edge q; K dot products of gs[dst_q] with the column blocks of h[src_q] ------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_gmm_bwd_w(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, const int32_t *__restrict__ ptr,
            const float *__restrict__ h, int64_t ldh, const float *__restrict__ gy, int64_t ldgy,
            float *__restrict__ gw, int64_t N, int64_t E, int K, int M, int lg) {
    constexpr int U = kKernelsGm;
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
    for (int k0 = 0; k0 < K; k0 += U) {
        double s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = 0.0;
        for (int c = sub * VEC; c < M; c += L * VEC) {
            const Cols<VEC> gv = cols_load<VEC>(gy + i * ldgy + c, ok);
            Cols<VEC> hv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) hv[u] = cols_load<VEC>(h + j * ldh + (int64_t)(k0 + u) * M + c, ok && k0 + u < K);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const double gs = (double)(ptr ? gv.a[v] / deg : gv.a[v]);           // (the float32 gs of g_h)
#pragma unroll
                for (int u = 0; u < U; ++u) s[u] = s[u] + gs * (double)hv[u].a[v];    // (the product is exact)
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double tot = WAVE ? wave_sum(s[u]) : group_sum(s[u], L);
            if (sub == 0 && k0 + u < K) gw[q * K + k0 + u] = (float)tot;
        }
    }
}

// ---- backward in mu / sigma: partial sums per chunk of edges, then the chunks in order; all in double -------------------------
// PP = the power of two >= K*D (at most 256) lanes take a pair each, S = 256 / PP slices of the chunk side by side
__device__ __forceinline__ double gmm_r(float a, float mu, float sigma) {
    return ((double)a - (double)mu) / ((double)kGmmEps + (double)sigma * (double)sigma);
}

__global__ void __launch_bounds__(256)
k_gmm_params_partial(const float *__restrict__ gw, const float *__restrict__ w, const float *__restrict__ a, int64_t lda,
                     const float *__restrict__ mu, const float *__restrict__ sigma, double *__restrict__ partial,
                     int64_t E, int64_t chunk, int K, int D, int lgp) {
    __shared__ double red[2][256];
    const int P = K * D, PP = 1 << lgp, S = 256 >> lgp;
    const int pi = threadIdx.x & (PP - 1), slice = threadIdx.x >> lgp;
    const int64_t q0 = (int64_t)blockIdx.x * chunk;
    const int64_t q1 = q0 + chunk < E ? q0 + chunk : E;
    double *out = partial + (int64_t)blockIdx.x * 2 * P;
    for (int pr = pi; pr < P; pr += PP) {
        const int k = pr / D, d = pr - k * D;
        const float m = mu[pr], sg = sigma[pr];
        double s1 = 0.0, s2 = 0.0;
        for (int64_t q = q0 + slice; q < q1; q += S) {
            const double t = (double)gw[q * K + k] * (double)w[q * K + k];
            const double r = gmm_r(a[q * lda + d], m, sg);
            const double tr = t * r;
            s1 = s1 + tr;
            s2 = s2 + tr * r;
        }
        if (S == 1) out[pr] = s1, out[P + pr] = s2;        // (P > 128: a lane owns its pairs, nothing to combine)
        else red[0][threadIdx.x] = s1, red[1][threadIdx.x] = s2;
    }
    if (S == 1) return;                                    // (uniform over the workgroup)
    __syncthreads();
    if (slice == 0 && pi < P) {
        double s1 = 0.0, s2 = 0.0;
        for (int s = 0; s < S; ++s) {
            s1 = s1 + red[0][s * PP + pi];
            s2 = s2 + red[1][s * PP + pi];
        }
        out[pi] = s1, out[P + pi] = s2;
    }
}

__global__ void __launch_bounds__(256)
k_gmm_params_final(const double *__restrict__ partial, const float *__restrict__ sigma, float *__restrict__ gmu,
                   float *__restrict__ gsigma, int64_t nb, int P) {
    const int pr = blockIdx.x * 256 + threadIdx.x;
    if (pr >= P) return;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t b = 0; b < nb; ++b) {
        s1 = s1 + partial[b * 2 * P + pr];
        s2 = s2 + partial[b * 2 * P + P + pr];
    }
    gmu[pr] = (float)s1;
    gsigma[pr] = (float)(s2 * (double)sigma[pr]);
}

// ---- backward in a: one thread per (q, d) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_gmm_bwd_a(const float *__restrict__ gw, const float *__restrict__ w, const float *__restrict__ a, int64_t lda,
            const float *__restrict__ mu, const float *__restrict__ sigma, float *__restrict__ ga, int64_t ldga, int64_t E,
            int K, int D) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * D) return;
    const int64_t q = idx / D;
    const int d = (int)(idx - q * D);
    const float av = a[q * lda + d];
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        const double t = (double)gw[q * K + k] * (double)w[q * K + k];
        s = s + t * gmm_r(av, mu[k * D + d], sigma[k * D + d]);
    }
    ga[q * ldga + d] = (float)-s;
}

// edges per workgroup of the partial pass: at least 512, and at most kGmmMaxChunks chunks
constexpr int64_t kGmmMaxChunks = 1024;
inline int64_t gmm_chunk(int64_t E) {
    const int64_t c = (E + kGmmMaxChunks - 1) / kGmmMaxChunks;
    return c < 512 ? 512 : c;
}
inline int64_t gmm_chunks(int64_t E) { return E > 0 ? (E + gmm_chunk(E) - 1) / gmm_chunk(E) : 0; }

}  // namespace dc

using namespace dc;

#define DC_GMM_SHAPE(name, N, K, M)                                                                                  \
    DC_REQUIRE((N) >= 0 && (M) >= 1, name ": need N >= 0, M >= 1 (N=%lld M=%lld)", (long long)(N), (long long)(M)); \
    DC_REQUIRE((K) >= 1 && (K) <= DC_GMM_MAX_K, name ": need 1 <= K <= %d (K=%lld)", DC_GMM_MAX_K, (long long)(K)); \
    DC_REQUIRE(sizes_ok(N, (K) * (M)), name ": size out of range")
#define DC_GMM_EDGES(name, E, K)                                                                                     \
    DC_REQUIRE((E) >= 0 && (E) < (int64_t)INT32_MAX / 4 && (E) * (K) < (int64_t)INT32_MAX,                         \
               name ": E out of range (E=%lld K=%lld)", (long long)(E), (long long)(K))
#define DC_GMM_DIM(name, K, D)                                                                                       \
    DC_REQUIRE((K) >= 1 && (K) <= DC_GMM_MAX_K, name ": need 1 <= K <= %d (K=%lld)", DC_GMM_MAX_K, (long long)(K)); \
    DC_REQUIRE((D) >= 1 && (D) <= DC_GMM_MAX_D, name ": need 1 <= D <= %d (D=%lld)", DC_GMM_MAX_D, (long long)(D))

// the four forms of a kernel: 16-byte or scalar columns, one wave per row or 64 / L rows per wave (ROWS rows of width W)
#define DC_GMM_LAUNCH(kernel, v4, ROWS, W, stream, ...)                                                            \
    do {                                                                                                           \
        const int lg_ = log2_lanes((v4) ? (W) / 4 : (W));                                                       \
        const int64_t rows_ = 256 >> lg_;                                                                          \
        const dim3 grid_((unsigned)(((ROWS) + rows_ - 1) / rows_));                                                \
        if ((v4) && lg_ == 6) DC_LAUNCH((kernel<4, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);         \
        else if (v4) DC_LAUNCH((kernel<4, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);                 \
        else if (lg_ == 6) DC_LAUNCH((kernel<1, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);            \
        else DC_LAUNCH((kernel<1, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, lg_);                         \
    } while (0)

extern "C" int dc_gmm_weights(const float *a, int64_t lda, const float *mu, const float *sigma, float *w, int64_t E,
                              int64_t K, int64_t D, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GMM_DIM("dc_gmm_weights", K, D);
    DC_GMM_EDGES("dc_gmm_weights", E, K);
    DC_REQUIRE(lda >= D, "dc_gmm_weights: leading dimension smaller than D");
    if (E == 0) return DC_OK;
    DC_REQUIRE(a && mu && sigma && w, "dc_gmm_weights: null pointer");
    DC_REQUIRE(w != a && w != mu && w != sigma, "dc_gmm_weights: w must not alias an input");
    DC_LAUNCH(k_gmm_weights, dim3((unsigned)((E * K + 255) / 256)), dim3(256), 0, stream, a, lda, mu, sigma, w, E, (int)K,
              (int)D);
    return check_launch("dc_gmm_weights");
}

extern "C" int dc_gmm_fwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const float *w, const float *h,
                          int64_t ldh, const float *base, int64_t ldb, int mean, int relu, float *y, int64_t ldy,
                          int64_t N, int64_t E, int64_t K, int64_t M, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GMM_SHAPE("dc_gmm_fwd", N, K, M);
    DC_GMM_EDGES("dc_gmm_fwd", E, K);
    DC_REQUIRE(ldh >= K * M && ldy >= M && (!base || ldb >= M), "dc_gmm_fwd: leading dimension smaller than the width");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && perm && h && y && (w || E == 0), "dc_gmm_fwd: null pointer");
    DC_REQUIRE(y != h && y != w && y != base, "dc_gmm_fwd: y must not alias h, w or base");
    const bool v4 = M % 4 == 0 && ldh % 4 == 0 && ldy % 4 == 0 && al16(h) && al16(y) &&
                    (!base || (ldb % 4 == 0 && al16(base)));
    DC_GMM_LAUNCH(k_gmm_fwd, v4, N, M, stream, ptr, other, perm, w, h, ldh, base, ldb, y, ldy, N, (int)K, mean, relu,
                  (int)M);
    return check_launch("dc_gmm_fwd");
}

extern "C" int dc_gmm_bwd_h(const int32_t *ptr_t, const int32_t *other_t, const int32_t *perm_t, const int32_t *ptr,
                            const float *w, const float *gy, int64_t ldgy, float *gh, int64_t ldgh, int64_t N, int64_t E,
                            int64_t K, int64_t M, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GMM_SHAPE("dc_gmm_bwd_h", N, K, M);
    DC_GMM_EDGES("dc_gmm_bwd_h", E, K);
    DC_REQUIRE(ldgy >= M && ldgh >= K * M, "dc_gmm_bwd_h: leading dimension smaller than the width");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr_t && other_t && perm_t && gy && gh && (w || E == 0), "dc_gmm_bwd_h: null pointer");
    DC_REQUIRE(gh != gy && gh != w, "dc_gmm_bwd_h: gh must not alias an input");
    const bool v4 = M % 4 == 0 && ldgy % 4 == 0 && ldgh % 4 == 0 && al16(gy) && al16(gh);
    const int64_t KM = K * M;
    DC_GMM_LAUNCH(k_gmm_bwd_h, v4, N, KM, stream, ptr_t, other_t, perm_t, ptr, w, gy, ldgy, gh, ldgh, N, (int)K, (int)M,
                  (int)KM);
    return check_launch("dc_gmm_bwd_h");
}

extern "C" int dc_gmm_bwd_w(const int64_t *src, const int64_t *dst, const int32_t *ptr, const float *h, int64_t ldh,
                            const float *gy, int64_t ldgy, float *gw, int64_t N, int64_t E, int64_t K, int64_t M,
                            dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GMM_SHAPE("dc_gmm_bwd_w", N, K, M);
    DC_GMM_EDGES("dc_gmm_bwd_w", E, K);
    DC_REQUIRE(ldh >= K * M && ldgy >= M, "dc_gmm_bwd_w: leading dimension smaller than the width");
    if (E == 0) return DC_OK;
    DC_REQUIRE(src && dst && h && gy && gw, "dc_gmm_bwd_w: null pointer");
    DC_REQUIRE(gw != h && gw != gy, "dc_gmm_bwd_w: gw must not alias an input");
    const bool v4 = M % 4 == 0 && ldh % 4 == 0 && ldgy % 4 == 0 && al16(h) && al16(gy);
    DC_GMM_LAUNCH(k_gmm_bwd_w, v4, E, M, stream, src, dst, ptr, h, ldh, gy, ldgy, gw, N, E, (int)K, (int)M);
    return check_launch("dc_gmm_bwd_w");
}

extern "C" int64_t dc_gmm_params_workspace_bytes(int64_t E, int64_t K, int64_t D) {
    if (E <= 0 || K < 1 || D < 1) return 0;
    return gmm_chunks(E) * 2 * K * D * (int64_t)sizeof(double);
}

extern "C" int dc_gmm_bwd_params(const float *gw, const float *w, const float *a, int64_t lda, const float *mu,
                                 const float *sigma, void *workspace, int64_t workspace_bytes, float *gmu, float *gsigma,
                                 float *ga, int64_t ldga, int64_t E, int64_t K, int64_t D, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_GMM_DIM("dc_gmm_bwd_params", K, D);
    DC_GMM_EDGES("dc_gmm_bwd_params", E, K);
    DC_REQUIRE(lda >= D && (!ga || ldga >= D), "dc_gmm_bwd_params: leading dimension smaller than D");
    if (E == 0) return DC_OK;
    DC_REQUIRE(gw && w && a && mu && sigma && gmu && gsigma, "dc_gmm_bwd_params: null pointer");
    DC_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= dc_gmm_params_workspace_bytes(E, K, D),
               "dc_gmm_bwd_params: workspace too small or not 8-byte aligned");
    const void *ins[] = {gw, w, a, mu, sigma};
    for (const void *in : ins)
        DC_REQUIRE(gmu != in && gsigma != in && ga != in && workspace != in,
                   "dc_gmm_bwd_params: an output must not alias an input");
    DC_REQUIRE(gmu != gsigma && (void *)gmu != workspace && (void *)gsigma != workspace && (void *)ga != workspace &&
                   ga != gmu && ga != gsigma, "dc_gmm_bwd_params: the outputs must not alias each other");
    const int P = (int)(K * D);
    int lgp = 0;
    while (lgp < 8 && (1 << lgp) < P) ++lgp;
    const int64_t nb = gmm_chunks(E);
    DC_LAUNCH(k_gmm_params_partial, dim3((unsigned)nb), dim3(256), 0, stream, gw, w, a, lda, mu, sigma,
              (double *)workspace, E, gmm_chunk(E), (int)K, (int)D, lgp);
    DC_LAUNCH(k_gmm_params_final, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, (const double *)workspace, sigma,
              gmu, gsigma, nb, P);
    if (ga)
        DC_LAUNCH(k_gmm_bwd_a, dim3((unsigned)((E * D + 255) / 256)), dim3(256), 0, stream, gw, w, a, lda, mu, sigma, ga,
                  ldga, E, (int)K, (int)D);
    return check_launch("dc_gmm_bwd_params");
}
