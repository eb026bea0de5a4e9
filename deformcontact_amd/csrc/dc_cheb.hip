// dc_cheb.hip -- ChebConv (PyG 2.5.2 cheb_conv.py + get_laplacian): the scaled Laplacian's weights and one step of the
// Chebyshev recurrence as a single hop launch.
//
// The operator.  Edges j -> i of the set AS GIVEN (a GraphIndex built with self_loops=False, normalize=False); a slot
// whose two ends coincide gets weight 0 - that is how the self loop is removed - and is not counted in a degree.
//   deg[j] = number of non-loop slots of the by-SOURCE segment of j (get_laplacian scatters on edge_index[0])
//   sym: dinv[j] = deg[j]^-1/2 (deg = 0 -> 0),  w = dinv[src] * dinv[dst]          rw: dinv[j] = 1 / deg[j],  w = dinv[src]
//   wl = (2 * -w) / lam        - in this order: the product of the two dinv, the negation, the doubling, ONE division
//   L^ x_i = sum_p wl_p x_{src(p)} + b x_i,   b = 2 / lam - 1 for every node
// dc_cheb_norm writes wl for BOTH orientations - wl_fwd per slot of the by-destination set (forward hops), wl_bwd per slot
// of the by-source set (the adjoint recurrence of the backward) - in two launches (dinv, then the weights), no atomics.
//
// The step (dc_cheb_hop), over row-major column views with a leading dimension each:
//   s = 0;  for p in [ptr[i], ptr[i+1]) in p order:  s += wl[p] * x[other[p]]     (product and sum rounded separately)
//   t = s + b * x[i]
//   y[i]  = k * t + c * z[i]       k in {1, 2}, c in {-1, 0, +1}; c = 0: z is not read and y = k * t
//   y2[i] = z2[i] - x[i]           (optional)
// y may be z and y2 may be z2 (the same lane reads the element before it writes it); neither may be x, whose rows other
// rows gather.  Tx_1 = L^ x is (k, c) = (1, 0); Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2} is (2, -1); the backward's
// G_{k-1} += 2 L^T G_k with G_{k-2} -= G_k as the second output is (2, +1); G_0 += L^T G_1 is (1, +1).
//
// Rules of the segment kernels (helpers: dc_segment.h): fixed order, no float atomics, no host read - two runs give the
// same bits.  Lanes as dc_sage.hip: a row is served by L lanes, L the power of two >= F / VEC within 4..64; L = 64 is the
// one-wave-per-row form of the hop (row, bounds, ids and weights wave-uniform: scalar loads), narrower rows pack 64 / L
// rows into a wave; 16-byte accesses where F % 4 == 0 and every pointer and stride allows it; U neighbour rows in
// flight before the first is consumed; logical blocks handed to the XCDs in contiguous chunks (xcd_remap).
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

constexpr int kEdgesCheb = 8;      // neighbour rows in flight per lane
constexpr int kNormLanes = 8;      // lanes per row of the two passes of dc_cheb_norm

}  // namespace

// ---- dinv[j] from the by-source set: non-loop slots counted by kNormLanes lanes, an integer sum (any order) ------------
__global__ void __launch_bounds__(256)
k_cheb_dinv(const int32_t *__restrict__ ptr_t, const int32_t *__restrict__ other_t, float *__restrict__ dinv, int64_t N,
            int rw) {
    const int64_t row = (int64_t)blockIdx.x * (256 / kNormLanes) + threadIdx.x / kNormLanes;
    const int sub = threadIdx.x % kNormLanes;
    const bool live = row < N;                       // (every lane stays for the cross-lane sum)
    int cnt = 0;
    if (live)
        for (int p = ptr_t[row] + sub, end = ptr_t[row + 1]; p < end; p += kNormLanes) cnt += other_t[p] != row ? 1 : 0;
    cnt = sub_sum<kNormLanes>(cnt);
    if (live && sub == 0) dinv[row] = rw ? (cnt > 0 ? 1.0f / (float)cnt : 0.0f) : inv_sqrt_count(cnt);
}

// ---- the weights of both orientations: rows [0, N) the by-destination set, rows [N, 2N) the by-source set ------------
__global__ void __launch_bounds__(256)
k_cheb_weights(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const int32_t *__restrict__ ptr_t,
               const int32_t *__restrict__ other_t, const float *__restrict__ dinv, float lam, int rw,
               float *__restrict__ wl_fwd, float *__restrict__ wl_bwd, int64_t N) {
    int64_t row = (int64_t)blockIdx.x * (256 / kNormLanes) + threadIdx.x / kNormLanes;
    const int sub = threadIdx.x % kNormLanes;
    if (row >= 2 * N) return;
    const bool fwd = row < N;
    if (!fwd) row -= N;
    const int32_t *p_ = fwd ? ptr : ptr_t, *o_ = fwd ? other : other_t;
    float *out = fwd ? wl_fwd : wl_bwd;
    const float dr = dinv[row];
    for (int p = p_[row] + sub, end = p_[row + 1]; p < end; p += kNormLanes) {
        const int64_t o = o_[p];
        // the source of the slot: `other` in the by-destination set, the row itself in the by-source set
        const float ds = fwd ? dinv[o] : dr, dd = fwd ? dr : dinv[o];
        const float w = rw ? ds : ds * dd;
        const float m = -w;
        const float d = 2.0f * m;
        out[p] = o == row ? 0.0f : d / lam;
    }
}

// ---- one recurrence step ---------------------------------------------------------------------------------------------
// SGPR budget of the wave form (MI355X_MICROARCH.md "Residency": a 256-thread block is admitted 8 per CU up to 80 SGPRs):
// the five views come as pointer + stride pairs; k and c arrive as floats, the optional operands as null pointers, so
// nothing but the kernel arguments and the row's bounds is wave-uniform state.  With U ids, weights and row addresses on
// top the wave form asks for ~106; the attribute caps the allocation as k_spmm_wave's does (the surplus lives in VGPR
// lanes, of which the kernel uses 53), the lane-group forms stay below it on their own.
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80)))
k_cheb_hop(const int32_t *__restrict__ ptr, const int32_t *__restrict__ other, const float *__restrict__ wl,
           const float *__restrict__ x, int64_t ldx, const float *z, int64_t ldz, float *y, int64_t ldy, const float *z2,
           int64_t ldz2, float *y2, int64_t ldy2, float b, float kf, float cf, int64_t N, int F, int lg) {
    constexpr int U = kEdgesCheb;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, N, row, sub, L)) return;
    const int beg = ptr[row], end = ptr[row + 1];
    for (int c = sub * VEC; c < F; c += L * VEC) {
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int p = beg; p < end; p += U) {
            const int n = end - p;
            int s[U];
            float ww[U];
            Cols<VEC> v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = u < n ? other[p + u] : (int)row;
                ww[u] = u < n ? wl[p + u] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = cols_load<VEC>(x + (int64_t)s[u] * ldx + c, u < n);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < n) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float m = ww[u] * v[u].a[k];
                        acc[k] = acc[k] + m;
                    }
                }
        }
        const Cols<VEC> xi = cols_load<VEC>(x + row * ldx + c, true);
        Cols<VEC> zi, z2i;
        if (z) zi = cols_load<VEC>(z + row * ldz + c, true);
        if (y2) z2i = cols_load<VEC>(z2 + row * ldz2 + c, true);
        float r[VEC], r2[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float d = b * xi.a[k];
            const float t = acc[k] + d;
            r[k] = kf * t;
            if (z) {
                const float e = cf * zi.a[k];
                r[k] = r[k] + e;
            }
            if (y2) r2[k] = z2i.a[k] - xi.a[k];
        }
        cols_store<VEC>(y + row * ldy + c, r);
        if (y2) cols_store<VEC>(y2 + row * ldy2 + c, r2);
    }
}

}  // namespace dc

using namespace dc;

extern "C" int dc_cheb_norm(const int32_t *ptr, const int32_t *other, const int32_t *ptr_t, const int32_t *other_t,
                            int rw, float lam, float *dinv, float *wl_fwd, float *wl_bwd, int64_t N,
                            dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(N >= 0, "dc_cheb_norm: need N >= 0 (N=%lld)", (long long)N);
    DC_REQUIRE(sizes_ok(2 * N, 1), "dc_cheb_norm: size out of range");
    DC_REQUIRE(rw == 0 || rw == 1, "dc_cheb_norm: mode must be 0 (sym) or 1 (rw), got %d", rw);
    DC_REQUIRE(lam > 0.f, "dc_cheb_norm: lambda_max must be > 0");      // (a NaN fails too)
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && ptr_t && other_t && dinv && wl_fwd && wl_bwd, "dc_cheb_norm: null pointer");
    DC_REQUIRE(wl_fwd != wl_bwd && dinv != wl_fwd && dinv != wl_bwd, "dc_cheb_norm: the outputs must not alias");
    constexpr int64_t rows = 256 / kNormLanes;
    DC_LAUNCH(k_cheb_dinv, dim3((unsigned)((N + rows - 1) / rows)), dim3(256), 0, stream, ptr_t, other_t, dinv, N, rw);
    DC_LAUNCH(k_cheb_weights, dim3((unsigned)((2 * N + rows - 1) / rows)), dim3(256), 0, stream, ptr, other, ptr_t,
              other_t, dinv, lam, rw, wl_fwd, wl_bwd, N);
    return check_launch("dc_cheb_norm");
}

extern "C" int dc_cheb_hop(const int32_t *ptr, const int32_t *other, const float *wl, const float *x, int64_t ldx,
                           const float *z, int64_t ldz, float *y, int64_t ldy, const float *z2, int64_t ldz2, float *y2,
                           int64_t ldy2, float b, int k, int c, int64_t N, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(N >= 0 && F >= 1, "dc_cheb_hop: need N >= 0, F >= 1 (N=%lld F=%lld)", (long long)N, (long long)F);
    DC_REQUIRE(sizes_ok(N, F), "dc_cheb_hop: size out of range");
    DC_REQUIRE((k == 1 || k == 2) && c >= -1 && c <= 1, "dc_cheb_hop: k must be 1 or 2 and c -1, 0 or +1 (k=%d c=%d)", k,
               c);
    DC_REQUIRE(ldx >= F && ldy >= F && (c == 0 || ldz >= F) && (!y2 || (ldz2 >= F && ldy2 >= F)),
               "dc_cheb_hop: leading dimension smaller than F");
    if (N == 0) return DC_OK;
    DC_REQUIRE(ptr && other && wl && x && y && (c == 0 || z) && (!y2 || z2), "dc_cheb_hop: null pointer");
    DC_REQUIRE(y != x && y2 != x && y2 != y,
               "dc_cheb_hop: y / y2 must not alias x or each other (y may be z, y2 may be z2)");
    if (c == 0) z = nullptr;
    // the 16-byte form: every view that is touched starts on 16 bytes and keeps its rows there
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y) && (!z || (ldz % 4 == 0 && al16(z))) &&
                    (!y2 || (ldz2 % 4 == 0 && ldy2 % 4 == 0 && al16(z2) && al16(y2)));
    const int lg = log2_lanes(v4 ? F / 4 : F);
    const int64_t rows = 256 >> lg;
    const dim3 grid((unsigned)((N + rows - 1) / rows));
    const float kf = (float)k, cf = (float)c;
#define DC_CHEB_ARGS ptr, other, wl, x, ldx, z, ldz, y, ldy, z2, ldz2, y2, ldy2, b, kf, cf, N, (int)F, lg
    if (v4 && lg == 6) DC_LAUNCH((k_cheb_hop<4, true>), grid, dim3(256), 0, stream, DC_CHEB_ARGS);
    else if (v4) DC_LAUNCH((k_cheb_hop<4, false>), grid, dim3(256), 0, stream, DC_CHEB_ARGS);
    else if (lg == 6) DC_LAUNCH((k_cheb_hop<1, true>), grid, dim3(256), 0, stream, DC_CHEB_ARGS);
    else DC_LAUNCH((k_cheb_hop<1, false>), grid, dim3(256), 0, stream, DC_CHEB_ARGS);
#undef DC_CHEB_ARGS
    return check_launch("dc_cheb_hop");
}
