// dc_pointops.hip -- the two point-set functions that go with knn / radius in a PointNet++ model (PyG 2.5.2: fps,
// knn_interpolate): farthest point sampling, and the inverse-squared-distance transfer of node rows from one point set
// onto another over the padded neighbour array of dc_neighbors.hip.
//
// Distances are those of the neighbour search: d2 = ((dx*dx + dy*dy) + dz*dz) in fp32, every product and sum rounded on
// its own.  Inputs are taken to be finite.
//
//   fps, per graph with the nodes [a, a+n), m picks, start s (all block-uniform):
//     dist[j] = +inf; c = s; out[0] = a + s
//     for t = 1 .. m-1:  dist[j] = min(dist[j], d2(j, c)) for every j;  c = the j with the largest dist[j], the LOWEST j
//                        among equals;  out[t] = a + c
//     Once every distinct point is taken all distances are 0 and the rule keeps returning the graph's first node.
//     One workgroup per graph.  Every thread runs the same m-1 iterations and meets the same barrier once in each; a
//     workgroup leaves only as a whole (a graph without nodes or without picks), before its first barrier.
//     The argmax orders the keys (bits of dist, ~j): dist >= 0, so its bit pattern orders as an unsigned integer, and
//     the larger ~j is the lower j.  Per wave: four DPP steps inside every row of 16 lanes, then the four rows through
//     scalar registers (no LDS round trip); the lane that owns the wave's key writes key and position to the wave's LDS
//     slot; after one barrier every thread reads the (at most 16) slots and takes the largest.  Two sets of slots
//     alternate, so one barrier per pick is enough: a slot is written again two picks later, after a barrier that every
//     reader of the older value has passed.
//     k_fps_resident<PER>: a thread keeps PER points (position and running minimum) in registers for the whole chain;
//     up to 1024 x 8 = DC_FPS_RESIDENT_POINTS points per graph.  k_fps_stream: any size; (x, y, z, dist) as 16 bytes per
//     point in a global workspace, one 16-byte load per point and pick (eight in flight per thread) and a 4-byte store
//     where the distance fell; a thread reads and writes its own points only, so no fence is needed.  A launch takes
//     ONE of the two for all its graphs, by the largest.
//
//   knn_interpolate, forward, one lane group per query i, ranks r < counts[i], j = nbr[i*k + r]:
//     w = 1.0f / max(d2(pos_x[j], pos_y[i]), 1e-16f) (a true division); num[c] = num[c] + w * x[j,c] and den = den + w in
//     rank order from 0 (product and sum rounded separately); y[i,c] = num[c] / den; a query without a neighbour gets a
//     row of zeros.  w [Ny, k] (0 in the padding) and den [Ny] are written for the backward when asked for.
//   backward, one lane group per source row j: the slots s = i*k + r with nbr[s] == j come as a by-source list
//     (ptr [Nx+1] into slots, ascending s inside a row); gx[j,c] = the compensated sum, in that order, of
//     w[s] * (gy[i,c] / den[i]).  A source that no query selected gets a zero row.
//
// Rules of the segment kernels (dc_segment.h): fp contract(off), every sum in a fixed order, no float atomics, no host
// read - two runs give the same bits, and every entry can be captured.
#include "dc_segment.h"

#pragma clang fp contract(off)

namespace dc {

namespace {

constexpr int kFpsThreads = 1024;                              // the largest workgroup
constexpr int kFpsWaves = kFpsThreads / kWave;
constexpr int kFpsPer = 8;                                     // points per thread of the widest resident form
constexpr int64_t kFpsResident = DC_FPS_RESIDENT_POINTS;
static_assert(kFpsResident == (int64_t)kFpsThreads * kFpsPer, "DC_FPS_RESIDENT_POINTS is 1024 threads x 8 points");

constexpr int kFpsInFlight = 8;                               // points in flight per thread of the workspace kernel
constexpr int kSlotsPi = 4;                                    // neighbour rows in flight per lane (knn_interpolate)

struct FpsSlots {                                              // [2]: the two alternating sets
    uint32_t hi[2][kFpsWaves];
    uint32_t lo[2][kFpsWaves];
    float p[2][kFpsWaves][3];
};

// the larger of two keys (hi, lo)
__device__ __forceinline__ void key_max(uint32_t &hi, uint32_t &lo, uint32_t oh, uint32_t ol) {
    const bool take = oh > hi || (oh == hi && ol > lo);
    hi = take ? oh : hi, lo = take ? ol : lo;
}

// a lane's value as another lane of its row of 16 holds it (DPP: a register move, no LDS round trip)
template <int CTRL>
__device__ __forceinline__ uint32_t row_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}

// the wave's largest key, in every lane.  All 64 lanes are active.  Inside a row of 16: lane ^ 1, lane ^ 2 (quad_perm),
// then the mirror of the 8 (the other quad) and of the 16 (the other 8) - after each step the group of 2, 4, 8, 16 lanes
// agrees on its maximum; the four rows meet through scalar registers.  The maximum does not depend on the order.
__device__ __forceinline__ void wave_key_max(uint32_t &hi, uint32_t &lo) {
    key_max(hi, lo, row_dpp<0xB1>(hi), row_dpp<0xB1>(lo));         // quad_perm [1, 0, 3, 2]
    key_max(hi, lo, row_dpp<0x4E>(hi), row_dpp<0x4E>(lo));         // quad_perm [2, 3, 0, 1]
    key_max(hi, lo, row_dpp<0x141>(hi), row_dpp<0x141>(lo));       // row_half_mirror
    key_max(hi, lo, row_dpp<0x140>(hi), row_dpp<0x140>(lo));       // row_mirror
    uint32_t mh = (uint32_t)__builtin_amdgcn_readlane((int)hi, 0), ml = (uint32_t)__builtin_amdgcn_readlane((int)lo, 0);
    key_max(mh, ml, (uint32_t)__builtin_amdgcn_readlane((int)hi, 16), (uint32_t)__builtin_amdgcn_readlane((int)lo, 16));
    key_max(mh, ml, (uint32_t)__builtin_amdgcn_readlane((int)hi, 32), (uint32_t)__builtin_amdgcn_readlane((int)lo, 32));
    key_max(mh, ml, (uint32_t)__builtin_amdgcn_readlane((int)hi, 48), (uint32_t)__builtin_amdgcn_readlane((int)lo, 48));
    hi = mh, lo = ml;
}

// the workgroup's largest key (hi, lo) with the position that belongs to it.  A thread without a point passes (0, 0):
// a point's low word is never 0.  ONE barrier; `set` alternates from call to call.
__device__ __forceinline__ void fps_pick(FpsSlots &s, int set, int waves, uint32_t hi, uint32_t lo, float bx, float by,
                                         float bz, uint32_t &cj, float &cx, float &cy, float &cz) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    uint32_t mh = hi, ml = lo;
    wave_key_max(mh, ml);
    if (hi == mh && lo == ml && (ml != 0u || lane == 0)) {     // the owner (a wave without points: lane 0, key 0)
        s.hi[set][wv] = mh, s.lo[set][wv] = ml;
        s.p[set][wv][0] = bx, s.p[set][wv][1] = by, s.p[set][wv][2] = bz;
    }
    __syncthreads();
    uint32_t gh = s.hi[set][0], gl = s.lo[set][0];
    int gw = 0;
    for (int w = 1; w < waves; ++w) {
        const uint32_t h = s.hi[set][w], l = s.lo[set][w];
        if (h > gh || (h == gh && l > gl)) gh = h, gl = l, gw = w;
    }
    cj = 0xFFFFFFFFu - gl;
    cx = s.p[set][gw][0], cy = s.p[set][gw][1], cz = s.p[set][gw][2];
}

// the graph of this workgroup: nodes [a, a+n), picks out[o .. o+m), start s relative to a.  false: nothing to do (or
// offsets that do not fit the arrays) - block-uniform, so the workgroup leaves as a whole
__device__ __forceinline__ bool fps_graph(const int64_t *__restrict__ ptr, const int64_t *__restrict__ optr,
                                          const int64_t *__restrict__ start, int64_t N, int64_t M, int64_t &a,
                                          int64_t &n, int64_t &o, int64_t &m, int64_t &s) {
    const int64_t g = blockIdx.x;
    a = 0, n = N, o = 0, m = M;
    if (ptr) a = ptr[g], n = ptr[g + 1] - a, o = optr[g], m = optr[g + 1] - o;
    if (n <= 0 || m <= 0 || a < 0 || a + n > N || o < 0 || o + m > M) return false;
    s = start ? start[g] - a : 0;
    if (s < 0 || s >= n) s = 0;
    return true;
}

}  // namespace

// ---- fps: positions and running minimum in registers ----------------------------------------------------------------------
template <int PER>
__global__ void __launch_bounds__(kFpsThreads)
k_fps_resident(const float *__restrict__ x, int64_t ldx, const int64_t *__restrict__ ptr,
               const int64_t *__restrict__ optr, const int64_t *__restrict__ start, int64_t *__restrict__ out,
               int64_t N, int64_t M) {
    __shared__ FpsSlots slots;
    int64_t a, n64, o, m, s;
    if (!fps_graph(ptr, optr, start, N, M, a, n64, o, m, s)) return;
    const int T = blockDim.x, t = threadIdx.x;
    if (n64 > (int64_t)PER * T) {                              // (a graph larger than the launch was sized for)
        for (int64_t q = t; q < m; q += T) out[o + q] = -1;
        return;
    }
    const int n = (int)n64;
    const float *xg = x + a * ldx;
    float px[PER], py[PER], pz[PER], dist[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int j = t + u * T;
        const bool ok = j < n;
        px[u] = ok ? xg[(int64_t)j * ldx] : 0.f;
        py[u] = ok ? xg[(int64_t)j * ldx + 1] : 0.f;
        pz[u] = ok ? xg[(int64_t)j * ldx + 2] : 0.f;
        dist[u] = INFINITY;
    }
    float cx = xg[s * ldx], cy = xg[s * ldx + 1], cz = xg[s * ldx + 2];
    uint32_t cj = (uint32_t)s;
    if (t == 0) out[o] = a + s;
    const int waves = T >> 6;
    for (int64_t it = 1; it < m; ++it) {
        float bd = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        uint32_t lo = 0u;
#pragma unroll
        for (int u = 0; u < PER; ++u) {                        // ascending j: a strict > keeps the lowest j among equals
            const int j = t + u * T;
            if (j < n) {
                const float dx = px[u] - cx, dy = py[u] - cy, dz = pz[u] - cz;
                const float d = fminf(dist[u], (dx * dx + dy * dy) + dz * dz);
                dist[u] = d;
                if (d > bd) bd = d, lo = 0xFFFFFFFFu - (uint32_t)j, bx = px[u], by = py[u], bz = pz[u];
            }
        }
        const uint32_t hi = lo ? __float_as_uint(bd) : 0u;
        fps_pick(slots, (int)(it & 1), waves, hi, lo, bx, by, bz, cj, cx, cy, cz);
        if (t == 0) out[o + it] = a + (int64_t)cj;
    }
}

// ---- fps: any size; (x, y, z, dist) per point in the workspace, indexed by the global node id -----------------------------
__global__ void __launch_bounds__(kFpsThreads)
k_fps_stream(const float *__restrict__ x, int64_t ldx, const int64_t *__restrict__ ptr,
             const int64_t *__restrict__ optr, const int64_t *__restrict__ start, int64_t *__restrict__ out,
             float4 *__restrict__ ws, int64_t N, int64_t M) {
    __shared__ FpsSlots slots;
    int64_t a, n64, o, m, s;
    if (!fps_graph(ptr, optr, start, N, M, a, n64, o, m, s)) return;
    const uint32_t T = blockDim.x, t = threadIdx.x, n = (uint32_t)n64;      // (N < 2^31 - 1: j + T does not wrap)
    const float *xg = x + a * ldx;
    float4 *wg = ws + a;
    for (uint32_t j = t; j < n; j += T)
        wg[j] = make_float4(xg[(int64_t)j * ldx], xg[(int64_t)j * ldx + 1], xg[(int64_t)j * ldx + 2], INFINITY);
    float cx = xg[s * ldx], cy = xg[s * ldx + 1], cz = xg[s * ldx + 2];
    uint32_t cj = (uint32_t)s;
    if (t == 0) out[o] = a + s;
    const int waves = (int)(T >> 6);
    for (int64_t it = 1; it < m; ++it) {
        float bd = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        uint32_t lo = 0u;
        for (uint32_t j0 = t; j0 < n; j0 += kFpsInFlight * T) {      // this thread's own points, ascending; all loads of
            float4 v[kFpsInFlight];                            // a round are issued before its first store
#pragma unroll
            for (int u = 0; u < kFpsInFlight; ++u) {
                const uint32_t j = j0 + u * T;
                v[u] = j < n ? wg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < kFpsInFlight; ++u) {
                const uint32_t j = j0 + u * T;
                if (j < n) {
                    const float dx = v[u].x - cx, dy = v[u].y - cy, dz = v[u].z - cz;
                    const float d = fminf(v[u].w, (dx * dx + dy * dy) + dz * dz);
                    if (d < v[u].w) wg[j].w = d;               // (most points are nearer to an earlier pick: no store)
                    if (d > bd) bd = d, lo = 0xFFFFFFFFu - j, bx = v[u].x, by = v[u].y, bz = v[u].z;
                }
            }
        }
        const uint32_t hi = lo ? __float_as_uint(bd) : 0u;
        fps_pick(slots, (int)(it & 1), waves, hi, lo, bx, by, bz, cj, cx, cy, cz);
        if (t == 0) out[o + it] = a + (int64_t)cj;
    }
}

// ---- knn_interpolate, forward: one lane group per query ---------------------------------------------------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_knn_interp_fwd(const float *__restrict__ x, int64_t ldx, const float *__restrict__ px, int64_t ldpx,
                 const float *__restrict__ py, int64_t ldpy, const int32_t *__restrict__ nbr,
                 const int32_t *__restrict__ counts, int k, float *__restrict__ y, int64_t ldy,
                 float *__restrict__ w_out, float *__restrict__ den_out, int64_t Nx, int64_t Ny, int F, int lg) {
    constexpr int U = kSlotsPi;
    int64_t i;
    int sub, L;
    if (!seg_row<WAVE>(lg, Ny, i, sub, L)) return;
    int cnt = counts[i];
    cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
    const float qx = py[i * ldpy], qy = py[i * ldpy + 1], qz = py[i * ldpy + 2];
    const int32_t *nb = nbr + i * k;
    for (int c = sub * VEC; c < F; c += L * VEC) {
        const bool save = w_out != nullptr && c == 0;          // lane 0 of the group, its first columns
        float num[VEC], den = 0.f;
#pragma unroll
        for (int q = 0; q < VEC; ++q) num[q] = 0.f;
        for (int r0 = 0; r0 < cnt; r0 += U) {
            const int nn = cnt - r0;
            int64_t j[U];
            bool ok[U];
            float wv[U];
            Cols<VEC> xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t jj = u < nn ? nb[r0 + u] : -1;
                ok[u] = jj >= 0 && jj < Nx;
                j[u] = ok[u] ? jj : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float ax = ok[u] ? px[j[u] * ldpx] : 0.f, ay = ok[u] ? px[j[u] * ldpx + 1] : 0.f,
                            az = ok[u] ? px[j[u] * ldpx + 2] : 0.f;
                const float dx = ax - qx, dy = ay - qy, dz = az - qz;
                wv[u] = 1.0f / fmaxf((dx * dx + dy * dy) + dz * dz, 1e-16f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = cols_load<VEC>(x + j[u] * ldx + c, ok[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < nn) {
                    if (ok[u]) {
#pragma unroll
                        for (int q = 0; q < VEC; ++q) num[q] = num[q] + wv[u] * xv[u].a[q];
                        den = den + wv[u];
                    }
                    if (save) w_out[i * k + r0 + u] = ok[u] ? wv[u] : 0.f;
                }
        }
        if (save) {
            for (int r = cnt; r < k; ++r) w_out[i * k + r] = 0.f;
            den_out[i] = den;
        }
        float out[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) out[q] = den > 0.f ? num[q] / den : 0.f;
        cols_store<VEC>(y + i * ldy + c, out);
    }
}

// ---- knn_interpolate, backward: one lane group per source row, over its slots in ascending order ----------------------------
template <int VEC, bool WAVE>
__global__ void __launch_bounds__(256)
k_knn_interp_bwd(const int64_t *__restrict__ ptr, const int64_t *__restrict__ slots, const float *__restrict__ w,
                 const float *__restrict__ den, const float *__restrict__ gy, int64_t ldgy, float *__restrict__ gx,
                 int64_t ldgx, int k, int64_t Nx, int64_t Ny, int F, int lg) {
    constexpr int U = kSlotsPi;
    int64_t row;
    int sub, L;
    if (!seg_row<WAVE>(lg, Nx, row, sub, L)) return;
    const int64_t S = Ny * k;
    int64_t beg = ptr[row], end = ptr[row + 1];
    beg = beg < 0 ? 0 : (beg > S ? S : beg);
    end = end < beg ? beg : (end > S ? S : end);
    for (int c = sub * VEC; c < F; c += L * VEC) {
        float acc[VEC], cmp[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = 0.f, cmp[q] = 0.f;
        for (int64_t p = beg; p < end; p += U) {
            const int64_t nn = end - p;
            int64_t i[U];
            bool ok[U];
            float ww[U], dd[U];
            Cols<VEC> g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t s = u < nn ? slots[p + u] : -1;
                ok[u] = s >= 0 && s < S;
                i[u] = ok[u] ? s / k : 0;
                ww[u] = ok[u] ? w[s] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                dd[u] = ok[u] ? den[i[u]] : 1.f;
                ok[u] = ok[u] && dd[u] > 0.f;
                g[u] = cols_load<VEC>(gy + i[u] * ldgy + c, ok[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        const float tq = g[u].a[q] / dd[u];
                        kahan_add(acc[q], cmp[q], ww[u] * tq);
                    }
                }
        }
        cols_store<VEC>(gx + row * ldgx + c, acc);
    }
}

}  // namespace dc

using namespace dc;

// the four forms of a row kernel, as in dc_edge.hip: 16-byte or scalar columns, one wave per row or 64 / L rows per wave
#define DC_POINT_LAUNCH(kernel, v4, ROWS, F, stream, ...)                                                          \
    do {                                                                                                           \
        const int lg_ = log2_lanes((v4) ? (F) / 4 : (F));                                                       \
        const int64_t rows_ = 256 >> lg_;                                                                          \
        const dim3 grid_((unsigned)(((ROWS) + rows_ - 1) / rows_));                                                \
        if ((v4) && lg_ == 6) DC_LAUNCH((kernel<4, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_); \
        else if (v4) DC_LAUNCH((kernel<4, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);       \
        else if (lg_ == 6) DC_LAUNCH((kernel<1, true>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);  \
        else DC_LAUNCH((kernel<1, false>), grid_, dim3(256), 0, stream, __VA_ARGS__, (int)(F), lg_);               \
    } while (0)

extern "C" int64_t dc_fps_resident_points(void) { return kFpsResident; }

extern "C" int64_t dc_fps_workspace_bytes(int64_t N, int64_t max_n) {
    if (N < 0 || N >= (int64_t)INT32_MAX || max_n < 0 || max_n > N) return -1;
    return max_n > kFpsResident ? 16 * N : 0;
}

extern "C" int dc_fps(const float *x, int64_t ldx, int64_t N, const int64_t *ptr, const int64_t *optr, int64_t B,
                      int64_t max_n, const int64_t *start, int64_t *out, int64_t M, void *workspace,
                      int64_t workspace_bytes, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(N >= 0 && N < (int64_t)INT32_MAX && B >= 0 && B < (int64_t)INT32_MAX && M >= 0 && M <= N &&
                   max_n >= 0 && max_n <= N,
               "dc_fps: bad sizes (N=%lld B=%lld M=%lld max_n=%lld; need 0 <= M <= N, 0 <= max_n <= N)", (long long)N,
               (long long)B, (long long)M, (long long)max_n);
    DC_REQUIRE(ldx >= 3, "dc_fps: leading dimension smaller than 3 (ldx=%lld)", (long long)ldx);
    DC_REQUIRE((ptr == nullptr) == (optr == nullptr), "dc_fps: ptr and optr come together (both or neither)");
    DC_REQUIRE(ptr != nullptr || B <= 1, "dc_fps: B=%lld graphs need ptr and optr", (long long)B);
    if (N == 0 || B == 0 || M == 0 || max_n == 0) return DC_OK;
    DC_REQUIRE(x && out, "dc_fps: null pointer");
    const bool resident = max_n <= kFpsResident;
    if (!resident) {
        DC_REQUIRE(workspace, "dc_fps: null pointer (a graph of %lld points needs the workspace)", (long long)max_n);
        DC_REQUIRE(al16(workspace) && workspace_bytes >= 16 * N,
                   "dc_fps: workspace too small or not 16-byte aligned (%lld bytes, need %lld)",
                   (long long)workspace_bytes, (long long)(16 * N));
    }
    const dim3 grid((unsigned)B);
    if (!resident) {
        DC_LAUNCH(k_fps_stream, grid, dim3(kFpsThreads), 0, stream, x, ldx, ptr, optr, start, out, (float4 *)workspace,
                  N, M);
        return check_launch("dc_fps");
    }
    // the fewest points per thread that 256 threads hold, then the fewest waves
    int per = 1;
    while (per < kFpsPer && (int64_t)per * 256 < max_n) per *= 2;
    int64_t threads = ((max_n + per - 1) / per + kWave - 1) / kWave * kWave;
    threads = threads > kFpsThreads ? kFpsThreads : threads;
    const dim3 block((unsigned)threads);
    switch (per) {
    case 1: DC_LAUNCH(k_fps_resident<1>, grid, block, 0, stream, x, ldx, ptr, optr, start, out, N, M); break;
    case 2: DC_LAUNCH(k_fps_resident<2>, grid, block, 0, stream, x, ldx, ptr, optr, start, out, N, M); break;
    case 4: DC_LAUNCH(k_fps_resident<4>, grid, block, 0, stream, x, ldx, ptr, optr, start, out, N, M); break;
    default: DC_LAUNCH(k_fps_resident<8>, grid, block, 0, stream, x, ldx, ptr, optr, start, out, N, M); break;
    }
    return check_launch("dc_fps");
}

extern "C" int dc_knn_interpolate_fwd(const float *x, int64_t ldx, const float *pos_x, int64_t ldpx, const float *pos_y,
                                      int64_t ldpy, const int32_t *nbr, const int32_t *counts, int k, float *y,
                                      int64_t ldy, float *w, float *den, int64_t Nx, int64_t Ny, int64_t F,
                                      dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(Nx >= 0 && Ny >= 0 && F >= 1, "dc_knn_interpolate_fwd: need Nx >= 0, Ny >= 0, width >= 1 (Nx=%lld Ny=%lld "
               "width=%lld)", (long long)Nx, (long long)Ny, (long long)F);
    DC_REQUIRE(sizes_ok(Nx, F) && sizes_ok(Ny, F), "dc_knn_interpolate_fwd: size out of range");
    DC_REQUIRE(k >= 1 && k <= DC_NEIGHBORS_MAX_CAP, "dc_knn_interpolate_fwd: k=%d outside 1..%d", k, DC_NEIGHBORS_MAX_CAP);
    DC_REQUIRE(ldx >= F && ldy >= F && ldpx >= 3 && ldpy >= 3,
               "dc_knn_interpolate_fwd: leading dimension smaller than F (x, y) or 3 (pos_x, pos_y)");
    if (Ny == 0) return DC_OK;
    DC_REQUIRE(pos_y && nbr && counts && y && (Nx == 0 || (x && pos_x)), "dc_knn_interpolate_fwd: null pointer");
    DC_REQUIRE((w == nullptr) == (den == nullptr), "dc_knn_interpolate_fwd: w and den come together (both or neither)");
    DC_REQUIRE(y != x && y != w && y != den && (w == nullptr || w != den),
               "dc_knn_interpolate_fwd: the outputs must not alias x or each other");
    const bool v4 = F % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y);
    DC_POINT_LAUNCH(k_knn_interp_fwd, v4, Ny, F, stream, x, ldx, pos_x, ldpx, pos_y, ldpy, nbr, counts, k, y, ldy, w,
                    den, Nx, Ny);
    return check_launch("dc_knn_interpolate_fwd");
}

extern "C" int dc_knn_interpolate_bwd(const int64_t *ptr, const int64_t *slots, const float *w, const float *den,
                                      const float *gy, int64_t ldgy, float *gx, int64_t ldgx, int k, int64_t Nx,
                                      int64_t Ny, int64_t F, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(Nx >= 0 && Ny >= 0 && F >= 1, "dc_knn_interpolate_bwd: need Nx >= 0, Ny >= 0, width >= 1 (Nx=%lld Ny=%lld "
               "width=%lld)", (long long)Nx, (long long)Ny, (long long)F);
    DC_REQUIRE(sizes_ok(Nx, F) && sizes_ok(Ny, F), "dc_knn_interpolate_bwd: size out of range");
    DC_REQUIRE(k >= 1 && k <= DC_NEIGHBORS_MAX_CAP, "dc_knn_interpolate_bwd: k=%d outside 1..%d", k, DC_NEIGHBORS_MAX_CAP);
    DC_REQUIRE(ldgy >= F && ldgx >= F, "dc_knn_interpolate_bwd: leading dimension smaller than F");
    if (Nx == 0) return DC_OK;
    DC_REQUIRE(ptr && gx && (Ny == 0 || (slots && w && den && gy)), "dc_knn_interpolate_bwd: null pointer");
    DC_REQUIRE(gx != gy && gx != w && gx != den, "dc_knn_interpolate_bwd: gx must not alias an input");
    const bool v4 = F % 4 == 0 && ldgy % 4 == 0 && ldgx % 4 == 0 && al16(gy) && al16(gx);
    DC_POINT_LAUNCH(k_knn_interp_bwd, v4, Nx, F, stream, ptr, slots, w, den, gy, ldgy, gx, ldgx, k, Nx, Ny);
    return check_launch("dc_knn_interpolate_bwd");
}
