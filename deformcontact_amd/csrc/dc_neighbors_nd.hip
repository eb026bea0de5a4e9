// dc_neighbors_nd.hip -- exact kNN over rows of any width F >= 1 (the feature-space search DGCNN's DynamicEdgeConv
// repeats in every layer; PyG knn / knn_graph on features).  The grid of dc_neighbors.hip is three-dimensional and
// does not help at 64 columns: this is a tiled brute force per graph.
//
// Rules (include/deformcontact.h): with d_c = x[j,c] - y[i,c], d2 = d_0*d_0, then
// d2 = d2 + d_c*d_c for c = 1 .. F-1 in column order, every difference, product and sum rounded on its own in fp32
// (for F = 3 the rule of dc_neighbors.hip); the candidates of a query - the rows of x with the query's graph id - are
// ranked by (d2, j) ascending and the first `cap` kept.  No |x|^2 + |y|^2 - 2 x.y form and no MFMA: both round
// differently and would rank near-ties differently.
//
// Shape: a 256-thread workgroup owns kWgQ = 32 consecutive queries, each wave kQ = 8 of them.  Both batch vectors are
// sorted, so the union of the workgroup's candidate ranges is one contiguous run of x; the workgroup walks it in tiles
// of 64 candidates (lane l of every wave takes candidate l) and stages a tile kW = 32 columns at a time in LDS, once
// for its four waves, together with the same columns of its 32 queries.  The partial d2 of each (query, candidate)
// stays in a register across the column chunks, so the column order holds for any F.  One candidate's chain over c is
// serial; the 8 queries of a wave are the independent chains, taken two at a time as packed fp32 operations (a packed
// add or multiply rounds each half like the scalar one; the build has -ffp-contract=off).  A query masks candidates
// outside its own [xs, xe).  The best-cap list is the wave-resident sorted list of dc_topk.h.
//
// LDS: the candidate tile is stored transposed, s_cand[c * 65 + l]: the 64 lanes reading column c of "their" candidate
// touch 64 consecutive dwords (no bank conflict), and the staging writes - 32 consecutive columns of one candidate per
// half wave - land on banks (c + l) mod 32, all different (a row stride of 64 would put them on one).  The queries
// are stored as pairs, s_qry[(pair * kW + c) * 2 + half]: one wave-uniform (broadcast) 16-byte read gives columns c
// and c + 1 of two queries in the register layout the packed operations take.  The next (tile, chunk) is fetched into
// registers while the current one is computed.
#include <limits.h>

#include "dc_common.h"
#include "dc_topk.h"

namespace dc {
namespace {

constexpr int kMaxCap = DC_NEIGHBORS_MAX_CAP;
constexpr int kW = DC_NEIGHBORS_ND_CHUNK;        // columns per staged chunk
constexpr int kQ = 8;                            // queries per wave (register-blocked; even: taken in pairs)
constexpr int kThreads = 256;
constexpr int kWgQ = kQ * (kThreads / 64);       // queries per workgroup
constexpr int kTile = 64;                        // candidates per tile: one per lane
constexpr int kPad = kTile + 1;                  // row stride of the transposed candidate tile
constexpr int kCandPer = kTile * kW / kThreads;  // staged candidate elements per thread
constexpr int kQryPer = kWgQ * kW / kThreads;    // staged query elements per thread
static_assert(kW % 2 == 0 && kQ % 2 == 0 && kThreads % kW == 0, "chunk / pair geometry");
static_assert(kWgQ <= 64, "the ranges of a workgroup's queries are found by its first wave");

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(kThreads)
k_query_nd(const float *__restrict__ x, int64_t ldx, int64_t nx, const int64_t *__restrict__ batch_x,
           const float *__restrict__ y, int64_t ldy, int64_t ny, const int64_t *__restrict__ batch_y, int f, int cap,
           int exclude_self, int32_t *nbr, int32_t *counts) {
    __shared__ float s_cand[kW * kPad];
    __shared__ __attribute__((aligned(16))) float s_qry[kWgQ * kW];
    __shared__ int s_xs[kWgQ], s_xe[kWgQ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * kWgQ;

    if (tid < kWgQ) {                                              // the query's graph: a run of batch_x
        const int64_t q = q0 + tid;
        int64_t xs = 0, xe = 0;
        if (q < ny && cap > 0) {
            xe = nx;
            if (batch_x) {
                const int64_t b = batch_y ? batch_y[q] : 0;
                xs = lower_bound(batch_x, (int64_t)0, nx, b);
                xe = upper_bound(batch_x, xs, nx, b);
            } else if (batch_y && batch_y[q] != 0) {
                xe = 0;
            }
        }
        s_xs[tid] = (int)xs, s_xe[tid] = (int)xe;
    }
    __syncthreads();
    int us = INT_MAX, ue = 0;                                      // the union of the non-empty ranges
    for (int i = 0; i < kWgQ; ++i) {
        const int a = s_xs[i], b = s_xe[i];
        if (a < b) us = a < us ? a : us, ue = b > ue ? b : ue;
    }
    us = __builtin_amdgcn_readfirstlane(us), ue = __builtin_amdgcn_readfirstlane(ue);   // (uniform: into SGPRs)
    const int64_t ntiles = ue > us ? ((int64_t)ue - us + kTile - 1) / kTile : 0;
    const int nchunks = (f + kW - 1) / kW;
    const int64_t total = ntiles * nchunks;

    int qxs[kQ], qxe[kQ];
    unsigned long long entry[kQ], kth[kQ];
#pragma unroll
    for (int i = 0; i < kQ; ++i) {
        qxs[i] = __builtin_amdgcn_readfirstlane(s_xs[wave * kQ + i]);
        qxe[i] = __builtin_amdgcn_readfirstlane(s_xe[wave * kQ + i]);
        entry[i] = kTopkNone, kth[i] = kTopkNone;
    }

    // The next (tile, chunk), in flight.  Addresses are clamped to the last candidate of the union and to the last
    // column instead of being guarded: a candidate at or past `ue` is masked when the tile is ranked (qxe <= ue), a
    // column at or past f is never read (the last chunk runs over its own `cw` columns).
    float pc[kCandPer], pq[kQryPer];
    const int st_c = tid % kW, st_r = tid / kW;                    // this thread's column and first row of a chunk
    const float *yrow[kQryPer];
#pragma unroll
    for (int r = 0; r < kQryPer; ++r) {
        const int64_t q = q0 + st_r + (kThreads / kW) * r;
        yrow[r] = y + (q < ny ? q : ny - 1) * ldy;                 // (a row past the end: the last one, unused)
    }
    auto fetch = [&](int64_t tile, int ch) {
        const int j0 = us + (int)tile * kTile + st_r;
        const int c = ch * kW + st_c < f ? ch * kW + st_c : f - 1;
#pragma unroll
        for (int r = 0; r < kCandPer; ++r) {
            const int j = j0 + (kThreads / kW) * r;
            pc[r] = x[(int64_t)(j < ue ? j : ue - 1) * ldx + c];
        }
#pragma unroll
        for (int r = 0; r < kQryPer; ++r) pq[r] = yrow[r][c];
    };

    v2f acc[kQ / 2];
#pragma unroll
    for (int p = 0; p < kQ / 2; ++p) acc[p] = (v2f)(0.0f);         // 0 + d*d = d*d exactly: d2 starts at d_0*d_0
    const v2f *qp = (const v2f *)s_qry + wave * (kQ / 2) * kW;     // pair p, column c at qp[p * kW + c]
    const float *cp = s_cand + lane;                               // column c of this lane's candidate at cp[c * kPad]

    int64_t tile = 0;
    int ch = 0;
    if (total > 0) fetch(0, 0);
    for (int64_t it = 0; it < total; ++it) {
        __syncthreads();                                           // the previous chunk has been read by every wave
        {
#pragma unroll
            for (int r = 0; r < kCandPer; ++r) s_cand[st_c * kPad + st_r + (kThreads / kW) * r] = pc[r];
#pragma unroll
            for (int r = 0; r < kQryPer; ++r) {
                const int qi = st_r + (kThreads / kW) * r;
                s_qry[((qi >> 1) * kW + st_c) * 2 + (qi & 1)] = pq[r];
            }
        }
        __syncthreads();
        const int64_t cur_tile = tile;
        const int cw = f - ch * kW < kW ? f - ch * kW : kW;       // columns of this chunk
        const bool last = ch == nchunks - 1;
        if (last) ch = 0, ++tile;
        else ++ch;
        if (it + 1 < total) fetch(tile, ch);

        if (cw == kW) {
#pragma unroll
            for (int c = 0; c < kW; c += 2) {
                const v2f x0 = (v2f)(cp[c * kPad]), x1 = (v2f)(cp[(c + 1) * kPad]);
#pragma unroll
                for (int p = 0; p < kQ / 2; ++p) {
                    const v4f qq = *(const v4f *)(qp + p * kW + c);
                    const v2f d0 = x0 - qq.xy;
                    acc[p] = acc[p] + d0 * d0;
                    const v2f d1 = x1 - qq.zw;
                    acc[p] = acc[p] + d1 * d1;
                }
            }
        } else {
#pragma unroll 1
            for (int c = 0; c < cw; ++c) {                         // (the last chunk where kW does not divide f)
                const v2f xv = (v2f)(cp[c * kPad]);
#pragma unroll
                for (int p = 0; p < kQ / 2; ++p) {
                    const v2f d = xv - qp[p * kW + c];
                    acc[p] = acc[p] + d * d;
                }
            }
        }
        if (last) {                                                // d2 of this tile is complete: rank it
            const int64_t j = (int64_t)us + cur_tile * kTile + lane;    // (the last tile may pass INT_MAX: masked)
#pragma unroll
            for (int i = 0; i < kQ; ++i) {
                const float d2 = (i & 1) ? acc[i / 2].y : acc[i / 2].x;
                const bool ok = j >= qxs[i] && j < qxe[i] && !(exclude_self && j == q0 + wave * kQ + i);
                topk_insert(ok ? topk_key(d2, (int)j) : kTopkNone, lane, cap, entry[i], kth[i]);
            }
#pragma unroll
            for (int p = 0; p < kQ / 2; ++p) acc[p] = (v2f)(0.0f);
        }
    }
#pragma unroll
    for (int i = 0; i < kQ; ++i) {
        const int64_t q = q0 + wave * kQ + i;
        if (q < ny) topk_store(entry[i], lane, cap, nbr + q * cap, counts + q);
    }
}

}  // namespace
}  // namespace dc

using namespace dc;

extern "C" int dc_neighbors_nd_fill(const float *x, int64_t ldx, int64_t nx, const int64_t *batch_x, const float *y,
                                    int64_t ldy, int64_t ny, const int64_t *batch_y, int64_t f, int cap,
                                    int exclude_self, int32_t *nbr, int32_t *counts, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (nx: the last tile's candidate numbers, up to nx + 63, are formed in int32)
    DC_REQUIRE(nx >= 0 && ny >= 0 && nx < (int64_t)INT32_MAX - kTile && ny < (int64_t)INT32_MAX,
               "dc_neighbors_nd_fill: bad sizes (nx=%lld, ny=%lld)", (long long)nx, (long long)ny);
    DC_REQUIRE(cap >= 0 && cap <= kMaxCap, "dc_neighbors_nd_fill: cap=%d outside [0, %d]", cap, kMaxCap);
    DC_REQUIRE(f >= 1 && f < (int64_t)INT32_MAX - kW, "dc_neighbors_nd_fill: width f=%lld is not >= 1 (or exceeds "
               "int32)", (long long)f);
    DC_REQUIRE((nx == 0 || ldx >= f) && (ny == 0 || ldy >= f), "dc_neighbors_nd_fill: leading dimension below the "
               "width f=%lld (ldx=%lld, ldy=%lld)", (long long)f, (long long)ldx, (long long)ldy);
    if (ny == 0 || (cap == 0 && !counts)) return DC_OK;
    // (cap = 0 with counts: the kernel walks nothing, reads neither x nor y and writes the zero counts)
    DC_REQUIRE(cap == 0 || (y && counts && nbr && (nx == 0 || x)), "dc_neighbors_nd_fill: null pointer");
    DC_LAUNCH(k_query_nd, dim3((unsigned)((ny + kWgQ - 1) / kWgQ)), dim3(kThreads), 0, stream, x, ldx, nx, batch_x, y,
              ldy, ny, batch_y, (int)f, cap, exclude_self, nbr, counts);
    return check_launch("dc_neighbors_nd_fill");
}
