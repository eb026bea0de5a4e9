// dc_neighbors.hip -- kNN and radius neighbour search on the device (PyG 2.5 knn / knn_graph / radius / radius_graph,
// /root/reference/utils/pointcloud_utils.py:7-13), replacing the host cKDTree builder (synth.radius_graph_points).
//
// Rules (include/deformcontact.h): d2 = ((dx*dx + dy*dy) + dz*dz) in fp32, every product and
// sum rounded on its own, dx = x_j - y_i; the candidates of a query (points of x in the query's own graph) are ranked
// by (d2, j) ascending; kNN keeps the first `cap`, radius the first `cap` of those with d2 < r*r (r*r rounded once).
//
// Search: one uniform grid per graph (bounding box from ordered-int atomics per segment, as k_bbox in dc_order.hip),
// the points sorted by (graph, cell) with rocPRIM's radix sort (preprocessing, as in dc_order.hip), and for each
// query a box of cells that grows until no unvisited point can enter the query's best `cap`.  A box row (fixed y, z
// cell) is one contiguous key range, found by binary search: no dense cell table, so a tiny r against a large extent
// costs nothing.  One wave per query; lane l holds the query's l-th best (d2, j) as one 64-bit key.
//
// Coverage is exact, not tolerance-based: the cell map c(v) = clamp(floor((v - lo) * inv)) is
// monotone, so a box built from the fp32 bounds lo_q <= q - rho and hi_q >= q + rho contains every point with
// q - rho <= p <= q + rho on all three axes.  Any point outside has |fl(p_a - q_a)| >= rho on some axis, hence a
// computed d2 >= fl(rho * rho) (rounding is monotone and every term of d2 is >= 0).  The search stops once the
// current cap-th key is below (fl(rho * rho), 0), i.e. its d2 is strictly smaller than that bound: an unvisited point
// at an equal d2 with a smaller j would outrank it, so equality does not stop it.
#include <math.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "dc_common.h"
#include "dc_topk.h"

namespace dc {
namespace {

constexpr int kMaxCap = DC_NEIGHBORS_MAX_CAP;   // one kept neighbour per lane of the query's wave
constexpr int kMaxDim = 1024;                   // cells per axis of a graph's grid: a cell id fits 30 bits
constexpr int kBboxChunk = 1024;                // points per wave in k_seg_bbox
constexpr int kMaxSteps = 4096;                 // box growth steps (a finite query needs at most ~kMaxDim + 2)
constexpr unsigned long long kNone = kTopkNone;  // an empty top-k slot (dc_topk.h); every real key is smaller

// a graph's grid, stored at the index of the graph's first point (its segment start)
struct GridParams {
    float lo[3], hi[3];   // bounding box
    float h, inv;         // cell size (the box growth step) and the factor of the cell map
    int dims[3], pad;
};

// the ONE cell map of points and of box bounds: monotone in v for any positive inv (NaN and +-inf clamp to the grid)
__device__ __forceinline__ int cell_of(float v, const GridParams &P, int a) {
    const float t = floorf(__fmul_rn(__fsub_rn(v, P.lo[a]), P.inv));
    return (int)fminf(fmaxf(t, 0.0f), (float)(P.dims[a] - 1));
}

__global__ void __launch_bounds__(256)
k_bbox_init_seg(unsigned *bbox, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 6 * n) return;
    bbox[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;                      // minima, maxima
}

__device__ __forceinline__ void bbox_flush(unsigned *bbox, int s, const float *lo, const float *hi) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(&bbox[6 * (int64_t)s + a], ord_key(lo[a]));
        atomicMax(&bbox[6 * (int64_t)s + 3 + a], ord_key(hi[a]));
    }
}

// Segment start of every point (the first index of its run of equal batch values) and each segment's bounding box.
// One wave walks 1,024 consecutive points, 64 at a time: a segmented shuffle reduction per window, the window's last
// run carried into the next window, so that one graph costs one atomic per value and wave (k_bbox's note: a same-
// address atomic retires every ~60 ns; one per point would take 36 ms for the 100k cloud).
__global__ void __launch_bounds__(256)
k_seg_bbox(const float *__restrict__ x, int64_t ld, int64_t n, const int64_t *__restrict__ batch, int32_t *seg,
           unsigned *bbox) {
    const int lane = threadIdx.x & 63;
    const int64_t beg = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * kBboxChunk;
    if (beg >= n) return;                                          // wave-uniform
    const int64_t end = beg + kBboxChunk < n ? beg + kBboxChunk : n;
    // the segment the chunk starts in may have begun in an earlier chunk (without a batch vector: one segment)
    int carry_s = batch ? (int)lower_bound(batch, (int64_t)0, beg, batch[beg]) : 0;
    float clo[3], chi[3];
    bool have = false;
    for (int64_t base = beg; base < end; base += 64) {
        const int64_t i = base + lane;
        const bool valid = i < end;
        const bool head = valid && (i == 0 || (batch && batch[i] != batch[i - 1]));
        const unsigned long long upto = __ballot(head) & ((2ull << lane) - 1);   // heads at lanes <= this one
        const int s = upto ? (int)(base + 63 - __clzll(upto)) : carry_s;
        if (valid) seg[i] = s;
        float lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = valid ? x[i * ld + a] : 0.0f;
        const int sv = valid ? s : -1;
        // segmented reduction: lane l ends with the box of lanes [l, 64) of its own run
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int os = __shfl_down(sv, off);
            const bool take = lane + off < 64 && os == sv;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float ol = __shfl_down(lo[a], off), oh = __shfl_down(hi[a], off);
                if (take) lo[a] = fminf(lo[a], ol), hi[a] = fmaxf(hi[a], oh);
            }
        }
        const int prev_s = __shfl_up(sv, 1);
        const bool rhead = valid && (lane == 0 || sv != prev_s);
        const unsigned long long rh = __ballot(rhead);             // lane 0 is always a run head (base < end)
        const int last = 63 - __clzll(rh);
        const int s0 = __shfl(sv, 0);
        if (have && s0 == carry_s) {                               // the first run continues the carried one
            if (lane == 0) {
#pragma unroll
                for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], clo[a]), hi[a] = fmaxf(hi[a], chi[a]);
            }
        } else if (have && lane == 0) {
            bbox_flush(bbox, carry_s, clo, chi);
        }
        if (rhead && lane != last) bbox_flush(bbox, sv, lo, hi);  // runs that end inside this window
        carry_s = __shfl(sv, last);
#pragma unroll
        for (int a = 0; a < 3; ++a) clo[a] = __shfl(lo[a], last), chi[a] = __shfl(hi[a], last);
        have = true;
    }
    if (lane == 0) bbox_flush(bbox, carry_s, clo, chi);
}

// every slot gets parameters (a slot that starts no segment a safe default): the grid of a segment from its box
__global__ void __launch_bounds__(256)
k_grid_params(const unsigned *__restrict__ bbox, const int32_t *__restrict__ seg, const int64_t *__restrict__ batch,
              int64_t n, int radius_mode, float rho_max, GridParams *params) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GridParams P;
    P.h = 1.0f, P.inv = 1.0f, P.pad = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) P.lo[a] = 0.0f, P.hi[a] = 0.0f, P.dims[a] = 1;
    if (seg[i] == (int32_t)i) {
        int64_t cnt = batch ? upper_bound(batch, i, n, batch[i]) - i : n - i;
        cnt = cnt < 1 ? 1 : cnt;
        float ext = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P.lo[a] = ord_val(bbox[6 * i + a]), P.hi[a] = ord_val(bbox[6 * i + 3 + a]);
            ext = fmaxf(ext, P.hi[a] - P.lo[a]);
        }
        // kNN: about two points per cell of a solid cloud; radius: cells of r / 2 (a box of 2 r spans 4-5 cells)
        float h;
        if (radius_mode) {
            h = 0.5f * rho_max;
        } else {
            const float g = fminf(fmaxf(ceilf(cbrtf(0.5f * (float)cnt)), 1.0f), (float)(kMaxDim - 1));
            h = ext / g;
        }
        h = fmaxf(h, ext * (1.0f / (kMaxDim - 1)));               // at most kMaxDim cells per axis
        if (!(h <= 3.0e38f)) h = ext;                              // r = inf: one cell as wide as the graph
        if (!(h >= 1.0e-30f)) h = 1.0f;                            // a zero extent or r = 0: any positive size
        P.h = h, P.inv = 1.0f / h;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float t = floorf((P.hi[a] - P.lo[a]) * P.inv) + 1.0f;
            P.dims[a] = (int)fminf(fmaxf(t, 1.0f), (float)kMaxDim);
        }
    }
    params[i] = P;
}

// key = (segment start, cell id): sorting keeps every graph in its own index range, cells in x-fastest order
__global__ void __launch_bounds__(256)
k_cell_keys(const float *__restrict__ x, int64_t ld, int64_t n, const int32_t *__restrict__ seg,
            const GridParams *__restrict__ params, unsigned long long *keys, int32_t *vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = seg[i];
    const GridParams P = params[s];
    const int cx = cell_of(x[i * ld], P, 0), cy = cell_of(x[i * ld + 1], P, 1), cz = cell_of(x[i * ld + 2], P, 2);
    keys[i] = ((unsigned long long)(unsigned)s << 32) | (unsigned)((cz * P.dims[1] + cy) * P.dims[0] + cx);
    vals[i] = (int32_t)i;
}

// the sorted points as (x, y, z, index bits): one 16-byte load per candidate
__global__ void __launch_bounds__(256)
k_sorted_points(const float *__restrict__ x, int64_t ld, int64_t n, const int32_t *__restrict__ order, float4 *spos) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t j = order[p];
    spos[p] = make_float4(x[j * ld], x[j * ld + 1], x[j * ld + 2], __int_as_float((int)j));
}

// the positions [b, b + cnt) of the cells [ca, cb] of one box row (row = the cell id of its x = 0 cell)
__device__ __forceinline__ void row_piece(const unsigned long long *keys, int64_t xs, int64_t xe,
                                          unsigned long long S, int row, int ca, int cb, int &b, int &cnt) {
    if (ca > cb) {
        b = 0, cnt = 0;
        return;
    }
    const int64_t lo = lower_bound(keys, xs, xe, S | (unsigned)(row + ca));
    const int64_t hi = lower_bound(keys, lo, xe, S | (unsigned)(row + cb + 1));
    b = (int)lo, cnt = (int)(hi - lo);
}

// One wave per query.  Rows of the box are dealt to lanes (up to two pieces per row: the cells the previous, smaller
// box did not cover), their lengths scanned across the wave, and the candidates taken 64 at a time.
__global__ void __launch_bounds__(256)
k_query(const float *__restrict__ y, int64_t ldy, int64_t ny, const int64_t *__restrict__ batch_y,
        const int64_t *__restrict__ batch_x, int64_t nx, const GridParams *__restrict__ params,
        const unsigned long long *__restrict__ keys, const float4 *__restrict__ spos, int cap, int radius_mode,
        float r2, float rho_max, int exclude_self, int32_t *nbr, int32_t *counts) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= ny) return;                                           // wave-uniform
    int64_t xs = 0, xe = nx;                                       // the query's graph: a run of batch_x
    if (batch_x) {
        const int64_t b = batch_y ? batch_y[q] : 0;
        xs = lower_bound(batch_x, (int64_t)0, nx, b);
        xe = upper_bound(batch_x, xs, nx, b);
    } else if (batch_y && batch_y[q] != 0) {
        xe = 0;
    }
    unsigned long long entry = kNone;                              // this lane's rank in the query's best list
    if (xs < xe) {
        const GridParams P = params[xs];
        float qv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) qv[a] = y[q * ldy + a];
        const unsigned long long S = (unsigned long long)(unsigned)xs << 32;
        unsigned long long kth = kNone;                            // entry of lane cap - 1
        float rho;
        if (radius_mode) {
            rho = fminf(P.h, rho_max);
        } else {                                                   // a query outside the box starts at its distance
            float dist = 0.0f;
#pragma unroll
            for (int a = 0; a < 3; ++a) dist = fmaxf(dist, fmaxf(P.lo[a] - qv[a], qv[a] - P.hi[a]));
            rho = P.h + dist;
        }
        int pl[3] = {0, 0, 0}, ph[3] = {-1, -1, -1};               // the box already searched (none yet)
        bool prev = false;
        for (int step = 0;; ++step) {
            int bl[3], bh[3];
            bool empty = false, full = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                // fl(q - M) <= q - rho and fl(q + M) >= q + rho, with room for the rounding of M and of q -+ M
                const float M = __fadd_rn(__fmul_rn(rho, 1.0001f), __fmul_rn(fabsf(qv[a]), 1.0e-6f));
                const float lq = __fsub_rn(qv[a], M), hq = __fadd_rn(qv[a], M);
                empty = empty || lq > P.hi[a] || hq < P.lo[a];     // no point of the graph lies within rho
                bl[a] = cell_of(lq, P, a), bh[a] = cell_of(hq, P, a);
                full = full && bl[a] == 0 && bh[a] == P.dims[a] - 1;
            }
            if (!empty) {
                const int wy = bh[1] - bl[1] + 1, nrows = wy * (bh[2] - bl[2] + 1);
                for (int r0 = 0; r0 < nrows; r0 += 64) {
                    const int r = r0 + lane;
                    int b0 = 0, n0 = 0, b1 = 0, n1 = 0;
                    if (r < nrows) {
                        const int cy = bl[1] + r % wy, cz = bl[2] + r / wy;
                        const int row = (cz * P.dims[1] + cy) * P.dims[0];
                        if (prev && cy >= pl[1] && cy <= ph[1] && cz >= pl[2] && cz <= ph[2]) {
                            row_piece(keys, xs, xe, S, row, bl[0], pl[0] - 1, b0, n0);
                            row_piece(keys, xs, xe, S, row, ph[0] + 1, bh[0], b1, n1);
                        } else {
                            row_piece(keys, xs, xe, S, row, bl[0], bh[0], b0, n0);
                        }
                    }
                    const int len = n0 + n1;
                    int incl = len;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const int o = __shfl_up(incl, off);
                        if (lane >= off) incl += o;
                    }
                    const int total = __shfl(incl, 63);
                    for (int t0 = 0; t0 < total; t0 += 64) {
                        const int t = t0 + lane;
                        int lo = 0, hi = 63;                       // the lane whose pieces hold candidate t
#pragma unroll
                        for (int it = 0; it < 6; ++it) {
                            const int mid = (lo + hi) >> 1;
                            if (__shfl(incl, mid) > t) hi = mid;
                            else lo = mid + 1;
                        }
                        const int L = lo;
                        const int first = __shfl(incl, L) - __shfl(len, L);
                        const int Lb0 = __shfl(b0, L), Ln0 = __shfl(n0, L), Lb1 = __shfl(b1, L);
                        unsigned long long key = kNone;
                        if (t < total) {
                            const int local = t - first;
                            const float4 c = spos[local < Ln0 ? Lb0 + local : Lb1 + (local - Ln0)];
                            const int j = __float_as_int(c.w);
                            const float dx = __fsub_rn(c.x, qv[0]), dy = __fsub_rn(c.y, qv[1]),
                                        dz = __fsub_rn(c.z, qv[2]);
                            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)),
                                                       __fmul_rn(dz, dz));
                            if (!(exclude_self && (int64_t)j == q) && (!radius_mode || d2 < r2))
                                key = ((unsigned long long)ord_key(d2) << 32) | (unsigned)j;
                        }
                        // insert the candidates below the current cap-th key, one at a time, keeping lanes sorted
                        topk_insert(key, lane, cap, entry, kth);
                    }
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) pl[a] = bl[a], ph[a] = bh[a];
                prev = true;
            }
            // every unvisited point has d2 >= fl(rho * rho): stop when the cap-th d2 is strictly below that
            const float bound = __fmul_rn(rho, rho);
            if (kth < ((unsigned long long)ord_key(bound) << 32)) break;
            if ((!empty && full) || (radius_mode && rho >= rho_max)) break;
            if (!(rho <= 3.0e38f) || step >= kMaxSteps) break;
            float next = __fadd_rn(rho, P.h);
            if (!(next > rho)) next = __fmul_rn(rho, 2.0f);
            rho = radius_mode ? fminf(next, rho_max) : next;
        }
    }
    topk_store(entry, lane, cap, nbr + q * cap, counts + q);
}

__global__ void __launch_bounds__(256)
k_no_neighbors(int32_t *nbr, int cap, int32_t *counts, int64_t ny) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ny) counts[i] = 0;
    if (i < ny * cap) nbr[i] = -1;
}

struct CountAsI64 {                                                // a count, clamped to [0, cap], as int64
    int cap;
    __device__ int64_t operator()(int32_t v) const { return v < 0 ? 0 : (v > cap ? cap : v); }
};

__global__ void __launch_bounds__(256)
k_compact(const int32_t *__restrict__ nbr, int cap, const int32_t *__restrict__ counts,
          const int64_t *__restrict__ incl, int64_t ny, int query_row, int64_t *out, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ny * cap) return;
    const int64_t q = i / cap, t = i - q * cap;
    const int64_t cnt = CountAsI64{cap}(counts[q]);
    if (t >= cnt) return;
    const int64_t e = (q > 0 ? incl[q - 1] : 0) + t;
    if (e >= m) return;                                            // (a num_edges below the counts' total)
    out[query_row * m + e] = q;
    out[(1 - query_row) * m + e] = nbr[i];
}

inline int64_t al256(int64_t b) { return (b + 255) & ~int64_t(255); }

inline int key_end_bit(int64_t n) {                                // the cell id's 32 bits + those of the largest start
    int b = 0;
    while (b < 32 && ((int64_t)1 << b) < n) ++b;
    return 32 + b;
}

size_t sort_temp_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                    (int32_t *)nullptr, (int32_t *)nullptr, (size_t)n, 0, key_end_bit(n),
                                    (hipStream_t)0);
    return bytes;
}

size_t scan_temp_bytes(int64_t n) {
    size_t bytes = 0;
    auto in = rocprim::make_transform_iterator((const int32_t *)nullptr, CountAsI64{1});
    (void)rocprim::inclusive_scan(nullptr, bytes, in, (int64_t *)nullptr, (size_t)n, rocprim::plus<int64_t>(),
                                  (hipStream_t)0);
    return bytes;
}

// fill workspace: bbox [6n] u32 | seg [n] i32 | params [n] | keys in, out [n] u64 | vals in, out [n] i32 |
// sorted points [n] float4 | sort temporaries
struct FillLayout {
    int64_t bbox, seg, params, keys_in, keys_out, vals_in, vals_out, spos, temp, total;
    explicit FillLayout(int64_t n) {
        bbox = 0;
        seg = bbox + al256(24 * n);
        params = seg + al256(4 * n);
        keys_in = params + al256((int64_t)sizeof(GridParams) * n);
        keys_out = keys_in + al256(8 * n);
        vals_in = keys_out + al256(8 * n);
        vals_out = vals_in + al256(4 * n);
        spos = vals_out + al256(4 * n);
        temp = spos + al256(16 * n);
        total = temp + al256((int64_t)sort_temp_bytes(n));
    }
};

}  // namespace
}  // namespace dc

using namespace dc;

extern "C" int64_t dc_neighbors_workspace_bytes(int64_t nx, int64_t ny) {
    if (nx < 0 || ny < 0 || nx >= (int64_t)INT32_MAX || ny >= (int64_t)INT32_MAX) return -1;
    return nx == 0 ? 0 : FillLayout(nx).total;
}

extern "C" int dc_neighbors_fill(const float *x, int64_t ldx, int64_t nx, const int64_t *batch_x, const float *y,
                                 int64_t ldy, int64_t ny, const int64_t *batch_y, int mode, float r, int cap,
                                 int exclude_self, int32_t *nbr, int32_t *counts, void *workspace,
                                 int64_t workspace_bytes, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(nx >= 0 && ny >= 0 && nx < (int64_t)INT32_MAX && ny < (int64_t)INT32_MAX,
               "dc_neighbors_fill: bad sizes (nx=%lld, ny=%lld)", (long long)nx, (long long)ny);
    DC_REQUIRE(cap >= 0 && cap <= kMaxCap, "dc_neighbors_fill: cap=%d outside [0, %d]", cap, kMaxCap);
    DC_REQUIRE(mode == DC_NEIGHBORS_KNN || mode == DC_NEIGHBORS_RADIUS, "dc_neighbors_fill: unknown mode %d", mode);
    DC_REQUIRE(mode == DC_NEIGHBORS_KNN || r >= 0.0f, "dc_neighbors_fill: radius %g is not >= 0", (double)r);
    DC_REQUIRE((nx == 0 || ldx >= 3) && (ny == 0 || ldy >= 3), "dc_neighbors_fill: leading dimension below 3");
    if (ny == 0) return DC_OK;
    DC_REQUIRE(y && counts && (cap == 0 || nbr), "dc_neighbors_fill: null pointer");
    if (nx == 0 || cap == 0) {
        DC_LAUNCH(k_no_neighbors, dim3((unsigned)((ny * (cap > 0 ? cap : 1) + 255) / 256)), dim3(256), 0, stream, nbr,
                  cap, counts, ny);
        return check_launch("dc_neighbors_fill");
    }
    DC_REQUIRE(x && workspace && workspace_bytes >= dc_neighbors_workspace_bytes(nx, ny),
               "dc_neighbors_fill: null pointer or workspace too small");
    // r*r rounded once in fp32; rho_max = the smallest float with fl(rho_max^2) >= r2: a point outside the box of
    // rho_max then has d2 >= r2 and fails d2 < r2
    const float r2 = r * r;
    float rho_max = sqrtf(r2);
    while (rho_max * rho_max < r2) rho_max = nextafterf(rho_max, INFINITY);
    const int radius_mode = mode == DC_NEIGHBORS_RADIUS;

    const FillLayout W(nx);
    char *ws = (char *)workspace;
    unsigned *bbox = (unsigned *)(ws + W.bbox);
    int32_t *seg = (int32_t *)(ws + W.seg);
    GridParams *params = (GridParams *)(ws + W.params);
    unsigned long long *keys_in = (unsigned long long *)(ws + W.keys_in), *keys_out = (unsigned long long *)(ws + W.keys_out);
    int32_t *vals_in = (int32_t *)(ws + W.vals_in), *vals_out = (int32_t *)(ws + W.vals_out);
    float4 *spos = (float4 *)(ws + W.spos);
    size_t temp_bytes = sort_temp_bytes(nx);

    const unsigned nb = (unsigned)((nx + 255) / 256);
    DC_LAUNCH(k_bbox_init_seg, dim3((unsigned)((6 * nx + 255) / 256)), dim3(256), 0, stream, bbox, nx);
    const int64_t waves = (nx + kBboxChunk - 1) / kBboxChunk;
    DC_LAUNCH(k_seg_bbox, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, x, ldx, nx, batch_x, seg, bbox);
    DC_LAUNCH(k_grid_params, dim3(nb), dim3(256), 0, stream, (const unsigned *)bbox, (const int32_t *)seg, batch_x, nx,
              radius_mode, rho_max, params);
    DC_LAUNCH(k_cell_keys, dim3(nb), dim3(256), 0, stream, x, ldx, nx, (const int32_t *)seg,
              (const GridParams *)params, keys_in, vals_in);
    trace_kernel("rocprim::radix_sort_pairs");
    // stable: points of one cell stay in index order
    if (rocprim::radix_sort_pairs(ws + W.temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)nx, 0,
                                  key_end_bit(nx), stream) != hipSuccess)
        return check_launch("dc_neighbors_fill (sort)");
    DC_LAUNCH(k_sorted_points, dim3(nb), dim3(256), 0, stream, x, ldx, nx, (const int32_t *)vals_out, spos);
    DC_LAUNCH(k_query, dim3((unsigned)((ny + 3) / 4)), dim3(256), 0, stream, y, ldy, ny, batch_y, batch_x, nx,
              (const GridParams *)params, (const unsigned long long *)keys_out, (const float4 *)spos, cap, radius_mode,
              r2, rho_max, exclude_self, nbr, counts);
    return check_launch("dc_neighbors_fill");
}

extern "C" int64_t dc_neighbors_compact_workspace_bytes(int64_t ny) {
    if (ny < 0 || ny >= (int64_t)INT32_MAX) return -1;
    return ny == 0 ? 0 : al256(8 * ny) + al256((int64_t)scan_temp_bytes(ny));
}

extern "C" int dc_neighbors_compact(const int32_t *nbr, int cap, const int32_t *counts, int64_t ny, int query_row,
                                    int64_t *edge_index, int64_t num_edges, void *workspace, int64_t workspace_bytes,
                                    dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(ny >= 0 && ny < (int64_t)INT32_MAX && num_edges >= 0, "dc_neighbors_compact: bad sizes (ny=%lld, "
               "num_edges=%lld)", (long long)ny, (long long)num_edges);
    DC_REQUIRE(cap >= 0 && cap <= kMaxCap, "dc_neighbors_compact: cap=%d outside [0, %d]", cap, kMaxCap);
    DC_REQUIRE(query_row == 0 || query_row == 1, "dc_neighbors_compact: query_row must be 0 or 1");
    if (ny == 0 || cap == 0 || num_edges == 0) return DC_OK;
    DC_REQUIRE(nbr && counts && edge_index && workspace &&
                   workspace_bytes >= dc_neighbors_compact_workspace_bytes(ny),
               "dc_neighbors_compact: null pointer or workspace too small");
    int64_t *incl = (int64_t *)workspace;
    size_t temp_bytes = scan_temp_bytes(ny);
    trace_kernel("rocprim::inclusive_scan");
    auto in = rocprim::make_transform_iterator(counts, CountAsI64{cap});
    if (rocprim::inclusive_scan((char *)workspace + al256(8 * ny), temp_bytes, in, incl, (size_t)ny,
                                rocprim::plus<int64_t>(), stream) != hipSuccess)
        return check_launch("dc_neighbors_compact (scan)");
    DC_LAUNCH(k_compact, dim3((unsigned)((ny * cap + 255) / 256)), dim3(256), 0, stream, nbr, cap, counts,
              (const int64_t *)incl, ny, query_row, edge_index, num_edges);
    return check_launch("dc_neighbors_compact");
}
