// dc_dense_prep.hip -- operand preparation for the fp16x2 ("h2") dense blocks (gfx950): the row maxima that set the
// power-of-two scales (dc_dense.h: H2Scales), the masked gradient, and the scaled, split weight images.
//
//   dc_rowabsmax_f32         : rowmax[i] = max |x[i, :]|
//   dc_tag_weight_rowmax     : w_rowmax[o] = max_s,f |W_s[o, f]|
//   dc_tag_mask_grad         : gm = g * (out > 0) and its row maxima
//   dc_tag_weight_prep(_zero): row maxima and fp16x2 images of the weights and of their transposes, one launch
//                              (three for tall matrices); k_weight_prep_grouped does the same for the grouped entry
//                              of dc_dense.hip
//   dc_tag_transpose_weights : wt[s][f][o] = ws[s][o][f] (the kernel is in dc_dense_split.hip)
#include "dc_dense.h"

namespace dc {

// rowmax[i] = max |x[i, 0:F]| : one wave per row
__global__ void __launch_bounds__(256)
k_rowabsmax(const float *__restrict__ x, int64_t ld, int64_t N, int F, float *__restrict__ rowmax,
            bool vec4) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const float *xr = x + row * ld;
    float m = 0.f;
    if (vec4) {
        for (int c = lane * 4; c < F; c += 256) {
            const float4 v = *reinterpret_cast<const float4 *>(xr + c);
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
    } else {
        for (int c = lane; c < F; c += 64) m = fmaxf(m, fabsf(xr[c]));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) rowmax[row] = m;
}

// out[o] = max over segments s and columns f of |W_s[o, f]| : one wave per output row
struct WRowmaxParams {
    const float *w[kMaxSeg];
    int nseg;
    int64_t Fo, Fi;
    float *out;
};
__global__ void __launch_bounds__(256) k_w_rowmax(WRowmaxParams p) {
    const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= p.Fo) return;
    const int lane = threadIdx.x & 63;
    float m = 0.f;
    for (int s = 0; s < p.nseg; ++s) {
        const float *wr = p.w[s] + o * p.Fi;
        for (int64_t c = lane; c < p.Fi; c += 64) m = fmaxf(m, fabsf(wr[c]));
    }
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) m = fmaxf(m, __shfl_xor(m, q));
    if (lane == 0) p.out[o] = m;
}

// gm[i,:] = g[i,:] * (out[i,:] > 0), rowmax[i] = max |gm[i,:]| : one wave per row
__global__ void __launch_bounds__(256)
k_mask_grad(const float *__restrict__ g, int64_t ldg, const float *__restrict__ mask, int64_t ldm,
            float *__restrict__ gm, int64_t ldgm, int64_t N, int F, float *__restrict__ rowmax_a,
            float *__restrict__ rowmax_b, bool vec4) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const float *gr = g + row * ldg, *mr = mask ? mask + row * ldm : nullptr;
    float *o = gm + row * ldgm;
    float m = 0.f;
    if (vec4) {
        for (int c = lane * 4; c < F; c += 256) {
            float4 v = *reinterpret_cast<const float4 *>(gr + c);
            if (mr) {
                const float4 k = *reinterpret_cast<const float4 *>(mr + c);
                v = make_float4(k.x > 0.f ? v.x : 0.f, k.y > 0.f ? v.y : 0.f, k.z > 0.f ? v.z : 0.f,
                                k.w > 0.f ? v.w : 0.f);
            }
            *reinterpret_cast<float4 *>(o + c) = v;
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
    } else {
        for (int c = lane; c < F; c += 64) {
            float v = gr[c];
            if (mr && !(mr[c] > 0.f)) v = 0.f;
            o[c] = v;
            m = fmaxf(m, fabsf(v));
        }
    }
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) m = fmaxf(m, __shfl_xor(m, q));
    if (lane == 0) {
        rowmax_a[row] = m;
        if (rowmax_b) rowmax_b[row] = m;
    }
}

// Everything the h2 dense blocks of one TAGConv layer need from its weights, in ONE launch:
//   blocks [0, ceil(Fo/4))          : w_rowmax[o] = max_s,f |W_s[o,f]| and (optional) the scaled
//                                     fp16x2 image of row o over the concatenated reduction
//                                     k = s*Fi + f  (wave per row o, two passes over its 4 KiB)
//   blocks [ceil(Fo/4), +ceil(Fi/4)): the same for the transposed weights: wt_rowmax[f] =
//                                     max_s,o |W_s[o,f]| and the image of row f over k = s*Fo + o
//                                     (wave per column f: strided reads of the L2-resident weights)
// Image of a row: per 16-wide stage one 64-byte record {h1[16], h2[16]} (fp16), x * 2^e = h1 + h2
// with the row's power-of-two scale (dc_dense.h) - the bytes k_fwd_h2 wants in LDS, so that kernel
// stages the weights by LDS-DMA without touching registers or the VALU.
__device__ __forceinline__ void wprep_put(_Float16 *img_row, int64_t k, float v, float scale) {
    const float x = v * scale;
    const _Float16 h = (_Float16)x;
    _Float16 *rec = img_row + (k >> 4) * 32 + (k & 15);
    rec[0] = h;
    rec[16] = (_Float16)(x - (float)h);
}
__device__ __forceinline__ void weight_prep_body(const WPrepParams &p) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.zero_n; i += (int64_t)gridDim.x * blockDim.x)
        p.zero[i] = 0.f;
    if (p.tall)
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.Fi; i += (int64_t)gridDim.x * blockDim.x)
            p.wt_rowmax[i] = 0.f;
    const int64_t rb = (p.Fo + 3) / 4;
    float m = 0.f;
    // up to 256 x 256 per segment (the encoder's layers) a wave keeps its row / column in registers between the maximum and the
    // image pass - one trip to L2 per wave instead of two dependent ones (round 6: the launch sits on each branch's critical path)
    const bool small = p.Fi <= 256 && p.Fo <= 256;
    if ((int64_t)blockIdx.x < rb) {
        const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (o >= p.Fo) return;
        float v[kMaxSeg][4];
        if (small) {
#pragma unroll
            for (int s = 0; s < kMaxSeg; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t c = lane + 64 * j;
                    v[s][j] = (s < p.nseg && c < p.Fi) ? p.w[s][o * p.Fi + c] : 0.f;
                    m = fmaxf(m, fabsf(v[s][j]));
                }
        } else {
            for (int s = 0; s < p.nseg; ++s) {
                const float *wr = p.w[s] + o * p.Fi;
                for (int64_t c = lane; c < p.Fi; c += 64) m = fmaxf(m, fabsf(wr[c]));
            }
        }
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) m = fmaxf(m, __shfl_xor(m, q));
        if (lane == 0) p.w_rowmax[o] = m;
        if (p.wimg) {
            const float sc = h2_scale(m);
            _Float16 *row = p.wimg + o * (2 * p.nseg * p.Fi);
            if (small) {
#pragma unroll
                for (int s = 0; s < kMaxSeg; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t c = lane + 64 * j;
                        if (s < p.nseg && c < p.Fi) wprep_put(row, s * p.Fi + c, v[s][j], sc);
                    }
            } else {
                for (int s = 0; s < p.nseg; ++s) {
                    const float *wr = p.w[s] + o * p.Fi;
                    for (int64_t c = lane; c < p.Fi; c += 64) wprep_put(row, s * p.Fi + c, wr[c], sc);
                }
            }
        }
    } else {
        const int64_t f = ((int64_t)blockIdx.x - rb) * 4 + (threadIdx.x >> 6);
        if (f >= p.Fi) return;
        float v[kMaxSeg][4];
        if (small) {
#pragma unroll
            for (int s = 0; s < kMaxSeg; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t o = lane + 64 * j;
                    v[s][j] = (s < p.nseg && o < p.Fo) ? p.w[s][o * p.Fi + f] : 0.f;
                    m = fmaxf(m, fabsf(v[s][j]));
                }
        } else {
            for (int s = 0; s < p.nseg; ++s) {
                const float *wc = p.w[s] + f;
                for (int64_t o = lane; o < p.Fo; o += 64) m = fmaxf(m, fabsf(wc[o * p.Fi]));
            }
        }
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) m = fmaxf(m, __shfl_xor(m, q));
        if (lane == 0) p.wt_rowmax[f] = m;
        const float sc = h2_scale(m);
        _Float16 *row = p.wtimg + f * (2 * p.nseg * p.Fo);
        if (small) {
#pragma unroll
            for (int s = 0; s < kMaxSeg; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t o = lane + 64 * j;
                    if (s < p.nseg && o < p.Fo) wprep_put(row, s * p.Fo + o, v[s][j], sc);
                }
        } else {
            for (int s = 0; s < p.nseg; ++s) {
                const float *wc = p.w[s] + f;
                for (int64_t o = lane; o < p.Fo; o += 64) wprep_put(row, s * p.Fo + o, wc[o * p.Fi], sc);
            }
        }
    }
}
__global__ void __launch_bounds__(256) k_weight_prep(WPrepParams p) { weight_prep_body(p); }
__global__ void __launch_bounds__(256) k_weight_prep_grouped(WPrepGroups q) { weight_prep_body(q.g[blockIdx.y]); }

// ---- the transposed half for TALL matrices (the attention's keys / values as "weights": Fo = 24,384 rows) ----------
// weight_prep_body gives a wave one column f and lets its lanes walk the rows: every lane of a load sits in another cache
// line - 0.8 GB of L2 requests and 193 us for a 25 MB matrix (6 launches, 1.2 ms of a batch-32 step).  Here the column
// maxima come from coalesced row reads (a thread per column, a block per 256-row chunk, joined with integer atomicMax:
// the values are non-negative floats) and the image from 64 x 64 tiles transposed through LDS; same scale, same
// rounding: wt_rowmax and the image are bit-identical to weight_prep_body's.
constexpr int kWtChunk = 256;
__global__ void __launch_bounds__(256)
k_wt_colmax(WPrepParams p) {
    const int64_t f = (int64_t)blockIdx.y * 256 + threadIdx.x;
    const int64_t o0 = (int64_t)blockIdx.x * kWtChunk, o1 = o0 + kWtChunk < p.Fo ? o0 + kWtChunk : p.Fo;
    if (f >= p.Fi) return;
    float m = 0.f;
    for (int s = 0; s < p.nseg; ++s) {
        const float *wc = p.w[s] + f;
        for (int64_t o = o0; o < o1; ++o) m = fmaxf(m, fabsf(wc[o * p.Fi]));
    }
    atomicMax(reinterpret_cast<int *>(p.wt_rowmax + f), __float_as_int(m));
}

// tile: 64 rows o x 64 columns f of segment s (blockIdx.z); needs Fo % 16 == 0 (records do not straddle segments)
__global__ void __launch_bounds__(256)
k_wt_image(WPrepParams p) {
    __shared__ _Float16 sh[64][64 + 8], sl[64][64 + 8];                  // [f][o]: the two planes of the tile, transposed
    __shared__ float ssc[64];
    const int s = blockIdx.z;
    const int64_t o0 = (int64_t)blockIdx.x * 64, f0 = (int64_t)blockIdx.y * 64;
    if (threadIdx.x < 64) {
        const int64_t f = f0 + threadIdx.x;
        ssc[threadIdx.x] = h2_scale(f < p.Fi ? p.wt_rowmax[f] : 0.f);
    }
    __syncthreads();
    const int c = threadIdx.x & 63, r4 = threadIdx.x >> 6;               // column of the tile, row phase
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
        const int r = r4 + 4 * j;
        const int64_t o = o0 + r, f = f0 + c;
        float v = 0.f;
        if (o < p.Fo && f < p.Fi) v = p.w[s][o * p.Fi + f];             // a wave reads 256 contiguous bytes of a row
        const float x = v * ssc[c];
        const _Float16 h = (_Float16)x;
        sh[c][r] = h;
        sl[c][r] = (_Float16)(x - (float)h);
    }
    __syncthreads();
    // one 64-byte record {h1[16], h2[16]} per thread: column f0 + t / 4, rows o0 + 16 (t % 4) .. + 15
    const int fc = threadIdx.x >> 2, rec = threadIdx.x & 3;
    const int64_t f = f0 + fc, ob = o0 + 16 * rec;
    if (f < p.Fi && ob < p.Fo) {
        _Float16 *dst = p.wtimg + f * (2 * p.nseg * p.Fo) + (((int64_t)s * p.Fo + ob) >> 4) * 32;
        const f16x8 *ph = reinterpret_cast<const f16x8 *>(&sh[fc][16 * rec]), *pl = reinterpret_cast<const f16x8 *>(&sl[fc][16 * rec]);
        f16x8 *d = reinterpret_cast<f16x8 *>(dst);
        d[0] = ph[0], d[1] = ph[1], d[2] = pl[0], d[3] = pl[1];
    }
}

void weight_prep_grouped_launch(const WPrepGroups &q, int64_t blocks, int ngroups, hipStream_t hs) {
    DC_LAUNCH(k_weight_prep_grouped, dim3((unsigned)blocks, (unsigned)ngroups), dim3(256), 0, hs, q);
}
}  // namespace dc

using namespace dc;

extern "C" int dc_tag_mask_grad(const float *g, int64_t ldg, const float *out_for_mask, int64_t ldo,
                                float *gm, int64_t ldgm, int64_t N, int64_t F, float *rowmax_a,
                                float *rowmax_b, dc_stream_t stream) {
    DC_REQUIRE(N >= 0 && F >= 1 && F < (1 << 24) && ldg >= F && ldgm >= F && (!out_for_mask || ldo >= F),
               "dc_tag_mask_grad: bad sizes");
    if (N == 0) return DC_OK;
    DC_REQUIRE(g && gm && rowmax_a, "dc_tag_mask_grad: null pointer");
    const bool vec4 = (F % 4 == 0) && (ldg % 4 == 0) && (ldgm % 4 == 0) && (((uintptr_t)g) & 15) == 0 &&
                      (((uintptr_t)gm) & 15) == 0 &&
                      (!out_for_mask || ((ldo % 4 == 0) && (((uintptr_t)out_for_mask) & 15) == 0));
    DC_LAUNCH(k_mask_grad, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g,
                       ldg, out_for_mask, ldo, gm, ldgm, N, (int)F, rowmax_a, rowmax_b, vec4);
    return check_launch("dc_tag_mask_grad");
}

extern "C" int dc_tag_weight_prep_zero(const float *const *ws, int nseg, int64_t Fo, int64_t Fi, float *w_rowmax,
                                       void *w_image, void *wt_image, float *wt_rowmax, float *zero, int64_t zero_n,
                                       dc_stream_t stream) {
    DC_REQUIRE(zero_n >= 0 && (zero_n == 0 || zero), "dc_tag_weight_prep_zero: bad zero buffer");
    DC_REQUIRE(nseg >= 1 && nseg <= kMaxSeg && Fo >= 1 && Fi >= 1 && ws && w_rowmax,
               "dc_tag_weight_prep: bad arguments");
    DC_REQUIRE((wt_image == nullptr) == (wt_rowmax == nullptr),
               "dc_tag_weight_prep: wt_image and wt_rowmax go together");
    DC_REQUIRE((!w_image || (nseg * Fi) % 16 == 0) && (!wt_image || (nseg * Fo) % 16 == 0),
               "dc_tag_weight_prep: images need a reduction extent that is a multiple of 16");
    DC_REQUIRE((((uintptr_t)w_image) & 15) == 0 && (((uintptr_t)wt_image) & 15) == 0,
               "dc_tag_weight_prep: images must be 16-byte aligned");
    WPrepParams p{};
    for (int s = 0; s < nseg; ++s) {
        DC_REQUIRE(ws[s], "dc_tag_weight_prep: null segment %d", s);
        p.w[s] = ws[s];
    }
    p.nseg = nseg, p.Fo = Fo, p.Fi = Fi, p.w_rowmax = w_rowmax, p.wt_rowmax = wt_rowmax;
    p.wimg = (_Float16 *)w_image, p.wtimg = (_Float16 *)wt_image;
    p.zero = zero, p.zero_n = zero_n;
    constexpr int tall_min = 2048;
    const bool tall = wt_image && Fo >= tall_min && Fo % 16 == 0;
    p.tall = tall ? 1 : 0;
    const int64_t blocks = (Fo + 3) / 4 + ((wt_image && !tall) ? (Fi + 3) / 4 : 0);
    DC_LAUNCH(k_weight_prep, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    if (tall) {
        DC_LAUNCH(k_wt_colmax, dim3((unsigned)((Fo + kWtChunk - 1) / kWtChunk), (unsigned)((Fi + 255) / 256)), dim3(256), 0,
                  (hipStream_t)stream, p);
        DC_LAUNCH(k_wt_image, dim3((unsigned)((Fo + 63) / 64), (unsigned)((Fi + 63) / 64), (unsigned)nseg), dim3(256), 0,
                  (hipStream_t)stream, p);
    }
    return check_launch("dc_tag_weight_prep");
}

extern "C" int dc_tag_weight_prep(const float *const *ws, int nseg, int64_t Fo, int64_t Fi,
                                  float *w_rowmax, void *w_image, void *wt_image, float *wt_rowmax,
                                  dc_stream_t stream) {
    return dc_tag_weight_prep_zero(ws, nseg, Fo, Fi, w_rowmax, w_image, wt_image, wt_rowmax, nullptr, 0, stream);
}

extern "C" int dc_rowabsmax_f32(const float *x, int64_t ld, int64_t N, int64_t F, float *rowmax,
                                dc_stream_t stream) {
    DC_REQUIRE(N >= 0 && F >= 1 && F < (1 << 24) && ld >= F, "dc_rowabsmax_f32: bad sizes");
    if (N == 0) return DC_OK;
    DC_REQUIRE(x && rowmax, "dc_rowabsmax_f32: null pointer");
    const bool vec4 = (F % 4 == 0) && (ld % 4 == 0) && (((uintptr_t)x) & 15) == 0;
    DC_LAUNCH(k_rowabsmax, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       x, ld, N, (int)F, rowmax, vec4);
    return check_launch("dc_rowabsmax_f32");
}

extern "C" int dc_tag_transpose_weights(const float *const *ws, int nseg, int64_t Fo, int64_t Fi,
                                        float *wt, dc_stream_t stream) {
    DC_REQUIRE(nseg >= 1 && nseg <= kMaxSeg && Fo >= 1 && Fi >= 1 && ws && wt,
               "dc_tag_transpose_weights: bad arguments");
    for (int s = 0; s < nseg; ++s) DC_REQUIRE(ws[s], "dc_tag_transpose_weights: null segment %d", s);
    transpose_weights_launch(ws, nseg, Fo, Fi, wt, (hipStream_t)stream);
    return check_launch("dc_tag_transpose_weights");
}

extern "C" int dc_tag_weight_rowmax(const float *const *ws, int nseg, int64_t Fo, int64_t Fi,
                                    float *w_rowmax, dc_stream_t stream) {
    DC_REQUIRE(nseg >= 1 && nseg <= kMaxSeg && Fo >= 1 && Fi >= 1 && ws && w_rowmax,
               "dc_tag_weight_rowmax: bad arguments");
    WRowmaxParams p{};
    for (int s = 0; s < nseg; ++s) {
        DC_REQUIRE(ws[s], "dc_tag_weight_rowmax: null segment %d", s);
        p.w[s] = ws[s];
    }
    p.nseg = nseg, p.Fo = Fo, p.Fi = Fi, p.out = w_rowmax;
    DC_LAUNCH(k_w_rowmax, dim3((unsigned)((Fo + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("dc_tag_weight_rowmax");
}
