// dc_dense_narrow.hip -- the dense block of a TAGConv layer with a SHORT reduction: the first layer of each encoder branch
// (/root/reference/models/model.py:44-50: TAGConv(21, 256) / TAGConv(25, 256), K = 3 -> reduction (K + 1) * F_in = 84 / 100,
// zero-padded to 96 / 112 in the hop slab).
//
//   out[N, 256] = act(slab[N, Kp] . Wcat[256, Kp]^T + b),   Wcat = [W_0 | W_1 | W_2 | W_3 | 0]  (lins[k].weight of PyG tag_conv.py)
//
// Round 6 measured what these layers cost the two-stream headline step by making them free (tools/r06/skip_probe.py): forward
// blocks 53 us, weight-gradient blocks 64 us, hops 36 us of a 617 us step - all of it on the critical path, none hidden by the
// second stream.  The generic split kernel (dc_dense_split.hip: k_fwd_split, 128 x 128 tiles, both operands split per tile and
// stage, 4-byte epilogue stores) took 25.7 / 20.7 us for 46 / 35 MB of compulsory traffic (0.22 of the HBM roofline) and
// needed a packing launch for Wcat in front of it.
//
// This kernel is built for the shape: the whole reduction is ONE stage.
//   * persistent 256-thread workgroups, one per CU; wave w owns output columns [64 w, 64 w + 64) and keeps ITS slice of the
//     weights - read from the K + 1 lins[k].weight matrices themselves (no packing launch: coalesced reads into an fp32 LDS
//     image, fragments picked out of it), split into the three bf16 planes once per launch - in registers for all row tiles
//     (24 * Kp / 16 VGPRs; one wave per SIMD, 512 registers each);
//   * per row tile (64 or 32 rows): fp32 rows global -> registers (issued one tile ahead) -> three bf16 planes -> LDS (rows
//     padded to Kp * 6 + 16 bytes: conflict-free ds_read_b128 fragment reads), one barrier, 6 products x Kp / 16 k-steps of
//     v_mfma_f32_32x32x16_bf16 per accumulator IN THE ORDER of k_fwd_split<., 6> (k-steps ascending, products smallest terms
//     first) - the outputs are bit-identical to it (tests/test_narrow_dense.py);
//   * epilogue through LDS: bias + ReLU in registers, accumulators into a [rows][256] fp32 image, one barrier, one 1-KiB row per
//     global_store_dwordx4 wave-instruction (the 4-byte stores of the accumulator layout cost 7.6 us per 33.5 MB).
// Bytes per launch (B = 32): 12.6 + 33.5 MB soft, 10.9 + 25.0 MB rigid; MFMA work 9.7 / 8.4 GFLOP: HBM-bound.
//
// Two forms of the first bullet.  k_fwd_narrow prepares the weights itself, in every workgroup, as described there (one
// workgroup per CU: the fp32 LDS image).  k_fwd_narrow_img - what the layer runs - takes them prepared once per call
// (dc_narrow_image.h) and runs two workgroups per CU: 16.3 / 14.9 us against 24.3 / 23.5 us (profiles/r11).
#include "dc_dense.h"
#include "dc_narrow_image.h"

namespace dc {

struct NarrowParams {
    const float *x;                 // hop slab [N, ld], Kp valid (zero-padded) columns
    int64_t ld;
    const float *w[kMaxSeg];        // lins[k].weight [Fo, fi]
    int nseg, fi;
    const float *bias;
    float *out;
    int64_t ldo, N;
    int relu, ntiles;
};

// The two barriers per tile are lds_barrier(), NOT __syncthreads(): its fence waits for vmcnt(0) - for the next tile's rows
// (issued one tile ahead on purpose) and for the previous tile's 64 KB of row stores - which put two memory round trips per
// tile on the critical path (30 us per launch instead of 12)

// The block's own weight prologue (k_fwd_narrow: the weights as the K + 1 lins[k].weight matrices) -> fb, this wave's
// fragments.
// First Wcat = [W_0 | ... | W_{nseg-1} | 0] as an fp32 image [256][Kp] in LDS, gathered with COALESCED reads of the
// lins[k].weight matrices (element e of segment s = row e / fi, column e % fi; a per-lane gather of the fragments straight
// from memory - 8 strided 4-byte loads per fragment - cost 20 us per launch: every workgroup made 7 M cache-line requests);
// then every lane picks its fragments out of the image: column 64 wid + 32 nb + c, k = 16 ks + 8 h .. + 7.
template <int KS>
__device__ __forceinline__ void narrow_self_weights(const NarrowParams &p, char *lds, bf16x8 (&fb)[2][KS][3]) {
    constexpr int KP = 16 * KS;
    constexpr int WROW = KP + 4;                        // image row in floats: +16 B keeps the fragment picks conflict-free
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    {
        // ALL loads (every segment) are issued before the first is used: a load per loop trip waited for each one in turn
        // (84 round trips to L2, 25 us per launch); a batch per segment still made four round trips
        float *wi = reinterpret_cast<float *>(lds);
        const int width = p.nseg * p.fi, per4 = kNarrowFo * p.fi / 4;         // float4 pieces per segment (256 fi / 4)
        constexpr int MAXQ = 8;                                              // fi <= 32
        f32x4 wv[kMaxSeg][MAXQ];
#pragma unroll
        for (int s = 0; s < kMaxSeg; ++s)
#pragma unroll
            for (int j = 0; j < MAXQ; ++j) {
                const int q = (int)threadIdx.x + 256 * j;
                if (s < p.nseg && q < per4) wv[s][j] = *reinterpret_cast<const f32x4 *>(p.w[s] + 4 * q);
            }
#pragma unroll
        for (int s = 0; s < kMaxSeg; ++s)
#pragma unroll
            for (int j = 0; j < MAXQ; ++j) {
                const int q = (int)threadIdx.x + 256 * j;
                if (s < p.nseg && q < per4) {
                    int o = (4 * q) / p.fi, f = 4 * q - o * p.fi;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        wi[o * WROW + s * p.fi + f] = wv[s][j][i];
                        if (++f == p.fi) f = 0, ++o;
                    }
                }
            }
        const int padw = KP - width;
        for (int e = threadIdx.x; e < kNarrowFo * padw; e += 256) {
            const int o = e / padw, f = e - o * padw;
            wi[o * WROW + width + f] = 0.f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const float *wr = reinterpret_cast<const float *>(lds) + (64 * wid + 32 * nb + c) * WROW + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(wr + 16 * ks);
            const f32x4 v1 = *reinterpret_cast<const f32x4 *>(wr + 16 * ks + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 hi, mid, lo;
                split1(j < 4 ? v0[j] : v1[j - 4], hi, mid, lo);
                fb[nb][ks][0][j] = hi, fb[nb][ks][1][j] = mid, fb[nb][ks][2][j] = lo;
            }
        }
    }
    __syncthreads();                                    // the image's LDS becomes the plane / staging images
}

// The block, in both forms.  KS: k-steps of 16 (Kp = 16 KS); MB: 32-row blocks per tile.
// WIMG: the weights come PREPARED - `img`, the bf16x3 fragment image of dc_narrow_image.h, written once per call by the
// layer's pack launch (or k_narrow_wimage below) - instead of being prepared by every one of the 256 workgroups (all K + 1
// weight matrices into a 102 KB fp32 LDS image, fragments picked, split1 on 256 x Kp numbers: 3.8 + ~2 us of a 23 us
// launch).  The prologue is then 2 KS 3 coalesced 1-KiB wave loads from L2, issued behind the first tile's rows and
// before anything is used: no LDS image, no barrier, and LDS is the tile images alone (52 / 55 / 58 KB) - TWO workgroups
// fit a CU (256 registers per lane) and one's loads, split and row stores run under the other's MFMAs.  Same tiles,
// k-step order, product order, bias, ReLU: the same bits.
// LATE: the next tile's rows are asked for BEHIND the MFMAs (they then travel under the other workgroup's): with seven
// k-steps their 16 registers beside 168 of fragments, 32 of accumulators and 12 of A fragments do not fit 256 (18 spilled).
template <int KS, int MB, bool WIMG, bool LATE>
__device__ __forceinline__ void narrow_block(const NarrowParams &p, const bf16x8 *__restrict__ img) {
    constexpr int TR = 32 * MB;                         // rows per tile
    constexpr int SROWA = KS * 96 + 16;                 // bytes per row of the plane image: [ks][plane][half][8 bf16] + pad
    constexpr int PPR = 4 * KS;                         // float4 pieces per row
    constexpr int TP = TR * PPR, NV = (TP + 255) / 256;
    constexpr int KP = 16 * KS;                         // padded reduction
    constexpr int kOffStage = ((TR * SROWA + 1023) / 1024) * 1024;
    constexpr int kLdsTiles = kOffStage + TR * 1024, kLdsW = kNarrowFo * (KP + 4) * 4;      // tile images / prologue weight image
    __shared__ __attribute__((aligned(1024))) char lds[(WIMG || kLdsTiles > kLdsW) ? kLdsTiles : kLdsW];
    char *const sA = lds;
    float *const so = reinterpret_cast<float *>(lds + kOffStage);
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;

    // ---- x tile staging: piece q = threadIdx.x + 256 j of the tile = float4 c4 of row r ----
    f32x4 xv[NV];
    auto load_tile = [&](int t) {
        const int64_t row0 = (int64_t)t * TR;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = (int)threadIdx.x + 256 * j;
            if (TP % 256 != 0 && q >= TP) continue;
            const int r = q / PPR, c4 = q - r * PPR;
            int64_t row = row0 + r;
            row = row < p.N ? row : p.N - 1;
            xv[j] = *reinterpret_cast<const f32x4 *>(p.x + row * p.ld + 4 * c4);
        }
    };
    int t = blockIdx.x;
    if (t < p.ntiles) load_tile(t);                     // the first tile's rows travel while the weights are prepared

    // ---- this wave's slice of the weights: fragments of all k-steps, three planes, in registers for the whole launch ----
    bf16x8 fb[2][KS][3];
    if constexpr (WIMG) {
        // columns [64 wid, 64 wid + 64) = column blocks 2 wid, 2 wid + 1 of the image
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    fb[nb][ks][pl] = img[((ks * 3 + pl) * 8 + 2 * wid + nb) * 64 + lane];
                }
    } else {
        narrow_self_weights<KS>(p, lds, fb);
    }
    float bcol[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) bcol[nb] = p.bias ? p.bias[64 * wid + 32 * nb + c] : 0.f;
    const bool relu = p.relu != 0;

    auto store_tile = [&]() {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int q = (int)threadIdx.x + 256 * j;
            if (TP % 256 != 0 && q >= TP) continue;
            const int r = q / PPR, c4 = q - r * PPR;
            bf16x4 hi, mid, lo;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __bf16 a, b, d;
                split1(xv[j][i], a, b, d);
                hi[i] = a, mid[i] = b, lo[i] = d;
            }
            // k = 4 c4 .. + 3: k-step c4 / 4, half (c4 & 3) / 2, position 4 (c4 & 1) inside the half's 8
            char *dst = sA + r * SROWA + (c4 >> 2) * 96 + ((c4 >> 1) & 1) * 16 + (c4 & 1) * 8;
            *reinterpret_cast<bf16x4 *>(dst) = hi;
            *reinterpret_cast<bf16x4 *>(dst + 32) = mid;
            *reinterpret_cast<bf16x4 *>(dst + 64) = lo;
        }
    };

    // one 1-KiB row per store instruction: wave w stores rows w, w + 4, ... of the staged tile
    auto store_rows = [&](int64_t row0) {
#pragma unroll 4
        for (int r = wid; r < TR; r += 4) {
            const int64_t row = row0 + r;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(so + r * 256 + 4 * lane);
            if (row < p.N) *reinterpret_cast<f32x4 *>(p.out + row * p.ldo + 4 * lane) = v;
        }
    };
    // Order inside an iteration (vector-memory operations retire in order, and hipcc's wait before the first use of the staged
    // rows is the conservative merge over both loop entries, i.e. vmcnt(0)): USE the rows of tile t (loaded one iteration ago,
    // the youngest operations in flight) -> row stores of tile t - 1 -> loads of tile t + 1 -> MFMAs of tile t.  Stores and
    // loads then travel under the MFMAs, and the wait at the top of the next iteration finds them a whole MFMA phase old.
    int64_t prev_row0 = -1;
    for (; t < p.ntiles; t += gridDim.x) {
        const int64_t row0 = (int64_t)t * TR;
        store_tile();                                   // (every wave is past the MFMAs of the previous tile: barrier B)
        if (prev_row0 >= 0) store_rows(prev_row0);
        if (!LATE && t + (int)gridDim.x < p.ntiles) load_tile(t + gridDim.x);
        lds_barrier();                               // A: the plane image is complete; the staging image has been read
        f32x16 acc[MB][2];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;
        constexpr int HI = 0, MID = 1, LO = 2;
        constexpr int pa6[6] = {LO, HI, MID, MID, HI, HI}, pb6[6] = {HI, LO, MID, HI, MID, HI};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 fa[MB][3];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    fa[mb][pl] = *reinterpret_cast<const bf16x8 *>(sA + (mb * 32 + c) * SROWA + ks * 96 + pl * 32 + h * 16);
#pragma unroll
            for (int tt = 0; tt < 6; ++tt)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mb][pa6[tt]], fb[nb][ks][pb6[tt]], acc[mb][nb], 0, 0, 0);
        }
        if (LATE && t + (int)gridDim.x < p.ntiles) load_tile(t + gridDim.x);
        // epilogue: bias + ReLU, accumulators -> [TR][256] image (C/D layout: row (reg & 3) + 8 (reg >> 2) + 4 h, column c)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[mb][nb][r] + bcol[nb];
                    if (relu) v = relu_keep_nan(v);
                    so[(mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 256 + 64 * wid + 32 * nb + c] = v;
                }
        lds_barrier();                               // B: image complete; every wave has read its plane fragments
        prev_row0 = row0;
    }
    if (prev_row0 >= 0) store_rows(prev_row0);
}

template <int KS, int MB>
__global__ void __launch_bounds__(256) k_fwd_narrow(NarrowParams p) { narrow_block<KS, MB, false, false>(p, nullptr); }

// WPC: workgroups per CU the register budget is for
template <int KS, int WPC>
__global__ void __launch_bounds__(256, WPC) k_fwd_narrow_img(NarrowParams p, const bf16x8 *__restrict__ img) {
    narrow_block<KS, 1, true, (WPC == 2 && KS > 6)>(p, img);
}

// the image on its own: calls in which no pack launch happens (cached hop slab, a caller's own slab)
__global__ void __launch_bounds__(256) k_narrow_wimage(NarrowImageParams q) { narrow_image_fill(q, (int)blockIdx.x); }

template <int KS, int WPC>
static void narrow_img_launch(const NarrowParams &p0, const void *img, hipStream_t hs) {
    NarrowParams p = p0;
    p.ntiles = (int)((p.N + 31) / 32);
    const int cap = 256 * WPC;              // workgroups per CU: two where 256 registers hold the fragments (wpad 96 / 112)
    const unsigned grid = (unsigned)(p.ntiles < cap ? p.ntiles : cap);
    DC_LAUNCH((k_fwd_narrow_img<KS, WPC>), dim3(grid), dim3(256), 0, hs, p, static_cast<const bf16x8 *>(img));
}

// 32-row tiles: four (soft) / three (rigid) per persistent workgroup at B = 32 - measured 23.1 / 20.8 us against 25.1 / 22.6 us with
// 64-row tiles (MB = 2: two / one and a half per workgroup; profiles/r06/e_narrow_time.txt)
template <int KS>
static void narrow_launch(const NarrowParams &p0, hipStream_t hs) {
    NarrowParams p = p0;
    p.ntiles = (int)((p.N + 31) / 32);
    const unsigned grid = (unsigned)(p.ntiles < 256 ? p.ntiles : 256);
    DC_LAUNCH((k_fwd_narrow<KS, 1>), dim3(grid), dim3(256), 0, hs, p);
}

}  // namespace dc

using namespace dc;

// Whether dc_tag_linear_fwd_narrow takes this shape (host-side query; the entry itself returns DC_EINVAL otherwise)
extern "C" int dc_tag_linear_fwd_narrow_ok(int64_t fi, int nseg, int64_t wpad, int64_t Fo) {
    return (Fo == kNarrowFo && nseg >= 1 && nseg <= kMaxSeg && fi >= 1 && fi <= 32 && nseg * fi <= wpad &&
            (wpad == 96 || wpad == 112 || wpad == 128)) ? 1 : 0;
}

extern "C" int dc_tag_linear_fwd_narrow(const float *slab, int64_t ld, const float *const *ws, int nseg, int64_t fi,
                                        const float *bias, int relu, float *out, int64_t ldo, int64_t N, int64_t wpad,
                                        int64_t Fo, dc_stream_t stream) {
    DC_REQUIRE(dc_tag_linear_fwd_narrow_ok(fi, nseg, wpad, Fo),
               "dc_tag_linear_fwd_narrow: needs Fo = 256, a padded reduction of 96 / 112 / 128 >= nseg * fi (got Fo=%lld wpad=%lld "
               "nseg=%d fi=%lld)", (long long)Fo, (long long)wpad, nseg, (long long)fi);
    DC_REQUIRE(N >= 0, "dc_tag_linear_fwd_narrow: negative N");
    if (N == 0) return DC_OK;
    DC_REQUIRE(slab && ws && out && ld >= wpad && ldo >= Fo, "dc_tag_linear_fwd_narrow: null pointer / short leading dimension");
    DC_REQUIRE(ld % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)slab & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "dc_tag_linear_fwd_narrow: rows of the slab and of the output must be 16-byte aligned");
    DC_REQUIRE(N < ((int64_t)1 << 31) - 64, "dc_tag_linear_fwd_narrow: too many rows");
    NarrowParams p{};
    p.x = slab, p.ld = ld, p.nseg = nseg, p.fi = (int)fi, p.bias = bias, p.out = out, p.ldo = ldo, p.N = N, p.relu = relu;
    for (int s = 0; s < nseg; ++s) {
        DC_REQUIRE(ws[s], "dc_tag_linear_fwd_narrow: null weight segment %d", s);
        // (this kernel's prologue reads the weights 16 bytes at a time; dc_tag_linear_fwd_narrow_img takes any 4-byte address)
        DC_REQUIRE(al16(ws[s]), "dc_tag_linear_fwd_narrow: weight segment %d is not 16-byte aligned", s);
        p.w[s] = ws[s];
    }
    hipStream_t hs = (hipStream_t)stream;
    switch (wpad) {
    case 96: narrow_launch<6>(p, hs); break;
    case 112: narrow_launch<7>(p, hs); break;
    default: narrow_launch<8>(p, hs); break;
    }
    return check_launch("dc_tag_linear_fwd_narrow");
}

extern "C" int dc_tag_narrow_wimage(const float *const *ws, int nseg, int64_t fi, int64_t wpad, void *wimg,
                                    dc_stream_t stream) {
    DC_REQUIRE(narrow_image_args_ok(ws, nseg, fi, wpad, wimg),
               "dc_tag_narrow_wimage: needs 1..%d 4-byte-aligned weight segments [256, fi <= 32], a padded reduction of 96 / "
               "112 / 128 >= nseg * fi and a 16-byte-aligned image (got nseg=%d fi=%lld wpad=%lld)", kMaxSeg, nseg,
               (long long)fi, (long long)wpad);
    const NarrowImageParams q = narrow_image_params(ws, nseg, fi, wpad, wimg);
    DC_LAUNCH(k_narrow_wimage, dim3((unsigned)narrow_image_blocks(q.ks)), dim3(256), 0, (hipStream_t)stream, q);
    return check_launch("dc_tag_narrow_wimage");
}

extern "C" int dc_tag_linear_fwd_narrow_img(const float *slab, int64_t ld, const void *wimg, const float *bias, int relu,
                                            float *out, int64_t ldo, int64_t N, int64_t wpad, int64_t Fo,
                                            dc_stream_t stream) {
    DC_REQUIRE(Fo == kNarrowFo && (wpad == 96 || wpad == 112 || wpad == 128),
               "dc_tag_linear_fwd_narrow_img: needs Fo = 256 and a padded reduction of 96 / 112 / 128 (got Fo=%lld wpad=%lld)",
               (long long)Fo, (long long)wpad);
    DC_REQUIRE(N >= 0, "dc_tag_linear_fwd_narrow_img: negative N");
    if (N == 0) return DC_OK;
    DC_REQUIRE(slab && wimg && out && ld >= wpad && ldo >= Fo, "dc_tag_linear_fwd_narrow_img: null pointer / short leading dimension");
    DC_REQUIRE(ld % 4 == 0 && ldo % 4 == 0 && al16(slab) && al16(out) && al16(wimg),
               "dc_tag_linear_fwd_narrow_img: rows of the slab and of the output and the image must be 16-byte aligned");
    DC_REQUIRE(N < ((int64_t)1 << 31) - 64, "dc_tag_linear_fwd_narrow_img: too many rows");
    NarrowParams p{};
    p.x = slab, p.ld = ld, p.bias = bias, p.out = out, p.ldo = ldo, p.N = N, p.relu = relu;
    hipStream_t hs = (hipStream_t)stream;
    switch (wpad) {
    case 96: narrow_img_launch<6, 2>(p, wimg, hs); break;
    case 112: narrow_img_launch<7, 2>(p, wimg, hs); break;
    default: narrow_img_launch<8, 1>(p, wimg, hs); break;
    }
    return check_launch("dc_tag_linear_fwd_narrow_img");
}
