// dc_narrow_image.h -- the prepared weights of the short-reduction forward block (dc_dense_narrow.hip: k_fwd_narrow_img):
// Wcat = [W_0 | ... | W_{nseg-1} | 0] (lins[k].weight of PyG tag_conv.py, [256, fi] each) split ONCE per call into the
// three bf16 planes of split1 and laid out in the order the kernel's lanes hold them as MFMA B fragments:
//
//   [KS k-steps][3 planes][8 column blocks of 32][64 lanes][8 bf16 = 16 B],   lane = c + 32 h
//
// record (ks, plane, block, lane) = plane `plane` of Wcat[32 block + c][16 ks + 8 h .. + 7]; columns k >= nseg * fi are
// zero.  24 KiB per k-step: 144 / 168 / 192 KiB for the padded reductions 96 / 112 / 128 - L2-resident; a wave of the
// forward block reads each of its fragments as one coalesced 1-KiB load.
//
// Two launches run the fill: the first layer's pack + first-hop launch carries it in a few workgroups behind its row
// blocks (dc_spmm.hip: k_spmm_sub_wimg), and a small kernel of its own does it where no such launch happens
// (dc_dense_narrow.hip: k_narrow_wimage).
#pragma once
#include "dc_dense.h"

namespace dc {

constexpr int kNarrowFo = 256;
constexpr int kNarrowImgStepBytes = 3 * 8 * 64 * 16;      // one k-step of the image

struct NarrowImageParams {
    const float *w[kMaxSeg];        // lins[k].weight [256, fi], any 4-byte-aligned address
    int nseg, fi, ks;               // ks k-steps of 16: the padded reduction
    void *img;                      // ks * kNarrowImgStepBytes, 16-byte aligned
};

// work items of the fill: one per (output column, half k-step) = 8 consecutive k of one Wcat row
__host__ __device__ constexpr int narrow_image_items(int ks) { return kNarrowFo * 2 * ks; }
__host__ __device__ constexpr int narrow_image_blocks(int ks) { return narrow_image_items(ks) / 256; }

// Block `blk` of narrow_image_blocks(ks) 256-thread workgroups.  Neighbouring threads take neighbouring pieces of one
// weight row (plain 4-byte reads, coalesced inside a segment); the three 16-byte records go where the forward block's
// lane (c, h) of column block o / 32 looks for them.
__device__ __forceinline__ void narrow_image_fill(const NarrowImageParams &p, int blk) {
    const int id = blk * 256 + (int)threadIdx.x;
    const int per = 2 * p.ks;
    const int o = id / per, kh = id - o * per;          // column of the output, half k-step
    if (o >= kNarrowFo) return;
    const int width = p.nseg * p.fi;
    float v[8];
    int s = (8 * kh) / p.fi, f = 8 * kh - s * p.fi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = 0.f;
        if (8 * kh + j < width) {
            // (the segment pointer picked without a runtime index into the kernel argument)
            const float *ws = p.w[0];
#pragma unroll
            for (int q = 1; q < kMaxSeg; ++q) ws = s == q ? p.w[q] : ws;
            v[j] = ws[o * p.fi + f];
        }
        if (++f == p.fi) f = 0, ++s;
    }
    bf16x8 pl[3];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __bf16 hi, mid, lo;
        split1(v[j], hi, mid, lo);
        pl[0][j] = hi, pl[1][j] = mid, pl[2][j] = lo;
    }
    const int ks = kh >> 1, h = kh & 1, lane = (o & 31) + 32 * h;
    char *dst = static_cast<char *>(p.img) + (size_t)ks * kNarrowImgStepBytes + ((o >> 5) * 64 + lane) * 16;
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x8 *>(dst + q * (8 * 64 * 16)) = pl[q];
}

// host side: the argument check both entries share
inline bool narrow_image_args_ok(const float *const *ws, int nseg, int64_t fi, int64_t wpad, const void *img) {
    if (!ws || !img || nseg < 1 || nseg > kMaxSeg || fi < 1 || fi > 32 || nseg * fi > wpad) return false;
    if (wpad != 96 && wpad != 112 && wpad != 128) return false;
    if ((uintptr_t)img & 15) return false;
    for (int s = 0; s < nseg; ++s)
        if (!ws[s] || ((uintptr_t)ws[s] & 3)) return false;
    return true;
}

inline NarrowImageParams narrow_image_params(const float *const *ws, int nseg, int64_t fi, int64_t wpad, void *img) {
    NarrowImageParams q{};
    for (int s = 0; s < nseg; ++s) q.w[s] = ws[s];
    q.nseg = nseg, q.fi = (int)fi, q.ks = (int)(wpad / 16), q.img = img;
    return q;
}

}  // namespace dc
