// dc_dense_bf16.hip -- the TAGConv dense block over bf16-STORED features (gfx950).
//
//   out[N,Fo] = act( A[N,K] . W[Fo,K]^T + bias )     A, W bf16 (K-contiguous), fp32 accumulate
//
// BASELINE.json configs[4] ("bf16 node/edge MLPs on MFMA"): A is the hop slab [x | A x | A^2 x | A^3 x]
// as dc_spmm_bf16 leaves it (K = (K_hops+1) * Fi), W the layer's lins[k].weight concatenated along K
// and rounded to bf16 once per call (dc_weights_to_bf16), out fp32 or bf16 (the next layer's slab).
// Plain bf16 operands on v_mfma_f32_32x32x16_bf16: one MFMA product per tile - the precision of the
// reference under torch.autocast(bfloat16), NOT the fp32-accurate split forms of dc_dense_split.hip.
//
// Structure: 128 x 128 block tile, 4 MFMA waves (2 x 2) + 4 LOADER waves, stage = 32 k (64 B per
// row).  BOTH operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no registers, no VALU,
// no ds_write), issued by the loader waves into a ring of kSlots stage buffers kAhead stages ahead
// and published with a COUNTED vmcnt + one s_barrier per stage (the pieces of the stages still in
// flight stay in flight across the barrier; barriers do not drain VMEM).  The DMA writes lane i's
// 16 bytes at base + 16 i, so a tile image is dense (64-byte rows); bank spread of the b128 fragment
// reads comes from an XOR swizzle of the four 16-byte pieces of a row (piece q of row r sits at
// position q ^ ((r >> 2) & 3)) applied on the GLOBAL side of the DMA.
#include "dc_dense.h"

namespace dc {

constexpr int kBfBK = 32;        // k per stage (bf16 elements): 64 bytes per row
constexpr int kBfSlots = 4;      // ring depth
constexpr int kBfAhead = 3;      // stages of DMA in flight behind the one being multiplied

struct Bf16Params {
    const uint16_t *a;     // [N, K] bf16, leading dimension lda (elements)
    const uint16_t *w;     // [Fo, K] bf16, leading dimension K
    const float *bias;     // [Fo] or null
    void *out;             // [N, Fo] fp32 or bf16, leading dimension ldo (elements)
    int64_t lda, ldo, N, K, Fo;
    int relu, out_bf16;
};

__global__ void __launch_bounds__(512)
k_fwd_bf16(Bf16Params p) {
    constexpr int BM = 128, kTile = BM * 64;                 // bytes of one operand tile of a stage
    __shared__ __attribute__((aligned(16))) char sA[kBfSlots][kTile];
    __shared__ __attribute__((aligned(16))) char sB[kBfSlots][kTile];

    const unsigned ntn = (unsigned)((p.Fo + BN - 1) / BN);
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    // column tiles of one row tile are neighbours in the logical order (same XCD, launched together):
    // the second read of the A rows is an L2 hit
    const int64_t row0 = (int64_t)(lb / ntn) * BM, col0 = (int64_t)(lb % ntn) * BN;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int nst = (int)(p.K / kBfBK);

    if (wid >= 4) {
        // ---------------- four loader waves: LDS-DMA only, never read LDS ----------------
        // (hipcc guards every ds_read of a wave that has LDS-DMAs in flight with s_waitcnt vmcnt(0) -
        // it cannot tell the slots apart - so the waves that issue the DMAs are not the ones that
        // read.  FOUR of them: one wave sustains only ~25 GB/s of LDS-DMA (MI355X_MICROARCH.md,
        // ldsdma-fill), a 128 x 128 x 32 bf16 stage needs 16 KiB per ~0.12 us of MFMA time; with a
        // single loader wave this kernel ran at 0.19 of the MFMA peak.)
        const int lw = wid - 4;                  // loader wave lw fills rows [32 lw, 32 lw + 32) of both tiles
        unsigned offA[2], offB[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int rowl = lw * 32 + q * 16 + (lane >> 2);
            const int piece = (lane & 3) ^ ((rowl >> 2) & 3);
            int64_t row = row0 + rowl;
            row = row < p.N ? row : p.N - 1;
            int64_t col = col0 + rowl;
            col = col < p.Fo ? col : p.Fo - 1;
            offA[q] = (unsigned)((row - row0) * p.lda + 8 * piece);       // elements
            offB[q] = (unsigned)((col - col0) * p.K + 8 * piece);
        }
        const uint16_t *baseA = p.a + row0 * p.lda;
        const uint16_t *baseB = p.w + col0 * p.K;
        auto dma = [&](int slot) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                __builtin_amdgcn_global_load_lds(DC_DMA_SRC(baseA + offA[q]),
                                                 DC_DMA_DST(sA[slot] + (lw * 32 + q * 16) * 64), 16, 0, 0);
                __builtin_amdgcn_global_load_lds(DC_DMA_SRC(baseB + offB[q]),
                                                 DC_DMA_DST(sB[slot] + (lw * 32 + q * 16) * 64), 16, 0, 0);
            }
            baseA += kBfBK;
            baseB += kBfBK;
        };
        for (int s = 0; s < kBfAhead && s < nst; ++s) dma(s);
        for (int it = 0; it < nst; ++it) {
            // wait until only the stages AFTER `it` (4 DMA instructions per wave and stage; up to two of
            // them pending here) are still in flight; the barrier publishes stage `it` and tells the
            // loaders that the MFMA waves are done with stage it - 1, whose slot then takes stage it + 3
            const int later = nst - 1 - it;
            if (later >= 2) DC_WAITVM(8);
            else if (later == 1) DC_WAITVM(4);
            else DC_WAITVM(0);
            __builtin_amdgcn_s_barrier();
            if (it + kBfAhead < nst) dma((it + kBfAhead) & (kBfSlots - 1));
        }
        return;
    }

    // ---------------- four MFMA waves (2 x 2), 64 x 64 of the tile each ----------------
    const int wm = wid >> 1, wn = wid & 1;
    // fragment positions: lane (fr = lane & 31, fh = lane >> 5) of k-step t reads the 8 bf16
    // k = 16 t + 8 fh .. +7 of its row = piece 2 t + fh, stored at (2 t + fh) ^ ((row >> 2) & 3)
    const int fr = lane & 31, fh = lane >> 5;
    int fragA[2][2], fragB[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ra = wm * 64 + b * 32 + fr, rb = wn * 64 + b * 32 + fr;
            fragA[b][t] = ra * 64 + 16 * ((2 * t + fh) ^ ((ra >> 2) & 3));
            fragB[b][t] = rb * 64 + 16 * ((2 * t + fh) ^ ((rb >> 2) & 3));
        }

    f32x16 acc[2][2];
    zero_acc<2>(acc);
    for (int it = 0; it < nst; ++it) {
        __builtin_amdgcn_s_barrier();
        const char *ca = sA[it & (kBfSlots - 1)], *cb = sB[it & (kBfSlots - 1)];
        bf16x8 fa[2][2], fb[2][2];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[b][t] = *reinterpret_cast<const bf16x8 *>(ca + fragA[b][t]);
                fb[b][t] = *reinterpret_cast<const bf16x8 *>(cb + fragB[b][t]);
            }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mb][t], fb[nb][t], acc[mb][nb], 0, 0, 0);
    }

    const bool relu = p.relu != 0;
    float bcol[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int64_t col = col0 + wn * 64 + nb * 32 + (threadIdx.x & 31);
        bcol[nb] = (p.bias && col < p.Fo) ? p.bias[col] : 0.f;
    }
    for_each_acc<2>(acc, wm, wn, [&](int rr, int c, float v) {
        const int64_t row = row0 + rr, col = col0 + c;
        if (row < p.N && col < p.Fo) {
            v += bcol[(c >> 5) & 1];
            if (relu) v = relu_keep_nan(v);
            if (p.out_bf16) ((uint16_t *)p.out)[row * p.ldo + col] = f32_to_bf16_rne(v);
            else ((float *)p.out)[row * p.ldo + col] = v;
        }
    });
}


// ---- 256 x 256 tiles, all operands by LDS-DMA in a four-stage ring, one raw barrier per stage (r03) ----------------
// The bf16 block of configs[4] is HBM-bound, not MFMA-bound: [100k, 1024] bf16 activations are read ONCE (205 MB)
// for 52 GFLOP - 204 FLOP per byte against a machine balance of 312 - so the floor is ~45 us (the 0.41 "of the MFMA
// peak" that 256 MB at the ~6 TB/s streaming rate allows), and what decides the time is how many bytes each CU keeps in
// flight (MI355X_MICROARCH.md: ~24 GB/s per CU with 72 KiB outstanding).  k_fwd_bf16 above (128 x 128 tiles, loader /
// consumer waves) and a two-buffer version of this kernel with one __syncthreads() per 64-deep K tile both ran at
// 111 us: one K tile of prefetch covers ~1 us of MFMA work against 2 - 4 us of loaded HBM latency.
// Here: a 512-thread workgroup owns 256 rows x 256 columns (A is read once, the 512 KB of weights come from L2), 8
// waves as 2 x 4 with 128 x 64 per wave (eight 32 x 32 accumulator blocks), BK = 32, BOTH operands global -> LDS by
// LDS-DMA into a ring of four 32 KB stages, THREE stages (48 KB of A per CU) in flight behind the one being multiplied,
// retired with a counted vmcnt and ONE raw s_barrier per stage (barriers do not drain VMEM; all LDS is one array, so
// hipcc does not guard the fragment reads against the DMAs still in flight).  The XOR swizzle of the four 16-byte
// pieces of a row is applied to the per-lane SOURCE address; the LDS image is lane-linear.  Same products in the same
// order as k_fwd_bf16: bit-identical results.
constexpr int kGxBM = 256, kGxBN = 256, kGxBK = 32;
constexpr int kGxRow = kGxBK * 2;                          // 64 bytes per LDS row
constexpr int kGxTile = kGxBM * kGxRow;                    // 16 KB per operand and stage
constexpr int kGxSlots = 4, kGxAhead = 3;

template <bool OUT_BF16>
__global__ void __launch_bounds__(512)
k_fwd_bf16x(Bf16Params p) {
    // [slot][operand]: 128 KB of ring; the epilogue's output image needs 256 x 528 B (bf16) / 128 x 1040 B (fp32): ONE array
    __shared__ __attribute__((aligned(16))) char lds[kGxBM * (kGxBN * 2 + 16)];
    const unsigned ntn = (unsigned)((p.Fo + kGxBN - 1) / kGxBN);
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t row0 = (int64_t)(lb / ntn) * kGxBM, col0 = (int64_t)(lb % ntn) * kGxBN;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int wm = wid >> 2, wn = wid & 3;
    const int nst = (int)(p.K / kGxBK);

    // staging: wave-instruction j (of 2) of wave w fills rows 16 (2 w + j) .. + 15 of a tile (1 KiB, lane-linear):
    // lane l is row 16 c + (l >> 2), position l & 3, and fetches the piece that belongs there: q = position ^ ((row >> 2) & 3)
    unsigned offA[2], offB[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int rl = 16 * (2 * wid + j) + (lane >> 2);
        const int q = (lane & 3) ^ ((rl >> 2) & 3);
        int64_t row = row0 + rl, col = col0 + rl;
        row = row < p.N ? row : p.N - 1;
        col = col < p.Fo ? col : p.Fo - 1;
        offA[j] = (unsigned)((row - row0) * p.lda + 8 * q);                 // elements
        offB[j] = (unsigned)((col - col0) * p.K + 8 * q);
    }
    const uint16_t *baseA = p.a + row0 * p.lda;
    const uint16_t *baseB = p.w + col0 * p.K;
    auto stage = [&](int slot) {                                            // 4 DMA instructions per wave and stage
        char *ta = lds + (2 * slot) * kGxTile, *tb = ta + kGxTile;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            __builtin_amdgcn_global_load_lds(DC_DMA_SRC(baseA + offA[j]), DC_DMA_DST(ta + (2 * wid + j) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(DC_DMA_SRC(baseB + offB[j]), DC_DMA_DST(tb + (2 * wid + j) * 1024), 16, 0, 0);
        }
        baseA += kGxBK;
        baseB += kGxBK;
    };
    // fragments: lane (fr = lane & 31, fh = lane >> 5) of k-step t reads k = 16 t + 8 fh .. + 7 of its row = piece 2 t + fh
    const int fr = lane & 31, fh = lane >> 5;
    int fragA[2], fragB[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        // rows wm * 128 + mb * 32 + fr and wn * 64 + nb * 32 + fr: (row >> 2) & 3 == (fr >> 2) & 3
        fragA[t] = (wm * 128 + fr) * kGxRow + 16 * ((2 * t + fh) ^ ((fr >> 2) & 3));
        fragB[t] = (wn * 64 + fr) * kGxRow + 16 * ((2 * t + fh) ^ ((fr >> 2) & 3));
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;

    // (vmcnt retires in order, so the L2-resident weights cannot ride a shallower ring than the activations: a weight
    // tile issued one stage ahead would sit BEHIND the activation tiles issued before it and waiting for it would
    // drain them - both operands share the ring depth)
    for (int s = 0; s < kGxAhead && s < nst; ++s) stage(s);
    for (int it = 0; it < nst; ++it) {
        // stage `it` has landed once only the DMA instructions of the LATER stages (4 per wave each, at most two of
        // them issued so far) are outstanding; the barrier publishes every wave's pieces and says that everybody is
        // done with stage it - 1, whose slot then takes stage it + 3
        const int later = nst - 1 - it;
        if (later >= 2) DC_WAITVM(8);
        else if (later == 1) DC_WAITVM(4);
        else DC_WAITVM(0);
        __builtin_amdgcn_s_barrier();
        if (it + kGxAhead < nst) stage((it + kGxAhead) & (kGxSlots - 1));
        const char *ta = lds + (2 * (it & (kGxSlots - 1))) * kGxTile, *tb = ta + kGxTile;
        bf16x8 fa[2][4], fb[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) fb[t][nb] = *reinterpret_cast<const bf16x8 *>(tb + fragB[t] + nb * 32 * kGxRow);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) fa[t][mb] = *reinterpret_cast<const bf16x8 *>(ta + fragA[t] + mb * 32 * kGxRow);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t][mb], fb[t][nb], acc[mb][nb], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    }

    // epilogue.  The C/D fragment is column-per-lane ((reg, lane) -> row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col
    // lane & 31): stored as it stands, a wave-instruction writes two 64-byte pieces (bf16) - 128 such instructions per
    // wave, 42 of the kernel's 129 us (r03 ablation).  The tile goes through LDS instead (the ring is free now) and leaves
    // as full rows, 16 bytes per lane: bf16 in one pass (256 rows x 512 B), fp32 in two (128 rows x 1 KiB each).
    const bool relu = p.relu != 0;
    const int c = lane & 31, h = lane >> 5;
    constexpr int esz = OUT_BF16 ? 2 : 4;
    constexpr int rs = kGxBN * esz + 16;                      // LDS row stride: + 16 B keeps the two half-waves on
    constexpr int npass = OUT_BF16 ? 1 : 2;                   // disjoint banks
    const bool vec_ok = ((p.ldo * esz) % 16 == 0) && (((uintptr_t)p.out) % 16 == 0);
    __syncthreads();
    for (int pass = 0; pass < npass; ++pass) {
        if (npass == 1 || wm == pass) {
            const int rbase = npass == 1 ? wm * 128 : 0;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int64_t col = col0 + wn * 64 + nb * 32 + c;
                const float bcol = (p.bias && col < p.Fo) ? p.bias[col] : 0.f;
                char *dst = lds + (wn * 64 + nb * 32 + c) * esz;
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int rl = rbase + mb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                        float v = acc[mb][nb][reg] + bcol;
                        if (relu) v = relu_keep_nan(v);
                        if (OUT_BF16) *reinterpret_cast<uint16_t *>(dst + rl * rs) = f32_to_bf16_rne(v);
                        else *reinterpret_cast<float *>(dst + rl * rs) = v;
                    }
            }
        }
        __syncthreads();
        constexpr int rows_here = npass == 1 ? kGxBM : kGxBM / 2;
        constexpr int tpr = kGxBN * esz / 16;                  // threads per row (16 B each): 32 (bf16) / 64 (fp32)
        constexpr int rpp = 512 / tpr;                        // rows per sweep
        const int tr = threadIdx.x / tpr, tc = threadIdx.x % tpr;
        constexpr int epl = 16 / esz;                         // elements per lane
        for (int r = tr; r < rows_here; r += rpp) {
            const int64_t row = row0 + (npass == 1 ? 0 : pass * 128) + r;
            const int64_t col = col0 + (int64_t)tc * epl;
            if (row >= p.N || col >= p.Fo) continue;
            const uint4 q = *reinterpret_cast<const uint4 *>(lds + r * rs + tc * 16);
            char *o = (char *)p.out + (row * p.ldo + col) * esz;
            if (vec_ok && col + epl <= p.Fo) {
                *reinterpret_cast<uint4 *>(o) = q;
            } else {                                          // ragged right edge / unaligned output: element by element
                const char *src = reinterpret_cast<const char *>(&q);
                for (int e = 0; e < epl && col + e < p.Fo; ++e)
                    for (int bb = 0; bb < esz; ++bb) o[e * esz + bb] = src[e * esz + bb];
            }
        }
        if (pass + 1 < npass) __syncthreads();
    }
}

// fp32 [rows, cols] (ld) -> bf16 (round to nearest even), optionally K-concatenating nseg matrices:
// dst[r, s * cols + c] = bf16(src[s][r, c])
__global__ void __launch_bounds__(256)
k_to_bf16(const float *const *src, int nseg, int64_t rows, int64_t cols, int64_t ld_src,
          uint16_t *dst, int64_t ld_dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = rows * cols;
    if (i >= per * nseg) return;
    const int s = (int)(i / per);
    const int64_t r = (i % per) / cols, c = (i % per) % cols;
    dst[r * ld_dst + s * cols + c] = f32_to_bf16_rne(src[s][r * ld_src + c]);
}

struct PtrPack { const float *p[kMaxSeg]; };

__global__ void __launch_bounds__(256)
k_to_bf16_pack(PtrPack src, int nseg, int64_t rows, int64_t cols, int64_t ld_src, uint16_t *dst,
               int64_t ld_dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = rows * cols;
    if (i >= per * nseg) return;
    const int s = (int)(i / per);
    const int64_t r = (i % per) / cols, c = (i % per) % cols;
    dst[r * ld_dst + s * cols + c] = f32_to_bf16_rne(src.p[s][r * ld_src + c]);
}


// ---- backward of the bf16-storage layer (BASELINE.json configs[4]: fwd + bwd) ---------------------------------------
// gm = g * (out > 0) in bf16 (block 0 of the gradient slab; the transposed bf16 hops and the forward-shaped dX block -
// k_fwd_bf16 over that slab with the transposed weights - follow), and dW: both operands node-major.
struct MaskBf16Params {
    const void *g, *mask;
    uint16_t *gm;
    int64_t ldg, ldm, ldgm, N;
    int F, g_bf16, mask_bf16;
};
__device__ __forceinline__ float ld_elem(const void *p, int64_t i, int is_bf16) {
    return is_bf16 ? __uint_as_float((uint32_t)((const uint16_t *)p)[i] << 16) : ((const float *)p)[i];
}
__global__ void __launch_bounds__(256)
k_mask_grad_bf16(MaskBf16Params p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = i / p.F;
    const int c = (int)(i % p.F);
    if (row >= p.N) return;
    float v = ld_elem(p.g, row * p.ldg + c, p.g_bf16);
    if (p.mask && !(ld_elem(p.mask, row * p.ldm + c, p.mask_bf16) > 0.f)) v = 0.f;
    p.gm[row * p.ldgm + c] = f32_to_bf16_rne(v);
}

// The same with 8 columns per thread and 16-byte accesses (F, the leading dimensions and the pointers allow it whenever
// the operands are the layer's own buffers): the scalar form above - a 64-bit division per element, 2-byte stores -
// took 83 us for [100k, 256] (2.5 TB/s).  Same values: the rounding is per element.
template <bool G_BF16, bool M_BF16>
__global__ void __launch_bounds__(256)
k_mask_grad_bf16x8(MaskBf16Params p) {
    const int per_row = p.F >> 3;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = i / per_row;
    const int c = (int)(i - row * per_row) << 3;
    if (row >= p.N) return;
    float v[8], m[8];
    auto ld8 = [&](const void *base, int64_t off, bool bf, float (&o)[8]) {
        if (bf) {
            const uint4 u = *reinterpret_cast<const uint4 *>((const uint16_t *)base + off);
            const uint32_t d[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) o[2 * j] = __uint_as_float(d[j] << 16), o[2 * j + 1] = __uint_as_float(d[j] & 0xffff0000u);
        } else {
            const float4 a = *reinterpret_cast<const float4 *>((const float *)base + off);
            const float4 b = *reinterpret_cast<const float4 *>((const float *)base + off + 4);
            o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
        }
    };
    ld8(p.g, row * p.ldg + c, G_BF16, v);
    if (p.mask) {
        ld8(p.mask, row * p.ldm + c, M_BF16, m);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (!(m[j] > 0.f)) v[j] = 0.f;
    }
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (uint32_t)f32_to_bf16_rne(v[2 * j]) | ((uint32_t)f32_to_bf16_rne(v[2 * j + 1]) << 16);
    *reinterpret_cast<uint4 *>(p.gm + row * p.ldgm + c) = make_uint4(o[0], o[1], o[2], o[3]);
}

// dW[o, f] of segment s = sum over nodes n of gm[n, o] * x_s[n, f], fp32 accumulate, per node chunk (partials summed in
// chunk order by the slab reduce: deterministic).  Shape of k_dw_h2w (dc_dense_split.hip) with plain bf16 operands: a
// 512-thread workgroup owns a 128 (o) x 256 (f) tile of one segment over one node chunk, a stage is 32 nodes, the [k][m]
// LDS images (rows padded by 64 B) are read with gfx950's transposing ds_read_b64_tr_b16, one bf16 MFMA product.
constexpr int kDwbK = 32;
constexpr int kDwbRowA = 128 * 2 + 64, kDwbRowB = 256 * 2 + 64;        // bytes per node row of the g / x image
constexpr int kDwbStage = kDwbK * (kDwbRowA + kDwbRowB);                // 28,672 B

__global__ void __launch_bounds__(512)
k_dw_bf16(DwBf16Params p) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kDwbStage];
    const unsigned nto = (unsigned)(p.Fo / 128), nfb = (unsigned)(p.Fi / 256);
    const unsigned per_chunk = nto * nfb * (unsigned)p.nseg;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned chunk = lb / per_chunk, rem = lb % per_chunk;
    const int s = (int)(rem / (nto * nfb));
    const int64_t o0 = (int64_t)((rem / nfb) % nto) * 128, f0 = (int64_t)(rem % nfb) * 256;
    const int64_t n_beg = (int64_t)chunk * p.chunk_rows;
    const int64_t n_end = (n_beg + p.chunk_rows < p.N) ? n_beg + p.chunk_rows : p.N;
    const int wid = threadIdx.x >> 6, wm = wid >> 2, wn = wid & 3;
    const bool do_bias = p.bias_partial && s == 0 && f0 == 0;

    // staging: g tile 32 x 128 bf16 (16 threads x 16 B per node row), x tile 32 x 256 bf16 (32 threads per row, 2 passes)
    const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int cx = threadIdx.x & 31, rx = threadIdx.x >> 5;
    const uint16_t *pg = p.g + (n_beg + rg) * p.ldg + o0 + 8 * cg;
    const uint16_t *px = p.x + (n_beg + rx) * p.ldx + (int64_t)s * p.Fi + f0 + 8 * cx;
    const int ldsg = rg * kDwbRowA + 16 * cg;
    const int ldsx = kDwbK * kDwbRowA + rx * kDwbRowB + 16 * cx;
    uint4 vg0, vg1, vx0[2], vx1[2];
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t n_next = n_beg;                                    // first node of the stage the next gload fetches
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    auto gload = [&](uint4 &vg, uint4 (&vx)[2]) {             // rows past the chunk's end read as zeros
        vg = n_next + rg < n_end ? *reinterpret_cast<const uint4 *>(pg) : zero4;
        vx[0] = n_next + rx < n_end ? *reinterpret_cast<const uint4 *>(px) : zero4;
        vx[1] = n_next + rx + 16 < n_end ? *reinterpret_cast<const uint4 *>(px + 16 * p.ldx) : zero4;
        pg += kDwbK * p.ldg;
        px += kDwbK * p.ldx;
        n_next += kDwbK;
    };
    auto lstore = [&](const uint4 &vg, const uint4 (&vx)[2], int b) {
        char *buf = lds + b * kDwbStage;
        *reinterpret_cast<uint4 *>(buf + ldsg) = vg;
        *reinterpret_cast<uint4 *>(buf + ldsx) = vx[0];
        *reinterpret_cast<uint4 *>(buf + ldsx + 16 * kDwbRowB) = vx[1];
        if (do_bias) {
            const uint32_t d[4] = {vg.x, vg.y, vg.z, vg.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bsum[2 * i] += __uint_as_float(d[i] << 16);
                bsum[2 * i + 1] += __uint_as_float(d[i] & 0xffff0000u);
            }
        }
    };
    f32x16 acc[2][2];
    zero_acc<2>(acc);
    auto compute = [&](int b) {
        const char *buf = lds + b * kDwbStage;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) fa[mb] = tr_operand<kDwbRowA>(buf + ks * 16 * kDwbRowA, wm * 64 + mb * 32);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                fb[nb] = tr_operand<kDwbRowB>(buf + kDwbK * kDwbRowA + ks * 16 * kDwbRowB, wn * 64 + nb * 32);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mb], fb[nb], acc[mb][nb], 0, 0, 0);
        }
    };

    const int nst = (int)((n_end - n_beg + kDwbK - 1) / kDwbK);
    if (nst > 0) {
        gload(vg0, vx0);
        if (nst > 1) gload(vg1, vx1);
        lstore(vg0, vx0, 0);
    }
    __syncthreads();
    int it = 0;
#define DC_DWB_STAGE(CUR, VG_L, VX_L, VG_S, VX_S)                                                     \
    gload(VG_L, VX_L);                                 /* stage it+2 */                               \
    __builtin_amdgcn_sched_barrier(0);                                                                \
    compute(CUR);                                                                                     \
    lstore(VG_S, VX_S, CUR ^ 1);                       /* stage it+1 */                               \
    __syncthreads();
    for (; it + 3 < nst; it += 2) {
        DC_DWB_STAGE(0, vg0, vx0, vg1, vx1)
        DC_DWB_STAGE(1, vg1, vx1, vg0, vx0)
    }
#undef DC_DWB_STAGE
#define DC_DWB_TAIL(K, CUR, VG_L, VX_L, VG_S, VX_S)                                                   \
    if (it + K < nst) {                                                                               \
        if (it + K + 2 < nst) gload(VG_L, VX_L);                                                      \
        compute(CUR);                                                                                 \
        if (it + K + 1 < nst) lstore(VG_S, VX_S, CUR ^ 1);                                            \
        __syncthreads();                                                                              \
    }
    for (; it < nst; it += 2) {
        DC_DWB_TAIL(0, 0, vg0, vx0, vg1, vx1)
        DC_DWB_TAIL(1, 1, vg1, vx1, vg0, vx0)
    }
#undef DC_DWB_TAIL

    float *out = p.partial + ((int64_t)chunk * p.nseg + s) * p.Fo * p.Fi;
    for_each_acc<2>(acc, wm, wn, [&](int r, int c, float v) { out[(o0 + r) * p.Fi + f0 + c] = v; });
    if (do_bias) {                                      // column sums of gm over the chunk's nodes
        float *red = reinterpret_cast<float *>(lds);    // [32 node rows][128 o]
#pragma unroll
        for (int i = 0; i < 8; ++i) red[rg * 128 + 8 * cg + i] = bsum[i];
        __syncthreads();
        if (threadIdx.x < 128) {
            float t = 0.f;
            for (int r = 0; r < 32; ++r) t += red[r * 128 + threadIdx.x];
            p.bias_partial[(int64_t)chunk * p.Fo + o0 + threadIdx.x] = t;
        }
    }
}

// ---- the same block with both operands by LDS-DMA (r04) --------------------------------------------------------------
// k_dw_bf16 above moves every stage through registers, two stages deep, one __syncthreads() per 32 nodes: on the
// 100k-point graph of configs[4] (98 stages per workgroup) a launch took 212 us - 2.1 us per stage, the loaded HBM
// latency of one register-staged prefetch, 0.10 of the MFMA peak and 1.2 TB/s of compulsory bytes.  Here the eight MFMA
// waves only read LDS and multiply; four loading waves (LDS-DMA: no registers, no VALU, no ds_write) keep FIVE stages
// of 24 KiB in flight per CU in a ring of six, retired with a counted vmcnt and one raw s_barrier per stage (the
// protocol of k_fwd_bf16).  The DMA writes lane-linear 1 KiB pieces, so a stage image is dense ([node][o] 256 B rows,
// [node][f] 512 B rows) and the bank spread the padded rows gave the transposing reads comes from an XOR of the 64-byte
// column chunk with node & 3, applied to the per-lane SOURCE offset.  Rows past the chunk's end fall out of the buffer
// resource's range and arrive as zeros.  Same products in the same order, the bias sums taken from the LDS image with
// the thread -> (row, columns) map of k_dw_bf16: bit-identical partials.
constexpr int kDwdSlots = 6, kDwdAhead = 5;
constexpr int kDwdRowA = 128 * 2, kDwdRowB = 256 * 2;                    // dense node rows of the g / x image
constexpr int kDwdStage = kDwbK * (kDwdRowA + kDwdRowB);                 // 24,576 B

template <int ROWB>
__device__ __forceinline__ bf16x8 dwd_tr_operand(const char *plane, int m0) {
    const int lane = threadIdx.x & 63, g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int h = g >> 1;
    // node rows 8 h + q and + 4 (both have node & 3 = q), column chunk m0 / 32 stored at chunk ^ q
    return tr_read<ROWB>(plane + (8 * h + q) * ROWB + (((m0 >> 5) ^ q) << 6) + 32 * (g & 1) + 8 * pp);
}

__global__ void __launch_bounds__(768)
k_dw_bf16d(DwBf16Params p) {
    __shared__ __attribute__((aligned(16))) char lds[kDwdSlots * kDwdStage];
    const unsigned nto = (unsigned)(p.Fo / 128), nfb = (unsigned)(p.Fi / 256);
    const unsigned per_chunk = nto * nfb * (unsigned)p.nseg;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned chunk = lb / per_chunk, rem = lb % per_chunk;
    const int s = (int)(rem / (nto * nfb));
    const int64_t o0 = (int64_t)((rem / nfb) % nto) * 128, f0 = (int64_t)(rem % nfb) * 256;
    const int64_t n_beg = (int64_t)chunk * p.chunk_rows;
    const int64_t n_end = (n_beg + p.chunk_rows < p.N) ? n_beg + p.chunk_rows : p.N;
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const bool do_bias = p.bias_partial && s == 0 && f0 == 0;
    const int nst = (int)((n_end - n_beg + kDwbK - 1) / kDwbK);
    const int64_t rows = n_end - n_beg;

    if (wid >= 8) {
        // ------------------------------------------------------------------ loading waves: LDS-DMA only
        // g plane: 8 instructions per stage (4 node rows x 256 B each; lane l = row l >> 4, piece l & 15), x plane: 16
        // (2 node rows x 512 B; lane l = row l >> 5, piece l & 31); piece i = chunk i >> 2, part i & 3 of its row
        // fetches source chunk (i >> 2) ^ (node & 3).  Wave w issues g instructions 2 w, 2 w + 1 and x instructions
        // 4 w .. 4 w + 3 of every stage: 6 per wave and stage.
        const int w = wid - 8;
        if (rows > 0) {
            const __amdgpu_buffer_rsrc_t rg_ = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint16_t *>(p.g + n_beg * p.ldg + o0), 0, (int)(((rows - 1) * p.ldg + 128) * 2), 0x00020000);
            const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint16_t *>(p.x + n_beg * p.ldx + (int64_t)s * p.Fi + f0), 0,
                (int)(((rows - 1) * p.ldx + 256) * 2), 0x00020000);
            const int rgl = lane >> 4, ig = lane & 15;
            const int voffg = (int)((int64_t)rgl * p.ldg * 2) + ((((ig >> 2) ^ rgl) << 6) | ((ig & 3) << 4));
            const int rxl = lane >> 5, ix = lane & 31;
            int voffx[2];
#pragma unroll
            for (int e = 0; e < 2; ++e)
                voffx[e] = (int)((int64_t)rxl * p.ldx * 2) + ((((ix >> 2) ^ (2 * e + rxl)) << 6) | ((ix & 3) << 4));
            const int gstep = (int)(4 * p.ldg * 2), xstep = (int)(2 * p.ldx * 2);       // bytes per instruction's rows
            const int gstage = (int)(kDwbK * p.ldg * 2), xstage = (int)(kDwbK * p.ldx * 2);
            auto stage = [&](int st) {
                char *dst = lds + (st % kDwdSlots) * kDwdStage;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int c = 2 * w + j;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rg_, DC_DMA_DST(dst + c * 1024), 16, voffg,
                                                             c * gstep + st * gstage, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = 4 * w + j;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx_, DC_DMA_DST(dst + kDwbK * kDwdRowA + c * 1024), 16, voffx[j & 1],
                                                             c * xstep + st * xstage, 0, 0);
                }
            };
#pragma unroll
            for (int st = 0; st < kDwdAhead; ++st)
                if (st < nst) stage(st);
            for (int it = 0; it < nst; ++it) {
                // all but the stages after `it` (at most kDwdAhead - 1 of them, 6 instructions each) have landed
                const int later = nst - 1 - it;
                if (later >= 4) DC_WAITVM(24);
                else if (later == 3) DC_WAITVM(18);
                else if (later == 2) DC_WAITVM(12);
                else if (later == 1) DC_WAITVM(6);
                else DC_WAITVM(0);
                __builtin_amdgcn_s_barrier();            // publishes stage it; the MFMA waves have left stage it - 1
                if (it + kDwdAhead < nst) stage(it + kDwdAhead);
            }
        }
        if (do_bias) {
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_barrier();
        }
        return;
    }

    // ------------------------------------------------------------------ eight MFMA waves (2 x 4), 64 (o) x 64 (f) each
    const int wm = wid >> 2, wn = wid & 3;
    const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;                  // bias sums: k_dw_bf16's staging map
    const int bias_off = rg * kDwdRowA + ((((cg >> 2) ^ (rg & 3)) << 6) | ((cg & 3) << 4));
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc[2][2];
    zero_acc<2>(acc);
    for (int it = 0; it < nst; ++it) {
        __builtin_amdgcn_s_barrier();
        const char *buf = lds + (it % kDwdSlots) * kDwdStage;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) fa[mb] = dwd_tr_operand<kDwdRowA>(buf + ks * 16 * kDwdRowA, wm * 64 + mb * 32);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                fb[nb] = dwd_tr_operand<kDwdRowB>(buf + kDwbK * kDwdRowA + ks * 16 * kDwdRowB, wn * 64 + nb * 32);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mb], fb[nb], acc[mb][nb], 0, 0, 0);
        }
        if (do_bias) {
            const uint4 vg = *reinterpret_cast<const uint4 *>(buf + bias_off);
            const uint32_t d[4] = {vg.x, vg.y, vg.z, vg.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bsum[2 * i] += __uint_as_float(d[i] << 16);
                bsum[2 * i + 1] += __uint_as_float(d[i] & 0xffff0000u);
            }
        }
    }

    float *out = p.partial + ((int64_t)chunk * p.nseg + s) * p.Fo * p.Fi;
    for_each_acc<2>(acc, wm, wn, [&](int r, int c, float v) { out[(o0 + r) * p.Fi + f0 + c] = v; });
    if (do_bias) {                                      // column sums of gm over the chunk's nodes
        __builtin_amdgcn_s_barrier();                   // every wave has left the ring
        float *red = reinterpret_cast<float *>(lds);    // [32 node rows][128 o]
#pragma unroll
        for (int i = 0; i < 8; ++i) red[rg * 128 + 8 * cg + i] = bsum[i];
        __builtin_amdgcn_s_waitcnt(0xC07F);             // lgkmcnt(0): the stores have reached LDS
        __builtin_amdgcn_s_barrier();
        if (threadIdx.x < 128) {
            float t = 0.f;
            for (int r = 0; r < 32; ++r) t += red[r * 128 + threadIdx.x];
            p.bias_partial[(int64_t)chunk * p.Fo + o0 + threadIdx.x] = t;
        }
    }
}

bool dw_bf16_launch(const DwBf16Params &p, hipStream_t hs) {
    if (p.Fo % 128 != 0 || p.Fi % 256 != 0 || p.chunk_rows % kDwbK != 0) return false;
    if (p.ldg % 8 != 0 || p.ldx % 8 != 0 || ((uintptr_t)p.g & 15) || ((uintptr_t)p.x & 15)) return false;
    const int64_t grid = (p.Fo / 128) * (p.Fi / 256) * p.nseg * p.nchunks;
    if (grid >= (int64_t)INT32_MAX) return false;
    // both operands by LDS-DMA when a chunk's byte offsets fit the buffer instructions' 32 bits (DC_DW_BF16_DMA=0: the
    // register-staged kernel; bit-identical partials)
    const bool dma = env_int("DC_DW_BF16_DMA", 1) != 0;          // (per call: tests flip it inside one process)
    const int64_t span = (p.chunk_rows + kDwbK) * (p.ldg > p.ldx ? p.ldg : p.ldx) * 2;
    if (dma && span < ((int64_t)1 << 31)) {
        DC_LAUNCH(k_dw_bf16d, dim3((unsigned)grid), dim3(768), 0, hs, p);
        return true;
    }
    DC_LAUNCH(k_dw_bf16, dim3((unsigned)grid), dim3(512), 0, hs, p);
    return true;
}

}  // namespace dc

using namespace dc;

extern "C" int dc_tag_linear_fwd_bf16(const uint16_t *a, int64_t lda, const uint16_t *w,
                                      const float *bias, int relu, void *out, int64_t ldo,
                                      int out_is_bf16, int64_t N, int64_t K, int64_t Fo,
                                      dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(N >= 0 && K >= 0 && Fo >= 0, "dc_tag_linear_fwd_bf16: negative size");
    if (N == 0 || Fo == 0) return DC_OK;
    DC_REQUIRE(a && w && out, "dc_tag_linear_fwd_bf16: null a/w/out");
    DC_REQUIRE(K >= kBfBK && K % kBfBK == 0, "dc_tag_linear_fwd_bf16: K=%lld must be a positive multiple of %d",
               (long long)K, kBfBK);
    DC_REQUIRE(lda >= K && lda % 8 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)w & 15) == 0,
               "dc_tag_linear_fwd_bf16: a / w must be 16-byte aligned with lda %% 8 == 0");
    DC_REQUIRE(ldo >= Fo, "dc_tag_linear_fwd_bf16: ldo < Fo");
    DC_REQUIRE(lda * 128 < ((int64_t)1 << 31) && K * 128 < ((int64_t)1 << 31),
               "dc_tag_linear_fwd_bf16: leading dimension too large for 32-bit tile offsets");
    Bf16Params p{a, w, bias, out, lda, ldo, N, K, Fo, relu, out_is_bf16};
    // 256 x 256 tiles (one per CU) once a launch has enough of them to fill most of the chip and K is whole 64-deep
    // tiles; else the 128 x 128 kernel (results are bit-identical).
    const int64_t xtiles = ((N + kGxBM - 1) / kGxBM) * ((Fo + kGxBN - 1) / kGxBN);
    const bool xok = K % kGxBK == 0 && lda * kGxBM < ((int64_t)1 << 31) && K * kGxBN < ((int64_t)1 << 31);
    if (xok && xtiles >= 160) {
        if (out_is_bf16) DC_LAUNCH(k_fwd_bf16x<true>, dim3((unsigned)xtiles), dim3(512), 0, stream, p);
        else DC_LAUNCH(k_fwd_bf16x<false>, dim3((unsigned)xtiles), dim3(512), 0, stream, p);
        return check_launch("dc_tag_linear_fwd_bf16");
    }
    const int64_t grid = ((N + 127) / 128) * ((Fo + BN - 1) / BN);
    DC_LAUNCH(k_fwd_bf16, dim3((unsigned)grid), dim3(512), 0, stream, p);
    return check_launch("dc_tag_linear_fwd_bf16");
}

extern "C" int dc_to_bf16(const float *const *srcs, int nseg, int64_t rows, int64_t cols,
                          int64_t ld_src, uint16_t *dst, int64_t ld_dst, dc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    DC_REQUIRE(nseg >= 1 && nseg <= kMaxSeg, "dc_to_bf16: nseg=%d out of range", nseg);
    DC_REQUIRE(rows >= 0 && cols >= 0, "dc_to_bf16: negative size");
    if (rows == 0 || cols == 0) return DC_OK;
    DC_REQUIRE(srcs && dst && ld_src >= cols && ld_dst >= cols * nseg, "dc_to_bf16: bad pointers / leading dimensions");
    PtrPack pk{};
    for (int s = 0; s < nseg; ++s) {
        DC_REQUIRE(srcs[s], "dc_to_bf16: null source %d", s);
        pk.p[s] = srcs[s];
    }
    const int64_t total = rows * cols * nseg;
    DC_LAUNCH(k_to_bf16_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, pk,
                       nseg, rows, cols, ld_src, dst, ld_dst);
    return check_launch("dc_to_bf16");
}

extern "C" int dc_tag_mask_grad_bf16(const void *g, int64_t ldg, int g_is_bf16, const void *out_for_mask,
                                     int64_t ldo, int mask_is_bf16, uint16_t *gm, int64_t ldgm, int64_t N,
                                     int64_t F, dc_stream_t stream) {
    DC_REQUIRE(N >= 0 && F >= 1 && F < (1 << 24) && ldg >= F && ldgm >= F && (!out_for_mask || ldo >= F),
               "dc_tag_mask_grad_bf16: bad sizes");
    if (N == 0) return DC_OK;
    DC_REQUIRE(g && gm, "dc_tag_mask_grad_bf16: null pointer");
    MaskBf16Params p{g, out_for_mask, gm, ldg, ldo, ldgm, N, (int)F, g_is_bf16, mask_is_bf16};
    const int64_t total = N * F;
    auto al = [](const void *q, int64_t ld, int bf) {        // 16-byte pieces of 8 columns: pointer and row pitch aligned
        return !q || (((uintptr_t)q & 15) == 0 && ld % (bf ? 8 : 4) == 0);
    };
    if (F % 8 == 0 && al(g, ldg, g_is_bf16) && al(out_for_mask, ldo, mask_is_bf16) && al(gm, ldgm, 1)) {
        const dim3 grid((unsigned)((total / 8 + 255) / 256));
        if (g_is_bf16 && mask_is_bf16) DC_LAUNCH((k_mask_grad_bf16x8<true, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else if (g_is_bf16) DC_LAUNCH((k_mask_grad_bf16x8<true, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else if (mask_is_bf16) DC_LAUNCH((k_mask_grad_bf16x8<false, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
        else DC_LAUNCH((k_mask_grad_bf16x8<false, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
        return check_launch("dc_tag_mask_grad_bf16");
    }
    DC_LAUNCH(k_mask_grad_bf16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("dc_tag_mask_grad_bf16");
}
