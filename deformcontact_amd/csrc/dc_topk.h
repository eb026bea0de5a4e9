// dc_topk.h -- the wave-resident best-`cap` list of the neighbour searches (dc_neighbors.hip, dc_neighbors_nd.hip)
// and the index helpers both use.  A candidate is one 64-bit key, ord_key(d2) << 32 | j, so that keys compare as
// (d2, j); lane l of the query's wave holds the l-th smallest key seen so far (kTopkNone = an empty slot).
#pragma once
#include "dc_common.h"

namespace dc {

constexpr unsigned long long kTopkNone = ~0ull;   // an empty slot; every real key is smaller

__device__ __forceinline__ unsigned ord_key(float f) {          // order-preserving map float -> unsigned
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_val(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__device__ __forceinline__ unsigned long long topk_key(float d2, int j) {
    return ((unsigned long long)ord_key(d2) << 32) | (unsigned)j;
}

// lane `l` (wave-uniform) of a 64-bit value, as a wave-uniform value: two v_readlane, no LDS crossbar
__device__ __forceinline__ unsigned long long wave_read(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// the value of lane - 1 (lane 0 keeps its own): DPP wave_shr:1, a VALU move per half
__device__ __forceinline__ unsigned long long wave_up1(unsigned long long v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned ulo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    const unsigned uhi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return ((unsigned long long)uhi << 32) | ulo;
}

// Insert this wave's 64 candidates (`key` of every lane; kTopkNone = none) into the sorted list: those below the
// current cap-th key `kth`, one at a time in lane order, each by a ballot for its rank and a shift that moves the tail
// up; after every insertion the candidates that no longer beat the new cap-th key drop out.  `entry` = this lane's
// slot, `kth` = the entry of lane cap - 1 (wave-uniform); 1 <= cap <= 64.  The whole wave must call it.
__device__ __forceinline__ void topk_insert(unsigned long long key, int lane, int cap, unsigned long long &entry,
                                            unsigned long long &kth) {
    unsigned long long m = __ballot(key < kth);
    while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        const unsigned long long c = wave_read(key, src);          // (c < kth: m holds only such lanes)
        const int pos = __popcll(__ballot(entry < c));
        const unsigned long long up = wave_up1(entry);
        if (lane == pos) entry = c;
        else if (lane > pos && lane < cap) entry = up;
        kth = wave_read(entry, cap - 1);
        m = __ballot(key < kth) & ~((2ull << src) - 1);            // the lanes behind src that still qualify
    }
}

// the list as a row of nbr [*, cap] (rank order, then -1) and its length
__device__ __forceinline__ void topk_store(unsigned long long entry, int lane, int cap, int32_t *nbr_row,
                                           int32_t *count_out) {
    const int count = __popcll(__ballot(entry != kTopkNone));
    if (lane < cap) nbr_row[lane] = lane < count ? (int32_t)(unsigned)entry : -1;
    if (lane == 0) *count_out = count;
}

// first index in [lo, hi) whose value is >= v (hi if none)
template <typename T>
__device__ __forceinline__ int64_t lower_bound(const T *a, int64_t lo, int64_t hi, T v) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
template <typename T>
__device__ __forceinline__ int64_t upper_bound(const T *a, int64_t lo, int64_t hi, T v) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace dc
