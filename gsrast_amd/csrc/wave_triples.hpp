// A wave's 64 records of an array of three floats per Gaussian, moved as 16-byte vectors (activations.hip, adam.hip).
//
// 64 records are 768 contiguous bytes: 48 lanes move them as 16-byte vectors to or from a wave-private LDS region of
// kTriple floats, where every lane finds its own three floats at a stride of three words (no bank conflict: 3 is odd).
// A vector straddles two records. `wanted` (bit r set = record r is in use) decides per vector: one with a wanted record is
// moved whole, one without is not touched. The region is private to the wave: __builtin_amdgcn_wave_barrier() between the
// staging and the reads, no workgroup barrier.
#pragma once
#include "gsr_common.hpp"

namespace gsr {

constexpr int kTriple = 3 * kWave;        // floats of one wave's records in an array of three floats per Gaussian

// The wave's `count` records of three floats, global -> LDS. `src` is 16-byte aligned (the array is, and a wave starts at a
// multiple of 768 bytes). `wanted`: bit r set = record r is read afterwards; a vector none of whose floats is wanted is
// not loaded.
__device__ __forceinline__ void stage_triples(const float* __restrict__ src, int count, float* w, int lane, unsigned long long wanted) {
    const int nfloats = 3 * count, bulk = nfloats & ~3;
    const int f = 4 * lane;
    if (f < bulk) {
        const int r0 = f / 3, r1 = (f + 3) / 3;                              // (f + 3 <= 191: record 63 at most)
        if (((wanted >> r0) | (wanted >> r1)) & 1ull)
            *reinterpret_cast<float4*>(w + f) = *reinterpret_cast<const float4*>(src + f);
    }
    const int t = bulk + lane;                                               // a partial wave's last one to three floats
    if (t < nfloats && ((wanted >> (t / 3)) & 1ull)) w[t] = src[t];
}

// ... and LDS -> global, by the same rule: a vector with a wanted record is written whole (an unwanted neighbour's floats
// are then what stage_triples with the same `wanted` loaded, or what the caller put there), one without is not written.
// The default writes every float of the wave's records.
__device__ __forceinline__ void flush_triples(float* __restrict__ dst, int count, const float* w, int lane,
                                              unsigned long long wanted = ~0ull) {
    const int nfloats = 3 * count, bulk = nfloats & ~3;
    const int f = 4 * lane;
    if (f < bulk) {
        const int r0 = f / 3, r1 = (f + 3) / 3;
        if (((wanted >> r0) | (wanted >> r1)) & 1ull)
            *reinterpret_cast<float4*>(dst + f) = *reinterpret_cast<const float4*>(w + f);
    }
    const int t = bulk + lane;
    if (t < nfloats && ((wanted >> (t / 3)) & 1ull)) dst[t] = w[t];
}

}  // namespace gsr
