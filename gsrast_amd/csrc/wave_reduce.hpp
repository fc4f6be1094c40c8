// Reductions over the 64 lanes of a wavefront, each written once: contrib.hip, absgrad.hip and features.hip take theirs from here,
// and backward.hip's wave_sum12 is wave_sum8 and wave_sum4 below plus one select (its device assembly came out instruction for
// instruction what it was with the sequences written out there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

// Reductions of unsigned values by DPP (the shifts of blockbin.hpp's prefix32_inclusive: lanes 31 and 63 end up with their
// halves' results; lanes without a source read 0, the identity of both operations on unsigned values). Wave-uniform result.
template <typename Op>
__device__ __forceinline__ uint32_t wave_reduce_u32(uint32_t v, Op op) {
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    return op((uint32_t)__builtin_amdgcn_readlane((int)v, 31), (uint32_t)__builtin_amdgcn_readlane((int)v, 63));
}
struct AddU32 { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct MaxU32 { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
// (a tile's last contributor: the largest n_contrib of its 256 pixels bounds every walk over its list)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return wave_reduce_u32(v, MaxU32{}); }

#define GSR_DPP(v, ctrl, rows) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rows, 0xf, false))
// Sums of TWO per-lane values over the 64 lanes: v_permlane32_swap folds the halves while laying the values side by side (rows
// 0, 1: x, rows 2, 3: y), then the row shifts and the row broadcast of blockbin.hpp's prefix32_inclusive (lanes without a source
// read 0). On return lane 31 holds the total of x and lane 63 that of y; the other lanes hold partial sums.
__device__ __forceinline__ float wave_sum2(float x, float y) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    float v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    v += GSR_DPP(v, 0x111, 0xf);
    v += GSR_DPP(v, 0x112, 0xf);
    v += GSR_DPP(v, 0x114, 0xf);
    v += GSR_DPP(v, 0x118, 0xf);
    v += GSR_DPP(v, 0x142, 0xa);      // row_bcast:15 into rows 1 and 3
    return v;
}

__device__ __forceinline__ void swap32(float& x, float& y) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float& x, float& y) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}
// Sums of EIGHT per-lane values over the 64 lanes (the first eight of backward.hip's wave_sum12): v_permlane32_swap and
// v_permlane16_swap fold the lanes while packing the values side by side, one select + row_ror:8 packs two registers into one
// and three quad / half-row steps finish. On return lane 0 / 32 / 16 / 48 / 8 / 40 / 24 / 56 holds the total of value 0 / ... / 7.
__device__ __forceinline__ float wave_sum8(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7, int lane) {
    swap32(a0, a1); float p = a0 + a1;           // rows 0, 1: value 0 (lanes l and l + 32 added); rows 2, 3: value 1
    swap32(a2, a3); float q = a2 + a3;
    swap32(a4, a5); float r = a4 + a5;
    swap32(a6, a7); float t = a6 + a7;
    swap16(p, q); const float t0 = p + q;        // rows: value 0, 2, 1, 3, each added over the four 16-lane groups
    swap16(r, t); const float t1 = r + t;        // rows: value 4, 6, 5, 7
    const bool upper = (lane & 8) != 0;
    float u = (upper ? t1 : t0) + GSR_DPP(upper ? t0 : t1, 0x128, 0xf);      // row_ror:8: lanes 0-7 of a row now carry t0, lanes 8-15 t1
    u += GSR_DPP(u, 0xB1, 0xf);                  // quad_perm [1,0,3,2]
    u += GSR_DPP(u, 0x4E, 0xf);                  // quad_perm [2,3,0,1]
    u += GSR_DPP(u, 0x141, 0xf);                 // row_half_mirror
    return u;
}
// ... and of FOUR more (wave_sum12's last four): on return every lane of row 0 / 2 / 1 / 3 holds the total of value 0 / 1 / 2 / 3.
__device__ __forceinline__ float wave_sum4(float a0, float a1, float a2, float a3) {
    swap32(a0, a1); float pp = a0 + a1;
    swap32(a2, a3); float qq = a2 + a3;
    swap16(pp, qq); float w = pp + qq;           // rows: value 0, 2, 1, 3
    w += GSR_DPP(w, 0x128, 0xf);
    w += GSR_DPP(w, 0xB1, 0xf);
    w += GSR_DPP(w, 0x4E, 0xf);
    w += GSR_DPP(w, 0x141, 0xf);
    return w;
}
#undef GSR_DPP

}  // namespace gsr
