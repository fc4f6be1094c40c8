// What the two preprocess kernels (preprocess.hip, preprocess_inria.hip) and the duplication (binning.hip) share: 3 x 3
// matrices, glm's min / max, the 16-pixel tile rectangle with its band clipping, the packed-rectangle encoding, and the
// parameter fields both kernels take from a call. The kernels' own arithmetic differs on purpose and stays in their files.
#pragma once
#include "gsr_common.hpp"

namespace gsr {

struct M3 { float m[3][3]; };   // m[col][row]

__device__ __forceinline__ float fminr(float a, float b) { return (b < a) ? b : a; }   // glm::min
__device__ __forceinline__ float fmaxr(float a, float b) { return (a < b) ? b : a; }   // glm::max

__device__ __forceinline__ M3 mul3(const M3& a, const M3& b) {
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int row = 0; row < 3; ++row)
            r.m[c][row] = a.m[0][row] * b.m[c][0] + a.m[1][row] * b.m[c][1] + a.m[2][row] * b.m[c][2];
    return r;
}
__device__ __forceinline__ M3 transpose3(const M3& a) {
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int row = 0; row < 3; ++row) r.m[c][row] = a.m[row][c];
    return r;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(hi, max(lo, v)); }

// getRect with the y range clipped to the tile-row band of this call (the whole grid
// when the call is not sharded: then it is exactly GSCuda.cu:249-259).
__device__ __forceinline__ void tile_rect(float px, float py, int ex, int ey, const FrameDims& d,
                                          int& x0, int& y0, int& x1, int& y1) {
    x0 = clampi((int)((px - (float)ex) / 16.0f), 0, d.grid_x);
    y0 = clampi((int)((py - (float)ey) / 16.0f), 0, d.grid_y);
    x1 = clampi((int)((((px + (float)ex) + 16.0f) - 1.0f) / 16.0f), 0, d.grid_x);
    y1 = clampi((int)((((py + (float)ey) + 16.0f) - 1.0f) / 16.0f), 0, d.grid_y);
    y0 = clampi(y0, d.row_begin, d.row_end);
    y1 = clampi(y1, d.row_begin, d.row_end);
}

// x0 | w << 8 | y0 << 16 | h << 24 of a band-clipped rectangle (grids up to 255 x 255)
__device__ __forceinline__ uint32_t pack_rect(int x0, int y0, int x1, int y1) {
    return (uint32_t)x0 | ((uint32_t)(x1 - x0) << 8) | ((uint32_t)y0 << 16) | ((uint32_t)(y1 - y0) << 24);
}

// Fills the fields PreprocessParams and InriaParams share. Only this code is single: the fields themselves are still declared
// in both structs, under the same names, because a struct's member order is its kernel's argument layout and a shared base
// would move it. A field added to both structs must be added here too — nothing else sets it. wave_sums: store_wave_sums.
template <typename Params>
inline void fill_preprocess_params(Params& p, const gsr_forward_args& a, const gsr_geometry_state& g, int32_t* radii,
                                   uint32_t* depth_keys, uint32_t* rect_packed, const FrameDims& d, uint4* wave_sums, uint32_t big_from) {
    p.n = a.num_gaussians;
    p.means3D = reinterpret_cast<const float4*>(a.means3D);
    p.scales = reinterpret_cast<const float4*>(a.scales);
    p.scale_modifier = a.scale_modifier;
    p.rotations = reinterpret_cast<const float4*>(a.rotations);
    p.opacities = a.opacities;
    p.shs = a.shs;
    p.cov3D_precomp = a.cov3D_precomp;
    p.colors_precomp = a.colors_precomp;
    p.view = a.view_matrix;
    p.proj = a.proj_matrix;
    p.tan_fovx = a.tan_fovx;
    p.tan_fovy = a.tan_fovy;
    p.radii = radii;
    p.means2D = reinterpret_cast<float2*>(g.means2D);
    p.depths = g.depths;
    p.cov3Ds = g.cov3D;
    p.rgb = g.rgb;
    p.conic_opacity = reinterpret_cast<float4*>(g.conic_opacity);
    p.tiles_touched = g.tiles_touched;
    p.depth_keys = depth_keys;
    p.rect_packed = rect_packed;
    p.wave_sums = wave_sums;
    p.big_from = big_from;
    p.dims = d;
}

}  // namespace gsr
