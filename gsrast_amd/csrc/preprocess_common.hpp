// What the two preprocess kernels (preprocess.hip, preprocess_inria.hip) and the duplication (binning.hip) share beyond
// gaussian_chain.hpp's 3 x 3 matrices and glm's min / max: the 16-pixel tile rectangle with its band clipping, the
// packed-rectangle encoding, and the parameter fields both kernels take from a call. The two kernels still spell out their own
// covariance arithmetic, which differs between them on purpose; gaussian_chain.hpp states the same arithmetic for every other pass.
// (Of that header they take M3, mul3, transpose3, fminr and fmaxr only; the whole of it is included because the two kernels are
// meant to take its float32 functions too, once that leaves their resource figures and the preprocess stage's time unchanged.)
#pragma once
#include "gaussian_chain.hpp"

namespace gsr {

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
