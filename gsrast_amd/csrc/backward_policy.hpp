// gsr_backward's argument contract and per-call constants (the stages of backward.hip call them), in the manner of
// frame_policy.hpp: host C++17 only and pure — the argument struct in, small structs out; no HIP, nothing is dereferenced
// (tests/test_backward_policy.py). Which pointers of gsr_backward_args must come together is decided here and nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gsrast_amd.h"
#include "frame_policy.hpp"      // (FrameDims, tile_band)

namespace gsr {

// What a legal gsr_backward call is: the modes its pointers and flags select, and its band of tile rows.
struct BackwardChoice {
    bool wide;             // sums_f64: the sums are kept in double, the float arrays of the sums are optional copies
    bool chain;            // the per-Gaussian chain runs (cov2D -> cov3D -> inputs, colour -> SH)
    bool depth;            // dL_dout_depth: the depth channel
    bool inria;            // GSR_FLAG_SEMANTICS_INRIA
    bool have_receipt;     // (any other magic than the library's: refused by lists_of_receipt)
    bool profile;          // GSR_FLAG_PROFILE
    bool depth_inverse;    // GSR_FLAG_DEPTH_INVERSE
    bool alpha;            // dL_dout_alpha of gsr_backward_alpha: the accumulated opacity's term (a seed of the render backward: nothing else comes with it)
    FrameDims d;
};

// The rules of include/gsrast_amd.h (gsr_backward_args), in the order a call that breaks several is answered for.
// dL_dout_alpha: the second argument of gsr_backward_alpha (include/gsrast_amd_opacity.h), null for gsr_backward: it adds no rule.
inline int choose_backward(const gsr_backward_args& a, BackwardChoice* out, const float* dL_dout_alpha = nullptr) {
    BackwardChoice c{};
    if (a.num_gaussians <= 0 || a.width <= 0 || a.height <= 0 || !a.background || !a.means2D || !a.conic_opacity || !a.colors ||
        !a.ranges || !a.n_contrib || !a.final_t || !a.dL_dout_color)
        return GSR_ERR_INVALID_ARG;
    // (the float arrays of the sums are where the sums are kept unless sums_f64 keeps them: optional outputs then)
    c.wide = a.sums_f64 != nullptr;
    if (!c.wide && (!a.dL_dmean2D || !a.dL_dconic_opacity || !a.dL_dcolors)) return GSR_ERR_INVALID_ARG;
    // the chain runs for whichever of its outputs is asked for; without sums_f64 it starts from dL_dcov3D's presence
    c.chain = a.dL_dcov3D || (c.wide && (a.dL_dmeans3D || a.dL_dscales || a.dL_dshs));
    if (c.chain && (!a.cov3D || !a.means3D || !a.view_matrix || !a.radii)) return GSR_ERR_INVALID_ARG;
    if ((a.dL_dmeans3D || a.dL_dscales || a.dL_drotations) && !c.chain) return GSR_ERR_INVALID_ARG;
    if (a.dL_dmeans3D && !a.proj_matrix) return GSR_ERR_INVALID_ARG;
    if ((a.dL_dscales || a.dL_drotations) && (!a.scales || !a.rotations || !a.dL_dscales)) return GSR_ERR_INVALID_ARG;
    c.inria = (a.flags & GSR_FLAG_SEMANTICS_INRIA) != 0;
    // the upstream profile's chain needs what its colour was computed from
    if (c.inria && a.dL_dshs && (!a.shs || !a.cam_pos || !a.clamped || !a.means3D)) return GSR_ERR_INVALID_ARG;
    // the depth channel: d_i is recomputed from means3D and the view; its sums go to depth_sums_f64 beside sums_f64, else to dL_ddepths
    c.depth = a.dL_dout_depth != nullptr;
    if (c.depth && (!a.means3D || !a.view_matrix || (c.wide ? !a.depth_sums_f64 : !a.dL_ddepths))) return GSR_ERR_INVALID_ARG;
    c.alpha = dL_dout_alpha != nullptr;
    c.profile = (a.flags & GSR_FLAG_PROFILE) != 0;
    c.depth_inverse = (a.flags & GSR_FLAG_DEPTH_INVERSE) != 0;
    if (tile_band(a.width, a.height, a.tile_row_begin, a.tile_row_end, &c.d) != GSR_OK) return GSR_ERR_INVALID_ARG;
    // without a receipt only the reference's contract can hold: the sorted lists in point_list
    c.have_receipt = a.receipt.magic != 0;
    if (!c.have_receipt && !a.point_list) return GSR_ERR_INVALID_ARG;
    *out = c;
    return GSR_OK;
}

// What the two semantics profiles differ in on the way from a Gaussian to its pixel, for gsr_backward's chain and for
// gsr_camera_backward alike. gscuda has ONE focal length, H / (2 tan_fovy), for both axes (GSCuda.cu:197-231), the upstream
// profile two; the epsilon is the one added to the homogeneous w of the projected mean.
struct ProfileLens { float focal_x, focal_y, w_eps; int sh_deg; };
inline ProfileLens profile_lens(bool inria, int width, int height, float tan_fovx, float tan_fovy, int sh_dims) {
    ProfileLens l;
    l.focal_y = (float)height / (2.0f * tan_fovy);
    l.focal_x = inria ? (float)width / (2.0f * tan_fovx) : l.focal_y;
    l.w_eps = inria ? 0.0000001f : 0.001f;
    l.sh_deg = sh_dims < 0 ? 0 : (sh_dims > 3 ? 3 : sh_dims);
    return l;
}

// The per-Gaussian output arrays of gsr_backward_args with their floats per row, in the order they are cleared. The first
// kBackwardSums are where the render backward's float atomics land: cleared on every call that does not keep the sums in
// double, and, like the rest, where nothing was rendered (R == 0: all-zero gradients). dL_ddepths counts only with the depth channel.
struct BackwardOutput { float* gsr_backward_args::*array; int row_floats; };
constexpr int kBackwardSums = 5;
constexpr BackwardOutput kBackwardOutputs[] = {
    {&gsr_backward_args::dL_dmean2D, 2},  {&gsr_backward_args::dL_dconic_opacity, 4}, {&gsr_backward_args::dL_dcolors, 3},
    {&gsr_backward_args::dL_dcov2D, 4},   {&gsr_backward_args::dL_ddepths, 1},
    {&gsr_backward_args::dL_dcov3D, 6},   {&gsr_backward_args::dL_dshs, 48},          {&gsr_backward_args::dL_dmeans3D, 4},
    {&gsr_backward_args::dL_dscales, 4},  {&gsr_backward_args::dL_drotations, 4},
};

}  // namespace gsr
