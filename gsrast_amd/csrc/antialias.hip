// Antialiased splatting (include/gsrast_amd_antialias.h): the opacity compensation c = sqrt(det(cov2D) / det(cov2D + 0.3 I))
// as its own per-Gaussian pass in front of gsr_forward, and its gradient behind gsr_backward. One lane per Gaussian,
// streaming (HBM-bound): no LDS, no atomics, nothing crosses lanes.
//
// The float32 arithmetic of the 2D covariance is gaussian_chain.hpp's, which is the two preprocess kernels' operation for
// operation, so that d1 below is the forward call's `det` bit for bit and the cull and clamp decisions are the forward's. The
// gradient is the same header's double side, the covariance part of gsr_backward's chain (backward.hip,
// preprocess_backward_kernel), seeded with dL/dcov2D.
#include "../../include/gsrast_amd_antialias.h"
#include "gaussian_chain.hpp"

namespace gsr {
namespace {

constexpr float kFloor = 0.000025f;      // upstream's floor of d0 / d1

struct AntialiasParams {
    int n;
    const float4* means3D;
    const float4* scales;
    const float4* rotations;
    const float* opacities;
    const float* view;
    const float* proj;
    float scale_modifier, tan_fovx, tan_fovy, focal_x, focal_y;
    // forward
    float* opacities_out;
    float* compensation;
    // backward
    const float* g_out;
    const int32_t* radii;
    float* dL_dopacities;
    float4* dL_dmeans3D;
    float4* dL_dscales;
    float4* dL_drotations;
};

// What the float32 forward decides for one Gaussian.
struct Compensation {
    float c = 1.0f;            // the factor
    bool flows = false;        // a gradient goes through c: the covariance was computed, d1 is finite and not zero, the floor is not active
    RatioClamp clamp = {};     // t.x / t.z (t.y / t.z) was clamped at +lim (-lim)
};

template <bool INRIA>
__device__ __forceinline__ Compensation compensation_of(const AntialiasParams& p, const float* view, const float* proj, const float4 mean,
                                                        const float4 sc, const float4 rot) {
    Compensation out;
    float tx, ty, tz;
    view_point<INRIA>(view, mean, tx, ty, tz);
    if constexpr (INRIA) {
        if (tz <= 0.2f) return out;
    } else {
        const float* m = proj;
        const float phx = (m[0] * mean.x + m[4] * mean.y) + (m[8] * mean.z + m[12] * mean.w);
        const float phy = (m[1] * mean.x + m[5] * mean.y) + (m[9] * mean.z + m[13] * mean.w);
        const float phz = (m[2] * mean.x + m[6] * mean.y) + (m[10] * mean.z + m[14] * mean.w);
        const float phw = (m[3] * mean.x + m[7] * mean.y) + (m[11] * mean.z + m[15] * mean.w);
        const float one_over_w = 1.0f / (0.001f + phw);
        const float prx = one_over_w * phx, pry = one_over_w * phy, prz = one_over_w * phz;
        if (prz < 0.0f || prz > 1.0f || prx < -1.3f || prx > 1.3f || pry < -1.3f || pry > 1.3f) return out;
    }
    const M3 sigma = covariance_of<INRIA>(p.scale_modifier, sc, rotation_of<INRIA>(rot));
    out.clamp = clamp_ratios_glm(tx, ty, tz, 1.3f * p.tan_fovx, 1.3f * p.tan_fovy);
    const M3 cv = cov2d_of(view, out.clamp, tz, p.focal_x, p.focal_y, sigma);
    const float a0 = cv.m[0][0], b = cv.m[0][1], c0 = cv.m[1][1];
    const float d0 = a0 * c0 - b * b;
    const float ca = a0 + 0.3f, cc = c0 + 0.3f;
    const float d1 = ca * cc - b * b;
    if (d1 == 0.0f || !__builtin_isfinite(d1)) return out;
    const float r = d0 / d1;
    out.c = sqrtf(fmaxr(kFloor, r));
    out.flows = kFloor < r;
    return out;
}

// Memory schedule of a wave: the view (and projection) matrix through the scalar cache, the three rows and the opacity of
// every lane in one round trip, then the stores.
template <bool INRIA>
__global__ __launch_bounds__(256) void antialias_forward_kernel(const AntialiasParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    float view[16], proj[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { view[i] = p.view[i]; proj[i] = INRIA ? 0.0f : p.proj[i]; }
    const float4 mean = ld4(p.means3D + idx), sc = ld4(p.scales + idx), rot = ld4(p.rotations + idx);
    const float o = p.opacities_out ? __builtin_nontemporal_load(p.opacities + idx) : 0.0f;
    const Compensation k = compensation_of<INRIA>(p, view, proj, mean, sc, rot);
    // (c == 1.0f: o * 1.0f is o bit for bit, a NaN's payload included, so no branch is needed for "o' = o")
    if (p.opacities_out) p.opacities_out[idx] = k.c == 1.0f ? o : o * k.c;
    if (p.compensation) p.compensation[idx] = k.c;
}

// Memory schedule: radii and g first (a culled Gaussian, or one the frame's backward left without a gradient — most of
// a scene — ends there and stores its zeros), then every remaining load, then the arithmetic, then the stores.
template <bool INRIA>
__global__ __launch_bounds__(256) void antialias_backward_kernel(const AntialiasParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    float view[16], proj[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { view[i] = p.view[i]; proj[i] = INRIA ? 0.0f : p.proj[i]; }
    const bool has_tile = p.radii == nullptr || p.radii[idx] > 0;
    const float g = has_tile ? __builtin_nontemporal_load(p.g_out + idx) : 0.0f;
    typedef double R;
    float g_o = 0.0f;
    R gmean[3] = {0, 0, 0}, gsc[3] = {0, 0, 0}, gq[4] = {0, 0, 0, 0};
    if (has_tile && g != 0.0f) {
        const float4 mean = ld4(p.means3D + idx), sc = ld4(p.scales + idx), rot = ld4(p.rotations + idx);
        const float o = __builtin_nontemporal_load(p.opacities + idx);
        const Compensation k = compensation_of<INRIA>(p, view, proj, mean, sc, rot);
        g_o = k.c * g;
        const bool chain = k.flows && (p.dL_dmeans3D || p.dL_dscales || p.dL_drotations);
        if (chain) {
            // t in double from the float32 inputs; the clamp decisions are the float32 forward's
            const R mx = (R)mean.x, my = (R)mean.y, mz = (R)mean.z;
            const R t0 = (R)view[0] * mx + (R)view[4] * my + (R)view[8] * mz + (R)view[12];
            const R t1 = (R)view[1] * mx + (R)view[5] * my + (R)view[9] * mz + (R)view[13];
            const R tz = (R)view[2] * mx + (R)view[6] * my + (R)view[10] * mz + (R)view[14];
            const R limx = (R)(1.3f * p.tan_fovx), limy = (R)(1.3f * p.tan_fovy);
            const RatioClamp& cl = k.clamp;
            const R cx = cl.hi_x ? limx : (cl.lo_x ? -limx : t0 / tz), cy = cl.hi_y ? limy : (cl.lo_y ? -limy : t1 / tz);
            const ProjectionFrame f = projection_frame(view, tz, cx, cy, cl.clx, cl.cly, (R)p.focal_x, (R)p.focal_y);
            const R mod = (R)p.scale_modifier;
            const R sv[3] = {mod * (R)sc.x, mod * (R)sc.y, mod * (R)sc.z};
            R Rm[3][3], qn[4], inv;
            rotation_f64<INRIA>(rot, Rm, qn, inv);
            R s[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    s[r][c] = Rm[r][0] * sv[0] * sv[0] * Rm[c][0] + Rm[r][1] * sv[1] * sv[1] * Rm[c][1] + Rm[r][2] * sv[2] * sv[2] * Rm[c][2];
            R a0, b, c0;
            cov2d_f64(f, s, a0, b, c0);
            const R ca = a0 + (R)0.3f, cc = c0 + (R)0.3f;
            const R d0 = a0 * c0 - b * b, d1 = ca * cc - b * b;
            const R r = d0 / d1;
            // G = o g through c = sqrt(r): dL/dr = G / (2 c); r = d0 / d1 to the three entries of cov2D
            const R gr = (R)o * (R)g / (2.0 * sqrt(r));
            const R id1 = 1.0 / d1;
            const R m00 = gr * (c0 - r * cc) * id1, m11 = gr * (a0 - r * ca) * id1;
            const R m01 = gr * (r - 1.0) * b * id1;          // each of the two off-diagonal entries: half of -2 b (1 - r) / d1
            if (p.dL_dmeans3D) mean_gradient(f, s, m00, m01, m11, gmean);
            if (p.dL_dscales || p.dL_drotations) {
                R gS[3][3], gR[3][3];
                sigma_gradient(f, m00, m01, m11, gS);
                scale_rotation_gradient(gS, Rm, sv, mod, gsc, gR);
                quaternion_gradient<INRIA>(gR, qn, inv, gq);
            }
        }
    }
    // ---- stores ----
    if (p.dL_dopacities) p.dL_dopacities[idx] = g_o;
    if (p.dL_dmeans3D) st4(p.dL_dmeans3D + idx, (float)gmean[0], (float)gmean[1], (float)gmean[2], 0.0f);
    if (p.dL_dscales) st4(p.dL_dscales + idx, (float)gsc[0], (float)gsc[1], (float)gsc[2], 0.0f);
    if (p.dL_drotations) st4(p.dL_drotations + idx, (float)gq[0], (float)gq[1], (float)gq[2], (float)gq[3]);
}

// What both argument structs share, checked and copied: every refusal of the header, before any HIP call.
template <typename Args>
int fill_params(const Args* a, AntialiasParams& p) {
    if (a->flags & ~(uint32_t)GSR_FLAG_SEMANTICS_INRIA) return GSR_ERR_INVALID_ARG;
    if (a->num_gaussians < 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!positive_finite(a->tan_fovx) || !positive_finite(a->tan_fovy) || !positive_finite(a->scale_modifier)) return GSR_ERR_INVALID_ARG;
    if (!a->means3D || !a->scales || !a->rotations || !a->opacities || !a->view_matrix) return GSR_ERR_INVALID_ARG;
    const bool inria = (a->flags & GSR_FLAG_SEMANTICS_INRIA) != 0;
    if (!inria && !a->proj_matrix) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->means3D, 16) || misaligned(a->scales, 16) || misaligned(a->rotations, 16)) return GSR_ERR_INVALID_ARG;
    p = AntialiasParams{};
    p.n = a->num_gaussians;
    p.means3D = reinterpret_cast<const float4*>(a->means3D);
    p.scales = reinterpret_cast<const float4*>(a->scales);
    p.rotations = reinterpret_cast<const float4*>(a->rotations);
    p.opacities = a->opacities;
    p.view = a->view_matrix;
    p.proj = a->proj_matrix;
    p.scale_modifier = a->scale_modifier;
    p.tan_fovx = a->tan_fovx;
    p.tan_fovy = a->tan_fovy;
    p.focal_y = (float)a->height / (2.0f * a->tan_fovy);
    p.focal_x = inria ? (float)a->width / (2.0f * a->tan_fovx) : p.focal_y;
    return GSR_OK;
}

int antialias_forward_impl(gsr_antialias_args* a) {
    if (!a || a->struct_size != sizeof(gsr_antialias_args)) return GSR_ERR_INVALID_ARG;
    AntialiasParams p;
    GSR_TRY(fill_params(a, p));
    if (!a->opacities_out && !a->compensation) return GSR_ERR_INVALID_ARG;
    if (a->opacities_out == a->opacities) return GSR_ERR_INVALID_ARG;
    if (p.n == 0) return GSR_OK;
    p.opacities_out = a->opacities_out;
    p.compensation = a->compensation;
    const dim3 grid((unsigned)(((long long)p.n + 255) / 256));
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(antialias_forward_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(antialias_forward_kernel<false>, grid, dim3(256), 0, stream, p);
    GSR_LAUNCH_CHECK("antialias_forward_kernel");
    return GSR_OK;
}

int antialias_backward_impl(gsr_antialias_backward_args* a) {
    if (!a || a->struct_size != sizeof(gsr_antialias_backward_args)) return GSR_ERR_INVALID_ARG;
    AntialiasParams p;
    GSR_TRY(fill_params(a, p));
    if (!a->dL_dopacities_out) return GSR_ERR_INVALID_ARG;
    if (!a->dL_dopacities && !a->dL_dmeans3D && !a->dL_dscales && !a->dL_drotations) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->dL_dmeans3D, 16) || misaligned(a->dL_dscales, 16) || misaligned(a->dL_drotations, 16)) return GSR_ERR_INVALID_ARG;
    if (p.n == 0) return GSR_OK;
    p.g_out = a->dL_dopacities_out;
    p.radii = a->radii;
    p.dL_dopacities = a->dL_dopacities;
    p.dL_dmeans3D = reinterpret_cast<float4*>(a->dL_dmeans3D);
    p.dL_dscales = reinterpret_cast<float4*>(a->dL_dscales);
    p.dL_drotations = reinterpret_cast<float4*>(a->dL_drotations);
    const dim3 grid((unsigned)(((long long)p.n + 255) / 256));
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(antialias_backward_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(antialias_backward_kernel<false>, grid, dim3(256), 0, stream, p);
    GSR_LAUNCH_CHECK("antialias_backward_kernel");
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

extern "C" int gsr_antialias_forward(gsr_antialias_args* a) { return gsr::entry_point(gsr::antialias_forward_impl, a); }
extern "C" int gsr_antialias_backward(gsr_antialias_backward_args* a) { return gsr::entry_point(gsr::antialias_backward_impl, a); }
