// The two operators of the normal-consistency loss (include/gsrast_amd_normals.h): the per-Gaussian normal — the shortest axis
// of the Gaussian in view space, turned towards the camera — with its gradient to the rotation, and the normal of a depth
// surface with its gradient to the depth. One lane per Gaussian (per pixel), streaming: no LDS, no atomics, nothing crosses
// lanes. The depth backward is a gather: a pixel recomputes the float32 decisions of its four neighbours and adds their shares.
//
// The float32 arithmetic states the header operation for operation (this file is compiled with -ffp-contract=off); R and t are
// gaussian_chain.hpp's, the preprocess kernels' own. The gradients are evaluated in double from the float32 inputs, with the
// float32 forward's decisions, and rounded once; from R to the quaternion they take that header's double side.
#include "../../include/gsrast_amd_normals.h"
#include "gaussian_chain.hpp"

namespace gsr {
namespace {

// ---- the per-Gaussian normal ----------------------------------------------------------------------------------------------------
struct GaussianNormalParams {
    int n;
    const float4* means3D;
    const float4* scales;
    const float4* rotations;
    const float* view;
    float* normals;                // forward: float[N][3]
    const float* g_normals;        // backward: float[N][3]
    const int32_t* radii;
    float4* dL_drotations;
};

// What the float32 forward decides for one Gaussian, and its output.
struct GaussianNormal {
    int axis = 0;                  // the shortest axis: the column of R
    bool flipped = false;          // n_v was negated
    bool valid = false;            // l is finite and not zero
    float n[3] = {0.0f, 0.0f, 0.0f};
};

template <bool INRIA>
__device__ __forceinline__ GaussianNormal gaussian_normal_of(const float* v, const float4 mean, const float4 sc, const float4 rot) {
    GaussianNormal out;
    const float s[3] = {sc.x, sc.y, sc.z};
    int a = 0;
    if (s[1] < s[a]) a = 1;
    if (s[2] < s[a]) a = 2;
    out.axis = a;
    float t0, t1, t2;
    view_point<INRIA>(v, mean, t0, t1, t2);
    float nw[3];
    rotation_axis<INRIA>(rotation_of<INRIA>(rot), a, nw);
    float nv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) nv[r] = (v[r] * nw[0] + v[4 + r] * nw[1]) + v[8 + r] * nw[2];
    const float d = (nv[0] * t0 + nv[1] * t1) + nv[2] * t2;
    if (d > 0.0f) {
        out.flipped = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) nv[r] = -nv[r];
    }
    const float l = sqrtf((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
    if (l == 0.0f || !__builtin_isfinite(l)) return out;
    out.valid = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) out.n[r] = nv[r] / l;
    return out;
}

// Memory schedule of a wave: the view matrix through the scalar cache, the three rows of every lane in one round trip, then
// three stores of 12-byte stride (a wave writes 768 contiguous bytes between them).
template <bool INRIA>
__global__ __launch_bounds__(256) void gaussian_normals_forward_kernel(const GaussianNormalParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    float view[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) view[i] = p.view[i];
    const float4 mean = ld4(p.means3D + idx), sc = ld4(p.scales + idx), rot = ld4(p.rotations + idx);
    const GaussianNormal k = gaussian_normal_of<INRIA>(view, mean, sc, rot);
    float* o = p.normals + 3 * (size_t)idx;
    o[0] = k.n[0]; o[1] = k.n[1]; o[2] = k.n[2];
}

// Memory schedule: radii and the incoming gradient first (a culled Gaussian, or one without a gradient — most of a scene — ends
// there and stores its zeros), then the three rows, the arithmetic, the store.
template <bool INRIA>
__global__ __launch_bounds__(256) void gaussian_normals_backward_kernel(const GaussianNormalParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    float view[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) view[i] = p.view[i];
    const bool has_tile = p.radii == nullptr || p.radii[idx] > 0;
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (has_tile) {
        const float* gi = p.g_normals + 3 * (size_t)idx;
        g[0] = gi[0]; g[1] = gi[1]; g[2] = gi[2];
    }
    typedef double R;
    R gq[4] = {0, 0, 0, 0};
    if (has_tile && !(g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f)) {
        const float4 mean = ld4(p.means3D + idx), sc = ld4(p.scales + idx), rot = ld4(p.rotations + idx);
        const GaussianNormal k = gaussian_normal_of<INRIA>(view, mean, sc, rot);
        if (k.valid) {
            const int a = k.axis;
            const R sigma = k.flipped ? -1.0 : 1.0;
            R Rm[3][3], qn[4], inv;
            rotation_f64<INRIA>(rot, Rm, qn, inv);
            R nw[3];
            rotation_axis_f64(Rm, a, nw);
            R v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = (R)view[i];
            R nv[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) nv[r] = sigma * (v[r] * nw[0] + v[4 + r] * nw[1] + v[8 + r] * nw[2]);
            const R l = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
            const R u[3] = {nv[0] / l, nv[1] / l, nv[2] / l};
            const R ug = u[0] * (R)g[0] + u[1] * (R)g[1] + u[2] * (R)g[2];
            R gnv[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) gnv[r] = ((R)g[r] - u[r] * ug) / l;
            // dL/dR: column a is sigma W^T dL/dn_v, the other columns are zero
            R gR[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const R gnw = sigma * (v[4 * r + 0] * gnv[0] + v[4 * r + 1] * gnv[1] + v[4 * r + 2] * gnv[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) gR[r][c] = (c == a) ? gnw : 0.0;
            }
            quaternion_gradient<INRIA>(gR, qn, inv, gq);
        }
    }
    st4(p.dL_drotations + idx, (float)gq[0], (float)gq[1], (float)gq[2], (float)gq[3]);
}

// ---- the normal of a depth surface ----------------------------------------------------------------------------------------------
constexpr int kTileX = 64, kTileY = 4;          // a workgroup's pixels: each wave one 256-byte row segment

struct DepthNormalParams {
    int width, height, tiles_x;
    float tan_fovx, tan_fovy;
    const float* depth;
    float* normals;                // forward: float[3][H][W]
    const float* g_normals;        // backward: float[3][H][W]
    float* dL_ddepth;
};

template <bool INRIA, typename T>
__device__ __forceinline__ T ndc_of(int i, T size) {
    if constexpr (INRIA) return ((T)2 * (T)i + (T)1) / size - (T)1;
    else return ((T)2 * (T)i) / size - (T)1;
}

// What the float32 forward decides for an interior pixel, and its output.
struct DepthNormal {
    bool valid = false, flipped = false;
    float n[3] = {0.0f, 0.0f, 0.0f};
};

template <bool INRIA>
__device__ __forceinline__ DepthNormal depth_normal_of(const DepthNormalParams& p, int x, int y, float du, float dl, float dr, float dd) {
    DepthNormal out;
    if (!(positive_finite(du) && positive_finite(dl) && positive_finite(dr) && positive_finite(dd))) return out;
    const float wf = (float)p.width, hf = (float)p.height;
    const float rx = ndc_of<INRIA>(x, wf) * p.tan_fovx, rxl = ndc_of<INRIA>(x - 1, wf) * p.tan_fovx, rxr = ndc_of<INRIA>(x + 1, wf) * p.tan_fovx;
    const float ry = ndc_of<INRIA>(y, hf) * p.tan_fovy, ryu = ndc_of<INRIA>(y - 1, hf) * p.tan_fovy, ryd = ndc_of<INRIA>(y + 1, hf) * p.tan_fovy;
    const float dvx = rx * dd - rx * du, dvy = ryd * dd - ryu * du, dvz = dd - du;
    const float dhx = rxr * dr - rxl * dl, dhy = ry * dr - ry * dl, dhz = dr - dl;
    float cx = dvy * dhz - dvz * dhy, cy = dvz * dhx - dvx * dhz, cz = dvx * dhy - dvy * dhx;
    if ((cx * rx + cy * ry) + cz > 0.0f) {
        out.flipped = true;
        cx = -cx; cy = -cy; cz = -cz;
    }
    const float l = sqrtf((cx * cx + cy * cy) + cz * cz);
    if (l == 0.0f || !__builtin_isfinite(l)) return out;
    out.valid = true;
    out.n[0] = cx / l; out.n[1] = cy / l; out.n[2] = cz / l;
    return out;
}

__device__ __forceinline__ bool interior(const DepthNormalParams& p, int x, int y) {
    return x >= 1 && x <= p.width - 2 && y >= 1 && y <= p.height - 2;
}

template <bool INRIA>
__global__ __launch_bounds__(kTileX * kTileY) void depth_normals_forward_kernel(const DepthNormalParams p) {
    const int x = (int)(blockIdx.x % (unsigned)p.tiles_x) * kTileX + (int)threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)p.tiles_x) * kTileY + (int)threadIdx.y;
    if (x >= p.width || y >= p.height) return;
    const size_t at = (size_t)y * p.width + x, plane = (size_t)p.width * p.height;
    DepthNormal k;
    if (interior(p, x, y)) {
        const float du = p.depth[at - p.width], dl = p.depth[at - 1], dr = p.depth[at + 1], dd = p.depth[at + p.width];
        k = depth_normal_of<INRIA>(p, x, y, du, dl, dr, dd);
    }
    p.normals[at] = k.n[0];
    p.normals[plane + at] = k.n[1];
    p.normals[2 * plane + at] = k.n[2];
}

// The share of pixel q = (x, y)'s normal that goes to one of its four neighbour depths: which = 0 its up (Du), 1 its left (Dl),
// 2 its right (Dr), 3 its down (Dd). 0.0 where q has no valid normal.
template <bool INRIA>
__device__ __forceinline__ double depth_normal_share(const DepthNormalParams& p, int x, int y, int which) {
    if (!interior(p, x, y)) return 0.0;
    const size_t at = (size_t)y * p.width + x, plane = (size_t)p.width * p.height;
    const float fu = p.depth[at - p.width], fl = p.depth[at - 1], fr = p.depth[at + 1], fd = p.depth[at + p.width];
    const DepthNormal k = depth_normal_of<INRIA>(p, x, y, fu, fl, fr, fd);
    if (!k.valid) return 0.0;
    typedef double R;
    const R g[3] = {(R)p.g_normals[at], (R)p.g_normals[plane + at], (R)p.g_normals[2 * plane + at]};
    const R wf = (R)(float)p.width, hf = (R)(float)p.height, tx = (R)p.tan_fovx, ty = (R)p.tan_fovy;
    const R rx = ndc_of<INRIA>(x, wf) * tx, rxl = ndc_of<INRIA>(x - 1, wf) * tx, rxr = ndc_of<INRIA>(x + 1, wf) * tx;
    const R ry = ndc_of<INRIA>(y, hf) * ty, ryu = ndc_of<INRIA>(y - 1, hf) * ty, ryd = ndc_of<INRIA>(y + 1, hf) * ty;
    const R du = (R)fu, dl = (R)fl, dr = (R)fr, dd = (R)fd;
    const R dv[3] = {rx * dd - rx * du, ryd * dd - ryu * du, dd - du};
    const R dh[3] = {rxr * dr - rxl * dl, ry * dr - ry * dl, dr - dl};
    const R c[3] = {dv[1] * dh[2] - dv[2] * dh[1], dv[2] * dh[0] - dv[0] * dh[2], dv[0] * dh[1] - dv[1] * dh[0]};
    const R l = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const R u[3] = {c[0] / l, c[1] / l, c[2] / l};
    const R ug = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
    const R sl = (k.flipped ? -1.0 : 1.0) / l;
    const R gc[3] = {(g[0] - u[0] * ug) * sl, (g[1] - u[1] * ug) * sl, (g[2] - u[2] * ug) * sl};
    if (which == 0 || which == 3) {
        const R gdv[3] = {dh[1] * gc[2] - dh[2] * gc[1], dh[2] * gc[0] - dh[0] * gc[2], dh[0] * gc[1] - dh[1] * gc[0]};      // dh x gc
        return which == 3 ? (gdv[0] * rx + gdv[1] * ryd) + gdv[2] : -((gdv[0] * rx + gdv[1] * ryu) + gdv[2]);
    }
    const R gdh[3] = {gc[1] * dv[2] - gc[2] * dv[1], gc[2] * dv[0] - gc[0] * dv[2], gc[0] * dv[1] - gc[1] * dv[0]};          // gc x dv
    return which == 2 ? (gdh[0] * rxr + gdh[1] * ry) + gdh[2] : -((gdh[0] * rxl + gdh[1] * ry) + gdh[2]);
}

template <bool INRIA>
__global__ __launch_bounds__(kTileX * kTileY) void depth_normals_backward_kernel(const DepthNormalParams p) {
    const int x = (int)(blockIdx.x % (unsigned)p.tiles_x) * kTileX + (int)threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)p.tiles_x) * kTileY + (int)threadIdx.y;
    if (x >= p.width || y >= p.height) return;
    // up, left, right, down of this pixel: it is that neighbour's down, right, left, up depth
    const double up = depth_normal_share<INRIA>(p, x, y - 1, 3);
    const double left = depth_normal_share<INRIA>(p, x - 1, y, 2);
    const double right = depth_normal_share<INRIA>(p, x + 1, y, 1);
    const double down = depth_normal_share<INRIA>(p, x, y + 1, 0);
    p.dL_ddepth[(size_t)y * p.width + x] = (float)(((up + left) + right) + down);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// What both Gaussian argument structs share, checked and copied: every refusal of the header, before any HIP call.
template <typename Args>
int fill_gaussian_params(const Args* a, GaussianNormalParams& p) {
    if (a->flags & ~(uint32_t)GSR_FLAG_SEMANTICS_INRIA) return GSR_ERR_INVALID_ARG;
    if (a->num_gaussians < 0) return GSR_ERR_INVALID_ARG;
    if (!a->means3D || !a->scales || !a->rotations || !a->view_matrix) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->means3D, 16) || misaligned(a->scales, 16) || misaligned(a->rotations, 16)) return GSR_ERR_INVALID_ARG;
    p = GaussianNormalParams{};
    p.n = a->num_gaussians;
    p.means3D = reinterpret_cast<const float4*>(a->means3D);
    p.scales = reinterpret_cast<const float4*>(a->scales);
    p.rotations = reinterpret_cast<const float4*>(a->rotations);
    p.view = a->view_matrix;
    return GSR_OK;
}

int gaussian_normals_forward_impl(gsr_gaussian_normals_args* a) {
    if (!a || a->struct_size != sizeof(gsr_gaussian_normals_args)) return GSR_ERR_INVALID_ARG;
    GaussianNormalParams p;
    GSR_TRY(fill_gaussian_params(a, p));
    if (!a->normals) return GSR_ERR_INVALID_ARG;
    if (p.n == 0) return GSR_OK;
    p.normals = a->normals;
    const dim3 grid((unsigned)(((long long)p.n + 255) / 256));
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(gaussian_normals_forward_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(gaussian_normals_forward_kernel<false>, grid, dim3(256), 0, stream, p);
    GSR_LAUNCH_CHECK("gaussian_normals_forward_kernel");
    return GSR_OK;
}

int gaussian_normals_backward_impl(gsr_gaussian_normals_backward_args* a) {
    if (!a || a->struct_size != sizeof(gsr_gaussian_normals_backward_args)) return GSR_ERR_INVALID_ARG;
    GaussianNormalParams p;
    GSR_TRY(fill_gaussian_params(a, p));
    if (!a->dL_dnormals || !a->dL_drotations || misaligned(a->dL_drotations, 16)) return GSR_ERR_INVALID_ARG;
    if (p.n == 0) return GSR_OK;
    p.g_normals = a->dL_dnormals;
    p.radii = a->radii;
    p.dL_drotations = reinterpret_cast<float4*>(a->dL_drotations);
    const dim3 grid((unsigned)(((long long)p.n + 255) / 256));
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(gaussian_normals_backward_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(gaussian_normals_backward_kernel<false>, grid, dim3(256), 0, stream, p);
    GSR_LAUNCH_CHECK("gaussian_normals_backward_kernel");
    return GSR_OK;
}

template <typename Args>
int fill_depth_params(const Args* a, DepthNormalParams& p, dim3& grid) {
    if (a->flags & ~(uint32_t)GSR_FLAG_SEMANTICS_INRIA) return GSR_ERR_INVALID_ARG;
    if (a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!positive_finite(a->tan_fovx) || !positive_finite(a->tan_fovy)) return GSR_ERR_INVALID_ARG;
    if (!a->depth) return GSR_ERR_INVALID_ARG;
    p = DepthNormalParams{};
    p.width = a->width;
    p.height = a->height;
    p.tiles_x = (a->width + kTileX - 1) / kTileX;
    p.tan_fovx = a->tan_fovx;
    p.tan_fovy = a->tan_fovy;
    p.depth = a->depth;
    const long long blocks = (long long)p.tiles_x * ((a->height + kTileY - 1) / kTileY);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    grid = dim3((unsigned)blocks);
    return GSR_OK;
}

int depth_normals_forward_impl(gsr_depth_normals_args* a) {
    if (!a || a->struct_size != sizeof(gsr_depth_normals_args)) return GSR_ERR_INVALID_ARG;
    DepthNormalParams p;
    dim3 grid;
    GSR_TRY(fill_depth_params(a, p, grid));
    if (!a->normals || a->normals == a->depth) return GSR_ERR_INVALID_ARG;
    p.normals = a->normals;
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(depth_normals_forward_kernel<true>, grid, dim3(kTileX, kTileY), 0, stream, p);
    else hipLaunchKernelGGL(depth_normals_forward_kernel<false>, grid, dim3(kTileX, kTileY), 0, stream, p);
    GSR_LAUNCH_CHECK("depth_normals_forward_kernel");
    return GSR_OK;
}

int depth_normals_backward_impl(gsr_depth_normals_backward_args* a) {
    if (!a || a->struct_size != sizeof(gsr_depth_normals_backward_args)) return GSR_ERR_INVALID_ARG;
    DepthNormalParams p;
    dim3 grid;
    GSR_TRY(fill_depth_params(a, p, grid));
    if (!a->dL_dnormals || !a->dL_ddepth || a->dL_ddepth == a->depth || a->dL_ddepth == a->dL_dnormals) return GSR_ERR_INVALID_ARG;
    p.g_normals = a->dL_dnormals;
    p.dL_ddepth = a->dL_ddepth;
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(depth_normals_backward_kernel<true>, grid, dim3(kTileX, kTileY), 0, stream, p);
    else hipLaunchKernelGGL(depth_normals_backward_kernel<false>, grid, dim3(kTileX, kTileY), 0, stream, p);
    GSR_LAUNCH_CHECK("depth_normals_backward_kernel");
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

extern "C" int gsr_gaussian_normals_forward(gsr_gaussian_normals_args* a) { return gsr::entry_point(gsr::gaussian_normals_forward_impl, a); }
extern "C" int gsr_gaussian_normals_backward(gsr_gaussian_normals_backward_args* a) { return gsr::entry_point(gsr::gaussian_normals_backward_impl, a); }
extern "C" int gsr_depth_normals_forward(gsr_depth_normals_args* a) { return gsr::entry_point(gsr::depth_normals_forward_impl, a); }
extern "C" int gsr_depth_normals_backward(gsr_depth_normals_backward_args* a) { return gsr::entry_point(gsr::depth_normals_backward_impl, a); }
