// Camera gradients (gsr_camera_backward): dL / d(view_matrix, proj_matrix, cam_pos) of the scalar that gsr_backward
// differentiates, from the per-Gaussian gradients that call left behind (dL_dmean2D, dL_dcov2D, dL_ddepths, dL_dcolors).
// The camera reaches L only through each visible Gaussian's pixel centre, 2-D covariance, depth and (upstream profile)
// view-dependent colour, so the gradient is a sum over the visible Gaussians of the OTHER contraction of the per-Gaussian
// chain that preprocess_backward_kernel (backward.hip) contracts with the Gaussian's own position.
//
// camera_pass_kernel: a fixed grid (sized from N alone) with a grid-stride loop. A thread first sums its Gaussians' 27
// non-zero camera entries in double registers; only then are the sums reduced over the wave (shuffles in a fixed
// order) and the block (LDS), and every block writes one row of partials into the caller's scratch. camera_sum_kernel,
// one block, adds the rows up in a fixed order and rounds each entry to float once. No atomics: two calls on the same
// input give the same bits on any device.
#include <hip/hip_runtime.h>

#include "backward_policy.hpp"
#include "gaussian_chain.hpp"

namespace gsr {
namespace {

constexpr int kCamThreads = 256;
constexpr int kCamWaves = kCamThreads / kWave;
constexpr int kCamMaxBlocks = 768;      // 3 blocks per CU of an MI355X: the whole grid is resident
constexpr int kCamTerms = 27;    // view rows 0-2 (12), proj rows 0, 1, 3 (12), cam_pos (3)
constexpr int kCamRow = 32;      // doubles per block row of the scratch (256 bytes)
// accumulator layout: view entry (row r, column c) at 3 c + r; proj entry (row 0 / 1 / 3, column c) at kProjAt + 3 c + 0 / 1 / 2
constexpr int kProjAt = 12, kCamAt = 24;

int camera_blocks(int n) {
    const long long blocks = ((long long)n + kCamThreads - 1) / kCamThreads;
    return (int)(blocks < kCamMaxBlocks ? blocks : kCamMaxBlocks);
}

struct CameraParams {
    unsigned n;
    const float4* __restrict__ means3D;
    const float* __restrict__ view;       // 16 floats, column-major, row 2 negated (the layout gsr_forward takes)
    const float* __restrict__ proj;
    const float* __restrict__ cam_pos;
    const float* __restrict__ cov3D;      // f32[6 N]
    const int32_t* __restrict__ radii;
    const float* __restrict__ shs;        // [N][16][3] (upstream profile with SH colour; else null)
    const uint8_t* __restrict__ clamped;  // bool[3 N]
    int sh_deg;
    const float2* __restrict__ dL_dmean2D;
    const float4* __restrict__ dL_dcov2D;  // (m00, m01, m11, 0)
    const float* __restrict__ dL_ddepths;  // or null: no depth channel
    const float* __restrict__ dL_dcolors;
    float tan_fovx, tan_fovy;
    float focal_x, focal_y;               // gscuda: both H / (2 tan_fovy)
    float w_eps;                          // gscuda 0.001f, upstream 1e-7f
    int width, height;
    int inria;                            // the projection takes (x, y, z, 1) instead of (x, y, z, mean.w)
    int depth_inverse;
    double* __restrict__ partial;         // [blocks][kCamRow]
};

// dB_k / d dir contracted with w_k = sh[k] . g over the k < (deg + 1)^2 basis functions (oracle/backward_np.py: sh_basis).
__device__ __forceinline__ void sh_direction_grad(int deg, double x, double y, double z, const float* __restrict__ sh,
                                                  const double (&g)[3], double (&gd)[3]) {
    constexpr double C1 = 0.4886025119029199;
    constexpr double C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                              0.5462742152960396};
    constexpr double C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                              -0.4570457994644658, 1.445305721320277, -0.5900435899266435};
    auto w = [&](int k) { return (double)sh[3 * k] * g[0] + (double)sh[3 * k + 1] * g[1] + (double)sh[3 * k + 2] * g[2]; };
    gd[0] = gd[1] = gd[2] = 0.0;
    if (deg < 1) return;
    gd[1] += -C1 * w(1); gd[2] += C1 * w(2); gd[0] += -C1 * w(3);
    if (deg < 2) return;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    {
        const double w4 = w(4), w5 = w(5), w6 = w(6), w7 = w(7), w8 = w(8);
        gd[0] += C2[0] * y * w4 - 2.0 * C2[2] * x * w6 + C2[3] * z * w7 + 2.0 * C2[4] * x * w8;
        gd[1] += C2[0] * x * w4 + C2[1] * z * w5 - 2.0 * C2[2] * y * w6 - 2.0 * C2[4] * y * w8;
        gd[2] += C2[1] * y * w5 + 4.0 * C2[2] * z * w6 + C2[3] * x * w7;
    }
    if (deg < 3) return;
    const double w9 = w(9), w10 = w(10), w11 = w(11), w12 = w(12), w13 = w(13), w14 = w(14), w15 = w(15);
    gd[0] += C3[0] * 6.0 * xy * w9 + C3[1] * yz * w10 + C3[2] * -2.0 * xy * w11 + C3[3] * -6.0 * xz * w12
           + C3[4] * (4.0 * zz - 3.0 * xx - yy) * w13 + C3[5] * 2.0 * xz * w14 + C3[6] * (3.0 * xx - 3.0 * yy) * w15;
    gd[1] += C3[0] * (3.0 * xx - 3.0 * yy) * w9 + C3[1] * xz * w10 + C3[2] * (4.0 * zz - xx - 3.0 * yy) * w11
           + C3[3] * -6.0 * yz * w12 + C3[4] * -2.0 * xy * w13 + C3[5] * -2.0 * yz * w14 + C3[6] * -6.0 * xy * w15;
    gd[2] += C3[1] * xy * w10 + C3[2] * 8.0 * yz * w11 + C3[3] * (6.0 * zz - 3.0 * xx - 3.0 * yy) * w12
           + C3[4] * 8.0 * xz * w13 + C3[5] * (xx - yy) * w14;
}

// What a visible Gaussian's terms read (68 bytes), loaded one Gaussian ahead of the arithmetic that uses it.
struct GaussianIn {
    float4 mean;
    float2 c3a, c3b, c3c;
    float2 g2;
    float4 gcv;
    float gdep;
};

__device__ __forceinline__ GaussianIn load_gaussian(const CameraParams& p, unsigned i) {
    GaussianIn g;
    g.mean = p.means3D[i];
    const float2* c3p = reinterpret_cast<const float2*>(p.cov3D + 6 * (size_t)i);
    g.c3a = c3p[0]; g.c3b = c3p[1]; g.c3c = c3p[2];
    g.g2 = p.dL_dmean2D[i];
    g.gcv = p.dL_dcov2D[i];
    g.gdep = p.dL_ddepths ? p.dL_ddepths[i] : 0.0f;
    return g;
}

// One visible Gaussian's camera terms, added to acc. The arithmetic is the chain's (preprocess_backward_kernel): t and the
// clamp decisions of t.x / t.z, t.y / t.z in the forward's float32 — gaussian_chain.hpp's, the statement that kernel calls —
// everything after in double, written out here on purpose: with fused multiply-adds (nothing there has to repeat a float32
// operation order) and one reciprocal of t.z.
template <bool SH>
__device__ __forceinline__ void add_camera_terms(const CameraParams& p, unsigned i, const GaussianIn& in, double (&acc)[kCamTerms]) {
    const float4 mean = in.mean;
    const float2 c3a = in.c3a, c3b = in.c3b, c3c = in.c3c;
    const float2 g2 = in.g2;
    const float4 gcv = in.gcv;
    const double gdep = (double)in.gdep;
    const float* vf = p.view;
    float txf, tyf, tzf;
    view_point<false>(vf, mean, txf, tyf, tzf);
    const RatioClamp cl = clamp_ratios_libm(txf, tyf, tzf, 1.3f * p.tan_fovx, 1.3f * p.tan_fovy);
    const bool clx = cl.clx, cly = cl.cly;
    {   // (the float32 above keeps the forward's operation order; from here on contraction is allowed)
#pragma clang fp contract(fast)
    const double tz = (double)tzf, cx = (double)cl.cx, cy = (double)cl.cy;
    const double tx = cx * tz, ty = cy * tz;
    const double fx = (double)p.focal_x, fy = (double)p.focal_y;
    const double itz = 1.0 / tz, itz2 = itz * itz;
    const double j00 = fx * itz, j11 = fy * itz, j02 = -fx * tx * itz2, j12 = -fy * ty * itz2;
    double W[3][3];                                       // W[r][c] = V[4 c + r], the upper 3 x 3 of the view matrix
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) W[r][c] = (double)vf[4 * c + r];
    // cov2D = P Sigma P^T with P = J W: gP = 2 gM P Sigma, dL/dW = J^T gP, and dL/dJ = gP W^T
    double P[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        P[0][c] = j00 * W[0][c] + j02 * W[2][c];
        P[1][c] = j11 * W[1][c] + j12 * W[2][c];
    }
    const double s[3][3] = {{c3a.x, c3a.y, c3b.x}, {c3a.y, c3b.y, c3c.x}, {c3b.x, c3c.x, c3c.y}};
    double ps[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) ps[r][c] = P[r][0] * s[0][c] + P[r][1] * s[1][c] + P[r][2] * s[2][c];
    const double m00 = gcv.x, m01 = gcv.y, m11 = gcv.z;
    double gP[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gP[0][c] = 2.0 * (m00 * ps[0][c] + m01 * ps[1][c]);
        gP[1][c] = 2.0 * (m01 * ps[0][c] + m11 * ps[1][c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        acc[3 * c + 0] += j00 * gP[0][c];
        acc[3 * c + 1] += j11 * gP[1][c];
        acc[3 * c + 2] += j02 * gP[0][c] + j12 * gP[1][c];
    }
    double gJ[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) gJ[r][k] = gP[r][0] * W[k][0] + gP[r][1] * W[k][1] + gP[r][2] * W[k][2];
    // dL/dt as the chain forms it; a clamped ratio passes its gradient to t.z only
    const double g_tx = -gJ[0][2] * fx * itz2, g_ty = -gJ[1][2] * fy * itz2;
    const double g_tz = -(gJ[0][0] * fx + gJ[1][1] * fy) * itz2 + (gJ[0][2] * fx * tx + gJ[1][2] * fy * ty) * (2.0 * itz2 * itz);
    const double gt0 = clx ? 0.0 : g_tx, gt1 = cly ? 0.0 : g_ty;
    double gt2 = g_tz + (clx ? g_tx * cx : 0.0) + (cly ? g_ty * cy : 0.0);
    gt2 += p.depth_inverse ? -gdep * itz2 : gdep;         // d_i = t.z, or 1 / t.z
    // t = V (x, y, z, 1)
    const double m[4] = {(double)mean.x, (double)mean.y, (double)mean.z, 1.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        acc[3 * c + 0] += gt0 * m[c];
        acc[3 * c + 1] += gt1 * m[c];
        acc[3 * c + 2] += gt2 * m[c];
    }
    // pixel centre: ((hx / wp) * 0.5 + 0.5) * W (gscuda) or ((hx / wp + 1) W - 1) / 2 (upstream), h = proj (x, y, z, m_w)
    const float* pm = p.proj;
    const double mw = p.inria ? 1.0 : (double)mean.w;
    const double mp[4] = {m[0], m[1], m[2], mw};
    const double hx = ((double)pm[0] * mp[0] + (double)pm[4] * mp[1]) + ((double)pm[8] * mp[2] + (double)pm[12] * mw);
    const double hy = ((double)pm[1] * mp[0] + (double)pm[5] * mp[1]) + ((double)pm[9] * mp[2] + (double)pm[13] * mw);
    const double wp = (double)p.w_eps + (((double)pm[3] * mp[0] + (double)pm[7] * mp[1]) + ((double)pm[11] * mp[2] + (double)pm[15] * mw));
    const double iw = 1.0 / wp;
    const double ax = 0.5 * (double)p.width * (double)g2.x * iw, ay = 0.5 * (double)p.height * (double)g2.y * iw;
    const double aw = -(ax * hx + ay * hy) * iw;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        acc[kProjAt + 3 * c + 0] += ax * mp[c];
        acc[kProjAt + 3 * c + 1] += ay * mp[c];
        acc[kProjAt + 3 * c + 2] += aw * mp[c];
    }
    if constexpr (SH) {
        // colour_c = max(0, 0.5 + sum_k B_k(dir) sh[k][c]), dir = (mean - cam) / |mean - cam|: the camera moves dir the other
        // way than the mean does; a channel clamped at zero passes nothing (oracle: inria_color_backward)
        const double dv[3] = {m[0] - (double)p.cam_pos[0], m[1] - (double)p.cam_pos[1], m[2] - (double)p.cam_pos[2]};
        const double len = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
        const double il = 1.0 / len;
        const double d[3] = {dv[0] * il, dv[1] * il, dv[2] * il};
        double g[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = p.clamped[3 * (size_t)i + c] ? 0.0 : (double)p.dL_dcolors[3 * (size_t)i + c];
        double gd[3];
        sh_direction_grad(p.sh_deg, d[0], d[1], d[2], p.shs + 48 * (size_t)i, g, gd);
        const double dot = d[0] * gd[0] + d[1] * gd[1] + d[2] * gd[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[kCamAt + j] -= (gd[j] - d[j] * dot) * il;
    }
    }
}

// The block's sums of the 27 entries, in a fixed order: over the wave by shuffles, then the waves in turn. Result in
// red[0][0 .. kCamTerms) (valid after the barrier this ends with).
__device__ __forceinline__ void block_sum(double (&acc)[kCamTerms], double (*red)[kCamTerms]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < kCamTerms; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
        acc[k] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kCamTerms; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < kCamTerms) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kCamWaves; ++w) v += red[w][threadIdx.x];
        red[0][threadIdx.x] = v;       // (thread k alone reads and writes column k)
    }
    __syncthreads();
}

template <bool SH>
__global__ __launch_bounds__(kCamThreads) void camera_pass_kernel(const CameraParams p) {
    __shared__ double red[kCamWaves][kCamTerms];
    double acc[kCamTerms];
#pragma unroll
    for (int k = 0; k < kCamTerms; ++k) acc[k] = 0.0;
    const unsigned stride = gridDim.x * kCamThreads;
    // radii first: an invisible Gaussian loads nothing else (a culled one may sit at t.z <= 0).
    // Two deep: while Gaussian i's terms are formed, the next one's inputs and the radius after that are in flight.
    unsigned i = blockIdx.x * kCamThreads + threadIdx.x;
    int r = i < p.n ? p.radii[i] : 0;
    GaussianIn cur = {};
    if (r > 0) cur = load_gaussian(p, i);
    unsigned next = i + stride;
    int r_next = next < p.n ? p.radii[next] : 0;
    while (i < p.n) {
        GaussianIn nxt = {};
        if (r_next > 0) nxt = load_gaussian(p, next);
        const unsigned after = next + stride;
        const int r_after = after < p.n ? p.radii[after] : 0;
        if (r > 0) add_camera_terms<SH>(p, i, cur, acc);
        i = next; r = r_next; cur = nxt;
        next = after; r_next = r_after;
    }
    block_sum(acc, red);
    if (threadIdx.x < kCamTerms) p.partial[(size_t)blockIdx.x * kCamRow + threadIdx.x] = red[0][threadIdx.x];
}

// One block: the rows of the partials in a fixed order (thread t: rows t, t + 256, ...), then as the pass kernel's blocks;
// the 35 floats of the three outputs, written in full (zeros where nothing depends on the entry).
__global__ __launch_bounds__(kCamThreads) void camera_sum_kernel(const double* __restrict__ partial, int rows,
                                                                 float* __restrict__ dview, float* __restrict__ dproj,
                                                                 float* __restrict__ dcam) {
    __shared__ double red[kCamWaves][kCamTerms];
    double acc[kCamTerms];
#pragma unroll
    for (int k = 0; k < kCamTerms; ++k) acc[k] = 0.0;
    for (int row = threadIdx.x; row < rows; row += kCamThreads) {
        const double* src = partial + (size_t)row * kCamRow;
#pragma unroll
        for (int k = 0; k < kCamTerms; ++k) acc[k] += src[k];
    }
    block_sum(acc, red);
    const int t = threadIdx.x;
    if (dview && t < 16) {
        const int r = t & 3, c = t >> 2;                  // column-major: entry t is (row t % 4, column t / 4)
        dview[t] = r < 3 ? (float)red[0][3 * c + r] : 0.0f;
    }
    if (dproj && t >= 16 && t < 32) {
        const int e = t - 16, r = e & 3, c = e >> 2;
        dproj[e] = r == 2 ? 0.0f : (float)red[0][kProjAt + 3 * c + (r == 3 ? 2 : r)];
    }
    if (dcam && t >= 32 && t < 35) dcam[t - 32] = (float)red[0][kCamAt + t - 32];
}

}  // namespace
}  // namespace gsr

using namespace gsr;

static int camera_backward_impl(gsr_camera_backward_args* a) {
    if (!a || a->struct_size != sizeof(gsr_camera_backward_args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    const int n = a->num_gaussians;
    if (n <= 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!a->means3D || !a->view_matrix || !a->proj_matrix || !a->cov3D || !a->radii || !a->dL_dmean2D || !a->dL_dcov2D ||
        !a->scratch)
        return GSR_ERR_INVALID_ARG;
    if (!a->dL_dview_matrix && !a->dL_dproj_matrix && !a->dL_dcam_pos) return GSR_ERR_INVALID_ARG;
    if (a->shs && (!a->dL_dcolors || !a->clamped || !a->cam_pos)) return GSR_ERR_INVALID_ARG;
    const bool inria = (a->flags & GSR_FLAG_SEMANTICS_INRIA) != 0;
    const bool sh = inria && a->shs != nullptr;          // (the reference's colour does not depend on the camera)
    const bool profile = (a->flags & GSR_FLAG_PROFILE) != 0;
    hipStream_t stream = (hipStream_t)a->stream;

    CameraParams p;
    p.n = (unsigned)n;
    p.means3D = reinterpret_cast<const float4*>(a->means3D);
    p.view = a->view_matrix;
    p.proj = a->proj_matrix;
    p.cam_pos = a->cam_pos;
    p.cov3D = a->cov3D;
    p.radii = a->radii;
    p.shs = sh ? a->shs : nullptr;
    p.clamped = a->clamped;
    // the focal lengths, w epsilon and SH degree of gsr_backward's chain
    const ProfileLens lens = profile_lens(inria, a->width, a->height, a->tan_fovx, a->tan_fovy, a->sh_dims);
    p.sh_deg = lens.sh_deg;
    p.dL_dmean2D = reinterpret_cast<const float2*>(a->dL_dmean2D);
    p.dL_dcov2D = reinterpret_cast<const float4*>(a->dL_dcov2D);
    p.dL_ddepths = a->dL_ddepths;
    p.dL_dcolors = a->dL_dcolors;
    p.tan_fovx = a->tan_fovx; p.tan_fovy = a->tan_fovy;
    p.focal_x = lens.focal_x; p.focal_y = lens.focal_y; p.w_eps = lens.w_eps;
    p.width = a->width; p.height = a->height;
    p.inria = inria ? 1 : 0;
    p.depth_inverse = (a->flags & GSR_FLAG_DEPTH_INVERSE) ? 1 : 0;
    p.partial = static_cast<double*>(a->scratch);

    CallEvents<2> events;
    hipEvent_t* const ev = events.ev;
    if (profile) {
        GSR_TRY(events.create());
        GSR_HIP_TRY(hipEventRecord(ev[0], stream));
    }
    const int blocks = camera_blocks(n);
    if (sh) hipLaunchKernelGGL(camera_pass_kernel<true>, dim3((unsigned)blocks), dim3(kCamThreads), 0, stream, p);
    else hipLaunchKernelGGL(camera_pass_kernel<false>, dim3((unsigned)blocks), dim3(kCamThreads), 0, stream, p);
    GSR_LAUNCH_CHECK("camera_pass_kernel");
    hipLaunchKernelGGL(camera_sum_kernel, dim3(1), dim3(kCamThreads), 0, stream, (const double*)p.partial, blocks,
                       a->dL_dview_matrix, a->dL_dproj_matrix, a->dL_dcam_pos);
    GSR_LAUNCH_CHECK("camera_sum_kernel");
    if (profile) {
        GSR_HIP_TRY(hipEventRecord(ev[1], stream));
        GSR_HIP_TRY(hipEventSynchronize(ev[1]));
        GSR_HIP_TRY(hipEventElapsedTime(&a->stage_ms, ev[0], ev[1]));
    }
    return GSR_OK;
}

extern "C" size_t gsr_camera_backward_scratch_bytes(int32_t num_gaussians) {
    return num_gaussians > 0 ? (size_t)camera_blocks(num_gaussians) * kCamRow * sizeof(double) : 0;
}

extern "C" int gsr_camera_backward(gsr_camera_backward_args* a) { return entry_point(camera_backward_impl, a); }
