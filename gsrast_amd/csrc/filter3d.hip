// The 3D smoothing filter of Mip-Splatting (include/gsrast_amd_filter3d.h): the nearest depth at which a training camera sees
// each Gaussian (observe), the filter value from it (finalize), the smoothing of scales and opacities in front of gsr_forward and
// its gradient behind gsr_backward. One lane per Gaussian throughout.
//
// observe is bound by vector issue (some thirty float operations per pair, the position in registers, the camera records
// through the scalar cache); the three others stream (HBM-bound): no LDS, and nothing crosses lanes but finalize's maximum.
// This file is compiled with -ffp-contract=off like every other: the float32 arithmetic is the header's, operation for operation.
#include "../../include/gsrast_amd_filter3d.h"
#include "gsr_common.hpp"

namespace gsr {
namespace {

constexpr int kCam = GSR_FILTER3D_CAMERA_FLOATS;
constexpr int kChunk = GSR_FILTER3D_CAMERA_CHUNK;
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint32_t kKBits = 0x3EE4F92Eu;             // the float32 nearest to the double 0.2 ** 0.5
constexpr size_t kTempBytes = 16;                    // one word, kept a whole 16-byte granule

// glm's
__device__ __forceinline__ float fmin_glm(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float fmax_glm(float a, float b) { return (a < b) ? b : a; }

// blockIdx.x: 256 Gaussians; blockIdx.y: a chunk of kChunk cameras. `cameras` is indexed by loop-uniform values only, so the
// records arrive by scalar loads and cost no vector memory traffic.
__global__ __launch_bounds__(256) void filter3d_observe_kernel(int n, int stride, int num_cameras, const float* __restrict__ positions,
                                                               const float* __restrict__ cameras, float* min_depth) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const float* p = positions + (size_t)idx * (size_t)stride;
    const float x = p[0], y = p[1], z = p[2];
    const float loaded = min_depth[idx];
    float best = loaded;
    const int first = blockIdx.y * kChunk;
    const int last = first + kChunk < num_cameras ? first + kChunk : num_cameras;
    for (int k = first; k < last; ++k) {
        const float* c = cameras + (size_t)k * kCam;
        const float t0 = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
        const float t1 = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
        const float t2 = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
        const float zc = fmax_glm(t2, 0.001f);
        const float px = (t0 / zc) * c[12] + c[14];
        const float py = (t1 / zc) * c[13] + c[15];
        const bool valid = t2 > 0.2f && px >= c[16] && px <= c[17] && py >= c[18] && py <= c[19];
        if (valid) best = fmin_glm(best, t2);
    }
    // positive floats order as their bit patterns do, +inf last: an integer minimum is the float minimum
    if (best < loaded) atomicMin(reinterpret_cast<unsigned int*>(min_depth) + idx, __float_as_uint(best));
}

// The largest finite min_depth: a wave reduction, then one integer atomic maximum per wave into word[0] (cleared by the call).
__global__ __launch_bounds__(256) void filter3d_max_kernel(int n, const float* __restrict__ min_depth, unsigned int* word) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    unsigned int v = 0u;
    if (idx < n) {
        const float m = min_depth[idx];
        if (m < __uint_as_float(kInfBits)) v = __float_as_uint(m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int o = (unsigned int)__shfl_xor((int)v, off, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v != 0u) atomicMax(word, v);
}

__global__ __launch_bounds__(256) void filter3d_value_kernel(int n, const float* __restrict__ min_depth, const unsigned int* __restrict__ word,
                                                             float max_focal, float* __restrict__ filter) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const float d_max = __uint_as_float(word[0]);
    const float m = min_depth[idx];
    const float d = (m < __uint_as_float(kInfBits)) ? m : d_max;
    filter[idx] = (d / max_focal) * __uint_as_float(kKBits);
}

// What the float32 forward computes of one Gaussian.
struct Smoothed {
    bool identity;
    float f2;
    float s[3];                // s'_j
    float coef;
};

__device__ __forceinline__ Smoothed smoothed_of(const float4 sc, const float f) {
    Smoothed out;
    out.f2 = f * f;
    out.identity = !(out.f2 > 0.0f);
    const float s[3] = {sc.x, sc.y, sc.z};
    float r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float q = s[j] * s[j];
        const float a = q + out.f2;
        out.s[j] = sqrtf(a);
        r[j] = q / a;
    }
    out.coef = sqrtf((r[0] * r[1]) * r[2]);
    return out;
}

struct ForwardParams {
    int n;
    const float4* scales;
    const float* opacities;
    const float* filter;
    float4* scales_out;
    float* opacities_out;
};

__global__ __launch_bounds__(256) void filter3d_forward_kernel(const ForwardParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    const float4 sc = ld4(p.scales + idx);
    const float f = __builtin_nontemporal_load(p.filter + idx);
    const float o = p.opacities_out ? __builtin_nontemporal_load(p.opacities + idx) : 0.0f;
    const Smoothed k = smoothed_of(sc, f);
    if (p.scales_out) {
        if (k.identity) st4(p.scales_out + idx, sc.x, sc.y, sc.z, sc.w);
        else st4(p.scales_out + idx, k.s[0], k.s[1], k.s[2], sc.w);
    }
    if (p.opacities_out) p.opacities_out[idx] = k.identity ? o : o * k.coef;
}

struct BackwardParams {
    int n;
    const float4* scales;
    const float* opacities;
    const float* filter;
    const float4* g_scales;
    const float* g_opacities;
    const int32_t* radii;
    float4* dL_dscales;
    float* dL_dopacities;
};

// Memory schedule: the radius first (a culled Gaussian ends there and stores its zeros), then every remaining load, the
// arithmetic, the stores.
__global__ __launch_bounds__(256) void filter3d_backward_kernel(const BackwardParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    float out_s[3] = {0.0f, 0.0f, 0.0f}, out_o = 0.0f;
    if (p.radii == nullptr || p.radii[idx] > 0) {
        const float4 sc = ld4(p.scales + idx);
        const float f = __builtin_nontemporal_load(p.filter + idx);
        const float4 gs = p.g_scales ? ld4(p.g_scales + idx) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float go = p.g_opacities ? __builtin_nontemporal_load(p.g_opacities + idx) : 0.0f;
        const Smoothed k = smoothed_of(sc, f);
        if (k.identity) {
            out_s[0] = gs.x; out_s[1] = gs.y; out_s[2] = gs.z;
            out_o = go;
        } else {
            out_o = k.coef * go;
            if (p.dL_dscales) {
                typedef double R;
                const float o = p.g_opacities ? __builtin_nontemporal_load(p.opacities + idx) : 0.0f;
                const R f2 = (R)f * (R)f;
                const R s[3] = {(R)sc.x, (R)sc.y, (R)sc.z}, g[3] = {(R)gs.x, (R)gs.y, (R)gs.z};
                R root[3], u[3], w[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const R a = s[j] * s[j] + f2;
                    root[j] = sqrt(a);
                    u[j] = fabs(s[j]) / root[j];
                    w[j] = __builtin_isinf(a) ? 0.0 : f2 / (a * root[j]);
                }
                const R G = (R)o * (R)go;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const R sign = s[j] > 0.0 ? 1.0 : (s[j] < 0.0 ? -1.0 : 0.0);
                    const R others = u[(j + 1) % 3] * u[(j + 2) % 3];
                    R v = g[j] * s[j] / root[j];
                    if (p.g_opacities) v += G * sign * w[j] * others;
                    out_s[j] = (float)v;
                }
            }
        }
    }
    if (p.dL_dscales) st4(p.dL_dscales + idx, out_s[0], out_s[1], out_s[2], 0.0f);
    if (p.dL_dopacities) p.dL_dopacities[idx] = out_o;
}

inline dim3 rows_grid(int n) { return dim3((unsigned)(((long long)n + 255) / 256)); }

int observe_impl(gsr_filter3d_observe_args* a) {
    if (!a || a->struct_size != sizeof(gsr_filter3d_observe_args)) return GSR_ERR_INVALID_ARG;
    if (a->flags != 0u || a->num_gaussians < 0 || a->num_cameras < 0) return GSR_ERR_INVALID_ARG;
    if (a->position_stride != 3 && a->position_stride != 4) return GSR_ERR_INVALID_ARG;
    if (!a->positions || !a->min_depth || (a->num_cameras > 0 && !a->cameras)) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->positions, 4) || misaligned(a->cameras, 4) || misaligned(a->min_depth, 4)) return GSR_ERR_INVALID_ARG;
    if (static_cast<const void*>(a->min_depth) == a->positions || static_cast<const void*>(a->min_depth) == a->cameras) return GSR_ERR_INVALID_ARG;
    const long long chunks = ((long long)a->num_cameras + kChunk - 1) / kChunk;
    if (chunks > 65535) return GSR_ERR_TOO_LARGE;
    if (a->num_gaussians == 0 || a->num_cameras == 0) return GSR_OK;
    dim3 grid = rows_grid(a->num_gaussians);
    grid.y = (unsigned)chunks;
    hipLaunchKernelGGL(filter3d_observe_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(a->stream), a->num_gaussians,
                       a->position_stride, a->num_cameras, a->positions, a->cameras, a->min_depth);
    GSR_LAUNCH_CHECK("filter3d_observe_kernel");
    return GSR_OK;
}

int finalize_impl(gsr_filter3d_finalize_args* a) {
    if (!a || a->struct_size != sizeof(gsr_filter3d_finalize_args)) return GSR_ERR_INVALID_ARG;
    if (a->flags != 0u || a->num_gaussians < 0) return GSR_ERR_INVALID_ARG;
    if (!positive_finite(a->max_focal)) return GSR_ERR_INVALID_ARG;
    if (!a->min_depth || !a->filter || !a->temp) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->min_depth, 4) || misaligned(a->filter, 4) || misaligned(a->temp, 16)) return GSR_ERR_INVALID_ARG;
    if (a->temp_bytes < kTempBytes) return GSR_ERR_INVALID_ARG;
    if (a->filter == a->min_depth || static_cast<const void*>(a->filter) == a->temp || static_cast<const void*>(a->min_depth) == a->temp)
        return GSR_ERR_INVALID_ARG;
    if (a->num_gaussians == 0) return GSR_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    unsigned int* word = reinterpret_cast<unsigned int*>(a->temp);
    GSR_HIP_TRY(hipMemsetAsync(word, 0, sizeof(unsigned int), stream));
    hipLaunchKernelGGL(filter3d_max_kernel, rows_grid(a->num_gaussians), dim3(256), 0, stream, a->num_gaussians, a->min_depth, word);
    GSR_LAUNCH_CHECK("filter3d_max_kernel");
    hipLaunchKernelGGL(filter3d_value_kernel, rows_grid(a->num_gaussians), dim3(256), 0, stream, a->num_gaussians, a->min_depth, word,
                       a->max_focal, a->filter);
    GSR_LAUNCH_CHECK("filter3d_value_kernel");
    return GSR_OK;
}

inline bool same(const void* out, const void* in) { return out != nullptr && out == in; }

int forward_impl(gsr_filter3d_args* a) {
    if (!a || a->struct_size != sizeof(gsr_filter3d_args)) return GSR_ERR_INVALID_ARG;
    if (a->flags != 0u || a->num_gaussians < 0) return GSR_ERR_INVALID_ARG;
    if (!a->scales || !a->opacities || !a->filter) return GSR_ERR_INVALID_ARG;
    if (!a->scales_out && !a->opacities_out) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->scales, 16) || misaligned(a->scales_out, 16) || misaligned(a->opacities, 4) || misaligned(a->filter, 4) ||
        misaligned(a->opacities_out, 4))
        return GSR_ERR_INVALID_ARG;
    const void* in[3] = {a->scales, a->opacities, a->filter};
    for (const void* q : in)
        if (same(a->scales_out, q) || same(a->opacities_out, q)) return GSR_ERR_INVALID_ARG;
    if (same(a->scales_out, a->opacities_out)) return GSR_ERR_INVALID_ARG;
    if (a->num_gaussians == 0) return GSR_OK;
    ForwardParams p;
    p.n = a->num_gaussians;
    p.scales = reinterpret_cast<const float4*>(a->scales);
    p.opacities = a->opacities;
    p.filter = a->filter;
    p.scales_out = reinterpret_cast<float4*>(a->scales_out);
    p.opacities_out = a->opacities_out;
    hipLaunchKernelGGL(filter3d_forward_kernel, rows_grid(p.n), dim3(256), 0, reinterpret_cast<hipStream_t>(a->stream), p);
    GSR_LAUNCH_CHECK("filter3d_forward_kernel");
    return GSR_OK;
}

int backward_impl(gsr_filter3d_backward_args* a) {
    if (!a || a->struct_size != sizeof(gsr_filter3d_backward_args)) return GSR_ERR_INVALID_ARG;
    if (a->flags != 0u || a->num_gaussians < 0) return GSR_ERR_INVALID_ARG;
    if (!a->scales || !a->opacities || !a->filter) return GSR_ERR_INVALID_ARG;
    if (!a->dL_dscales_out && !a->dL_dopacities_out) return GSR_ERR_INVALID_ARG;
    if (!a->dL_dscales && !a->dL_dopacities) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->scales, 16) || misaligned(a->dL_dscales_out, 16) || misaligned(a->dL_dscales, 16) || misaligned(a->opacities, 4) ||
        misaligned(a->filter, 4) || misaligned(a->dL_dopacities_out, 4) || misaligned(a->radii, 4) || misaligned(a->dL_dopacities, 4))
        return GSR_ERR_INVALID_ARG;
    const void* in[6] = {a->scales, a->opacities, a->filter, a->dL_dscales_out, a->dL_dopacities_out, a->radii};
    for (const void* q : in)
        if (same(a->dL_dscales, q) || same(a->dL_dopacities, q)) return GSR_ERR_INVALID_ARG;
    if (same(a->dL_dscales, a->dL_dopacities)) return GSR_ERR_INVALID_ARG;
    if (a->num_gaussians == 0) return GSR_OK;
    BackwardParams p;
    p.n = a->num_gaussians;
    p.scales = reinterpret_cast<const float4*>(a->scales);
    p.opacities = a->opacities;
    p.filter = a->filter;
    p.g_scales = reinterpret_cast<const float4*>(a->dL_dscales_out);
    p.g_opacities = a->dL_dopacities_out;
    p.radii = a->radii;
    p.dL_dscales = reinterpret_cast<float4*>(a->dL_dscales);
    p.dL_dopacities = a->dL_dopacities;
    hipLaunchKernelGGL(filter3d_backward_kernel, rows_grid(p.n), dim3(256), 0, reinterpret_cast<hipStream_t>(a->stream), p);
    GSR_LAUNCH_CHECK("filter3d_backward_kernel");
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

extern "C" size_t gsr_filter3d_temp_bytes(int32_t num_gaussians) { return num_gaussians < 0 ? 0 : gsr::kTempBytes; }
extern "C" int gsr_filter3d_observe(gsr_filter3d_observe_args* a) { return gsr::entry_point(gsr::observe_impl, a); }
extern "C" int gsr_filter3d_finalize(gsr_filter3d_finalize_args* a) { return gsr::entry_point(gsr::finalize_impl, a); }
extern "C" int gsr_filter3d_forward(gsr_filter3d_args* a) { return gsr::entry_point(gsr::forward_impl, a); }
extern "C" int gsr_filter3d_backward(gsr_filter3d_backward_args* a) { return gsr::entry_point(gsr::backward_impl, a); }
