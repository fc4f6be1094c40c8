// A trainer's raw parameters <-> the arrays gsr_forward takes, and the gradients back.
//
//   gsr_activate_params          — positions (x,y,z) -> (x,y,z,1), log-scales -> exp with w = e, quaternions normalised,
//       opacity logits -> sigmoid: the arithmetic of ply_activate_kernel (activation_math.hpp), from separate arrays
//       instead of the 62-float file record.
//   gsr_activate_params_backward — the gradients of gsr_backward (vec4 arrays) through those four functions, to the raw
//       arrays (3 / 1 / 3 / 4 floats per Gaussian). Formed in double from the float32 inputs and rounded once, as the
//       N-sized chain of backward.hip is. A Gaussian the frame culled (radii[i] <= 0) gets zeros and loads nothing else.
//
// Both are bound by their bytes (forward 44 read + 52 written per Gaussian; backward at most 4 + 4 + 12 + 16 + 4 x 16 = 100
// read + 44 written). One wave takes 64 Gaussians. The vec4 arrays are one 16-byte access per lane; the arrays of three
// floats per Gaussian are 768 contiguous bytes per wave: 48 lanes move them as 16-byte vectors to or from a wave-private
// LDS region, where every lane finds its own three floats at a stride of three words (no bank conflict: 3 is odd).
#include "activation_math.hpp"
#include "gsr_common.hpp"
#include "wave_triples.hpp"      // (stage_triples / flush_triples)

namespace gsr {
namespace {

__global__ __launch_bounds__(256) void activate_params_kernel(int n, const float* __restrict__ raw_means,
                                                              const float* __restrict__ raw_opacity,
                                                              const float* __restrict__ raw_scales,
                                                              const float4* __restrict__ raw_rotations,
                                                              float4* __restrict__ means3D, float4* __restrict__ scales,
                                                              float4* __restrict__ rotations, float* __restrict__ opacities) {
    __shared__ __attribute__((aligned(16))) float lds[4][2][kTriple];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long first = ((long long)blockIdx.x * 4 + wave) * kWave;     // first Gaussian of this wave
    if (first >= n) return;
    const int count = (int)min((long long)kWave, (long long)n - first);
    float* wm = lds[wave][0];
    float* ws = lds[wave][1];
    stage_triples(raw_means + 3 * first, count, wm, lane, ~0ull);
    stage_triples(raw_scales + 3 * first, count, ws, lane, ~0ull);
    __builtin_amdgcn_wave_barrier();                                         // wave-private LDS: no workgroup barrier
    if (lane < count) {
        const long long i = first + lane;
        const float4 q = raw_rotations[i];
        const float x = raw_opacity[i];
        const float* m = wm + 3 * lane;
        const float* s = ws + 3 * lane;
        means3D[i] = make_float4(m[0], m[1], m[2], 1.0f);
        scales[i] = activate_scale(s[0], s[1], s[2]);
        rotations[i] = activate_rotation(q.x, q.y, q.z, q.w);
        opacities[i] = activate_opacity(x);
    }
}

struct ActivateBackwardParams {
    int n;
    const float* raw_opacity;
    const float* raw_scales;
    const float4* raw_rotations;
    const int32_t* radii;
    const float4* dL_dmeans3D;
    const float4* dL_dscales;
    const float4* dL_drotations;
    const float4* dL_dconic_opacity;
    float* dL_draw_means;
    float* dL_draw_opacity;
    float* dL_draw_scales;
    float4* dL_draw_rotations;
};

__global__ __launch_bounds__(256) void activate_params_backward_kernel(const ActivateBackwardParams p) {
    __shared__ __attribute__((aligned(16))) float lds[4][3][kTriple];       // raw scales in | mean gradients out | scale gradients out
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long first = ((long long)blockIdx.x * 4 + wave) * kWave;
    if (first >= p.n) return;
    const int count = (int)min((long long)kWave, (long long)p.n - first);
    const long long i = first + lane;
    const bool valid = lane < count;
    // the radius first: a culled Gaussian loads nothing else
    const bool visible = valid && (p.radii == nullptr || p.radii[i] > 0);
    const unsigned long long wanted = __ballot(visible);
    float* w_in = lds[wave][0];
    float* w_means = lds[wave][1];
    float* w_scales = lds[wave][2];
    // ---- loads ----
    if (p.dL_draw_scales) stage_triples(p.raw_scales + 3 * first, count, w_in, lane, wanted);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 gm = zero, gs = zero, gq = zero, r = zero, gco = zero;
    float x = 0.0f;
    if (visible) {
        if (p.dL_draw_means) gm = p.dL_dmeans3D[i];
        if (p.dL_draw_scales) gs = p.dL_dscales[i];
        if (p.dL_draw_rotations) { gq = p.dL_drotations[i]; r = p.raw_rotations[i]; }
        if (p.dL_draw_opacity) { gco = p.dL_dconic_opacity[i]; x = p.raw_opacity[i]; }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- arithmetic: double from the float32 inputs, rounded to float once ----
    if (p.dL_draw_means && valid) {
        w_means[3 * lane] = gm.x; w_means[3 * lane + 1] = gm.y; w_means[3 * lane + 2] = gm.z;
    }
    if (p.dL_draw_scales && valid) {
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        if (visible) {
            const float* s = w_in + 3 * lane;
            o0 = (float)((double)gs.x * exp((double)s[0]));
            o1 = (float)((double)gs.y * exp((double)s[1]));
            o2 = (float)((double)gs.z * exp((double)s[2]));
        }
        w_scales[3 * lane] = o0; w_scales[3 * lane + 1] = o1; w_scales[3 * lane + 2] = o2;
    }
    float go = 0.0f;
    if (p.dL_draw_opacity && visible) {
        // sigmoid(x) sigmoid(-x) = e / (1 + e)^2 with e = exp(-|x|): no overflow at either end
        const double e = exp(-fabs((double)x));
        go = (float)((double)gco.w * (e / ((1.0 + e) * (1.0 + e))));
    }
    float4 gr = zero;
    if (p.dL_draw_rotations && visible) {
        const double r0 = r.x, r1 = r.y, r2 = r.z, r3 = r.w;
        const double inv = 1.0 / sqrt((r0 * r0 + r1 * r1) + (r2 * r2 + r3 * r3));
        const double q0 = r0 * inv, q1 = r1 * inv, q2 = r2 * inv, q3 = r3 * inv;
        const double dot = (q0 * (double)gq.x + q1 * (double)gq.y) + (q2 * (double)gq.z + q3 * (double)gq.w);
        gr = make_float4((float)(((double)gq.x - q0 * dot) * inv), (float)(((double)gq.y - q1 * dot) * inv),
                         (float)(((double)gq.z - q2 * dot) * inv), (float)(((double)gq.w - q3 * dot) * inv));
    }
    __builtin_amdgcn_wave_barrier();
    // ---- stores ----
    if (p.dL_draw_means) flush_triples(p.dL_draw_means + 3 * first, count, w_means, lane);
    if (p.dL_draw_scales) flush_triples(p.dL_draw_scales + 3 * first, count, w_scales, lane);
    if (valid) {
        if (p.dL_draw_opacity) p.dL_draw_opacity[i] = go;
        if (p.dL_draw_rotations) p.dL_draw_rotations[i] = gr;
    }
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

static int activate_params_impl(int n, const float* raw_means, const float* raw_opacity, const float* raw_scales, const float* raw_rotations,
                                float* means3D, float* scales, float* rotations, float* opacities, void* stream) {
    if (n <= 0) return GSR_OK;
    if (!raw_means || !raw_opacity || !raw_scales || !raw_rotations || !means3D || !scales || !rotations || !opacities)
        return GSR_ERR_INVALID_ARG;
    // (every array but the two of one float per Gaussian is moved in 16-byte vectors)
    if (misaligned(raw_means, 16) || misaligned(raw_scales, 16) || misaligned(raw_rotations, 16) || misaligned(means3D, 16) ||
        misaligned(scales, 16) || misaligned(rotations, 16))
        return GSR_ERR_INVALID_ARG;
    const unsigned blocks = (unsigned)(((long long)n + 255) / 256);
    hipLaunchKernelGGL(activate_params_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, raw_means, raw_opacity,
                       raw_scales, reinterpret_cast<const float4*>(raw_rotations), reinterpret_cast<float4*>(means3D),
                       reinterpret_cast<float4*>(scales), reinterpret_cast<float4*>(rotations), opacities);
    GSR_LAUNCH_CHECK("activate_params_kernel");
    return GSR_OK;
}
int gsr_activate_params(int n, const float* raw_means, const float* raw_opacity, const float* raw_scales, const float* raw_rotations,
                        float* means3D, float* scales, float* rotations, float* opacities, void* stream) {
    return entry_point(activate_params_impl, n, raw_means, raw_opacity, raw_scales, raw_rotations, means3D, scales, rotations, opacities, stream);
}

static int activate_params_backward_impl(int n, const float* raw_opacity, const float* raw_scales, const float* raw_rotations, const int32_t* radii,
                                         const float* dL_dmeans3D, const float* dL_dscales, const float* dL_drotations, const float* dL_dconic_opacity,
                                         float* dL_draw_means, float* dL_draw_opacity, float* dL_draw_scales, float* dL_draw_rotations, void* stream) {
    if (n <= 0) return GSR_OK;
    // an output that is asked for needs what it is computed from; one that is not, nothing
    if (dL_draw_means && !dL_dmeans3D) return GSR_ERR_INVALID_ARG;
    if (dL_draw_opacity && (!raw_opacity || !dL_dconic_opacity)) return GSR_ERR_INVALID_ARG;
    if (dL_draw_scales && (!raw_scales || !dL_dscales)) return GSR_ERR_INVALID_ARG;
    if (dL_draw_rotations && (!raw_rotations || !dL_drotations)) return GSR_ERR_INVALID_ARG;
    if (!dL_draw_means && !dL_draw_opacity && !dL_draw_scales && !dL_draw_rotations) return GSR_OK;
    if ((dL_draw_means && (misaligned(dL_draw_means, 16) || misaligned(dL_dmeans3D, 16))) ||
        (dL_draw_opacity && misaligned(dL_dconic_opacity, 16)) ||
        (dL_draw_scales && (misaligned(dL_draw_scales, 16) || misaligned(raw_scales, 16) || misaligned(dL_dscales, 16))) ||
        (dL_draw_rotations && (misaligned(dL_draw_rotations, 16) || misaligned(raw_rotations, 16) || misaligned(dL_drotations, 16))))
        return GSR_ERR_INVALID_ARG;
    ActivateBackwardParams p;
    p.n = n;
    p.raw_opacity = raw_opacity;
    p.raw_scales = raw_scales;
    p.raw_rotations = reinterpret_cast<const float4*>(raw_rotations);
    p.radii = radii;
    p.dL_dmeans3D = reinterpret_cast<const float4*>(dL_dmeans3D);
    p.dL_dscales = reinterpret_cast<const float4*>(dL_dscales);
    p.dL_drotations = reinterpret_cast<const float4*>(dL_drotations);
    p.dL_dconic_opacity = reinterpret_cast<const float4*>(dL_dconic_opacity);
    p.dL_draw_means = dL_draw_means;
    p.dL_draw_opacity = dL_draw_opacity;
    p.dL_draw_scales = dL_draw_scales;
    p.dL_draw_rotations = reinterpret_cast<float4*>(dL_draw_rotations);
    const unsigned blocks = (unsigned)(((long long)n + 255) / 256);
    hipLaunchKernelGGL(activate_params_backward_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    GSR_LAUNCH_CHECK("activate_params_backward_kernel");
    return GSR_OK;
}
int gsr_activate_params_backward(int n, const float* raw_opacity, const float* raw_scales, const float* raw_rotations, const int32_t* radii,
                                 const float* dL_dmeans3D, const float* dL_dscales, const float* dL_drotations, const float* dL_dconic_opacity,
                                 float* dL_draw_means, float* dL_draw_opacity, float* dL_draw_scales, float* dL_draw_rotations, void* stream) {
    return entry_point(activate_params_backward_impl, n, raw_opacity, raw_scales, raw_rotations, radii, dL_dmeans3D, dL_dscales, dL_drotations,
                       dL_dconic_opacity, dL_draw_means, dL_draw_opacity, dL_draw_scales, dL_draw_rotations, stream);
}

}  // extern "C"
