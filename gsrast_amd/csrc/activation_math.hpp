// The activations of SplatData::loadFromPly (apps/gsrast/SplatData.cpp:8-11,28-66) in float32, one function per output,
// shared by the two kernels that apply them: ply_activate_kernel (ply.hip, from the 62-float file record) and
// activate_params_kernel (activations.hip, from a trainer's raw parameter arrays). One definition, so that the two
// agree bit for bit: same operations, same order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace gsr {

__device__ __forceinline__ float4 activate_scale(float s0, float s1, float s2) {
    return make_float4(expf(s0), expf(s1), expf(s2), expf(1.0f));
}

// real part first; the norm as glm::dot(vec4) sums it, the reciprocal as glm::inversesqrt forms it
__device__ __forceinline__ float4 activate_rotation(float q0, float q1, float q2, float q3) {
    const float d = (q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3);
    const float inv = 1.0f / sqrtf(d);
    return make_float4(q0 * inv, q1 * inv, q2 * inv, q3 * inv);
}

__device__ __forceinline__ float activate_opacity(float x) {
    return 1.0f / (1.0f + expf(-x));                                         // sigmoid, SplatData.cpp:8-11
}

}  // namespace gsr
