// Upstream's build_rotation of an already normalised quaternion (r, x, y, z), in float32, one definition shared by the two
// kernels that move a position by a Gaussian's own covariance: densify_apply_kernel (densify.hip, the children of a split)
// and mcmc_noise_kernel (mcmc.hip). include/gsrast_amd.h states the nine entries; the operations and their order here are
// that text, so that both kernels — and tests/densify_ref.py's build_rotation — agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

struct Rotation3 {
    float m[3][3];
};

// q = activate_rotation(...): (r, x, y, z) in (q.x, q.y, q.z, q.w)
__device__ __forceinline__ Rotation3 rotation_matrix(const float4 q) {
    const float r = q.x, x = q.y, y = q.z, w = q.w;                          // w stands for z
    Rotation3 R;
    R.m[0][0] = 1.0f - 2.0f * (y * y + w * w); R.m[0][1] = 2.0f * (x * y - r * w); R.m[0][2] = 2.0f * (x * w + r * y);
    R.m[1][0] = 2.0f * (x * y + r * w); R.m[1][1] = 1.0f - 2.0f * (x * x + w * w); R.m[1][2] = 2.0f * (y * w - r * x);
    R.m[2][0] = 2.0f * (x * w - r * y); R.m[2][1] = 2.0f * (y * w + r * x); R.m[2][2] = 1.0f - 2.0f * (x * x + y * y);
    return R;
}

// R d, each row summed as (Ra0 d0 + Ra1 d1) + Ra2 d2
__device__ __forceinline__ void rotate(const Rotation3& R, const float (&d)[3], float (&out)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = (R.m[a][0] * d[0] + R.m[a][1] * d[1]) + R.m[a][2] * d[2];
}

// R^T v, each entry summed as (R0j v0 + R1j v1) + R2j v2
__device__ __forceinline__ void rotate_transposed(const Rotation3& R, const float (&v)[3], float (&out)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = (R.m[0][j] * v[0] + R.m[1][j] * v[1]) + R.m[2][j] * v[2];
}

}  // namespace gsr
