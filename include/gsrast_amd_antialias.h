/* gsrast_amd_antialias.h — antialiased splatting: the opacity compensation as its own pass (an addition to gsrast_amd.h).
 *
 * Both preprocess kernels dilate the projected covariance by 0.3 on its diagonal (the screen-space low-pass filter) and use the
 * opacity unchanged: a splat smaller than a pixel is spread over the pixel at full opacity. The antialiased mode (upstream's
 * `antialiasing`, gsplat's rasterize_mode="antialiased", the 2D filter of Mip-Splatting) scales each opacity by
 *     c = sqrt(det(cov2D) / det(cov2D + 0.3 I))
 * so that the dilation keeps the splat's total weight. In gsr_forward the opacity decides nothing before the blend — radius,
 * rectangle, tiles, depth order and lists come from the dilated covariance alone, the opacity is copied into conic_opacity.w —
 * so an antialiased frame is gsr_forward handed o' = o * c, and its backward is gsr_backward, whose dL_dconic_opacity[:, 3] is
 * then dL/do', followed by gsr_antialias_backward. Mip-Splatting's 3D smoothing filter is a pass of its own in front of this one
 * (gsrast_amd_filter3d.h), whose scales and opacities are then this call's inputs. Not in here: cov3D_precomp inputs, and the
 * gradient of c with respect to the camera — the view and projection matrices are READ, NOT DIFFERENTIATED.
 *
 * The quantity, operation by operation. float32, no fused multiply-add, IEEE division and square root, unless said otherwise;
 * min / max are glm's: min(a, b) = (b < a) ? b : a, max(a, b) = (a < b) ? b : a; products of 3 x 3 matrices add their three
 * terms left to right: (A B)[r][c] = (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c]. V = view_matrix and Pm = proj_matrix,
 * column-major: V(r, c) = V[4 c + r]. W is the 3 x 3 matrix W[r][c] = V(r, c). For Gaussian i with mean m = (mx, my, mz, mw),
 * scale s, rotation q (four floats each), k = scale_modifier:
 *
 * The reference profile (flags without GSR_FLAG_SEMANTICS_INRIA), as csrc/preprocess.hip:
 *     h_r  = (Pm(r,0) mx + Pm(r,1) my) + (Pm(r,2) mz + Pm(r,3) mw)            r = 0, 1, 2, 3
 *     iw   = 1 / (0.001f + h_3);  p = (iw h_0, iw h_1, iw h_2)
 *     CULLED iff p.z < 0 or p.z > 1 or p.x < -1.3f or p.x > 1.3f or p.y < -1.3f or p.y > 1.3f
 *     dq   = (q0 q0 + q1 q1) + (q2 q2 + q3 q3);  inv = 1 / sqrtf(dq);  (x, y, z, w) = (q0 inv, q1 inv, q2 inv, q3 inv)
 *     R    = | D(x x + y y)   E(y z - x w)   E(y w + x z) |      D(u) = (float)(2.0 * (double)u - 1.0)
 *            | E(y z + x w)   D(x x + z z)   E(z w - x y) |      E(u) = (float)(2.0 * (double)u)
 *            | E(y w - x z)   E(z w + x y)   D(x x + w w) |      (u itself is formed in float32)
 *     M    = R diag(k s0, k s1, k s2);  Sigma = M M^T
 *     t_r  = (V(r,0) mx + V(r,1) my) + (V(r,2) mz + V(r,3) 1.0f)             r = 0, 1, 2
 *     f_x = f_y = (float)height / (2.0f * tan_fovy)
 * The upstream profile (GSR_FLAG_SEMANTICS_INRIA), as csrc/preprocess_inria.hip:
 *     t_r  = ((V(r,0) mx + V(r,1) my) + V(r,2) mz) + V(r,3)                  r = 0, 1, 2
 *     CULLED iff t_2 <= 0.2f
 *     (r, x, y, z) = q, not normalised
 *     R    = | 1 - 2 (y y + z z)   2 (x y - r z)       2 (x z + r y)     |
 *            | 2 (x y + r z)       1 - 2 (x x + z z)   2 (y z - r x)     |
 *            | 2 (x z - r y)       2 (y z + r x)       1 - 2 (x x + y y) |
 *     M    = diag(k s0, k s1, k s2) R^T;  Sigma = M^T M
 *     f_x = (float)width / (2.0f * tan_fovx);  f_y = (float)height / (2.0f * tan_fovy)
 * Both profiles, from there:
 *     lx = 1.3f * tan_fovx;  ly = 1.3f * tan_fovy
 *     ux = min(lx, max(-lx, t_0 / t_2)) * t_2;  uy = min(ly, max(-ly, t_1 / t_2)) * t_2;  z = t_2
 *     J  = | f_x / z   0         (-f_x * ux) / (z * z) |        (upstream profile: -(f_x * ux) / (z * z), the same bits)
 *          | 0         f_y / z   (-f_y * uy) / (z * z) |
 *          | 0         0         0                     |
 *     T  = J W  (the zero entries of J are multiplied and added like the others);  cv = (T Sigma) T^T
 *     a0 = cv[0][0], b = cv[1][0], c0 = cv[1][1]             (row 1, column 0: the entry the preprocess kernels read)
 *     d0 = a0 * c0 - b * b
 *     ca = a0 + 0.3f, cc = c0 + 0.3f
 *     d1 = ca * cc - b * b                                   (bit for bit the forward call's `det`)
 *     r  = d0 / d1
 *     c  = sqrtf(max(0.000025f, r))                          (a NaN r gives the floor; 0.000025 is upstream's)
 *     o' = o * c
 * c = 1.0f exactly, o' = o bit for bit, and the gradient through c is zero, where the Gaussian is CULLED (the profile's
 * preprocess computes no covariance for it) or d1 is zero or not finite.
 *
 * gsr_antialias_forward writes compensation[i] = c and opacities_out[i] = o' for every i < num_gaussians; either output may be
 * NULL (not both). opacities_out must not alias opacities.
 *
 * gsr_antialias_backward, with g = dL_dopacities_out[i]:
 *     dL_dopacities[i] = c * g                               (one float32 product of the c above)
 * and G = o * g goes through c to the mean, the scales and the rotation: nothing where the floor is active, !(0.000025f < r),
 * or c = 1 by the rule above; otherwise dL/dr = G / (2 c), from r to (a0, b, c0), through cv = T Sigma T^T to Sigma and to t (J
 * depends on t; where t_0 / t_2 (t_1 / t_2) was clamped, t_0 (t_1) receives nothing and t_2 receives the clamped ratio's share,
 * exactly as gsr_backward's chain cuts them), from Sigma to s and q (the reference profile through the normalisation of q too), from t to
 * (mx, my, mz) through W. The DECISIONS — the cull, the test of d1, the floor and the two clamps — are the float32 forward's above; the
 * chain itself is evaluated in float64 from the float32 inputs, like gsr_backward's, and each result is rounded to float32 once.
 * dL_dmeans3D, dL_dscales and dL_drotations are [N][4] with the fourth float of the first two written as 0; every output is
 * WRITTEN, not accumulated, for every i < num_gaussians; a NULL output is not computed; at least one must be given.
 * A row gets +0 in every output, and nothing else of it is loaded, when radii != NULL and radii[i] <= 0, or when g == 0.0f.
 *
 * Both calls are asynchronous on `stream`, allocate nothing, synchronise nothing; one Gaussian per lane, no sum crosses lanes:
 * two calls on the same inputs agree bit for bit. num_gaussians == 0 returns GSR_OK and writes nothing.
 *
 * GSR_ERR_INVALID_ARG, decided before any HIP call: args NULL or a struct_size other than this header's; a flag other than
 * GSR_FLAG_SEMANTICS_INRIA; num_gaussians < 0; width or height <= 0; tan_fovx, tan_fovy or scale_modifier not finite or not
 * positive; a NULL means3D, scales, rotations, opacities or view_matrix; a NULL proj_matrix under the reference profile (the
 * upstream profile does not read it); a NULL dL_dopacities_out; every output NULL; opacities_out == opacities; an input or
 * output row array off a 16-byte boundary. Codes are returned and recorded as by every entry point of gsrast_amd.h. */
#ifndef GSRAST_AMD_ANTIALIAS_H
#define GSRAST_AMD_ANTIALIAS_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_antialias_args {
    uint32_t struct_size;          /* sizeof(gsr_antialias_args) */
    uint32_t flags;                /* GSR_FLAG_SEMANTICS_INRIA as the forward call's */
    int32_t num_gaussians, width, height;
    float tan_fovx, tan_fovy, scale_modifier;
    const float* means3D;          /* vec4[N] */
    const float* scales;           /* vec4[N] */
    const float* rotations;        /* vec4[N] */
    const float* opacities;        /* float[N] */
    const float* view_matrix;      /* 16 floats, device, column-major, as gsr_forward_args.view_matrix */
    const float* proj_matrix;      /* 16 floats, device, as gsr_forward_args.proj_matrix: the reference profile's cull; NULL allowed with GSR_FLAG_SEMANTICS_INRIA */
    float* opacities_out;          /* float[N] or NULL */
    float* compensation;           /* float[N] or NULL (at least one of the two) */
    void* stream;                  /* hipStream_t */
} gsr_antialias_args;

typedef struct gsr_antialias_backward_args {
    uint32_t struct_size;          /* sizeof(gsr_antialias_backward_args) */
    uint32_t flags;
    int32_t num_gaussians, width, height;
    float tan_fovx, tan_fovy, scale_modifier;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* opacities;
    const float* view_matrix;
    const float* proj_matrix;
    const float* dL_dopacities_out; /* float[N]: dL/do' */
    const int32_t* radii;          /* i32[N] or NULL: the frame's radii */
    float* dL_dopacities;          /* float[N] or NULL */
    float* dL_dmeans3D;            /* vec4[N] or NULL */
    float* dL_dscales;             /* vec4[N] or NULL */
    float* dL_drotations;          /* vec4[N] or NULL (at least one of the four) */
    void* stream;
} gsr_antialias_backward_args;

int gsr_antialias_forward(gsr_antialias_args* args);
int gsr_antialias_backward(gsr_antialias_backward_args* args);

#ifdef __cplusplus
}
#endif
#endif
