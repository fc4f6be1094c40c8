/* gsrast_amd_normals.h — the two operators of the normal-consistency loss (an addition to gsrast_amd.h): the per-Gaussian normal,
 * and the normal of a rendered depth surface.
 *
 * 2DGS, GOF, RaDe-GS and PGSR pair the depth distortion loss (gsrast_amd_distortion.h) with L_n = mean_p (1 - N_r(p) . N_d(p)):
 * N_r is the alpha-blended map of per-Gaussian normals — gsr_gaussian_normals_forward's output composited by gsr_features_forward
 * as three channels — and N_d is the normal of the surface the rendered depth describes, gsr_depth_normals_forward of the expected
 * depth, scaled by the accumulated opacity. A 3D Gaussian has no normal of its own: as in GOF and PGSR it is the direction of its
 * SHORTEST axis, turned towards the camera. Not in here: the normal is not differentiated with respect to the scales (which
 * axis is shortest is a decision), the mean or the camera (they decide the flip, and W is read, not differentiated); the depth
 * normal is not differentiated with respect to tan_fovx / tan_fovy.
 *
 * The quantities, operation by operation. float32, no fused multiply-add, IEEE division and square root, unless said otherwise.
 * V = view_matrix, column-major: V(r, c) = V[4 c + r]. W is the 3 x 3 matrix W[r][c] = V(r, c).
 *
 * ---- gsr_gaussian_normals_forward. For Gaussian i with mean m = (mx, my, mz, mw), scale s, rotation q (four floats each; the
 * fourth float of m and of s is not read):
 * The reference profile (flags without GSR_FLAG_SEMANTICS_INRIA), as csrc/preprocess.hip and gsrast_amd_antialias.h:
 *     dq   = (q0 q0 + q1 q1) + (q2 q2 + q3 q3);  inv = 1 / sqrtf(dq);  (x, y, z, w) = (q0 inv, q1 inv, q2 inv, q3 inv)
 *     R    = | D(x x + y y)   E(y z - x w)   E(y w + x z) |      D(u) = (float)(2.0 * (double)u - 1.0)
 *            | E(y z + x w)   D(x x + z z)   E(z w - x y) |      E(u) = (float)(2.0 * (double)u)
 *            | E(y w - x z)   E(z w + x y)   D(x x + w w) |      (u itself is formed in float32)
 *     t_r  = (V(r,0) mx + V(r,1) my) + (V(r,2) mz + V(r,3) 1.0f)             r = 0, 1, 2
 * The upstream profile (GSR_FLAG_SEMANTICS_INRIA), as csrc/preprocess_inria.hip:
 *     (r, x, y, z) = q, not normalised
 *     R    = | 1 - 2 (y y + z z)   2 (x y - r z)       2 (x z + r y)     |
 *            | 2 (x y + r z)       1 - 2 (x x + z z)   2 (y z - r x)     |
 *            | 2 (x z - r y)       2 (y z + r x)       1 - 2 (x x + y y) |
 *     t_r  = ((V(r,0) mx + V(r,1) my) + V(r,2) mz) + V(r,3)                  r = 0, 1, 2
 * In both the covariance the profile's preprocess draws is Sigma = R diag(s^2) R^T: column j of R is the axis of scale s_j.
 * Both profiles, from there:
 *     a    = 0;  if (s1 < s[a]) a = 1;  if (s2 < s[a]) a = 2          (the shortest axis; ties and NaNs keep the lower index)
 *     n_w  = (R[0][a], R[1][a], R[2][a])                                (column a of R)
 *     n_v[r] = (W[r][0] n_w[0] + W[r][1] n_w[1]) + W[r][2] n_w[2]       r = 0, 1, 2
 *     d    = (n_v[0] t_0 + n_v[1] t_1) + n_v[2] t_2
 *     if (d > 0) n_v = -n_v                                             (towards the camera: a view matrix of determinant -1, as
 *                                                                        the reference's caller hands over, changes nothing here)
 *     l    = sqrtf((n_v[0] n_v[0] + n_v[1] n_v[1]) + n_v[2] n_v[2])
 *     normals[i] = (n_v[0] / l, n_v[1] / l, n_v[2] / l)
 * normals[i] = (+0, +0, +0), and the backward gives row i no gradient, where l is zero or not finite.
 * normals is float[N][3], tightly packed: a `features` argument of gsr_features_forward with channels = 3 as it stands.
 *
 * gsr_gaussian_normals_backward, with g = dL_dnormals[i] (three floats): the DECISIONS — a, the flip, the test of l — are the
 * float32 forward's above. The chain is evaluated in float64 from the float32 inputs and each result is rounded to float32 once:
 * R in double without the D / E roundings (the reference profile with x, y, z, w = q / |q| in double), sigma = -1 where the
 * forward flipped and +1 elsewhere, n_v = sigma W n_w, u = n_v / |n_v|, dL/dn_v = (g - u (u . g)) / |n_v|, dL/dn_w = sigma W^T
 * dL/dn_v, which is dL/dR's column a (its other columns are zero), from R to q — under the reference profile through the
 * normalisation of q too. Nothing goes to the scales, the mean or the camera. dL_drotations is vec4[N], WRITTEN, not accumulated,
 * for every i < num_gaussians. A row gets +0 in all four floats, and nothing else of it is loaded, when radii != NULL and
 * radii[i] <= 0, or when its three incoming floats all compare equal to 0.0f; it gets +0 too where the forward wrote zeros.
 *
 * ---- gsr_depth_normals_forward. depth is float[height][width]: a view-space z per pixel (the expected depth of a frame, say).
 * With Wf = (float)width, Hf = (float)height, for integer pixel coordinates:
 *     the reference profile:   ndc_x(x) = (2.0f * (float)x) / Wf - 1.0f           ndc_y(y) = (2.0f * (float)y) / Hf - 1.0f
 *                              (csrc/preprocess.hip places NDC p at pixel (p 0.5 + 0.5) W)
 *     the upstream profile:    ndc_x(x) = (2.0f * (float)x + 1.0f) / Wf - 1.0f    ndc_y(y) = (2.0f * (float)y + 1.0f) / Hf - 1.0f
 *                              (csrc/preprocess_inria.hip places it at ((p + 1) W - 1) / 2)
 *     rx(x) = ndc_x(x) * tan_fovx;  ry(y) = ndc_y(y) * tan_fovy;  the point of pixel (x, y) is P(x, y) = (rx D, ry D, D)
 * For an interior pixel, 1 <= x <= width - 2 and 1 <= y <= height - 2, with the four neighbour depths
 * Du = depth[y-1][x], Dl = depth[y][x-1], Dr = depth[y][x+1], Dd = depth[y+1][x]:
 *     dv = P(x, y+1) - P(x, y-1) = (rx(x) Dd - rx(x) Du,      ry(y+1) Dd - ry(y-1) Du,   Dd - Du)
 *     dh = P(x+1, y) - P(x-1, y) = (rx(x+1) Dr - rx(x-1) Dl,  ry(y) Dr - ry(y) Dl,       Dr - Dl)
 *     c  = dv x dh = (dv.y dh.z - dv.z dh.y,   dv.z dh.x - dv.x dh.z,   dv.x dh.y - dv.y dh.x)
 *     if ((c.x rx(x) + c.y ry(y)) + c.z > 0) c = -c                      (towards the camera; with four positive depths the sum
 *                                                                         is negative in exact arithmetic: this guards the rounding)
 *     l  = sqrtf((c.x c.x + c.y c.y) + c.z c.z)
 *     normals[0][y][x] = c.x / l;  normals[1][y][x] = c.y / l;  normals[2][y][x] = c.z / l
 * normals is float[3][height][width], planar like a feature map; every element is written. The three planes are +0 on the one-pixel
 * border; where any of Du, Dl, Dr, Dd is not finite or not > 0; where l is zero or not finite. depth[y][x] itself is not read
 * for pixel (x, y). A constant depth gives exactly (0, 0, -1) on every interior pixel. width or height below 3 is valid: there is
 * no interior pixel, every element is +0.
 *
 * gsr_depth_normals_backward: dL_ddepth[p], for every pixel p, is the sum over the up to four neighbours q of p — in the fixed
 * order up (x, y-1), left (x-1, y), right (x+1, y), down (x, y+1) — whose normal is valid (interior, its four depths finite and
 * > 0, its l nonzero and finite: the float32 forward's decisions, its flip too) of  dn(q)/dD(p) . g(q),  g(q) = dL_dnormals[:][q].
 * Each term is evaluated in float64 from the float32 depths: the rays as above with every operation in double from the integer
 * coordinates, (double)Wf, (double)Hf, (double)tan_fovx and (double)tan_fovy; dv, dh, c in double; sigma = -1 where the forward
 * flipped; u = c / |c|; dL/dc = sigma (g - u (u . g)) / |c|; dL/ddv = dh x dL/dc; dL/ddh = dL/dc x dv; and p's share of it:
 *     q is up of p    (p is q's Dd):   dL/ddv . (rx(x), ry(y_q + 1), 1)
 *     q is left of p  (p is q's Dr):   dL/ddh . (rx(x_q + 1), ry(y), 1)
 *     q is right of p (p is q's Dl):  -dL/ddh . (rx(x_q - 1), ry(y), 1)
 *     q is down of p  (p is q's Du):  -dL/ddv . (rx(x), ry(y_q - 1), 1)
 * A neighbour that is not valid contributes 0.0. The four terms are added in double, ((up + left) + right) + down, and the sum
 * is rounded to float32 once. A gather: no atomics, two calls on the same inputs agree bit for bit. Every element of dL_ddepth
 * is written.
 *
 * All four calls are asynchronous on `stream`, allocate nothing, synchronise nothing; one Gaussian (one pixel) per lane, no sum
 * crosses lanes. num_gaussians == 0 returns GSR_OK and writes nothing.
 *
 * GSR_ERR_INVALID_ARG, decided before any HIP call: args NULL or a struct_size other than this header's; a flag other than
 * GSR_FLAG_SEMANTICS_INRIA. The Gaussian calls: num_gaussians < 0; a NULL means3D, scales, rotations or view_matrix; a NULL
 * normals (forward); a NULL dL_dnormals or dL_drotations (backward); means3D, scales, rotations or dL_drotations off a 16-byte
 * boundary. The depth calls: width or height <= 0; tan_fovx or tan_fovy not finite or not positive; a NULL depth; a NULL normals,
 * or normals == depth (forward); a NULL dL_dnormals or dL_ddepth, or dL_ddepth == depth or == dL_dnormals (backward).
 * GSR_ERR_TOO_LARGE, likewise: an image of more than 2^31 - 1 blocks of 64 x 4 pixels. Codes are returned and recorded as by
 * every entry point of gsrast_amd.h. */
#ifndef GSRAST_AMD_NORMALS_H
#define GSRAST_AMD_NORMALS_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_gaussian_normals_args {
    uint32_t struct_size;          /* sizeof(gsr_gaussian_normals_args) */
    uint32_t flags;                /* GSR_FLAG_SEMANTICS_INRIA as the forward call's */
    int32_t num_gaussians;
    const float* means3D;          /* vec4[N] */
    const float* scales;           /* vec4[N] */
    const float* rotations;        /* vec4[N] */
    const float* view_matrix;      /* 16 floats, device, column-major, as gsr_forward_args.view_matrix */
    float* normals;                /* float[N][3] */
    void* stream;                  /* hipStream_t */
} gsr_gaussian_normals_args;

typedef struct gsr_gaussian_normals_backward_args {
    uint32_t struct_size;          /* sizeof(gsr_gaussian_normals_backward_args) */
    uint32_t flags;
    int32_t num_gaussians;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* view_matrix;
    const float* dL_dnormals;      /* float[N][3] */
    const int32_t* radii;          /* i32[N] or NULL: the frame's radii */
    float* dL_drotations;          /* vec4[N] */
    void* stream;
} gsr_gaussian_normals_backward_args;

typedef struct gsr_depth_normals_args {
    uint32_t struct_size;          /* sizeof(gsr_depth_normals_args) */
    uint32_t flags;                /* GSR_FLAG_SEMANTICS_INRIA: the profile's pixel-centre convention */
    int32_t width, height;
    float tan_fovx, tan_fovy;
    const float* depth;            /* float[H][W] */
    float* normals;                /* float[3][H][W] */
    void* stream;
} gsr_depth_normals_args;

typedef struct gsr_depth_normals_backward_args {
    uint32_t struct_size;          /* sizeof(gsr_depth_normals_backward_args) */
    uint32_t flags;
    int32_t width, height;
    float tan_fovx, tan_fovy;
    const float* depth;            /* float[H][W] */
    const float* dL_dnormals;      /* float[3][H][W] */
    float* dL_ddepth;              /* float[H][W] */
    void* stream;
} gsr_depth_normals_backward_args;

int gsr_gaussian_normals_forward(gsr_gaussian_normals_args* args);
int gsr_gaussian_normals_backward(gsr_gaussian_normals_backward_args* args);
int gsr_depth_normals_forward(gsr_depth_normals_args* args);
int gsr_depth_normals_backward(gsr_depth_normals_backward_args* args);

#ifdef __cplusplus
}
#endif
#endif
