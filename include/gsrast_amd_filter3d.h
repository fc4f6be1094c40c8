/* gsrast_amd_filter3d.h — the 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024): the per-Gaussian sampling rate over the
 * training cameras, the smoothing of scales and opacities by it, and the smoothing's gradient (an addition to gsrast_amd.h).
 *
 * The antialiased mode (gsrast_amd_antialias.h) is the 2D half of Mip-Splatting: it keeps a splat's weight when the scene is seen
 * from further away than it was trained. The 3D filter is the other half: it bounds every Gaussian's size from below by the finest
 * sampling rate any training camera saw it at, so that no Gaussian becomes thinner than a training pixel and a viewer that moves
 * closer sees no erosion or speckle. Per Gaussian i it is one float, filter[i], made in two steps —
 *     gsr_filter3d_observe    min_depth[i] = the nearest view-space depth at which a camera of a batch sees Gaussian i
 *     gsr_filter3d_finalize   filter[i] = (min_depth[i] / max_focal) * sqrt(0.2)
 * every 100 training steps and after each densification, as upstream's compute_3D_filter, and used in every step:
 *     gsr_filter3d_forward    s'_j = sqrt(s_j^2 + filter^2), o' = o * sqrt(prod_j s_j^2 / s'_j^2)
 *     gsr_filter3d_backward   its gradient
 * between the activation kernels and gsr_forward (in front of gsr_antialias_forward, which then sees s' and o').
 *
 * All arithmetic below is float32, no fused multiply-add, IEEE division and square root, unless said otherwise; min / max are glm's:
 * min(a, b) = (b < a) ? b : a, max(a, b) = (a < b) ? b : a.
 *
 * gsr_filter3d_observe. positions: num_gaussians rows of position_stride floats (3: raw xyz rows; 4: means3D rows), of which
 * (x, y, z) are the first three. cameras: num_cameras records of GSR_FILTER3D_CAMERA_FLOATS = 20 floats on the device:
 *     [0..11]   V(0,0) V(0,1) V(0,2) V(0,3)  V(1,0) .. V(1,3)  V(2,0) .. V(2,3): the three rows of the view matrix that produce t_0,
 *               t_1, t_2; V(r, c) = view_matrix[4 c + r] of gsr_forward_args.view_matrix, row 2 already negated: t_2 > 0 is in front
 *     [12] f_x  [13] f_y                                      focal lengths in pixels
 *     [14] c_x = W / 2   [15] c_y = H / 2
 *     [16] x_lo = -0.15 W  [17] x_hi = 1.15 W  [18] y_lo = -0.15 H  [19] y_hi = 1.15 H
 *               (each formed on the host in double and rounded to float32 once: what torch does with upstream's Python scalars)
 * Per pair (Gaussian i, camera k):
 *     t_r = ((V(r,0) x + V(r,1) y) + V(r,2) z) + V(r,3)                       r = 0, 1, 2  (the upstream profile's order)
 *     zc  = max(t_2, 0.001f)
 *     px  = (t_0 / zc) * f_x + c_x
 *     py  = (t_1 / zc) * f_y + c_y
 *     VALID iff t_2 > 0.2f and px >= x_lo and px <= x_hi and py >= y_lo and py <= y_hi    (a NaN anywhere: not VALID)
 * and min_depth[i] = min(min_depth[i], t_2 of every VALID pair). min_depth is READ AND WRITTEN: the caller fills it with +inf
 * before the first batch (it must hold +inf or positive floats), and "never seen" is min_depth[i] == +inf. A minimum over positive
 * floats is exact and commutative: the result is the same bits for any batching, any order of the cameras, and across repeated
 * calls; one call over the cameras A and B equals a call over A followed by a call over B. One Gaussian per lane; the cameras are
 * dealt to workgroups in chunks of GSR_FILTER3D_CAMERA_CHUNK; each lane ends with at most one integer atomic minimum on the bit
 * pattern of its min_depth (VALID depths are above 0.2: positive floats order as their bits do, +inf last), and with none where it
 * found nothing nearer than what it loaded. No float atomics, nothing crosses lanes. num_cameras == 0 writes nothing.
 *
 * gsr_filter3d_finalize. d_max = the largest min_depth[i] that is < +inf (found on the device: a wave reduction, then one integer
 * atomic maximum per wave into a word of `temp` that the call clears; exact and order-free), +0 if there is none.
 *     d         = (min_depth[i] < +inf) ? min_depth[i] : d_max
 *     filter[i] = (d / max_focal) * K          K = 0x3EE4F92E = 0.4472135901451111, the float32 nearest to the double 0.2 ** 0.5
 * max_focal: the largest f_x over all cameras observed, computed by the caller as upstream does. If no Gaussian was seen, every
 * filter[i] is +0 (upstream raises there), which gsr_filter3d_forward treats as "no filter". temp: gsr_filter3d_temp_bytes(N)
 * bytes of device memory, 16-byte aligned, contents irrelevant. One 4-byte clear and two kernel launches; nothing is read back.
 *
 * gsr_filter3d_forward. For Gaussian i with scales s = scales[i] (four floats), opacity o and f = filter[i]:
 *     f2   = f * f
 *     q_j  = s_j * s_j;  a_j = q_j + f2;  s'_j = sqrtf(a_j);  r_j = q_j / a_j          j = 0, 1, 2
 *     coef = sqrtf((r_0 * r_1) * r_2)
 *     o'   = o * coef
 * scales_out[i] = (s'_0, s'_1, s'_2, s_3): the activation kernel's fourth float travels unchanged. opacities_out[i] = o'.
 * IDENTITY is the case !(f2 > 0.0f) — a zero filter, one whose square underflows to zero, a NaN: both outputs are the inputs bit
 * for bit, and the gradient passes through unchanged. Either output may be NULL (not both); no output may alias an input.
 *
 * gsr_filter3d_backward, with g_s = dL_dscales_out[i] and g_o = dL_dopacities_out[i] (a NULL one counts as zeros; at least one
 * must be given):
 *     dL_dopacities[i] = coef * g_o                       (one float32 product of the forward's coef; g_o under IDENTITY)
 *     dL_dscales[i][j] = g_s[j] * s_j / s'_j + (o * g_o) * sign(s_j) * f2 / (a_j * sqrt(a_j)) * prod_{k != j} u_k,
 *                        u_k = |s_k| / sqrt(a_k), sign(0) = 0                                  (g_s[j] under IDENTITY)
 *     dL_dscales[i][3] = 0
 * The IDENTITY decision is the float32 forward's; the chain itself is evaluated in float64 from the float32 inputs (f2 = f * f in
 * double too), like gsr_antialias_backward's and gsr_backward's, and each result is rounded to float32 once. Where a_j is +inf (an
 * infinite filter) the factor f2 / (a_j * sqrt(a_j)) is taken as 0, its limit. The filter is a constant (upstream's no_grad
 * buffer): it gets no gradient. Outputs are WRITTEN, not accumulated, for every i < num_gaussians; a NULL output is not computed;
 * at least one must be given. When radii != NULL and radii[i] <= 0 the row gets +0 in every output and nothing else of it is
 * loaded. One Gaussian per lane; rows move in 16-byte vectors.
 *
 * What is upstream's (Mip-Splatting, scene/gaussian_model.py): the validity test with its 0.2 near plane and 15 % screen margin,
 * the 0.001 clamp, the minimum over cameras, the fill of unseen Gaussians with the largest seen depth, the factor sqrt(0.2) over the
 * largest focal length, and s' and o' as get_scaling_with_3D_filter / get_opacity_with_3D_filter define them.
 * What is NOT upstream's: "never seen" is +inf in min_depth (upstream: a cap of 100000 and a flag array); coef is the product of
 * the three ratios r_j, each in [0, 1], not sqrt(det1 / det2) of the two products — scales of 1e9 or 1e-20 then neither overflow
 * nor underflow into NaN; the IDENTITY rule; the empty case above; and the screen-space dilation stays 0.3 (Mip-Splatting's own
 * rasterizer uses 0.1).
 *
 * Every call is asynchronous on `stream`, allocates nothing, synchronises nothing; two calls on the same inputs agree bit for bit.
 * num_gaussians == 0 returns GSR_OK and writes nothing.
 *
 * GSR_ERR_INVALID_ARG, decided before any HIP call: args NULL or a struct_size other than this header's; any non-zero flag;
 * num_gaussians or num_cameras < 0; a position_stride other than 3 or 4; a NULL positions, min_depth, filter, scales or opacities
 * (where the call takes it), a NULL cameras with num_cameras > 0, a NULL temp; both dL_dscales_out and dL_dopacities_out NULL; every
 * output NULL; an output that is also an input of the same call; a max_focal that is not finite or not positive; a vec4 array
 * (scales, scales_out, dL_dscales_out, dL_dscales) or temp off a 16-byte boundary; temp_bytes below gsr_filter3d_temp_bytes.
 * GSR_ERR_TOO_LARGE: more cameras than 65535 chunks. Codes are returned and recorded as by every entry point of gsrast_amd.h. */
#ifndef GSRAST_AMD_FILTER3D_H
#define GSRAST_AMD_FILTER3D_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_FILTER3D_CAMERA_FLOATS 20
#define GSR_FILTER3D_CAMERA_CHUNK 64

typedef struct gsr_filter3d_observe_args {
    uint32_t struct_size;          /* sizeof(gsr_filter3d_observe_args) */
    uint32_t flags;                /* 0 */
    int32_t num_gaussians;
    int32_t position_stride;       /* 3 or 4 floats per row */
    int32_t num_cameras;
    const float* positions;        /* float[N][position_stride] */
    const float* cameras;          /* float[num_cameras][20], device */
    float* min_depth;              /* float[N], read and written */
    void* stream;                  /* hipStream_t */
} gsr_filter3d_observe_args;

typedef struct gsr_filter3d_finalize_args {
    uint32_t struct_size;          /* sizeof(gsr_filter3d_finalize_args) */
    uint32_t flags;                /* 0 */
    int32_t num_gaussians;
    float max_focal;               /* the largest f_x over all cameras */
    const float* min_depth;        /* float[N] */
    float* filter;                 /* float[N] */
    void* temp;                    /* gsr_filter3d_temp_bytes(N) bytes, 16-byte aligned */
    size_t temp_bytes;
    void* stream;
} gsr_filter3d_finalize_args;

typedef struct gsr_filter3d_args {
    uint32_t struct_size;          /* sizeof(gsr_filter3d_args) */
    uint32_t flags;                /* 0 */
    int32_t num_gaussians;
    const float* scales;           /* vec4[N] */
    const float* opacities;        /* float[N] */
    const float* filter;           /* float[N] */
    float* scales_out;             /* vec4[N] or NULL */
    float* opacities_out;          /* float[N] or NULL (at least one of the two) */
    void* stream;
} gsr_filter3d_args;

typedef struct gsr_filter3d_backward_args {
    uint32_t struct_size;          /* sizeof(gsr_filter3d_backward_args) */
    uint32_t flags;                /* 0 */
    int32_t num_gaussians;
    const float* scales;           /* vec4[N]: the forward call's inputs */
    const float* opacities;        /* float[N] */
    const float* filter;           /* float[N] */
    const float* dL_dscales_out;   /* vec4[N] or NULL: dL/ds' */
    const float* dL_dopacities_out; /* float[N] or NULL: dL/do' (at least one of the two) */
    const int32_t* radii;          /* i32[N] or NULL: the frame's radii */
    float* dL_dscales;             /* vec4[N] or NULL */
    float* dL_dopacities;          /* float[N] or NULL (at least one of the two) */
    void* stream;
} gsr_filter3d_backward_args;

size_t gsr_filter3d_temp_bytes(int32_t num_gaussians);      /* 0 for a negative count */
int gsr_filter3d_observe(gsr_filter3d_observe_args* args);
int gsr_filter3d_finalize(gsr_filter3d_finalize_args* args);
int gsr_filter3d_forward(gsr_filter3d_args* args);
int gsr_filter3d_backward(gsr_filter3d_backward_args* args);

#ifdef __cplusplus
}
#endif
#endif
