/* gsrast_amd_absgrad.h — the absolute screen-space gradient of a frame (AbsGS, Ye et al. 2024; `absgrad` in gsplat), an
 * addition to gsrast_amd.h.
 *
 * gsr_backward's dL_dmean2D is, per Gaussian, a SIGNED sum over pixels: a large blurry splat that straddles fine detail is pulled
 * one way by half of its pixels and the other way by the rest, the sum cancels, and adaptive density control never splits it.
 * AbsGS ranks by the sum of the absolute values of the pixels' shares instead, per axis. That quantity exists only inside the
 * render backward's per-pixel walk. gsr_absgrad is one more back-to-front walk over the sorted lists a gsr_forward call left, with
 * the seeds a gsr_backward / gsr_backward_alpha of the same frame takes, that keeps these two sums and nothing else. Nothing of
 * the forward call is written: the three chunks are read only, and a gsr_backward of the same receipt may run before or after it.
 *
 * The quantity, operation by operation. L is the scalar that gsr_backward / gsr_backward_alpha differentiates:
 *     L = sum(dL_dout_color * out_color) [+ sum(dL_dout_depth * out_depth)] [+ sum(dL_dout_alpha * (1 - final_t))]
 * the second term when backward->dL_dout_depth is given, the third when dL_dout_alpha is. For pixel p = (x, y) of tile t, with
 * g = dL_dout_color[:, p], g_d = dL_dout_depth[p], g_a = dL_dout_alpha[p], bg = background, and the record at 0-based position k
 * of t's list, Gaussian i (float32; the forward blend's operation order and its exp, which is libm's expf bit for bit):
 *     dx = means2D[i].x - (float)x, dy = means2D[i].y - (float)y, (A, B, C, o) = conic_opacity[i]
 *     power = -0.5f * ((A * dx) * dx + (C * dy) * dy) - (B * dx) * dy
 *     G = exp(power), raw = o * G, alpha = min(0.99f, raw)
 * The record is BLENDED into p iff the render backward counts it: k < n_contrib[p], !(power > 0) and !(alpha < 1/255) — the
 * forward's own arithmetic decides, so the set is the forward's. The pixel's walk runs BACK TO FRONT over its blended records,
 * from its last contributor, as render_backward_kernel's does:
 *     T <- final_t[p], S <- T * ((bg . g) [- g_a])                          before the walk
 *     T <- T / (1 - alpha)                                                  the transmittance in front of the record (T_i)
 *     cg = c_i . g [+ d_i * g_d]                                            c_i = colors[i]; d_i = the view-space z of means3D[i]
 *                                                                           (its reciprocal under GSR_FLAG_DEPTH_INVERSE)
 *     dL_dalpha = T * cg - S / (1 - alpha)
 *     S <- S + cg * alpha * T
 *     u = K d = (A * dx + B * dy, B * dx + C * dy)
 *     share(p, i) = raw > 0.99f ? (0, 0) : (-u.x, -u.y) * raw * dL_dalpha    the pixel's share of dL/d means2D[i]
 * A record whose raw > 0.99 (alpha is clamped: it does not move with the parameters) contributes zero but still divides T and
 * adds to S. The sums of gsr_backward are sum_p share(p, i); this call returns
 *     abs_dL_dmean2D[i] = ( sum_p |share(p, i).x| , sum_p |share(p, i).y| )
 * over the pixels of the call's band of tile rows, in pixel units with no NDC factor — the convention of dL_dmean2D, so
 * gsr_densify_accumulate takes the array unchanged.
 * The terms of L enter ONE dL_dalpha per pixel before the absolute value is taken: the result for colour + depth is NOT the sum of
 * the results for each alone (nor is it for any other pair of terms); it is <= that sum and >= |dL_dmean2D| componentwise.
 *
 * Accuracy. The per-pixel arithmetic is the render backward's (fused multiply-adds, the reciprocal of 1 - alpha in one
 * instruction), a lane sums its four pixels in float, the wave's 64 lanes are reduced in float, and one double atomic per value,
 * record and tile goes to sums_f64 — only for records some pixel of the tile blended. A second kernel over N rounds each pair to
 * float once, writes abs_dL_dmean2D IN FULL and leaves the scratch zero again. A row nothing blended is exactly +0.0 — those rows
 * are the ones whose sums are zero. All terms are non-negative, so nothing cancels across tiles; the order in which the tiles'
 * doubles arrive can still move the last bit before the rounding: two runs need not agree bit for bit.
 * Non-finite conics, opacities and gradients are outside this definition: nothing is read or written out of bounds for them.
 *
 * The call is asynchronous on backward->stream, synchronises nothing (GSR_FLAG_PROFILE apart, which waits to time the two
 * kernels) and allocates nothing. Of *backward it reads num_gaussians, width, height, background, means2D, conic_opacity, colors,
 * ranges, n_contrib, final_t, point_list, dL_dout_color, dL_dout_depth (and, with it, means3D and view_matrix), receipt,
 * tile_row_begin / tile_row_end and stream; its outputs, scratch, chain inputs and flags are neither read nor written.
 * A receipt with num_rendered == 0, or an empty band of tile rows: zeros are written, GSR_OK.
 *
 * GSR_ERR_INVALID_ARG, decided before any launch and before any HIP call: args or args->backward NULL; either struct_size other
 * than its header's; a receipt without the magic (a receipt is required); a receipt that does not fit num_gaussians / width /
 * height / the tile rows, or whose binning chunk's `values` is not point_list; a forward call that skipped its sorted lists
 * (GSR_PLAN_LISTS_SKIPPED in receipt.plan_used: there is no walk through the block lists here); a NULL background, means2D,
 * conic_opacity, colors, ranges, n_contrib or final_t; a NULL dL_dout_color; dL_dout_depth without means3D or view_matrix; a NULL
 * abs_dL_dmean2D or sums_f64; sums_f64 or abs_dL_dmean2D off an 8-byte boundary. Codes are returned and recorded as by every
 * entry point of gsrast_amd.h. */
#ifndef GSRAST_AMD_ABSGRAD_H
#define GSRAST_AMD_ABSGRAD_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_absgrad_args {
    uint32_t struct_size;                 /* sizeof(gsr_absgrad_args) */
    uint32_t flags;                       /* GSR_FLAG_DEPTH_INVERSE as the forward / backward calls'; GSR_FLAG_PROFILE */
    const gsr_backward_args* backward;    /* the struct a gsr_backward of this frame takes: read only, see above */
    const float* dL_dout_alpha;           /* f32[W H] or NULL: gsr_backward_alpha's second argument */
    float* abs_dL_dmean2D;                /* vec2[N], required; written in full */
    double* sums_f64;                     /* f64[2 N] scratch, required; ZERO on entry, left zero on return */
    float stage_ms;                       /* out, with GSR_FLAG_PROFILE: the walk and the rounding together (else 0) */
} gsr_absgrad_args;

int gsr_absgrad(gsr_absgrad_args* args);

#ifdef __cplusplus
}
#endif
#endif
