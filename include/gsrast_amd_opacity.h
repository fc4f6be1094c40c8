/* gsrast_amd_opacity.h — the gradient of the accumulated opacity in the backward pass (an addition to gsrast_amd.h).
 *
 * gsr_forward leaves out_alpha = 1 - final_t per pixel (accum_alpha in the image chunk holds final_t). gsr_backward
 * differentiates L = sum(dL_dout_color * out_color) [+ sum(dL_dout_depth * out_depth)]; this call is gsr_backward with one
 * more term,
 *     L += sum_p dL_dout_alpha[p] (1 - final_t[p]).
 * final_t already reaches the colour through the background, out_color_c = C_c + final_t bg_c, so
 *     L = sum_c g_c C_c + final_t (bg . g - g_a) + const
 * and the whole term is the seed of "what lies behind" that every pixel starts its walk with, in float32:
 *     S = final_t * ((bg0 * g0 + bg1 * g1 + bg2 * g2) - g_a)       (g_a = dL_dout_alpha[p]; gsr_backward: S = final_t * (bg0 * g0 + ...))
 * Every output of gsr_backward receives its share — that of colours (1, 0, 0) against (g_a, 0, 0) over a zero background;
 * dL_dcolors and dL_dshs none: the opacity does not depend on the colours. There is no new output and no new scratch; the
 * receipt of any forward call serves; tile-row bands add up as before; a pixel nothing was blended into (n_contrib == 0)
 * contributes nothing; R == 0 gives all-zero gradients. args->dL_dout_color stays required: a caller that wants this term
 * alone passes zeros there. gsr_camera_backward needs nothing for it: the term is in the per-Gaussian gradients it reads.
 *
 * The gradient is an argument of the call, not a field of gsr_backward_args: that struct's size is what gsr_backward checks
 * of its callers, and it stays what they were compiled with.
 *
 * args             as for gsr_backward, every rule of it (struct_size included)
 * dL_dout_alpha    device f32[W H], row-major like final_t; or NULL: the call is gsr_backward(args), output for output
 * Returns and records GSR_* codes as gsr_backward does. */
#ifndef GSRAST_AMD_OPACITY_H
#define GSRAST_AMD_OPACITY_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int gsr_backward_alpha(gsr_backward_args* args, const float* dL_dout_alpha);

#ifdef __cplusplus
}
#endif
#endif
