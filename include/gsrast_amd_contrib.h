/* gsrast_amd_contrib.h — per-Gaussian contribution statistics of a frame, exact (an addition to gsrast_amd.h).
 *
 * What a Gaussian does to a picture — its blending weights alpha_i T_i over the pixels — exists only inside the blend's walk over
 * the sorted lists. gsr_contribution walks the lists a gsr_forward call left (either semantics) once more, front to back, and
 * accumulates four integer statistics per Gaussian. Nothing of the forward call is written: the three chunks are read only, and a
 * gsr_backward of the same receipt may follow.
 *
 * The quantity, operation by operation (float32 unless said otherwise; no fused multiply-add; exp = the forward blend's, which is
 * libm's expf bit for bit). For pixel p = (x, y) of tile t and the record at 1-based position k of t's list, Gaussian i:
 *     dx = means2D[i].x - (float)x, dy = means2D[i].y - (float)y, (A, B, C, o) = conic_opacity[i]
 *     power = -0.5f * ((A * dx) * dx + (C * dy) * dy) - (B * dx) * dy
 *     alpha = min(0.99f, o * exp(power))
 * The record is BLENDED into p iff the forward call blended it: !(power > 0), !(alpha < 1/255), p was not finished, and
 * T * (1 - alpha) < t_cutoff did not finish p on this record (t_cutoff: 0.001, or 0.0001 under GSR_FLAG_SEMANTICS_INRIA). T is
 * the forward's front-to-back transmittance: 1 in front of the list, T <- T * (1 - alpha) after every blended record. The forward
 * call left the position of p's last blended record in n_contrib[p]: the record at position k is blended into p iff it passes
 * the two tests on power and alpha and k <= n_contrib[p] — the same set, and what this call evaluates (t_cutoff itself is
 * therefore not compared again). A record a pixel stops on is not blended. For a blended record
 *     w = alpha * T                                (the product the blend forms; not the backward's reciprocal reconstruction)
 *     q = (uint32_t)(w * 4294967296.0f)            (the scaling by 2^32 is exact; truncated toward zero)
 * w <= 0.99, so q fits 32 bits; w >= t_cutoff / 255 > 2^-22, so q > 0 and the truncation loses less than 2^-32.
 *
 * Each result is ACCUMULATED INTO the caller's array (zero them before the first frame; several views add up):
 *     weight_sum[i] += sum of q over the pixels that blended i                       (the summed weight is weight_sum * 2^-32)
 *     weight_max[i]  = max(weight_max[i], max of q over those pixels)
 *     pixels[i]     += the number of pixels that blended i
 *     dominant[i]   += the number of pixels whose largest q among their blended records is i's: the comparison is a strict `>` in
 *                      list order from a start of 0, so a tie goes to the front-most record; a pixel that blended nothing counts
 *                      for nobody
 * Integer adds and maxima commute: every array is bit for bit the same whatever order tiles, waves and atomics arrive in, within
 * a call and across calls. No floating-point atomic is used.
 * Non-finite conics and opacities are outside this definition: nothing is read or written out of bounds for them, their q is
 * unspecified.
 *
 * The call covers the tile rows of the receipt, is asynchronous on `stream`, synchronises nothing (GSR_FLAG_PROFILE apart, which
 * waits for the pass to time it), and allocates nothing. A receipt with num_rendered == 0 returns GSR_OK and writes nothing. A
 * NULL output is neither computed, where that saves work, nor written.
 *
 * GSR_ERR_INVALID_ARG, decided before any launch and before any HIP call: args NULL or a struct_size other than this header's;
 * a receipt without the magic; a receipt that does not fit num_gaussians / width / height; a point_list that is not `values` of
 * the receipt's binning chunk; a forward call that skipped its sorted lists (GSR_PLAN_LISTS_SKIPPED in receipt.plan_used); a NULL
 * means2D, conic_opacity, ranges or n_contrib; all four outputs NULL; weight_sum, pixels or dominant off an 8-byte boundary.
 * Codes are returned and recorded as by every entry point of gsrast_amd.h. */
#ifndef GSRAST_AMD_CONTRIB_H
#define GSRAST_AMD_CONTRIB_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_contribution_args {
    uint32_t struct_size;          /* sizeof(gsr_contribution_args) */
    uint32_t flags;                /* GSR_FLAG_SEMANTICS_INRIA as the forward call's; GSR_FLAG_PROFILE */
    int32_t num_gaussians, width, height;
    const float* means2D;          /* vec2[N]  geometry chunk of the forward call */
    const float* conic_opacity;    /* vec4[N]  geometry chunk */
    const uint32_t* ranges;        /* uvec2[tiles]  image chunk */
    const uint32_t* n_contrib;     /* u32[W H]      image chunk */
    const uint32_t* point_list;    /* u32[R]   binning chunk: values */
    gsr_forward_receipt receipt;   /* gsr_forward_args.receipt of that call, by value: required */
    uint64_t* weight_sum;          /* u64[N] or NULL */
    uint32_t* weight_max;          /* u32[N] or NULL */
    uint64_t* pixels;              /* u64[N] or NULL */
    uint64_t* dominant;            /* u64[N] or NULL (at least one of the four) */
    void* stream;                  /* hipStream_t */
    float stage_ms;                /* out, with GSR_FLAG_PROFILE: the pass (else 0) */
} gsr_contribution_args;

int gsr_contribution(gsr_contribution_args* args);

#ifdef __cplusplus
}
#endif
#endif
