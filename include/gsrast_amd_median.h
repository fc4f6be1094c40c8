/* gsrast_amd_median.h — the median depth map of a drawn frame, the per-pixel Gaussian ids, and the map's gradient (an addition to
 * gsrast_amd.h).
 *
 * The median depth of the geometry-aware splatting trainers (2DGS's depth_ratio = 1, RaDe-GS's depth, every TSDF-fusion script):
 * per pixel, the value of the record at which the transmittance falls through a threshold — a DECISION along the pixel's list,
 * not a sum over it, so no set of feature channels gives it. The same walk answers which Gaussian lies under a pixel: the id of
 * the selected record, and the id of the record with the largest blending weight (the `dominant` decision of gsr_contribution,
 * kept per pixel here). gsr_median_forward walks the sorted lists a gsr_forward call left once more, front to back, with that
 * call's own alpha, T and decisions; nothing of the forward call is written: the three chunks are read only.
 *
 * FORWARD, operation by operation (float32; NO fused multiply-add; exp = the forward blend's). For pixel p = (x, y) of tile t and
 * the record at 1-based position k of t's list, Gaussian i:
 *     dx = means2D[i].x - (float)x, dy = means2D[i].y - (float)y, (A, B, C, o) = conic_opacity[i]
 *     pw = -0.5f * ((A * dx) * dx + (C * dy) * dy) - (B * dx) * dy
 *     alpha = min(0.99f, o * exp(pw))
 * The record is BLENDED into p iff !(pw > 0), !(alpha < 1/255) and k <= n_contrib[p] (gsrast_amd_features.h: the set the forward
 * call blended). T starts at 1, sel = dom = GSR_MEDIAN_NONE, best = 0; per blended record in list order
 *     if (T > threshold) sel = i                       T is the transmittance IN FRONT of the record
 *     w = alpha * T;   q = (uint32_t)(w * 4294967296.0f)
 *     if (q > best) { best = q; dom = i; }             gsr_contribution's rule: strict, a tie stays in front, q == 0 never wins
 *     T = T * (1.0f - alpha)
 * and the pixel leaves as
 *     ids[y * W + x] = sel,      dominant_ids[y * W + x] = dom,
 *     out[y * W + x] = sel == GSR_MEDIAN_NONE ? 0.0f : values[sel]            a gather: the value's bits
 * threshold is a float, 0 <= threshold < 1:
 *     0.5             2DGS's median: the last blended record with T > 0.5 in front of it
 *     0               the last blended record
 *     just under 1    the first blended record (first hit)
 * T does not increase along a list, so sel is the last record of the prefix whose records have T > threshold in front of them;
 * a pixel whose transmittance never crosses keeps its last blended record. RaDe-GS's variant — no value where T never crosses —
 * is this map masked by !(final_t > threshold).
 * Each of out (with values), ids and dominant_ids may be NULL, not all three. A pixel nothing was blended into, every pixel of
 * a tile without a list, and every pixel of the band when the receipt's num_rendered is 0 get 0.0f / GSR_MEDIAN_NONE. Rows
 * outside the band of tile rows are not written. (How the walk is cut short — a pixel that has crossed leaves it, with
 * dominant_ids once (uint32_t)((0.99f * T) * 4294967296.0f) <= best, which no later w can exceed since float multiplication is
 * monotone — changes no result.)
 *
 * BACKWARD. L = sum_p g(p) out(p), g = dL_dout, with the selection held fixed:
 *     dL_dvalues[i] = sum over the pixels p of the band with ids[p] == i of g(p)
 * It is not a list walk: it reads only `ids` (the forward call's), dL_dout, the dimensions and the band of tile rows. It reads
 * NOTHING of the frame — none of the chunks' arrays — and does not look at `receipt`: the call is valid after the rasterizer has
 * drawn again, which is what lets an autograd graph outlive the next draw. An id >= num_gaussians, GSR_MEDIAN_NONE included, is
 * dropped. Every g is converted to double before it is added; the lanes of a 16 x 4 strip of a tile that hold the same id are
 * added on chip, one double atomic per distinct id and strip goes to value_sums_f64, and a second kernel over N rounds every sum
 * to float once, writes dL_dvalues IN FULL (a row nothing selected is +0.0) and leaves value_sums_f64 zero again. A sum
 * of n doubles is off by at most n 2^-53 sum |g| before its one rounding to float (2^-32 sum |g| up to 2^21 pixels a Gaussian);
 * with g in multiples of 2^-10 below 1 in magnitude nothing rounds on the way and the result is the same bits on every call.
 * Otherwise the order in which the strips' doubles arrive can move the last bit.
 *
 * What is NOT differentiated: the selection. sel is a decision, so the map is a step function of the geometry — it does not move
 * with a Gaussian's position, shape or opacity until the selection changes, and then it jumps. No gradient reaches means2D,
 * conic_opacity or anything upstream of them through this map; its gradient reaches the values only (for the view depth: the
 * mean's z through whatever formed the values).
 *
 * Both calls are asynchronous on `stream`, synchronise nothing (GSR_FLAG_PROFILE apart, which waits to time the kernels) and
 * allocate nothing. A receipt with num_rendered == 0: the forward writes 0.0f / GSR_MEDIAN_NONE into the band; an empty band of
 * tile rows: the forward writes nothing, the backward zeros into dL_dvalues; GSR_OK.
 *
 * GSR_ERR_INVALID_ARG, decided before any launch and before any HIP call: args NULL or a struct_size other than this header's;
 * num_gaussians, width or height not positive; tile rows outside the frame. Forward: a threshold outside [0, 1) (a NaN included);
 * a receipt without the magic (a receipt is required); a receipt that does not fit num_gaussians / width / height, tile rows that do
 * not lie inside the receipt's (any band of the rows the forward call drew is walked on its own: one row answers a pick), or whose binning chunk's `values` is not point_list; a forward call that skipped its sorted lists (GSR_PLAN_LISTS_SKIPPED); a
 * NULL means2D, conic_opacity, ranges, n_contrib or final_t; out, ids and dominant_ids all NULL; out without values; means2D or
 * ranges off an 8-byte boundary, conic_opacity off a 16-byte one. Backward: a NULL ids, dL_dout, dL_dvalues or value_sums_f64;
 * value_sums_f64 off an 8-byte boundary. Codes are returned and recorded as by every entry point of gsrast_amd.h. */
#ifndef GSRAST_AMD_MEDIAN_H
#define GSRAST_AMD_MEDIAN_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_MEDIAN_NONE 0xFFFFFFFFu   /* ids / dominant_ids of a pixel nothing was blended into */

typedef struct gsr_median_args {
    uint32_t struct_size;          /* sizeof(gsr_median_args) */
    uint32_t flags;                /* GSR_FLAG_PROFILE */
    int32_t num_gaussians, width, height;
    float threshold;               /* forward: 0 <= threshold < 1 */
    const float* means2D;          /* forward: vec2[N]  geometry chunk of the forward call */
    const float* conic_opacity;    /* forward: vec4[N]  geometry chunk */
    const uint32_t* ranges;        /* forward: uvec2[tiles]  image chunk */
    const uint32_t* n_contrib;     /* forward: u32[W H]      image chunk */
    const float* final_t;          /* forward: f32[W H]      image chunk */
    const uint32_t* point_list;    /* forward: u32[R]   binning chunk: values */
    gsr_forward_receipt receipt;   /* forward: gsr_forward_args.receipt of that call, by value: required. backward: not looked at */
    const float* values;           /* forward: f32[N], one scalar per Gaussian; NULL only with out NULL */
    float* out;                    /* forward: f32[W H] or NULL */
    uint32_t* ids;                 /* forward: u32[W H] or NULL, written. backward: read */
    uint32_t* dominant_ids;        /* forward: u32[W H] or NULL */
    const float* dL_dout;          /* backward: f32[W H] */
    float* dL_dvalues;             /* backward: f32[N], written in full */
    double* value_sums_f64;        /* backward: f64[N] scratch (gsr_median_temp_bytes); ZERO on entry, left zero on return */
    int32_t tile_row_begin, tile_row_end;   /* both zero = every row of the frame; forward: a band inside the receipt's rows */
    void* stream;                  /* hipStream_t */
    float stage_ms;                /* out, with GSR_FLAG_PROFILE: the call's kernels (else 0) */
} gsr_median_args;

/* bytes of value_sums_f64 for n Gaussians: 8 n (0 for an n the calls refuse) */
size_t gsr_median_temp_bytes(int32_t num_gaussians);
int gsr_median_forward(gsr_median_args* args);
int gsr_median_backward(gsr_median_args* args);

#ifdef __cplusplus
}
#endif
#endif
