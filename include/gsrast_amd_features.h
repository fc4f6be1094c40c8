/* gsrast_amd_features.h — N-channel feature maps of a drawn frame, forward and backward (an addition to gsrast_amd.h).
 *
 * Everything a 3DGS user renders besides colour — normals, semantic or language features, labels, any scalar attribute — is the
 * blend's weights alpha_i T_i applied to another per-Gaussian vector f_i. gsr_features_forward walks the sorted lists a
 * gsr_forward call left once more, front to back, and composites C channels with that call's own alpha, T and decisions;
 * gsr_features_backward walks them back to front and returns the gradient w.r.t. the features and, optionally, ADDS the
 * geometry's share of that gradient into the double sums a gsr_backward of the same frame then chains down to the parameters.
 * Nothing of the forward call is written: the three chunks are read only.
 *
 * FORWARD, operation by operation (float32; no fused multiply-add except where said; exp = the forward blend's, libm's expf bit
 * for bit). For pixel p = (x, y) of tile t and the record at 1-based position k of t's list, Gaussian i:
 *     dx = means2D[i].x - (float)x, dy = means2D[i].y - (float)y, (A, B, C, o) = conic_opacity[i]
 *     power = -0.5f * ((A * dx) * dx + (C * dy) * dy) - (B * dx) * dy
 *     alpha = min(0.99f, o * exp(power))
 * The record is BLENDED into p iff !(power > 0), !(alpha < 1/255) and k <= n_contrib[p]: the set the forward call blended
 * (gsrast_amd_contrib.h; the cut-off is not compared again). T starts at 1 and, per blended record in list order,
 *     w = alpha * T
 *     acc[c] = fmaf(features[i * C + c], w, acc[c])        for every channel c
 *     T = T * (1 - alpha)
 * and the pixel leaves as
 *     out[c * W * H + y * W + x] = acc[c] + final_t[p] * background[c]      (a product, then a sum; `acc[c]` alone with a NULL background)
 * Pixels of tiles without a list, and every pixel of the band when the receipt's num_rendered is 0, get background[c] (or 0).
 * Rows outside the band of tile rows are not written.
 * Consequence, part of the contract: with features = the colours the forward call composited and background = its background,
 * `out` is that call's out_color bit for bit; with features = d_i (C = 1) and a NULL background it is its out_depth bit for bit.
 *
 * BACKWARD. L = sum(dL_dout * out). Per pixel the walk runs back to front over its blended records, as render_backward_kernel's
 * and gsr_absgrad's do (gsrast_amd_absgrad.h states it operation by operation): T <- final_t[p]; per record T <- T * rcp(1 - alpha)
 * (the transmittance in front of it, one instruction), w = alpha * T,
 *     dL_dfeatures[i * C + c] = sum over pixels of w * dL_dout[c, p]
 * Each lane sums its four pixels in float (fused multiply-adds), the wave's 64 lanes are reduced in float, and one double atomic
 * per value, record and tile goes to feature_sums_f64; a second kernel over N C rounds every sum to float once, writes
 * dL_dfeatures IN FULL (a row nothing blended is +0.0) and leaves the scratch zero again. The order in which the tiles' doubles
 * arrive can move the last bit: two runs need not agree bit for bit.
 * Channels are processed in chunks of K = GSR_FEATURES_CHUNK (GSR_FEATURES_CHUNK_NARROW when C is at most that): a (tile, chunk)
 * pair is one wavefront. That is exact, because dL/dalpha is a sum of per-channel terms, each with its own suffix sum.
 * geometry_sums_f64 (optional), f64[12 N] in the layout of gsr_backward_args.sums_f64 (mean2D 2, conic 3 + opacity 1, colour 3,
 * cov2D 3): per chunk, with cg = sum_{c in chunk} f_ic g_c(p) and the seed S = final_t[p] * sum_{c in chunk} background[c] g_c(p),
 *     dL_dalpha = fmaf(T, cg, -(S * rcp(1 - alpha))), S <- fmaf(cg, w, S)
 * and from dL_dalpha exactly the terms render_backward_kernel forms: raw = o * G > 0.99f contributes nothing but still divides T
 * and adds to S; otherwise dpow = raw * dL_dalpha, gop = G * dL_dalpha, u = K d, and the pass ADDS
 *     slots 0, 1: -u * dpow       slots 2..4: (-0.5 dx^2, -dx dy, -0.5 dy^2) * dpow       slot 5: gop
 *     slots 9..11: 0.5 dpow (ux ux, ux uy, uy uy)
 * as double atomics. Slots 6..8 (colour) are not touched. A gsr_backward / gsr_backward_alpha of the same receipt and tile rows,
 * called next on the same stream with this array as its sums_f64, adds the render backward's own sums to them and chains the
 * total (see sums_f64 in gsrast_amd.h). With geometry_sums_f64 NULL only dL_dfeatures is computed — the frozen-geometry case —
 * and no suffix sum is formed at all.
 * Non-finite conics, opacities, features and gradients are outside this definition: nothing is read or written out of bounds.
 *
 * Both calls are asynchronous on `stream`, synchronise nothing (GSR_FLAG_PROFILE apart, which waits to time the kernels) and
 * allocate nothing. A receipt with num_rendered == 0, or an empty band of tile rows: the forward writes the background into the
 * band (nothing for an empty band), the backward writes zeros; GSR_OK.
 *
 * GSR_ERR_INVALID_ARG, decided before any launch and before any HIP call: args NULL or a struct_size other than this header's;
 * channels < 1 or > GSR_FEATURES_MAX_CHANNELS; a receipt without the magic (a receipt is required); a receipt that does not fit
 * num_gaussians / width / height / the tile rows, or whose binning chunk's `values` is not point_list; a forward call that
 * skipped its sorted lists (GSR_PLAN_LISTS_SKIPPED in receipt.plan_used); a NULL means2D, conic_opacity, ranges, n_contrib,
 * final_t or features; forward: a NULL out; backward: a NULL dL_dout, dL_dfeatures or feature_sums_f64; means2D, ranges or a
 * double array off an 8-byte boundary, conic_opacity off a 16-byte one. Codes are returned and recorded as by every entry point of
 * gsrast_amd.h. */
#ifndef GSRAST_AMD_FEATURES_H
#define GSRAST_AMD_FEATURES_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_FEATURES_MAX_CHANNELS 256
/* channels a wavefront carries per walk, the compile-time widths of the kernels (multiples of 8; tuning builds define others):
 * a call of at most GSR_FEATURES_CHUNK_NARROW channels runs the narrow instance, every other call the wide one */
#ifndef GSR_FEATURES_CHUNK
#define GSR_FEATURES_CHUNK 16
#endif
#ifndef GSR_FEATURES_CHUNK_NARROW
#define GSR_FEATURES_CHUNK_NARROW 8
#endif

typedef struct gsr_features_args {
    uint32_t struct_size;          /* sizeof(gsr_features_args) */
    uint32_t flags;                /* GSR_FLAG_PROFILE */
    int32_t num_gaussians, width, height;
    int32_t channels;              /* C, 1 .. GSR_FEATURES_MAX_CHANNELS */
    const float* means2D;          /* vec2[N]  geometry chunk of the forward call */
    const float* conic_opacity;    /* vec4[N]  geometry chunk */
    const uint32_t* ranges;        /* uvec2[tiles]  image chunk */
    const uint32_t* n_contrib;     /* u32[W H]      image chunk */
    const float* final_t;          /* f32[W H]      image chunk */
    const uint32_t* point_list;    /* u32[R]   binning chunk: values */
    gsr_forward_receipt receipt;   /* gsr_forward_args.receipt of that call, by value: required */
    const float* features;         /* f32[N C], row-major, one row per Gaussian */
    const float* background;       /* f32[C] or NULL (zeros) */
    float* out;                    /* forward: f32[C W H], planar like out_color */
    const float* dL_dout;          /* backward: f32[C W H] */
    float* dL_dfeatures;           /* backward: f32[N C], written in full */
    double* feature_sums_f64;      /* backward: f64[N C] scratch (gsr_features_temp_bytes); ZERO on entry, left zero on return */
    double* geometry_sums_f64;     /* backward: f64[12 N] or NULL; added into, see above */
    int32_t tile_row_begin, tile_row_end;   /* as gsr_backward_args': both zero = the receipt's frame, every row */
    void* stream;                  /* hipStream_t */
    float stage_ms;                /* out, with GSR_FLAG_PROFILE: the call's kernels (else 0) */
} gsr_features_args;

/* bytes of feature_sums_f64 for n Gaussians and `channels` channels (0 for arguments the calls refuse) */
size_t gsr_features_temp_bytes(int32_t num_gaussians, int32_t channels);
int gsr_features_forward(gsr_features_args* args);
int gsr_features_backward(gsr_features_args* args);

#ifdef __cplusplus
}
#endif
#endif
