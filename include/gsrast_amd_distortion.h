/* gsrast_amd_distortion.h — the depth distortion map of a drawn frame and its gradient (an addition to gsrast_amd.h).
 *
 * The distortion loss of Mip-NeRF 360 (Barron et al. 2022) as the geometry-aware splatting trainers use it (2DGS, GOF, RaDe-GS,
 * PGSR; `distloss=True` in gsplat): per pixel, over the records the frame blended, for a per-Gaussian scalar m (view depth,
 * inverse depth, an NDC-mapped depth),
 *     D(p) = sum_i sum_j w_i w_j |m_i - m_j|^q,      w_i = alpha_i T_i,      q = 1 or 2 (`power`)
 * It is quadratic in the blending weights of one pixel, so no set of feature channels gives it. gsr_distortion_forward walks the
 * sorted lists a gsr_forward call left once more, front to back, with that call's own alpha, T and decisions;
 * gsr_distortion_backward walks them back to front and returns the gradient w.r.t. the values and, optionally, ADDS the
 * geometry's share into the double sums a gsr_backward of the same frame then chains down to the parameters. Nothing of the
 * forward call is written: the three chunks are read only. The interval term of Mip-NeRF 360 has no counterpart: a splat has no
 * interval.
 *
 * FORWARD, operation by operation (float32; NO fused multiply-add except where fmaf is written; exp = the forward blend's). For
 * pixel p = (x, y) of tile t and the record at 1-based position k of t's list, Gaussian i, with m = values[i]:
 *     dx = means2D[i].x - (float)x, dy = means2D[i].y - (float)y, (A, B, C, o) = conic_opacity[i]
 *     pw = -0.5f * ((A * dx) * dx + (C * dy) * dy) - (B * dx) * dy
 *     alpha = min(0.99f, o * exp(pw))
 * The record is BLENDED into p iff !(pw > 0), !(alpha < 1/255) and k <= n_contrib[p] (gsrast_amd_features.h: the set the forward
 * call blended). T starts at 1 and D, M1, M2, m0 at 0; per blended record in list order
 *     if (T == 1.0f) m0 = m                     the pixel's first blended record: the values are CENTRED on it
 *     d = m - m0;   w = alpha * T;   Ap = 1.0f - T
 *     q = 2:   dd = d * d;   e = fmaf(dd, Ap, fmaf(-2.0f * d, M1, M2));   M2 = fmaf(dd, w, M2)
 *     q = 1:   e = fmaf(d, Ap, -M1)
 *     D = fmaf(w, e, D);   M1 = fmaf(d, w, M1);   T = T * (1.0f - alpha)
 * and the pixel leaves as
 *     out[y * W + x] = 2.0f * D,      moments[(0, 1, 2) * W * H + y * W + x] = m0, M1, M2        (M2 stays 0 for q = 1)
 * e is sum_{j<i} w_j (d_i - d_j)^q, so out is the double sum over ordered pairs. A pixel nothing was blended into, every pixel
 * of a tile without a list, and every pixel of the band when the receipt's num_rendered is 0 get 0 in all four planes. Rows
 * outside the band of tile rows are not written.
 * The centring is part of the contract: m^2 A - 2 m M1 + M2 on raw depths loses every digit when the depth is 10 and the spread
 * 0.01, and D does not change under a common shift of m, so the centred form is the same function. Values that are multiples of
 * 2^-10 and the same values shifted by 1024 give the same `out` bit for bit.
 * q = 1 is SIGNED in list order: out = 2 sum_i w_i sum_{j<i} w_j (m_i - m_j). That equals the absolute form wherever m does not
 * decrease along each list. That holds for the depth the frame sorted by (the geometry chunk's depths: the view-space z under
 * GSR_FLAG_SEMANTICS_INRIA, the NDC z under the reference's profile) and for every monotone function of it; under the reference's
 * profile two view depths whose NDC z tie in float32 (3e-5 apart at a distance of 5 with near = 0.05) may come in either order,
 * and such a pair then enters with its sign. For other values it is what it says. 2DGS's code computes half of q = 2.
 *
 * BACKWARD. L = sum_p g(p) out(p), g = dL_dout. Per pixel the walk runs back to front over its blended records as
 * render_backward_kernel's and gsr_absgrad's do (gsrast_amd_absgrad.h): T <- final_t[p]; per record inv = rcp(1 - alpha) (one
 * instruction), Tn = T * inv (the transmittance in front of the record), w = alpha * Tn, then T <- Tn. Before the walk the pixel
 * reads g, m0 = moments[0], M1n = moments[1], M2n = moments[2] (q = 2 only) and forms Tf = final_t[p],
 *     q = 2: An = 1.0f - Tf            q = 1: Tb = Tf (the transmittance behind the record in hand), Ms = 0
 *     S = 0
 * Per blended record, with d = m - m0 (float32, fmaf only where written):
 *     q = 2:   t = fmaf(d, An, -M1n)                                       d out / d m_i = 4 w t
 *              dv = 4.0f * t
 *              c = 2.0f * fmaf(d * d, An, fmaf(-2.0f * d, M1n, M2n))       d out / d w_i
 *     q = 1:   As = Tb - Tf;   Ap = 1.0f - Tn;   M1p = (M1n - Ms) - w * d
 *              dv = 2.0f * (Ap - As)                                       d out / d m_i = 2 w (Ap - As)
 *              c = 2.0f * ((fmaf(d, Ap, -M1p) + Ms) - d * As)
 *              Ms = fmaf(w, d, Ms);   Tb = Tn
 *     value sum of the lane:   a = fmaf(w * g, dv, a)
 *     dL_dalpha = g * fmaf(Tn, c, -(S * inv));   S = fmaf(c, w, S)
 * and from dL_dalpha on exactly the terms render_backward_kernel forms (gsrast_amd_features.h states them): raw = o * G > 0.99f
 * contributes nothing to the geometry but still divides T and adds to S; otherwise dpow = raw * dL_dalpha, gop = G * dL_dalpha,
 * u = K d, and the pass ADDS into geometry_sums_f64 (the layout of gsr_backward_args.sums_f64)
 *     slots 0, 1: -u * dpow       slots 2..4: (-0.5 dx^2, -dx dy, -0.5 dy^2) * dpow       slot 5: gop
 *     slots 9..11: 0.5 dpow (ux ux, ux uy, uy uy)
 * Slots 6..8 (colour) are not touched. (out does not depend on m0: the sum of d out / d m_i over a pixel's records is 0.)
 * Each lane sums its four pixels in float, the wave's 64 lanes are reduced in float, and one double atomic per value, record and
 * tile goes to value_sums_f64 / geometry_sums_f64; a second kernel over N rounds every value sum to float once, writes dL_dvalues
 * IN FULL (a row nothing blended is +0.0) and leaves value_sums_f64 zero again. The order in which the tiles' doubles arrive can
 * move the last bit. A gsr_backward / gsr_backward_alpha of the same receipt and tile rows, called next on the same stream with
 * geometry_sums_f64 as its sums_f64, chains the total (see sums_f64 in gsrast_amd.h); gsr_features_backward may seed the same
 * array first. With geometry_sums_f64 NULL only dL_dvalues is computed — the frozen-geometry case — and neither c nor S is
 * formed. With all values equal, out and everything added to the geometry sums are exactly zero for both powers, and so is
 * dL_dvalues for q = 2 (for q = 1 the signed form's derivative, 2 w (Ap - As), is not zero there).
 * Non-finite conics, opacities, values and gradients are outside this definition: nothing is read or written out of bounds.
 *
 * Both calls are asynchronous on `stream`, synchronise nothing (GSR_FLAG_PROFILE apart, which waits to time the kernels) and
 * allocate nothing. A receipt with num_rendered == 0: the forward writes zeros into the band, the backward zeros into
 * dL_dvalues; an empty band of tile rows: the forward writes nothing; GSR_OK.
 *
 * GSR_ERR_INVALID_ARG, decided before any launch and before any HIP call: args NULL or a struct_size other than this header's;
 * power other than 1 or 2; a receipt without the magic (a receipt is required); a receipt that does not fit num_gaussians / width
 * / height / the tile rows, or whose binning chunk's `values` is not point_list; a forward call that skipped its sorted lists
 * (GSR_PLAN_LISTS_SKIPPED); a NULL means2D, conic_opacity, ranges, n_contrib, final_t or values; forward: a NULL out or moments;
 * backward: a NULL moments, dL_dout, dL_dvalues or value_sums_f64; means2D, ranges or a double array off an 8-byte boundary,
 * conic_opacity off a 16-byte one. Codes are returned and recorded as by every entry point of gsrast_amd.h. */
#ifndef GSRAST_AMD_DISTORTION_H
#define GSRAST_AMD_DISTORTION_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsr_distortion_args {
    uint32_t struct_size;          /* sizeof(gsr_distortion_args) */
    uint32_t flags;                /* GSR_FLAG_PROFILE */
    int32_t num_gaussians, width, height;
    int32_t power;                 /* q: 1 or 2 */
    const float* means2D;          /* vec2[N]  geometry chunk of the forward call */
    const float* conic_opacity;    /* vec4[N]  geometry chunk */
    const uint32_t* ranges;        /* uvec2[tiles]  image chunk */
    const uint32_t* n_contrib;     /* u32[W H]      image chunk */
    const float* final_t;          /* f32[W H]      image chunk */
    const uint32_t* point_list;    /* u32[R]   binning chunk: values */
    gsr_forward_receipt receipt;   /* gsr_forward_args.receipt of that call, by value: required */
    const float* values;           /* f32[N]: m, one scalar per Gaussian */
    float* out;                    /* forward: f32[W H] */
    float* moments;                /* forward: written, backward: read. f32[3 W H]: m0, M1, M2 of the forward call with the same values and power */
    const float* dL_dout;          /* backward: f32[W H] */
    float* dL_dvalues;             /* backward: f32[N], written in full */
    double* value_sums_f64;        /* backward: f64[N] scratch (gsr_distortion_temp_bytes); ZERO on entry, left zero on return */
    double* geometry_sums_f64;     /* backward: f64[12 N] or NULL; added into, see above */
    int32_t tile_row_begin, tile_row_end;   /* as gsr_backward_args': both zero = the receipt's frame, every row */
    void* stream;                  /* hipStream_t */
    float stage_ms;                /* out, with GSR_FLAG_PROFILE: the call's kernels (else 0) */
} gsr_distortion_args;

/* bytes of value_sums_f64 for n Gaussians: 8 n (0 for an n the calls refuse) */
size_t gsr_distortion_temp_bytes(int32_t num_gaussians);
int gsr_distortion_forward(gsr_distortion_args* args);
int gsr_distortion_backward(gsr_distortion_args* args);

#ifdef __cplusplus
}
#endif
#endif
