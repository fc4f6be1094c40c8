/* gsrast_amd_mcmc.h: the three steps of 3DGS-MCMC (Kheradmand et al. 2024) over the raw parameters — the companion of
 * gsrast_amd.h for a trainer that keeps a fixed budget of Gaussians instead of cloning, splitting and pruning them
 * (csrc/mcmc.hip). The GSR_* codes are those of gsrast_amd.h, and the error contract stated there covers the
 * status-returning calls of this header too: each returns a GSR_* code, leaves it as the calling thread's last error
 * (gsr_last_error) and forgets the HIP text of the call before it (gsr_last_hip_error).
 *
 * Every call enqueues on stream, does not synchronise, does not allocate and keeps no state in the library. The arrays
 * are those of gsr_activate_params: xyz f32[n][3], opacity_logit f32[n], log_scale f32[n][3], rotation f32[n][4] (real
 * part first, not normalised), shs f32[n][48]. activate_opacity, activate_scale and activate_rotation below are the
 * functions gsr_activate_params applies (csrc/activation_math.hpp): the same operations, so the same bits. */
#ifndef GSRAST_AMD_MCMC_H
#define GSRAST_AMD_MCMC_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- gsr_mcmc_noise: every step, one launch, in place on xyz over all n rows ----
 * scaler = learning rate x noise_lr, formed by the caller in double and rounded to float once. noise: standard normal, the
 * caller's tensor, as in gsr_densify_apply. Definition of the result, per row i, in float32 without contraction:
 *   o = activate_opacity(opacity_logit[i])
 *   t = 100.0f * ((1.0f - o) - 0.995f)          g = activate_opacity(t)          c = g * scaler
 *   v[k] = noise[i][k] * c                                                                  k = 0, 1, 2
 *   (s0, s1, s2) = activate_scale(log_scale[i])   (r, x, y, z) = activate_rotation(rotation[i])
 *   R = the nine entries gsr_densify_apply states (upstream's build_rotation)
 *   u[j] = s[j] * ((R0j*v[0] + R1j*v[1]) + R2j*v[2])                                        j = 0, 1, 2      (S R^T v)
 *   w[j] = s[j] * u[j]
 *   xyz'[a] = xyz[a] + ((Ra0*w[0] + Ra1*w[1]) + Ra2*w[2])                                   a = 0, 1, 2      (R S S R^T v)
 * so that the move is the Gaussian's covariance times the gated noise. With scaler == 0 every finite row keeps its bits
 * (x + 0 for a finite product). opacity_logit, log_scale, rotation and noise are read only.
 * Refused with GSR_ERR_INVALID_ARG before any HIP call: a wrong struct_size; n < 0; with n > 0 a NULL array; xyz,
 * log_scale, rotation or noise not 16-byte aligned, opacity_logit not 4-byte aligned. More rows than one launch covers
 * (n > GSR_MCMC_MAX_ROWS): GSR_ERR_TOO_LARGE. n == 0 is GSR_OK without a HIP call. */
#define GSR_MCMC_MAX_ROWS 2147483647ll    /* the 32-bit scan, row indices in i32 */
#define GSR_MCMC_MAX_RATIO 51             /* a row sampled 50 times or more is treated as sampled 50 times */
typedef struct gsr_mcmc_noise_args {
    uint32_t struct_size;          /* = sizeof(gsr_mcmc_noise_args) */
    float scaler;
    int64_t n;
    float* xyz;                    /* read and written */
    const float* opacity_logit;
    const float* log_scale;
    const float* rotation;
    const float* noise;            /* f32[n][3] */
    void* stream;
} gsr_mcmc_noise_args;
int gsr_mcmc_noise(const gsr_mcmc_noise_args* args);

/* ---- gsr_mcmc_plan: which rows are dead, and the weights the live ones are sampled by ----
 * A row is DEAD when opacity_logit[i] <= logit_min_opacity: the comparison is in the raw domain (no exponential enters
 * it; the caller forms logit(min_opacity) in double and rounds it to float once, as for gsr_densify_plan). A NaN is not
 * dead. dead_idx (i32, capacity n) receives the dead rows in ascending order, counts[0] of them; the rest of it is not
 * written. weights[i] = +0 for a dead row, activate_opacity(opacity_logit[i]) otherwise. counts (i32[2], device) =
 * (dead, alive), dead + alive == n. temp: gsr_mcmc_plan_temp_bytes(n) bytes of device memory, 16-byte aligned, the call's
 * alone until it has finished (a flag per row, scanned in place by ONE run of the reduce-then-scan, and the scan's own
 * scratch). Two launches and the scan's; no kernel waits for another workgroup.
 * Refused with GSR_ERR_INVALID_ARG before any HIP call: n < 0; a NULL counts; with n > 0 another NULL pointer; temp not
 * 16-byte aligned or another array not 4-byte aligned. n > GSR_MCMC_MAX_ROWS: GSR_ERR_TOO_LARGE, and
 * gsr_mcmc_plan_temp_bytes is then 0, as it is for n < 0. n == 0 writes counts = (0, 0). */
size_t gsr_mcmc_plan_temp_bytes(int64_t n);
int gsr_mcmc_plan(int64_t n, const float* opacity_logit, float logit_min_opacity, void* temp, int32_t* dead_idx,
                  float* weights, int32_t* counts, void* stream);

/* ---- gsr_mcmc_relocate: the sampled rows share their opacity with their copies ----
 * sampled[j], j < m: the row that sample j drew (a row may be drawn any number of times). dst: NULL, or the row that
 * receives the copy of sample j. The result is defined as three steps; it does not depend on how they are scheduled.
 *
 * 1. c[i] = the number of j with sampled[j] == i (integer atomics: their sum has no order). A pair j whose sampled[j] —
 *    or, with dst, whose dst[j] — lies outside [0, n) is ignored in every step and adds one to `rejected`, the first
 *    32-bit word of temp, which the caller may read after the call.
 * 2. Every row with c[i] > 0 is updated in place, once; both moments of all five arrays of that row become +0. With
 *    ratio = min(c[i] + 1, GSR_MCMC_MAX_RATIO) and o = (double)activate_opacity(opacity_logit[i]), all in DOUBLE without
 *    contraction, in this order:
 *      o_new = -expm1(log1p(-o) / ratio)                              (= 1 - (1 - o)^(1/ratio), without the cancellation)
 *      D = 0;  for i = 1..ratio:  p = 1;  for k = 0..i-1:  p = p * o_new;  term = (C(i-1,k) * p) / sqrt((double)(k+1))
 *                                                           D = (k even) ? D + term : D - term
 *      o_c = min(max(o_new, (double)min_opacity), 1 - 2^-23)
 *      opacity_logit'[i] = (float) log(o_c / (1 - o_c))
 *      log_scale'[i][a]  = log_scale[i][a] + (float) log(o / D)       (one float32 addition per axis)
 *    C(a, b), the binomial coefficient, by the recurrence C(a, 0) = 1, C(a, b+1) = (C(a, b) * (a - b)) / (b + 1) in
 *    double: every product stays below 2^53 up to C(50, 25) * 50 and every quotient is an integer, so each value is exact.
 *    (Upstream evaluates this in float32 and tests the opacity after the activation; ratio == 1 cannot occur here.)
 * 3. With dst != NULL, row dst[j] of all five arrays becomes a bitwise copy of row sampled[j] AFTER step 2, and both its
 *    moments +0. The caller guarantees that the dst rows are distinct and that none of them is a sampled row; otherwise
 *    the values of the rows concerned are unspecified, but every access stays inside the arrays.
 *
 * The two moment pointers of an array are both NULL (no optimiser state: none is written) or both set. temp:
 * gsr_mcmc_relocate_temp_bytes(n) bytes of device memory, 16-byte aligned, the call's alone until it has finished
 * (`rejected` in a 16-byte head, then c[n]).
 * Refused with GSR_ERR_INVALID_ARG before any HIP call: a wrong struct_size; n or m below 0; with n > 0 a NULL param;
 * with m > 0 a NULL sampled or temp; moment pointers of an array partly set; a parameter, moment or temp array not
 * 16-byte aligned, sampled or dst not 4-byte aligned; min_opacity not inside (0, 1). n or m > GSR_MCMC_MAX_ROWS:
 * GSR_ERR_TOO_LARGE, and gsr_mcmc_relocate_temp_bytes(n) is then 0, as it is for n < 0. m == 0 is GSR_OK and touches
 * nothing (temp included). */
typedef struct gsr_mcmc_array {
    float* param;                  /* f32[n * w], w = 3 / 1 / 3 / 4 / 48 for xyz / opacity_logit / log_scale / rotation / shs */
    float* exp_avg;
    float* exp_avg_sq;
} gsr_mcmc_array;
typedef struct gsr_mcmc_relocate_args {
    uint32_t struct_size;          /* = sizeof(gsr_mcmc_relocate_args) */
    float min_opacity;
    int64_t n;
    int64_t m;
    const int32_t* sampled;        /* i32[m] */
    const int32_t* dst;            /* i32[m] or NULL */
    gsr_mcmc_array xyz, opacity_logit, log_scale, rotation, shs;
    void* temp;
    void* stream;
} gsr_mcmc_relocate_args;
size_t gsr_mcmc_relocate_temp_bytes(int64_t n);
int gsr_mcmc_relocate(const gsr_mcmc_relocate_args* args);

#ifdef __cplusplus
}
#endif
#endif
