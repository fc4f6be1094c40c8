/* gsrast_amd_init.h: initialisation of a scene from a point cloud — the companion of gsrast_amd.h for what runs once, before
 * the first frame. The GSR_* codes are those of gsrast_amd.h, and the error contract stated there covers the
 * status-returning calls of this header too: each returns a GSR_* code, leaves it as the calling thread's last error
 * (gsr_last_error) and forgets the HIP text of the call before it (gsr_last_hip_error). */
#ifndef GSRAST_AMD_INIT_H
#define GSRAST_AMD_INIT_H

#include "gsrast_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mean squared distance to the three nearest neighbours (csrc/knn.hip) ----
 * The role of simple_knn's distCUDA2 in upstream's create_from_pcd: the value the initial isotropic scale is taken from.
 *
 * Definition of the result, in float32 without contraction. For rows i != j (INDICES are compared, not positions: a
 * duplicate of point i is a neighbour of it at distance 0):
 *   dx = x[i] - x[j]     dy = y[i] - y[j]     dz = z[i] - z[j]
 *   d2(i, j) = (dx*dx + dy*dy) + dz*dz
 *   k = min(3, n - 1);  b0 <= b1 <= b2: the k smallest values of d2(i, .) in ascending order
 *   n >= 4:  mean_dist2[i] = ((b0 + b1) + b2) / 3.0f          (/ correctly rounded)
 *   n == 3:  mean_dist2[i] = (b0 + b1) / 2.0f
 *   n == 2:  mean_dist2[i] = b0
 *   n == 1:  mean_dist2[i] = +0
 * The k smallest values are unique as a multiset, so the result is a pure function of xyz: it does not depend on the
 * order in which the search meets the candidates, and two calls give the same bits. The search is exact, not approximate:
 * a box of candidates is skipped only where a lower bound of every d2 in it, rounded the same way as d2 itself, is no
 * smaller than the third-best distance that each of the queries it is skipped for has already found.
 *
 * Not upstream's behaviour: for n < 4 upstream sums FLT_MAX placeholders for the neighbours that do not exist (its result
 * is then about 1e38 or inf); here the mean is taken over the neighbours there are. Upstream orders the points by a Morton
 * code of 10 bits per axis and searches boxes of 1024 points; here the code has GSR_KNN_MORTON_BITS bits per axis, so that
 * one far outlier does not collapse every other point into a few cells. The code only orders the work and never affects
 * the result.
 *
 * Coordinates must be finite. With a non-finite coordinate the values are unspecified, but the call still terminates and
 * reads and writes inside its arrays only.
 *
 * The call is asynchronous on stream: no host synchronisation, no allocation, no state kept in the library. xyz is read
 * only. temp: gsr_knn_temp_bytes(n) bytes of device memory, 16-byte aligned, the call's alone until it has finished (the
 * codes and their sort, the points in sorted order, the boxes of GSR_KNN_LEAF consecutive sorted points and of
 * GSR_KNN_NODE consecutive such leaves). Refused with GSR_ERR_INVALID_ARG before any HIP call: n < 0; with n > 0 a NULL
 * xyz, mean_dist2 or temp; xyz or mean_dist2 not 4-byte aligned; temp not 16-byte aligned. n > GSR_KNN_MAX_POINTS (the
 * sort's 32-bit positions, one launch of the search): GSR_ERR_TOO_LARGE, and gsr_knn_temp_bytes is then 0, as it is for
 * n < 0. n == 0 is GSR_OK without a HIP call. */
#define GSR_KNN_LEAF 64              /* consecutive sorted points under one box: one wavefront's queries */
#define GSR_KNN_NODE 32              /* consecutive leaves under one box of the upper level */
#define GSR_KNN_MORTON_BITS 21       /* bits per axis of the code that orders the points */
#define GSR_KNN_MAX_POINTS 1073741824ll
size_t gsr_knn_temp_bytes(int64_t n);
int gsr_knn_mean_dist2(int64_t n, const float* xyz /* f32[n][3] */, float* mean_dist2 /* f32[n] */, void* temp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
