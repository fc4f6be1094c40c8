// The covariance chain of one Gaussian, stated once: quaternion -> R -> Sigma = M M^T, t = V mean, the 1.3 tan clamp of t.x / t.z
// and t.y / t.z, the Jacobian J and cov2D = (W J)^T Sigma (W J) in float32, and the gradient of that chain in double. Inline
// device functions only: no kernels, no launches, no parameter structs. INRIA selects the upstream profile where the two differ.
//
// The float32 side keeps each profile's operation order (every file is compiled with -ffp-contract=off), so the kernels that
// call it make the same decisions bit for bit: antialias.hip's d1 is the forward's `det`, and the clamp decisions of
// backward.hip, camera_backward.hip and antialias.hip are the forward's. Callers: antialias.hip (both sides), normals.hip (R, t,
// R -> q), backward.hip's preprocess_backward_kernel (t, the clamp, the double side) and camera_backward.hip (t and the clamp).
// preprocess.hip and preprocess_inria.hip — the forward itself — remain the second statement of the float32 side, and an edit
// to the float32 side here has to be made there too. They are the benchmark's path and move here only with unchanged resource
// figures and an unchanged preprocess stage (profiles/chain_passes_cost.txt has the figures that kept them where they are).
#pragma once
#include "gsr_common.hpp"

namespace gsr {

struct M3 { float m[3][3]; };   // m[col][row]

__device__ __forceinline__ float fminr(float a, float b) { return (b < a) ? b : a; }   // glm::min
__device__ __forceinline__ float fmaxr(float a, float b) { return (a < b) ? b : a; }   // glm::max

__device__ __forceinline__ M3 mul3(const M3& a, const M3& b) {
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int row = 0; row < 3; ++row)
            r.m[c][row] = a.m[0][row] * b.m[c][0] + a.m[1][row] * b.m[c][1] + a.m[2][row] * b.m[c][2];
    return r;
}
__device__ __forceinline__ M3 transpose3(const M3& a) {
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int row = 0; row < 3; ++row) r.m[c][row] = a.m[row][c];
    return r;
}

// ---- float32: the forward's arithmetic ------------------------------------------------------------------------------------------

// The rotation matrix of a quaternion as each profile's forward builds it. gscuda: (x, y, z, w) normalised, x the real part, the
// entries rounded through double (quatToMat). Upstream: (r, x, y, z) as given, written row-wise into a column-major constructor.
template <bool INRIA>
__device__ __forceinline__ M3 rotation_of(const float4 rot) {
    M3 rm;
    if constexpr (INRIA) {
        const float r = rot.x, x = rot.y, y = rot.z, z = rot.w;
        rm.m[0][0] = 1.0f - 2.0f * (y * y + z * z); rm.m[0][1] = 2.0f * (x * y - r * z); rm.m[0][2] = 2.0f * (x * z + r * y);
        rm.m[1][0] = 2.0f * (x * y + r * z); rm.m[1][1] = 1.0f - 2.0f * (x * x + z * z); rm.m[1][2] = 2.0f * (y * z - r * x);
        rm.m[2][0] = 2.0f * (x * z - r * y); rm.m[2][1] = 2.0f * (y * z + r * x); rm.m[2][2] = 1.0f - 2.0f * (x * x + y * y);
    } else {
        const float dq = (rot.x * rot.x + rot.y * rot.y) + (rot.z * rot.z + rot.w * rot.w);
        const float inv = 1.0f / sqrtf(dq);
        const float x = rot.x * inv, y = rot.y * inv, z = rot.z * inv, w = rot.w * inv;
        rm.m[0][0] = (float)(2.0 * (double)(x * x + y * y) - 1.0);
        rm.m[0][1] = (float)(2.0 * (double)(y * z + x * w));
        rm.m[0][2] = (float)(2.0 * (double)(y * w - x * z));
        rm.m[1][0] = (float)(2.0 * (double)(y * z - x * w));
        rm.m[1][1] = (float)(2.0 * (double)(x * x + z * z) - 1.0);
        rm.m[1][2] = (float)(2.0 * (double)(z * w + x * y));
        rm.m[2][0] = (float)(2.0 * (double)(y * w + x * z));
        rm.m[2][1] = (float)(2.0 * (double)(z * w - x * y));
        rm.m[2][2] = (float)(2.0 * (double)(x * x + w * w) - 1.0);
    }
    return rm;
}

// Axis a of the Gaussian in world space: column a of the rotation (constant indices only: the matrix stays in registers). The
// caller has built all nine entries for the one column it takes: that is the price of one statement of R (normals.hip formed
// three entries per branch before), a few registers in its streaming kernels and nothing in their time.
template <bool INRIA>
__device__ __forceinline__ void rotation_axis(const M3& rm, int a, float (&nw)[3]) {
    if constexpr (INRIA) {
        if (a == 0) { nw[0] = rm.m[0][0]; nw[1] = rm.m[1][0]; nw[2] = rm.m[2][0]; }
        else if (a == 1) { nw[0] = rm.m[0][1]; nw[1] = rm.m[1][1]; nw[2] = rm.m[2][1]; }
        else { nw[0] = rm.m[0][2]; nw[1] = rm.m[1][2]; nw[2] = rm.m[2][2]; }
    } else {
        if (a == 0) { nw[0] = rm.m[0][0]; nw[1] = rm.m[0][1]; nw[2] = rm.m[0][2]; }
        else if (a == 1) { nw[0] = rm.m[1][0]; nw[1] = rm.m[1][1]; nw[2] = rm.m[1][2]; }
        else { nw[0] = rm.m[2][0]; nw[1] = rm.m[2][1]; nw[2] = rm.m[2][2]; }
    }
}

// Sigma = M M^T in each profile's own product order: gscuda M = R S, upstream Sigma = (S R)^T (S R). Symmetric bit for bit (its
// entries (r, c) and (c, r) are the same products added in the same order): the six floats the preprocess kernels keep of it
// and spread again are this matrix.
template <bool INRIA>
__device__ __forceinline__ M3 covariance_of(float scale_modifier, const float4 sc, const M3& rm) {
    M3 s;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) s.m[c][r] = 0.0f;
    s.m[0][0] = scale_modifier * sc.x;
    s.m[1][1] = scale_modifier * sc.y;
    s.m[2][2] = scale_modifier * sc.z;
    if constexpr (INRIA) {
        const M3 mm = mul3(s, rm);
        return mul3(transpose3(mm), mm);
    } else {
        const M3 rs = mul3(rm, s);
        return mul3(rs, transpose3(rs));
    }
}

// t = V (x, y, z, 1) in each profile's summation order. (preprocess_backward_kernel and camera_pass_kernel take the gscuda order
// for both profiles: view_point<false>.)
template <bool INRIA>
__device__ __forceinline__ void view_point(const float* v, const float4 mean, float& tx, float& ty, float& tz) {
    if constexpr (INRIA) {
        tx = v[0] * mean.x + v[4] * mean.y + v[8] * mean.z + v[12];
        ty = v[1] * mean.x + v[5] * mean.y + v[9] * mean.z + v[13];
        tz = v[2] * mean.x + v[6] * mean.y + v[10] * mean.z + v[14];
    } else {
        tx = (v[0] * mean.x + v[4] * mean.y) + (v[8] * mean.z + v[12] * 1.0f);
        ty = (v[1] * mean.x + v[5] * mean.y) + (v[9] * mean.z + v[13] * 1.0f);
        tz = (v[2] * mean.x + v[6] * mean.y) + (v[10] * mean.z + v[14] * 1.0f);
    }
}

// t.x / t.z and t.y / t.z clamped to +-1.3 tan (computeCov2D), with the decisions.
struct RatioClamp {
    float cx, cy;                       // the clamped ratios
    bool hi_x, lo_x, hi_y, lo_y;        // the ratio lay above +lim (below -lim)
    bool clx, cly;                      // clamped: t.x (t.y) no longer moves the entry, t.z does
};
// Two variants, because they treat a NaN ratio differently (the value is -lim in both; only the second counts it as clamped):
// with glm's min / max and clx = hi || lo, as the forward states the clamp — antialias.hip;
__device__ __forceinline__ RatioClamp clamp_ratios_glm(float tx, float ty, float tz, float limx, float limy) {
    RatioClamp k;
    const float rx = tx / tz, ry = ty / tz;
    k.cx = fminr(limx, fmaxr(-limx, rx));
    k.cy = fminr(limy, fmaxr(-limy, ry));
    k.hi_x = limx < rx; k.lo_x = rx < -limx;
    k.hi_y = limy < ry; k.lo_y = ry < -limy;
    k.clx = k.hi_x || k.lo_x; k.cly = k.hi_y || k.lo_y;
    return k;
}
// with fminf / fmaxf and clx = (ratio != clamped ratio) — preprocess_backward_kernel and camera_pass_kernel. (Neither reads
// hi_* / lo_*: they are filled so that one type serves both variants.)
__device__ __forceinline__ RatioClamp clamp_ratios_libm(float tx, float ty, float tz, float limx, float limy) {
    RatioClamp k;
    const float rx = tx / tz, ry = ty / tz;
    k.cx = fminf(limx, fmaxf(-limx, rx));
    k.cy = fminf(limy, fmaxf(-limy, ry));
    k.hi_x = limx < rx; k.lo_x = rx < -limx;
    k.hi_y = limy < ry; k.lo_y = ry < -limy;
    k.clx = rx != k.cx; k.cly = ry != k.cy;
    return k;
}

// J at t = (cx t.z, cy t.z, t.z) and cov2D = (W J)^T Sigma (W J): entries [0][0], [0][1], [1][1] of the result.
__device__ __forceinline__ M3 cov2d_of(const float* view, const RatioClamp& k, float tz, float focal_x, float focal_y, const M3& sigma) {
    const float ux = k.cx * tz, uy = k.cy * tz;
    M3 j;
    j.m[0][0] = focal_x / tz; j.m[0][1] = 0.0f; j.m[0][2] = (-focal_x * ux) / (tz * tz);
    j.m[1][0] = 0.0f; j.m[1][1] = focal_y / tz; j.m[1][2] = (-focal_y * uy) / (tz * tz);
    j.m[2][0] = 0.0f; j.m[2][1] = 0.0f; j.m[2][2] = 0.0f;
    M3 wv;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) wv.m[c][r] = view[4 * r + c];
    const M3 tm = mul3(wv, j);
    return mul3(mul3(transpose3(tm), sigma), tm);
}

// ---- double: the gradient of the chain, from the float32 inputs and decisions ---------------------------------------------------

// The projection at one Gaussian: the view matrix, t as clamped, J's four entries and P = J W (2 x 3), cov2D = P Sigma P^T.
struct ProjectionFrame {
    double v[16];
    double tz, cx, cy, tx, ty;          // t.z, the clamped ratios, t.x = cx t.z, t.y = cy t.z
    bool clx, cly;
    double fx, fy, j00, j11, j02, j12;
    double P[2][3];
};
__device__ __forceinline__ ProjectionFrame projection_frame(const float* view, double tz, double cx, double cy, bool clx, bool cly,
                                                            double fx, double fy) {
    ProjectionFrame f;
#pragma unroll
    for (int i = 0; i < 16; ++i) f.v[i] = (double)view[i];
    f.tz = tz; f.cx = cx; f.cy = cy; f.clx = clx; f.cly = cly;
    f.tx = cx * tz; f.ty = cy * tz;
    f.fx = fx; f.fy = fy;
    f.j00 = fx / tz; f.j11 = fy / tz; f.j02 = -fx * f.tx / (tz * tz); f.j12 = -fy * f.ty / (tz * tz);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f.P[0][c] = f.j00 * f.v[4 * c + 0] + f.j02 * f.v[4 * c + 2];
        f.P[1][c] = f.j11 * f.v[4 * c + 1] + f.j12 * f.v[4 * c + 2];
    }
    return f;
}

// The three entries of cov2D = P Sigma P^T (before the 0.3 of the low-pass filter).
__device__ __forceinline__ void cov2d_f64(const ProjectionFrame& f, const double (&s)[3][3], double& a, double& b, double& c) {
    double ps[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) ps[r][k] = f.P[r][0] * s[0][k] + f.P[r][1] * s[1][k] + f.P[r][2] * s[2][k];
    a = ps[0][0] * f.P[0][0] + ps[0][1] * f.P[0][1] + ps[0][2] * f.P[0][2];
    b = ps[0][0] * f.P[1][0] + ps[0][1] * f.P[1][1] + ps[0][2] * f.P[1][2];
    c = ps[1][0] * f.P[1][0] + ps[1][1] * f.P[1][1] + ps[1][2] * f.P[1][2];
}

// gSigma = P^T gM P, the full symmetric matrix's entries; gM = (m00, m01; m01, m11) the gradient w.r.t. the full symmetric cov2D.
__device__ __forceinline__ void sigma_gradient(const ProjectionFrame& f, double m00, double m01, double m11, double (&gS)[3][3]) {
    double gp[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gp[0][c] = m00 * f.P[0][c] + m01 * f.P[1][c];
        gp[1][c] = m01 * f.P[0][c] + m11 * f.P[1][c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) gS[r][c] = f.P[0][r] * gp[0][c] + f.P[1][r] * gp[1][c];
}

// The mean's gradient through the Jacobian J(t): cov2D = J Mw J^T with Mw = W Sigma W^T; gJ = 2 gcov J Mw.
__device__ __forceinline__ void mean_gradient(const ProjectionFrame& f, const double (&s)[3][3], double m00, double m01, double m11,
                                              double (&gmean)[3]) {
    const double* v = f.v;
    double ws[3][3], mw[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) ws[r][c] = v[0 + r] * s[0][c] + v[4 + r] * s[1][c] + v[8 + r] * s[2][c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) mw[r][c] = ws[r][0] * v[0 + c] + ws[r][1] * v[4 + c] + ws[r][2] * v[8 + c];
    const double J[2][3] = {{f.j00, 0.0, f.j02}, {0.0, f.j11, f.j12}};
    double jm[2][3], gJ[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) jm[r][c] = J[r][0] * mw[0][c] + J[r][1] * mw[1][c] + J[r][2] * mw[2][c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gJ[0][c] = 2.0 * (m00 * jm[0][c] + m01 * jm[1][c]);
        gJ[1][c] = 2.0 * (m01 * jm[0][c] + m11 * jm[1][c]);
    }
    const double tz = f.tz, fx = f.fx, fy = f.fy;
    const double itz2 = 1.0 / (tz * tz);
    const double g_tx = -gJ[0][2] * fx * itz2, g_ty = -gJ[1][2] * fy * itz2;
    const double g_tz = -(gJ[0][0] * fx + gJ[1][1] * fy) * itz2 + (gJ[0][2] * fx * f.tx + gJ[1][2] * fy * f.ty) * (2.0 / (tz * tz * tz));
    // a clamped t.x = cx t.z no longer moves with t.x, and moves with t.z instead
    const double gt0 = f.clx ? 0.0 : g_tx, gt1 = f.cly ? 0.0 : g_ty;
    const double gt2 = g_tz + (f.clx ? g_tx * f.cx : 0.0) + (f.cly ? g_ty * f.cy : 0.0);
#pragma unroll
    for (int j = 0; j < 3; ++j) gmean[j] = v[4 * j + 0] * gt0 + v[4 * j + 1] * gt1 + v[4 * j + 2] * gt2;
}

// The rotation in double, Rm[row][column], Sigma = Rm diag(sv^2) Rm^T in both profiles. qn: the quaternion the entries are
// formed from — as given (upstream: (r, x, y, z), inv = 1) or normalised by inv (gscuda: x the real part).
template <bool INRIA>
__device__ __forceinline__ void rotation_f64(const float4 rot, double (&Rm)[3][3], double (&qn)[4], double& inv) {
    qn[0] = (double)rot.x; qn[1] = (double)rot.y; qn[2] = (double)rot.z; qn[3] = (double)rot.w;
    inv = 1.0;
    if constexpr (INRIA) {
        const double r = qn[0], x = qn[1], y = qn[2], z = qn[3];
        Rm[0][0] = 1.0 - 2.0 * (y * y + z * z); Rm[0][1] = 2.0 * (x * y - r * z); Rm[0][2] = 2.0 * (x * z + r * y);
        Rm[1][0] = 2.0 * (x * y + r * z); Rm[1][1] = 1.0 - 2.0 * (x * x + z * z); Rm[1][2] = 2.0 * (y * z - r * x);
        Rm[2][0] = 2.0 * (x * z - r * y); Rm[2][1] = 2.0 * (y * z + r * x); Rm[2][2] = 1.0 - 2.0 * (x * x + y * y);
    } else {
        inv = 1.0 / sqrt((qn[0] * qn[0] + qn[1] * qn[1]) + (qn[2] * qn[2] + qn[3] * qn[3]));
#pragma unroll
        for (int i = 0; i < 4; ++i) qn[i] *= inv;
        const double x = qn[0], y = qn[1], z = qn[2], w = qn[3];
        Rm[0][0] = 2.0 * (x * x + y * y) - 1.0; Rm[0][1] = 2.0 * (y * z - x * w); Rm[0][2] = 2.0 * (y * w + x * z);
        Rm[1][0] = 2.0 * (y * z + x * w); Rm[1][1] = 2.0 * (x * x + z * z) - 1.0; Rm[1][2] = 2.0 * (z * w - x * y);
        Rm[2][0] = 2.0 * (y * w - x * z); Rm[2][1] = 2.0 * (z * w + x * y); Rm[2][2] = 2.0 * (x * x + w * w) - 1.0;
    }
}

// Column a of Rm (rotation_axis in double; Rm is [row][column] in both profiles).
__device__ __forceinline__ void rotation_axis_f64(const double (&Rm)[3][3], int a, double (&nw)[3]) {
    if (a == 0) { nw[0] = Rm[0][0]; nw[1] = Rm[1][0]; nw[2] = Rm[2][0]; }
    else if (a == 1) { nw[0] = Rm[0][1]; nw[1] = Rm[1][1]; nw[2] = Rm[2][1]; }
    else { nw[0] = Rm[0][2]; nw[1] = Rm[1][2]; nw[2] = Rm[2][2]; }
}

// Sigma = M M^T, M = Rm diag(sv): gM = 2 gSigma M, to the scales (sv = mod s) and to Rm.
__device__ __forceinline__ void scale_rotation_gradient(const double (&gS)[3][3], const double (&Rm)[3][3], const double (&sv)[3],
                                                        double mod, double (&gsc)[3], double (&gR)[3][3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double gm[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) gm[r] = 2.0 * (gS[r][0] * Rm[0][c] + gS[r][1] * Rm[1][c] + gS[r][2] * Rm[2][c]) * sv[c];
        gsc[c] = mod * (Rm[0][c] * gm[0] + Rm[1][c] * gm[1] + Rm[2][c] * gm[2]);
#pragma unroll
        for (int r = 0; r < 3; ++r) gR[r][c] = gm[r] * sv[c];
    }
}

// From Rm to the quaternion as given: upstream directly; gscuda dR/dq for the normalised quaternion, then through the normalisation.
template <bool INRIA>
__device__ __forceinline__ void quaternion_gradient(const double (&gR)[3][3], const double (&qn)[4], double inv, double (&gq)[4]) {
    if constexpr (INRIA) {
        const double r = qn[0], x = qn[1], y = qn[2], z = qn[3];
        gq[0] = 2.0 * (z * (gR[1][0] - gR[0][1]) + y * (gR[0][2] - gR[2][0]) + x * (gR[2][1] - gR[1][2]));
        gq[1] = 2.0 * (y * (gR[0][1] + gR[1][0]) + z * (gR[0][2] + gR[2][0]) + r * (gR[2][1] - gR[1][2])) - 4.0 * x * (gR[1][1] + gR[2][2]);
        gq[2] = 2.0 * (x * (gR[0][1] + gR[1][0]) + r * (gR[0][2] - gR[2][0]) + z * (gR[1][2] + gR[2][1])) - 4.0 * y * (gR[0][0] + gR[2][2]);
        gq[3] = 2.0 * (r * (gR[1][0] - gR[0][1]) + x * (gR[0][2] + gR[2][0]) + y * (gR[1][2] + gR[2][1])) - 4.0 * z * (gR[0][0] + gR[1][1]);
    } else {
        const double x = qn[0], y = qn[1], z = qn[2], w = qn[3];
        const double gx = 4.0 * x * (gR[0][0] + gR[1][1] + gR[2][2]) + 2.0 * (w * (gR[1][0] - gR[0][1]) + z * (gR[0][2] - gR[2][0]) + y * (gR[2][1] - gR[1][2]));
        const double gy = 4.0 * y * gR[0][0] + 2.0 * (z * (gR[0][1] + gR[1][0]) + w * (gR[0][2] + gR[2][0]) + x * (gR[2][1] - gR[1][2]));
        const double gz = 4.0 * z * gR[1][1] + 2.0 * (y * (gR[0][1] + gR[1][0]) + w * (gR[1][2] + gR[2][1]) + x * (gR[0][2] - gR[2][0]));
        const double gw = 4.0 * w * gR[2][2] + 2.0 * (y * (gR[0][2] + gR[2][0]) + z * (gR[1][2] + gR[2][1]) + x * (gR[1][0] - gR[0][1]));
        const double dot = x * gx + y * gy + z * gz + w * gw;
        gq[0] = (gx - x * dot) * inv; gq[1] = (gy - y * dot) * inv; gq[2] = (gz - z * dot) * inv; gq[3] = (gw - w * dot) * inv;
    }
}

}  // namespace gsr
