// Antialiased splatting (include/gsrast_amd_antialias.h): the opacity compensation c = sqrt(det(cov2D) / det(cov2D + 0.3 I))
// as its own per-Gaussian pass in front of gsr_forward, and its gradient behind gsr_backward. One lane per Gaussian,
// streaming (HBM-bound): no LDS, no atomics, nothing crosses lanes.
//
// The float32 arithmetic of the 2D covariance restates the two preprocess kernels' (preprocess.hip, preprocess_inria.hip:
// this file is compiled with -ffp-contract=off like them) operation for operation, so that d1 below is the forward call's
// `det` bit for bit and the cull and clamp decisions are the forward's. The gradient restates the covariance part of
// gsr_backward's chain (backward.hip, preprocess_backward_kernel), seeded with dL/dcov2D, in double like that one.
#include "../../include/gsrast_amd_antialias.h"
#include "preprocess_common.hpp"

namespace gsr {
namespace {

constexpr float kFloor = 0.000025f;      // upstream's floor of d0 / d1

struct AntialiasParams {
    int n;
    const float4* means3D;
    const float4* scales;
    const float4* rotations;
    const float* opacities;
    const float* view;
    const float* proj;
    float scale_modifier, tan_fovx, tan_fovy, focal_x, focal_y;
    // forward
    float* opacities_out;
    float* compensation;
    // backward
    const float* g_out;
    const int32_t* radii;
    float* dL_dopacities;
    float4* dL_dmeans3D;
    float4* dL_dscales;
    float4* dL_drotations;
};

// What the float32 forward decides for one Gaussian.
struct Compensation {
    float c = 1.0f;            // the factor
    bool flows = false;        // a gradient goes through c: the covariance was computed, d1 is finite and not zero, the floor is not active
    bool hi_x = false, lo_x = false, hi_y = false, lo_y = false;      // t.x / t.z (t.y / t.z) was clamped at +lim (-lim)
};

template <bool INRIA>
__device__ __forceinline__ Compensation compensation_of(const AntialiasParams& p, const float* view, const float* proj, const float4 mean,
                                                        const float4 sc, const float4 rot) {
    Compensation out;
    float tx, ty, tz;
    M3 sigma;
    M3 s;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) s.m[c][r] = 0.0f;
    s.m[0][0] = p.scale_modifier * sc.x;
    s.m[1][1] = p.scale_modifier * sc.y;
    s.m[2][2] = p.scale_modifier * sc.z;
    if constexpr (INRIA) {
        const float* v = view;
        tx = v[0] * mean.x + v[4] * mean.y + v[8] * mean.z + v[12];
        ty = v[1] * mean.x + v[5] * mean.y + v[9] * mean.z + v[13];
        tz = v[2] * mean.x + v[6] * mean.y + v[10] * mean.z + v[14];
        if (tz <= 0.2f) return out;
        const float r = rot.x, x = rot.y, y = rot.z, z = rot.w;
        M3 rm;
        rm.m[0][0] = 1.0f - 2.0f * (y * y + z * z); rm.m[0][1] = 2.0f * (x * y - r * z); rm.m[0][2] = 2.0f * (x * z + r * y);
        rm.m[1][0] = 2.0f * (x * y + r * z); rm.m[1][1] = 1.0f - 2.0f * (x * x + z * z); rm.m[1][2] = 2.0f * (y * z - r * x);
        rm.m[2][0] = 2.0f * (x * z - r * y); rm.m[2][1] = 2.0f * (y * z + r * x); rm.m[2][2] = 1.0f - 2.0f * (x * x + y * y);
        const M3 mm = mul3(s, rm);
        sigma = mul3(transpose3(mm), mm);
    } else {
        const float* m = proj;
        const float phx = (m[0] * mean.x + m[4] * mean.y) + (m[8] * mean.z + m[12] * mean.w);
        const float phy = (m[1] * mean.x + m[5] * mean.y) + (m[9] * mean.z + m[13] * mean.w);
        const float phz = (m[2] * mean.x + m[6] * mean.y) + (m[10] * mean.z + m[14] * mean.w);
        const float phw = (m[3] * mean.x + m[7] * mean.y) + (m[11] * mean.z + m[15] * mean.w);
        const float one_over_w = 1.0f / (0.001f + phw);
        const float prx = one_over_w * phx, pry = one_over_w * phy, prz = one_over_w * phz;
        if (prz < 0.0f || prz > 1.0f || prx < -1.3f || prx > 1.3f || pry < -1.3f || pry > 1.3f) return out;
        const float dq = (rot.x * rot.x + rot.y * rot.y) + (rot.z * rot.z + rot.w * rot.w);
        const float inv = 1.0f / sqrtf(dq);
        const float x = rot.x * inv, y = rot.y * inv, z = rot.z * inv, w = rot.w * inv;
        M3 rm;
        rm.m[0][0] = (float)(2.0 * (double)(x * x + y * y) - 1.0);
        rm.m[0][1] = (float)(2.0 * (double)(y * z + x * w));
        rm.m[0][2] = (float)(2.0 * (double)(y * w - x * z));
        rm.m[1][0] = (float)(2.0 * (double)(y * z - x * w));
        rm.m[1][1] = (float)(2.0 * (double)(x * x + z * z) - 1.0);
        rm.m[1][2] = (float)(2.0 * (double)(z * w + x * y));
        rm.m[2][0] = (float)(2.0 * (double)(y * w + x * z));
        rm.m[2][1] = (float)(2.0 * (double)(z * w - x * y));
        rm.m[2][2] = (float)(2.0 * (double)(x * x + w * w) - 1.0);
        const M3 rs = mul3(rm, s);
        sigma = mul3(rs, transpose3(rs));
        const float* v = view;
        tx = (v[0] * mean.x + v[4] * mean.y) + (v[8] * mean.z + v[12] * 1.0f);
        ty = (v[1] * mean.x + v[5] * mean.y) + (v[9] * mean.z + v[13] * 1.0f);
        tz = (v[2] * mean.x + v[6] * mean.y) + (v[10] * mean.z + v[14] * 1.0f);
    }
    // Sigma is symmetric bit for bit (its entries (r, c) and (c, r) are the same products added in the same order): the
    // six floats the preprocess kernels keep of it and spread again are this matrix
    const float limx = 1.3f * p.tan_fovx, limy = 1.3f * p.tan_fovy;
    const float rx = tx / tz, ry = ty / tz;
    const float ux = fminr(limx, fmaxr(-limx, rx)) * tz;
    const float uy = fminr(limy, fmaxr(-limy, ry)) * tz;
    out.hi_x = limx < rx; out.lo_x = rx < -limx;
    out.hi_y = limy < ry; out.lo_y = ry < -limy;
    M3 j;
    j.m[0][0] = p.focal_x / tz; j.m[0][1] = 0.0f; j.m[0][2] = (-p.focal_x * ux) / (tz * tz);
    j.m[1][0] = 0.0f; j.m[1][1] = p.focal_y / tz; j.m[1][2] = (-p.focal_y * uy) / (tz * tz);
    j.m[2][0] = 0.0f; j.m[2][1] = 0.0f; j.m[2][2] = 0.0f;
    M3 wv;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) wv.m[c][r] = view[4 * r + c];
    const M3 tm = mul3(wv, j);
    const M3 cv = mul3(mul3(transpose3(tm), sigma), tm);
    const float a0 = cv.m[0][0], b = cv.m[0][1], c0 = cv.m[1][1];
    const float d0 = a0 * c0 - b * b;
    const float ca = a0 + 0.3f, cc = c0 + 0.3f;
    const float d1 = ca * cc - b * b;
    if (d1 == 0.0f || !__builtin_isfinite(d1)) return out;
    const float r = d0 / d1;
    out.c = sqrtf(fmaxr(kFloor, r));
    out.flows = kFloor < r;
    return out;
}

typedef float nt_f4 __attribute__((ext_vector_type(4)));
// (the rows are read once: streaming loads, as in preprocess.hip)
__device__ __forceinline__ float4 ld4(const float4* q) {
    const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(q));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float4* q, float x, float y, float z, float w) {
    __builtin_nontemporal_store((nt_f4){x, y, z, w}, reinterpret_cast<nt_f4*>(q));
}

// Memory schedule of a wave: the view (and projection) matrix through the scalar cache, the three rows and the opacity of
// every lane in one round trip, then the stores.
template <bool INRIA>
__global__ __launch_bounds__(256) void antialias_forward_kernel(const AntialiasParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    float view[16], proj[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { view[i] = p.view[i]; proj[i] = INRIA ? 0.0f : p.proj[i]; }
    const float4 mean = ld4(p.means3D + idx), sc = ld4(p.scales + idx), rot = ld4(p.rotations + idx);
    const float o = p.opacities_out ? __builtin_nontemporal_load(p.opacities + idx) : 0.0f;
    const Compensation k = compensation_of<INRIA>(p, view, proj, mean, sc, rot);
    // (c == 1.0f: o * 1.0f is o bit for bit, a NaN's payload included, so no branch is needed for "o' = o")
    if (p.opacities_out) p.opacities_out[idx] = k.c == 1.0f ? o : o * k.c;
    if (p.compensation) p.compensation[idx] = k.c;
}

// Memory schedule: radii and g first (a culled Gaussian, or one the frame's backward left without a gradient — most of
// a scene — ends there and stores its zeros), then every remaining load, then the arithmetic, then the stores.
template <bool INRIA>
__global__ __launch_bounds__(256) void antialias_backward_kernel(const AntialiasParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;
    float view[16], proj[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { view[i] = p.view[i]; proj[i] = INRIA ? 0.0f : p.proj[i]; }
    const bool has_tile = p.radii == nullptr || p.radii[idx] > 0;
    const float g = has_tile ? __builtin_nontemporal_load(p.g_out + idx) : 0.0f;
    typedef double R;
    float g_o = 0.0f;
    R gmean[3] = {0, 0, 0}, gsc[3] = {0, 0, 0}, gq[4] = {0, 0, 0, 0};
    if (has_tile && g != 0.0f) {
        const float4 mean = ld4(p.means3D + idx), sc = ld4(p.scales + idx), rot = ld4(p.rotations + idx);
        const float o = __builtin_nontemporal_load(p.opacities + idx);
        const Compensation k = compensation_of<INRIA>(p, view, proj, mean, sc, rot);
        g_o = k.c * g;
        const bool chain = k.flows && (p.dL_dmeans3D || p.dL_dscales || p.dL_drotations);
        if (chain) {
            R v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = (R)view[i];
            const R mx = (R)mean.x, my = (R)mean.y, mz = (R)mean.z;
            const R t0 = v[0] * mx + v[4] * my + v[8] * mz + v[12];
            const R t1 = v[1] * mx + v[5] * my + v[9] * mz + v[13];
            const R tz = v[2] * mx + v[6] * my + v[10] * mz + v[14];
            const R limx = (R)(1.3f * p.tan_fovx), limy = (R)(1.3f * p.tan_fovy);
            const bool clx = k.hi_x || k.lo_x, cly = k.hi_y || k.lo_y;
            const R cx = k.hi_x ? limx : (k.lo_x ? -limx : t0 / tz), cy = k.hi_y ? limy : (k.lo_y ? -limy : t1 / tz);
            const R tx = cx * tz, ty = cy * tz;
            const R fx = (R)p.focal_x, fy = (R)p.focal_y;
            const R j00 = fx / tz, j11 = fy / tz, j02 = -fx * tx / (tz * tz), j12 = -fy * ty / (tz * tz);
            // P = J W (2 x 3): cov2D = P Sigma P^T
            R P[2][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                P[0][c] = j00 * v[4 * c + 0] + j02 * v[4 * c + 2];
                P[1][c] = j11 * v[4 * c + 1] + j12 * v[4 * c + 2];
            }
            // Sigma = Rm diag(sv^2) Rm^T in both profiles
            const R mod = (R)p.scale_modifier;
            const R sv[3] = {mod * (R)sc.x, mod * (R)sc.y, mod * (R)sc.z};
            R Rm[3][3];
            R qn[4] = {(R)rot.x, (R)rot.y, (R)rot.z, (R)rot.w};
            [[maybe_unused]] R inv = 1.0;
            if constexpr (INRIA) {
                const R r = qn[0], x = qn[1], y = qn[2], z = qn[3];
                Rm[0][0] = 1.0 - 2.0 * (y * y + z * z); Rm[0][1] = 2.0 * (x * y - r * z); Rm[0][2] = 2.0 * (x * z + r * y);
                Rm[1][0] = 2.0 * (x * y + r * z); Rm[1][1] = 1.0 - 2.0 * (x * x + z * z); Rm[1][2] = 2.0 * (y * z - r * x);
                Rm[2][0] = 2.0 * (x * z - r * y); Rm[2][1] = 2.0 * (y * z + r * x); Rm[2][2] = 1.0 - 2.0 * (x * x + y * y);
            } else {
                inv = 1.0 / sqrt((qn[0] * qn[0] + qn[1] * qn[1]) + (qn[2] * qn[2] + qn[3] * qn[3]));
#pragma unroll
                for (int i = 0; i < 4; ++i) qn[i] *= inv;
                const R x = qn[0], y = qn[1], z = qn[2], w = qn[3];
                Rm[0][0] = 2.0 * (x * x + y * y) - 1.0; Rm[0][1] = 2.0 * (y * z - x * w); Rm[0][2] = 2.0 * (y * w + x * z);
                Rm[1][0] = 2.0 * (y * z + x * w); Rm[1][1] = 2.0 * (x * x + z * z) - 1.0; Rm[1][2] = 2.0 * (z * w - x * y);
                Rm[2][0] = 2.0 * (y * w - x * z); Rm[2][1] = 2.0 * (z * w + x * y); Rm[2][2] = 2.0 * (x * x + w * w) - 1.0;
            }
            R s[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    s[r][c] = Rm[r][0] * sv[0] * sv[0] * Rm[c][0] + Rm[r][1] * sv[1] * sv[1] * Rm[c][1] + Rm[r][2] * sv[2] * sv[2] * Rm[c][2];
            R ps[2][3];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) ps[r][c] = P[r][0] * s[0][c] + P[r][1] * s[1][c] + P[r][2] * s[2][c];
            const R a0 = ps[0][0] * P[0][0] + ps[0][1] * P[0][1] + ps[0][2] * P[0][2];
            const R b = ps[0][0] * P[1][0] + ps[0][1] * P[1][1] + ps[0][2] * P[1][2];
            const R c0 = ps[1][0] * P[1][0] + ps[1][1] * P[1][1] + ps[1][2] * P[1][2];
            const R ca = a0 + (R)0.3f, cc = c0 + (R)0.3f;
            const R d0 = a0 * c0 - b * b, d1 = ca * cc - b * b;
            const R r = d0 / d1;
            // G = o g through c = sqrt(r): dL/dr = G / (2 c); r = d0 / d1 to the three entries of cov2D
            const R gr = (R)o * (R)g / (2.0 * sqrt(r));
            const R id1 = 1.0 / d1;
            const R m00 = gr * (c0 - r * cc) * id1, m11 = gr * (a0 - r * ca) * id1;
            const R m01 = gr * (r - 1.0) * b * id1;          // each of the two off-diagonal entries: half of -2 b (1 - r) / d1
            // gS = P^T gM P (the full symmetric matrix's entries)
            R gp[2][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gp[0][c] = m00 * P[0][c] + m01 * P[1][c];
                gp[1][c] = m01 * P[0][c] + m11 * P[1][c];
            }
            R gS[3][3];
#pragma unroll
            for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                for (int c = 0; c < 3; ++c) gS[rr][c] = P[0][rr] * gp[0][c] + P[1][rr] * gp[1][c];
            if (p.dL_dmeans3D) {
                // through the Jacobian J(t): cov2D = J Mw J^T with Mw = W Sigma W^T; gJ = 2 gcov J Mw
                R ws[3][3], mw[3][3];
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                    for (int c = 0; c < 3; ++c) ws[rr][c] = v[0 + rr] * s[0][c] + v[4 + rr] * s[1][c] + v[8 + rr] * s[2][c];
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                    for (int c = 0; c < 3; ++c) mw[rr][c] = ws[rr][0] * v[0 + c] + ws[rr][1] * v[4 + c] + ws[rr][2] * v[8 + c];
                const R J[2][3] = {{j00, 0.0, j02}, {0.0, j11, j12}};
                R jm[2][3], gJ[2][3];
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                    for (int c = 0; c < 3; ++c) jm[rr][c] = J[rr][0] * mw[0][c] + J[rr][1] * mw[1][c] + J[rr][2] * mw[2][c];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    gJ[0][c] = 2.0 * (m00 * jm[0][c] + m01 * jm[1][c]);
                    gJ[1][c] = 2.0 * (m01 * jm[0][c] + m11 * jm[1][c]);
                }
                const R itz2 = 1.0 / (tz * tz);
                const R g_tx = -gJ[0][2] * fx * itz2, g_ty = -gJ[1][2] * fy * itz2;
                const R g_tz = -(gJ[0][0] * fx + gJ[1][1] * fy) * itz2 + (gJ[0][2] * fx * tx + gJ[1][2] * fy * ty) * (2.0 / (tz * tz * tz));
                // a clamped t.x = cx t.z no longer moves with t.x, and moves with t.z instead
                const R gt0 = clx ? 0.0 : g_tx, gt1 = cly ? 0.0 : g_ty;
                const R gt2 = g_tz + (clx ? g_tx * cx : 0.0) + (cly ? g_ty * cy : 0.0);
#pragma unroll
                for (int jx = 0; jx < 3; ++jx) gmean[jx] = v[4 * jx + 0] * gt0 + v[4 * jx + 1] * gt1 + v[4 * jx + 2] * gt2;
            }
            if (p.dL_dscales || p.dL_drotations) {
                // Sigma = M M^T, M = Rm diag(sv): gM = 2 gSigma M
                R gR[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    R gm[3];
#pragma unroll
                    for (int rr = 0; rr < 3; ++rr) gm[rr] = 2.0 * (gS[rr][0] * Rm[0][c] + gS[rr][1] * Rm[1][c] + gS[rr][2] * Rm[2][c]) * sv[c];
                    gsc[c] = mod * (Rm[0][c] * gm[0] + Rm[1][c] * gm[1] + Rm[2][c] * gm[2]);
#pragma unroll
                    for (int rr = 0; rr < 3; ++rr) gR[rr][c] = gm[rr] * sv[c];
                }
                if constexpr (INRIA) {
                    const R r_ = qn[0], x = qn[1], y = qn[2], z = qn[3];
                    gq[0] = 2.0 * (z * (gR[1][0] - gR[0][1]) + y * (gR[0][2] - gR[2][0]) + x * (gR[2][1] - gR[1][2]));
                    gq[1] = 2.0 * (y * (gR[0][1] + gR[1][0]) + z * (gR[0][2] + gR[2][0]) + r_ * (gR[2][1] - gR[1][2])) - 4.0 * x * (gR[1][1] + gR[2][2]);
                    gq[2] = 2.0 * (x * (gR[0][1] + gR[1][0]) + r_ * (gR[0][2] - gR[2][0]) + z * (gR[1][2] + gR[2][1])) - 4.0 * y * (gR[0][0] + gR[2][2]);
                    gq[3] = 2.0 * (r_ * (gR[1][0] - gR[0][1]) + x * (gR[0][2] + gR[2][0]) + y * (gR[1][2] + gR[2][1])) - 4.0 * z * (gR[0][0] + gR[1][1]);
                } else {
                    // dR/dq for the normalised quaternion (x = real part), then through the normalisation
                    const R x = qn[0], y = qn[1], z = qn[2], w = qn[3];
                    const R gx = 4.0 * x * (gR[0][0] + gR[1][1] + gR[2][2]) + 2.0 * (w * (gR[1][0] - gR[0][1]) + z * (gR[0][2] - gR[2][0]) + y * (gR[2][1] - gR[1][2]));
                    const R gy = 4.0 * y * gR[0][0] + 2.0 * (z * (gR[0][1] + gR[1][0]) + w * (gR[0][2] + gR[2][0]) + x * (gR[2][1] - gR[1][2]));
                    const R gz = 4.0 * z * gR[1][1] + 2.0 * (y * (gR[0][1] + gR[1][0]) + w * (gR[1][2] + gR[2][1]) + x * (gR[0][2] - gR[2][0]));
                    const R gw = 4.0 * w * gR[2][2] + 2.0 * (y * (gR[0][2] + gR[2][0]) + z * (gR[1][2] + gR[2][1]) + x * (gR[1][0] - gR[0][1]));
                    const R dot = x * gx + y * gy + z * gz + w * gw;
                    gq[0] = (gx - x * dot) * inv; gq[1] = (gy - y * dot) * inv; gq[2] = (gz - z * dot) * inv; gq[3] = (gw - w * dot) * inv;
                }
            }
        }
    }
    // ---- stores ----
    if (p.dL_dopacities) p.dL_dopacities[idx] = g_o;
    if (p.dL_dmeans3D) st4(p.dL_dmeans3D + idx, (float)gmean[0], (float)gmean[1], (float)gmean[2], 0.0f);
    if (p.dL_dscales) st4(p.dL_dscales + idx, (float)gsc[0], (float)gsc[1], (float)gsc[2], 0.0f);
    if (p.dL_drotations) st4(p.dL_drotations + idx, (float)gq[0], (float)gq[1], (float)gq[2], (float)gq[3]);
}

inline bool positive_finite(float v) { return v > 0.0f && v <= 3.402823466e+38f; }      // (false for NaN and Inf)

// What both argument structs share, checked and copied: every refusal of the header, before any HIP call.
template <typename Args>
int fill_params(const Args* a, AntialiasParams& p) {
    if (a->flags & ~(uint32_t)GSR_FLAG_SEMANTICS_INRIA) return GSR_ERR_INVALID_ARG;
    if (a->num_gaussians < 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!positive_finite(a->tan_fovx) || !positive_finite(a->tan_fovy) || !positive_finite(a->scale_modifier)) return GSR_ERR_INVALID_ARG;
    if (!a->means3D || !a->scales || !a->rotations || !a->opacities || !a->view_matrix) return GSR_ERR_INVALID_ARG;
    const bool inria = (a->flags & GSR_FLAG_SEMANTICS_INRIA) != 0;
    if (!inria && !a->proj_matrix) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->means3D, 16) || misaligned(a->scales, 16) || misaligned(a->rotations, 16)) return GSR_ERR_INVALID_ARG;
    p = AntialiasParams{};
    p.n = a->num_gaussians;
    p.means3D = reinterpret_cast<const float4*>(a->means3D);
    p.scales = reinterpret_cast<const float4*>(a->scales);
    p.rotations = reinterpret_cast<const float4*>(a->rotations);
    p.opacities = a->opacities;
    p.view = a->view_matrix;
    p.proj = a->proj_matrix;
    p.scale_modifier = a->scale_modifier;
    p.tan_fovx = a->tan_fovx;
    p.tan_fovy = a->tan_fovy;
    p.focal_y = (float)a->height / (2.0f * a->tan_fovy);
    p.focal_x = inria ? (float)a->width / (2.0f * a->tan_fovx) : p.focal_y;
    return GSR_OK;
}

int antialias_forward_impl(gsr_antialias_args* a) {
    if (!a || a->struct_size != sizeof(gsr_antialias_args)) return GSR_ERR_INVALID_ARG;
    AntialiasParams p;
    GSR_TRY(fill_params(a, p));
    if (!a->opacities_out && !a->compensation) return GSR_ERR_INVALID_ARG;
    if (a->opacities_out == a->opacities) return GSR_ERR_INVALID_ARG;
    if (p.n == 0) return GSR_OK;
    p.opacities_out = a->opacities_out;
    p.compensation = a->compensation;
    const dim3 grid((unsigned)(((long long)p.n + 255) / 256));
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(antialias_forward_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(antialias_forward_kernel<false>, grid, dim3(256), 0, stream, p);
    GSR_LAUNCH_CHECK("antialias_forward_kernel");
    return GSR_OK;
}

int antialias_backward_impl(gsr_antialias_backward_args* a) {
    if (!a || a->struct_size != sizeof(gsr_antialias_backward_args)) return GSR_ERR_INVALID_ARG;
    AntialiasParams p;
    GSR_TRY(fill_params(a, p));
    if (!a->dL_dopacities_out) return GSR_ERR_INVALID_ARG;
    if (!a->dL_dopacities && !a->dL_dmeans3D && !a->dL_dscales && !a->dL_drotations) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->dL_dmeans3D, 16) || misaligned(a->dL_dscales, 16) || misaligned(a->dL_drotations, 16)) return GSR_ERR_INVALID_ARG;
    if (p.n == 0) return GSR_OK;
    p.g_out = a->dL_dopacities_out;
    p.radii = a->radii;
    p.dL_dopacities = a->dL_dopacities;
    p.dL_dmeans3D = reinterpret_cast<float4*>(a->dL_dmeans3D);
    p.dL_dscales = reinterpret_cast<float4*>(a->dL_dscales);
    p.dL_drotations = reinterpret_cast<float4*>(a->dL_drotations);
    const dim3 grid((unsigned)(((long long)p.n + 255) / 256));
    hipStream_t stream = reinterpret_cast<hipStream_t>(a->stream);
    if (a->flags & GSR_FLAG_SEMANTICS_INRIA) hipLaunchKernelGGL(antialias_backward_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(antialias_backward_kernel<false>, grid, dim3(256), 0, stream, p);
    GSR_LAUNCH_CHECK("antialias_backward_kernel");
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

extern "C" int gsr_antialias_forward(gsr_antialias_args* a) { return gsr::entry_point(gsr::antialias_forward_impl, a); }
extern "C" int gsr_antialias_backward(gsr_antialias_backward_args* a) { return gsr::entry_point(gsr::antialias_backward_impl, a); }
