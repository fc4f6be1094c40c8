// The depth distortion map of a drawn frame (include/gsrast_amd_distortion.h): 2 sum_i w_i sum_{j<i} w_j (m_i - m_j)^q per pixel
// over the sorted lists a forward call left, w = alpha T, and its gradient — passes of their own on the walks of list_walk.hpp,
// as features.hip's are, so that the blend, contrib_kernel and render_backward_kernel keep their object code. One wavefront per
// 16 x 16 tile, the record's value m staged in wave-private LDS beside the record:
//   - distortion_forward_kernel is the replay: per pixel the prefix moments M1 = sum w d, M2 = sum w d^2 of the values centred on
//     the pixel's first blended record (d = m - m0), and D = sum w e with e the record's distance to everything in front of it.
//     It leaves out = 2 D and the three planes m0, M1, M2 the backward reads.
//   - distortion_backward_kernel is the back walk: with the pixel's totals every record's d out / d w (c) and d out / d m come
//     from what the pixel read once; dL_dalpha = g (Tn c - S inv) with S the suffix sum of c w, and from there (GEO) the render
//     backward's own lines, added into slots 0..5 and 9..11 of the double sums a gsr_backward of the same frame then reads.
//     Without GEO neither c nor S is formed.
// A record's value sum rides in the seventh input of the wave_sum8 that carries the six geometry sums: two reductions a record,
// as in features.hip.
#include <hip/hip_runtime.h>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "list_walk.hpp"
#include "../../include/gsrast_amd_distortion.h"

namespace gsr {
namespace {

constexpr uint32_t kGeoFloats = 12;      // the layout of gsr_backward_args.sums_f64 (backward.hip: kAccFloats)

struct DistortionParams {
    WalkFrame frame;
    const float* values;          // f32[N]
    float* out;                   // forward: f32[W H]
    float* moments;               // forward: written; backward: read. f32[3 W H]
    const float* dL_dout;         // backward: f32[W H]
    double* value_sums;           // backward: f64[N]
    double* geometry_sums;        // backward (GEO): f64[12 N]
};

// ---- forward ----------------------------------------------------------------------------------------------------------------
struct DistortionStage : ReplayStage {
    float value[kWave];                  // a record's m
};

template <int POWER>
__global__ __launch_bounds__(kWave) void distortion_forward_kernel(const DistortionParams p) {
    __shared__ DistortionStage st;
    const int lane = (int)threadIdx.x;
    int tx, ty;
    const int tile = walk_tile(p.frame, &tx, &ty);
    if (tile < 0) return;
    const size_t plane = (size_t)p.frame.dims.width * (size_t)p.frame.dims.height;

    TileLanes s;
    tile_lanes_init(s, tx, ty, lane, p.frame.dims.width, p.frame.dims.height, -1);
    float D[4] = {}, M1[4] = {}, M2[4] = {}, m0[4] = {};

    replay_walk(p.frame, tile, tx, ty, lane, s, st, [&](const TileBox& box, const RecordBatch& b) {
        const uint32_t kept = stage_replay(box, st, b, p.frame.num_gaussians, [&](uint32_t slot, uint32_t id) {
            st.value[slot] = p.values[id];
        });
        for (uint32_t j = 0; j < kept; ++j) {
            const ReplayRecord r = replay_candidates(s, st, j);
            if (!r.any()) continue;
            const float m = st.value[j];
            replay_blend(s, st, j, r, [&](const int k, const unsigned long long live, const float alpha) {
                if (__builtin_amdgcn_inverse_ballot_w64(live)) {
                    const float T = s.T[k];
                    if (T == 1.0f) m0[k] = m;
                    const float d = m - m0[k], w = alpha * T, Ap = 1.0f - T;
                    float e;
                    if constexpr (POWER == 2) {
                        const float dd = d * d;
                        e = __builtin_fmaf(dd, Ap, __builtin_fmaf(-2.0f * d, M1[k], M2[k]));
                        M2[k] = __builtin_fmaf(dd, w, M2[k]);
                    } else {
                        e = __builtin_fmaf(d, Ap, -M1[k]);
                    }
                    D[k] = __builtin_fmaf(w, e, D[k]);
                    M1[k] = __builtin_fmaf(d, w, M1[k]);
                }
            });
        }
    });
    // (a tile without a list, a pixel nothing was blended into: the zeros the four started as)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!s.inside[k]) continue;
        const size_t pid = (size_t)(s.py0 + 4 * k) * (size_t)p.frame.dims.width + (size_t)s.px;
        p.out[pid] = 2.0f * D[k];
        p.moments[pid] = m0[k];
        p.moments[plane + pid] = M1[k];
        p.moments[2 * plane + pid] = M2[k];
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
template <int POWER, bool GEO>
__global__ __launch_bounds__(kWave) void distortion_backward_kernel(const DistortionParams p) {
    __shared__ BackStage st;
    __shared__ float s_value[kWave];
    const int lane = threadIdx.x;
    int tx, ty;
    const int tile = walk_tile(p.frame, &tx, &ty);
    if (tile < 0) return;
    const size_t plane = (size_t)p.frame.dims.width * (size_t)p.frame.dims.height;

    // Which of a record's sums this lane files: wave_sum8 leaves value kSumOfRow[r] in lane 8 r; wave_sum4 value kSumOfRow4[r]
    // in every lane of row r (lane 16 r + 4 files it). Of the eight, values 0..5 are the geometry's slots 0..5 (the render
    // backward's, backward.hip), value 6 is the record's value sum and value 7 is unused; the four are slots 9..11 and one unused.
    constexpr int kSumOfRow[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    constexpr int kSumOfRow4[4] = {9, 11, 10, 12};
    constexpr int kValueSum = 6;
    const int my8 = (lane & 7) == 0 ? kSumOfRow[lane >> 3] : -1;
    const int my_geo = (lane & 7) == 0 ? (my8 < 6 ? my8 : -1) : ((lane & 15) == 4 && kSumOfRow4[lane >> 4] < 12 ? kSumOfRow4[lane >> 4] : -1);

    BackLanes s;
    float g[4] = {}, m0[4] = {}, M1n[4] = {};
    [[maybe_unused]] float M2n[4] = {};
    [[maybe_unused]] float An[4], Tf[4], Tb[4], Ms[4], S[4];
    // the record in hand: its value and this lane's sums over its four pixels
    float m = 0.0f, a_v = 0.0f;
    [[maybe_unused]] float a_mx, a_my, a_A, a_B, a_C, a_op, a_m00, a_m01, a_m11;
    back_walk<true>(
        p.frame, tile, tx, ty, lane, s, st,
        /* seed */ [&](const int k, const size_t pid) {
            g[k] = p.dL_dout[pid];
            m0[k] = p.moments[pid];
            M1n[k] = p.moments[plane + pid];
            if constexpr (POWER == 2) M2n[k] = p.moments[2 * plane + pid];
        },
        /* start */ [&]() {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (POWER == 2) An[k] = 1.0f - s.T[k];
                else { Tf[k] = s.T[k]; Tb[k] = s.T[k]; Ms[k] = 0.0f; }
                if constexpr (GEO) S[k] = 0.0f;
            }
        },
        /* payload */ [&](const uint32_t slot, const uint32_t id) { s_value[slot] = p.values[id]; },
        /* begin */ [&](const int j) {
            m = s_value[j];
            a_v = 0.0f;
            if constexpr (GEO) a_mx = a_my = a_A = a_B = a_C = a_op = a_m00 = a_m01 = a_m11 = 0.0f;
        },
        /* on_pixel */ [&](const int k, const BackPixel& px) {
            const float d = m - m0[k];
            float dv;
            [[maybe_unused]] float c = 0.0f;
            if constexpr (POWER == 2) {
                const float t = __builtin_fmaf(d, An[k], -M1n[k]);
                dv = 4.0f * t;
                if constexpr (GEO) c = 2.0f * __builtin_fmaf(d * d, An[k], __builtin_fmaf(-2.0f * d, M1n[k], M2n[k]));
            } else {
                const float As = Tb[k] - Tf[k], Ap = 1.0f - px.Tn;
                dv = 2.0f * (Ap - As);
                if constexpr (GEO) {
                    const float M1p = (M1n[k] - Ms[k]) - px.w * d;
                    c = 2.0f * ((__builtin_fmaf(d, Ap, -M1p) + Ms[k]) - d * As);
                    Ms[k] = __builtin_fmaf(px.w, d, Ms[k]);          // (w is 0 where the pixel did not blend the record)
                }
                Tb[k] = px.act ? px.Tn : Tb[k];
            }
            a_v = __builtin_fmaf(px.w * g[k], dv, a_v);
            if constexpr (GEO) {
                // from here to the sums: render_backward_kernel's lines (backward.hip), as features_backward_kernel has them
                const float dx = px.dx, dy = px.dy;
                const float dL_dalpha = g[k] * __builtin_fmaf(px.Tn, c, -(S[k] * px.inv));
                S[k] = __builtin_fmaf(c, px.w, S[k]);
                const bool live = px.live();
                const float gop = live ? px.G * dL_dalpha : 0.0f;
                const float dpow = live ? px.raw * dL_dalpha : 0.0f;
                a_op += gop;
                a_A = __builtin_fmaf(-0.5f * dx * dx, dpow, a_A);
                a_B = __builtin_fmaf(-(dx * dy), dpow, a_B);
                a_C = __builtin_fmaf(-0.5f * dy * dy, dpow, a_C);
                const float ux = px.ux(), uy = px.uy();
                a_mx = __builtin_fmaf(-ux, dpow, a_mx);
                a_my = __builtin_fmaf(-uy, dpow, a_my);
                const float hux = 0.5f * dpow * ux, huy = 0.5f * dpow * uy;      // (the masked factor first: 0 x finite)
                a_m00 = __builtin_fmaf(hux, ux, a_m00); a_m01 = __builtin_fmaf(hux, uy, a_m01); a_m11 = __builtin_fmaf(huy, uy, a_m11);
            }
        },
        /* file */ [&](const int j) {
            const size_t id = st.id[j];
            if constexpr (GEO) {
                const float t8 = wave_sum8(a_mx, a_my, a_A, a_B, a_C, a_op, a_v, 0.0f, lane);
                const float t4 = wave_sum4(a_m00, a_m01, a_m11, 0.0f);
                if (my8 == kValueSum && t8 != 0.0f) unsafeAtomicAdd(p.value_sums + id, (double)t8);
                const float total = (lane & 7) == 4 ? t4 : t8;
                if (my_geo >= 0 && total != 0.0f) unsafeAtomicAdd(p.geometry_sums + kGeoFloats * id + (uint32_t)my_geo, (double)total);
            } else {
                const float total = wave_sum2(a_v, 0.0f);            // (lane 31 holds the total of the first)
                if (lane == 31 && total != 0.0f) unsafeAtomicAdd(p.value_sums + id, (double)total);
            }
        });
}

// What both calls check, in the header's order; *nothing: no record to walk (R == 0 or an empty band).
int distortion_check(gsr_distortion_args* a, bool backward, FrameDims* d, bool* nothing) {
    if (!a || a->struct_size != sizeof(gsr_distortion_args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    if (a->num_gaussians <= 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (a->power != 1 && a->power != 2) return GSR_ERR_INVALID_ARG;
    if (!a->means2D || !a->conic_opacity || !a->ranges || !a->n_contrib || !a->final_t || !a->values) return GSR_ERR_INVALID_ARG;
    if (!a->moments) return GSR_ERR_INVALID_ARG;
    if (backward ? (!a->dL_dout || !a->dL_dvalues || !a->value_sums_f64) : !a->out) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->means2D, 8) || misaligned(a->conic_opacity, 16) || misaligned(a->ranges, 8)) return GSR_ERR_INVALID_ARG;
    if (backward && (misaligned(a->value_sums_f64, 8) || misaligned(a->geometry_sums_f64, 8))) return GSR_ERR_INVALID_ARG;
    return walk_check(a->receipt, a->num_gaussians, a->width, a->height, a->tile_row_begin, a->tile_row_end, false, a->point_list, d, nothing);
}

DistortionParams distortion_params(const gsr_distortion_args* a, const FrameDims& d) {
    DistortionParams p;
    p.frame = walk_frame(a->ranges, a->point_list, a->means2D, a->conic_opacity, a->n_contrib, a->final_t, d, a->num_gaussians,
                         a->receipt.num_rendered);
    p.values = a->values;
    p.out = a->out;
    p.moments = a->moments;
    p.dL_dout = a->dL_dout;
    p.value_sums = a->value_sums_f64;
    p.geometry_sums = a->geometry_sums_f64;
    return p;
}

int distortion_forward_impl(gsr_distortion_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(distortion_check(a, false, &d, &nothing));
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (d.row_begin != d.row_end) {          // (R == 0: every tile of the band is a tile without a list)
        const DistortionParams p = distortion_params(a, d);
        const dim3 grid((unsigned)blocks);
        if (a->power == 2) hipLaunchKernelGGL(distortion_forward_kernel<2>, grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL(distortion_forward_kernel<1>, grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("distortion_forward_kernel");
    }
    return timer.end(stream, &a->stage_ms);
}

int distortion_backward_impl(gsr_distortion_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(distortion_check(a, true, &d, &nothing));
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    const size_t count = (size_t)a->num_gaussians;
    if (exceeds_grid(blocks) || exceeds_grid(finish_sums_workgroups(count))) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (!nothing) {
        DistortionParams p = distortion_params(a, d);
        // (the tiles that were slow in the forward blend are the slow ones here: they go first, as they did there)
        p.frame.tile_order = tile_order_of_call(a->receipt, d.row_begin, d.row_end);
        const bool square = a->power == 2, geo = a->geometry_sums_f64 != nullptr;
        const dim3 grid((unsigned)blocks);
        if (square && geo) hipLaunchKernelGGL((distortion_backward_kernel<2, true>), grid, dim3(kWave), 0, stream, p);
        else if (square) hipLaunchKernelGGL((distortion_backward_kernel<2, false>), grid, dim3(kWave), 0, stream, p);
        else if (geo) hipLaunchKernelGGL((distortion_backward_kernel<1, true>), grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL((distortion_backward_kernel<1, false>), grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("distortion_backward_kernel");
    }
    GSR_TRY(launch_finish_sums<1>(count, a->value_sums_f64, a->dL_dvalues, stream));
    return timer.end(stream, &a->stage_ms);
}

}  // namespace
}  // namespace gsr

extern "C" size_t gsr_distortion_temp_bytes(int32_t num_gaussians) {
    return num_gaussians <= 0 ? 0 : sizeof(double) * (size_t)num_gaussians;
}
extern "C" int gsr_distortion_forward(gsr_distortion_args* a) { return gsr::entry_point(gsr::distortion_forward_impl, a); }
extern "C" int gsr_distortion_backward(gsr_distortion_args* a) { return gsr::entry_point(gsr::distortion_backward_impl, a); }
