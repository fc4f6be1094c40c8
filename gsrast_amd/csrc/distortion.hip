// The depth distortion map of a drawn frame (include/gsrast_amd_distortion.h): 2 sum_i w_i sum_{j<i} w_j (m_i - m_j)^q per pixel
// over the sorted lists a forward call left, w = alpha T, and its gradient — passes of their own on the walks of list_walk.hpp,
// as features.hip's are, so that the blend, contrib_kernel and render_backward_kernel keep their object code. One wavefront per
// 16 x 16 tile, the record's value m staged in wave-private LDS beside the record:
//   - distortion_forward_kernel is the replay: per pixel the prefix moments M1 = sum w d, M2 = sum w d^2 of the values centred on
//     the pixel's first blended record (d = m - m0), and D = sum w e with e the record's distance to everything in front of it.
//     It leaves out = 2 D and the three planes m0, M1, M2 the backward reads.
//   - distortion_backward_kernel is the back walk: with the pixel's totals every record's d out / d w (c) and d out / d m come
//     from what the pixel read once; dL_dalpha = g (Tn c - S inv) with S the suffix sum of c w, and from there (GEO) the walk's
//     GeometrySums: the render backward's own lines, added into the double sums a gsr_backward of the same frame then reads.
//     Without GEO neither c nor S is formed.
// A record's value sum rides in the seventh input of the wave_sum8 that carries the six geometry sums (GeometrySums::file's
// `extra`): two reductions a record, as in features.hip.
#include <hip/hip_runtime.h>

#include "list_walk.hpp"
#include "../../include/gsrast_amd_distortion.h"

namespace gsr {
namespace {

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

    [[maybe_unused]] const bool files_value = sum8_of_lane(lane) == GeometrySums::kExtra;      // (GEO: the record's value sum rides there)

    BackLanes s;
    float g[4] = {}, m0[4] = {}, M1n[4] = {};
    [[maybe_unused]] float M2n[4] = {};
    [[maybe_unused]] float An[4], Tf[4], Tb[4], Ms[4], S[4];
    // the record in hand: its value and this lane's sums over its four pixels
    float m = 0.0f, a_v = 0.0f;
    [[maybe_unused]] GeometrySums geo(lane);
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
            if constexpr (GEO) geo.clear();
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
                const float dL_dalpha = g[k] * __builtin_fmaf(px.Tn, c, -(S[k] * px.inv));
                S[k] = __builtin_fmaf(c, px.w, S[k]);
                geo.add(px, dL_dalpha);
            }
        },
        /* file */ [&](const int j) {
            const size_t id = st.id[j];
            if constexpr (GEO) {
                const float total = geo.file(p.geometry_sums, id, lane, a_v);
                if (files_value && total != 0.0f) unsafeAtomicAdd(p.value_sums + id, (double)total);
            } else {
                const float total = wave_sum2(a_v, 0.0f);            // (lane 31 holds the total of the first)
                if (lane == 31 && total != 0.0f) unsafeAtomicAdd(p.value_sums + id, (double)total);
            }
        });
}

// What both calls check beside walk_pass_check; *nothing: no record to walk (R == 0 or an empty band).
int distortion_check(gsr_distortion_args* a, bool backward, FrameDims* d, bool* nothing) {
    GSR_TRY(walk_pass_check(a, d, nothing));
    if (a->power != 1 && a->power != 2) return GSR_ERR_INVALID_ARG;
    if (!a->values || !a->moments) return GSR_ERR_INVALID_ARG;
    if (backward ? (!a->dL_dout || !a->dL_dvalues || !a->value_sums_f64) : !a->out) return GSR_ERR_INVALID_ARG;
    if (backward && (misaligned(a->value_sums_f64, 8) || misaligned(a->geometry_sums_f64, 8))) return GSR_ERR_INVALID_ARG;
    return GSR_OK;
}

DistortionParams distortion_params(const gsr_distortion_args* a, const WalkFrame& frame) {
    DistortionParams p;
    p.frame = frame;
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
    return walk_pass_call(a, d, nothing, nullptr, [&](const WalkFrame& frame, unsigned blocks, hipStream_t stream) {
        const DistortionParams p = distortion_params(a, frame);
        const dim3 grid(blocks);
        if (a->power == 2) hipLaunchKernelGGL(distortion_forward_kernel<2>, grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL(distortion_forward_kernel<1>, grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("distortion_forward_kernel");
        return GSR_OK;
    });
}

int distortion_backward_impl(gsr_distortion_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(distortion_check(a, true, &d, &nothing));
    const WalkSums sums = {(size_t)a->num_gaussians, a->value_sums_f64, a->dL_dvalues};
    return walk_pass_call(a, d, nothing, &sums, [&](const WalkFrame& frame, unsigned blocks, hipStream_t stream) {
        const DistortionParams p = distortion_params(a, frame);
        const bool square = a->power == 2, geo = a->geometry_sums_f64 != nullptr;
        const dim3 grid(blocks);
        if (square && geo) hipLaunchKernelGGL((distortion_backward_kernel<2, true>), grid, dim3(kWave), 0, stream, p);
        else if (square) hipLaunchKernelGGL((distortion_backward_kernel<2, false>), grid, dim3(kWave), 0, stream, p);
        else if (geo) hipLaunchKernelGGL((distortion_backward_kernel<1, true>), grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL((distortion_backward_kernel<1, false>), grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("distortion_backward_kernel");
        return GSR_OK;
    });
}

}  // namespace
}  // namespace gsr

extern "C" size_t gsr_distortion_temp_bytes(int32_t num_gaussians) {
    return num_gaussians <= 0 ? 0 : sizeof(double) * (size_t)num_gaussians;
}
extern "C" int gsr_distortion_forward(gsr_distortion_args* a) { return gsr::entry_point(gsr::distortion_forward_impl, a); }
extern "C" int gsr_distortion_backward(gsr_distortion_args* a) { return gsr::entry_point(gsr::distortion_backward_impl, a); }
