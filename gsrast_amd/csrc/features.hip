// N-channel feature maps of a drawn frame (include/gsrast_amd_features.h): sum_i f_i alpha_i T_i per pixel over the sorted lists a
// forward call left, and its gradient — passes of their own, so that the blend, contrib_kernel and render_backward_kernel keep
// their object code. Both kernels are one wavefront per (16 x 16 tile, chunk of K channels) on the walks of list_walk.hpp, the
// survivors' K feature floats staged in wave-private LDS beside their records:
//   - features_forward_kernel is the replay: what a blended (record, pixel) adds is composite_record's acc = fmaf(f, alpha T, acc)
//     per channel, and a pixel leaves as tile_lanes_write forms it, acc + final_t bg. With the frame's colours and background
//     that is out_color bit for bit.
//   - features_backward_kernel is the back walk, and from dL_dalpha on (GEO) the walk's GeometrySums: the render backward's own
//     lines, added into the double sums a gsr_backward of the same frame then reads. Without GEO neither cg nor the suffix
//     sum S is formed: w g is all a frozen geometry needs.
// A record's K feature sums are reduced eight at a time by the fold-and-pack of backward.hip's wave_sum12 (three lane swaps
// pack eight values into one register, four DPP steps finish: 8 sums for the price of about 2 separate ones) and leave as ONE
// double atomic instruction per eight channels, eight lanes on 64 contiguous bytes of feature_sums_f64.
#include <hip/hip_runtime.h>

#include "list_walk.hpp"
#include "../../include/gsrast_amd_features.h"

namespace gsr {
namespace {

// The chunk width K is a template parameter with two instances: the narrow one serves calls of up to that many channels
// (normals, a label: C = 3 pays for 8 accumulators per pixel, not 16), the wide one every other call. The widths were chosen
// by measuring 8, 16 and 24 on the bench frame: DESIGN.md section 8 has the table, profiles/features_cost.txt the kernels as built.
constexpr int kChunkNarrow = GSR_FEATURES_CHUNK_NARROW, kChunkWide = GSR_FEATURES_CHUNK;
static_assert(kChunkNarrow % 8 == 0 && kChunkNarrow >= 8 && kChunkWide % 8 == 0 && kChunkWide >= kChunkNarrow && kChunkWide <= 32,
              "the reduction packs eight sums per register");
inline int chunk_of(int channels) { return channels <= kChunkNarrow ? kChunkNarrow : kChunkWide; }

struct FeatureParams {
    WalkFrame frame;
    const float* features;        // f32[N C]
    const float* background;      // f32[C] or null
    float* out;                   // forward: f32[C W H]
    const float* dL_dout;         // backward: f32[C W H]
    double* feature_sums;         // backward: f64[N C]
    double* geometry_sums;        // backward (GEO): f64[12 N]
    uint32_t channels;
};

// A record's K features of one chunk into its staging slot (16-byte aligned: slots are K floats apart), zeros past the call's
// last channel. The row in memory is only known to lie on a 4-byte boundary (C is any number), so it is read float by float;
// the slot is written four floats per LDS instruction.
template <int K>
__device__ __forceinline__ void stage_feature_row(float* slot, const float* row, uint32_t nc) {
#pragma unroll
    for (int c = 0; c < K; c += 4) {
        float4 v;
        v.x = (uint32_t)c < nc ? row[c] : 0.0f;
        v.y = (uint32_t)(c + 1) < nc ? row[c + 1] : 0.0f;
        v.z = (uint32_t)(c + 2) < nc ? row[c + 2] : 0.0f;
        v.w = (uint32_t)(c + 3) < nc ? row[c + 3] : 0.0f;
        *reinterpret_cast<float4*>(slot + c) = v;
    }
}
// ... and back out of it, into registers
template <int K>
__device__ __forceinline__ void load_feature_row(float (&feat)[K], const float* slot) {
#pragma unroll
    for (int c = 0; c < K; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(slot + c);
        feat[c] = v.x; feat[c + 1] = v.y; feat[c + 2] = v.z; feat[c + 3] = v.w;
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <int K>
struct FeatureStage : ReplayStage {
    float feat[kWave * K];               // a record's K features (zeros past the last channel)
};

template <int K>
__global__ __launch_bounds__(kWave) void features_forward_kernel(const FeatureParams p) {
    __shared__ FeatureStage<K> st;
    const int lane = (int)threadIdx.x;
    int tx, ty;
    const int tile = walk_tile(p.frame, &tx, &ty);
    if (tile < 0) return;
    const uint32_t c0 = blockIdx.y * (uint32_t)K, nc = min((uint32_t)K, p.channels - c0);
    const size_t plane = (size_t)p.frame.dims.width * (size_t)p.frame.dims.height;

    TileLanes s;
    tile_lanes_init(s, tx, ty, lane, p.frame.dims.width, p.frame.dims.height, -1);
    float acc[4][K];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < K; ++c) acc[k][c] = 0.0f;

    const bool has_list = replay_walk(p.frame, tile, tx, ty, lane, s, st, [&](const TileBox& box, const RecordBatch& b) {
        const uint32_t kept = stage_replay(box, st, b, p.frame.num_gaussians, [&](uint32_t slot, uint32_t id) {
            stage_feature_row<K>(&st.feat[slot * K], p.features + (size_t)id * (size_t)p.channels + c0, nc);
        });
        for (uint32_t j = 0; j < kept; ++j) {
            const ReplayRecord r = replay_candidates(s, st, j);
            if (!r.any()) continue;
            float feat[K];
            load_feature_row<K>(feat, &st.feat[j * K]);
            replay_blend(s, st, j, r, [&](const int k, const unsigned long long live, const float alpha) {
                if (__builtin_amdgcn_inverse_ballot_w64(live)) {
                    const float w = alpha * s.T[k];
#pragma unroll
                    for (int c = 0; c < K; ++c) acc[k][c] = __builtin_fmaf(feat[c], w, acc[k][c]);
                }
            });
        }
    });
    // tile_lanes_write's expression per channel: acc + final_t bg (a tile without a list: 0 + 1 bg)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!s.inside[k]) continue;
        const size_t pid = (size_t)(s.py0 + 4 * k) * (size_t)p.frame.dims.width + (size_t)s.px;
        const float tf = has_list ? p.frame.final_t[pid] : 1.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if ((uint32_t)c >= nc) continue;
            float* dst = p.out + (size_t)(c0 + (uint32_t)c) * plane + pid;
            if (p.background) *dst = acc[k][c] + tf * p.background[c0 + (uint32_t)c];
            else *dst = acc[k][c];
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
template <int K, bool GEO>
__global__ __launch_bounds__(kWave) void features_backward_kernel(const FeatureParams p) {
    __shared__ BackStage st;
    __shared__ __attribute__((aligned(16))) float s_feat[kWave * K];      // (GEO; unused and not allocated without)
    const int lane = threadIdx.x;
    int tx, ty;
    const int tile = walk_tile(p.frame, &tx, &ty);
    if (tile < 0) return;
    const size_t plane = (size_t)p.frame.dims.width * (size_t)p.frame.dims.height;
    const uint32_t c0 = blockIdx.y * (uint32_t)K, nc = min((uint32_t)K, p.channels - c0);

    const int my_feat = sum8_of_lane(lane);        // which of a reduction's eight channel sums this lane files

    BackLanes s;
    float g[4][K] = {};
    [[maybe_unused]] float S[4];
    // the record in hand: its features (GEO) and this lane's sums over its four pixels
    float a_f[K];
    [[maybe_unused]] float feat[K];
    [[maybe_unused]] GeometrySums geo(lane);
    back_walk<true>(
        p.frame, tile, tx, ty, lane, s, st,
        /* seed */ [&](const int k, const size_t pid) {
#pragma unroll
            for (int c = 0; c < K; ++c)
                if ((uint32_t)c < nc) g[k][c] = p.dL_dout[(size_t)(c0 + (uint32_t)c) * plane + pid];
        },
        /* start */ [&]() {
            if constexpr (GEO) {
                // what lies behind, dotted with this chunk's dL/dout: S = T_f sum_c bg_c g_c
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float bgg = 0.0f;
                    if (p.background) {
#pragma unroll
                        for (int c = 0; c < K; ++c)
                            if ((uint32_t)c < nc) bgg = __builtin_fmaf(p.background[c0 + (uint32_t)c], g[k][c], bgg);
                    }
                    S[k] = s.T[k] * bgg;
                }
            }
        },
        /* payload */ [&](const uint32_t slot, const uint32_t id) {
            // (without GEO the features themselves are not needed: dL_dfeatures is sum w g)
            if constexpr (GEO) stage_feature_row<K>(&s_feat[slot * K], p.features + (size_t)id * (size_t)p.channels + c0, nc);
        },
        /* begin */ [&](const int j) {
#pragma unroll
            for (int c = 0; c < K; ++c) a_f[c] = 0.0f;
            if constexpr (GEO) {
                load_feature_row<K>(feat, &s_feat[j * K]);
                geo.clear();
            }
        },
        /* on_pixel */ [&](const int k, const BackPixel& px) {
#pragma unroll
            for (int c = 0; c < K; ++c) a_f[c] = __builtin_fmaf(px.w, g[k][c], a_f[c]);
            if constexpr (GEO) {
                float cg = feat[K - 1] * g[k][K - 1];
#pragma unroll
                for (int c = K - 2; c >= 0; --c) cg = __builtin_fmaf(feat[c], g[k][c], cg);
                const float dL_dalpha = __builtin_fmaf(px.Tn, cg, -(S[k] * px.inv));
                S[k] = __builtin_fmaf(cg, px.w, S[k]);
                geo.add(px, dL_dalpha);
            }
        },
        /* file */ [&](const int j) {
            const size_t id = st.id[j];
            // eight channels per reduction, one atomic instruction with eight lanes on 64 contiguous bytes
#pragma unroll
            for (int c = 0; c < K; c += 8) {
                const float total = wave_sum8(a_f[c], a_f[c + 1], a_f[c + 2], a_f[c + 3], a_f[c + 4], a_f[c + 5], a_f[c + 6], a_f[c + 7], lane);
                if (my_feat >= 0 && (uint32_t)(c + my_feat) < nc && total != 0.0f)
                    unsafeAtomicAdd(p.feature_sums + id * (size_t)p.channels + c0 + (uint32_t)(c + my_feat), (double)total);
            }
            if constexpr (GEO) geo.file(p.geometry_sums, id, lane, 0.0f);
        });
}

// What both calls check beside walk_pass_check; *nothing: no record to walk (R == 0 or an empty band).
int features_check(gsr_features_args* a, bool backward, FrameDims* d, bool* nothing) {
    GSR_TRY(walk_pass_check(a, d, nothing));
    if (a->channels < 1 || a->channels > GSR_FEATURES_MAX_CHANNELS) return GSR_ERR_INVALID_ARG;
    if (!a->features) return GSR_ERR_INVALID_ARG;
    if (backward ? (!a->dL_dout || !a->dL_dfeatures || !a->feature_sums_f64) : !a->out) return GSR_ERR_INVALID_ARG;
    if (backward && (misaligned(a->feature_sums_f64, 8) || misaligned(a->geometry_sums_f64, 8))) return GSR_ERR_INVALID_ARG;
    return GSR_OK;
}

FeatureParams feature_params(const gsr_features_args* a, const WalkFrame& frame) {
    FeatureParams p;
    p.frame = frame;
    p.features = a->features;
    p.background = a->background;
    p.out = a->out;
    p.dL_dout = a->dL_dout;
    p.feature_sums = a->feature_sums_f64;
    p.geometry_sums = a->geometry_sums_f64;
    p.channels = (uint32_t)a->channels;
    return p;
}

int features_forward_impl(gsr_features_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(features_check(a, false, &d, &nothing));
    return walk_pass_call(a, d, nothing, nullptr, [&](const WalkFrame& frame, unsigned blocks, hipStream_t stream) {
        const FeatureParams p = feature_params(a, frame);
        const int k = chunk_of(a->channels);
        const dim3 grid(blocks, (unsigned)((a->channels + k - 1) / k));
        if (k == kChunkNarrow) hipLaunchKernelGGL(features_forward_kernel<kChunkNarrow>, grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL(features_forward_kernel<kChunkWide>, grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("features_forward_kernel");
        return GSR_OK;
    });
}

int features_backward_impl(gsr_features_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(features_check(a, true, &d, &nothing));
    const WalkSums sums = {(size_t)a->num_gaussians * (size_t)a->channels, a->feature_sums_f64, a->dL_dfeatures};
    return walk_pass_call(a, d, nothing, &sums, [&](const WalkFrame& frame, unsigned blocks, hipStream_t stream) {
        const FeatureParams p = feature_params(a, frame);
        const int k = chunk_of(a->channels);
        const bool narrow = k == kChunkNarrow, geo = a->geometry_sums_f64 != nullptr;
        const dim3 grid(blocks, (unsigned)((a->channels + k - 1) / k));
        if (narrow && geo) hipLaunchKernelGGL((features_backward_kernel<kChunkNarrow, true>), grid, dim3(kWave), 0, stream, p);
        else if (narrow) hipLaunchKernelGGL((features_backward_kernel<kChunkNarrow, false>), grid, dim3(kWave), 0, stream, p);
        else if (geo) hipLaunchKernelGGL((features_backward_kernel<kChunkWide, true>), grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL((features_backward_kernel<kChunkWide, false>), grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("features_backward_kernel");
        return GSR_OK;
    });
}

}  // namespace
}  // namespace gsr

extern "C" size_t gsr_features_temp_bytes(int32_t num_gaussians, int32_t channels) {
    if (num_gaussians <= 0 || channels < 1 || channels > GSR_FEATURES_MAX_CHANNELS) return 0;
    return sizeof(double) * (size_t)num_gaussians * (size_t)channels;
}
extern "C" int gsr_features_forward(gsr_features_args* a) { return gsr::entry_point(gsr::features_forward_impl, a); }
extern "C" int gsr_features_backward(gsr_features_args* a) { return gsr::entry_point(gsr::features_backward_impl, a); }
