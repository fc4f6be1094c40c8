// The median depth map of a drawn frame and the per-pixel Gaussian ids (include/gsrast_amd_median.h): per pixel the record in
// front of which the transmittance is last above a threshold, its value gathered, and the record with the largest blending
// weight — a pass of its own on the replay of list_walk.hpp, as contrib.hip's and distortion.hip's are, so that the blend and
// the other walks keep their object code. One wavefront per 16 x 16 tile:
//   - median_forward_kernel is the replay with two (DOM: four) registers per pixel and nothing staged beside a record but its
//     id: no payload, no sums, no reduction. A pixel that has crossed the threshold — and, DOM, that no later weight can win —
//     takes itself out of the walk by zeroing its s.last[k]; once every pixel of the tile has, the remaining batches are skipped.
//   - median_backward_kernel is no list walk: a tile's pixels read their id and gradient, the lanes of a 16 x 4 strip that hold
//     the same id are added in double on chip (the loop over distinct ids at the end of contrib_kernel<true>), and one double
//     atomic per distinct id and strip goes to the sums finish_sums_kernel<1> then rounds once.
#include <hip/hip_runtime.h>

#include "list_walk.hpp"
#include "../../include/gsrast_amd_median.h"

namespace gsr {
namespace {

struct MedianParams {
    WalkFrame frame;
    const float* values;          // f32[N] or null (no out)
    float threshold;
    float* out;                   // f32[W H] or null
    uint32_t* ids;                // u32[W H] or null
    uint32_t* dominant_ids;       // u32[W H] (DOM)
};

struct MedianStage : ReplayStage {
    uint32_t id[kWave];                  // the record's Gaussian
};

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <bool DOM>
__global__ __launch_bounds__(kWave) void median_forward_kernel(const MedianParams p) {
    __shared__ MedianStage st;
    const int lane = (int)threadIdx.x;
    int tx, ty;
    const int tile = walk_tile(p.frame, &tx, &ty);
    if (tile < 0) return;

    TileLanes s;
    tile_lanes_init(s, tx, ty, lane, p.frame.dims.width, p.frame.dims.height, -1);
    const float threshold = p.threshold;
    uint32_t sel[4] = {GSR_MEDIAN_NONE, GSR_MEDIAN_NONE, GSR_MEDIAN_NONE, GSR_MEDIAN_NONE};
    [[maybe_unused]] uint32_t best[4] = {0u, 0u, 0u, 0u};
    [[maybe_unused]] uint32_t dom[4] = {GSR_MEDIAN_NONE, GSR_MEDIAN_NONE, GSR_MEDIAN_NONE, GSR_MEDIAN_NONE};
    bool open = true;                    // wave-uniform: some pixel of the tile is still in the walk

    replay_walk(p.frame, tile, tx, ty, lane, s, st, [&](const TileBox& box, const RecordBatch& b) {
        if (!open) return;
        const uint32_t kept = stage_replay(box, st, b, p.frame.num_gaussians, [&](uint32_t slot, uint32_t id) { st.id[slot] = id; });
        for (uint32_t j = 0; j < kept; ++j) {
            const ReplayRecord r = replay_candidates(s, st, j);
            if (!r.any()) continue;
            const uint32_t id = st.id[j];
            replay_blend(s, st, j, r, [&](const int k, const unsigned long long live, const float alpha) {
                if (__builtin_amdgcn_inverse_ballot_w64(live)) {
                    const float T = s.T[k];
                    if (T > threshold) sel[k] = id;
                    const float Tn = T * (1.0f - alpha);              // (what replay_blend leaves in s.T[k] behind this call)
                    bool leave = !(Tn > threshold);                   // T does not rise again: no later record is selected
                    if constexpr (DOM) {
                        const float w = alpha * T;
                        const uint32_t qv = (uint32_t)(w * 4294967296.0f);
                        if (qv > best[k]) { best[k] = qv; dom[k] = id; }
                        // alpha <= 0.99 and T <= Tn from here on, and float multiplication is monotone: no later q exceeds this
                        leave = leave && (uint32_t)((0.99f * Tn) * 4294967296.0f) <= best[k];
                    }
                    if (leave) s.last[k] = 0u;                        // no later record is a candidate of this pixel
                }
            });
        }
        open = __ballot((s.last[0] | s.last[1] | s.last[2] | s.last[3]) != 0u) != 0ull;
    });
    // (a tile without a list, a pixel nothing was blended into: NONE, as the registers started)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!s.inside[k]) continue;
        const size_t pid = (size_t)(s.py0 + 4 * k) * (size_t)p.frame.dims.width + (size_t)s.px;
        if (p.ids) p.ids[pid] = sel[k];
        if constexpr (DOM) p.dominant_ids[pid] = dom[k];
        if (p.out) p.out[pid] = sel[k] == GSR_MEDIAN_NONE ? 0.0f : p.values[sel[k]];      // (sel < N: stage_replay drops the others)
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
struct MedianBackParams {
    FrameDims dims;
    uint32_t num_gaussians;
    const uint32_t* ids;          // u32[W H]
    const float* dL_dout;         // f32[W H]
    double* value_sums;           // f64[N]
};

__global__ __launch_bounds__(kWave) void median_backward_kernel(const MedianBackParams p) {
    const int lane = (int)threadIdx.x;
    const int tile_local = tile_of_workgroup((int)blockIdx.x, p.dims.grid_x, p.dims.row_end - p.dims.row_begin);
    if (tile_local < 0) return;
    const int tile = p.dims.row_begin * p.dims.grid_x + tile_local;
    const int px = (tile % p.dims.grid_x) * kTile + (lane & 15), py0 = (tile / p.dims.grid_x) * kTile + (lane >> 4);
    uint32_t id[4];
    float g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = py0 + 4 * k;
        id[k] = GSR_MEDIAN_NONE;
        g[k] = 0.0f;
        if (px < p.dims.width && py < p.dims.height) {
            const size_t pid = (size_t)py * (size_t)p.dims.width + (size_t)px;
            id[k] = p.ids[pid];
            g[k] = p.dL_dout[pid];
        }
    }
    // one add per distinct Gaussian of a strip: the first of its lanes adds the double sum of all of them
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned long long open = __ballot(id[k] < p.num_gaussians);
        while (open != 0ull) {
            const int l = (int)__builtin_ctzll(open);
            const uint32_t u = (uint32_t)__builtin_amdgcn_readlane((int)id[k], l);
            const unsigned long long same = __ballot(id[k] == u) & open;
            double v = ((same >> lane) & 1ull) ? (double)g[k] : 0.0;
            if (__popcll(same) > 1) {                                 // (wave-uniform)
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
            }
            if (lane == l && v != 0.0) unsafeAtomicAdd(p.value_sums + u, v);
            open &= ~same;
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// walk_pass_check with one difference: the call's band of tile rows may be any band INSIDE the receipt's (a tile's list is walked
// on its own, so a part of the frame the forward call drew is as good as the whole: SplatRasterizer.pick walks one row).
int median_forward_check(gsr_median_args* a, FrameDims* d, bool* nothing) {
    if (!a || a->struct_size != sizeof(gsr_median_args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    if (a->num_gaussians <= 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!a->means2D || !a->conic_opacity || !a->ranges || !a->n_contrib || !a->final_t) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->means2D, 8) || misaligned(a->conic_opacity, 16) || misaligned(a->ranges, 8)) return GSR_ERR_INVALID_ARG;
    const gsr_forward_receipt& r = a->receipt;
    FrameDims band;
    if (tile_band(a->width, a->height, a->tile_row_begin, a->tile_row_end, &band) != GSR_OK) return GSR_ERR_INVALID_ARG;
    if (r.tile_row_begin < 0 || r.tile_row_end > band.grid_y || r.tile_row_begin > r.tile_row_end) return GSR_ERR_INVALID_ARG;
    GSR_TRY(walk_check(r, a->num_gaussians, a->width, a->height, r.tile_row_begin, r.tile_row_end, true, a->point_list, d, nothing));
    if (band.row_begin < d->row_begin || band.row_end > d->row_end) return GSR_ERR_INVALID_ARG;
    d->row_begin = band.row_begin;
    d->row_end = band.row_end;
    *nothing = r.num_rendered == 0 || d->row_begin == d->row_end;
    return GSR_OK;
}

int median_forward_impl(gsr_median_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(median_forward_check(a, &d, &nothing));
    if (!(a->threshold >= 0.0f && a->threshold < 1.0f)) return GSR_ERR_INVALID_ARG;         // (a NaN fails both)
    if (!a->out && !a->ids && !a->dominant_ids) return GSR_ERR_INVALID_ARG;
    if (a->out && !a->values) return GSR_ERR_INVALID_ARG;
    return walk_pass_call(a, d, nothing, nullptr, [&](const WalkFrame& frame, unsigned blocks, hipStream_t stream) {
        MedianParams p;
        p.frame = frame;
        p.values = a->values;
        p.threshold = a->threshold;
        p.out = a->out;
        p.ids = a->ids;
        p.dominant_ids = a->dominant_ids;
        if (a->dominant_ids) hipLaunchKernelGGL(median_forward_kernel<true>, dim3(blocks), dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL(median_forward_kernel<false>, dim3(blocks), dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("median_forward_kernel");
        return GSR_OK;
    });
}

// Reads nothing of the frame and does not look at the receipt: the ids are the forward call's, whatever was drawn since.
int median_backward_impl(gsr_median_args* a) {
    if (!a || a->struct_size != sizeof(gsr_median_args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    if (a->num_gaussians <= 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!a->ids || !a->dL_dout || !a->dL_dvalues || !a->value_sums_f64) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->value_sums_f64, 8)) return GSR_ERR_INVALID_ARG;
    MedianBackParams p;
    if (tile_band(a->width, a->height, a->tile_row_begin, a->tile_row_end, &p.dims) != GSR_OK) return GSR_ERR_INVALID_ARG;
    const long long blocks = patch_workgroups(p.dims.grid_x, p.dims.row_end - p.dims.row_begin);
    if (exceeds_grid(blocks) || exceeds_grid(finish_sums_workgroups((size_t)a->num_gaussians))) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----
    p.num_gaussians = (uint32_t)a->num_gaussians;
    p.ids = a->ids;
    p.dL_dout = a->dL_dout;
    p.value_sums = a->value_sums_f64;
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (p.dims.row_begin != p.dims.row_end) {
        hipLaunchKernelGGL(median_backward_kernel, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("median_backward_kernel");
    }
    GSR_TRY(launch_finish_sums<1>((size_t)a->num_gaussians, a->value_sums_f64, a->dL_dvalues, stream));
    return timer.end(stream, &a->stage_ms);
}

}  // namespace
}  // namespace gsr

extern "C" size_t gsr_median_temp_bytes(int32_t num_gaussians) {
    return num_gaussians <= 0 ? 0 : sizeof(double) * (size_t)num_gaussians;
}
extern "C" int gsr_median_forward(gsr_median_args* a) { return gsr::entry_point(gsr::median_forward_impl, a); }
extern "C" int gsr_median_backward(gsr_median_args* a) { return gsr::entry_point(gsr::median_backward_impl, a); }
