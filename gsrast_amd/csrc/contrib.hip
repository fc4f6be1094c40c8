// Per-Gaussian contribution statistics of a frame (include/gsrast_amd_contrib.h): the replay of list_walk.hpp over the sorted
// lists a forward call left. alpha, T and every decision are the forward's bits; what the walk produces instead of a colour is,
// per blended record and pixel, q = (uint32)(alpha T 2^32), reduced over the wave's 256 pixels ON CHIP before anything goes to memory:
//   - a record's pixel count is the popcount of the lane masks its tests produce anyway;
//   - its sum and maximum of q are reduced across the lanes by DPP row shifts (18 vector issues per record that blended somewhere
//     in the tile, none for the others) and parked in the record's wave-private LDS slot;
//   - after the batch lane j files record j: at most ONE global atomic per array per staged record that blended anywhere in the tile;
//   - `dominant` is two registers per pixel (best q, its Gaussian) and, at the end of the tile, one add per distinct Gaussian of
//     a 16 x 4 strip.
// Only integer atomics (u64 add, u32 max): they commute, so the four arrays do not depend on the order anything arrives in.
#include "list_walk.hpp"
#include "../../include/gsrast_amd_contrib.h"

namespace gsr {
namespace {

struct ContribParams {
    WalkFrame frame;
    unsigned long long* weight_sum;
    uint32_t* weight_max;
    unsigned long long* pixels;
    unsigned long long* dominant;
};

// The replay's staging area, and what the wave found of each record.
struct ContribStage : ReplayStage {
    uint32_t id[kWave];                  // the record's Gaussian
    unsigned long long sum[kWave];       // sum of q over the tile's pixels
    uint32_t mx[kWave];                  // max of q
    uint32_t cnt[kWave];                 // pixels that blended it (0: nothing is filed)
};

// composite_record (blend_core.hpp) with the statistics in place of the colours. best / best_id: the pixel's largest q so far
// and its Gaussian (DOM).
template <bool DOM>
__device__ __forceinline__ void contrib_record(TileLanes& s, ContribStage& st, uint32_t j, int lane, bool need_sum, bool need_max,
                                               uint32_t (&best)[4], uint32_t (&best_id)[4]) {
    const ReplayRecord r = replay_candidates(s, st, j);
    if (!r.any()) return;
    const uint32_t id = st.id[j];
    uint32_t count = 0u;                       // wave-uniform
    unsigned long long lane_sum = 0ull;        // this lane's four pixels: < 2^34
    uint32_t lane_max = 0u;
    replay_blend(s, st, j, r, [&](const int k, const unsigned long long live, const float alpha) {
        count += (uint32_t)__popcll(live);
        if (__builtin_amdgcn_inverse_ballot_w64(live)) {
            const float w = alpha * s.T[k];
            const uint32_t qv = (uint32_t)(w * 4294967296.0f);
            lane_sum += qv;
            lane_max = lane_max > qv ? lane_max : qv;
            if constexpr (DOM) {
                if (qv > best[k]) { best[k] = qv; best_id[k] = id; }
            }
        }
    });
    if (count == 0u) return;
    // sum of up to 256 values below 2^32, as two 32-bit sums: the low 24 bits of the lanes' sums (64 of them: below 2^30) and the rest (below 2^16)
    unsigned long long total = 0ull;
    uint32_t top = 0u;
    if (need_sum) {
        const uint32_t lo = wave_reduce_u32((uint32_t)lane_sum & 0xFFFFFFu, AddU32{});
        const uint32_t hi = wave_reduce_u32((uint32_t)(lane_sum >> 24), AddU32{});
        total = (unsigned long long)lo + ((unsigned long long)hi << 24);
    }
    if (need_max) top = wave_reduce_u32(lane_max, MaxU32{});
    if (lane == 0) { st.sum[j] = total; st.mx[j] = top; st.cnt[j] = count; }
}

// (Measured on the bench frame with scripts/contrib_cost.py and not kept: the forward's slow-tiles-first order as the render
// backward takes it, and register bounds (amdgpu_waves_per_eu 8, 7 with `dominant`) that make all 8 160 tiles of a 1920 x 1080
// frame resident at once — the pass took 0.257 ms with both, 0.252 and 0.261 ms without (two runs): no difference beyond the
// spread between runs. It is bound by what a wave issues per record, not by its tail.)
template <bool DOM>
__global__ __launch_bounds__(kWave) void contrib_kernel(const ContribParams p) {
    __shared__ ContribStage st;
    const int lane = (int)threadIdx.x;
    int tx, ty;
    const int tile = walk_tile(p.frame, &tx, &ty);
    if (tile < 0) return;
    TileLanes s;
    tile_lanes_init(s, tx, ty, lane, p.frame.dims.width, p.frame.dims.height, -1);
    const bool need_sum = p.weight_sum != nullptr, need_max = p.weight_max != nullptr;
    uint32_t best[4] = {0u, 0u, 0u, 0u}, best_id[4] = {0u, 0u, 0u, 0u};
    replay_walk(p.frame, tile, tx, ty, lane, s, st, [&](const TileBox& box, const RecordBatch& b) {
        const uint32_t kept = stage_replay(box, st, b, p.frame.num_gaussians, [&](uint32_t slot, uint32_t id) { st.id[slot] = id; st.cnt[slot] = 0u; });
        for (uint32_t j = 0; j < kept; ++j) contrib_record<DOM>(s, st, j, lane, need_sum, need_max, best, best_id);
        // lane j files record j
        if ((uint32_t)lane < kept) {
            const uint32_t c = st.cnt[lane];
            if (c != 0u) {
                const uint32_t id = st.id[lane];
                if (need_sum) atomicAdd(&p.weight_sum[id], st.sum[lane]);
                if (need_max) atomicMax(&p.weight_max[id], st.mx[lane]);
                if (p.pixels) atomicAdd(&p.pixels[id], (unsigned long long)c);
            }
        }
    });
    if constexpr (DOM) {
        // one add per distinct Gaussian of a strip: the first of its lanes adds how many they are (no list: every best is 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned long long open = __ballot(best[k] != 0u);
            while (open != 0ull) {
                const int l = (int)__builtin_ctzll(open);
                const uint32_t u = (uint32_t)__builtin_amdgcn_readlane((int)best_id[k], l);
                const unsigned long long same = __ballot(best_id[k] == u) & open;
                if (lane == l) atomicAdd(&p.dominant[u], (unsigned long long)__popcll(same));
                open &= ~same;
            }
        }
    }
}

int contribution_impl(gsr_contribution_args* a) {
    if (!a || a->struct_size != sizeof(gsr_contribution_args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    if (a->num_gaussians <= 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!a->means2D || !a->conic_opacity || !a->ranges || !a->n_contrib) return GSR_ERR_INVALID_ARG;
    if (!a->weight_sum && !a->weight_max && !a->pixels && !a->dominant) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->weight_sum, 8) || misaligned(a->pixels, 8) || misaligned(a->dominant, 8) || misaligned(a->weight_max, 4) ||
        misaligned(a->means2D, 8) || misaligned(a->conic_opacity, 16) || misaligned(a->ranges, 8))
        return GSR_ERR_INVALID_ARG;
    const gsr_forward_receipt& r = a->receipt;
    const int grid_y = (a->height + kTile - 1) / kTile;
    if (r.tile_row_begin < 0 || r.tile_row_end > grid_y || r.tile_row_begin > r.tile_row_end) return GSR_ERR_INVALID_ARG;
    FrameDims d;
    bool nothing = false;
    GSR_TRY(walk_check(r, a->num_gaussians, a->width, a->height, r.tile_row_begin, r.tile_row_end, true, a->point_list, &d, &nothing));
    if (nothing) return GSR_OK;      // (nothing was blended: nothing is written)

    ContribParams p;
    p.frame = walk_frame(a->ranges, a->point_list, a->means2D, a->conic_opacity, a->n_contrib, nullptr, d, a->num_gaussians, r.num_rendered);
    p.weight_sum = reinterpret_cast<unsigned long long*>(a->weight_sum);
    p.weight_max = a->weight_max;
    p.pixels = reinterpret_cast<unsigned long long*>(a->pixels);
    p.dominant = reinterpret_cast<unsigned long long*>(a->dominant);
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;

    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (a->dominant) hipLaunchKernelGGL(contrib_kernel<true>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
    else hipLaunchKernelGGL(contrib_kernel<false>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
    GSR_LAUNCH_CHECK("contrib_kernel");
    return timer.end(stream, &a->stage_ms);
}

}  // namespace
}  // namespace gsr

extern "C" int gsr_contribution(gsr_contribution_args* a) { return gsr::entry_point(gsr::contribution_impl, a); }
