// Per-Gaussian contribution statistics of a frame (include/gsrast_amd_contrib.h): one more front-to-back walk over the sorted
// lists a forward call left, one wavefront per 16 x 16 tile, four pixels per lane as the forward blend lays them out
// (blend_core.hpp: TileLanes, the staging with the footprint cull, the filter in front of the reference's arithmetic, exp_ref).
// alpha, T and every decision are the forward's bits; what the walk produces instead of a colour is, per blended record and
// pixel, q = (uint32)(alpha T 2^32), reduced over the wave's 256 pixels ON CHIP before anything goes to memory:
//   - a record's pixel count is the popcount of the lane masks its tests produce anyway;
//   - its sum and maximum of q are reduced across the lanes by DPP row shifts (18 vector issues per record that blended somewhere
//     in the tile, none for the others) and parked in the record's wave-private LDS slot;
//   - after the batch lane j files record j: at most ONE global atomic per array per staged record that blended anywhere in the tile;
//   - `dominant` is two registers per pixel (best q, its Gaussian) and, at the end of the tile, one add per distinct Gaussian of
//     a 16 x 4 strip.
// Only integer atomics (u64 add, u32 max): they commute, so the four arrays do not depend on the order anything arrives in.
//
// Which pixels take part in list position k comes from n_contrib, not from replaying the cut-off test: a pixel blends the
// records that pass the power and alpha tests up to and including its last contributor (the render backward's rule), and the
// wave-reduced maximum of n_contrib bounds the walk — a tile whose pixels all saturated after 300 records of a 30 000-record list
// is left after 300.
#include "blend_core.hpp"
#include "blockbin.hpp"          // (lists_of_receipt)
#include "../../include/gsrast_amd_contrib.h"

namespace gsr {
namespace {

struct ContribParams {
    const uint2* ranges;
    const uint32_t* point_list;
    const float2* means2D;
    const float4* conic_opacity;
    const uint32_t* n_contrib;
    unsigned long long* weight_sum;
    uint32_t* weight_max;
    unsigned long long* pixels;
    unsigned long long* dominant;
    FrameDims dims;
    uint32_t num_gaussians;
    uint32_t num_rendered;
};

// One wave's staging area (wave-private LDS: no barrier): the survivors of a batch of 64 list entries, compacted, and what
// the wave found of each.
struct ContribStage {
    float2 xy[kWave];
    float4 co[kWave];                    // the filter's pre-scaled conic and floor (StagedRecords::co)
    float4 raw[kWave];                   // conic + opacity as fetched
    uint32_t id[kWave];                  // the record's Gaussian
    uint32_t number[kWave];              // its 1-based position in the tile's list
    unsigned long long sum[kWave];       // sum of q over the tile's pixels
    uint32_t mx[kWave];                  // max of q
    uint32_t cnt[kWave];                 // pixels that blended it (0: nothing is filed)
    unsigned long long exp_tab[32];
};

// Reductions over the 64 lanes by DPP (the shifts of blockbin.hpp's prefix32_inclusive: lanes 31 and 63 end up with their
// halves' results; lanes without a source read 0, the identity of both operations on unsigned values). Wave-uniform result.
template <typename Op>
__device__ __forceinline__ uint32_t wave_reduce_u32(uint32_t v, Op op) {
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    return op((uint32_t)__builtin_amdgcn_readlane((int)v, 31), (uint32_t)__builtin_amdgcn_readlane((int)v, 63));
}
struct AddU32 { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct MaxU32 { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };

// stage_batch (blend_core.hpp) without the colours: the same footprint test, the same filter conic, floor and margins, so that
// the candidates of a record are the forward's. A list entry that names no Gaussian of the scene is dropped.
__device__ __forceinline__ uint32_t stage_contrib(const TileFeed& f, ContribStage& st, const RecordBatch& b, uint32_t num_gaussians) {
    const bool present = b.present() && b.id < num_gaussians;
    const uint32_t rank = b.rank(), pos = b.pos;
    const bool keep = present && !record_misses_tile(b.xy, b.co, f.box);
    const unsigned long long m2 = __ballot(keep);
    if (keep) {
        const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0u));
        const float dxm = fmaxf(fabsf(b.xy.x - f.box.x_lo), fabsf(b.xy.x - f.box.x_hi)), dym = fmaxf(fabsf(b.xy.y - f.box.y_lo), fabsf(b.xy.y - f.box.y_hi));
        const float terms = fabsf(b.co.x) * dxm * dxm + fabsf(b.co.z) * dym * dym + 2.0f * fabsf(b.co.y) * dxm * dym;
        const float p0 = -__logf(255.0f * b.co.w);
        const float floor2 = !(b.co.w > -__builtin_inff()) ? -__builtin_inff() : (b.co.w <= 0.0f ? __builtin_inff() : (p0 - 1e-3f - 1e-6f * terms) * kLog2e);
        const bool filtered = terms < 1.0e6f;                                   // (NaN: not filtered)
        st.xy[slot] = b.xy;
        st.co[slot] = filtered ? make_float4((-0.5f * kLog2e) * b.co.x, -kLog2e * b.co.y, (-0.5f * kLog2e) * b.co.z, floor2)
                               : make_float4(0.0f, 0.0f, 0.0f, -__builtin_inff());
        st.raw[slot] = b.co;
        st.id[slot] = b.id;
        st.number[slot] = pos + rank + 1u;
        st.cnt[slot] = 0u;
    }
    return (uint32_t)__popcll(m2);
}

// composite_record (blend_core.hpp) with the statistics in place of the colours. s.last[k] holds the pixel's n_contrib; best /
// best_id: the pixel's largest q so far and its Gaussian (DOM).
template <bool DOM>
__device__ __forceinline__ void contrib_record(TileLanes& s, ContribStage& st, uint32_t j, int lane, bool need_sum, bool need_max,
                                               uint32_t (&best)[4], uint32_t (&best_id)[4]) {
    constexpr float kAlphaMin = 1.0f / 255.0f;
    const float2 xy = st.xy[j];
    const float4 q = st.co[j];
    const uint32_t number = st.number[j];
    const float dx = xy.x - s.fx;
    const float h0 = (q.x * dx) * dx;
    const float g = q.y * dx;
    f32x2 gy; gy.x = xy.y; gy.y = xy.y;
    f32x2 gg; gg.x = g; gg.y = g;
    f32x2 hh; hh.x = h0; hh.y = h0;
    f32x2 cz; cz.x = q.z; cz.y = q.z;
    const f32x2 dy01 = gy - s.fy01, dy23 = gy - s.fy23;
    const f32x2 fw01 = __builtin_elementwise_fma(dy01, __builtin_elementwise_fma(cz, dy01, gg), hh);
    const f32x2 fw23 = __builtin_elementwise_fma(dy23, __builtin_elementwise_fma(cz, dy23, gg), hh);
    const float filter[4] = {fw01.x, fw01.y, fw23.x, fw23.y};
    // the forward's candidates (a pixel outside the image has a NaN row coordinate) that have not yet had their last contributor
    unsigned long long cand[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        cand[k] = __ballot(filter[k] <= kFilterSlack * kLog2e) & __ballot(filter[k] >= q.w) & __ballot(number <= s.last[k]);
    if ((cand[0] | cand[1] | cand[2] | cand[3]) == 0ull) return;
    const float4 raw = st.raw[j];
    const uint32_t id = st.id[j];
    // the reference's operation order from here on (compiled without contraction)
    const float t1 = (raw.x * dx) * dx, bdx = raw.y * dx;
    uint32_t count = 0u;                       // wave-uniform
    unsigned long long lane_sum = 0ull;        // this lane's four pixels: < 2^34
    uint32_t lane_max = 0u;
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) {
        if ((cand[2 * pair] | cand[2 * pair + 1]) == 0ull) continue;
        const f32x2 dy = pair == 0 ? dy01 : dy23;
        const f32x2 pw = -0.5f * (t1 + (raw.z * dy) * dy) - bdx * dy;
        const float e0 = exp_ref(pw.x, st.exp_tab), e1 = exp_ref(pw.y, st.exp_tab);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * pair + h;
            if (cand[k] == 0ull) continue;
            const float power = h == 0 ? pw.x : pw.y;
            const float alpha = fminf(0.99f, raw.w * (h == 0 ? e0 : e1));
            const unsigned long long live = cand[k] & ~__ballot(power > 0.0f) & ~__ballot(alpha < kAlphaMin);
            if (live == 0ull) continue;
            count += (uint32_t)__popcll(live);
            if (__builtin_amdgcn_inverse_ballot_w64(live)) {
                const float w = alpha * s.T[k];
                const uint32_t qv = (uint32_t)(w * 4294967296.0f);
                s.T[k] = s.T[k] * (1.0f - alpha);
                lane_sum += qv;
                lane_max = lane_max > qv ? lane_max : qv;
                if constexpr (DOM) {
                    if (qv > best[k]) { best[k] = qv; best_id[k] = id; }
                }
            }
        }
    }
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
    const int rows = p.dims.row_end - p.dims.row_begin;
    // (tiles dealt to the XCDs in patches, as in the forward blend: blend_core.hpp)
    const int tile_local = tile_of_workgroup((int)blockIdx.x, p.dims.grid_x, rows);
    if (tile_local < 0) return;
    const int tile = p.dims.row_begin * p.dims.grid_x + tile_local;
    const int tx = tile % p.dims.grid_x, ty = tile / p.dims.grid_x;
    const uint2 range = p.ranges[tile];
    if (range.x >= range.y || range.y > p.num_rendered) return;       // no list (or not one of this call's R entries)
    const uint32_t total = range.y - range.x;

    TileLanes s;
    tile_lanes_init(s, tx, ty, lane, p.dims.width, p.dims.height, -1);
    uint32_t mine = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (s.inside[k]) s.last[k] = p.n_contrib[(size_t)(s.py0 + 4 * k) * (size_t)p.dims.width + (size_t)s.px];
        mine = mine > s.last[k] ? mine : s.last[k];
    }
    // the walk ends with the tile's last contributor
    const uint32_t walk = min(total, wave_reduce_u32(mine, MaxU32{}));
    if (walk == 0u) return;
    exp_table_init(st.exp_tab, lane);

    TileFeed feed;
    feed.means2D = p.means2D; feed.colors = nullptr; feed.conic_opacity = p.conic_opacity;
    feed.box = tile_box(tx, ty, p.dims.width, p.dims.height);
    feed.total = walk; feed.t_cutoff = 0.0f;
    // batch k = list positions [64 k, 64 k + 64); ids are fetched two batches ahead, records one batch ahead (blend.hip)
    auto next_batch = [&](uint32_t pos) {
        RecordBatch nb;
        nb.valid = pos < walk;
        if (nb.valid) {
            const uint32_t cnt = min((uint32_t)kWave, walk - pos);
            nb.mask = cnt == kWave ? ~0ull : ((1ull << cnt) - 1ull);
            nb.pos = pos;
            if ((uint32_t)lane < cnt) nb.id = p.point_list[range.x + pos + (uint32_t)lane];
        }
        return nb;
    };
    auto fetch = [&](RecordBatch& b) {       // (fetch_records, bounded by the scene's size)
        b.xy = make_float2(0.0f, 0.0f);
        b.co = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (b.valid && b.present() && b.id < p.num_gaussians) { b.xy = feed.means2D[b.id]; b.co = feed.conic_opacity[b.id]; }
    };
    const bool need_sum = p.weight_sum != nullptr, need_max = p.weight_max != nullptr;
    uint32_t best[4] = {0u, 0u, 0u, 0u}, best_id[4] = {0u, 0u, 0u, 0u};
    RecordBatch b0 = next_batch(0);
    fetch(b0);
    RecordBatch b1 = next_batch(kWave);
    for (uint32_t pos = 2 * kWave; b0.valid; pos += kWave) {
        fetch(b1);
        RecordBatch b2 = next_batch(pos);
        const uint32_t kept = stage_contrib(feed, st, b0, p.num_gaussians);
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
        b0 = b1;
        b1 = b2;
    }
    if constexpr (DOM) {
        // one add per distinct Gaussian of a strip: the first of its lanes adds how many they are
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
    if (r.magic != GSR_RECEIPT_MAGIC || r.tile_row_begin < 0 || r.tile_row_end > grid_y || r.tile_row_begin > r.tile_row_end)
        return GSR_ERR_INVALID_ARG;
    BlockFeed block_lists;
    bool from_blocks = false, lists_written = true;
    GSR_TRY(lists_of_receipt(r, a->num_gaussians, a->width, a->height, r.tile_row_begin, r.tile_row_end, a->point_list, &block_lists,
                             &from_blocks, &lists_written));
    if (r.num_rendered == 0 || r.tile_row_begin == r.tile_row_end) return GSR_OK;      // (nothing was blended: nothing is written)
    if (!lists_written || !a->point_list) return GSR_ERR_INVALID_ARG;      // (no walk through the block lists here)

    ContribParams p;
    p.ranges = reinterpret_cast<const uint2*>(a->ranges);
    p.point_list = a->point_list;
    p.means2D = reinterpret_cast<const float2*>(a->means2D);
    p.conic_opacity = reinterpret_cast<const float4*>(a->conic_opacity);
    p.n_contrib = a->n_contrib;
    p.weight_sum = reinterpret_cast<unsigned long long*>(a->weight_sum);
    p.weight_max = a->weight_max;
    p.pixels = reinterpret_cast<unsigned long long*>(a->pixels);
    p.dominant = reinterpret_cast<unsigned long long*>(a->dominant);
    p.dims.width = a->width; p.dims.height = a->height;
    p.dims.grid_x = (a->width + kTile - 1) / kTile; p.dims.grid_y = grid_y;
    p.dims.row_begin = r.tile_row_begin; p.dims.row_end = r.tile_row_end;
    p.num_gaussians = (uint32_t)a->num_gaussians;
    p.num_rendered = r.num_rendered;
    const long long blocks = patch_workgroups(p.dims.grid_x, r.tile_row_end - r.tile_row_begin);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;

    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    const bool profile = (a->flags & GSR_FLAG_PROFILE) != 0;
    CallEvents<2> events;
    if (profile) {
        GSR_TRY(events.create());
        GSR_HIP_TRY(hipEventRecord(events.ev[0], stream));
    }
    if (a->dominant) hipLaunchKernelGGL(contrib_kernel<true>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
    else hipLaunchKernelGGL(contrib_kernel<false>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
    GSR_LAUNCH_CHECK("contrib_kernel");
    if (profile) {
        GSR_HIP_TRY(hipEventRecord(events.ev[1], stream));
        GSR_HIP_TRY(hipEventSynchronize(events.ev[1]));
        GSR_HIP_TRY(hipEventElapsedTime(&a->stage_ms, events.ev[0], events.ev[1]));
    }
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

extern "C" int gsr_contribution(gsr_contribution_args* a) { return gsr::entry_point(gsr::contribution_impl, a); }
