// The two walks over a tile's SORTED list that the passes behind a forward call share, each written once as __device__
// __forceinline__ templates that take the pass's part as callables — every callable is inlined into the unrolled loops, so the
// pixel index k stays a compile-time index into the per-pixel register arrays — and, at the end, the host side those calls
// share. Who takes what: the replay contrib.hip, features.hip and distortion.hip (forward); the back walk absgrad.hip,
// features.hip and distortion.hip (backward), the last two with GeometrySums behind it where the geometry moves; the host
// side's walk_check, walk_frame and StageTimer all four, finish_sums the three backward calls, and walk_pass_check /
// walk_pass_call features.hip and distortion.hip, whose argument structs name the frame's fields alike. Common to both walks: one wavefront per 16 x 16 tile, four pixels per lane
// (x = lane & 15, y = (lane >> 4) + 4 k), tiles dealt to the XCDs in patches (blend_core.hpp: tile_of_workgroup), batches of 64
// list entries with ids two batches ahead and records one batch ahead, a batch compacted by record_misses_tile, one lane per
// record, into wave-private LDS (no barrier: its writes and reads are ordered inside the wave). A list entry is bounded by the
// receipt's R and the scene's N before it indexes anything; an entry that names no Gaussian of the scene is dropped.
//
// The skeletons are RESTATED here, not shared with the forward blend and render_backward_kernel: those two keep their own
// copies so that the kernels every frame and every training step time keep their object code. These lines must agree with
// them — change one and the two no longer describe the same pixels; only the tests tie them together:
//   - the REPLAY (front to back) with blend_core.hpp: stage_batch's footprint test, filter conic, floor (-ln(255 o) less 1e-3
//     and 1e-6 terms) and `terms < 1e6`; composite_record's filter window (kFilterSlack), its reference-order power, exp_ref,
//     alpha = min(0.99, o e), `power > 0`, `alpha < 1/255` and T = T (1 - alpha). What replaces the cut-off test: a pixel blends
//     the records that pass those tests up to and including its last contributor (n_contrib), and the wave maximum of n_contrib
//     bounds the walk — a tile whose pixels all saturated after 300 records of a 30 000-record list is left after 300.
//   - the BACK WALK (back to front) with render_backward_kernel (backward.hip): every pixel starts at its own last contributor
//     with T = final_t; the record's floor -ln(255 o) - 1e-3 skips strips it is too faint for before the exponential; power in
//     the forward's operation order, exp_ref, alpha >= 1/255: the forward's set; T_i = T_{i+1} rcp(1 - alpha); raw > 0.99 zeroes
//     a pixel's share of the geometry but not the walk; u = K d by two multiply-adds; GeometrySums: its lines from dL_dalpha on.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "blend_core.hpp"           // (and, through gsr_common.hpp, frame_policy.hpp: tile_band)
#include "blockbin.hpp"             // (lists_of_receipt, tile_order_of_call)
#include "wave_reduce.hpp"

namespace gsr {

// What a walk reads of the frame. final_t: the back walk's (and whoever forms a pixel from it); tile_order: the forward
// blend's workgroup order (tile_order_of_call), or null: patch order.
struct WalkFrame {
    const uint2* ranges;
    const uint32_t* point_list;
    const float2* means2D;
    const float4* conic_opacity;
    const uint32_t* n_contrib;
    const float* final_t;
    FrameDims dims;
    const uint32_t* tile_order;
    uint32_t num_gaussians;
    uint32_t num_rendered;
};

// This workgroup's tile (-1: a pad of the patch grid) ...
__device__ __forceinline__ int walk_tile(const WalkFrame& f, int* tx, int* ty) {
    const int rows = f.dims.row_end - f.dims.row_begin;
    const int tile_local = tile_of_workgroup(f.tile_order ? (int)f.tile_order[blockIdx.x] : (int)blockIdx.x, f.dims.grid_x, rows);
    if (tile_local < 0) return -1;
    const int tile = f.dims.row_begin * f.dims.grid_x + tile_local;
    *tx = tile % f.dims.grid_x;
    *ty = tile / f.dims.grid_x;
    return tile;
}
// ... and whether it has a list that is one of this call's R entries. (R == 0: the forward call left even the tile ranges
// unwritten — what is read here is then not looked at)
__device__ __forceinline__ bool walk_range(const WalkFrame& f, int tile, uint2* range) {
    *range = f.ranges[tile];
    return f.num_rendered != 0u && range->x < range->y && range->y <= f.num_rendered;
}

// ---- front to back: the forward's blend replayed from T = 1 -----------------------------------------------------------------
// One wave's staging area: the survivors of a batch of 64 list entries, compacted. A pass derives its own from it.
struct ReplayStage {
    float2 xy[kWave];
    float4 co[kWave];                    // the filter's pre-scaled conic and floor (StagedRecords::co)
    float4 raw[kWave];                   // conic + opacity as fetched
    uint32_t number[kWave];              // the record's 1-based position in the tile's list
    unsigned long long exp_tab[32];
};

// stage_batch (blend_core.hpp) without the colours: the same footprint test, the same filter conic, floor and margins, so that
// the candidates of a record are the forward's. payload(slot, id): what the pass stages beside the record.
template <typename Payload>
__device__ __forceinline__ uint32_t stage_replay(const TileBox& box, ReplayStage& st, const RecordBatch& b, uint32_t num_gaussians, Payload payload) {
    const bool present = b.present() && b.id < num_gaussians;
    const uint32_t rank = b.rank(), pos = b.pos;
    const bool keep = present && !record_misses_tile(b.xy, b.co, box);
    const unsigned long long m2 = __ballot(keep);
    if (keep) {
        const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0u));
        const float dxm = fmaxf(fabsf(b.xy.x - box.x_lo), fabsf(b.xy.x - box.x_hi)), dym = fmaxf(fabsf(b.xy.y - box.y_lo), fabsf(b.xy.y - box.y_hi));
        const float terms = fabsf(b.co.x) * dxm * dxm + fabsf(b.co.z) * dym * dym + 2.0f * fabsf(b.co.y) * dxm * dym;
        const float p0 = -__logf(255.0f * b.co.w);
        const float floor2 = !(b.co.w > -__builtin_inff()) ? -__builtin_inff() : (b.co.w <= 0.0f ? __builtin_inff() : (p0 - 1e-3f - 1e-6f * terms) * kLog2e);
        const bool filtered = terms < 1.0e6f;                                   // (NaN: not filtered)
        st.xy[slot] = b.xy;
        st.co[slot] = filtered ? make_float4((-0.5f * kLog2e) * b.co.x, -kLog2e * b.co.y, (-0.5f * kLog2e) * b.co.z, floor2)
                               : make_float4(0.0f, 0.0f, 0.0f, -__builtin_inff());
        st.raw[slot] = b.co;
        st.number[slot] = pos + rank + 1u;
        payload(slot, b.id);
    }
    return (uint32_t)__popcll(m2);
}

// Staged record j against the wave's pixels: the forward's candidates (a pixel outside the image has a NaN row coordinate) that
// have not yet had their last contributor (s.last[k] holds the pixel's n_contrib). The pass does its own late loads once any() says so.
struct ReplayRecord {
    float dx;
    f32x2 dy01, dy23;
    unsigned long long cand[4];
    __device__ __forceinline__ bool any() const { return (cand[0] | cand[1] | cand[2] | cand[3]) != 0ull; }
};
__device__ __forceinline__ ReplayRecord replay_candidates(const TileLanes& s, const ReplayStage& st, uint32_t j) {
    ReplayRecord r;
    const float2 xy = st.xy[j];
    const float4 q = st.co[j];
    const uint32_t number = st.number[j];
    r.dx = xy.x - s.fx;
    const float h0 = (q.x * r.dx) * r.dx;
    const float g = q.y * r.dx;
    f32x2 gy; gy.x = xy.y; gy.y = xy.y;
    f32x2 gg; gg.x = g; gg.y = g;
    f32x2 hh; hh.x = h0; hh.y = h0;
    f32x2 cz; cz.x = q.z; cz.y = q.z;
    r.dy01 = gy - s.fy01; r.dy23 = gy - s.fy23;
    const f32x2 fw01 = __builtin_elementwise_fma(r.dy01, __builtin_elementwise_fma(cz, r.dy01, gg), hh);
    const f32x2 fw23 = __builtin_elementwise_fma(r.dy23, __builtin_elementwise_fma(cz, r.dy23, gg), hh);
    const float filter[4] = {fw01.x, fw01.y, fw23.x, fw23.y};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r.cand[k] = __ballot(filter[k] <= kFilterSlack * kLog2e) & __ballot(filter[k] >= q.w) & __ballot(number <= s.last[k]);
    return r;
}

// composite_record's pair loop (blend_core.hpp) in the reference's operation order (compiled without contraction).
// on_live(k, live, alpha), called wave-uniformly where some lane blends the record into its pixel k: the lanes of `live`
// add their w = alpha s.T[k]; T moves on behind the call.
template <typename OnLive>
__device__ __forceinline__ void replay_blend(TileLanes& s, const ReplayStage& st, uint32_t j, const ReplayRecord& r, OnLive on_live) {
    constexpr float kAlphaMin = 1.0f / 255.0f;
    const float4 raw = st.raw[j];
    const float t1 = (raw.x * r.dx) * r.dx, bdx = raw.y * r.dx;
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) {
        if ((r.cand[2 * pair] | r.cand[2 * pair + 1]) == 0ull) continue;
        const f32x2 dy = pair == 0 ? r.dy01 : r.dy23;
        const f32x2 pw = -0.5f * (t1 + (raw.z * dy) * dy) - bdx * dy;
        const float e0 = exp_ref(pw.x, st.exp_tab), e1 = exp_ref(pw.y, st.exp_tab);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * pair + h;
            if (r.cand[k] == 0ull) continue;
            const float power = h == 0 ? pw.x : pw.y;
            const float alpha = fminf(0.99f, raw.w * (h == 0 ? e0 : e1));
            const unsigned long long live = r.cand[k] & ~__ballot(power > 0.0f) & ~__ballot(alpha < kAlphaMin);
            if (live == 0ull) continue;
            on_live(k, live, alpha);
            if (__builtin_amdgcn_inverse_ballot_w64(live)) s.T[k] = s.T[k] * (1.0f - alpha);
        }
    }
}

// The walk of one tile: reads n_contrib into s.last, ends with the tile's last contributor, and hands every batch, its records
// fetched, to on_batch(box, batch). False: the tile has no list (nothing was read but its range).
template <typename OnBatch>
__device__ __forceinline__ bool replay_walk(const WalkFrame& f, int tile, int tx, int ty, int lane, TileLanes& s, ReplayStage& st, OnBatch on_batch) {
    uint2 range;
    if (!walk_range(f, tile, &range)) return false;
    uint32_t mine = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (s.inside[k]) s.last[k] = f.n_contrib[(size_t)(s.py0 + 4 * k) * (size_t)f.dims.width + (size_t)s.px];
        mine = mine > s.last[k] ? mine : s.last[k];
    }
    const uint32_t walk = min(range.y - range.x, wave_max_u32(mine));
    if (walk == 0u) return true;
    exp_table_init(st.exp_tab, lane);
    const TileBox box = tile_box(tx, ty, f.dims.width, f.dims.height);
    // batch k = list positions [64 k, 64 k + 64); ids are fetched two batches ahead, records one batch ahead (blend.hip)
    auto next_batch = [&](uint32_t pos) {
        RecordBatch nb;
        nb.valid = pos < walk;
        if (nb.valid) {
            const uint32_t cnt = min((uint32_t)kWave, walk - pos);
            nb.mask = cnt == kWave ? ~0ull : ((1ull << cnt) - 1ull);
            nb.pos = pos;
            if ((uint32_t)lane < cnt) nb.id = f.point_list[range.x + pos + (uint32_t)lane];
        }
        return nb;
    };
    auto fetch = [&](RecordBatch& b) {       // (fetch_records, bounded by the scene's size)
        b.xy = make_float2(0.0f, 0.0f);
        b.co = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (b.valid && b.present() && b.id < f.num_gaussians) { b.xy = f.means2D[b.id]; b.co = f.conic_opacity[b.id]; }
    };
    RecordBatch b0 = next_batch(0);
    fetch(b0);
    RecordBatch b1 = next_batch(kWave);
    for (uint32_t pos = 2 * kWave; b0.valid; pos += kWave) {
        fetch(b1);
        RecordBatch b2 = next_batch(pos);
        on_batch(box, b0);
        b0 = b1;
        b1 = b2;
    }
    return true;
}

// ---- back to front: render_backward_kernel's walk ---------------------------------------------------------------------------
struct BackLanes {                 // per-lane state of the four pixels a lane owns
    int px, py0;
    float fx, fy[4];
    uint32_t last[4];              // the pixel's n_contrib
    float T[4];                    // transmittance behind the record the walk has reached: final_t at the start
};
struct BackStage {                 // one wave's staging area; a pass keeps its payload in arrays of its own beside it
    float4 co[kWave];
    float2 xy[kWave];
    uint32_t id[kWave];
    uint32_t pos[kWave];           // the record's 0-based position in the tile's list
    float floor[kWave];            // the alpha floor: a pixel can pass alpha >= 1/255 only where power >= -ln(255 opacity), less a margin (backward.hip)
    unsigned long long exp_tab[32];
};
// What a record gives one of the wave's pixel slots k, where act_mask says some lane's pixel blended it.
struct BackPixel {
    unsigned long long act_mask;
    bool act;                      // this lane's pixel is one of them
    float dx, dy;
    float4 co;
    float G, raw;                  // exp(power) and opacity x G; alpha = min(0.99, raw)
    float inv, Tn;                 // 1 / (1 - alpha); transmittance in front of this record
    float w;                       // alpha Tn, 0 where !act
    // clamped: alpha does not move with the parameters
    __device__ __forceinline__ bool live() const { return __builtin_amdgcn_inverse_ballot_w64(act_mask & ~__ballot(raw > 0.99f)); }
    __device__ __forceinline__ float ux() const { return __builtin_fmaf(co.x, dx, co.y * dy); }
    __device__ __forceinline__ float uy() const { return __builtin_fmaf(co.y, dx, co.z * dy); }
};

// Which of wave_sum8's eight totals this lane is left with (wave_reduce.hpp: lane 8 r holds value kSumOfRow[r]); -1: none.
__device__ __forceinline__ int sum8_of_lane(int lane) {
    constexpr int kSumOfRow[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    return (lane & 7) == 0 ? kSumOfRow[lane >> 3] : -1;
}

// The geometry tail of a back walk whose pass forms a dL_dalpha per (record, pixel): render_backward_kernel's lines (backward.hip)
// from there on — the clamp rule raw > 0.99, dpow, gop, u = K d, the pixel-by-pixel cov2D sums — and the filing of a record's
// nine sums into slots 0..5 and 9..11 of the double sums a gsr_backward of the same frame then reads (gsr_backward_args.sums_f64;
// slots 6..8, the colour's, are not touched). This lane's sums over its four pixels of the record in hand.
struct GeometrySums {
    static constexpr uint32_t kFloats = 12;      // the layout of gsr_backward_args.sums_f64 (backward.hip: kAccFloats)
    float mx, my, A, B, C, op, m00, m01, m11;
    __device__ __forceinline__ void clear() { mx = my = A = B = C = op = m00 = m01 = m11 = 0.0f; }
    __device__ __forceinline__ void add(const BackPixel& px, const float dL_dalpha) {
        const float dx = px.dx, dy = px.dy;
        const bool live = px.live();
        const float gop = live ? px.G * dL_dalpha : 0.0f;
        const float dpow = live ? px.raw * dL_dalpha : 0.0f;
        op += gop;
        A = __builtin_fmaf(-0.5f * dx * dx, dpow, A);
        B = __builtin_fmaf(-(dx * dy), dpow, B);
        C = __builtin_fmaf(-0.5f * dy * dy, dpow, C);
        const float ux = px.ux(), uy = px.uy();
        mx = __builtin_fmaf(-ux, dpow, mx);
        my = __builtin_fmaf(-uy, dpow, my);
        const float hux = 0.5f * dpow * ux, huy = 0.5f * dpow * uy;      // (the masked factor first: 0 x finite)
        m00 = __builtin_fmaf(hux, ux, m00); m01 = __builtin_fmaf(hux, uy, m01); m11 = __builtin_fmaf(huy, uy, m11);
    }
    // Two reductions a record, one atomic per filing lane. The lane map and the reductions are one decision: of wave_sum8's
    // eight, values 0..5 are slots 0..5, value kExtra is `extra` — a sum of the pass's own that rides along; what is returned is
    // its total in the lane where sum8_of_lane is kExtra — and value 7 is unused; wave_sum4 leaves value kSumOfRow4[r] in
    // every lane of row r (lane 16 r + 4 files it): slots 9..11 and one unused. (slot is formed once, ahead of the walk, where
    // the passes formed it themselves: inside file() features_backward_kernel<8, true> lost a wave per SIMD to registers)
    static constexpr int kExtra = 6;
    int slot;                                    // the slot this lane files, -1: none
    __device__ __forceinline__ explicit GeometrySums(const int lane) {
        constexpr int kSumOfRow4[4] = {9, 11, 10, 12};
        const int of8 = sum8_of_lane(lane);
        slot = (lane & 7) == 0 ? (of8 < kExtra ? of8 : -1) : ((lane & 15) == 4 && kSumOfRow4[lane >> 4] < 12 ? kSumOfRow4[lane >> 4] : -1);
    }
    __device__ __forceinline__ float file(double* geometry_sums, const size_t id, const int lane, const float extra) const {
        const float t8 = wave_sum8(mx, my, A, B, C, op, extra, 0.0f, lane);
        const float t4 = wave_sum4(m00, m01, m11, 0.0f);
        const float total = (lane & 7) == 4 ? t4 : t8;
        if (slot >= 0 && total != 0.0f) unsafeAtomicAdd(geometry_sums + kFloats * id + (uint32_t)slot, (double)total);
        return t8;
    }
};

// The whole walk of one tile. The pass's callables, all inlined:
//   seed(k, pid)           for a pixel slot inside the image: loads the pass's own per-pixel inputs (g), zero for the others;
//   start()                once, s.last and s.T set and a record to walk: what the pass forms of them (S);
//   payload(slot, id)      stages what the pass keeps beside a surviving record;
//   begin(j)               staged record j is next: the pass's late loads, its sums back to zero;
//   on_pixel(k, px)        wave-uniformly, for every pixel slot where some lane blended the record;
//   file(j)                once per record that any pixel took: st.id[j] receives the pass's sums.
// LIST_FIRST: a tile without a list leaves before its pixels' seeds are read (features_backward_kernel, up to 4 K loads a lane);
// else the range is read beside them (absgrad_kernel) — each pass as it was before the walk was shared.
template <bool LIST_FIRST, typename Seed, typename Start, typename Payload, typename Begin, typename OnPixel, typename File>
__device__ __forceinline__ void back_walk(const WalkFrame& f, int tile, int tx, int ty, int lane, BackLanes& s, BackStage& st, Seed seed,
                                          Start start, Payload payload, Begin begin, OnPixel on_pixel, File file) {
    exp_table_init(st.exp_tab, lane);
    uint2 range;
    const bool has_list = walk_range(f, tile, &range);
    if (LIST_FIRST && !has_list) return;
    s.px = tx * kTile + (lane & 15); s.py0 = ty * kTile + (lane >> 4);
    s.fx = (float)s.px;
    uint32_t hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = s.py0 + 4 * k;
        s.fy[k] = (float)py;
        const bool inside = s.px < f.dims.width && py < f.dims.height;
        s.last[k] = 0; s.T[k] = 1.0f;
        if (inside) {          // (one block: the pixel's loads all leave before the first of them is waited for)
            const size_t pid = (size_t)py * (size_t)f.dims.width + (size_t)s.px;
            s.last[k] = f.n_contrib[pid];
            s.T[k] = f.final_t[pid];
            seed(k, pid);
        }
        hi = max(hi, s.last[k]);
    }
    if (!has_list) return;
    hi = min(wave_max_u32(hi), range.y - range.x);                      // (a last contributor lies inside the list)
    if (hi == 0) return;
    start();
    const TileBox box = tile_box(tx, ty, f.dims.width, f.dims.height);

    auto walk_batch = [&](const bool present, const uint32_t id, const uint32_t idx_l, const float2 xy_l, const float4 co_l) {
        const bool keep = present && !record_misses_tile(xy_l, co_l, box);
        const unsigned long long kept_mask = __ballot(keep);
        if (keep) {
            const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept_mask, 0u));
            st.id[slot] = id;
            st.pos[slot] = idx_l;
            st.xy[slot] = xy_l;
            st.co[slot] = co_l;
            payload(slot, id);
            const float op = co_l.w;
            st.floor[slot] = !(op > -__builtin_inff()) ? -__builtin_inff() : (op <= 0.0f ? __builtin_inff() : -__logf(255.0f * op) - 1e-3f);
        }
        for (int j = (int)__popcll(kept_mask) - 1; j >= 0; --j) {
            const uint32_t idx0 = st.pos[j];
            const float2 xy = st.xy[j];
            BackPixel px;
            px.co = st.co[j];
            px.dx = xy.x - s.fx;
            const float4 co = px.co;
            const float dx = px.dx, flo = st.floor[j];
            begin(j);
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long inlist = __ballot(idx0 < s.last[k]);    // else: behind this pixel's last contributor
                if (inlist == 0ull) continue;
                const float dy = xy.y - s.fy[k];
                const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
                const unsigned long long cand = inlist & ~__ballot(power > 0.0f) & __ballot(power >= flo);
                if (cand == 0ull) continue;
                px.G = exp_ref(power, st.exp_tab);               // the forward's exp: same contributing set
                px.raw = co.w * px.G;
                const float alpha = fminf(0.99f, px.raw);
                px.act_mask = cand & ~__ballot(alpha < 1.0f / 255.0f);
                if (px.act_mask == 0ull) continue;
                px.act = __builtin_amdgcn_inverse_ballot_w64(px.act_mask);
                any = true;
                px.dy = dy;
                px.inv = __builtin_amdgcn_rcpf(1.0f - alpha);
                px.Tn = s.T[k] * px.inv;
                s.T[k] = px.act ? px.Tn : s.T[k];
                px.w = px.act ? alpha * px.Tn : 0.0f;
                on_pixel(k, px);
            }
            if (any) file(j);
        }
    };

    struct Batch {
        bool valid = false, present = false;
        uint32_t id = 0, idx_l = 0;
        float2 xy = {0.0f, 0.0f};
        float4 co = {0.0f, 0.0f, 0.0f, 0.0f};
    };
    // batch c = list positions [64 c, 64 c + 64) below hi, highest first
    int it_c = (int)((hi - 1) / kWave);
    auto next_batch = [&]() {
        Batch nb;
        if (it_c < 0) return nb;
        const uint32_t first = (uint32_t)it_c * kWave;
        --it_c;
        nb.valid = true;
        nb.idx_l = first + (uint32_t)lane;
        nb.present = (uint32_t)lane < min((uint32_t)kWave, hi - first);
        nb.id = f.point_list[range.x + (nb.present ? nb.idx_l : 0u)];
        nb.present = nb.present && nb.id < f.num_gaussians;
        return nb;
    };
    auto fetch = [&](Batch& nb) {
        const uint32_t at = (nb.valid && nb.present) ? nb.id : 0u;
        nb.xy = f.means2D[at];
        nb.co = f.conic_opacity[at];
    };
    Batch b0 = next_batch();
    fetch(b0);
    Batch b1 = next_batch();
    while (b0.valid) {
        fetch(b1);
        Batch b2 = next_batch();
        walk_batch(b0.present, b0.id, b0.idx_l, b0.xy, b0.co);
        b0 = b1;
        b1 = b2;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// What every call checks of its receipt before it walks: the band of tile rows (the call's tile_row_begin / tile_row_end, as
// tile_band reads them — or, band_as_is, rows taken as they stand: gsr_contribution names none and passes the receipt's), the
// lists the forward call left for it (lists_of_receipt), and that they are the sorted lists in point_list: there is no walk
// through the block lists here. *nothing: no record to walk (R == 0 or an empty band).
inline int walk_check(const gsr_forward_receipt& r, int n, int width, int height, int row_begin, int row_end, bool band_as_is,
                      const void* point_list, FrameDims* d, bool* nothing) {
    if (r.magic != GSR_RECEIPT_MAGIC) return GSR_ERR_INVALID_ARG;
    if (tile_band(width, height, row_begin, row_end, d) != GSR_OK) return GSR_ERR_INVALID_ARG;
    if (band_as_is) { d->row_begin = row_begin; d->row_end = row_end; }
    BlockFeed block_lists;
    bool from_blocks = false, lists_written = true;
    GSR_TRY(lists_of_receipt(r, n, width, height, d->row_begin, d->row_end, point_list, &block_lists, &from_blocks, &lists_written));
    *nothing = r.num_rendered == 0 || d->row_begin == d->row_end;
    if (!*nothing && (!lists_written || !point_list)) return GSR_ERR_INVALID_ARG;
    return GSR_OK;
}

inline WalkFrame walk_frame(const uint32_t* ranges, const uint32_t* point_list, const float* means2D, const float* conic_opacity,
                            const uint32_t* n_contrib, const float* final_t, const FrameDims& d, int num_gaussians, uint32_t num_rendered) {
    WalkFrame f;
    f.ranges = reinterpret_cast<const uint2*>(ranges);
    f.point_list = point_list;
    f.means2D = reinterpret_cast<const float2*>(means2D);
    f.conic_opacity = reinterpret_cast<const float4*>(conic_opacity);
    f.n_contrib = n_contrib;
    f.final_t = final_t;
    f.dims = d;
    f.tile_order = nullptr;
    f.num_gaussians = (uint32_t)num_gaussians;
    f.num_rendered = num_rendered;
    return f;
}

// For the passes whose argument struct (Args: gsr_features_args, gsr_distortion_args) names the frame's fields alike — what both
// of a pass's calls check of them, in the header's order, the pass's own fields left to the pass; and the frame of such a struct.
template <typename Args>
inline int walk_pass_check(Args* a, FrameDims* d, bool* nothing) {
    if (!a || a->struct_size != sizeof(Args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    if (a->num_gaussians <= 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (!a->means2D || !a->conic_opacity || !a->ranges || !a->n_contrib || !a->final_t) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->means2D, 8) || misaligned(a->conic_opacity, 16) || misaligned(a->ranges, 8)) return GSR_ERR_INVALID_ARG;
    return walk_check(a->receipt, a->num_gaussians, a->width, a->height, a->tile_row_begin, a->tile_row_end, false, a->point_list, d, nothing);
}
template <typename Args>
inline WalkFrame walk_frame(const Args* a, const FrameDims& d) {
    return walk_frame(a->ranges, a->point_list, a->means2D, a->conic_opacity, a->n_contrib, a->final_t, d, a->num_gaussians,
                      a->receipt.num_rendered);
}

struct StageTimer {               // GSR_FLAG_PROFILE: the call's kernels between two events
    CallEvents<2> events;
    bool on = false;
    int begin(bool profile, hipStream_t stream) {
        on = profile;
        if (!on) return GSR_OK;
        GSR_TRY(events.create());
        GSR_HIP_TRY(hipEventRecord(events.ev[0], stream));
        return GSR_OK;
    }
    int end(hipStream_t stream, float* ms) {
        if (!on) return GSR_OK;
        GSR_HIP_TRY(hipEventRecord(events.ev[1], stream));
        GSR_HIP_TRY(hipEventSynchronize(events.ev[1]));
        GSR_HIP_TRY(hipEventElapsedTime(ms, events.ev[0], events.ev[1]));
        return GSR_OK;
    }
};

inline long long finish_sums_workgroups(size_t count) { return (long long)((count + 255) / 256); }
// Rounds every double sum once, writes the output in full and leaves the scratch zero (most received nothing: no write for those).
// A thread takes V sums and writes them as one vector of V floats (`out` lies on a 4 V-byte boundary; the scratch is only known
// to lie on an 8-byte one): gsr_absgrad's pairs go as pairs, as its own kernel rounded them before this one — with one sum per
// thread over 2 N the call missed the timing rule against the parent in the one run that had it (profiles/walk_passes_cost.txt).
// (a template in an unnamed namespace: a translation unit that does not launch it does not carry it, one that does has its own)
namespace {
template <int V>
__global__ __launch_bounds__(256) void finish_sums_kernel(size_t count, double* __restrict__ sums, float* __restrict__ out) {
    static_assert(V == 1 || V == 2, "one float or a float2 per thread");
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = sums[V * i + e];
    if constexpr (V == 2) *reinterpret_cast<float2*>(out + 2 * i) = make_float2((float)v[0], (float)v[1]);
    else out[i] = (float)v[0];
#pragma unroll
    for (int e = 0; e < V; ++e)
        if (v[e] != 0.0) sums[V * i + e] = 0.0;
}
// count: vectors of V sums
template <int V>
inline int launch_finish_sums(size_t count, double* sums, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(finish_sums_kernel<V>, dim3((unsigned)finish_sums_workgroups(count)), dim3(256), 0, stream, count, sums, out);
    GSR_LAUNCH_CHECK("finish_sums_kernel");
    return GSR_OK;
}

// The call of such a pass once walk_pass_check has passed: launch(frame, workgroups, stream) is the pass's own kernel launch.
// The caller says which call it is. Forward (backward == nullptr): the kernel runs whenever the band has a row, at R == 0 too —
// every tile is then a tile without a list, and background and zeros get written. Backward: `backward` names the double sums
// the kernel adds into and the output they are rounded to; the kernel runs only where there is a record to walk, in the forward
// blend's tile order (the tiles that were slow there are the slow ones here: they go first, as they did there), and the sums
// are finished either way: the output is written in full.
struct WalkSums {
    size_t count;
    double* sums;
    float* out;
};
template <typename Args, typename Launch>
inline int walk_pass_call(Args* a, const FrameDims& d, bool nothing, const WalkSums* backward, Launch launch) {
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    if (exceeds_grid(blocks) || (backward && exceeds_grid(finish_sums_workgroups(backward->count)))) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (backward ? !nothing : d.row_begin != d.row_end) {
        WalkFrame frame = walk_frame(a, d);
        if (backward) frame.tile_order = tile_order_of_call(a->receipt, d.row_begin, d.row_end);
        GSR_TRY(launch(frame, (unsigned)blocks, stream));
    }
    if (backward) GSR_TRY(launch_finish_sums<1>(backward->count, backward->sums, backward->out, stream));
    return timer.end(stream, &a->stage_ms);
}
}  // namespace

}  // namespace gsr
