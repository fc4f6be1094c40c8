// gsr_forward's per-frame choices (the stages of api.hip call them): the switch points, what they read and the rules that apply them. Host C++17
// only and pure — plain values in, small structs out; no HIP, no history pointer. gsr_forward copies what a rule reads out
// of the tile history, calls the rule where the choice is made and writes back what it returns (tests/test_frame_policy.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gsrast_amd.h"

namespace gsr {

constexpr int kTile = 16;          // BLOCK_W / BLOCK_H, reference GSCuda.cu:20-21

struct FrameDims {
    int width, height;
    int grid_x, grid_y;            // tile grid of the whole image
    int row_begin, row_end;        // tile rows this call bins / sorts / blends
};

// The tile grid of a width x height image and the band of tile rows a call works on (tile_row_begin / tile_row_end of
// gsr_forward_args and gsr_backward_args: both zero = every row; begin == end = an empty band). A band that does not lie
// inside the grid is refused.
inline int tile_band(int width, int height, int row_begin_arg, int row_end_arg, FrameDims* d) {
    d->width = width;
    d->height = height;
    d->grid_x = (width + kTile - 1) / kTile;
    d->grid_y = (height + kTile - 1) / kTile;
    d->row_begin = 0;
    d->row_end = d->grid_y;
    if (row_begin_arg != 0 || row_end_arg != 0) {
        if (row_begin_arg < 0 || row_end_arg > d->grid_y || row_begin_arg > row_end_arg) return GSR_ERR_INVALID_ARG;
        d->row_begin = row_begin_arg;
        d->row_end = row_end_arg;
    }
    return GSR_OK;
}

// Instances per visible Gaussian (R / V) at which the plans and the blend's feed change hands (each with the frames it was
// measured on; `profiles/r05_trained_like.txt` has all of them on a scene of flat, opaque splats on surfaces):
constexpr uint64_t kBlockPlanMinInstances = 6;    // block plan from here on, sort plan below
constexpr uint64_t kBlockFeedMinInstances = 48;   // a SERIAL blend reads the block lists from here on, the sorted lists below
constexpr uint32_t kBigSplatTiles = 256;          // "a big splat" (16 x 16 tiles and more) for the plan's choice
constexpr uint64_t kOverlapMinInstances = 16;     // the blend may run beside the emission (block-fed) from here on — when the tile times say it is the shorter of the two
// A blend fed from the sorted lists gives EVERY tile four waves (deep tiles, blend.hip) below this many instances per visible
// Gaussian: short lists of small splats, where a frame ends on the lone waves of its few deep tiles and four waves per tile
// cost the others next to nothing. Blend, one wave per tile -> four, bench scene (`profiles/r06_deep_tiles.txt`): R/V = 3.6: 0.66 ->
// 0.30 ms, 5.3: 0.54 -> 0.31, 7.3: 0.54 -> 0.43, 11: 0.60 -> 0.59, 16: 0.63 -> 0.66, 23: 0.46 -> 0.56 (long lists that few
// records of survive: the walk is the work, and the four waves meet at a barrier every 256 entries of it); on 49 unrelated
// views of the same scene (bench.py's random views, serial blends): 0.57-0.97 of one wave's time up to 12, 0.83-1.00 at 12-16,
// 0.94-1.06 at 16-24, up to 1.23 beyond. The switch is at 16 — where the blend may start to run beside the emission
// (kOverlapMinInstances), fed from the block lists, which have no deep tiles. Above it: one
// wave per tile (four for the history's slowest tiles only was built and measured neutral there: GSR_DEEP_BY_HISTORY).
constexpr uint64_t kDeepAllMaxInstances = 16;
constexpr unsigned long long kColorsTicksPerMega = 2040;   // colors_visible_kernel alone: 10 ns units per million Gaussians (50 M: 1.02 ms, 64 bytes fetched per Gaussian at the memory's request rate)

// What the launch heuristics need to know about the chip, derived from its CU count (hipDeviceAttributeMultiprocessorCount,
// read once per device: an MI355X in a partitioned mode shows fewer CUs per device, and every figure below follows).
struct DeviceShape {
    int cus;                                 // compute units of the device
    uint32_t blend_slots;                    // wave slots of the blend kernels: 4 SIMDs x 5 waves (96 VGPRs) per CU — 5 120 on 256 CUs
    uint32_t blend_slots_beside;             // ... beside the emission's persistent workgroups, which keep their registers: 3 per SIMD — 3 072
    unsigned long long light_frame_ticks;    // 250 us (in 10 ns) per blend wave slot, summed over the tiles: below it a frame counts as LIGHT
    uint32_t persistent_workgroups(uint32_t per_cu) const { return (uint32_t)cus * per_cu; }
};
// (include/gsrast_amd.h gsr_device_shape, tests/test_capi_cpu.py)
inline DeviceShape device_shape_of(int cus) {
    DeviceShape s;
    s.cus = cus > 0 ? cus : 1;
    s.blend_slots = (uint32_t)s.cus * 4u * 5u;
    s.blend_slots_beside = (uint32_t)s.cus * 4u * 3u;
    s.light_frame_ticks = 25000ull * (unsigned long long)s.blend_slots;
    return s;
}

// What the environment asks for, read once per process (A/B runs and the tests set these before the first call; thread_state.hip
// read_env_knobs).
struct EnvKnobs {
    bool tile_history;         // GSR_TILE_HISTORY=0: no call reads or writes a tile history
    int colors_beside;         // GSR_COLORS_BESIDE=0|1|2: geomState.rgb inside the preprocess / beside the depth sort / beside the blend; -1: by size
    int fused_depth;           // GSR_FUSED_DEPTH=0|1: the depth order with / without the compaction whatever the size; -1: by size
    int colors_early_pct;      // GSR_COLORS_EARLY_PCT=0..100: of the colours written beside the blend, the share that starts right behind the preprocess; -1: the default
    int depth_records;         // GSR_DEPTH_RECORDS=0|1: the depth order's triples as three arrays / as 12-byte records between its passes; -1: records without the compaction
    bool deep_by_history;      // GSR_DEEP_BY_HISTORY=1: above that, the history's slowest tiles get four waves (tile_order_kernel's
                               // count; measured neutral, `profiles/r06_deep_tiles.txt`: off by default)
    int sort_single_ticket = -1;   // GSR_SORT_SINGLE_TICKET=0|1: the onesweep's tiles in XCD runs / by one ticket (radix_sort.hip take_tile); -1: by CU count
};

// What the rules read of the call's tile history (gsr_tile_history, api_internal.hpp: the same fields, copied). A call without a
// history reads the zeros of a HistoryView{}.
struct HistoryView {
    bool wanted = false;        // the last statistics say the frame ends on a few slow tiles (or is a light one)
    bool decorrelated = false;  // ... and that the two last frames did not resemble each other
    bool overlapped = false;    // the last block-plan call ran its blend beside the emission
    bool block_fed = false;     // ... and read the block lists (else the sorted lists: a tile's time then says less about the block-fed blend)
    uint32_t mean = 0, longest = 0;   // mean and longest tile time of the last statistics; mean 0: none yet for this size
    uint32_t calls = 0;         // calls since the ticks were last cleared
};

// The history's refresh at the start of a call: `h` as it takes in the statistics tile_order_kernel has left, if they are
// fresh (`stats`: [1] longest tile, [2] mean, [4] order dropped; else nullptr), and whether this call sorts an order.
// The order costs a launch on the second stream and the host a few microseconds, and it pays on frames that END on a
// few slow tiles and on light frames: it is sorted when the last statistics say the longest tile takes 2.5 times what the
// tiles would take spread evenly over the chip's 5 120 wave slots — and every fourth call, to have fresh statistics (a
// camera that leaves the cloud is noticed within five frames).
struct HistoryStep { HistoryView view; bool order_now; };
inline HistoryStep step_history(HistoryView h, const uint32_t* stats, unsigned long long tiles, const DeviceShape& shape) {
    if (stats) {
        h.wanted = 2ull * (unsigned long long)shape.blend_slots * stats[1] > 5ull * tiles * stats[2] ||
                   (stats[2] != 0u && tiles * stats[2] < shape.light_frame_ticks);      // (or a light frame: tile_order_kernel)
        h.mean = stats[2];
        h.longest = stats[1];
        h.decorrelated = stats[4] != 0u;
    }
    // (while the frames do not resemble each other the sort runs every call: it is what looks whether they do again — a
    // camera cut is over after three frames — and it hands out the patch order as long as they do not)
    return {h, h.wanted || h.decorrelated || (h.calls % 4u) == 1u};        // (call 0 has no ticks yet)
}

// Before the preprocess: where geomState.rgb is written (colors_mode 0: inside the preprocess, 1: beside the depth sort,
// 2: beside the blend), how many of them [0, colors_early) start right behind the preprocess in mode 2, and the depth order's
// form.
struct EarlyChoice { int colors_mode; size_t colors_early; bool fused_depth, depth_records; };
inline EarlyChoice choose_early(int n, uint32_t flags, bool colors_precomp, bool xy_plan, const HistoryView& h,
                                unsigned long long tiles, const EnvKnobs& env, const DeviceShape& shape) {
    EarlyChoice c;
    // Up to 16 M Gaussians beside the depth sort: there its kernels wait on latency and the colours cost them 0.05 ms for the
    // 0.10 ms the preprocess saves — bench frame 1.315 -> 1.268 ms. At 50 M they are bound by HBM themselves and lose what
    // the preprocess gains (6.10 -> 6.19 ms): there the colours are written beside the BLEND — vector-bound —, which takes a
    // record's colour straight from the SH array meanwhile (TileFeed::dc_stride).
    // ... where there IS a blend to hide behind: a frame whose blend runs beside the emission (the history's last frame did) would
    // write its colours behind that blend, beside the rest of the emission — bound by the memory as well, and the frame ends with
    // it; beside the depth sort they cost less (20 M Gaussians of the bench scene, 919 M instances: 3.87 -> 3.76 ms).
    const bool colors_movable = !(flags & GSR_FLAG_SEMANTICS_INRIA) && !colors_precomp && !(flags & GSR_FLAG_SERIAL_EMIT);
    const bool blend_beside_emission = h.mean != 0u && h.overlapped;
    c.colors_mode = !colors_movable ? 0 : (env.colors_beside >= 0 ? env.colors_beside : ((n <= (1 << 24) || blend_beside_emission) ? 1 : 2));
    // Colours beside the blend (mode 2) where the blend is SHORTER than the colours kernel (50 M Gaussians: 1.02 ms of colours
    // alone, 1.37 beside a blend of 0.70 — the frame ended 0.65 ms after its blend): the Gaussians [0, colors_early) get theirs
    // right behind the preprocess — beside the scan and the digit counts, which wait on LDS atomics and latency, and on into the
    // first depth pass, which pays for it (336 -> 545 us with two fifths of them) —, the rest beside the blend, which then
    // outlasts it or nearly: 50 M 4.93-5.07 -> 4.78-4.94 ms. The share: what the history's blend leaves uncovered of
    // kColorsTicksPerMega x N, at most half; none without a history.
    c.colors_early = 0;
    if (c.colors_mode == 2) {
        unsigned long long pct = 0;
        if (env.colors_early_pct >= 0) {
            pct = (unsigned long long)env.colors_early_pct;
        } else if (h.mean != 0u && !h.decorrelated) {
            const unsigned long long blend_ticks = std::max((unsigned long long)h.mean * tiles / (unsigned long long)shape.blend_slots,
                                                            (unsigned long long)h.longest);
            const unsigned long long colors_ticks = kColorsTicksPerMega * (unsigned long long)n / 1000000ull;
            if (colors_ticks > blend_ticks) pct = std::min(50ull, 100ull * (colors_ticks - blend_ticks) / colors_ticks);
        }
        c.colors_early = (size_t)n * (size_t)pct / 100u;
    }
    // Scenes beyond 16 M Gaussians (there every kernel of the depth order is bound by HBM): no compaction — its 20 N bytes buy
    // nothing where nearly every Gaussian is visible (50 M: 0.20 ms). The digit counts come from a pass over the keys alone
    // and the first depth pass reads the per-Gaussian arrays itself, leaving out what has no tile (onesweep_kernel, DROP).
    c.fused_depth = xy_plan && (env.fused_depth >= 0 ? env.fused_depth == 1 : n > (1 << 24));
    // Between the passes the (key, index, rectangle) triples travel as 12-byte RECORDS — a digit's run leaves a tile as one
    // piece instead of three, a lane fetches its key's triple with one load (50 M Gaussians: 347 + 2 x 322 -> 340 + 309 + 294 us).
    // Where the passes are bound by latency, not by the memory (up to 16 M Gaussians: with the compaction), it changes nothing
    // (bench frame and the path's poses: +-0.003 ms) and the arrays stay.
    c.depth_records = xy_plan && (env.depth_records >= 0 ? env.depth_records == 1 : c.fused_depth);
    return c;
}

// Behind the read-back (R instances, V visible Gaussians, big_instances of them in splats of kBigSplatTiles tiles and more):
// the binning plan, whether the blend runs beside the emission (`overlap`, on the second stream), and which lists feed it.
// `overlap` and `block_fed` are also the history's new `overlapped` / `block_fed`; plan_used: GSR_PLAN_* of the choice.
struct BinningChoice { bool use_blocks, overlap, blend_from_lists, block_fed; uint32_t plan_used; };
inline BinningChoice choose_binning(uint32_t R, uint32_t V, unsigned long long big_instances, bool xy_plan, bool blockbin_ok,
                                    uint32_t flags, const HistoryView& h, unsigned long long tiles, const DeviceShape& shape) {
    BinningChoice c{};
    // The block plan pays per (Gaussian, block) entry and per unit, the sort plan 36 bytes per instance: what decides is
    // the instances per VISIBLE Gaussian. Measured (binning without the blend, sort / blocks): R/V = 2.7 (50 M tiny splats)
    // 5.6 / 5.9 ms, 5.3 (the bench scene from far away) 0.98 / 1.00 ms, 7.5: 2.08 / 1.81 ms, 11: 2.76 / 1.58 ms, 88: 2x.
    // ... of the splats that ARE small: the sort plan's emission walks a Gaussian's columns and keys chunk by chunk of 512
    // Gaussians, and a few hundred background splats that cover a thousand tiles each (any trained scene seen from outside)
    // make its slowest chunks five times the others — 1 M flat splats + 500 huge ones from 48 units away, R/V = 2.8:
    // 1.53 against 1.08 ms; 5.8 M: 2.46 / 2.14 (`profiles/r05_trained_like.txt`). With an eighth of the frame's instances in
    // such splats the frame goes to the block plan whatever its average.
    c.use_blocks = xy_plan && blockbin_ok && !(flags & GSR_FLAG_PLAN_SORT);
    if (c.use_blocks && !(flags & GSR_FLAG_PLAN_BLOCKS))
        c.use_blocks = (uint64_t)R >= kBlockPlanMinInstances * (uint64_t)V || 8ull * big_instances >= (unsigned long long)R;
    c.plan_used = c.use_blocks ? GSR_PLAN_BLOCKS : (xy_plan ? GSR_PLAN_SORT : GSR_PLAN_GENERIC);
    if (!c.use_blocks) return c;          // (the other plans' blends run behind their lists, fed from them)
    // The blend of the block plan reads the block lists, not the sorted lists, so it does not depend on the emission: beside
    // each other (GSR_FLAG_OVERLAP_EMIT forces it) the emission, bound by the HBM write path, and the blend, bound by vector
    // ALU work, make 5 % shorter frames. By default: beside each other when the blend — what the tiles of the last calls
    // took, spread over the chip's 5 120 wave slots — is expected to be the shorter of the two (the emission: 12 R bytes at
    // 5 TB/s); a blend already running beside the emission takes about twice as long per tile, hence the second threshold.
    bool overlap = (flags & GSR_FLAG_OVERLAP_EMIT) != 0;
    // (not while the history's frames do not resemble each other: the last frame's tile times then say nothing about this one)
    if (!overlap && !(flags & GSR_FLAG_SERIAL_EMIT) && h.mean != 0u && !h.decorrelated && (uint64_t)R >= kOverlapMinInstances * (uint64_t)V) {
        // how long the blend will take: the tiles' times spread over the chip's 5 120 wave slots — beside the emission, whose
        // persistent workgroups keep their registers, over the 3 072 it gets there —, but never less than the longest tile
        // (frames of small splats end on a few lone waves: the mean alone said 0.16 ms for a blend of 0.36)
        unsigned long long blend_ticks = std::max((unsigned long long)h.mean * tiles /
                                                      (unsigned long long)(h.overlapped ? shape.blend_slots_beside : shape.blend_slots),
                                                  (unsigned long long)h.longest);
        // (times of a blend fed from the SORTED lists: out of the block lists a tile walks every unit of its block for its
        // entries — measured on the stand-in, block feed over sorted-list feed: 1.1 at 88 instances per visible Gaussian,
        // 1.44 at 23, 3 at 5 = 1 + 10 V / R)
        if (!h.block_fed) blend_ticks = blend_ticks * ((unsigned long long)R + 10ull * (unsigned long long)V) / (unsigned long long)R;
        // The emission: 12 R bytes at 4 TB/s (measured 4.9 on the bench frame's 3.2 GB, 3.8 on 1 GB, 3.3-4.6 on 0.46 GB) — then the blend must be the shorter of the two, beside a kernel that fills
        // the memory pipes it is throttled (the stand-in from outside the cloud, R/V = 22: 1.66 -> 1.99 ms) —, but never
        // under the 0.07 ms a wave takes for its share of one unit: a light frame's emission leaves the chip idle, and a
        // blend of up to twice that still gains beside it (1 M flat splats, frames of 0.4 ms; `profiles/r05_trained_like.txt`).
        // Once overlapped, the times are those of a blend that shares the chip: while the emission runs it advances at 0.46
        // of its pace (bench frame: 0.11 ms alone, 0.24 beside an emission that outlasts it), so b' = b / 0.46 if that ends
        // inside the emission e, else e + (b - 0.46 e). The time it would take alone is taken back out of b' and held to
        // the same limit, a tenth more (the stand-in from outside the cloud, entered from an overlapped pose, stayed
        // overlapped under a looser bound: 1.48 -> 1.70 ms, for good).
        const unsigned long long emit_bw = 12ull * (unsigned long long)R / 40000ull, emit_floor = 7000ull;
        unsigned long long limit = emit_bw >= emit_floor ? emit_bw : 2ull * emit_floor;
        // (a frame that is block-fed either way — 48 instances per visible Gaussian and more — changes nothing but the
        // company its blend keeps: there a blend of up to twice the emission still gains, 1 M-splat stand-in, emission
        // 0.10 ms, blend 0.13-0.24: 6-10 %; three times loses: the bench frame with faint splats)
        if (h.block_fed && (uint64_t)R >= kBlockFeedMinInstances * (uint64_t)V) limit *= 2ull;
        if (h.overlapped) {
            const unsigned long long e = std::max(emit_bw, emit_floor);
            const unsigned long long alone = blend_ticks <= e ? blend_ticks * 46ull / 100ull : blend_ticks - e * 54ull / 100ull;
            overlap = 10ull * alone < 11ull * limit;
        } else {
            overlap = blend_ticks < limit;
        }
    }
    // (GSR_FLAG_NO_SORTED_LISTS: there is no emission to run beside)
    c.overlap = overlap && !(flags & GSR_FLAG_NO_SORTED_LISTS);
    // Which lists feed the blend. Out of the block lists a tile walks every unit of its block and picks its entries
    // by mask: as good as the sorted list where a Gaussian covers most tiles of its blocks, but with small splats a
    // tile owns a few of a unit's 2048 entries and pays a round trip to memory per unit for them (the bench scene
    // from outside the cloud, R/V = 23: 0.65 against 0.45 ms; from far away, R/V = 5: 1.98 against 0.65 ms; bench
    // frame, R/V = 88: equal). With the sorted lists written anyway, sparse frames blend from them.
    c.blend_from_lists = !c.overlap && !(flags & GSR_FLAG_NO_SORTED_LISTS) && (uint64_t)R < kBlockFeedMinInstances * (uint64_t)V;
    c.block_fed = !c.blend_from_lists;
    if (c.overlap) c.plan_used |= GSR_PLAN_EMIT_OVERLAPPED;
    if (c.blend_from_lists) c.plan_used |= GSR_PLAN_BLEND_FROM_LISTS;
    if (flags & GSR_FLAG_NO_SORTED_LISTS) c.plan_used |= GSR_PLAN_LISTS_SKIPPED;
    return c;
}

// The blend's deep tiles (blend.hip: four waves or more per tile), once the order's sort has been launched or not
// (order_now: this call's blend takes an order sorted for it).
struct BlendChoice { bool deep_wanted, deep_all; int deep_waves; };
inline BlendChoice choose_blend(uint32_t R, uint32_t V, bool block_fed, bool order_now, int colors_mode, uint32_t flags,
                                const HistoryView& h, unsigned long long tiles, bool deep_by_history, const DeviceShape& shape) {
    BlendChoice c;
    // (deep tiles: the leading entries of an order sorted for THIS call; the block-fed blend has none)
    c.deep_wanted = deep_by_history && !block_fed && order_now && !h.decorrelated && !(flags & GSR_FLAG_NO_DEEP_TILES);
    const uint32_t deep_forced = flags & (GSR_FLAG_DEEP_TILES_ALL | GSR_FLAG_DEEP_WAVES_8 | GSR_FLAG_DEEP_WAVES_16);
    // (not where geomState.rgb is written BESIDE the blend — colors_mode 2, scenes beyond 16 M Gaussians —: eight deep
    // workgroups a CU hold every vector register of its SIMDs, the colours kernel waits for them to retire and the frame for
    // the colours kernel: 50 M Gaussians 5.09 -> 5.33 ms, 5.13-5.22 with the blend kept to 5-6 workgroups a CU by idle LDS;
    // with the colours passed as colorsPrecomp there is no such kernel: 4.37 -> 4.29)
    const bool deep_by_rule = colors_mode != 2 && !(flags & GSR_FLAG_NO_DEEP_TILES) && (uint64_t)R < kDeepAllMaxInstances * (uint64_t)V;
    c.deep_all = !block_fed && (deep_forced != 0u || deep_by_rule);
    // How many waves a deep tile gets: four — or eight, sixteen where the history says the frame's work sits in few tiles:
    // tiles x mean / longest is how many tiles AS LONG AS THE LONGEST the frame amounts to; with fewer of them than the chip has
    // SIMDs eight waves per tile win, with fewer than a quarter sixteen (measured, blend with 4 / 8 / 16 waves per tile,
    // `profiles/r06_deep_tiles.txt` — a trained-like scene of 5.83 M splats from 32 / 48 / 70 units away, 358 / 200 / 96 such
    // tiles: 1.15 / 1.01 / 1.03, 1.82 / 1.66 / 1.17, 3.20 / 2.88 / 2.20 ms (one wave per tile: 1.77, 3.06, 5.86); the bench
    // scene from 40 / 50 units, 948 / 422: 0.297 / 0.283 / 0.68 and 0.240 / 0.212 / 0.30; from 30 units, 1 609: 0.31 / 0.38 / 1.03)
    c.deep_waves = (deep_forced & GSR_FLAG_DEEP_WAVES_16) ? 16 : ((deep_forced & GSR_FLAG_DEEP_WAVES_8) ? 8 : 4);
    if (c.deep_all && deep_forced == 0u && h.mean != 0u && h.longest != 0u && !h.decorrelated) {
        const unsigned long long as_longest = tiles * (unsigned long long)h.mean / (unsigned long long)h.longest;
        const unsigned long long simds = 4ull * (unsigned long long)shape.cus;
        c.deep_waves = 4ull * as_longest <= simds ? 16 : (as_longest <= simds ? 8 : 4);
    }
    return c;
}

}  // namespace gsr
