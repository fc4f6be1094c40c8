// What the three host translation units of the C ABI share: chunks.hip (the layout of the caller's chunks), thread_state.hip
// (per-thread resources, tile histories, environment knobs) and api.hip (error reporting, test entry points, gsr_forward).
#pragma once
#include <string.h>

#include <vector>

#include "gsr_common.hpp"
#include "blockbin.hpp"
#include "radix_sort.hpp"

// A tile history (include/gsrast_amd.h, GSR_FLAG_NO_TILE_HISTORY): how long the tiles of a view's two last frames took, the
// order the next blend takes them in (TileOrder, blend_core.hpp), and what the host remembers of tile_order_kernel's
// statistics. One per view — the caller's own (gsr_tile_history_create), or one the library keeps per host thread, device
// and stream. It decides WHEN a tile is composited, never what comes out.
struct gsr_tile_history {
    uint32_t magic = 0;
    int device = -1;
    uint32_t* ticks[2] = {nullptr, nullptr};  // device: tile times (10 ns) of the two last frames; ticks[cur] receives the next one's
    uint32_t* order = nullptr;                // device: the blend's workgroup order
    uint32_t* deep = nullptr;                 // device word: how many leading entries of the order are DEEP tiles (blend.hip)
    uint32_t* stats = nullptr;                // pinned host words, written by tile_order_kernel: [0] fresh, [1] longest tile, [2] mean,
    uint32_t* stats_dev = nullptr;            //   [3] similarity of the two frames x 1000, [4] order dropped (they do not resemble each other)
    int cur = 0;
    int dims[4] = {0, 0, 0, 0};               // width, height, tile rows [begin, end) the ticks belong to
    uint32_t order_serial = 0;                // the call whose blend took `order` (0: none)
    gsr::HistoryView view;                    // what the per-frame rules read of it (frame_policy.hpp)
    uint32_t last_serial = 0;                 // the owning thread's call counter at its last use (the library's own histories: which to give up)
    bool used = false;
    hipStream_t last_stream = nullptr;        // the stream of the call that used it last: what orders two calls' kernels
    hipEvent_t ev_order = nullptr;            // "the order is sorted" (recorded on the library's second stream)
    hipEvent_t ev_switch = nullptr;           // a caller's own history taken to another stream: that stream waits for the old one's tail
};

namespace gsr {

// ---- chunk layout (chunks.hip) ----
// Layout of GeometryState::scanningSpace (the reference keeps CUB's scan temp there,
// AuxBuffer.cu:49-51; this library keeps all of its per-Gaussian scratch there).
struct GeoScratch {
    char* scan_temp;          // partial sums of the two prefix scans
    uint32_t* depth_key;      // u32[N] depth bits or ~0 (written by preprocess)
    uint32_t* rect_idx;       // u32[N] packed band-clipped rectangle in index order (written by preprocess)
    uint32_t* sort_info;      // the frame's device words: InfoWord, shared_words.hpp
    uint32_t* vis_partial;    // per 4096-key chunk: visible keys before it (compaction)
    uint32_t* main_partial;   // the same for the keys with the main top byte only (the depth order's side way, radix_sort.hip)
    uint32_t* big_partial;    // per 4096 Gaussians: the instances of those that touch kBigSplatTiles tiles or more
    uint4* wave_sums;         // per 64 Gaussians: {tilesTouched summed, with a tile, instances of the big ones, with another top byte} (written by the preprocess, summed by the scan)
    DepthTriple side;         // the side list (kDepthSideMax entries); its words: sort_info + kInfoSide
    DepthTriple c;            // the visible (depth key, index) pairs in index order: the sort's input
    DepthTriple a;            // depth-sort ping (three passes end here; kDepthSideMax elements of room in front of each array)
    DepthTriple b;            // depth-sort pong = result (sorted depth bits, sorted index)
                              // (.r: the packed rectangles of the same Gaussians, moved with the pairs — tile grids up to 255 x 255)
    SweepScratch sweep;       // onesweep status words for the N-sized sort: pass 0 (+ error word, digit histograms)
    SweepScratch sweep_more[3];   // passes 1-3: their own look-back words, so one clear up front covers all four
    char* emit_scratch;       // column-major emission: [chunk][column] table, block partials, column starts
    char* block_scratch;      // block binning: [chunk][block] table, partials, block meta, tile counts / starts
    size_t bytes;
};
GeoScratch carve_geo_scratch(char* base, size_t n);

// Layout of BinningState::sortingSpace: one scratch copy of the pairs + onesweep status.
struct BinScratch {
    uint64_t* tmp_k;
    uint32_t* tmp_v;
    SweepScratch sweep;       // pass 1 (also holds the two tile-digit histograms)
    SweepScratch sweep2;      // pass 2: its own look-back words, so both clears precede pass 1
    size_t bytes;
};
BinScratch carve_bin_scratch(char* base, size_t r);

// ---- per-thread resources (thread_state.hip) ----
// Pinned landing zone for the numRendered read-back plus the events / side stream of a call: one per host
// thread AND device (events and streams belong to the device that was current when they were created). These are
// resources, not state: nothing a later call needs to know about an earlier one is kept here — that travels in the
// gsr_forward_receipt, and lives in the caller's chunks.
struct Readback {
    uint32_t* host_dev = nullptr;      // the same words as the device sees them (pinned host memory is mapped)
    uint32_t* host = nullptr;          // the pinned host block: HostWord, shared_words.hpp
    uint32_t serial = 0;               // calls made so far by this thread on this device
    unsigned long long* staged_dev = nullptr;
    unsigned long long* staged_host = nullptr;   // = host + kHostStaged
    hipEvent_t ev[2 * GSR_NUM_STAGES] = {};   // [2s] start, [2s+1] end of stage s
    bool events = false;
    bool recorded[GSR_NUM_STAGES] = {};
    int begin_of[GSR_NUM_STAGES] = {};        // event index a stage starts at (default 2s)
    hipEvent_t ev_begin(int stage) const { return ev[2 * stage]; }
    hipEvent_t ev_end(int stage) const { return ev[2 * stage + 1]; }
    void ev_alias_begin(int stage, int after_stage) { begin_of[stage] = 2 * after_stage + 1; }
    hipEvent_t ev_r = nullptr;                // "numRendered has landed in host memory"
    hipStream_t side = nullptr;               // block plan, GSR_FLAG_OVERLAP_EMIT: the blend runs here, beside the emission
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // the tile histories this thread's calls without one of their own take: one per stream (history_of_call)
    std::vector<gsr_tile_history*> default_histories;
    hipEvent_t ev_colors = nullptr;           // "geomState.rgb is written" (colors_visible_kernel on the side stream)
    hipEvent_t ev_pre_blend = nullptr;        // "the blend is about to start" (colours beside the blend)
    int ensure();
    int ensure_side();
    int ensure_colors();
    int ensure_staged();
    int ensure_events();
};
// The calling thread's resources for the CURRENT device.
int current_readback(Readback*& out);
const EnvKnobs& env_knobs();
// The call's tile history: the caller's own, or this thread's for the call's stream (none: *out = nullptr).
int history_of_call(const gsr_forward_args& a, const FrameDims& d, bool enabled, hipStream_t stream, Readback& rb,
                    gsr_tile_history** out);

}  // namespace gsr
