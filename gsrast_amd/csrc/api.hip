// C-ABI entry points (include/gsrast_amd.h): error reporting, the stage-level entry points the parity tests call, and the
// gsr_forward orchestration. The chunk layout is in chunks.hip, what a thread's calls keep between them in thread_state.hip.
//
// gsr_forward follows reference apps/gsrast/gscuda/GSCuda.cu:695-811 (gscuda::forward): one context (ForwardCall) and one
// function per stage over it, in the order forward_stages() calls them.
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "api_internal.hpp"

namespace gsr {

static thread_local int g_last_error = GSR_OK;
static thread_local char g_hip_error[256] = "";

void set_hip_error(hipError_t e, const char* what) {
    snprintf(g_hip_error, sizeof(g_hip_error), "%s: %s", what, hipGetErrorString(e));
}
void clear_hip_error() { g_hip_error[0] = 0; }

int record_error(int code) { g_last_error = code; return code; }

namespace {

// (SideJoin: whatever way the call is left — a failing step included — the caller's stream waits for what this call
// has put on the second stream: for `pending`, an event already recorded there, or, while `tail` is armed, for an
// event recorded behind everything the second stream holds at that moment)
struct SideJoin {
    hipStream_t stream;
    hipEvent_t pending;
    Readback* rb;
    bool tail;
    ~SideJoin() {
        if (tail && rb->side && rb->ev_join) {
            if (hipEventRecord(rb->ev_join, rb->side) == hipSuccess) (void)hipStreamWaitEvent(stream, rb->ev_join, 0);
            else (void)hipGetLastError();
        } else if (pending) {
            (void)hipStreamWaitEvent(stream, pending, 0);
        }
    }
};

// The state of one gsr_forward call: what its stages hand to each other.
struct ForwardCall {
    gsr_forward_args* const a;
    const hipStream_t stream;
    Readback& rb;
    const int n;
    const bool profile, count_staged, inria;
    FrameDims d{};
    int num_tiles = 0;
    unsigned long long tiles = 0;                  // (this call's)
    bool xy_plan = false;                          // tile grids up to 255 x 255: a packed rectangle per Gaussian
    char *geo_chunk = nullptr, *img_chunk = nullptr, *bin_chunk = nullptr;
    gsr_geometry_state geom{};
    gsr_image_state img{};
    gsr_binning_state bin{};
    GeoScratch gs{};
    BinScratch bs{};
    int32_t* radii = nullptr;
    uint32_t serial = 0;
    uint32_t* async_words = nullptr;               // this call's error slot in the pinned block, as the host sees it
    uint32_t *err_n = nullptr, *err_r = nullptr;   // ... its words for the N-sized depth sort / the R-sized sort, as the device sees them
    DeviceShape shape{};
    const EnvKnobs& env;
    gsr_tile_history* hist = nullptr;
    HistoryView view;                              // (what the rules read of the history from here on; none: zeros)
    bool order_now = false;
    uint32_t* t_ticks = nullptr;
    EarlyChoice early{};
    SweepScratch four[4];
    DepthSide side;
    FrameCounts counts{};                          // the read-back, decoded
    DepthTriple sorted;                            // depth-sorted keys / indices / rectangles (.r: xy_plan only)
    uint32_t* spare_k = nullptr;                   // the other pair of buffers' keys (free once the depth order is complete)
    uint32_t R = 0;
    BinningChoice plan{};
    SideJoin join;

    ForwardCall(gsr_forward_args* a_, Readback& rb_)
        : a(a_), stream((hipStream_t)a_->stream), rb(rb_), n(a_->num_gaussians), profile((a_->flags & GSR_FLAG_PROFILE) != 0),
          count_staged((a_->flags & GSR_FLAG_COUNT_STAGED) != 0), inria((a_->flags & GSR_FLAG_SEMANTICS_INRIA) != 0),
          env(env_knobs()), join{stream, nullptr, &rb_, false} {}

    // stage timing (GSR_FLAG_PROFILE): the begin and the end of stage s on stream st; mark(): its end was recorded elsewhere
    int begin(int s, hipStream_t st) { if (profile) GSR_HIP_TRY(hipEventRecord(rb.ev_begin(s), st)); return GSR_OK; }
    int end(int s, hipStream_t st) { if (profile) { GSR_HIP_TRY(hipEventRecord(rb.ev_end(s), st)); rb.recorded[s] = true; } return GSR_OK; }
    int begin(int s) { return begin(s, stream); }
    int end(int s) { return end(s, stream); }
    void mark(int s) { if (profile) rb.recorded[s] = true; }
    int nv() const { return (int)counts.visible; }
    size_t colors_rest() const { return (size_t)n - early.colors_early; }     // (colours beside the blend: those not started early)
};

// Argument checks, and the calling thread's resources for this call.
int check_arguments(gsr_forward_args* a, Readback** out) {
    const int n = a->num_gaussians;
    if (n <= 0 || a->width <= 0 || a->height <= 0 || !a->geometry_alloc || !a->binning_alloc || !a->image_alloc ||
        !a->background || !a->means3D || !a->opacities || !a->view_matrix || !a->proj_matrix || !a->out_color ||
        (!a->shs && !a->colors_precomp) || (!a->cov3D_precomp && (!a->scales || !a->rotations)))
        return GSR_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GSR_ERR_NO_DEVICE;
    if ((a->flags & GSR_FLAG_SEMANTICS_INRIA) && !a->cam_pos && !a->colors_precomp) return GSR_ERR_INVALID_ARG;
    Readback* rb = nullptr;
    GSR_TRY(current_readback(rb));
    GSR_TRY(rb->ensure());
    if (a->flags & GSR_FLAG_PROFILE) GSR_TRY(rb->ensure_events());
    if (a->flags & GSR_FLAG_COUNT_STAGED) GSR_TRY(rb->ensure_staged());
    *out = rb;
    return GSR_OK;
}

// The call's tile rows, and the geometry and image states carved from the caller's chunks.
int carve_chunks(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    FrameDims& d = c.d;
    GSR_TRY(tile_band(a->width, a->height, a->tile_row_begin, a->tile_row_end, &d));
    c.num_tiles = d.grid_x * d.grid_y;
    c.tiles = (unsigned long long)(d.row_end - d.row_begin) * (unsigned long long)d.grid_x;
    c.xy_plan = d.grid_x <= 255 && d.grid_y <= 255;

    // GSCuda.cu:723-729
    c.geo_chunk = a->geometry_alloc(a->geometry_user, gsr_required_geometry(c.n));
    if (!c.geo_chunk) return GSR_ERR_ALLOC;
    gsr_geometry_from_chunk(c.geo_chunk, c.n, &c.geom);
    c.radii = a->radii ? a->radii : c.geom.internal_radii;

    // GSCuda.cu:734-736
    const int P = a->width * a->height;
    c.img_chunk = a->image_alloc(a->image_user, gsr_required_image(P) + 128);
    if (!c.img_chunk) return GSR_ERR_ALLOC;
    gsr_image_from_chunk(c.img_chunk, P, &c.img);
    c.gs = carve_geo_scratch(c.geom.scanning_space, (size_t)c.n);
    return GSR_OK;
}

// This call's error words: the next of the slots (the call that owned it 64 calls ago is long complete: the host
// has waited for every call's read-back since). Zeroed here, written only by a kernel whose bounded look-back spin
// gave up, read by gsr_poll_async_error through the receipt.
void claim_error_slot(ForwardCall& c) {
    Readback& rb = c.rb;
    if (++rb.serial == 0u) ++rb.serial;                    // (0 is what an untouched error word holds)
    c.serial = rb.serial;
    const uint32_t slot_at = kHostAsyncBase + kAsyncSlotWords * (c.serial % kAsyncSlots);
    c.async_words = rb.host + slot_at;
    c.async_words[kAsyncErrN] = c.async_words[kAsyncErrR] = c.async_words[kAsyncZero] = 0;
    c.async_words[kAsyncSerial] = c.serial;
    c.err_n = rb.host_dev + slot_at + kAsyncErrN;         // N-sized depth sort
    c.err_r = rb.host_dev + slot_at + kAsyncErrR;         // R-sized sort (sort plan, generic plan)
    for (bool& r : rb.recorded) r = false;
    for (int s = 0; s < GSR_NUM_STAGES; ++s) rb.begin_of[s] = 2 * s;
}

// what the caller takes away from this call (complete once GSR_OK is certain)
void issue_receipt(ForwardCall& c, char* bin_chunk_or_null) {
    gsr_forward_args* const a = c.a;
    gsr_forward_receipt& r = a->receipt;
    r.plan_used = a->plan_used;
    r.num_gaussians = c.n; r.width = a->width; r.height = a->height;
    r.tile_row_begin = c.d.row_begin; r.tile_row_end = c.d.row_end;
    r.num_rendered = a->num_rendered; r.num_visible = c.counts.visible;
    r.serial = c.serial;
    r.geometry_chunk = c.geo_chunk; r.image_chunk = c.img_chunk; r.binning_chunk = bin_chunk_or_null;
    r.async_words = c.async_words;
    r.tile_history = a->tile_history;
    r.magic = GSR_RECEIPT_MAGIC;
}

// Slow tiles first (TileOrder, blend_core.hpp): the order of this call's blend workgroups is sorted from the tile times of
// the history's last frame while the depth sort runs, on the library's second stream. Which history: the caller's, or
// this thread's own for the call's stream (a call of another size starts from zeros = patch order).
int step_tile_history(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    GSR_TRY(current_device_shape(&c.shape));
    GSR_TRY(history_of_call(*a, c.d, c.env.tile_history, c.stream, c.rb, &c.hist));
    // The ticks are recorded by every call, the order is sorted when step_history says so (frame_policy.hpp)
    gsr_tile_history* const hist = c.hist;
    if (!hist) return GSR_OK;
    const int dims_now[4] = {a->width, a->height, c.d.row_begin, c.d.row_end};
    if (memcmp(dims_now, hist->dims, sizeof(dims_now)) != 0) {
        GSR_HIP_TRY(hipMemsetAsync(hist->ticks[0], 0, sizeof(uint32_t) * 2 * (size_t)kTileOrderMax, c.stream));
        memcpy(hist->dims, dims_now, sizeof(dims_now));
        hist->view.wanted = hist->view.decorrelated = hist->view.overlapped = false;
        hist->view.calls = 0; hist->stats[0] = 0; hist->view.mean = hist->view.longest = 0; hist->order_serial = 0;
    }
    const bool fresh = hist->stats[0] != 0u;
    const HistoryStep step = step_history(hist->view, fresh ? hist->stats : nullptr, c.tiles, c.shape);
    if (fresh) hist->stats[0] = 0;
    c.view = hist->view = step.view;
    c.order_now = step.order_now;
    ++hist->view.calls;
    c.t_ticks = hist->ticks[hist->cur];                 // (this call's times; the order is sorted from the other set)
    hist->cur ^= 1;
    return GSR_OK;
}

// geomState.rgb of the Gaussians [first, first + count) on stream `s`
int launch_colors(ForwardCall& c, size_t first, int count, hipStream_t s) {
    return launch_colors_visible(count, c.geom.tiles_touched + first, c.a->shs ? c.a->shs + 48u * first : nullptr, c.geom.rgb + 3u * first, s);
}
// ... on the second stream, behind what the caller's stream holds now; `pending` for the call's SideJoin
int fork_colors(ForwardCall& c, size_t first, int count) {
    Readback& rb = c.rb;
    GSR_HIP_TRY(hipEventRecord(rb.ev_pre_blend, c.stream));
    GSR_HIP_TRY(hipStreamWaitEvent(rb.side, rb.ev_pre_blend, 0));
    c.join.tail = true;
    GSR_TRY(launch_colors(c, first, count, rb.side));
    GSR_HIP_TRY(hipEventRecord(rb.ev_colors, rb.side));
    c.join.pending = rb.ev_colors;
    c.join.tail = false;
    return GSR_OK;
}

// geomState.rgb (GSCuda.cu:362-366) is a strided read nothing needs before the blend: by default it is written by a kernel
// of its own on the second stream while the scan and the depth sort run (launch_colors_visible, preprocess.hip) — or
// beside the blend (choose_early, frame_policy.hpp). Whatever way the call ends, the caller's stream has waited for it
// (the chunk is the caller's).
int preprocess_and_fork_colors(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    const GeoScratch& gs = c.gs;
    c.early = choose_early(c.n, a->flags, a->colors_precomp != nullptr, c.xy_plan, c.view, c.tiles, c.env, c.shape);
    const int colors_mode = c.early.colors_mode;
    if (colors_mode != 0) GSR_TRY(c.rb.ensure_colors());
    GSR_TRY(c.begin(GSR_STAGE_PREPROCESS));
    if (c.inria)
        GSR_TRY(launch_preprocess_inria(*a, c.geom, c.radii, gs.depth_key, c.xy_plan ? gs.rect_idx : nullptr, c.d, c.stream, gs.wave_sums, kBigSplatTiles));
    else
        GSR_TRY(launch_preprocess(*a, c.geom, c.radii, gs.depth_key, c.xy_plan ? gs.rect_idx : nullptr, c.d, c.stream, gs.wave_sums,
                                  colors_mode != 0, kBigSplatTiles));   // :744-768
    GSR_TRY(c.end(GSR_STAGE_PREPROCESS));
    // Forked right behind the preprocess (tilesTouched is final there): the scan's and the compaction's small launches
    // leave most of the chip idle, and what the colours kernel gets done beside them it does not take from the depth passes
    // (forked behind the read-back's event instead — no event of its own on the caller's stream — the three passes took
    // 151 us for their 108: bench frame 1.215 -> 1.205 ms, from outside the cloud 1.52 -> 1.49, (0,0,-30) 1.42 -> 1.39).
    // Mode 2: the first colors_early of them only, the rest beside the blend further down.
    if (colors_mode == 1 || c.early.colors_early != 0u) GSR_TRY(fork_colors(c, 0, colors_mode == 1 ? c.n : (int)c.early.colors_early));
    return GSR_OK;
}

DepthTriple with_rects(const DepthTriple& t, bool keep) { return DepthTriple{t.k, t.v, keep ? t.r : nullptr}; }

// The scan of tilesTouched, and what the depth order needs before its passes: the compaction (or the digit counts alone)
// and the event behind the kernels that write the pinned host words.
int scan_and_prepare_depth_order(ForwardCall& c) {
    const GeoScratch& gs = c.gs;
    GSR_TRY(c.begin(GSR_STAGE_SCAN));
    // (the same pass counts the Gaussians with a tile per 4096: the offsets of the depth order's compaction below)
    // Its first launch also clears the depth order's four scratch areas (look-back words, tickets, the digit histograms:
    // adjacent in the chunk), and its one-workgroup launch leaves V and the un-wrapped instance count in the pinned host
    // words themselves: a memset and a copy command of their own were two more 5 us stops on this chain of small launches.
    ScanByproducts by;
    by.info = gs.sort_info;
    by.host = c.rb.host_dev;
    by.nonzero = gs.vis_partial;
    by.clear = gs.sweep.ticket;
    by.clear_bytes = 4 * sweep_scratch_bytes((size_t)c.n);
    by.wave_sums = gs.wave_sums;
    by.main_count = gs.main_partial;
    by.side_max = kDepthSideMax;
    by.big = gs.big_partial;
    by.big_from = kBigSplatTiles;
    GSR_TRY(launch_inclusive_scan(c.geom.tiles_touched, c.geom.point_offsets, (size_t)c.n, gs.scan_temp, c.stream, by));      // :771
    GSR_TRY(c.end(GSR_STAGE_SCAN));
    // The sort of reference :794-797 is an LSD radix sort of (tile | depth) keys. Its low
    // half is the same for every key of a Gaussian, so those digit passes run once per
    // Gaussian BEFORE duplication (N keys, not R): depth order here, tile order below.
    GSR_TRY(c.begin(GSR_STAGE_DEPTH_ORDER));
    // "a bounded look-back spin gave up" is written by the kernel straight into the pinned host words (it never
    // happens on a healthy device; a copy at the end of every frame for it cost 5 us of stream time)
    for (int i = 0; i < 4; ++i) { c.four[i] = i ? gs.sweep_more[i - 1] : gs.sweep; c.four[i].error_word = c.err_n; c.four[i].error_value = c.serial; }
    // Only Gaussians with at least one tile in this call take part from here on (V of N: 52 % on the
    // bench frame, a few per cent per rank when the frame is sharded): their (depth key, index) pairs
    // are compacted in index order — the same kernels count the digits of the four sort passes.
    // With a packed rectangle per Gaussian (grids up to 255 x 255) the rectangle travels with the index through the depth
    // passes: both binning plans want it in depth order, and gathering it by index afterwards is a random 4-byte read per
    // Gaussian (0.93 ms of the 50 M frame).
    // (the depth keys are float bits of NDC z: nearly every visible Gaussian has z in [0.5, 1) and the top byte 0x3F; the
    // handful that does not — 23 of 3 M on the bench frame — goes a side way instead of costing everybody a fourth pass)
    DepthSide& side = c.side;
    side.words = gs.sort_info + kInfoSide;
    side.main_partial = gs.main_partial;
    side.keys = gs.side.k; side.vals = gs.side.v; side.rects = c.xy_plan ? gs.side.r : nullptr;
    side.capacity = kDepthSideMax;
    // (beyond 16 M Gaussians, early.fused_depth: no compaction — the first depth pass leaves out what has no tile)
    if (c.early.fused_depth) {
        GSR_TRY(sort_u32_prepare_counts(gs.depth_key, (uint32_t)c.n, c.four, gs.sort_info, c.stream, c.rb.host_dev, &side));
    } else {
        DepthPrepare p;
        p.keys_in = gs.depth_key;
        p.rect_by_index = c.xy_plan ? gs.rect_idx : nullptr;
        p.out = with_rects(gs.c, c.xy_plan);
        p.partial = gs.vis_partial;
        p.offsets_ready = true;
        p.sc4 = c.four;
        p.info = gs.sort_info;
        p.host = c.rb.host_dev;
        p.side = &side;
        GSR_TRY(sort_u32_prepare(p, (uint32_t)c.n, c.stream));
    }
    // :772 — the pipeline's one device->host read: the binning chunk is sized by R. The host waits for the
    // copies only (an event). They also bring V and whether the fourth depth pass is needed: depth keys are
    // float bits, and when every visible Gaussian has the same top byte (NDC z in [0.5, 1)) that pass would
    // move nothing.
    // (no copy command: the kernels that computed the three figures wrote them into the pinned words as well; numRendered
    // is the low word of the un-wrapped instance count)
    GSR_HIP_TRY(hipEventRecord(c.rb.ev_r, c.stream));
    return GSR_OK;
}

// The first three depth passes are needed whatever the read-back says, so they are queued BEFORE the host waits
// (grids sized for N keys, the true count V read on the device): the device sorts while the host sleeps.
// (early.depth_records: between the passes the triples travel as 12-byte records — in the room of the compaction's arrays
// where there is no compaction, else in that of the first pass's destination (dead before the last pass writes its three
// arrays there), and in the other pair's)
int queue_depth_passes(ForwardCall& c) {
    const GeoScratch& gs = c.gs;
    DepthPasses p;
    p.sc4 = c.four;
    p.first = 0; p.last = 3;
    p.n_dev = gs.sort_info + kInfoVisible;
    p.rec_b = c.early.depth_records ? gs.b.k : nullptr;
    if (c.early.fused_depth) {
        p.in = DepthTriple{gs.depth_key, nullptr, gs.rect_idx};
        p.a = gs.a; p.b = gs.b;
        p.drop_side = &c.side;
        p.rec_a = c.early.depth_records ? gs.c.k : nullptr;
    } else {
        p.in = with_rects(gs.c, c.xy_plan);
        p.a = with_rects(gs.a, c.xy_plan); p.b = with_rects(gs.b, c.xy_plan);
        p.rec_a = c.early.depth_records ? gs.a.k : nullptr;
    }
    GSR_TRY(sort_u32_passes(p, (uint32_t)c.n, c.stream));
    if (c.order_now) {
        // (behind the same event — it follows the history's last blend in stream order — and queued while the host would
        // only wait: nothing is added to the caller's stream, and by the time the blend is launched the order is there)
        // From here until this call's blend has been launched the order belongs to no call (a backward of an earlier one
        // must not take it: order_serial).
        gsr_tile_history* const hist = c.hist;
        hist->order_serial = 0;
        GSR_HIP_TRY(hipStreamWaitEvent(c.rb.side, c.rb.ev_r, 0));
        bool sorted = false;
        GSR_TRY(launch_tile_order(c.d, hist->ticks[hist->cur], c.t_ticks, hist->order, hist->stats_dev, c.rb.side, &sorted, hist->deep, c.shape));
        if (sorted) GSR_HIP_TRY(hipEventRecord(hist->ev_order, c.rb.side));
        else c.order_now = false;                               // (no room for the sort on this device: patch order)
    }
    return GSR_OK;
}

// The host's one wait, the decoded read-back, and what of the depth order depends on it: the fourth pass, the side list.
int read_back_and_finish_depth_order(ForwardCall& c) {
    const GeoScratch& gs = c.gs;
    GSR_HIP_TRY(hipEventSynchronize(c.rb.ev_r));
    const FrameCounts& k = c.counts = decode_host_words(c.rb.host);
    // The reference's offsets are u32 (AuxBuffer.cuh:51): a frame whose instance count does not fit them would size
    // the binning chunk by the wrapped count while the emission writes per true count. Refused before anything
    // R-sized is touched (launch_sort_pairs draws the same line at n >= 0xFFFFFFFF).
    if (k.total >= 0xFFFFFFFFull) return GSR_ERR_TOO_LARGE;
    // (side_listed: the keys the compaction actually put on the side list — it must be the count the scan decided on, or
    // depth_side_kernel would rank entries of an earlier frame)
    // (without the compaction the side list is filled by the first depth pass, which may still be running: its count is not known here)
    if (k.side_way && (k.four_passes || k.side_m > kDepthSideMax || k.side_lo > k.side_m || k.side_m > k.visible ||
                       (!c.early.fused_depth && k.side_listed != k.side_m)))
        return GSR_ERR_INTERNAL;
    if (k.four_passes) {
        DepthPasses p;
        p.in = with_rects(gs.c, c.xy_plan);
        p.a = with_rects(gs.a, c.xy_plan); p.b = with_rects(gs.b, c.xy_plan);
        p.sc4 = c.four;
        p.first = 3; p.last = 4;
        GSR_TRY(sort_u32_passes(p, k.visible, c.stream));
    }
    if (k.side_way)
        GSR_TRY(launch_depth_side(c.side, k.side_m, k.side_lo, k.visible - k.side_m, gs.a.k, gs.a.v, c.xy_plan ? gs.a.r : nullptr, c.stream));
    // depth-sorted keys / indices, and the other pair of buffers (free from here on)
    c.sorted = k.four_passes ? gs.b : DepthTriple{gs.a.k - k.side_lo, gs.a.v - k.side_lo, gs.a.r - k.side_lo};
    c.spare_k = k.four_passes ? gs.a.k : gs.b.k;
    c.R = (uint32_t)k.total;                               // (= pointOffsets[N - 1], GSCuda.cu:772)
    c.a->num_rendered = c.R;
    return GSR_OK;
}

float t_cutoff(const ForwardCall& c) { return c.inria ? 0.0001f : 0.001f; }                 // :653 / upstream

// What every blend of the call reads and writes (the colours, the staged counter and the depth channel: the caller's to add)
BlendIO blend_io(const ForwardCall& c, const float* colors) {
    BlendIO io;
    io.ranges = c.img.ranges;
    io.means2D = c.geom.means2D;
    io.colors = colors;
    io.conic_opacity = c.geom.conic_opacity;
    io.final_t = c.img.accum_alpha;
    io.n_contrib = c.img.n_contrib;
    io.background = c.a->background;
    io.out_color = c.a->out_color;
    io.t_cutoff = t_cutoff(c);
    return io;
}

// R == 0: no binning chunk, no lists
int finish_without_instances(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    // (no record: the depth channel is zero on every pixel of the processed rows)
    if (a->out_depth) {
        const int y0 = c.d.row_begin * kTile, y1 = std::min(c.d.row_end * kTile, a->height);
        if (y1 > y0)
            GSR_HIP_TRY(hipMemsetAsync(a->out_depth + (size_t)y0 * (size_t)a->width, 0, sizeof(float) * (size_t)(y1 - y0) * (size_t)a->width, c.stream));
    }
    // (colours beside the blend: there is no blend — the zeros of a frame without a tile are written here)
    if (c.early.colors_mode == 2) GSR_TRY(launch_colors(c, c.early.colors_early, (int)c.colors_rest(), c.stream));
    if (c.inria) {
        // upstream still runs the tile loop: every pixel gets the background (the reference returns here, :775-778)
        GSR_HIP_TRY(hipMemsetAsync(c.img.ranges, 0, sizeof(uint32_t) * 2 * (size_t)c.num_tiles, c.stream));
        GSR_TRY(launch_blend(c.d, blend_io(c, a->colors_precomp ? a->colors_precomp : c.geom.rgb), nullptr, c.stream));
    }
    issue_receipt(c, nullptr);               // (after the last step that can fail)
    return GSR_OK;
}

// The binning chunk, and which plan fills it.
// Tile grids up to 255 x 255: the tile-column pass is produced directly by a column-major
// emission and only the tile-row pass runs as a sort. Larger grids: depth-ordered emission and
// 8-bit digit passes over the tile bits.
// Two binning plans give the same sorted lists. "blocks": the lists are written directly by
// tile-block owners (blockbin.hip), nothing R-sized is sorted. "sort": column-major emission +
// one onesweep pass on the tile row. Which one, and the block plan's blend: choose_binning (frame_policy.hpp).
int plan_binning(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    c.bin_chunk = a->binning_alloc(a->binning_user, gsr_required_binning(c.R) + 128);    // :782-784
    if (!c.bin_chunk) return GSR_ERR_ALLOC;
    gsr_binning_from_chunk(c.bin_chunk, c.R, &c.bin);
    c.bs = carve_bin_scratch(c.bin.sorting_space, c.R);
    c.plan = choose_binning(c.R, c.counts.visible, c.counts.big_instances, c.xy_plan, blockbin_supported(c.d.grid_x, c.d.grid_y),
                            a->flags, c.view, c.tiles, c.shape);
    a->plan_used = c.plan.plan_used;
    if (c.hist) { c.hist->view.overlapped = c.plan.overlap; c.hist->view.block_fed = c.plan.block_fed; }     // (what the next call reads of this one)
    // (the block plan has no R-sized sort: sortingSpace then holds its unit tables, not look-back words)
    if (!c.plan.use_blocks)
        GSR_HIP_TRY(hipMemsetAsync(c.bs.sweep.error_word, 0, 128 + 256 * sizeof(uint32_t), c.stream));   // error word + tile-row histogram
    // (before the streams fork: the blend may run on the side stream)
    if (c.count_staged) GSR_HIP_TRY(hipMemsetAsync(c.rb.staged_dev, 0, sizeof(unsigned long long), c.stream));
    return GSR_OK;
}

// keysUnsorted / valuesUnsorted hold the block lists (rectangle | depth bits, index) in the block plan
BlockLists block_lists(const ForwardCall& c) {
    BlockLists l;
    l.n = c.nv();
    l.grid_x = c.d.grid_x; l.grid_y = c.d.grid_y;
    l.r_total = c.R;
    l.geo_scratch = c.gs.block_scratch;
    l.bin_scratch = c.bin.sorting_space;
    l.ent_rd = c.bin.keys_unsorted;
    l.ent_idx = c.bin.values_unsorted;
    return l;
}

// The block plan: block lists, unit masks, prefixes and tile ranges, then — unless the caller wants no sorted lists — the emission.
int bin_blocks(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    Readback& rb = c.rb;
    const BlockLists l = block_lists(c);
    GSR_TRY(launch_block_binning(l, c.sorted, c.img.ranges, c.inria, c.stream, c.profile ? rb.ev_end(GSR_STAGE_DEPTH_ORDER) : nullptr,
                                 c.gs.sort_info + kInfoNonemptyTiles, (a->flags & GSR_FLAG_NO_SORTED_LISTS) ? c.bin.values : nullptr,
                                 c.shape.cus));
    // depth order + block lists | unit masks + prefixes + ranges (recorded as "sort_pass1") | emission
    if (c.profile) rb.ev_alias_begin(GSR_STAGE_SORT_PASS1, GSR_STAGE_DEPTH_ORDER);
    GSR_TRY(c.end(GSR_STAGE_SORT_PASS1));
    c.mark(GSR_STAGE_DEPTH_ORDER);
    // plan.overlap: the emission runs beside the blend, which goes to the second stream, and the caller's stream waits
    // for it before gsr_forward's work is complete — each of the two kernels then runs ~20 % longer while they share the
    // chip, so per-kernel times are no longer those of the kernels alone.
    // (the emission stays on the caller's stream and is launched first: its persistent workgroups must be resident
    // before the blend's thousands of waves arrive — the other way round the blend takes every register file and the
    // emission starts when the blend is nearly over: no gain)
    if (c.plan.overlap) {
        GSR_TRY(rb.ensure_side());
        GSR_HIP_TRY(hipEventRecord(rb.ev_fork, c.stream));
        GSR_HIP_TRY(hipStreamWaitEvent(rb.side, rb.ev_fork, 0));
        c.join.tail = true;                          // (until the join at the end of the call has been queued)
    }
    // (What a gsr_backward call after this one may use — the block lists and, for its per-entry gradient sums, the
    // bytes of keysUnsorted — it works out from the receipt: lists_of_receipt.)
    // GSR_FLAG_NO_SORTED_LISTS: this plan's blend reads the block lists, and no caller of the reference reads
    // BinningState (GSGaussians.cpp:214-219 maps GeometryState only): a forward-only caller may skip the 12 R
    // bytes of sorted keys / values altogether. keys / values are then left unwritten.
    // (plan_used then carries GSR_PLAN_LISTS_SKIPPED; values[0] = GSR_LISTS_SKIPPED_STAMP: written with the tile ranges)
    if (!(a->flags & GSR_FLAG_NO_SORTED_LISTS)) {
        GSR_TRY(c.begin(GSR_STAGE_DUPLICATE));
        GSR_TRY(launch_block_emit(l, c.bin.keys, c.bin.values, c.stream, c.plan.overlap, c.shape.cus));
        GSR_TRY(c.end(GSR_STAGE_DUPLICATE));
    }
    return GSR_OK;
}

// :800-801 (the sort plans; under the block plan the ranges are the tile starts it has already computed)
int tile_ranges(ForwardCall& c) {
    GSR_TRY(c.begin(GSR_STAGE_RANGES));
    GSR_TRY(launch_tile_ranges(c.bin.keys, c.R, c.img.ranges, c.num_tiles, c.inria, c.stream, c.gs.sort_info + kInfoNonemptyTiles));
    return c.end(GSR_STAGE_RANGES);
}

// The sort plan on grids up to 255 x 255: column-major emission, then one onesweep pass on the tile row.
int bin_columns(ForwardCall& c) {
    const FrameDims& d = c.d;
    const gsr_binning_state& bin = c.bin;
    uint32_t* hist_y = c.bs.sweep.hist;
    SweepScratch bsw = c.bs.sweep;
    bsw.error_word = c.err_r; bsw.error_value = c.serial;
    if (d.grid_y > 1) GSR_TRY(sweep_clear(bsw, c.R, (uint32_t)d.grid_y, c.stream));
    // one pass: with a single tile row the column-major list is already the sorted list
    uint64_t* emit_k = d.grid_y > 1 ? bin.keys_unsorted : bin.keys;
    uint32_t* emit_v = d.grid_y > 1 ? bin.values_unsorted : bin.values;
    // the depth-order stage ends and the emission stage starts at an event inside the launcher
    GSR_TRY(launch_emit_columns(c.nv(), c.sorted.k, c.sorted.v, c.sorted.r, d.grid_x, d.grid_y, c.gs.emit_scratch, hist_y,
                                emit_k, emit_v, c.stream, c.profile ? c.rb.ev_end(GSR_STAGE_DEPTH_ORDER) : nullptr,
                                c.profile ? c.rb.ev_begin(GSR_STAGE_DUPLICATE) : nullptr));   // :787
    c.mark(GSR_STAGE_DEPTH_ORDER);
    GSR_TRY(c.end(GSR_STAGE_DUPLICATE));
    if (d.grid_y > 1) {
        DigitSpec sy;
        sy.mode = kDigitTileY; sy.shift = 0; sy.nbins = (uint32_t)d.grid_y; sy.grid_x = (uint32_t)d.grid_x;
        sy.inv_grid_x = 1.0f / (float)d.grid_x;
        GSR_TRY(c.begin(GSR_STAGE_SORT_PASS2));
        GSR_TRY(sweep_pass_u64(bin.keys_unsorted, bin.values_unsorted, bin.keys, bin.values, c.R, sy, hist_y, bsw, c.stream, true));
        GSR_TRY(c.end(GSR_STAGE_SORT_PASS2));
    } else {
        // keep the "unsorted" arrays populated as the reference does
        GSR_HIP_TRY(hipMemcpyAsync(bin.keys_unsorted, bin.keys, 8 * (size_t)c.R, hipMemcpyDeviceToDevice, c.stream));
        GSR_HIP_TRY(hipMemcpyAsync(bin.values_unsorted, bin.values, 4 * (size_t)c.R, hipMemcpyDeviceToDevice, c.stream));
    }
    return tile_ranges(c);
}

// Larger grids: depth-ordered emission (the reference's duplicateWithKeys) and 8-bit digit passes over the tile bits.
int bin_generic(ForwardCall& c) {
    const gsr_binning_state& bin = c.bin;
    const int32_t* rects_in = c.inria ? nullptr : c.a->rects;      // upstream rectangles are radius-based
    GSR_TRY(launch_gather_counts(c.nv(), c.sorted.k, c.sorted.v, c.geom.tiles_touched, c.spare_k, c.stream));
    GSR_TRY(launch_inclusive_scan(c.spare_k, c.spare_k, (size_t)c.nv(), c.gs.scan_temp, c.stream));
    GSR_TRY(c.end(GSR_STAGE_DEPTH_ORDER));
    GSR_TRY(c.begin(GSR_STAGE_DUPLICATE));
    GSR_TRY(launch_duplicate(c.nv(), c.sorted.k, c.sorted.v, c.spare_k, c.geom, c.radii, rects_in, c.d, bin.keys_unsorted,
                             bin.values_unsorted, nullptr, nullptr, c.stream));         // :787
    GSR_TRY(c.end(GSR_STAGE_DUPLICATE));
    const int end_bit = 32 + (int)gsr_higher_msb((uint32_t)c.num_tiles);                 // :791
    GSR_TRY(c.begin(GSR_STAGE_SORT_PASS2));
    GSR_TRY(launch_sort_pairs(bin.keys_unsorted, bin.keys, bin.values_unsorted, bin.values, c.R, 32, end_bit,
                              bin.sorting_space, c.stream, c.err_r, c.serial));
    GSR_TRY(c.end(GSR_STAGE_SORT_PASS2));
    return tile_ranges(c);
}

// :803-810 — on the caller's stream, or (plan.overlap) on the second stream beside the emission
int blend(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    Readback& rb = c.rb;
    gsr_tile_history* const hist = c.hist;
    const float* colors = a->colors_precomp ? a->colors_precomp : c.geom.rgb;                // :803
    hipStream_t blend_stream = c.plan.overlap ? rb.side : c.stream;
    // (the colours: long since written — the blend's stream is made to wait only if they are not; a blend on the side stream
    // follows them in stream order, and the caller's stream joins that stream below)
    if (c.join.pending) {
        if (blend_stream == c.stream && hipEventQuery(rb.ev_colors) != hipSuccess) {
            (void)hipGetLastError();
            GSR_HIP_TRY(hipStreamWaitEvent(c.stream, rb.ev_colors, 0));
        }
        c.join.pending = nullptr;
        a->plan_used |= GSR_PLAN_COLORS_BESIDE;
    }
    // (the order: long since sorted — the blend's stream is made to wait only if it is not)
    if (c.order_now && hipEventQuery(hist->ev_order) != hipSuccess) {
        (void)hipGetLastError();                              // ("not ready" is no error of this call)
        GSR_HIP_TRY(hipStreamWaitEvent(blend_stream, hist->ev_order, 0));
    }
    if (c.order_now && !c.view.decorrelated) a->plan_used |= GSR_PLAN_TILES_REORDERED;
    if (c.view.decorrelated) a->plan_used |= GSR_PLAN_TILE_ORDER_DROPPED;
    // Colours beside the blend (scenes beyond 16 M Gaussians): the blend takes them from the SH array; geomState.rgb is
    // written meanwhile on the other stream — or, where the blend itself runs on the second stream beside the emission,
    // behind it there — and the caller's stream waits for it before the call's work is complete.
    const bool colors_late = c.early.colors_mode == 2;
    if (colors_late && !c.plan.overlap) GSR_TRY(fork_colors(c, c.early.colors_early, (int)c.colors_rest()));     // (joined when gsr_forward is left)
    if (colors_late) { colors = a->shs; a->plan_used |= GSR_PLAN_COLORS_BESIDE; }
    // Deep tiles (blend.hip): choose_blend, frame_policy.hpp — with the order as the sort's launch left it
    const BlendChoice deep = choose_blend(c.R, c.counts.visible, c.plan.block_fed, c.order_now, c.early.colors_mode, a->flags, c.view, c.tiles,
                                          c.env.deep_by_history, c.shape);
    if (deep.deep_wanted || deep.deep_all) a->plan_used |= GSR_PLAN_DEEP_TILES;
    BlendIO io = blend_io(c, colors);
    io.colors_are_shs = colors_late;
    io.staged_counter = c.count_staged ? rb.staged_dev : nullptr;
    // The depth channel (out_depth): the blend's DEPTH instantiations, chosen after every per-call rule has decided — the
    // rules of frame_policy.hpp never see it, so a call chooses the same plan, feed, overlap and deep tiles with or without it.
    io.depth.out = a->out_depth;
    io.depth.means3D = a->means3D;
    io.depth.view = a->view_matrix;
    io.depth.inverse = (a->flags & GSR_FLAG_DEPTH_INVERSE) ? 1u : 0u;
    BlendOrder order;
    order.tile_order = c.order_now ? hist->order : nullptr;
    order.tile_ticks = c.t_ticks;
    GSR_TRY(c.begin(GSR_STAGE_BLEND, blend_stream));
    if (c.plan.block_fed) {
        GSR_TRY(launch_blend_blocks(c.d, block_lists(c), io, blend_stream, order));
    } else {
        order.deep_count = deep.deep_wanted ? hist->deep : nullptr;
        order.deep_all = deep.deep_all;
        order.deep_waves = deep.deep_waves;
        GSR_TRY(launch_blend(c.d, io, c.bin.values, blend_stream, c.gs.sort_info + kInfoNonemptyTiles, c.R, order));   // :804-810
    }
    if (c.order_now) hist->order_serial = c.serial;               // (the blend that takes the order is in its stream: a backward of this call may take it too)
    return c.end(GSR_STAGE_BLEND, blend_stream);
}

// The caller's stream joins the second one, and what GSR_FLAG_PROFILE / GSR_FLAG_COUNT_STAGED read after a wait.
int join_and_profile(ForwardCall& c) {
    gsr_forward_args* const a = c.a;
    Readback& rb = c.rb;
    if (c.plan.overlap) {                                                     // the image is complete when the side stream is
        if (c.early.colors_mode == 2) GSR_TRY(launch_colors(c, c.early.colors_early, (int)c.colors_rest(), rb.side));   // (beside the rest of the emission)
        GSR_HIP_TRY(hipEventRecord(rb.ev_join, rb.side));
        GSR_HIP_TRY(hipStreamWaitEvent(c.stream, rb.ev_join, 0));
        c.join.tail = false;
    }
    if (!c.profile && !c.count_staged) return GSR_OK;
    if (c.count_staged)
        GSR_HIP_TRY(hipMemcpyAsync(rb.staged_host, rb.staged_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
    GSR_HIP_TRY(hipStreamSynchronize(c.stream));
    if (c.count_staged) a->records_staged = *rb.staged_host;
    if (c.profile) {
        for (int s = 0; s < GSR_NUM_STAGES; ++s) {
            if (!rb.recorded[s]) continue;
            float ms = 0.0f;
            GSR_HIP_TRY(hipEventElapsedTime(&ms, rb.ev[rb.begin_of[s]], rb.ev_end(s)));
            a->stage_ms[s] = ms;
        }
    }
    return GSR_OK;
}

// The host call sequence of gsr_forward (DESIGN.md lists it)
int forward_stages(ForwardCall& c) {
    GSR_TRY(carve_chunks(c));
    claim_error_slot(c);
    GSR_TRY(step_tile_history(c));
    GSR_TRY(preprocess_and_fork_colors(c));
    GSR_TRY(scan_and_prepare_depth_order(c));
    GSR_TRY(queue_depth_passes(c));
    GSR_TRY(read_back_and_finish_depth_order(c));
    if (c.R == 0) return finish_without_instances(c);
    GSR_TRY(plan_binning(c));
    GSR_TRY(c.plan.use_blocks ? bin_blocks(c) : c.xy_plan ? bin_columns(c) : bin_generic(c));
    GSR_TRY(blend(c));
    GSR_TRY(join_and_profile(c));
    issue_receipt(c, c.bin_chunk);
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

uint32_t gsr_higher_msb(uint32_t n) {   // GSCuda.cu:481-502
    int msb = (int)sizeof(uint32_t) * 4;
    int step = msb;
    while (step > 1) {
        step /= 2;
        if (n >> msb) msb += step; else msb -= step;
    }
    if (n >> msb) msb++;
    return (uint32_t)msb;
}

int gsr_last_error(void) { return g_last_error; }
const char* gsr_last_hip_error(void) { return g_hip_error; }
const char* gsr_error_string(int code) {
    switch (code) {
        case GSR_OK: return "ok";
        case GSR_ERR_INVALID_ARG: return "invalid argument";
        case GSR_ERR_ALLOC: return "chunk allocator returned NULL";
        case GSR_ERR_HIP: return "HIP runtime error";
        case GSR_ERR_NO_DEVICE: return "no HIP device";
        case GSR_ERR_TOO_LARGE: return "numRendered exceeds 32-bit offsets";
        case GSR_ERR_INTERNAL: return "radix sort look-back gave up (bounded spin expired)";
        case GSR_ERR_STALE_RECEIPT: return "the receipt's error slot has been handed to a later call";
        default: return "unknown error";
    }
}

size_t gsr_scan_temp_bytes(size_t n) { return scan_temp_bytes(n); }
static int inclusive_scan_impl(const uint32_t* in, uint32_t* out, size_t n, char* temp, void* stream) {
    if (n && (!in || !out || !temp)) return GSR_ERR_INVALID_ARG;
    return launch_inclusive_scan(in, out, n, temp, (hipStream_t)stream);
}
int gsr_inclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, char* temp, void* stream) {
    return entry_point(inclusive_scan_impl, in, out, n, temp, stream);
}
size_t gsr_sort_temp_bytes(size_t n) { return sort_temp_bytes(n); }
static int sort_pairs_impl(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* values_in, uint32_t* values_out, size_t n,
                           int begin_bit, int end_bit, char* temp, void* stream) {
    if (n && (!keys_in || !keys_out || !values_in || !values_out || !temp)) return GSR_ERR_INVALID_ARG;
    return launch_sort_pairs(keys_in, keys_out, values_in, values_out, n, begin_bit, end_bit, temp, (hipStream_t)stream);
}
int gsr_sort_pairs_u64_u32(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* values_in,
                           uint32_t* values_out, size_t n, int begin_bit, int end_bit, char* temp, void* stream) {
    return entry_point(sort_pairs_impl, keys_in, keys_out, values_in, values_out, n, begin_bit, end_bit, temp, stream);
}

// (three calls whose launchers, in preprocess.hip and blend.hip, refuse what the call refuses)
int gsr_colors_from_dc(int n, const float* shs, float* colors, void* stream) { return entry_point(launch_colors_from_dc, n, shs, colors, (hipStream_t)stream); }
int gsr_blend_expf(int n, const float* in, float* out, void* stream) { return entry_point(launch_exp_test, n, in, out, (hipStream_t)stream); }
int gsr_footprint_misses_tile(int n, const float* means2D, const float* conic_opacity, const int32_t* tile_xy, int width,
                              int height, uint8_t* misses, void* stream) {
    return entry_point(launch_footprint_test, n, means2D, conic_opacity, tile_xy, width, height, misses, (hipStream_t)stream);
}

static int poll_async_error_impl(const gsr_forward_receipt* r) {
    if (!r || r->magic != GSR_RECEIPT_MAGIC || !r->async_words) return GSR_ERR_INVALID_ARG;
    const volatile uint32_t* w = r->async_words;
    // (the kernels write the owning call's serial, not 1: a late writer of an older call cannot raise the new owner's flag)
    if (w[kAsyncErrN] == r->serial || w[kAsyncErrR] == r->serial) return GSR_ERR_INTERNAL;
    if (w[kAsyncSerial] != r->serial) return GSR_ERR_STALE_RECEIPT;   // the slot has a new owner: nothing is known about that call any more
    return GSR_OK;
}
int gsr_poll_async_error(const gsr_forward_receipt* r) { return entry_point(poll_async_error_impl, r); }

static int forward_impl(gsr_forward_args* a) {
    if (!a || a->struct_size != sizeof(gsr_forward_args)) return GSR_ERR_INVALID_ARG;
    a->num_rendered = 0;
    a->records_staged = 0;
    a->plan_used = 0;
    memset(a->stage_ms, 0, sizeof(a->stage_ms));
    memset(&a->receipt, 0, sizeof(a->receipt));
    Readback* rb = nullptr;
    GSR_TRY(check_arguments(a, &rb));
    ForwardCall call(a, *rb);                  // (its SideJoin: the caller's stream waits for the second one however the stages end)
    return forward_stages(call);
}
int gsr_forward(gsr_forward_args* a) { return entry_point(forward_impl, a); }

}  // extern "C"
