/* gsrast_amd.h — C ABI of the MI355X (gfx950) forward Gaussian-splat rasterizer.
 *
 * Drop-in boundary for the reference's rasterizer entry point
 *   gscuda::forward            apps/gsrast/gscuda/GSCuda.cuh:103-126 (def. GSCuda.cu:695-811)
 *   ≅ CudaRasterizer::Rasterizer::forward (apps/gsrast/GSGaussians.cpp:18-23)
 * and for the chunk-layout helpers its callers re-derive pointers with
 *   gscuda::required<T>, gs::{Geometry,Image,Binning}State::fromChunk
 *                              apps/gsrast/gscuda/AuxBuffer.cuh:8-14,38-76, AuxBuffer.cu:13-21,44-89
 *
 * The reference interface is a C++ ABI (by-value std::function, namespaces); this header is
 * the plain-C core a binding targets. include/gscuda_shim.hpp re-creates the exact C++
 * signature on top of it. All pointers named "device" are HIP device pointers owned by
 * the caller. Everything a frame needs lives in the caller's chunks; what the library itself allocates, once per host
 * thread and device, is listed here in full: 1 KB of pinned host memory (the numRendered read-back and the calls' error
 * words), a second stream of the lowest priority and a handful of events, an 8-byte device counter (GSR_FLAG_COUNT_STAGED
 * only), and per tile history (below: one per stream the thread calls on, at most eight, or the caller's own
 * gsr_tile_history) 384 KB of device memory and 64 bytes of pinned host memory. None of it influences any output. The
 * reference owns nothing (GSCuda.cu:723-784: caller chunks only), so all of it can be given back: gsr_thread_release()
 * frees what the CALLING thread's calls have allocated, and the library does the same by itself when a thread that called
 * it ends — a host that renders from short-lived worker threads keeps nothing behind.
 */
#ifndef GSRAST_AMD_H
#define GSRAST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_VERSION 1

/* Error codes (gsr_forward's return value; the reference returns void and its caller
 * polls the runtime's sticky error, apps/gsrast/CudaBuffer.hpp:8-12). */
enum {
    GSR_OK = 0,
    GSR_ERR_INVALID_ARG = 1,   /* null pointer / non-positive size / bad struct_size      */
    GSR_ERR_ALLOC = 2,         /* an allocator callback returned NULL                      */
    GSR_ERR_HIP = 3,           /* a HIP runtime call or kernel launch failed               */
    GSR_ERR_NO_DEVICE = 4,     /* no gfx950 device visible                                 */
    GSR_ERR_TOO_LARGE = 5,     /* sum of tiles touched >= 2^32 - 1: does not fit the reference's u32 offsets (checked
                                  on the un-wrapped 64-bit total before the binning chunk is requested) */
    GSR_ERR_INTERNAL = 6,      /* a bounded device-side wait expired (see gsr_poll_async_error) */
    GSR_ERR_STALE_RECEIPT = 7  /* gsr_poll_async_error: the receipt's error slot belongs to a later call (64 calls on): unknown */
};

/* Chunk allocator: replaces std::function<char*(size_t)> (GSCuda.cuh:103-105). Must
 * return device memory of at least `bytes` bytes, 128-byte aligned or better. */
typedef char* (*gsr_alloc_fn)(void* user, size_t bytes);

/* gs::GeometryState (AuxBuffer.cuh:38-54); field order = carve order (AuxBuffer.cu:44-63). */
typedef struct gsr_geometry_state {
    uint32_t* tiles_touched;   /* u32[N]                                   */
    size_t    scan_size;       /* bytes of scanning_space                  */
    uint32_t  num_rendered;    /* host copy of point_offsets[N-1]          */
    char*     scanning_space;  /* scan scratch (this library's own layout) */
    float*    depths;          /* f32[N]  NDC z                            */
    uint8_t*  clamped;         /* bool[3N], never written (as reference)   */
    int32_t*  internal_radii;  /* i32[N]                                   */
    float*    means2D;         /* vec2[N]                                  */
    float*    cov3D;           /* f32[6N]                                  */
    float*    conic_opacity;   /* vec4[N]                                  */
    float*    rgb;             /* vec3[N], 12-byte stride                  */
    uint32_t* point_offsets;   /* u32[N] inclusive scan of tiles_touched   */
} gsr_geometry_state;

/* gs::ImageState (AuxBuffer.cuh:56-63). `size` = width*height. */
typedef struct gsr_image_state {
    uint32_t* ranges;          /* uvec2[size]; only the first ceil(W/16)*ceil(H/16) are used */
    uint32_t* n_contrib;       /* u32[size]                                */
    float*    accum_alpha;     /* f32[size] final transmittance            */
} gsr_image_state;

/* gs::BinningState (AuxBuffer.cuh:65-75). `size` = numRendered. */
typedef struct gsr_binning_state {
    uint64_t* keys_unsorted;   /* u64[R] (tile << 32) | depth bits         */
    uint64_t* keys;            /* u64[R] sorted                            */
    uint32_t* values_unsorted; /* u32[R] Gaussian index                    */
    uint32_t* values;          /* u32[R] sorted                            */
    size_t    sorting_size;    /* bytes of sorting_space                   */
    char*     sorting_space;   /* radix-sort scratch                       */
} gsr_binning_state;

/* fromChunk: carve the sub-arrays out of `chunk`; returns the advanced chunk pointer
 * (the reference advances a char*& in place). */
char* gsr_geometry_from_chunk(char* chunk, int num_gaussians, gsr_geometry_state* out);
char* gsr_image_from_chunk(char* chunk, int size, gsr_image_state* out);
char* gsr_binning_from_chunk(char* chunk, size_t size, gsr_binning_state* out);
/* required<T>(n): fromChunk on a null base (AuxBuffer.cuh:8-14). */
size_t gsr_required_geometry(int num_gaussians);
size_t gsr_required_image(int size);
size_t gsr_required_binning(size_t size);

/* Per-stage device times of the last profiled gsr_forward call, in milliseconds. */
enum {
    GSR_STAGE_PREPROCESS = 0,   /* preprocess kernel                                             */
    GSR_STAGE_SCAN = 1,         /* inclusive scan of tiles touched (3 small kernels)             */
    GSR_STAGE_DEPTH_ORDER = 2,  /* per-Gaussian depth sort + N-sized binning preparation         */
    GSR_STAGE_DUPLICATE = 3,    /* key emission kernel                                           */
    GSR_STAGE_SORT_PASS1 = 4,   /* block plan: unit counts + prefixes; else unused               */
    GSR_STAGE_SORT_PASS2 = 5,   /* onesweep kernel, tile-row digit (remaining passes)            */
    GSR_STAGE_RANGES = 6,       /* clear + tile ranges kernel                                    */
    GSR_STAGE_BLEND = 7,        /* blend kernel                                                  */
    GSR_NUM_STAGES = 8
};

#define GSR_FLAG_PROFILE 0x1u   /* record HIP events around every stage into stage_ms       */
#define GSR_FLAG_COUNT_STAGED 0x2u /* count records staged by the blend stage (R_f) into records_staged */
/* Semantics profile of the UPSTREAM rasterizer (graphdeco-inria/diff-gaussian-rasterization) instead
 * of the reference's gscuda variant (SURVEY.md §8a divergence table D1-D12, §8f-2): SH up to degree
 * `sh_dims` on shs laid out [N][16][3], view-space depth keys, cull at view z <= 0.2, half-pixel
 * centre, radius-based square rectangles (`rects` ignored), separate focal lengths, transmittance
 * cut-off 1e-4, R == 1 renders, R == 0 still writes the background. cam_pos is read. A Gaussian whose
 * radius converts to 0 or whose 2-D determinant is not finite (an overflowed covariance) has no tile,
 * like one behind the camera: zeros in every per-Gaussian array. Parity of this profile is unpinned
 * (no upstream source in the reference tree). */
#define GSR_FLAG_SEMANTICS_INRIA 0x4u
/* Binning plan (both produce bit-identical sorted keys / values / ranges; default: chosen per frame: the block plan from 6
 * instances (numRendered) per visible Gaussian up, or when an eighth of the instances belongs to splats of 256 tiles and more —
 * the few hundred background splats of a trained scene seen from outside — whatever the average). PLAN_SORT: column-major key
 * emission + one onesweep radix pass;
 * keysUnsorted / valuesUnsorted then hold the reference's pairs in (tile column, depth) order.
 * PLAN_BLOCKS: the sorted lists are written directly by tile-block owners, no R-sized sort;
 * keysUnsorted / valuesUnsorted then hold that plan's block lists (scratch, as sortingSpace is). */
#define GSR_FLAG_PLAN_SORT 0x8u
#define GSR_FLAG_PLAN_BLOCKS 0x10u
/* Block plan: the blend can run on a second stream beside the emission of the sorted lists — one is bound by vector issue, the
 * other by the HBM write path (or, on light frames, by nothing: a wave per unit) — reading the block lists instead of the sorted
 * ones. Same results; the call's work is complete, as always, when `stream` is. It pays where the blend is the shorter of the
 * two (bench frame 1.34 -> 1.22 ms, 4K 4.21 -> 3.85 ms; faint splats, blend three times the emission: 3.10 -> 3.16), and each
 * kernel runs longer while they share the chip. By DEFAULT the library decides per call, from 16 instances per visible Gaussian
 * up, from the call's tile history (see GSR_FLAG_NO_TILE_HISTORY; without one, or while its frames do not resemble each other:
 * serial) and this call's R: overlapped when the blend — the tiles' times spread over the chip, never less than the longest
 * tile, and 1 + 10 V / R times that if they were measured on a blend fed from the sorted lists — is expected to end before an
 * emission of 12 R bytes at 4 TB/s does (twice that on frames that are block-fed either way; on light frames: before 0.14 ms);
 * plan_used then carries GSR_PLAN_EMIT_OVERLAPPED. GSR_FLAG_OVERLAP_EMIT forces it on (block plan), GSR_FLAG_SERIAL_EMIT off: one
 * kernel after the other on the caller's stream, per-kernel times those of the kernels alone; a serial blend reads the sorted
 * lists below 48 instances per visible Gaussian and the block lists from there on. (`profiles/r05_trained_like.txt`: the
 * library's choice against every forced one on 240 poses of two scene families.) */
#define GSR_FLAG_OVERLAP_EMIT 0x20u
#define GSR_FLAG_SERIAL_EMIT 0x100u
/* (Also by default, gscuda semantics without colors_precomp: geomState.rgb is written by a kernel of its own on the
 * library's second stream — a strided read nothing needs before the blend, 0.10 ms of the bench frame's preprocess. Up to
 * 16 M Gaussians right behind the preprocess, while the scan and the depth sort run (0.02-0.03 ms more there), and the
 * call's stream waits for it before the blend; beyond,
 * where the depth sort is bound by HBM itself, beside the blend, which takes a record's colour straight from `shs` meanwhile
 * (50 M Gaussians: 6.3 -> 5.9 ms). The caller's stream has waited for it on every way out of the call. Same bits.
 * GSR_FLAG_SERIAL_EMIT keeps the colours in the preprocess kernel as well.) */
/* Forward-only callers: under the block plan the blend can be fed from the block lists without reading the sorted
 * keys / values (it is by default on frames of 48 or more instances per visible Gaussian), and no caller of the reference reads BinningState (GSGaussians.cpp:214-219 maps GeometryState
 * only). With this flag such a call skips writing them (12 R bytes): BinningState.keys / values are then left
 * UNWRITTEN except for values[0] = GSR_LISTS_SKIPPED_STAMP, plan_used carries GSR_PLAN_LISTS_SKIPPED, and a gsr_backward
 * call that is given this call's receipt (any thread; chunks untouched) walks the tile lists out of the block lists.
 * Pixels, ranges, finalT, nContrib and numRendered are unchanged. Ignored under the other plans, whose blend
 * reads the sorted list. Default off: the reference's contract (sorted lists in the binning chunk) holds. */
#define GSR_FLAG_NO_SORTED_LISTS 0x40u
/* Slow tiles first. A frame's blend lasts as long as its slowest tiles, and a camera moves little between two frames:
 * every tile's wave leaves how long it ran in a TILE HISTORY, and the next call that is given the same history sorts its
 * blend workgroups by it beside the depth sort, on a stream of the library's (blend 0.61 -> 0.53 ms from (0,0,-30) on the
 * bench scene). Outputs do not depend on it — the same tiles are composited the same way, sooner or later.
 * Which history a call takes: gsr_forward_args.tile_history, a gsr_tile_history the caller created (one per VIEW: a
 * rasterizer object, an eye of a stereo pair) — or, when that is NULL, one the library keeps per host thread, device and
 * STREAM of the call (at most eight streams per thread and device; calls on further streams run without). A history
 * belongs to the stream of the call that used it last: kernels of two calls that share a history are ordered by that
 * stream alone, so calls on different streams never share a default history (a ninth stream takes over the history the
 * thread has not used for the longest time). A caller who moves its OWN history to another stream: the library orders the
 * new stream behind the old one's work by an event it records on the OLD stream at that moment — which must therefore
 * still exist; a caller that has destroyed it (after waiting for it) says so first: gsr_tile_history_forget_stream. A history whose frames stop resembling each other — a trainer that draws an
 * unrelated camera every call, two views alternating on one history — is noticed (the two last frames' tile times are
 * compared when the order is sorted: each tile's SHARE of its frame's total tile time, the smaller of its two shares summed
 * over the tiles, below 0.8) and the order is dropped, patch order as without a history, until they do again: plan_used
 * then carries GSR_PLAN_TILE_ORDER_DROPPED. The order is sorted when the statistics of the calls before say the frame ends
 * on a few slow tiles or is a light one, on every call while the order is dropped (the sort is what looks whether the
 * frames resemble each other again), and every fourth call otherwise, to keep the statistics fresh. A history also carries the statistics by which the library decides, per call, whether the
 * blend runs beside the emission (GSR_FLAG_OVERLAP_EMIT). This flag switches all of it off for the call: it neither reads
 * nor writes a history and uses no second stream for it (GSR_TILE_HISTORY=0 in the environment does the same for every
 * call of the process). Frames of more than 32 768 tiles (beyond 3840 x 2160) keep no tile times either: the order is
 * sorted by one workgroup in LDS. */
#define GSR_FLAG_NO_TILE_HISTORY 0x80u
/* Deep tiles (csrc/blend.hip). A blend fed from the sorted lists may give a tile a workgroup of FOUR waves: they walk the
 * tile's list together (one fetch, one footprint test per entry) and composite one 16 x 4 strip each — a wave alone on its
 * SIMD issues a vector instruction every five cycles where the SIMD takes one every two or three, and a frame of small
 * splats lasts as long as the lone waves of its few deep tiles. Same pixels, finalT, nContrib, records_staged: every pixel
 * sees the same records in the same order. By default every tile of a frame with fewer than 16 instances per visible
 * Gaussian is composited that way (and every tile of a call with few tiles: a rank's band of a sharded frame); plan_used
 * then carries GSR_PLAN_DEEP_TILES. GSR_FLAG_NO_DEEP_TILES: never; GSR_FLAG_DEEP_TILES_ALL: whatever the frame (a
 * diagnostic, and what the tests compare the ordinary way against). Neither reads nor needs a tile history. */
#define GSR_FLAG_NO_DEEP_TILES 0x200u
#define GSR_FLAG_DEEP_TILES_ALL 0x400u
/* With deep tiles, EIGHT or SIXTEEN waves per tile (strips of 16 x 2 or 16 x 1 pixels; the upper lanes of a wave idle) instead
 * of four: what the library picks by itself when the view's tile history says the frame's work sits in a few hundred tiles
 * (a far view of a dense scene: a chip with one wave per SIMD issues at 40 % of what two waves per SIMD do). Diagnostics,
 * like GSR_FLAG_DEEP_TILES_ALL, which they imply; same outputs bit for bit. */
#define GSR_FLAG_DEEP_WAVES_8 0x800u
#define GSR_FLAG_DEEP_WAVES_16 0x1000u
/* Depth channel (gsr_forward_args.out_depth, gsr_backward_args.dL_dout_depth): the channel holds inverse depth 1 / z_i
 * instead of z_i. Honoured by gsr_forward and gsr_backward (give both calls the same choice). */
#define GSR_FLAG_DEPTH_INVERSE 0x2000u
enum { GSR_PLAN_SORT = 1, GSR_PLAN_BLOCKS = 2, GSR_PLAN_GENERIC = 3 /* grids wider than 255 tiles */,
       GSR_PLAN_LISTS_SKIPPED = 0x100 /* or-ed in: GSR_FLAG_NO_SORTED_LISTS took effect */,
       GSR_PLAN_BLEND_FROM_LISTS = 0x200 /* or-ed in: block plan whose blend read the sorted lists (sparse frames: fewer
                                            than 48 instances per visible Gaussian), not the block lists */,
       GSR_PLAN_TILES_REORDERED = 0x400 /* or-ed in: the blend started the slow tiles of the call before first
                                           (see GSR_FLAG_NO_TILE_HISTORY; informational) */,
       GSR_PLAN_EMIT_OVERLAPPED = 0x800 /* or-ed in: the blend ran beside the emission (see GSR_FLAG_OVERLAP_EMIT) */,
       GSR_PLAN_COLORS_BESIDE = 0x1000 /* or-ed in: geomState.rgb was written beside the scan / depth sort (or the blend), not by the preprocess */,
       GSR_PLAN_TILE_ORDER_DROPPED = 0x2000 /* or-ed in: the history's last frames did not resemble each other (another view
                                               every call): the blend took the patch order (informational) */,
       GSR_PLAN_DEEP_TILES = 0x4000 /* or-ed in: the blend composited its tiles by four waves each (see GSR_FLAG_NO_DEEP_TILES;
                                       informational) */ };

/* A tile history (see GSR_FLAG_NO_TILE_HISTORY): opaque, created for the CURRENT device, owned by the caller, one per view.
 * gsr_tile_history_destroy: the streams it was used on must be idle. */
typedef struct gsr_tile_history gsr_tile_history;
int gsr_tile_history_create(gsr_tile_history** out);
int gsr_tile_history_destroy(gsr_tile_history* history);
/* What the library last learnt about the history (host side, no device access; for tools and tests): out[0] = mean tile
 * time of its last sorted frame in units of 10 ns (0: none yet), [1] = that frame's longest tile (both as ONE wave would take:
 * a tile composited by four waves counts 2.5 times what it took), [2] = similarity of its two
 * last frames x 1000 (the smaller of a tile's two shares of its frame's tile time, summed over the tiles), [3] = 1 if the order is dropped at present,
 * [4] = calls since the history was last cleared (a new size), [5] = 1 if the last block-plan call ran its blend beside the
 * emission. */
int gsr_tile_history_stats(const gsr_tile_history* history, uint32_t out[6]);

/* The stream the history's last call ran on is gone (the caller waited for it and destroyed it): the next call with this
 * history, on whatever stream, is not ordered behind it. Host side only. */
int gsr_tile_history_forget_stream(gsr_tile_history* history);

/* For tools and tests: the tile times the history's LAST call recorded, times[tile] for the first `count` tiles of the frame
 * (row-major tile index) in units of 10 ns — bit 31 set: the tile was composited by four waves (a deep tile) —, and in
 * *deep_tiles (optional) how many leading entries of the last sorted order were deep tiles. Synchronises the device. */
int gsr_tile_history_times(const gsr_tile_history* history, uint32_t* times, int count, uint32_t* deep_tiles);

/* Gives back everything the library has allocated for the CALLING host thread, on every device (see the list at the top):
 * the second stream is drained first, so nothing of the library's own is in flight afterwards; work the thread's calls put
 * on the CALLER's streams is the caller's to wait for, as ever, before it frees the chunks. Receipts of the thread's
 * earlier calls can no longer be polled (gsr_poll_async_error reads their pinned words: do not pass one afterwards), and a
 * gsr_backward call for one of them runs without the forward's tile order. A later call of the thread starts from nothing
 * again. Also run when the thread ends. Always GSR_OK. */
int gsr_thread_release(void);

/* The environment switches (GSR_TILE_HISTORY, GSR_COLORS_BESIDE, GSR_COLORS_EARLY_PCT, GSR_FUSED_DEPTH, GSR_DEPTH_RECORDS,
 * GSR_DEEP_BY_HISTORY: A/B runs and tests, none needed in production) are read once per process, by the
 * first call that needs them; a test that changes one afterwards calls this to have them read again (no call in flight on
 * another thread meanwhile). */
void gsr_reread_environment(void);

/* The figures the launch heuristics derive from a device's compute-unit count (hipDeviceAttributeMultiprocessorCount, read
 * once per device — an MI355X in a partitioned mode shows fewer): out[0] = CUs, [1] = wave slots of the blend kernels
 * (4 SIMDs x 5 waves per CU), [2] = the same beside the emission's persistent workgroups (3 per SIMD), [3] = [1] again as
 * the divisor of the light-frame rule (250 us of tile time per slot). Pure: no device needed (tests/test_capi_cpu.py). */
void gsr_device_shape(int compute_units, uint32_t out[4]);

/* Receipt of one gsr_forward call: everything a LATER call (gsr_backward, gsr_poll_async_error) needs to know about it.
 * The reference keeps all per-call state in the caller-owned chunks (GSCuda.cu:723-725,734-736,782-784); so does this
 * library — the receipt only says which chunks those were, how many instances (R) and visible Gaussians (V) the call
 * found and which binning plan left which lists there. It is plain data: copy it, hand it to another host thread, keep
 * several (one per rasterizer). It describes the chunks as that call left them, so it is valid until the next
 * gsr_forward call that is given the same chunks. */
#define GSR_RECEIPT_MAGIC 0x31525347u   /* "GSR1" */
/* First word of BinningState.values after a call that left the sorted lists unwritten (GSR_FLAG_NO_SORTED_LISTS took
 * effect): no Gaussian index, so a gsr_backward call WITHOUT a receipt can tell that there is no list to walk. */
#define GSR_LISTS_SKIPPED_STAMP 0xFFFFFFFFu
typedef struct gsr_forward_receipt {
    uint32_t magic;                /* GSR_RECEIPT_MAGIC once gsr_forward has returned GSR_OK, else 0 */
    uint32_t plan_used;            /* as gsr_forward_args.plan_used */
    int32_t  num_gaussians, width, height;
    int32_t  tile_row_begin, tile_row_end;   /* the tile rows the call processed (0, ceil(H/16) for the whole frame) */
    uint32_t num_rendered;         /* R */
    uint32_t num_visible;          /* V: Gaussians with at least one tile in this call */
    uint32_t serial;               /* which call of its host thread and device */
    char*    geometry_chunk;       /* what the three allocator callbacks returned (binning: NULL if R == 0) */
    char*    image_chunk;
    char*    binning_chunk;
    const volatile uint32_t* async_words;   /* host memory (pinned, never freed): {N-sized sort gave up, R-sized sort gave up
                                               (each: 0, or the serial of the call whose kernel gave up), serial of the call
                                               that owns the words, 0} — see gsr_poll_async_error */
    gsr_tile_history* tile_history;         /* gsr_forward_args.tile_history of the call (NULL: one of the library's own). A caller's
                                               history must outlive the receipts that name it (gsr_backward looks into it for
                                               the forward blend's tile order) */
} gsr_forward_receipt;

/* Arguments of one forward call. Fields up to box_max are, in order, the parameters of
 * gscuda::forward (GSCuda.cuh:103-126); the rest are extensions with neutral defaults (0). */
typedef struct gsr_forward_args {
    uint32_t struct_size;          /* = sizeof(gsr_forward_args) */
    uint32_t flags;
    gsr_alloc_fn geometry_alloc;   void* geometry_user;
    gsr_alloc_fn binning_alloc;    void* binning_user;
    gsr_alloc_fn image_alloc;      void* image_user;
    int32_t num_gaussians;
    int32_t sh_dims;               /* D, unused by the gscuda semantics */
    int32_t M;                     /* unused */
    const float* background;       /* device vec3 */
    int32_t width, height;
    const float* means3D;          /* device vec4[N] */
    const float* shs;              /* device f32[48 N], DC first */
    const float* colors_precomp;   /* device vec3[N] or NULL */
    const float* opacities;        /* device f32[N] */
    const float* scales;           /* device vec4[N] */
    float scale_modifier;
    const float* rotations;        /* device vec4[N], real part first */
    const float* cov3D_precomp;    /* device f32[6 N] or NULL */
    const float* view_matrix;      /* device 16 f32 column-major, row 2 negated */
    const float* proj_matrix;      /* device 16 f32 column-major, perspective*view */
    const float* cam_pos;          /* device vec3, unused */
    float tan_fovx, tan_fovy;
    int32_t prefiltered;           /* unused */
    float* out_color;              /* device f32[3 W H], planar CHW */
    int32_t* radii;                /* device i32[N] or NULL (falls back to internal_radii) */
    int32_t* rects;                /* device i32[2 N] or NULL (radius-based rectangles) */
    const float* box_min;          /* unused (reference overrides with -FLT_MAX) */
    const float* box_max;          /* unused */
    /* ---- extensions ---- */
    void* stream;                  /* hipStream_t; NULL = the default stream */
    int32_t tile_row_begin;        /* multi-GPU: only tile rows [begin,end) are binned,   */
    int32_t tile_row_end;          /*   sorted and blended; 0,0 = all rows. In such a call  */
                                   /*   a Gaussian without a tile in the band counts as     */
                                   /*   invisible (radius 0, its geometry fields unwritten) */
    gsr_tile_history* tile_history;/* the view's tile history, or NULL: the library's own for this thread, device and
                                      stream (see GSR_FLAG_NO_TILE_HISTORY) */
    /* ---- outputs ---- */
    uint32_t num_rendered;         /* R = sum of tiles touched (for the rows processed)    */
    uint64_t records_staged;       /* R_f, only with GSR_FLAG_COUNT_STAGED                 */
    float stage_ms[GSR_NUM_STAGES];/* only with GSR_FLAG_PROFILE                           */
    uint32_t plan_used;            /* GSR_PLAN_* of this call (0 if R == 0), | GSR_PLAN_LISTS_SKIPPED */
    gsr_forward_receipt receipt;   /* hand it to gsr_backward / gsr_poll_async_error (magic = 0 unless GSR_OK is returned) */
    /* ---- depth channel (appended: callers that set struct_size = sizeof recompile unchanged) ---- */
    float* out_depth;              /* device f32[W H], or NULL: no depth channel, exactly the call without it. Definition:
                                      per Gaussian, z_i is the view-space depth computed in float in this operation order
                                      (no contraction): z = (V[2]*x + V[6]*y) + (V[10]*z3 + V[14]*1.0f), V = view_matrix,
                                      (x, y, z3) = means3D[i] — positive in front of the camera in both semantics; it is NOT
                                      geomState.depths (NDC z under the gscuda semantics). d_i = z_i, or with
                                      GSR_FLAG_DEPTH_INVERSE d_i = 1.0f / z_i (IEEE division). Per pixel
                                      out_depth[p] = sum d_i alpha_i T_i, accumulated as fmaf(d_i, alpha_i T_i, acc) in the order
                                      and under the tests of the colour channels: no background term, no normalisation (the
                                      accumulated opacity is 1 - accum_alpha: divide by it for expected depth). out_depth equals,
                                      bit for bit, channel 0 of out_color of a call with colors_precomp[i] = (d_i, d_i, d_i) and
                                      a zero background. Every pixel of the processed tile rows is written on every GSR_OK call
                                      (zeros when R == 0, unlike out_color); pixels outside tile_row_begin / _end are not touched. */
} gsr_forward_args;

/* The forward pass. Calls geometry_alloc(required_geometry(N)), then
 * image_alloc(required_image(W*H)+128), then — only if R>0, after the scan —
 * binning_alloc(required_binning(R)+128): once each, in that order (GSCuda.cu:723-784).
 * Synchronises `stream` once mid-call to read R back (GSCuda.cu:772). Returns GSR_*.
 * R == 0 returns GSR_OK and leaves out_color untouched (GSCuda.cu:775-778); out_depth, if given, is zeroed. */
int gsr_forward(gsr_forward_args* args);

/* The error contract. It covers every function of this header that returns a GSR_* code — not the queries that return a
 * size_t, the *_from_chunk functions, gsr_exchange_plan (a count), gsr_higher_msb, gsr_device_shape, gsr_reread_environment
 * and the three functions below. Each covered call forgets the previous HIP text on entry and leaves the code it returns as
 * the calling thread's last error: a successful call sets it to GSR_OK. */
int gsr_last_error(void);
const char* gsr_error_string(int code);
/* Text of the HIP error behind the GSR_ERR_HIP of the calling thread's most recent covered call ("" if it did not fail in HIP). */
const char* gsr_last_hip_error(void);

/* After the caller has synchronised the stream of the gsr_forward call that issued `receipt`: GSR_OK, or
 * GSR_ERR_INTERNAL if a radix-sort look-back wait expired during that call (the frame is then invalid). Mirrors the
 * reference caller polling the sticky error after its sync (CudaBuffer.hpp:8-12). Any thread may ask. The words a call
 * reports into are one of 64 slots per host thread and device, handed out in turn: asked about a call that lies more
 * than 63 calls back the answer is GSR_ERR_STALE_RECEIPT (its slot has a new owner; nothing is known any more). A kernel
 * that gives up writes its own call's serial, so a call still running on another stream when its slot comes round again
 * cannot raise the new owner's flag. NULL or a receipt without the magic: GSR_ERR_INVALID_ARG. */
int gsr_poll_async_error(const gsr_forward_receipt* receipt);

/* getHigherMsb (GSCuda.cu:481-502): bits of the tile id that take part in the sort. */
uint32_t gsr_higher_msb(uint32_t n);

/* ---- stage entry points (unit-level parity tests; all asynchronous on `stream`) ---- */
/* Inclusive u32 prefix sum (replaces cub::DeviceScan::InclusiveSum, GSCuda.cu:771).
 * temp needs gsr_scan_temp_bytes(n) bytes. in == out is allowed. */
size_t gsr_scan_temp_bytes(size_t n);
int gsr_inclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, char* temp, void* stream);
/* Stable LSD radix sort of (u64 key, u32 value) pairs on key bits [begin_bit, end_bit)
 * (replaces cub::DeviceRadixSort::SortPairs, GSCuda.cu:794-797). Inputs are preserved. Bits outside the window take no
 * part: pairs whose windows are equal keep their input order. The window is clamped, in this order: end_bit > 64 becomes 64,
 * begin_bit < 0 becomes 0, and end_bit <= begin_bit becomes begin_bit + 1 (the one bit at begin_bit); begin_bit must be
 * below 64. temp needs gsr_sort_temp_bytes(n) bytes and need not be cleared; n == 0 does nothing. */
size_t gsr_sort_temp_bytes(size_t n);
int gsr_sort_pairs_u64_u32(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* values_in,
                           uint32_t* values_out, size_t n, int begin_bit, int end_bit, char* temp, void* stream);

/* The colours of the reference's semantics, once per scene: colors[3 i + c] = 0.5f + 0.4f * shs[48 i + c] (GSCuda.cu:362-366;
 * the colour does not depend on the view). Passed as `colors_precomp` (GSCuda.cuh:111; the blend then reads them instead of
 * geomState.rgb, GSCuda.cu:803) they spare every frame the 12-byte read at a 192-byte stride — one 128-byte line per visible
 * Gaussian — and the 12 N bytes of geomState.rgb: same pixels bit for bit. Device pointers; asynchronous on stream. */
int gsr_colors_from_dc(int n, const float* shs, float* colors, void* stream);

/* The blend's exponential (csrc/blend_core.hpp, exp_ref: the float exponential of GSCuda.cu:645 computed as glibc's expf
 * computes it), argument by argument: out[i] = exp(in[i]), in[i] <= 0.5 and not NaN; device pointers. For the tests: it must
 * agree bit for bit with the host's expf, which is what makes alpha, T and every threshold decision of the blend those of the CPU oracle. */
int gsr_blend_expf(int n, const float* in, float* out, void* stream);

/* The blend's footprint test (csrc/blend_core.hpp), record by record: misses[i] = 1 iff the library would drop record i
 * (centre means2D[i], conic + opacity conic_opacity[i]) when it stages the list of tile tile_xy[i] = (tx, ty) of a
 * width x height image, i.e. iff it has PROVEN that no pixel of that tile passes alpha >= 1/255 (GSCuda.cu:645-646).
 * All pointers are device pointers. For the tests: a dropped record that could light a pixel would be a parity bug. */
int gsr_footprint_misses_tile(int n, const float* means2D, const float* conic_opacity, const int32_t* tile_xy,
                              int width, int height, uint8_t* misses, void* stream);

/* ---- backward pass (next row after the hot path: BASELINE config 5) ----
 * Gradients of L = sum(dL_dout_color * out_color) of ONE gsr_forward call (gscuda semantics) w.r.t. the
 * per-Gaussian quantities its blend loop reads, and on to the 3-D covariance and the DC harmonics. The
 * reference has no backward pass (parity unpinned); conventions, checked by finite differences in
 * oracle/backward_np.py:
 *   dL_dmean2D        vec2[N]  w.r.t. the pixel-space centre (no NDC factor)
 *   dL_dconic_opacity vec4[N]  w.r.t. (A, B, C) of power = -0.5 (A dx^2 + C dy^2) - B dx dy, and opacity
 *   dL_dcolors        vec3[N]
 *   dL_dcov2D         vec4[N]  w.r.t. the 2-D covariance, (m00, m01, m11, 0) (optional; what the chain below should start from)
 *   dL_dcov3D         f32[6N]  w.r.t. the six stored covariance numbers (optional; without sums_f64, NULL skips the chain)
 *   dL_dshs           f32[48N] colour = 0.5 + 0.4 DC: the DC triple of every Gaussian, = 0.4 dL_dcolors, and zeros in the 13
 *                              floats behind it (one whole 64-byte write per Gaussian; floats 16..47 are not touched);
 *                              optional — a caller that scales dL_dcolors itself saves 0.18 ms of strided writes per frame
 *   dL_dmeans3D       vec4[N]  (x, y, z, 0) through the pixel-space centre and through the Jacobian of cov2D; optional
 *   dL_dscales        vec4[N]  (x, y, z, 0);  dL_drotations vec4[N] w.r.t. the quaternion as given; optional
 *                              (not available when the forward call took cov3D_precomp)
 * Every output is optional once sums_f64 is given (the sums then live there and the float arrays are only copies): a NULL
 * output is not computed where that saves work and never written. The chain writes 150-odd bytes per Gaussian when all are
 * asked for; BASELINE config 5's set (dL_dmean2D, dL_dcov3D, dL_dshs) is 96 of them. Without sums_f64 the three arrays of the
 * sums are required, and dL_dmeans3D / dL_dscales / dL_drotations need dL_dcov3D.
 * Hard tests of the forward (power > 0, alpha < 1/255, transmittance cut-off) select a branch; where
 * alpha is clamped to 0.99 its derivative w.r.t. the Gaussian's parameters is zero. The state pointers are
 * those of the forward call's chunks (gsr_*_from_chunk): it must have run on the same inputs, same size.
 * With flags = GSR_FLAG_SEMANTICS_INRIA (the forward call's flag) the chain is the upstream profile's: two focal
 * lengths, w epsilon 1e-7, the raw quaternion, and colour = max(0, 0.5 + SH(view direction)) — dL_dshs then receives
 * all (sh_dims + 1)^2 coefficient triples of every Gaussian (zeros beyond them and for culled Gaussians; a channel
 * that was clamped at zero passes nothing), and dL_dmeans3D the term through the view direction. */
typedef struct gsr_backward_args {
    uint32_t struct_size;          /* = sizeof(gsr_backward_args) */
    uint32_t flags;                /* GSR_FLAG_PROFILE */
    int32_t num_gaussians, width, height;
    const float* background;       /* device vec3 */
    /* state of the forward call */
    const float* means2D;          /* geometry chunk */
    const float* conic_opacity;
    const float* colors;           /* geometry rgb, or the colors_precomp the forward call was given */
    const float* cov3D;            /* geometry cov3D, or the cov3D_precomp given (only for the chain) */
    const int32_t* radii;          /* internal_radii or the radii buffer given (only for the chain) */
    const uint32_t* ranges;        /* image chunk */
    const uint32_t* n_contrib;
    const float* final_t;          /* accum_alpha */
    const uint32_t* point_list;    /* binning chunk: values (with a receipt: must be the values array of ITS binning chunk) */
    /* inputs of the forward call that the covariance chain needs again */
    const float* means3D;
    const float* view_matrix;
    float tan_fovx, tan_fovy;
    const float* dL_dout_color;    /* device f32[3 W H], planar like out_color */
    /* outputs (device) */
    float* dL_dmean2D;             /* these three: required without sums_f64, optional with it */
    float* dL_dconic_opacity;
    float* dL_dcolors;
    float* dL_dcov3D;              /* or NULL */
    float* dL_dshs;                /* or NULL */
    float* dL_dcov2D;              /* vec4[N] (m00, m01, m11, 0): w.r.t. the full symmetric 2-D covariance (a, b; b, c) of
                                      GSCuda.cu:226-230, summed pixel by pixel by the render backward; or NULL. The chain to
                                      dL_dcov3D and beyond starts from it when given — without it the chain derives it as
                                      -K (dL/dK) K from dL_dconic_opacity, which loses cond(K)^2 of the sums' digits (a splat
                                      that fills the screen: 1e6) */
    double* sums_f64;              /* f64[12 N] scratch or NULL. ZERO on entry, left zero on return. With it the twelve sums of a
                                      Gaussian (the four arrays above) are accumulated in double — a splat that fills the screen
                                      collects terms of either sign from 8 160 tiles, and in float their order of arrival shows
                                      in the fourth digit of its gradients, differently every run — and rounded to float once;
                                      the float arrays need not be cleared by anybody then.
                                      SEEDED SUMS: instead of zeros the rows of Gaussians with radii > 0 may hold, on entry, sums
                                      in this layout that gsr_features_backward (gsrast_amd_features.h: geometry_sums_f64) or
                                      gsr_distortion_backward (gsrast_amd_distortion.h: geometry_sums_f64) of the SAME forward call
                                      and tile rows left there; both may seed the same array before one gsr_backward. They are
                                      added to what the render backward sums
                                      (every output and the chain see the total), and everything is left zero on return; a zero
                                      scratch behaves exactly as before. Every path only ever ADDS to the array before the
                                      per-Gaussian kernel reads, rounds and zeroes it: the render backward's direct double
                                      atomics, and flush_block_acc_kernel's where the block lists feed it. With an empty band of
                                      tile rows neither runs and the per-Gaussian kernel alone reads and zeroes the rows. With
                                      num_rendered == 0 the call returns before that kernel and neither reads nor zeroes the
                                      array — gsr_features_backward of such a receipt adds nothing, so there is nothing to
                                      lose. Rows with radii <= 0 are never read: a seed there would stay (no list names such
                                      a Gaussian, so gsr_features_backward never writes one) */
    /* chain down to the inputs (all optional; without sums_f64 they need dL_dcov3D) */
    const float* proj_matrix;      /* inputs of the forward call */
    const float* scales;
    const float* rotations;
    float scale_modifier;
    float* dL_dmeans3D;            /* or NULL */
    float* dL_dscales;             /* or NULL */
    float* dL_drotations;          /* or NULL (needs dL_dscales) */
    void* stream;
    int32_t tile_row_begin, tile_row_end;   /* as gsr_forward: the rows the forward call processed */
    float stage_ms[2];             /* with GSR_FLAG_PROFILE: render backward, covariance / colour chain */
    /* ---- GSR_FLAG_SEMANTICS_INRIA: the forward call ran with the upstream semantics ---- */
    const float* cam_pos;          /* inputs of the forward call (needed with dL_dshs) */
    const float* shs;              /* device f32[48 N], [16][3] per Gaussian */
    const uint8_t* clamped;        /* geometry chunk: bool[3 N], colour channel was clamped at zero */
    int32_t sh_dims;               /* SH degree the forward call evaluated (0..3) */
    /* ---- which forward call this is the backward of ---- */
    gsr_forward_receipt receipt;   /* gsr_forward_args.receipt of that call, by value. With it the block lists that call left
                                      in its chunks are used where it ran the block plan (all tiles if GSR_FLAG_NO_SORTED_LISTS
                                      left `values` unwritten, else the tiles of shallow blocks, keysUnsorted serving as
                                      scratch for per-entry sums), and R == 0 gives all-zero gradients. All zero (no receipt):
                                      the reference's contract only — the sorted lists must be in point_list; the call then
                                      reads point_list[0] back (one stream sync) and refuses GSR_LISTS_SKIPPED_STAMP with
                                      GSR_ERR_INVALID_ARG. A receipt that does not fit the other arguments (sizes, rows,
                                      point_list): GSR_ERR_INVALID_ARG. */
    /* ---- depth channel (appended; see gsr_forward_args.out_depth and GSR_FLAG_DEPTH_INVERSE, which flags must repeat) ----
     * L gains sum_p dL_dout_depth[p] out_depth[p]. d_i is recomputed from means3D and view_matrix (both then required), so
     * the receipt of any forward call serves, whether or not it wrote out_depth. Every other output receives the depth
     * channel's share: the colour backward plus that of colours (d_i, 0, 0) against (dL_dout_depth, 0, 0), no background;
     * dL_dmeans3D also gets dL_ddepths[i] (V[2], V[6], V[10]), times -1 / z_i^2 with GSR_FLAG_DEPTH_INVERSE. */
    const float* dL_dout_depth;    /* device f32[W H], or NULL: no depth channel */
    float* dL_ddepths;             /* f32[N]: dL/dd_i = sum alpha T dL_dout_depth. Required with dL_dout_depth unless sums_f64 is
                                      given (then optional) */
    double* depth_sums_f64;        /* f64[N] scratch, ZERO on entry, left zero on return: the dL_ddepths sums in double. Required
                                      when sums_f64 is given and dL_dout_depth is not NULL (a separate array: the f64[12 N]
                                      layout of sums_f64 stays as it is) */
} gsr_backward_args;
int gsr_backward(gsr_backward_args* args);

/* ---- camera gradients: the backward pass on to the camera (after gsr_backward, on the same stream) ----
 * The derivatives of the same scalar L that gsr_backward differentiates (the colour term sum dL_dout_color * out_color,
 * plus sum dL_dout_depth * out_depth when that call had a depth gradient, plus sum dL_dout_alpha * (1 - final_t) when it was
 * gsr_backward_alpha of gsrast_amd_opacity.h: that term is in the per-Gaussian gradients, nothing more is needed here) w.r.t. the 16 + 16 + 3 floats exactly as passed
 * to gsr_forward: view_matrix and proj_matrix column-major (the view's row 2 negated, as the reference's caller builds it),
 * cam_pos. Entry (row r, column c) of a matrix is element 4 c + r. Only visible Gaussians (radii[i] > 0) contribute, and the
 * camera reaches L only through each one's
 *   pixel centre means2D_i  proj rows 0, 1, 3 (h = proj (x, y, z, mean.w); the upstream profile: (x, y, z, 1))
 *   cov2D_i = J(t) W Sigma W^T J(t)^T + 0.3 I, t = V (x, y, z, 1), W the upper 3 x 3 of V: view rows 0-2. The clamps of
 *                           t.x / t.z and t.y / t.z to +-1.3 tan_fov are decided in float32 as gsr_forward decides them; a
 *                           clamped ratio passes its gradient to t.z only
 *   depth d_i = t.z (1 / t.z with GSR_FLAG_DEPTH_INVERSE)  view row 2, only when dL_ddepths is given
 *   upstream colour through dir = (mean - cam_pos) / |mean - cam_pos|  cam_pos, only with shs (a channel clamped at zero
 *                           passes nothing; the reference's colour and colors_precomp do not depend on the camera)
 * Entries nothing depends on are written as exact zeros: view row 3, proj row 2 (NDC depth only sorts and culls), cam_pos
 * under the reference's semantics or without shs. Culling, radii, rectangles, tile membership, depth order and the alpha
 * clamps are decisions with zero derivative; tan_fovx / tan_fovy are not differentiated.
 * The call reads gsr_backward's per-Gaussian outputs: dL_dcov2D is required (the covariance gradient is not derived from
 * dL_dconic_opacity). Per-Gaussian terms are formed in double and summed in double per thread, wave and block in an order
 * fixed by num_gaussians alone (no atomics), then rounded to float once: two calls on the same arrays give the same bits on
 * any device. Nothing visible: all outputs are zeros. A tile-row band (gsr_backward with tile_row_begin / _end) gives that
 * band's share: the result is linear in the per-Gaussian gradients, so the bands' results add up to the whole frame's.
 * Refused with GSR_ERR_INVALID_ARG before any HIP call: a wrong struct_size, a non-positive size, a missing required
 * input or scratch, no output at all, shs without dL_dcolors / clamped / cam_pos. */
size_t gsr_camera_backward_scratch_bytes(int32_t num_gaussians);   /* device scratch the call needs: a function of N only */
typedef struct gsr_camera_backward_args {
    uint32_t struct_size;          /* = sizeof(gsr_camera_backward_args) */
    uint32_t flags;                /* GSR_FLAG_SEMANTICS_INRIA, GSR_FLAG_DEPTH_INVERSE (as the forward / backward calls),
                                      GSR_FLAG_PROFILE (stage_ms) */
    int32_t num_gaussians, width, height;
    /* inputs of the forward call (device) */
    const float* means3D;          /* vec4[N] */
    const float* view_matrix;      /* 16 floats */
    const float* proj_matrix;      /* 16 floats */
    const float* cam_pos;          /* vec3; needed with shs only */
    float tan_fovx, tan_fovy;
    /* state of the forward call */
    const float* cov3D;            /* f32[6 N]: geometry cov3D, or the cov3D_precomp given */
    const int32_t* radii;          /* internal_radii or the radii buffer given */
    const float* shs;              /* upstream profile with SH colour: f32[48 N], [16][3] per Gaussian; NULL: no colour term */
    const uint8_t* clamped;        /* geometry chunk: bool[3 N] (with shs) */
    int32_t sh_dims;               /* SH degree the forward call evaluated (0..3) */
    /* per-Gaussian outputs of gsr_backward */
    const float* dL_dmean2D;       /* vec2[N], required */
    const float* dL_dcov2D;        /* vec4[N] (m00, m01, m11, 0), required */
    const float* dL_ddepths;       /* f32[N], or NULL: no depth channel */
    const float* dL_dcolors;       /* vec3[N], required with shs */
    /* outputs (device, each optional, at least one): float32, always written in full */
    float* dL_dview_matrix;        /* 16 floats, layout of view_matrix */
    float* dL_dproj_matrix;        /* 16 floats, layout of proj_matrix */
    float* dL_dcam_pos;            /* 3 floats */
    void* scratch;                 /* device, gsr_camera_backward_scratch_bytes(num_gaussians) bytes, 8-byte aligned */
    void* stream;
    float stage_ms;                /* with GSR_FLAG_PROFILE: the camera pass's device time */
} gsr_camera_backward_args;
int gsr_camera_backward(gsr_camera_backward_args* args);

/* ---- point-splat path (gscuda::forwardPoints, GSCuda.cuh:19-42 / GSCuda.cu:26-155; the reference never
 * calls it) ---- Same argument struct as gsr_forward; read: num_gaussians, width, height, background,
 * means3D (a stride of THREE floats here, GSCuda.cu:65), shs, proj_matrix, out_color, geometry_alloc (asked for
 * 32 bytes, as the reference does for its empty pc::GeometryState), image_alloc, stream. Every centre inside
 * NDC [-1,1]^2 x [0,1] lands on one pixel; the nearest wins (the lowest index among equal depths — the
 * reference's unordered colour write makes its own result timing dependent). */
typedef struct gsr_points_image_state {   /* pc::ImageState (AuxBuffer.cuh:26-33), `size` = width*height */
    float*    depth;           /* f32[size] NDC z of the winner, 1.0 where none   */
    float*    out_color;       /* f32[3 size] planar temporary image              */
    float*    default_depth;   /* f32[1] = 1.0                                    */
    uint64_t* winner;          /* u64[size] (depth bits << 32 | index), this library's depth-test table */
} gsr_points_image_state;
char* gsr_points_image_from_chunk(char* chunk, int size, gsr_points_image_state* out);
size_t gsr_required_points_image(int size);
int gsr_forward_points(gsr_forward_args* args);

/* ---- multi-GPU: the row-band exchange of a frame sharded by screen tile rows (the reference is single-GPU:
 * nothing of this replaces a reference interface) ----
 * One process per GPU. Every rank holds the whole planar frame (3 x height x width floats, device memory) and has rendered
 * tile rows [bounds[rank], bounds[rank + 1]) of it (gsr_forward_args.tile_row_begin / _end); one call moves every band
 * into place in the peers' frames: ncclGroupStart, one ncclSend / ncclRecv per (peer, colour plane) of exact size, ncclGroupEnd
 * — no staging, no padding. RCCL is loaded at run time from `rccl_path` (NULL: librccl.so.1; a process that uses PyTorch
 * passes the copy torch has mapped), so the library does not depend on it.
 *   gsr_exchange_unique_id : one rank creates the 128-byte id (ncclGetUniqueId) and hands it to the others by any means
 *   gsr_exchange_create    : every rank, with ITS device current (ncclCommInitRank: collective, blocks until all have called)
 *   gsr_exchange_bands     : bounds = world + 1 tile-row boundaries (0 ... ceil(height / 16), non-decreasing; empty bands
 *                            allowed); root < 0: every rank receives every band (all-gather); root = r: only rank r
 *                            receives (gather: 1 / world of the traffic when one rank displays). Asynchronous on `stream`.
 *   gsr_exchange_plan      : host only, no communicator: the transfers a rank would issue, in order (tests, tools)
 *   gsr_exchange_loopback  : `planes` pieces of `count` floats sent from src to dst on the OWN rank through the same
 *                            group of ncclSend / ncclRecv (a diagnostic: what a single GPU can run of the transfers)
 * All return GSR_OK or an error code (gsr_exchange_plan: the count, or the negated code); gsr_exchange_last_error() has
 * the RCCL / loader message behind a GSR_ERR_HIP. */
typedef struct gsr_exchange gsr_exchange;
int gsr_exchange_unique_id(const char* rccl_path, char* id128);
int gsr_exchange_create(const char* rccl_path, const char* id128, int rank, int world, gsr_exchange** out);
int gsr_exchange_bands(gsr_exchange* x, float* frame, int width, int height, const int32_t* bounds, int root, void* stream);
int gsr_exchange_plan(int rank, int world, int width, int height, const int32_t* bounds, int root, int max_ops,
                      int32_t* is_send, int32_t* peer, uint64_t* offset, uint64_t* count);
int gsr_exchange_loopback(gsr_exchange* x, const float* src, float* dst, uint64_t count, int planes, void* stream);
int gsr_exchange_destroy(gsr_exchange* x);
const char* gsr_exchange_last_error(void);

/* ---- scene loading (next row after the hot path) ---- */
/* Header of a 3DGS .ply as the reference reads it (apps/gsrast/SplatData.cpp:114-145): vertex
 * count = third token of the third line; data starts after the "end_header" line. Host only.
 * Returns GSR_ERR_INVALID_ARG if the file cannot be opened or has no end_header. */
int gsr_ply_parse_header(const char* path, int* num_splats, long long* data_offset);
/* Activations of SplatData::loadFromPly (SplatData.cpp:28-66) on the GPU: raw_device holds n
 * records of 62 floats (SplatData.hpp:17-25) in HBM; outputs are the SoA gsr_forward takes
 * (means3D/scales/rotations vec4[n], opacities f32[n], shs f32[48 n]). Asynchronous on stream. */
int gsr_ply_activate(const float* raw_device, int n, float* means3D, float* scales, float* rotations,
                     float* opacities, float* shs, void* stream);
/* The 48 SH floats of a record are f_dc_0..2 followed by f_rest_0..44, and a 3DGS .ply stores f_rest CHANNEL-major
 * (R1..R15, G1..G15, B1..B15). The reference copies them as they lie (SplatData.cpp:146) and reads only the DC
 * triple (GSCuda.cu:362-366): GSR_SH_LAYOUT_FILE, what gsr_ply_activate does. GSR_FLAG_SEMANTICS_INRIA reads shs as
 * [N][16][3], coefficient-major (upstream's layout, SURVEY.md divergence D2): a scene that is to be drawn with that
 * flag and sh_dims >= 1 must be loaded with GSR_SH_LAYOUT_COEFFICIENT_MAJOR, which transposes f_rest on the way. */
enum { GSR_SH_LAYOUT_FILE = 0, GSR_SH_LAYOUT_COEFFICIENT_MAJOR = 1 };
int gsr_ply_activate_layout(const float* raw_device, int n, float* means3D, float* scales, float* rotations,
                            float* opacities, float* shs, int sh_layout, void* stream);

/* ---- a trainer's raw parameters (csrc/activations.hip) ---- */
/* The same activations from separate arrays instead of the file record: what a trainer optimises (positions f32[3 n],
 * opacity logits f32[n], log-scales f32[3 n], unnormalised quaternions f32[4 n], real part first) -> the arrays
 * gsr_forward takes: means3D (x, y, z, 1), scales (exp s, exp s, exp s, e), rotations r / |r| (all vec4[n]) and
 * opacities 1 / (1 + exp(-x)) (f32[n]). Float32 arithmetic in the operation order of gsr_ply_activate: bit-equal results
 * for equal raw values. SH coefficients need no activation. Device pointers, every one required; the arrays of three and
 * four floats per Gaussian 16-byte aligned (GSR_ERR_INVALID_ARG otherwise, before any HIP call); n <= 0 is GSR_OK and
 * touches nothing. Asynchronous on stream. */
int gsr_activate_params(int n, const float* raw_means, const float* raw_opacity, const float* raw_scales,
                        const float* raw_rotations, float* means3D, float* scales, float* rotations, float* opacities,
                        void* stream);
/* The gradients gsr_backward returns (dL_dmeans3D, dL_dscales, dL_drotations vec4[n]; the opacity's is
 * dL_dconic_opacity[i].w) through those activations, to the raw arrays:
 *   dL_draw_means[3 i + k]  = dL_dmeans3D[i][k]                                   k < 3
 *   dL_draw_scales[3 i + k] = dL_dscales[i][k] * exp(s[k])                        k < 3
 *   dL_draw_opacity[i]      = dL_dconic_opacity[i].w * sigmoid(x) * sigmoid(-x)
 *   dL_draw_rotations[i]    = (g - q (q . g)) / |r|,  q = r / |r|,  g = dL_drotations[i]
 * each formed in double from the float32 inputs and rounded to float once. Every output is optional: a NULL output is not
 * computed or written, and the inputs only it reads may then be NULL too; an output that is given without its inputs, or a
 * vector array that is not 16-byte aligned, is GSR_ERR_INVALID_ARG before any HIP call. radii (i32[n], the forward call's
 * geomState.internal_radii, or NULL): a Gaussian with radii[i] <= 0 gets exact zeros in every output and nothing else of
 * it is loaded. A zero quaternion has no gradient (NaN). n <= 0 is GSR_OK. Asynchronous on stream. */
int gsr_activate_params_backward(int n, const float* raw_opacity, const float* raw_scales, const float* raw_rotations,
                                 const int32_t* radii, const float* dL_dmeans3D, const float* dL_dscales,
                                 const float* dL_drotations, const float* dL_dconic_opacity, float* dL_draw_means,
                                 float* dL_draw_opacity, float* dL_draw_scales, float* dL_draw_rotations, void* stream);

/* ---- the optimiser step over those raw parameters (csrc/adam.hip) ----
 * One in-place Adam update of up to GSR_ADAM_MAX_TENSORS arrays that share a row count: array k has row_floats floats per
 * row, a row being one Gaussian (3 / 1 / 3 / 4 / 48 for the five raw arrays). Per element, in float32 without contraction
 * and in exactly this order, which is the definition of the result:
 *   m' = m + b1c * (g - m)
 *   v' = b2 * v + b2c * (g * g)
 *   den = sqrtf(v') / rs + eps
 *   p' = p - step_size * (m' / den)
 * sqrtf and / are correctly rounded, so p', m', v' are a function of the inputs alone (not of the launch shape, the
 * other arrays of the call, or `visible`); float32 denormals are not pinned. The six scalars are the caller's, per array,
 * so that parameter groups with different rates, betas and eps share a call. For Adam at step t >= 1 (computed in double,
 * each rounded to float once):
 *   step_size = lr / (1 - beta1^t)   rs = sqrt(1 - beta2^t)   b1c = 1 - beta1   b2 = beta2   b2c = 1 - beta2   eps
 * visible (i32[num_rows], device, or NULL): row i is updated iff visible[i] > 0 — a frame's radii can be passed as they
 * are. A row that is not keeps the bits of param, exp_avg and exp_avg_sq, and its grad is never used (it may be NaN): of
 * such a row the kernel reads the visibility word only, except where a 16-byte vector of a three-float array also holds
 * floats of a visible neighbour; that vector is read and written back whole, the row's floats unchanged. NULL: every row.
 * Refused with GSR_ERR_INVALID_ARG before any HIP call: a wrong struct_size, num_rows < 0, num_tensors outside
 * 1..GSR_ADAM_MAX_TENSORS, and for any array a NULL among its four pointers, one that is not 16-byte aligned, or
 * row_floats <= 0. More rows than one launch covers: GSR_ERR_TOO_LARGE. num_rows == 0 is GSR_OK and touches nothing.
 * One launch, asynchronous on stream; the arrays must not overlap. */
#define GSR_ADAM_MAX_TENSORS 8
typedef struct gsr_adam_tensor {
    float* param;                  /* f32[num_rows * row_floats], updated in place */
    const float* grad;             /* f32[num_rows * row_floats] */
    float* exp_avg;                /* m, updated in place */
    float* exp_avg_sq;             /* v, updated in place */
    int32_t row_floats;
    float step_size, rs, b1c, b2, b2c, eps;
} gsr_adam_tensor;
typedef struct gsr_adam_args {
    uint32_t struct_size;          /* = sizeof(gsr_adam_args) */
    int32_t num_tensors;
    int64_t num_rows;
    const int32_t* visible;
    void* stream;
    gsr_adam_tensor tensors[GSR_ADAM_MAX_TENSORS];
} gsr_adam_args;
int gsr_adam_step(const gsr_adam_args* args);

/* ---- the photometric training loss and its gradient (csrc/photo_loss.hip) ----
 * loss = (1 - lambda) * L1 + lambda * (1 - SSIM) of image against target, both f32[channels][height][width], and dloss /
 * dimage. SSIM is the mean of the per-pixel map m below over an 11 x 11 Gaussian window, sigma 1.5, zero padded. All
 * per-pixel arithmetic is float32 without contraction, / correctly rounded, in exactly this order, which is the definition
 * of the result (it does not depend on the tile shape or the launch):
 *   window   g[k] = exp(-(k - 5)^2 / 4.5) / sum, k = 0..10: computed and normalised in double, rounded to float once
 *            (GSR_PHOTO_LOSS_WINDOW below spells the eleven floats out).
 *   conv(a)  separable: h(r,c) = sum_k g[k] * a(r, c + k - 5), then conv(a)(r,c) = sum_k g[k] * h(r + k - 5, c); each sum is
 *            acc = acc + g[k] * v from acc = 0.0f with k ascending; a tap outside the image contributes g[k] * 0.
 *   per pixel and channel, x = image, y = target, C1 = 0.01^2, C2 = 0.03^2 (each rounded to float once):
 *     mu1 = conv(x)   mu2 = conv(y)
 *     s11 = conv(x*x) - mu1*mu1   s22 = conv(y*y) - mu2*mu2   s12 = conv(x*y) - mu1*mu2
 *     a1 = 2*(mu1*mu2) + C1   a2 = 2*s12 + C2   b1 = (mu1*mu1 + mu2*mu2) + C1   b2 = (s11 + s22) + C2
 *     m     = (a1*a2) / (b1*b2)
 *     d_s12 = (2*a1) / (b1*b2)
 *     d_s11 = -(m / b2)
 *     d_mu1 = (2*mu2*a2) / (b1*b2) - (2*mu1*m) / b1
 *     t_mu  = (d_mu1 - 2*mu1*d_s11) - mu2*d_s12
 *   loss terms: the float values |x - y| and m are summed in DOUBLE, per workgroup and then over the workgroups' partial
 *     sums in a fixed order (no floating-point atomic takes part: two runs give the same bits). In double, with n = channels *
 *     height * width:  l1 = l1_sum / n,  ssim = ssim_sum / n,  loss = (1 - lambda) * l1 + lambda * (1 - ssim);  each of
 *     the three is rounded to float once: out[3] = (loss, l1, ssim), on the device.
 *   gradient: cs = -lambda / n and cl = (1 - lambda) / n (in double on the host, each rounded to float once), up =
 *     *dL_dloss, read on the device:
 *     S   = (conv(t_mu) + 2*x*conv(d_s11)) + y*conv(d_s12)
 *     sgn = (x - y > 0) - (x - y < 0)
 *     dL_dimage = up * (cs*S + cl*sgn)
 * gsr_photo_loss_forward writes out and, with want_backward != 0, the three maps t_mu, d_s11, d_s12 into scratch;
 * gsr_photo_loss_backward convolves them and writes dL_dimage. The caller owns scratch
 * (gsr_photo_loss_scratch_bytes(channels, width, height) bytes: the workgroups' partial sums and the three maps) and keeps
 * it, image and target unchanged between the two calls; the library keeps nothing. Both calls enqueue on stream and do not
 * synchronise. Refused with GSR_ERR_INVALID_ARG before anything is launched: a wrong struct_size; channels, width or height
 * below 1; lambda_dssim outside [0, 1] (or NaN); a NULL among image, target, scratch and (forward) out or (backward) dL_dloss,
 * dL_dimage; image, target, scratch or dL_dimage not 16-byte aligned, out or dL_dloss not 4-byte aligned. More than 2^31 - 1
 * floats per image, 65535 channels or 65535 * 16 rows: GSR_ERR_TOO_LARGE. Inputs are taken as finite. */
#define GSR_PHOTO_LOSS_WINDOW { 0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f, \
                                0.213005543f, 0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f }
typedef struct gsr_photo_loss_args {
    uint32_t struct_size;          /* = sizeof(gsr_photo_loss_args) */
    int32_t channels, width, height;
    double lambda_dssim;           /* a double, so that cs and cl are those of the caller's lambda and not of its float */
    const float* image;            /* f32[channels][height][width] */
    const float* target;
    void* scratch;                 /* gsr_photo_loss_scratch_bytes(channels, width, height) bytes */
    float* out;                    /* forward: f32[3] = (loss, l1, ssim) */
    const float* dL_dloss;         /* backward: one float, the upstream gradient */
    float* dL_dimage;              /* backward: f32[channels][height][width] */
    int32_t want_backward;         /* forward: also write what the backward reads into scratch */
    void* stream;
} gsr_photo_loss_args;
size_t gsr_photo_loss_scratch_bytes(int channels, int width, int height);     /* 0 for sizes the calls refuse */
int gsr_photo_loss_forward(const gsr_photo_loss_args* args);
int gsr_photo_loss_backward(const gsr_photo_loss_args* args);

/* ---- adaptive density control over the raw parameters (csrc/densify.hip) ----
 * Three calls: the statistics of a frame, the decision which Gaussians are cloned, split and pruned, and the move of the
 * five raw arrays and their Adam moments into arrays of the new row count. Each enqueues on stream and does not
 * synchronise; the caller reads `counts` back between the second and the third (it allocates the new arrays).
 *
 * gsr_densify_accumulate: one launch, no atomics. For a row with radii[i] > 0, in float32 without contraction, in this order:
 *   gx = dL_dmean2D[i].x * half_width     gy = dL_dmean2D[i].y * half_height      (upstream's NDC convention: 0.5 W, 0.5 H;
 *                                                                                  gsr_backward's dL_dmean2D carries no NDC factor)
 *   grad_accum[i] = grad_accum[i] + sqrtf(gx*gx + gy*gy)
 *   denom[i]      = denom[i] + 1
 *   max_radii[i]  = max(max_radii[i], radii[i])
 * Of a row with radii[i] <= 0 the kernel reads the radii word only: its gradient may be NaN, its three statistics keep
 * their bits. Refused with GSR_ERR_INVALID_ARG before any HIP call: n < 0, a NULL pointer, dL_dmean2D not 8-byte aligned or
 * another array not 4-byte aligned. More rows than one launch covers: GSR_ERR_TOO_LARGE. n == 0 is GSR_OK. */
int gsr_densify_accumulate(int64_t n, const float* dL_dmean2D, const int32_t* radii, float half_width, float half_height,
                           float* grad_accum, int32_t* denom, int32_t* max_radii, void* stream);
/* gsr_densify_plan: the decision, taken in the raw domain (no exponential enters it; the caller forms the thresholds in
 * double and rounds each to float once: log_dense = log(percent_dense * extent), logit_min_opacity = logit(min_opacity),
 * log_world = log(0.1 * extent), log_shrink = log(0.8 * 2)). Per source row i, in float32, which is the definition of the
 * result:
 *   g      = denom[i] > 0 ? grad_accum[i] / (float)denom[i] : 0     (/ correctly rounded; a NaN g counts as 0)
 *   m      = the largest of log_scale[i][0..2]                      (m = s0; if (s1 > m) m = s1; if (s2 > m) m = s2)
 *   hot    = g >= max_grad            big = m > log_dense
 *   clone  = hot && !big              split = hot && big
 *   doomed(M) = opacity_logit[i] < logit_min_opacity || (max_screen > 0 && (max_radii[i] > max_screen || M > log_world))
 *   doomed = doomed(m)                child_doomed = doomed(m - log_shrink)      (the subtraction in float32)
 * Row i yields one KEPT row if !split && !doomed, one CLONE row if clone && !doomed, two CHILD rows if split &&
 * !child_doomed. A clone and a child are tested with their PARENT's max_radii: they inherit it for this test (early
 * upstream versions zeroed max_radii2D when they densified, and their screen-size pruning never fired because of it).
 * max_screen <= 0 switches the two size tests off. Output rows in upstream's concatenation order: the kept rows in source
 * order, then the clones in source order, then child 0 of every surviving split parent in source order, then child 1 of
 * each. src_of[r] (i32, capacity 3 n) = the source row of output row r, r < K + C + 2 S; counts (i32[4], device) =
 * (K, C, S, K + C + 2 S) with K kept rows, C clones and S surviving split parents. temp: gsr_densify_plan_temp_bytes(n)
 * bytes of device memory, 16-byte aligned (three flag arrays, scanned in place, and the scan's own scratch).
 * Refused with GSR_ERR_INVALID_ARG before any HIP call: n < 0, a NULL pointer, temp not 16-byte aligned or another array
 * not 4-byte aligned. 3 n > 2^31 - 1 (the scan's sums and the counts are 32-bit): GSR_ERR_TOO_LARGE, and
 * gsr_densify_plan_temp_bytes is then 0. n == 0 writes counts = 0. */
size_t gsr_densify_plan_temp_bytes(int64_t n);
int gsr_densify_plan(int64_t n, const float* opacity_logit, const float* log_scale, const float* grad_accum,
                     const int32_t* denom, const int32_t* max_radii, float max_grad, float log_dense,
                     float logit_min_opacity, float log_world, float log_shrink, int32_t max_screen, void* temp,
                     int32_t* src_of, int32_t* counts, void* stream);
/* gsr_densify_apply: one launch over the K + C + 2 S output rows of all five arrays; output row r gathers from source row
 * src_of[r], and a source row that no output row names is never read. Rows [0, K) are kept rows, [K, K + C) clones,
 * [K + C, K + C + S) child 0 and [K + C + S, K + C + 2 S) child 1 of the split parent with rank j = r - (K + C) resp.
 * r - (K + C + S).
 *   kept   the parameter and both moments are copied bit for bit
 *   clone  the parameter is copied bit for bit; both moments are +0
 *   child  both moments are +0; opacity_logit, rotation and shs are copied bit for bit;
 *          log_scale'[c] = log_scale[c] - log_shrink, and, in float32 without contraction, with the parent's values:
 *            (s0, s1, s2) = exp(log_scale)  and  (r, x, y, z) = rotation / |rotation|  exactly as gsr_activate_params forms
 *            them (the Gaussian the noise is scaled by is the one that is rendered)
 *            d[c] = s[c] * noise[j][k][c]                                          k = 0, 1: the child
 *            R00 = 1 - 2*(y*y + z*z)   R01 = 2*(x*y - r*z)       R02 = 2*(x*z + r*y)
 *            R10 = 2*(x*y + r*z)       R11 = 1 - 2*(x*x + z*z)   R12 = 2*(y*z - r*x)
 *            R20 = 2*(x*z - r*y)       R21 = 2*(y*z + r*x)       R22 = 1 - 2*(x*x + y*y)        (upstream's build_rotation)
 *            xyz'[a] = xyz[a] + ((Ra0*d[0] + Ra1*d[1]) + Ra2*d[2])
 * The four moment pointers of an array are all NULL (no optimiser state yet: none is read or written) or all set. Source
 * and destination arrays must not overlap. Refused with GSR_ERR_INVALID_ARG before any HIP call: a wrong struct_size; n_src
 * or a count below 0; counts[3] != K + C + 2 S; K + S or C + S above n_src; a NULL src_of, src or dst; a NULL noise with
 * S > 0; moment pointers of an array partly set; a parameter or moment array not 16-byte aligned, src_of or noise not
 * 4-byte aligned. More rows than one launch covers: GSR_ERR_TOO_LARGE. counts[3] == 0 is GSR_OK and touches nothing. */
typedef struct gsr_densify_array {
    const float* src;              /* f32[n_src * w], w = 3 / 1 / 3 / 4 / 48 for xyz / opacity_logit / log_scale / rotation / shs */
    const float* src_exp_avg;
    const float* src_exp_avg_sq;
    float* dst;                    /* f32[counts[3] * w] */
    float* dst_exp_avg;
    float* dst_exp_avg_sq;
} gsr_densify_array;
typedef struct gsr_densify_apply_args {
    uint32_t struct_size;          /* = sizeof(gsr_densify_apply_args) */
    float log_shrink;
    int64_t n_src;
    int32_t counts[4];             /* (K, C, S, K + C + 2 S), as gsr_densify_plan wrote them */
    const int32_t* src_of;         /* i32[counts[3]] */
    const float* noise;            /* f32[S][2][3], standard normal, the caller's */
    void* stream;
    gsr_densify_array xyz, opacity_logit, log_scale, rotation, shs;
} gsr_densify_apply_args;
int gsr_densify_apply(const gsr_densify_apply_args* args);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_AMD_H */
