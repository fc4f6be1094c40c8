// Shared declarations of the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gsrast_amd.h"
#include "frame_policy.hpp"      // (kTile, FrameDims, DeviceShape, the launch heuristics' switch points)
#include "shared_words.hpp"      // (the pinned host block, sort_info)

namespace gsr {

constexpr int kWave = 64;          // gfx950 wavefront

// Records the failing HIP call for gsr_last_hip_error(), and forgets it: entry_point() starts every entry point with that
// (the one other caller, history_of_call, swallows an expected allocation failure).
void set_hip_error(hipError_t e, const char* what);
void clear_hip_error();
// Sets the calling thread's sticky error (gsr_last_error) and returns `code`.
int record_error(int code);
// The error contract of include/gsrast_amd.h, for every extern "C" function that returns a GSR_* code: the previous HIP text
// is forgotten, `impl` runs and returns plain codes (GSR_HIP_TRY, GSR_TRY and GSR_LAUNCH_CHECK included), its code is recorded.
template <typename Impl, typename... Args>
inline int entry_point(Impl impl, Args... args) { clear_hip_error(); return record_error(impl(args...)); }
// Refused before a launch: a pointer off a `to`-byte boundary (a power of two; null passes), more workgroups than a grid holds.
inline bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }
inline bool exceeds_grid(long long blocks) { return blocks > 0x7FFFFFFFll; }
__host__ __device__ inline bool positive_finite(float v) { return v > 0.0f && v <= 3.402823466e+38f; }      // (false for NaN and Inf)

// A vec4 row that is read (written) once: a streaming load (store), so that it does not push out of the caches what the next
// kernels read at once (preprocess.hip: 0.146 -> 0.129 ms on the bench frame).
typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float4* q) {
    const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(q));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float4* q, float x, float y, float z, float w) {
    __builtin_nontemporal_store((nt_f4){x, y, z, w}, reinterpret_cast<nt_f4*>(q));
}

#define GSR_HIP_TRY(expr)                                   \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) {                             \
            ::gsr::set_hip_error(e_, #expr);                \
            return GSR_ERR_HIP;                             \
        }                                                   \
    } while (0)

// A step of a launch sequence: a GSR_* code other than GSR_OK ends the sequence.
#define GSR_TRY(call)                                       \
    do {                                                    \
        const int rc_ = (call);                             \
        if (rc_ != GSR_OK) return rc_;                      \
    } while (0)

#define GSR_LAUNCH_CHECK(name)                              \
    do {                                                    \
        hipError_t e_ = hipGetLastError();                  \
        if (e_ != hipSuccess) {                             \
            ::gsr::set_hip_error(e_, name);                 \
            return GSR_ERR_HIP;                             \
        }                                                   \
    } while (0)

// The N events of one profiled call: created on the device that is current for THIS call, destroyed when it returns.
template <int N>
struct CallEvents {
    hipEvent_t ev[N] = {};
    int create() {
        for (auto& e : ev) GSR_HIP_TRY(hipEventCreate(&e));
        return GSR_OK;
    }
    ~CallEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// What the scan wants to know of a preprocess wave's 64 Gaussians, left as ONE 16-byte record per wave so that its first
// launch reads 0.25 bytes per Gaussian instead of re-reading tilesTouched (50 M Gaussians: 80 -> 13 us): {sum of tilesTouched,
// Gaussians with a tile, the instances of those of big_from tiles and more, those with a tile whose depth key has another
// top byte than the main one}. Lanes past the last Gaussian have left the kernel: the last wave sums by readlane.
__device__ __forceinline__ void store_wave_sums(uint4* __restrict__ wave_sums, int idx, uint32_t tiles, bool other_top, uint32_t big_from) {
    const unsigned long long active = __ballot(true);
    const uint32_t z = (uint32_t)__popcll(__ballot(tiles != 0u)), o = (uint32_t)__popcll(__ballot(tiles != 0u && other_top));
    uint32_t s = tiles, b = tiles >= big_from ? tiles : 0u;
    if (active == ~0ull) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off, 64); b += __shfl_xor(b, off, 64); }
    } else {
        uint32_t ss = 0, bb = 0;
        for (unsigned long long m = active; m != 0ull; m &= m - 1ull) {
            const int l = __ffsll((long long)m) - 1;
            ss += (uint32_t)__builtin_amdgcn_readlane((int)s, l);
            bb += (uint32_t)__builtin_amdgcn_readlane((int)b, l);
        }
        s = ss; b = bb;
    }
    if ((threadIdx.x & 63) == 0) wave_sums[idx >> 6] = make_uint4(s, z, b, o);
}

// Where the depth channel of a blend comes from and goes to (gsr_forward_args.out_depth; out == null: no depth channel).
struct DepthTarget {
    float* out = nullptr;
    const float* means3D = nullptr;      // vec4[N]
    const float* view = nullptr;         // the view matrix (row 2 is read)
    uint32_t inverse = 0;                // GSR_FLAG_DEPTH_INVERSE
};

// ---- stage launchers (each asynchronous on `stream`) ----
int launch_preprocess(const gsr_forward_args& a, const gsr_geometry_state& g, int32_t* radii,
                      uint32_t* depth_keys, uint32_t* rect_packed, const FrameDims& d, hipStream_t stream,
                      uint4* wave_sums = nullptr, bool colors_elsewhere = false, uint32_t big_from = 0xFFFFFFFFu);   // wave_sums: store_wave_sums
// geomState.rgb for the Gaussians with a tile (zeros for the others), as preprocess_kernel writes it — for a second stream
int launch_colors_visible(int n, const uint32_t* tiles_touched, const float* shs, float* rgb, hipStream_t stream);

int launch_colors_from_dc(int n, const float* shs, float* colors, hipStream_t stream);

int launch_preprocess_inria(const gsr_forward_args& a, const gsr_geometry_state& g, int32_t* radii, uint32_t* depth_keys,
                            uint32_t* rect_packed, const FrameDims& d, hipStream_t stream, uint4* wave_sums = nullptr,
                            uint32_t big_from = 0xFFFFFFFFu);

// What the depth order takes from the scan of tilesTouched on the way (gsr_forward; a plain scan leaves all of it null).
struct ScanByproducts {
    uint32_t* info = nullptr;            // sort_info (shared_words.hpp): gets kInfoTotal, the 64-bit total, and — with `nonzero` — kInfoVisible
    uint32_t* host = nullptr;            // the pinned host block (needs info): kHostVisible = the non-zero total, kHostTotal = the 64-bit
                                         // total, written by the scan itself
    uint32_t* nonzero = nullptr;         // u32 per 4096 elements: the exclusive prefix of the tiles' counts of non-zero elements (the
                                         // depth order's compaction offsets, radix_sort.hip); their total: kInfoVisible
    void* clear = nullptr;               // device memory the first launch also zeroes (16-byte granules)
    size_t clear_bytes = 0;
    // wave_sums / main_count (both or neither; need nonzero and big): the preprocess's per-wave records (store_wave_sums) — the
    // first launch then reads those instead of `in` — and the depth order's side list (kInfoSide, kHostSideWay, kHostSideCounted), see scan.hip
    const uint4* wave_sums = nullptr;
    uint32_t* main_count = nullptr;
    uint32_t side_max = 0;
    uint32_t* big = nullptr;             // u32 per 4096 elements (needs host): kHostBigInstances = the 64-bit sum of the elements >= big_from
    uint32_t big_from = 0;
};
int launch_inclusive_scan(const uint32_t* in, uint32_t* out, size_t n, char* temp, hipStream_t stream,
                          const ScanByproducts& by = ScanByproducts{});
size_t scan_temp_bytes(size_t n);

int launch_gather_counts(int n, const uint32_t* sorted_depth, const uint32_t* sorted_idx, const uint32_t* tiles_touched,
                         uint32_t* counts, hipStream_t stream);
int launch_duplicate(int n, const uint32_t* sorted_depth, const uint32_t* sorted_idx, const uint32_t* emit_end,
                     const gsr_geometry_state& g, const int32_t* radii, const int32_t* rects, const FrameDims& d,
                     uint64_t* keys, uint32_t* values, uint32_t* hist_x, uint32_t* hist_y, hipStream_t stream);

int launch_sort_pairs(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* values_in,
                      uint32_t* values_out, size_t n, int begin_bit, int end_bit, char* temp, hipStream_t stream, uint32_t* error_word = nullptr,
                      uint32_t error_value = 1u);
size_t sort_temp_bytes(size_t n);
struct SweepScratch;
// The depth order's side list (radix_sort.hip, depth_side_kernel): the visible keys whose top byte is not main_top, when
// the scan found few of them. words: sort_info + kInfoSide, indexed by SideWord (shared_words.hpp). main_partial: the compaction's offsets counted for the main keys only.
constexpr uint32_t kDepthSideMax = 1024;
constexpr uint32_t kDepthMainTop = 0x3Fu;            // float bits of [0.5, 1)
struct DepthSide {
    uint32_t* words = nullptr;
    const uint32_t* main_partial = nullptr;
    uint32_t *keys = nullptr, *vals = nullptr, *rects = nullptr;
    uint32_t capacity = 0, main_top = kDepthMainTop;
};
int launch_depth_side(const DepthSide& side, uint32_t m, uint32_t m_lo, uint32_t main_count, uint32_t* out_k, uint32_t* out_v,
                      uint32_t* out_r, hipStream_t stream);
// Depth order (radix_sort.hip). sc4: one scratch area per pass, already zeroed by the caller (look-back words,
// tickets, error word, histograms); the error word and the digit histograms live in sc4[0].
size_t depth_compact_scratch_bytes(size_t n);
// A depth pass's keys, values (Gaussian indices) and packed rectangles: three arrays of one length that travel together.
struct DepthTriple { uint32_t *k = nullptr, *v = nullptr, *r = nullptr; };
struct DepthPrepare {
    const uint32_t* keys_in = nullptr;
    // rect_by_index / out.r (both or neither): the visible Gaussians' packed rectangles, compacted with the pairs; passed on as
    // the passes' `in.r` they travel with the indices and arrive in depth order (gathering them by index afterwards is a
    // random 4-byte read per Gaussian).
    const uint32_t* rect_by_index = nullptr;
    DepthTriple out;
    uint32_t* partial = nullptr;
    // offsets_ready: `partial` / info[kInfoVisible] already hold the compaction offsets per 4096 keys and the visible count (the
    // scan of tilesTouched produced them on the way: a key is the sentinel exactly where tilesTouched is 0)
    bool offsets_ready = false;
    const SweepScratch* sc4 = nullptr;
    uint32_t* info = nullptr;            // sort_info
    uint32_t* host = nullptr;            // optional, the pinned host block: gets the top digits too, for a host that reads them after an event
    const DepthSide* side = nullptr;
};
int sort_u32_prepare(const DepthPrepare& p, uint32_t n, hipStream_t stream);
// Passes [first, last): in -> a -> b -> a -> b (radix_sort.hip explains the optional members)
struct DepthPasses {
    DepthTriple in, a, b;                // in.v null: the value is the input index; in.r / a.r / b.r: all or none
    const SweepScratch* sc4 = nullptr;
    int first = 0, last = 0;
    const uint32_t* n_dev = nullptr;
    const DepthSide* drop_side = nullptr;
    uint32_t *rec_a = nullptr, *rec_b = nullptr;
};
int sort_u32_passes(const DepthPasses& p, uint32_t n, hipStream_t stream);
// Scenes beyond 16 M Gaussians: no compaction — the digit counts only (and the words of info and host as sort_u32_prepare);
// the first pass then reads the per-Gaussian keys itself, dropping the sentinels (sort_u32_passes, drop_side).
int sort_u32_prepare_counts(const uint32_t* keys_in, uint32_t n, const SweepScratch* sc4, uint32_t* info, hipStream_t stream,
                            uint32_t* host, const DepthSide* side);

// Column-major emission (emit.hip): count, column scan and emission. The two events (may be null)
// are recorded between the N-sized preparation and the emission kernel, for stage timing.
size_t emit_scratch_bytes(size_t n);
int launch_emit_columns(int n, const uint32_t* sorted_depth, const uint32_t* sorted_idx, const uint32_t* sorted_rect,
                        int grid_x, int grid_y, char* scratch, uint32_t* hist_y, uint64_t* keys,
                        uint32_t* values, hipStream_t stream, hipEvent_t mark_prep_end, hipEvent_t mark_emit_begin);

// Block binning (blockbin.hip): the sorted lists written directly by tile-block owners.
bool blockbin_supported(int grid_x, int grid_y);
size_t blockbin_geo_bytes(size_t n);
size_t blockbin_bin_bytes(size_t r);
// What the block plan's launchers share: the frame's sizes, its tables' two scratch areas and the R-sized block lists.
struct BlockLists {
    int n = 0;                           // visible Gaussians
    int grid_x = 0, grid_y = 0;
    uint32_t r_total = 0;
    char* geo_scratch = nullptr;
    char* bin_scratch = nullptr;
    uint64_t* ent_rd = nullptr;          // (rectangle | depth bits) of the block-list entries
    uint32_t* ent_idx = nullptr;         // their Gaussians
};
// What both blend launchers read and write.
struct BlendIO {
    const uint32_t* ranges = nullptr;
    const float* means2D = nullptr;
    const float* colors = nullptr;
    bool colors_are_shs = false;                 // (`colors` = the SH array: TileFeed::dc_stride)
    const float* conic_opacity = nullptr;
    float* final_t = nullptr;
    uint32_t* n_contrib = nullptr;
    const float* background = nullptr;
    float* out_color = nullptr;
    unsigned long long* staged_counter = nullptr;
    float t_cutoff = 0.0f;
    DepthTarget depth;                           // (out_depth: the depth channel too, blend_core.hpp)
};
// The order of a blend's workgroups and its deep tiles.
struct BlendOrder {
    const uint32_t* tile_order = nullptr;        // (longest tiles first: TileOrder, blend_core.hpp)
    uint32_t* tile_ticks = nullptr;
    const uint32_t* deep_count = nullptr;        // (device word: the order's leading entries that get four waves, blend.hip)
    bool deep_all = false;                       // (every tile gets four waves)
    int deep_waves = 4;                          // (... or 8 or 16: frames whose work sits in few tiles)
};
// sorted: the l.n visible Gaussians in depth order
int launch_block_binning(const BlockLists& l, const DepthTriple& sorted, uint32_t* ranges, bool close_single, hipStream_t stream,
                         hipEvent_t ev_coarse_end, uint32_t* nonempty_tiles = nullptr, uint32_t* skipped_stamp = nullptr,
                         int cus = 256);
int launch_block_emit(const BlockLists& l, uint64_t* keys, uint32_t* values, hipStream_t stream,
                      bool beside_blend = false,           // (the blend runs on another stream meanwhile: leave it room)
                      int cus = 256);
int launch_blend_blocks(const FrameDims& d, const BlockLists& l, const BlendIO& io, hipStream_t stream,
                        const BlendOrder& order = BlendOrder{});          // (its deep_* members are not read: the block-fed blend has no deep tiles)

// nonempty (may be null): device word, zero before the launch; receives the number of tiles that got a list
int launch_tile_ranges(const uint64_t* keys, size_t n, uint32_t* ranges, int num_tiles, bool close_single, hipStream_t stream,
                       uint32_t* nonempty = nullptr);

int launch_blend(const FrameDims& d, const BlendIO& io, const uint32_t* point_list, hipStream_t stream,
                 const uint32_t* nonempty_tiles = nullptr, uint32_t num_rendered = 0,       // (both: see blend.hip, four waves per tile)
                 const BlendOrder& order = BlendOrder{});
// Longest tiles first: the order of this call's blend workgroups from the ticks the tiles of the call before left.
constexpr int kTileOrderMax = 32768;      // workgroups (one per tile, patch grid padded) up to which the order is kept: 128 KB of LDS for its sort
int current_device_shape(DeviceShape* out);                // the current device's, cached per device (thread_state.hip)
int tile_order_workgroups(const FrameDims& d);
// ticks / ticks_before: the tile times of the history's last frame and of the one before it; *sorted = false (and nothing
// launched): this device has no room for the sort's LDS
// deep_count (device word, optional): receives how many leading entries of the order are DEEP tiles (blend.hip);
// wave_slots: the chip's wave slots for the blend kernels (device_shape)
int launch_tile_order(const FrameDims& d, const uint32_t* ticks, const uint32_t* ticks_before, uint32_t* order, uint32_t* stats,
                      hipStream_t stream, bool* sorted, uint32_t* deep_count, const DeviceShape& shape);

int launch_exp_test(int n, const float* in, float* out, hipStream_t stream);
int launch_footprint_test(int n, const float* xy, const float* conic_opacity, const int32_t* tile_xy, int width, int height,
                          uint8_t* misses, hipStream_t stream);

}  // namespace gsr
