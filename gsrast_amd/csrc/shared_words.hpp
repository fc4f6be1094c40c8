// The words that kernels of several files and the host share by position: the pinned host block of a thread's calls
// (Readback::host, thread_state.hip) and GeoScratch::sort_info (chunks.hip). This header is the only place where their
// numbers appear; kernels and launchers receive the block's BASE and index it by these names.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gsr {

// ---- the pinned host block: mapped host memory, written by the kernels that compute the figures, read by the host after
// gsr_forward's one event wait (no copy command in between). The layout is this struct — its fields cannot overlap —, and
// the kernels, which take the block as u32 words, index it by the word numbers derived from it.
constexpr uint32_t kAsyncSlots = 64;       // error-word slots handed out in turn, one per gsr_forward call
struct AsyncSlot { uint32_t err_n, err_r, serial, zero; };   // {N-sized sort gave up, R-sized sort gave up (both written by the kernels themselves), serial of the owning call, 0}
struct HostBlock {
    uint64_t total;            // the sum of tilesTouched without the u32 wrap-around (partial_scan_kernel); numRendered is its low word
    uint64_t staged;           // the staged-record count lands here (GSR_FLAG_COUNT_STAGED, a copy command)
    uint64_t big_instances;    // the instances of the splats of kBigSplatTiles tiles and more (partial_scan_kernel)
    uint32_t visible;          // V: the Gaussians with a tile (partial_scan_kernel)
    uint32_t top_digits;       // distinct top-byte digits of the visible depth keys (top_digit_count_kernel)
    uint32_t side_way;         // the depth order's side way is taken (partial_scan_kernel)
    uint32_t side_lo;          // side keys below the main top byte (top_digit_count_kernel)
    uint32_t side_counted;     // side keys as the scan counted them (partial_scan_kernel)
    uint32_t side_listed;      // side keys as the compaction listed them (top_digit_count_kernel)
    uint32_t unused[4];
    AsyncSlot async[kAsyncSlots];
};
#define GSR_WORD_OF(type, field) ((uint32_t)(offsetof(type, field) / sizeof(uint32_t)))
enum HostWord : uint32_t {
    kHostTotal = GSR_WORD_OF(HostBlock, total), kHostStaged = GSR_WORD_OF(HostBlock, staged),
    kHostBigInstances = GSR_WORD_OF(HostBlock, big_instances), kHostVisible = GSR_WORD_OF(HostBlock, visible),
    kHostTopDigits = GSR_WORD_OF(HostBlock, top_digits), kHostSideWay = GSR_WORD_OF(HostBlock, side_way),
    kHostSideLo = GSR_WORD_OF(HostBlock, side_lo), kHostSideCounted = GSR_WORD_OF(HostBlock, side_counted),
    kHostSideListed = GSR_WORD_OF(HostBlock, side_listed), kHostAsyncBase = GSR_WORD_OF(HostBlock, async),
};
constexpr uint32_t kAsyncSlotWords = sizeof(AsyncSlot) / sizeof(uint32_t);
enum AsyncWord : uint32_t {
    kAsyncErrN = GSR_WORD_OF(AsyncSlot, err_n), kAsyncErrR = GSR_WORD_OF(AsyncSlot, err_r),
    kAsyncSerial = GSR_WORD_OF(AsyncSlot, serial), kAsyncZero = GSR_WORD_OF(AsyncSlot, zero),
};
constexpr uint32_t kHostWords = sizeof(HostBlock) / sizeof(uint32_t);
static_assert(offsetof(HostBlock, total) % 8 == 0 && offsetof(HostBlock, staged) % 8 == 0 && offsetof(HostBlock, big_instances) % 8 == 0,
              "the 64-bit host fields are 8-byte aligned");
static_assert(offsetof(HostBlock, async) >= offsetof(HostBlock, side_listed) + sizeof(uint32_t), "the async slots start behind the fixed fields");

// ---- GeoScratch::sort_info: device words, laid out the same way
struct InfoBlock {
    uint32_t top_digits;       // distinct top-byte digits of the visible depth keys
    uint32_t visible;          // the keys the depth passes sort: V, or the main keys only when the side way is taken
    uint64_t total;            // the sum of tilesTouched without the u32 wrap-around
    uint32_t nonempty_tiles;   // tiles with a list: zeroed by top_digit_count_kernel, counted by the tile ranges, read by the blend
    uint32_t unused[3];
    uint32_t side[3];          // the side list's words (DepthSide::words), indexed by SideWord
};
enum InfoWord : uint32_t {
    kInfoTopDigits = GSR_WORD_OF(InfoBlock, top_digits), kInfoVisible = GSR_WORD_OF(InfoBlock, visible),
    kInfoTotal = GSR_WORD_OF(InfoBlock, total), kInfoNonemptyTiles = GSR_WORD_OF(InfoBlock, nonempty_tiles),
    kInfoSide = GSR_WORD_OF(InfoBlock, side),
};
enum SideWord : uint32_t {
    kSideTaken = 0,            // the side way is taken (decided by the scan)
    kSideListed = 1,           // keys on the list
    kSideBelow = 2,            // those of them below the main top byte
};
constexpr uint32_t kInfoBytes = 128;
static_assert(offsetof(InfoBlock, total) % 8 == 0 && sizeof(InfoBlock) <= kInfoBytes, "sort_info's words");
#undef GSR_WORD_OF

// What gsr_forward reads of the host block, decoded once after the event wait.
struct FrameCounts {
    uint32_t visible;                    // V: the length of every depth-ordered array
    unsigned long long total;            // the true instance count
    bool four_passes;                    // the visible keys take more than one top byte
    bool side_way;                       // (then the stream's keys share their top byte: three passes)
    uint32_t side_m, side_lo;            // keys on the side way, and those of them below the main top byte (0 without the side way)
    uint32_t side_listed;                // the keys the compaction actually put on the side list
    unsigned long long big_instances;
};
inline FrameCounts decode_host_words(const uint32_t* host) {
    FrameCounts c;
    c.visible = host[kHostVisible];
    c.total = (unsigned long long)host[kHostTotal] | ((unsigned long long)host[kHostTotal + 1] << 32);
    c.four_passes = host[kHostTopDigits] > 1u;
    c.side_way = host[kHostSideWay] != 0u;
    c.side_m = c.side_way ? host[kHostSideCounted] : 0u;
    c.side_lo = c.side_way ? host[kHostSideLo] : 0u;
    c.side_listed = host[kHostSideListed];
    c.big_instances = (unsigned long long)host[kHostBigInstances] | ((unsigned long long)host[kHostBigInstances + 1] << 32);
    return c;
}

}  // namespace gsr
