// The layout of the caller's chunks (include/gsrast_amd.h): the three states carved from them, this library's own scratch
// inside GeometryState::scanningSpace and BinningState::sortingSpace, and what a receipt says about them afterwards.
//
// The chunk carving follows reference apps/gsrast/gscuda/AuxBuffer.cu:13-21 (obtain) and :44-89 (fromChunk).
#include <algorithm>

#include "api_internal.hpp"

namespace gsr {
namespace {

// obtain(): AuxBuffer.cu:13-21 — align the running pointer up, hand out `bytes`.
template <typename T>
inline void obtain(char*& chunk, T*& out, size_t bytes, size_t align = 128) {
    const size_t offset = reinterpret_cast<size_t>(chunk);
    const size_t aligned = align * ((offset + align - 1) / align);
    out = reinterpret_cast<T*>(aligned);
    chunk = reinterpret_cast<char*>(aligned + bytes);
}

inline size_t align128(size_t v) { return (v + 127) / 128 * 128; }

}  // namespace

GeoScratch carve_geo_scratch(char* base, size_t n) {
    GeoScratch g;
    size_t off = 0;
    g.scan_temp = base + off; off += align128(scan_temp_bytes(n));
    g.depth_key = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.rect_idx = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.sort_info = reinterpret_cast<uint32_t*>(base + off); off += kInfoBytes;
    g.vis_partial = reinterpret_cast<uint32_t*>(base + off); off += depth_compact_scratch_bytes(n);
    g.main_partial = reinterpret_cast<uint32_t*>(base + off); off += depth_compact_scratch_bytes(n);
    g.big_partial = reinterpret_cast<uint32_t*>(base + off); off += depth_compact_scratch_bytes(n);
    g.wave_sums = reinterpret_cast<uint4*>(base + off); off += align128(16 * ((n + 63) / 64));
    g.side.k = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * kDepthSideMax);
    g.side.v = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * kDepthSideMax);
    g.side.r = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * kDepthSideMax);
    // (three groups of three consecutive arrays: between its passes the depth order keeps the triples as 12-byte RECORDS in
    // the room of a group — a and b, or c where there is no compaction to fill them)
    g.c.k = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.c.v = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.c.r = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    off += 4 * kDepthSideMax; g.a.k = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    off += 4 * kDepthSideMax; g.a.v = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    off += 4 * kDepthSideMax; g.a.r = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.b.k = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.b.v = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.b.r = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * n);
    g.sweep = carve_sweep_scratch(base + off, n); off += sweep_scratch_bytes(n);
    for (auto& sw : g.sweep_more) { sw = carve_sweep_scratch(base + off, n); off += sweep_scratch_bytes(n); }
    g.emit_scratch = base + off; off += align128(emit_scratch_bytes(n));
    g.block_scratch = base + off; off += align128(blockbin_geo_bytes(n));
    g.bytes = off;
    return g;
}

BinScratch carve_bin_scratch(char* base, size_t r) {
    BinScratch b;
    size_t off = 0;
    b.tmp_k = reinterpret_cast<uint64_t*>(base + off); off += align128(8 * r);
    b.tmp_v = reinterpret_cast<uint32_t*>(base + off); off += align128(4 * r);
    b.sweep = carve_sweep_scratch(base + off, r); off += sweep_scratch_bytes(r);
    b.sweep2 = carve_sweep_scratch(base + off, r); off += sweep_scratch_bytes(r);
    b.bytes = off;
    return b;
}

// What a gsr_backward call may read of the forward call that issued `r` (see gsr_backward_args.receipt): derived from
// the receipt and the chunk layouts alone — no state of this library is consulted, so any host thread may ask, after any
// number of other calls, as long as the chunks are as that call left them.
int lists_of_receipt(const gsr_forward_receipt& r, int n, int width, int height, int row_begin, int row_end,
                     const void* point_list, BlockFeed* feed, bool* from_blocks, bool* lists_written) {
    *from_blocks = false;
    *lists_written = true;
    if (r.magic != GSR_RECEIPT_MAGIC) return GSR_ERR_INVALID_ARG;
    if (r.num_gaussians != n || r.width != width || r.height != height || r.tile_row_begin != row_begin ||
        r.tile_row_end != row_end || !r.geometry_chunk || !r.image_chunk)
        return GSR_ERR_INVALID_ARG;
    if (r.num_rendered == 0) return GSR_OK;                     // (no binning chunk, no lists: the caller zeroes its outputs)
    if (!r.binning_chunk) return GSR_ERR_INVALID_ARG;
    gsr_binning_state bin;
    gsr_binning_from_chunk(r.binning_chunk, r.num_rendered, &bin);
    if (point_list != bin.values) return GSR_ERR_INVALID_ARG;
    *lists_written = !(r.plan_used & GSR_PLAN_LISTS_SKIPPED);
    // (not after a blend from the sorted lists: BlockMeta::walked, which bounds the per-entry sums, is the block-fed
    // blend's by-product; the backward then takes the sorted lists for every tile)
    if ((r.plan_used & 0xFFu) == GSR_PLAN_BLOCKS && !(r.plan_used & GSR_PLAN_BLEND_FROM_LISTS)) {
        gsr_geometry_state geom;
        gsr_geometry_from_chunk(r.geometry_chunk, n, &geom);
        const GeoScratch gs = carve_geo_scratch(geom.scanning_space, (size_t)n);
        const int grid_x = (width + kTile - 1) / kTile, grid_y = (height + kTile - 1) / kTile;
        // the block lists (read by nothing else once the forward call is complete) and, for the per-entry gradient sums,
        // the 8 R bytes of keysUnsorted: the (rectangle | depth) halves of the block-list entries there are dead after
        // the unit masks and the emission
        *feed = block_feed((int)r.num_visible, grid_x, grid_y, r.num_rendered, gs.block_scratch, bin.values_unsorted, bin.sorting_space);
        feed->acc = reinterpret_cast<float*>(bin.keys_unsorted);
        feed->acc_floats = 2ull * (unsigned long long)r.num_rendered;
        *from_blocks = true;
    }
    if (!*from_blocks && !*lists_written) return GSR_ERR_INVALID_ARG;
    return GSR_OK;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

char* gsr_geometry_from_chunk(char* chunk, int n, gsr_geometry_state* s) {
    const size_t N = (size_t)(n < 0 ? 0 : n);
    obtain(chunk, s->tiles_touched, sizeof(uint32_t) * N);
    s->scan_size = carve_geo_scratch(nullptr, N).bytes;
    s->num_rendered = 0;
    obtain(chunk, s->scanning_space, s->scan_size);
    obtain(chunk, s->depths, sizeof(float) * N);
    obtain(chunk, s->clamped, sizeof(uint8_t) * N * 3);
    obtain(chunk, s->internal_radii, sizeof(int32_t) * N);
    obtain(chunk, s->means2D, sizeof(float) * 2 * N);
    obtain(chunk, s->cov3D, sizeof(float) * 6 * N);
    obtain(chunk, s->conic_opacity, sizeof(float) * 4 * N);
    obtain(chunk, s->rgb, sizeof(float) * 3 * N);
    obtain(chunk, s->point_offsets, sizeof(uint32_t) * N);
    return chunk;
}

char* gsr_image_from_chunk(char* chunk, int size, gsr_image_state* s) {
    const size_t P = (size_t)(size < 0 ? 0 : size);
    obtain(chunk, s->ranges, sizeof(uint32_t) * 2 * P);
    obtain(chunk, s->n_contrib, sizeof(uint32_t) * P);
    obtain(chunk, s->accum_alpha, sizeof(float) * P);
    return chunk;
}

char* gsr_binning_from_chunk(char* chunk, size_t size, gsr_binning_state* s) {
    obtain(chunk, s->keys_unsorted, sizeof(uint64_t) * size);
    obtain(chunk, s->keys, sizeof(uint64_t) * size);
    obtain(chunk, s->values_unsorted, sizeof(uint32_t) * size);
    obtain(chunk, s->values, sizeof(uint32_t) * size);
    s->sorting_size = std::max(std::max(carve_bin_scratch(nullptr, size).bytes, sort_temp_bytes(size)), blockbin_bin_bytes(size));
    obtain(chunk, s->sorting_space, s->sorting_size);
    return chunk;
}

size_t gsr_required_geometry(int n) { gsr_geometry_state s; return reinterpret_cast<size_t>(gsr_geometry_from_chunk(nullptr, n, &s)); }
size_t gsr_required_image(int size) { gsr_image_state s; return reinterpret_cast<size_t>(gsr_image_from_chunk(nullptr, size, &s)); }
size_t gsr_required_binning(size_t size) { gsr_binning_state s; return reinterpret_cast<size_t>(gsr_binning_from_chunk(nullptr, size, &s)); }

}  // extern "C"
