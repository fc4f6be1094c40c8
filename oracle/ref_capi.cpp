// ref_capi.cpp — a thin C ABI over the reference's own translation units (GSCuda.cu, AuxBuffer.cu, CudaHelpers.cu),
// compiled for the host against the stand-ins of oracle/ref_host/ by oracle/build_ref.py and linked into
// oracle/_ref/libgscuda_ref.so. TEST INFRASTRUCTURE ONLY; oracle/ref_cpu.py is its only caller.
//
// This file is the project's own text. It includes the reference's two headers at build time (from the reference tree)
// and calls gscuda::forward / forwardPoints / getHigherMsb / required<> / fromChunk as they stand. The three chunks
// are zero-filled host memory, 128-byte aligned (the reference asks for no slack on the geometry chunk); after the call
// every array of the three states is found again with the reference's own fromChunk and copied out.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "GSCuda.cuh"
#include "AuxBuffer.cuh"
#include <cub/cub.cuh>

namespace gscuda {
uint32_t getHigherMsb(uint32_t n);      // GSCuda.cu:481, not declared in GSCuda.cuh
}

namespace {

struct Chunk {
    char* base = nullptr;
    size_t bytes = 0;
    int calls = 0;
    char* take(size_t n) {
        std::free(base);
        bytes = n;
        ++calls;
        const size_t rounded = ((n ? n : 1) + 127) / 128 * 128;
        base = static_cast<char*>(std::aligned_alloc(128, rounded));
        std::memset(base, 0, rounded);
        return base;
    }
    ~Chunk() { std::free(base); }
};

std::vector<uint64_t> g_keys_unsorted, g_keys;
std::vector<uint32_t> g_values_unsorted, g_values;

template <typename T>
void copy_out(void* dst, const T* src, size_t count) {
    if (dst && count) std::memcpy(dst, src, sizeof(T) * count);
}

}  // namespace

extern "C" {

// Every pointer is host memory. Inputs as gscuda::forward takes them (colors_precomp, cov3d_precomp, radii, rects: null
// for "not given"). Outputs: null for "not wanted". The four lists of the BinningState hold num_rendered entries, known
// only after the call: they are kept until the next call and fetched with gsref_last_lists.
struct gsref_forward_args {
    int32_t num_gaussians, width, height;
    float scale_modifier, tan_fovx, tan_fovy;
    const float* background;
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3d_precomp;
    const float* view;
    const float* proj;
    const float* cam_pos;
    float* out_color;            // in / out: [3][H][W], left untouched when nothing is rendered
    int32_t* radii;              // the caller's radii, or null: GeometryState::internalRadii is used
    int32_t* rects;              // [N][2], or null: the radius path
    // GeometryState, [N] each
    uint32_t* tiles_touched;
    float* depths;
    uint8_t* clamped;            // [N][3]
    int32_t* internal_radii;
    float* means2D;
    float* cov3D;
    float* conic_opacity;
    float* rgb;
    uint32_t* point_offsets;
    // ImageState, [W * H] each (the reference sizes ranges by pixels, not by tiles)
    uint32_t* ranges;            // [W * H][2]
    uint32_t* n_contrib;
    float* accum_alpha;
    // what the call did
    uint32_t num_rendered;
    int32_t geometry_calls, image_calls, binning_calls;
    uint64_t geometry_bytes, image_bytes, binning_bytes;
};

// The temporary sizes the cub stand-in reports from now on (CUB's own are a property of CUB; the stand-in needs none).
void gsref_set_temp_sizes(size_t scan, size_t sort) {
    ref_host::g_temp_sizes.scan = scan;
    ref_host::g_temp_sizes.sort = sort;
}

uint32_t gsref_higher_msb(uint32_t n) { return gscuda::getHigherMsb(n); }

size_t gsref_required_geometry(int n) { return gscuda::required<gscuda::gs::GeometryState>(n); }
size_t gsref_required_image(int n) { return gscuda::required<gscuda::gs::ImageState>(n); }
size_t gsref_required_binning(int n) { return gscuda::required<gscuda::gs::BinningState>(n); }
size_t gsref_required_points_geometry(int n) { return gscuda::required<gscuda::pc::GeometryState>(n); }
size_t gsref_required_points_image(int n) { return gscuda::required<gscuda::pc::ImageState>(n); }

// out: tilesTouched, scanSize, scanningSpace, depths, clamped, internalRadii, means2D, cov3D, conicOpacity, rgb,
// pointOffsets, end of the chunk (addresses as integers; scanSize is a size).
void gsref_geometry_from_chunk(uint64_t base, int n, uint64_t out[12]) {
    char* chunk = reinterpret_cast<char*>(base);
    gscuda::gs::GeometryState s = gscuda::gs::GeometryState::fromChunk(chunk, n);
    const void* p[] = {s.tilesTouched, nullptr, s.scanningSpace, s.depths, s.clamped, s.internalRadii, s.means2D, s.cov3D,
                       s.conicOpacity, s.rgb, s.pointOffsets, chunk};
    for (int i = 0; i < 12; ++i) out[i] = reinterpret_cast<uint64_t>(p[i]);
    out[1] = s.scanSize;
}

// out: ranges, nContrib, accumAlpha, end
void gsref_image_from_chunk(uint64_t base, int n, uint64_t out[4]) {
    char* chunk = reinterpret_cast<char*>(base);
    gscuda::gs::ImageState s = gscuda::gs::ImageState::fromChunk(chunk, n);
    const void* p[] = {s.ranges, s.nContrib, s.accumAlpha, chunk};
    for (int i = 0; i < 4; ++i) out[i] = reinterpret_cast<uint64_t>(p[i]);
}

// out: pointListKeysUnsorted, pointListKeys, pointListUnsorted, pointList, sortingSize, listSortingSpace, end
void gsref_binning_from_chunk(uint64_t base, int n, uint64_t out[7]) {
    char* chunk = reinterpret_cast<char*>(base);
    gscuda::gs::BinningState s = gscuda::gs::BinningState::fromChunk(chunk, n);
    const void* p[] = {s.pointListKeysUnsorted, s.pointListKeys, s.pointListUnsorted, s.pointList, nullptr, s.listSortingSpace, chunk};
    for (int i = 0; i < 7; ++i) out[i] = reinterpret_cast<uint64_t>(p[i]);
    out[4] = s.sortingSize;
}

// out: depth, outColor, defaultDepth, end
void gsref_points_image_from_chunk(uint64_t base, int n, uint64_t out[4]) {
    char* chunk = reinterpret_cast<char*>(base);
    gscuda::pc::ImageState s = gscuda::pc::ImageState::fromChunk(chunk, n);
    const void* p[] = {s.depth, s.outColor, s.defaultDepth, chunk};
    for (int i = 0; i < 4; ++i) out[i] = reinterpret_cast<uint64_t>(p[i]);
}

int gsref_forward(gsref_forward_args* a) {
    if (!a || a->num_gaussians <= 0 || a->width <= 0 || a->height <= 0) return 1;   // (pointOffsets[N - 1] needs N >= 1)
    Chunk geometry, binning, image;
    const int n = a->num_gaussians, pixels = a->width * a->height;
    gscuda::forward([&](size_t b) { return geometry.take(b); }, [&](size_t b) { return binning.take(b); },
                    [&](size_t b) { return image.take(b); }, n, 0, 0, a->background, a->width, a->height, a->means3D, a->shs,
                    a->colors_precomp, a->opacities, a->scales, a->scale_modifier, a->rotations, a->cov3d_precomp, a->view,
                    a->proj, a->cam_pos, a->tan_fovx, a->tan_fovy, false, a->out_color, a->radii, a->rects, nullptr, nullptr);
    char* chunk = geometry.base;
    const gscuda::gs::GeometryState g = gscuda::gs::GeometryState::fromChunk(chunk, n);
    copy_out(a->tiles_touched, g.tilesTouched, n);
    copy_out(a->depths, g.depths, n);
    copy_out(a->clamped, reinterpret_cast<const uint8_t*>(g.clamped), 3 * (size_t)n);
    copy_out(a->internal_radii, g.internalRadii, n);
    copy_out(a->means2D, reinterpret_cast<const float*>(g.means2D), 2 * (size_t)n);
    copy_out(a->cov3D, g.cov3D, 6 * (size_t)n);
    copy_out(a->conic_opacity, reinterpret_cast<const float*>(g.conicOpacity), 4 * (size_t)n);
    copy_out(a->rgb, reinterpret_cast<const float*>(g.rgb), 3 * (size_t)n);
    copy_out(a->point_offsets, g.pointOffsets, n);
    a->num_rendered = g.pointOffsets[n - 1];        // GSCuda.cu:772
    chunk = image.base;
    const gscuda::gs::ImageState im = gscuda::gs::ImageState::fromChunk(chunk, pixels);
    copy_out(a->ranges, reinterpret_cast<const uint32_t*>(im.ranges), 2 * (size_t)pixels);
    copy_out(a->n_contrib, im.nContrib, pixels);
    copy_out(a->accum_alpha, im.accumAlpha, pixels);
    g_keys_unsorted.clear(); g_keys.clear(); g_values_unsorted.clear(); g_values.clear();
    if (binning.calls > 0) {
        const size_t r = a->num_rendered;
        chunk = binning.base;
        const gscuda::gs::BinningState b = gscuda::gs::BinningState::fromChunk(chunk, (int)r);
        g_keys_unsorted.assign(b.pointListKeysUnsorted, b.pointListKeysUnsorted + r);
        g_keys.assign(b.pointListKeys, b.pointListKeys + r);
        g_values_unsorted.assign(b.pointListUnsorted, b.pointListUnsorted + r);
        g_values.assign(b.pointList, b.pointList + r);
    }
    a->geometry_calls = geometry.calls; a->image_calls = image.calls; a->binning_calls = binning.calls;
    a->geometry_bytes = geometry.bytes; a->image_bytes = image.bytes; a->binning_bytes = binning.bytes;
    return 0;
}

// The BinningState lists of the last gsref_forward call (empty when it rendered nothing): returns their length; copies
// them where a pointer is given.
uint64_t gsref_last_lists(uint64_t* keys_unsorted, uint64_t* keys, uint32_t* values_unsorted, uint32_t* values) {
    copy_out(keys_unsorted, g_keys_unsorted.data(), g_keys_unsorted.size());
    copy_out(keys, g_keys.data(), g_keys.size());
    copy_out(values_unsorted, g_values_unsorted.data(), g_values_unsorted.size());
    copy_out(values, g_values.data(), g_values.size());
    return g_keys.size();
}

// gscuda::forwardPoints; out_color [3][H][W], depth [H][W] (pc::ImageState::depth). calls[3] / bytes[3]: geometry,
// binning, image allocator.
int gsref_forward_points(int n, int width, int height, const float* background, const float* means3D /*[N][3]*/,
                         const float* shs, const float* proj, float* out_color, float* depth, int32_t calls[3], uint64_t bytes[3]) {
    if (n <= 0 || width <= 0 || height <= 0) return 1;
    Chunk geometry, binning, image;
    gscuda::forwardPoints([&](size_t b) { return geometry.take(b); }, [&](size_t b) { return binning.take(b); },
                          [&](size_t b) { return image.take(b); }, n, 0, 0, background, width, height, means3D, shs, nullptr,
                          nullptr, nullptr, 1.0f, nullptr, nullptr, nullptr, proj, nullptr, 0.0f, 0.0f, false, out_color, nullptr,
                          nullptr, nullptr, nullptr);
    char* chunk = image.base;
    const gscuda::pc::ImageState im = gscuda::pc::ImageState::fromChunk(chunk, width * height);
    copy_out(depth, im.depth, (size_t)width * height);
    if (calls) { calls[0] = geometry.calls; calls[1] = binning.calls; calls[2] = image.calls; }
    if (bytes) { bytes[0] = geometry.bytes; bytes[1] = binning.bytes; bytes[2] = image.bytes; }
    return 0;
}

}  // extern "C"
