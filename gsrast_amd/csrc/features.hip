// N-channel feature maps of a drawn frame (include/gsrast_amd_features.h): sum_i f_i alpha_i T_i per pixel over the sorted lists a
// forward call left, and its gradient — passes of their own, so that the blend, contrib_kernel and render_backward_kernel keep
// their object code. Both kernels are one wavefront per (16 x 16 tile, chunk of K channels), four pixels per lane, tiles
// dealt in XCD patches, batches of 64 list entries with ids two batches ahead and records one batch ahead, compacted by
// record_misses_tile, the survivors' K feature floats staged in wave-private LDS beside their records. List entries are
// bounded by the receipt's R and the scene's N before they index anything.
//
// The skeletons are DUPLICATED on purpose, as absgrad.hip says of itself:
//   - features_forward_kernel is contrib_kernel's walk (contrib.hip): the forward's staging, filter, reference-order power,
//     exp_ref, alpha and T = T (1 - alpha) replayed from 1, the pixels of a record decided by n_contrib and the power and alpha
//     tests; what a blended (record, pixel) adds is composite_record's acc = fmaf(f, alpha T, acc) per channel, and a pixel leaves
//     as tile_lanes_write forms it, acc + final_t bg. With the frame's colours and background that is out_color bit for bit.
//   - features_backward_kernel is render_backward_kernel's walk (backward.hip) as absgrad_kernel restates it: back to front from
//     n_contrib with T = final_t, T_i = T_{i+1} rcp(1 - alpha), and from dL_dalpha on (GEO) the render backward's own lines — the
//     clamp rule raw > 0.99, dpow, gop, u = K d, the pixel-by-pixel cov2D sums — added into slots 0..5 and 9..11 of the double
//     sums a gsr_backward of the same frame then reads (slots 6..8, the colour's, are not touched). Without GEO neither cg nor
//     the suffix sum S is formed: w g is all a frozen geometry needs.
// A record's K feature sums are reduced eight at a time by the fold-and-pack of backward.hip's wave_sum12 (three lane swaps
// pack eight values into one register, four DPP steps finish: 8 sums for the price of about 2 separate ones) and leave as ONE
// double atomic instruction per eight channels, eight lanes on 64 contiguous bytes of feature_sums_f64.
#include <hip/hip_runtime.h>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "blend_core.hpp"           // (and, through gsr_common.hpp, frame_policy.hpp: tile_band)
#include "blockbin.hpp"             // (lists_of_receipt, tile_order_of_call)
#include "../../include/gsrast_amd_features.h"

namespace gsr {
namespace {

// The chunk width K is a template parameter with two instances: the narrow one serves calls of up to that many channels
// (normals, a label: C = 3 pays for 8 accumulators per pixel, not 16), the wide one every other call. The widths were chosen
// by measuring 8, 16 and 24 on the bench frame: DESIGN.md section 8 has the table, profiles/features_cost.txt the kernels as built.
constexpr int kChunkNarrow = GSR_FEATURES_CHUNK_NARROW, kChunkWide = GSR_FEATURES_CHUNK;
static_assert(kChunkNarrow % 8 == 0 && kChunkNarrow >= 8 && kChunkWide % 8 == 0 && kChunkWide >= kChunkNarrow && kChunkWide <= 32,
              "the reduction packs eight sums per register");
inline int chunk_of(int channels) { return channels <= kChunkNarrow ? kChunkNarrow : kChunkWide; }
constexpr uint32_t kGeoFloats = 12;      // the layout of gsr_backward_args.sums_f64 (backward.hip: kAccFloats)

struct FeatureParams {
    const uint2* ranges;
    const uint32_t* point_list;
    const float2* means2D;
    const float4* conic_opacity;
    const uint32_t* n_contrib;
    const float* final_t;
    const float* features;        // f32[N C]
    const float* background;      // f32[C] or null
    float* out;                   // forward: f32[C W H]
    const float* dL_dout;         // backward: f32[C W H]
    double* feature_sums;         // backward: f64[N C]
    double* geometry_sums;        // backward (GEO): f64[12 N]
    FrameDims dims;
    const uint32_t* tile_order;   // backward: the forward blend's workgroup order, or null: patch order
    uint32_t num_gaussians;
    uint32_t num_rendered;
    uint32_t channels;
};

// A record's K features of one chunk into its staging slot (16-byte aligned: slots are K floats apart), zeros past the call's
// last channel. The row in memory is only known to lie on a 4-byte boundary (C is any number), so it is read float by float;
// the slot is written four floats per LDS instruction.
template <int K>
__device__ __forceinline__ void stage_feature_row(float* slot, const float* row, uint32_t nc) {
#pragma unroll
    for (int c = 0; c < K; c += 4) {
        float4 v;
        v.x = (uint32_t)c < nc ? row[c] : 0.0f;
        v.y = (uint32_t)(c + 1) < nc ? row[c + 1] : 0.0f;
        v.z = (uint32_t)(c + 2) < nc ? row[c + 2] : 0.0f;
        v.w = (uint32_t)(c + 3) < nc ? row[c + 3] : 0.0f;
        *reinterpret_cast<float4*>(slot + c) = v;
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <int K>
struct FeatureStage {                    // one wave's staging area (wave-private LDS: no barrier)
    float2 xy[kWave];
    float4 co[kWave];                    // the filter's pre-scaled conic and floor (StagedRecords::co)
    float4 raw[kWave];                   // conic + opacity as fetched
    uint32_t number[kWave];              // the record's 1-based position in the tile's list
    float feat[kWave * K];          // its K features (zeros past the last channel)
    unsigned long long exp_tab[32];
};

// stage_contrib (contrib.hip) with the record's features in place of its statistics: the same footprint test, filter conic,
// floor and margins, so that the candidates of a record are the forward's. An entry that names no Gaussian of the scene is dropped.
template <int K>
__device__ __forceinline__ uint32_t stage_features(const TileFeed& f, FeatureStage<K>& st, const RecordBatch& b, const FeatureParams& p,
                                                   uint32_t c0, uint32_t nc) {
    const bool present = b.present() && b.id < p.num_gaussians;
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
        st.number[slot] = pos + rank + 1u;
        stage_feature_row<K>(&st.feat[slot * K], p.features + (size_t)b.id * (size_t)p.channels + c0, nc);
    }
    return (uint32_t)__popcll(m2);
}

// composite_record (blend_core.hpp) as contrib_record restates it, with K channels in place of three. s.last[k] holds the
// pixel's n_contrib.
template <int K>
__device__ __forceinline__ void feature_record(TileLanes& s, const FeatureStage<K>& st, uint32_t j, float (&acc)[4][K]) {
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
    float feat[K];
#pragma unroll
    for (int c = 0; c < K; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(&st.feat[j * K + c]);
        feat[c] = v.x; feat[c + 1] = v.y; feat[c + 2] = v.z; feat[c + 3] = v.w;
    }
    // the reference's operation order from here on (compiled without contraction)
    const float t1 = (raw.x * dx) * dx, bdx = raw.y * dx;
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
            if (__builtin_amdgcn_inverse_ballot_w64(live)) {
                const float w = alpha * s.T[k];
#pragma unroll
                for (int c = 0; c < K; ++c) acc[k][c] = __builtin_fmaf(feat[c], w, acc[k][c]);
                s.T[k] = s.T[k] * (1.0f - alpha);
            }
        }
    }
}

template <int K>
__global__ __launch_bounds__(kWave) void features_forward_kernel(const FeatureParams p) {
    __shared__ FeatureStage<K> st;
    const int lane = (int)threadIdx.x;
    const int rows = p.dims.row_end - p.dims.row_begin;
    // (tiles dealt to the XCDs in patches, as in the forward blend: blend_core.hpp)
    const int tile_local = tile_of_workgroup((int)blockIdx.x, p.dims.grid_x, rows);
    if (tile_local < 0) return;
    const int tile = p.dims.row_begin * p.dims.grid_x + tile_local;
    const int tx = tile % p.dims.grid_x, ty = tile / p.dims.grid_x;
    const uint32_t c0 = blockIdx.y * (uint32_t)K, nc = min((uint32_t)K, p.channels - c0);
    const size_t plane = (size_t)p.dims.width * (size_t)p.dims.height;

    TileLanes s;
    tile_lanes_init(s, tx, ty, lane, p.dims.width, p.dims.height, -1);
    float acc[4][K];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < K; ++c) acc[k][c] = 0.0f;

    // (R == 0: the forward call left even the tile ranges unwritten — what is read here is then not looked at)
    const uint2 range = p.ranges[tile];
    const bool has_list = p.num_rendered != 0u && range.x < range.y && range.y <= p.num_rendered;
    uint32_t walk = 0u;
    if (has_list) {
        uint32_t mine = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (s.inside[k]) s.last[k] = p.n_contrib[(size_t)(s.py0 + 4 * k) * (size_t)p.dims.width + (size_t)s.px];
            mine = mine > s.last[k] ? mine : s.last[k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine = max(mine, (uint32_t)__shfl_xor((int)mine, off, kWave));
        walk = min(range.y - range.x, mine);           // the walk ends with the tile's last contributor
    }
    if (walk != 0u) {
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
        RecordBatch b0 = next_batch(0);
        fetch(b0);
        RecordBatch b1 = next_batch(kWave);
        for (uint32_t pos = 2 * kWave; b0.valid; pos += kWave) {
            fetch(b1);
            RecordBatch b2 = next_batch(pos);
            const uint32_t kept = stage_features(feed, st, b0, p, c0, nc);
            // wave-private LDS: the writes above and the reads below are ordered inside the wave
            for (uint32_t j = 0; j < kept; ++j) feature_record(s, st, j, acc);
            b0 = b1;
            b1 = b2;
        }
    }
    // tile_lanes_write's expression per channel: acc + final_t bg (a tile without a list: 0 + 1 bg)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!s.inside[k]) continue;
        const size_t pid = (size_t)(s.py0 + 4 * k) * (size_t)p.dims.width + (size_t)s.px;
        const float tf = has_list ? p.final_t[pid] : 1.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if ((uint32_t)c >= nc) continue;
            float* dst = p.out + (size_t)(c0 + (uint32_t)c) * plane + pid;
            if (p.background) *dst = acc[k][c] + tf * p.background[c0 + (uint32_t)c];
            else *dst = acc[k][c];
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
#define GSR_DPP(v, ctrl) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false))
__device__ __forceinline__ void swap32(float& x, float& y) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float& x, float& y) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}
// Sums of EIGHT per-lane values over the 64 lanes (the first eight of backward.hip's wave_sum12): v_permlane32_swap and
// v_permlane16_swap fold the lanes while packing the values side by side, one select + row_ror:8 packs two registers into one
// and three quad / half-row steps finish. On return lane 0 / 32 / 16 / 48 / 8 / 40 / 24 / 56 holds the total of value 0 / ... / 7.
__device__ __forceinline__ float wave_sum8(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7, int lane) {
    swap32(a0, a1); float p = a0 + a1;           // rows 0, 1: value 0 (lanes l and l + 32 added); rows 2, 3: value 1
    swap32(a2, a3); float q = a2 + a3;
    swap32(a4, a5); float r = a4 + a5;
    swap32(a6, a7); float t = a6 + a7;
    swap16(p, q); const float t0 = p + q;        // rows: value 0, 2, 1, 3, each added over the four 16-lane groups
    swap16(r, t); const float t1 = r + t;        // rows: value 4, 6, 5, 7
    const bool upper = (lane & 8) != 0;
    float u = (upper ? t1 : t0) + GSR_DPP(upper ? t0 : t1, 0x128);      // row_ror:8: lanes 0-7 of a row now carry t0, lanes 8-15 t1
    u += GSR_DPP(u, 0xB1);                       // quad_perm [1,0,3,2]
    u += GSR_DPP(u, 0x4E);                       // quad_perm [2,3,0,1]
    u += GSR_DPP(u, 0x141);                      // row_half_mirror
    return u;
}
// ... and of FOUR more (wave_sum12's last four): on return every lane of row 0 / 2 / 1 / 3 holds the total of value 0 / 1 / 2 / 3.
__device__ __forceinline__ float wave_sum4(float a0, float a1, float a2, float a3) {
    swap32(a0, a1); float pp = a0 + a1;
    swap32(a2, a3); float qq = a2 + a3;
    swap16(pp, qq); float w = pp + qq;           // rows: value 0, 2, 1, 3
    w += GSR_DPP(w, 0x128);
    w += GSR_DPP(w, 0xB1);
    w += GSR_DPP(w, 0x4E);
    w += GSR_DPP(w, 0x141);
    return w;
}
#undef GSR_DPP

template <int K, bool GEO>
__global__ __launch_bounds__(kWave) void features_backward_kernel(const FeatureParams p) {
    __shared__ uint32_t s_id[kWave];
    __shared__ uint32_t s_idx[kWave];
    __shared__ float2 s_xy[kWave];
    __shared__ float4 s_co[kWave];
    __shared__ float s_floor[kWave];
    __shared__ __attribute__((aligned(16))) float s_feat[kWave * K];
    __shared__ unsigned long long s_exp[32];
    exp_table_init(s_exp, (int)threadIdx.x);       // (wave-private LDS: ordered inside the wave)

    const int rows = p.dims.row_end - p.dims.row_begin;
    const int tile_local = tile_of_workgroup(p.tile_order ? (int)p.tile_order[blockIdx.x] : (int)blockIdx.x, p.dims.grid_x, rows);
    if (tile_local < 0) return;
    const int tile = p.dims.row_begin * p.dims.grid_x + tile_local;
    const int tx = tile % p.dims.grid_x, ty = tile / p.dims.grid_x;
    const int lane = threadIdx.x;
    const int px = tx * kTile + (lane & 15), py0 = ty * kTile + (lane >> 4);
    const float fx = (float)px;
    const size_t plane = (size_t)p.dims.width * (size_t)p.dims.height;
    const uint32_t c0 = blockIdx.y * (uint32_t)K, nc = min((uint32_t)K, p.channels - c0);

    const uint2 range = p.ranges[tile];
    if (range.x >= range.y || range.y > p.num_rendered) return;        // no list (or not one of this call's R entries)

    uint32_t last[4];
    float T[4], fy[4], g[4][K];
    [[maybe_unused]] float S[4];
    uint32_t hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = py0 + 4 * k;
        fy[k] = (float)py;
        const bool inside = px < p.dims.width && py < p.dims.height;
        last[k] = 0; T[k] = 1.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) g[k][c] = 0.0f;
        if (inside) {
            const size_t pid = (size_t)py * (size_t)p.dims.width + (size_t)px;
            last[k] = p.n_contrib[pid];
            T[k] = p.final_t[pid];
#pragma unroll
            for (int c = 0; c < K; ++c)
                if ((uint32_t)c < nc) g[k][c] = p.dL_dout[(size_t)(c0 + (uint32_t)c) * plane + pid];
        }
        if constexpr (GEO) {
            // what lies behind, dotted with this chunk's dL/dout: S = T_f sum_c bg_c g_c
            float bgg = 0.0f;
            if (p.background) {
#pragma unroll
                for (int c = 0; c < K; ++c)
                    if ((uint32_t)c < nc) bgg = __builtin_fmaf(p.background[c0 + (uint32_t)c], g[k][c], bgg);
            }
            S[k] = T[k] * bgg;
        }
        hi = max(hi, last[k]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hi = max(hi, (uint32_t)__shfl_xor((int)hi, off, kWave));
    hi = min(hi, range.y - range.x);                                    // (a last contributor lies inside the list)
    if (hi == 0) return;
    const TileBox box = tile_box(tx, ty, p.dims.width, p.dims.height);

    // Which of a record's sums this lane files: wave_sum8 leaves value kSumOfRow[r] in lane 8 r; wave_sum4 value kSumOfRow4[r]
    // in every lane of row r (lane 16 r + 4 files it) — the geometry's slots are the render backward's (backward.hip).
    constexpr int kSumOfRow[8] = {0, 4, 2, 6, 1, 5, 3, 7};
    constexpr int kSumOfRow4[4] = {9, 11, 10, 12};
    const int my_feat = (lane & 7) == 0 ? kSumOfRow[lane >> 3] : -1;
    // (geometry: values 0..5 of the eight are slots 0..5, values 6 and 7 are unused; the four are slots 9..11 and one unused)
    const int my_geo = (lane & 7) == 0 ? (kSumOfRow[lane >> 3] < 6 ? kSumOfRow[lane >> 3] : -1)
                                       : ((lane & 15) == 4 && kSumOfRow4[lane >> 4] < 12 ? kSumOfRow4[lane >> 4] : -1);

    auto walk_batch = [&](const bool present, const uint32_t id, const uint32_t idx_l, const float2 xy_l, const float4 co_l) {
        const bool keep = present && !record_misses_tile(xy_l, co_l, box);
        const unsigned long long kept_mask = __ballot(keep);
        if (keep) {
            const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept_mask, 0u));
            s_id[slot] = id;
            s_idx[slot] = idx_l;
            s_xy[slot] = xy_l;
            s_co[slot] = co_l;
            // (without GEO the features themselves are not needed: dL_dfeatures is sum w g)
            if constexpr (GEO) stage_feature_row<K>(&s_feat[slot * K], p.features + (size_t)id * (size_t)p.channels + c0, nc);
            // the alpha floor: a pixel can pass alpha >= 1/255 only where power >= -ln(255 opacity), less a margin (backward.hip)
            const float op = co_l.w;
            s_floor[slot] = !(op > -__builtin_inff()) ? -__builtin_inff() : (op <= 0.0f ? __builtin_inff() : -__logf(255.0f * op) - 1e-3f);
        }
        // wave-private LDS: the writes above and the reads below are ordered inside the wave
        for (int j = (int)__popcll(kept_mask) - 1; j >= 0; --j) {
            const uint32_t idx0 = s_idx[j];                      // 0-based position in the tile's list
            const float2 xy = s_xy[j];
            const float4 co = s_co[j];
            const float dx = xy.x - fx;
            float a_f[K];
            [[maybe_unused]] float feat[K];
#pragma unroll
            for (int c = 0; c < K; ++c) a_f[c] = 0.0f;
            if constexpr (GEO) {
#pragma unroll
                for (int c = 0; c < K; c += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(&s_feat[j * K + c]);
                    feat[c] = v.x; feat[c + 1] = v.y; feat[c + 2] = v.z; feat[c + 3] = v.w;
                }
            }
            [[maybe_unused]] float a_mx = 0.0f, a_my = 0.0f, a_A = 0.0f, a_B = 0.0f, a_C = 0.0f, a_op = 0.0f;
            [[maybe_unused]] float a_m00 = 0.0f, a_m01 = 0.0f, a_m11 = 0.0f;
            bool any = false;
            const float hxx = -0.5f * dx * dx, flo = s_floor[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long inlist = __ballot(idx0 < last[k]);      // else: behind this pixel's last contributor
                if (inlist == 0ull) continue;
                const float dy = xy.y - fy[k];
                const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
                const unsigned long long cand = inlist & ~__ballot(power > 0.0f) & __ballot(power >= flo);
                if (cand == 0ull) continue;
                const float G = exp_ref(power, s_exp);           // the forward's exp: same contributing set
                const float raw = co.w * G;
                const float alpha = fminf(0.99f, raw);
                const unsigned long long act_mask = cand & ~__ballot(alpha < 1.0f / 255.0f);
                if (act_mask == 0ull) continue;
                const bool act = __builtin_amdgcn_inverse_ballot_w64(act_mask);
                any = true;
                const float inv = __builtin_amdgcn_rcpf(1.0f - alpha);
                const float Tn = T[k] * inv;                     // transmittance in front of this record
                T[k] = act ? Tn : T[k];
                const float w = act ? alpha * Tn : 0.0f;
#pragma unroll
                for (int c = 0; c < K; ++c) a_f[c] = __builtin_fmaf(w, g[k][c], a_f[c]);
                if constexpr (GEO) {
                    float cg = feat[K - 1] * g[k][K - 1];
#pragma unroll
                    for (int c = K - 2; c >= 0; --c) cg = __builtin_fmaf(feat[c], g[k][c], cg);
                    // from here to the sums: render_backward_kernel's lines (backward.hip)
                    const float dL_dalpha = __builtin_fmaf(Tn, cg, -(S[k] * inv));
                    S[k] = __builtin_fmaf(cg, w, S[k]);
                    const bool live = __builtin_amdgcn_inverse_ballot_w64(act_mask & ~__ballot(raw > 0.99f));   // clamped: alpha does not move with the parameters
                    const float gop = live ? G * dL_dalpha : 0.0f;
                    const float dpow = live ? raw * dL_dalpha : 0.0f;
                    a_op += gop;
                    a_A = __builtin_fmaf(hxx, dpow, a_A);
                    a_B = __builtin_fmaf(-(dx * dy), dpow, a_B);
                    a_C = __builtin_fmaf(-0.5f * dy * dy, dpow, a_C);
                    const float ux = __builtin_fmaf(co.x, dx, co.y * dy), uy = __builtin_fmaf(co.y, dx, co.z * dy);
                    a_mx = __builtin_fmaf(-ux, dpow, a_mx);
                    a_my = __builtin_fmaf(-uy, dpow, a_my);
                    const float hux = 0.5f * dpow * ux, huy = 0.5f * dpow * uy;      // (the masked factor first: 0 x finite)
                    a_m00 = __builtin_fmaf(hux, ux, a_m00); a_m01 = __builtin_fmaf(hux, uy, a_m01); a_m11 = __builtin_fmaf(huy, uy, a_m11);
                }
            }
            if (!any) continue;
            const size_t id = s_id[j];
            // eight channels per reduction, one atomic instruction with eight lanes on 64 contiguous bytes
#pragma unroll
            for (int c = 0; c < K; c += 8) {
                const float total = wave_sum8(a_f[c], a_f[c + 1], a_f[c + 2], a_f[c + 3], a_f[c + 4], a_f[c + 5], a_f[c + 6], a_f[c + 7], lane);
                if (my_feat >= 0 && (uint32_t)(c + my_feat) < nc && total != 0.0f)
                    unsafeAtomicAdd(p.feature_sums + id * (size_t)p.channels + c0 + (uint32_t)(c + my_feat), (double)total);
            }
            if constexpr (GEO) {
                const float t8 = wave_sum8(a_mx, a_my, a_A, a_B, a_C, a_op, 0.0f, 0.0f, lane);
                const float t4 = wave_sum4(a_m00, a_m01, a_m11, 0.0f);
                const float total = (lane & 7) == 4 ? t4 : t8;
                if (my_geo >= 0 && total != 0.0f) unsafeAtomicAdd(p.geometry_sums + kGeoFloats * id + (uint32_t)my_geo, (double)total);
            }
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
        nb.id = p.point_list[range.x + (nb.present ? nb.idx_l : 0u)];
        nb.present = nb.present && nb.id < p.num_gaussians;       // (an entry that names no Gaussian of the scene is dropped)
        return nb;
    };
    auto fetch = [&](Batch& nb) {
        const uint32_t at = (nb.valid && nb.present) ? nb.id : 0u;
        nb.xy = p.means2D[at];
        nb.co = p.conic_opacity[at];
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

// Rounds every sum once, writes the output in full and leaves the scratch zero (most rows received nothing: no write for those).
__global__ __launch_bounds__(256) void features_finish_kernel(size_t count, double* __restrict__ sums, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double v = sums[i];
    out[i] = (float)v;
    if (v != 0.0) sums[i] = 0.0;
}

// What both calls check, in the header's order; *nothing: no record to walk (R == 0 or an empty band).
int features_check(gsr_features_args* a, bool backward, FrameDims* d, bool* nothing) {
    if (!a || a->struct_size != sizeof(gsr_features_args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    if (a->num_gaussians <= 0 || a->width <= 0 || a->height <= 0) return GSR_ERR_INVALID_ARG;
    if (a->channels < 1 || a->channels > GSR_FEATURES_MAX_CHANNELS) return GSR_ERR_INVALID_ARG;
    if (!a->means2D || !a->conic_opacity || !a->ranges || !a->n_contrib || !a->final_t || !a->features) return GSR_ERR_INVALID_ARG;
    if (backward ? (!a->dL_dout || !a->dL_dfeatures || !a->feature_sums_f64) : !a->out) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->means2D, 8) || misaligned(a->conic_opacity, 16) || misaligned(a->ranges, 8)) return GSR_ERR_INVALID_ARG;
    if (backward && (misaligned(a->feature_sums_f64, 8) || misaligned(a->geometry_sums_f64, 8))) return GSR_ERR_INVALID_ARG;
    const gsr_forward_receipt& r = a->receipt;
    if (r.magic != GSR_RECEIPT_MAGIC) return GSR_ERR_INVALID_ARG;
    if (tile_band(a->width, a->height, a->tile_row_begin, a->tile_row_end, d) != GSR_OK) return GSR_ERR_INVALID_ARG;
    BlockFeed block_lists;
    bool from_blocks = false, lists_written = true;
    GSR_TRY(lists_of_receipt(r, a->num_gaussians, a->width, a->height, d->row_begin, d->row_end, a->point_list, &block_lists, &from_blocks,
                             &lists_written));
    *nothing = r.num_rendered == 0 || d->row_begin == d->row_end;
    if (!*nothing && (!lists_written || !a->point_list)) return GSR_ERR_INVALID_ARG;      // (no walk through the block lists here)
    return GSR_OK;
}

FeatureParams feature_params(const gsr_features_args* a, const FrameDims& d) {
    FeatureParams p;
    p.ranges = reinterpret_cast<const uint2*>(a->ranges);
    p.point_list = a->point_list;
    p.means2D = reinterpret_cast<const float2*>(a->means2D);
    p.conic_opacity = reinterpret_cast<const float4*>(a->conic_opacity);
    p.n_contrib = a->n_contrib;
    p.final_t = a->final_t;
    p.features = a->features;
    p.background = a->background;
    p.out = a->out;
    p.dL_dout = a->dL_dout;
    p.feature_sums = a->feature_sums_f64;
    p.geometry_sums = a->geometry_sums_f64;
    p.dims = d;
    p.tile_order = nullptr;
    p.num_gaussians = (uint32_t)a->num_gaussians;
    p.num_rendered = a->receipt.num_rendered;
    p.channels = (uint32_t)a->channels;
    return p;
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

int features_forward_impl(gsr_features_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(features_check(a, false, &d, &nothing));
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (d.row_begin != d.row_end) {          // (R == 0: every tile of the band is a tile without a list)
        const FeatureParams p = feature_params(a, d);
        const int k = chunk_of(a->channels);
        const dim3 grid((unsigned)blocks, (unsigned)((a->channels + k - 1) / k));
        if (k == kChunkNarrow) hipLaunchKernelGGL(features_forward_kernel<kChunkNarrow>, grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL(features_forward_kernel<kChunkWide>, grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("features_forward_kernel");
    }
    return timer.end(stream, &a->stage_ms);
}

int features_backward_impl(gsr_features_args* a) {
    FrameDims d;
    bool nothing = false;
    GSR_TRY(features_check(a, true, &d, &nothing));
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    const size_t count = (size_t)a->num_gaussians * (size_t)a->channels;
    const long long finish_blocks = (long long)((count + 255) / 256);
    if (exceeds_grid(blocks) || exceeds_grid(finish_blocks)) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----
    hipStream_t stream = static_cast<hipStream_t>(a->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (!nothing) {
        FeatureParams p = feature_params(a, d);
        // (the tiles that were slow in the forward blend are the slow ones here: they go first, as they did there)
        p.tile_order = tile_order_of_call(a->receipt, d.row_begin, d.row_end);
        const int k = chunk_of(a->channels);
        const bool narrow = k == kChunkNarrow, geo = a->geometry_sums_f64 != nullptr;
        const dim3 grid((unsigned)blocks, (unsigned)((a->channels + k - 1) / k));
        if (narrow && geo) hipLaunchKernelGGL((features_backward_kernel<kChunkNarrow, true>), grid, dim3(kWave), 0, stream, p);
        else if (narrow) hipLaunchKernelGGL((features_backward_kernel<kChunkNarrow, false>), grid, dim3(kWave), 0, stream, p);
        else if (geo) hipLaunchKernelGGL((features_backward_kernel<kChunkWide, true>), grid, dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL((features_backward_kernel<kChunkWide, false>), grid, dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("features_backward_kernel");
    }
    hipLaunchKernelGGL(features_finish_kernel, dim3((unsigned)finish_blocks), dim3(256), 0, stream, count, a->feature_sums_f64, a->dL_dfeatures);
    GSR_LAUNCH_CHECK("features_finish_kernel");
    return timer.end(stream, &a->stage_ms);
}

}  // namespace
}  // namespace gsr

extern "C" size_t gsr_features_temp_bytes(int32_t num_gaussians, int32_t channels) {
    if (num_gaussians <= 0 || channels < 1 || channels > GSR_FEATURES_MAX_CHANNELS) return 0;
    return sizeof(double) * (size_t)num_gaussians * (size_t)channels;
}
extern "C" int gsr_features_forward(gsr_features_args* a) { return gsr::entry_point(gsr::features_forward_impl, a); }
extern "C" int gsr_features_backward(gsr_features_args* a) { return gsr::entry_point(gsr::features_backward_impl, a); }
