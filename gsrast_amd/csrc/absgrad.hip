// The absolute screen-space gradient of a frame (AbsGS; include/gsrast_amd_absgrad.h): per Gaussian, the sum over pixels of the
// ABSOLUTE value of each pixel's share of dL/d means2D, per axis — what the render backward's signed sums cannot give back.
//
// absgrad_kernel is the walk of render_backward_kernel (backward.hip) with ten of its twelve accumulators removed, as a pass of
// its own so that the kernel every training step times keeps its object code. The skeleton is DUPLICATED here on purpose, and
// these parts are deliberately the same as in backward.hip — change one and the two no longer describe the same pixels:
//   - one wavefront per 16 x 16 tile, four pixels per lane (x = lane & 15, y = (lane >> 4) + 4 k), tiles dealt in XCD patches and
//     taken in the forward blend's order (tile_order_of_call);
//   - every pixel starts at its own last contributor (n_contrib) with T = final_t and S = T ((bg . g) [- g_a]), and the batches of
//     64 list entries come back to front, ids two batches ahead, records one batch ahead;
//   - a batch is compacted by record_misses_tile, one lane per record; the record's floor -ln(255 o) - 1e-3 skips strips it is too
//     faint for before the exponential; power in the forward's operation order, exp_ref, alpha >= 1/255: the forward's set;
//   - T_i = T_{i+1} * rcp(1 - alpha), cg and dL_dalpha by fused multiply-adds, raw > 0.99 zeroes the share but not the walk;
//   - u = K d by the same two multiply-adds.
// What differs: only the sorted lists are read (point_list, as gsr_contribution does: no block feed, no per-entry sums); the two
// values a record keeps are sums of |u dpow|; they are reduced with one lane swap and five DPP steps and leave as one double
// atomic instruction with two lanes; list entries are bounded by the receipt's R and the scene's N before they index anything.
#include <hip/hip_runtime.h>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "blend_core.hpp"           // (and, through gsr_common.hpp, frame_policy.hpp: tile_band)
#include "blockbin.hpp"             // (lists_of_receipt, tile_order_of_call)
#include "../../include/gsrast_amd_absgrad.h"

namespace gsr {
namespace {

struct AbsgradParams {
    const uint2* ranges;
    const uint32_t* point_list;
    const float2* means2D;
    const float* colors;
    const float4* conic_opacity;
    const float* final_t;
    const uint32_t* n_contrib;
    const float* background;
    const float* dL_dout;
    const float* dL_dout_depth;   // f32[W H] (DEPTH instance only)
    const float* dL_dout_alpha;   // f32[W H] or null
    const float4* means3D;        // (DEPTH)
    const float* view;            // (DEPTH: row 2 is read)
    uint32_t depth_inverse;
    double* sums;                 // f64[2 N]
    FrameDims dims;
    const uint32_t* tile_order;   // the forward blend's workgroup order, or null: patch order
    uint32_t num_gaussians;
    uint32_t num_rendered;
};

// Sums of TWO per-lane values over the 64 lanes: v_permlane32_swap folds the halves while laying the values side by side (rows
// 0, 1: x, rows 2, 3: y), then the row shifts and the row broadcast of blockbin.hpp's prefix32_inclusive (lanes without a source
// read 0). On return lane 31 holds the total of x and lane 63 that of y; the other lanes hold partial sums.
__device__ __forceinline__ float wave_sum2(float x, float y) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    float v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
#define GSR_DPP0(v, ctrl, rows) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rows, 0xf, false))
    v += GSR_DPP0(v, 0x111, 0xf);
    v += GSR_DPP0(v, 0x112, 0xf);
    v += GSR_DPP0(v, 0x114, 0xf);
    v += GSR_DPP0(v, 0x118, 0xf);
    v += GSR_DPP0(v, 0x142, 0xa);      // row_bcast:15 into rows 1 and 3
#undef GSR_DPP0
    return v;
}

template <bool DEPTH> struct AbsDepthSlots { __device__ static float* get() { return nullptr; } };
template <> struct AbsDepthSlots<true> {
    __device__ static float* get() {
        __shared__ float s_dep[kWave];
        return s_dep;
    }
};

template <bool DEPTH>
__global__ __launch_bounds__(64) void absgrad_kernel(const AbsgradParams p) {
    float* const s_dep = AbsDepthSlots<DEPTH>::get();
    __shared__ uint32_t s_id[kWave];
    __shared__ float2 s_xy[kWave];
    __shared__ float4 s_co[kWave];
    __shared__ float4 s_rgb[kWave];
    __shared__ float s_floor[kWave];
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
    const float bg0 = p.background[0], bg1 = p.background[1], bg2 = p.background[2];

    uint32_t last[4];
    float T[4], S[4], g0[4], g1[4], g2[4], fy[4];
    float gd[4] = {0.0f, 0.0f, 0.0f, 0.0f};         // dL/d out_depth (DEPTH)
    uint32_t hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = py0 + 4 * k;
        fy[k] = (float)py;
        const bool inside = px < p.dims.width && py < p.dims.height;
        last[k] = 0; T[k] = 1.0f; g0[k] = g1[k] = g2[k] = 0.0f;
        float ga = 0.0f;                             // dL/d out_alpha
        if (inside) {
            const size_t pid = (size_t)py * (size_t)p.dims.width + (size_t)px;
            last[k] = p.n_contrib[pid];
            T[k] = p.final_t[pid];
            g0[k] = p.dL_dout[pid]; g1[k] = p.dL_dout[pid + plane]; g2[k] = p.dL_dout[pid + 2 * plane];
            if constexpr (DEPTH) gd[k] = p.dL_dout_depth[pid];
            if (p.dL_dout_alpha) ga = p.dL_dout_alpha[pid];
        }
        // what lies behind, dotted with dL/dC; the accumulated opacity's whole term is this seed (x - 0 is x: one expression)
        S[k] = T[k] * ((bg0 * g0[k] + bg1 * g1[k] + bg2 * g2[k]) - ga);
        hi = max(hi, last[k]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hi = max(hi, (uint32_t)__shfl_xor((int)hi, off, kWave));
    const uint2 range = p.ranges[tile];
    if (range.x >= range.y || range.y > p.num_rendered) return;        // no list (or not one of this call's R entries)
    hi = min(hi, range.y - range.x);                                    // (a last contributor lies inside the list)
    if (hi == 0) return;
    const TileBox box = tile_box(tx, ty, p.dims.width, p.dims.height);

    auto walk_batch = [&](const bool present, const uint32_t id, const uint32_t idx_l, const float2 xy_l, const float4 co_l) {
        const bool keep = present && !record_misses_tile(xy_l, co_l, box);
        const unsigned long long kept_mask = __ballot(keep);
        if (keep) {
            const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept_mask, 0u));
            s_id[slot] = id;
            s_xy[slot] = xy_l;
            s_co[slot] = co_l;
            const float* col = p.colors + 3 * (size_t)id;
            s_rgb[slot] = make_float4(col[0], col[1], col[2], __uint_as_float(idx_l));
            if constexpr (DEPTH) {
                // d_i as the forward blend computed it (blend_core.hpp: depth_value)
                const float4 m = p.means3D[id];
                const float z = (p.view[2] * m.x + p.view[6] * m.y) + (p.view[10] * m.z + p.view[14] * 1.0f);
                s_dep[slot] = p.depth_inverse ? 1.0f / z : z;
            }
            // the alpha floor: a pixel can pass alpha >= 1/255 only where power >= -ln(255 opacity), less a margin (backward.hip)
            const float op = co_l.w;
            s_floor[slot] = !(op > -__builtin_inff()) ? -__builtin_inff() : (op <= 0.0f ? __builtin_inff() : -__logf(255.0f * op) - 1e-3f);
        }
        // wave-private LDS: the writes above and the reads below are ordered inside the wave
        for (int j = (int)__popcll(kept_mask) - 1; j >= 0; --j) {
            const float4 col = s_rgb[j];
            const uint32_t idx0 = __float_as_uint(col.w);        // 0-based position in the tile's list
            const float2 xy = s_xy[j];
            const float4 co = s_co[j];
            const float dx = xy.x - fx;
            float a_x = 0.0f, a_y = 0.0f;                        // this lane's four pixels: sums of |share|
            float dep = 0.0f;
            if constexpr (DEPTH) dep = s_dep[j];
            bool any = false;
            const float flo = s_floor[j];
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
                float cg = __builtin_fmaf(col.x, g0[k], __builtin_fmaf(col.y, g1[k], col.z * g2[k]));
                if constexpr (DEPTH) cg = __builtin_fmaf(dep, gd[k], cg);
                const float w = act ? alpha * Tn : 0.0f;
                const float dL_dalpha = __builtin_fmaf(Tn, cg, -(S[k] * inv));
                S[k] = __builtin_fmaf(cg, w, S[k]);
                const bool live = __builtin_amdgcn_inverse_ballot_w64(act_mask & ~__ballot(raw > 0.99f));   // clamped: alpha does not move
                const float dpow = live ? raw * dL_dalpha : 0.0f;
                const float ux = __builtin_fmaf(co.x, dx, co.y * dy), uy = __builtin_fmaf(co.y, dx, co.z * dy);
                // (a lane that is not live: |u| x 0 — u is finite wherever the power was)
                a_x += fabsf(ux * dpow);
                a_y += fabsf(uy * dpow);
            }
            if (!any) continue;
            const float total = wave_sum2(a_x, a_y);
            if ((lane & 31) == 31 && total != 0.0f)              // lane 31: x, lane 63: y — one instruction, two addresses side by side
                unsafeAtomicAdd(p.sums + 2 * (size_t)s_id[j] + (size_t)(lane >> 5), (double)total);
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

// Rounds every pair once, writes the output in full and leaves the scratch zero (most rows received nothing: no write for those).
// (the scratch is only known to lie on an 8-byte boundary: two doubles, not a double2)
__global__ __launch_bounds__(256) void absgrad_finish_kernel(int n, double* __restrict__ sums, float2* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double sx = sums[2 * (size_t)i], sy = sums[2 * (size_t)i + 1];
    out[i] = make_float2((float)sx, (float)sy);
    if (sx != 0.0) sums[2 * (size_t)i] = 0.0;
    if (sy != 0.0) sums[2 * (size_t)i + 1] = 0.0;
}

int absgrad_impl(gsr_absgrad_args* a) {
    if (!a || a->struct_size != sizeof(gsr_absgrad_args)) return GSR_ERR_INVALID_ARG;
    a->stage_ms = 0.0f;
    const gsr_backward_args* const b = a->backward;
    if (!b || b->struct_size != sizeof(gsr_backward_args)) return GSR_ERR_INVALID_ARG;
    if (b->num_gaussians <= 0 || b->width <= 0 || b->height <= 0 || !b->background || !b->means2D || !b->conic_opacity || !b->colors ||
        !b->ranges || !b->n_contrib || !b->final_t || !b->dL_dout_color)
        return GSR_ERR_INVALID_ARG;
    const bool depth = b->dL_dout_depth != nullptr;
    if (depth && (!b->means3D || !b->view_matrix)) return GSR_ERR_INVALID_ARG;
    if (!a->abs_dL_dmean2D || !a->sums_f64 || misaligned(a->sums_f64, 8) || misaligned(a->abs_dL_dmean2D, 8)) return GSR_ERR_INVALID_ARG;
    if (misaligned(b->means2D, 8) || misaligned(b->conic_opacity, 16) || misaligned(b->ranges, 8) || (depth && misaligned(b->means3D, 16)))
        return GSR_ERR_INVALID_ARG;
    FrameDims d;
    if (tile_band(b->width, b->height, b->tile_row_begin, b->tile_row_end, &d) != GSR_OK) return GSR_ERR_INVALID_ARG;
    const gsr_forward_receipt& r = b->receipt;
    BlockFeed block_lists;
    bool from_blocks = false, lists_written = true;
    GSR_TRY(lists_of_receipt(r, b->num_gaussians, b->width, b->height, d.row_begin, d.row_end, b->point_list, &block_lists, &from_blocks,
                             &lists_written));
    const bool nothing = r.num_rendered == 0 || d.row_begin == d.row_end;
    if (!nothing && (!lists_written || !b->point_list)) return GSR_ERR_INVALID_ARG;      // (no walk through the block lists here)
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----

    hipStream_t stream = static_cast<hipStream_t>(b->stream);
    const bool profile = (a->flags & GSR_FLAG_PROFILE) != 0;
    CallEvents<2> events;
    if (profile) {
        GSR_TRY(events.create());
        GSR_HIP_TRY(hipEventRecord(events.ev[0], stream));
    }
    if (!nothing) {
        AbsgradParams p;
        p.ranges = reinterpret_cast<const uint2*>(b->ranges);
        p.point_list = b->point_list;
        p.means2D = reinterpret_cast<const float2*>(b->means2D);
        p.colors = b->colors;
        p.conic_opacity = reinterpret_cast<const float4*>(b->conic_opacity);
        p.final_t = b->final_t;
        p.n_contrib = b->n_contrib;
        p.background = b->background;
        p.dL_dout = b->dL_dout_color;
        p.dL_dout_depth = b->dL_dout_depth;
        p.dL_dout_alpha = a->dL_dout_alpha;
        p.means3D = reinterpret_cast<const float4*>(b->means3D);
        p.view = b->view_matrix;
        p.depth_inverse = (a->flags & GSR_FLAG_DEPTH_INVERSE) ? 1u : 0u;
        p.sums = a->sums_f64;
        p.dims = d;
        // (the tiles that were slow in the forward blend are the slow ones here: they go first, as they did there)
        p.tile_order = tile_order_of_call(r, d.row_begin, d.row_end);
        p.num_gaussians = (uint32_t)b->num_gaussians;
        p.num_rendered = r.num_rendered;
        if (depth) hipLaunchKernelGGL(absgrad_kernel<true>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL(absgrad_kernel<false>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("absgrad_kernel");
    }
    hipLaunchKernelGGL(absgrad_finish_kernel, dim3((unsigned)((b->num_gaussians + 255) / 256)), dim3(256), 0, stream, b->num_gaussians,
                       a->sums_f64, reinterpret_cast<float2*>(a->abs_dL_dmean2D));
    GSR_LAUNCH_CHECK("absgrad_finish_kernel");
    if (profile) {
        GSR_HIP_TRY(hipEventRecord(events.ev[1], stream));
        GSR_HIP_TRY(hipEventSynchronize(events.ev[1]));
        GSR_HIP_TRY(hipEventElapsedTime(&a->stage_ms, events.ev[0], events.ev[1]));
    }
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

extern "C" int gsr_absgrad(gsr_absgrad_args* a) { return gsr::entry_point(gsr::absgrad_impl, a); }
