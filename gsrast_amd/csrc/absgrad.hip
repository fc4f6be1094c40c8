// The absolute screen-space gradient of a frame (AbsGS; include/gsrast_amd_absgrad.h): per Gaussian, the sum over pixels of the
// ABSOLUTE value of each pixel's share of dL/d means2D, per axis — what the render backward's signed sums cannot give back.
//
// absgrad_kernel is the back walk of list_walk.hpp (render_backward_kernel's, restated there) with ten of the render backward's
// twelve accumulators removed, as a pass of its own so that the kernel every training step times keeps its object code. Its own
// part: S = T ((bg . g) [- g_a]) behind every pixel, cg and dL_dalpha by the render backward's fused multiply-adds (the depth
// slot d_i beside the colour), and the two values a record keeps, sums of |u dpow|: they are reduced with one lane swap and
// five DPP steps and leave as one double atomic instruction with two lanes. Only the sorted lists are read (point_list, as
// gsr_contribution does: no block feed, no per-entry sums).
#include <hip/hip_runtime.h>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "list_walk.hpp"
#include "../../include/gsrast_amd_absgrad.h"

namespace gsr {
namespace {

struct AbsgradParams {
    WalkFrame frame;
    const float* colors;
    const float* background;
    const float* dL_dout;
    const float* dL_dout_depth;   // f32[W H] (DEPTH instance only)
    const float* dL_dout_alpha;   // f32[W H] or null
    const float4* means3D;        // (DEPTH)
    const float* view;            // (DEPTH: row 2 is read)
    uint32_t depth_inverse;
    double* sums;                 // f64[2 N]
};

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
    __shared__ BackStage st;
    __shared__ float4 s_rgb[kWave];
    const int lane = threadIdx.x;
    int tx, ty;
    const int tile = walk_tile(p.frame, &tx, &ty);
    if (tile < 0) return;
    const size_t plane = (size_t)p.frame.dims.width * (size_t)p.frame.dims.height;
    const float bg0 = p.background[0], bg1 = p.background[1], bg2 = p.background[2];

    BackLanes s;
    float S[4], g0[4] = {}, g1[4] = {}, g2[4] = {};
    float gd[4] = {}, ga[4] = {};                    // dL/d out_depth (DEPTH), dL/d out_alpha
    float4 col;                                      // the record in hand: its colour, d_i, and this lane's sums of |share|
    float dep = 0.0f, a_x = 0.0f, a_y = 0.0f;
    back_walk<false>(
        p.frame, tile, tx, ty, lane, s, st,
        /* seed */ [&](const int k, const size_t pid) {
            g0[k] = p.dL_dout[pid]; g1[k] = p.dL_dout[pid + plane]; g2[k] = p.dL_dout[pid + 2 * plane];
            if constexpr (DEPTH) gd[k] = p.dL_dout_depth[pid];
            if (p.dL_dout_alpha) ga[k] = p.dL_dout_alpha[pid];
        },
        /* start */ [&]() {
            // what lies behind, dotted with dL/dC; the accumulated opacity's whole term is this seed (x - 0 is x: one expression)
#pragma unroll
            for (int k = 0; k < 4; ++k) S[k] = s.T[k] * ((bg0 * g0[k] + bg1 * g1[k] + bg2 * g2[k]) - ga[k]);
        },
        /* payload */ [&](const uint32_t slot, const uint32_t id) {
            const float* c = p.colors + 3 * (size_t)id;
            // (.w is idle: the list position has the walk's own slot — 256 bytes of LDS more than packing it here, in a kernel
            // whose occupancy the registers bound; one 16-byte write and read per record either way)
            s_rgb[slot] = make_float4(c[0], c[1], c[2], 0.0f);
            if constexpr (DEPTH) {
                // d_i as the forward blend computed it (blend_core.hpp: depth_value)
                const float4 m = p.means3D[id];
                const float z = (p.view[2] * m.x + p.view[6] * m.y) + (p.view[10] * m.z + p.view[14] * 1.0f);
                s_dep[slot] = p.depth_inverse ? 1.0f / z : z;
            }
        },
        /* begin */ [&](const int j) {
            col = s_rgb[j];
            if constexpr (DEPTH) dep = s_dep[j];
            a_x = 0.0f; a_y = 0.0f;
        },
        /* on_pixel */ [&](const int k, const BackPixel& px) {
            float cg = __builtin_fmaf(col.x, g0[k], __builtin_fmaf(col.y, g1[k], col.z * g2[k]));
            if constexpr (DEPTH) cg = __builtin_fmaf(dep, gd[k], cg);
            const float dL_dalpha = __builtin_fmaf(px.Tn, cg, -(S[k] * px.inv));
            S[k] = __builtin_fmaf(cg, px.w, S[k]);
            const float dpow = px.live() ? px.raw * dL_dalpha : 0.0f;
            // (a lane that is not live: |u| x 0 — u is finite wherever the power was)
            a_x += fabsf(px.ux() * dpow);
            a_y += fabsf(px.uy() * dpow);
        },
        /* file */ [&](const int j) {
            const float total = wave_sum2(a_x, a_y);
            if ((lane & 31) == 31 && total != 0.0f)              // lane 31: x, lane 63: y — one instruction, two addresses side by side
                unsafeAtomicAdd(p.sums + 2 * (size_t)st.id[j] + (size_t)(lane >> 5), (double)total);
        });
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
    const gsr_forward_receipt& r = b->receipt;
    FrameDims d;
    bool nothing = false;
    GSR_TRY(walk_check(r, b->num_gaussians, b->width, b->height, b->tile_row_begin, b->tile_row_end, false, b->point_list, &d, &nothing));
    const long long blocks = patch_workgroups(d.grid_x, d.row_end - d.row_begin);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    // ---- nothing is refused from here on ----

    hipStream_t stream = static_cast<hipStream_t>(b->stream);
    StageTimer timer;
    GSR_TRY(timer.begin((a->flags & GSR_FLAG_PROFILE) != 0, stream));
    if (!nothing) {
        AbsgradParams p;
        p.frame = walk_frame(b->ranges, b->point_list, b->means2D, b->conic_opacity, b->n_contrib, b->final_t, d, b->num_gaussians, r.num_rendered);
        // (the tiles that were slow in the forward blend are the slow ones here: they go first, as they did there)
        p.frame.tile_order = tile_order_of_call(r, d.row_begin, d.row_end);
        p.colors = b->colors;
        p.background = b->background;
        p.dL_dout = b->dL_dout_color;
        p.dL_dout_depth = b->dL_dout_depth;
        p.dL_dout_alpha = a->dL_dout_alpha;
        p.means3D = reinterpret_cast<const float4*>(b->means3D);
        p.view = b->view_matrix;
        p.depth_inverse = (a->flags & GSR_FLAG_DEPTH_INVERSE) ? 1u : 0u;
        p.sums = a->sums_f64;
        if (depth) hipLaunchKernelGGL(absgrad_kernel<true>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
        else hipLaunchKernelGGL(absgrad_kernel<false>, dim3((unsigned)blocks), dim3(kWave), 0, stream, p);
        GSR_LAUNCH_CHECK("absgrad_kernel");
    }
    GSR_TRY(launch_finish_sums<2>((size_t)b->num_gaussians, a->sums_f64, a->abs_dL_dmean2D, stream));
    return timer.end(stream, &a->stage_ms);
}

}  // namespace
}  // namespace gsr

extern "C" int gsr_absgrad(gsr_absgrad_args* a) { return gsr::entry_point(gsr::absgrad_impl, a); }
