// Per-Gaussian preprocess: cull, 3D covariance, EWA 2D covariance, conic, screen rect,
// DC colour, depth, tiles touched. One lane per Gaussian, streaming (HBM-bound).
//
// Follows the semantics of reference apps/gsrast/gscuda/GSCuda.cu:261-375
// (preprocessCUDA) with helpers :157-162 (quatToMat), :168-195 (computeCov3D),
// :197-231 (computeCov2D), :237-259 (getRect). Arithmetic keeps the reference's
// float32 operation order (this file is compiled with -ffp-contract=off), including
// the double intermediates of quatToMat, so every integer output (radii, rects,
// tilesTouched) is reproducible bit for bit.
#include "preprocess_common.hpp"

namespace gsr {
namespace {

__device__ __forceinline__ float4 mat4_vec4(const float* __restrict__ m, float x, float y, float z, float w) {
    float4 o;
    o.x = (m[0] * x + m[4] * y) + (m[8] * z + m[12] * w);
    o.y = (m[1] * x + m[5] * y) + (m[9] * z + m[13] * w);
    o.z = (m[2] * x + m[6] * y) + (m[10] * z + m[14] * w);
    o.w = (m[3] * x + m[7] * y) + (m[11] * z + m[15] * w);
    return o;
}

struct PreprocessParams {
    int n;
    const float4* means3D;
    const float4* scales;
    float scale_modifier;
    const float4* rotations;
    const float* opacities;
    const float* shs;
    const float* cov3D_precomp;
    const float* colors_precomp;
    bool skip_colors;           // colours given (colors_precomp) or computed by colors_visible_kernel beside the depth sort
    const float* view;
    const float* proj;
    float tan_fovx, tan_fovy, focal;
    int32_t* radii;
    float2* means2D;
    float* depths;
    float* cov3Ds;
    float* rgb;
    float4* conic_opacity;
    uint32_t* tiles_touched;
    uint32_t* depth_keys;          // depth bits of Gaussians with >= 1 tile in this call, else ~0
    uint32_t* rect_packed;         // x0 | w << 8 | y0 << 16 | h << 24 of the band-clipped rectangle (grids <= 255), else 0
    uint4* wave_sums;              // per 64 Gaussians: what the scan wants to know of them (store_wave_sums; may be null)
    uint32_t big_from;
    int2* rects;
    FrameDims dims;
};

// Memory schedule of a wave: (1) the means, (2) scale and rotation of the lanes inside the frustum, (3) opacity and
// the DC triple of the lanes that turn out to have a tile, (4) all stores. Nothing is loaded after the first store:
// the compiler has to assume that a store may alias a later load (the pointers come in through a struct), which in
// the first version of this kernel serialised seven dependent round trips per wave (cov3D store -> view matrix
// reload -> ... -> sh[0] -> store -> sh[1] -> store -> sh[2] -> store -> opacity). Fetching (3) together with (2)
// was measured too (0.39 vs 0.35 ms): the frustum test is loose (1.3 x NDC), a third of the lanes that pass it have
// no tile, and their 128-byte DC lines cost more than the saved round trip.
__global__ __launch_bounds__(256) void preprocess_kernel(const PreprocessParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n) return;

    // The two matrices are wave-uniform: they come in through the scalar cache, once, before anything is stored.
    float view[16], proj[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { view[i] = p.view[i]; proj[i] = p.proj[i]; }

    int32_t out_radius = 0;
    uint32_t out_tiles = 0, out_rect = 0;

    // (the inputs are read once: streaming loads, ld4)
    const float4 mean = ld4(p.means3D + idx);
    const float4 ph = mat4_vec4(proj, mean.x, mean.y, mean.z, mean.w);
    const float one_over_w = 1.0f / (0.001f + ph.w);
    const float prx = one_over_w * ph.x, pry = one_over_w * ph.y, prz = one_over_w * ph.z;
    const bool in_frustum = !(prz < 0.0f || prz > 1.0f || prx < -1.3f || prx > 1.3f || pry < -1.3f || pry > 1.3f);
    // what the stores at the end write (zeros where the reference writes nothing: see there)
    float o_c3[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, o_rgb[3] = {0.0f, 0.0f, 0.0f}, o_pix = 0.0f, o_piy = 0.0f, o_depth = 0.0f;
    float o_co[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int o_ex = 0, o_ey = 0;
    if (in_frustum) {
        // ---- every remaining load of this Gaussian ----
        float c3[6];
        float4 sc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rot = sc;
        if (p.cov3D_precomp) {
            const float2* src = reinterpret_cast<const float2*>(p.cov3D_precomp + 6 * (size_t)idx);
            const float2 a = src[0], b = src[1], c = src[2];
            c3[0] = a.x; c3[1] = a.y; c3[2] = b.x; c3[3] = b.y; c3[4] = c.x; c3[5] = c.y;
        } else {
            sc = ld4(p.scales + idx);
            rot = ld4(p.rotations + idx);
        }
        if (!p.cov3D_precomp) {
            M3 s;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 3; ++r) s.m[c][r] = 0.0f;
            s.m[0][0] = p.scale_modifier * sc.x;
            s.m[1][1] = p.scale_modifier * sc.y;
            s.m[2][2] = p.scale_modifier * sc.z;
            const float dq = (rot.x * rot.x + rot.y * rot.y) + (rot.z * rot.z + rot.w * rot.w);
            const float inv = 1.0f / sqrtf(dq);
            const float x = rot.x * inv, y = rot.y * inv, z = rot.z * inv, w = rot.w * inv;
            M3 rm;
            rm.m[0][0] = (float)(2.0 * (double)(x * x + y * y) - 1.0);
            rm.m[0][1] = (float)(2.0 * (double)(y * z + x * w));
            rm.m[0][2] = (float)(2.0 * (double)(y * w - x * z));
            rm.m[1][0] = (float)(2.0 * (double)(y * z - x * w));
            rm.m[1][1] = (float)(2.0 * (double)(x * x + z * z) - 1.0);
            rm.m[1][2] = (float)(2.0 * (double)(z * w + x * y));
            rm.m[2][0] = (float)(2.0 * (double)(y * w + x * z));
            rm.m[2][1] = (float)(2.0 * (double)(z * w - x * y));
            rm.m[2][2] = (float)(2.0 * (double)(x * x + w * w) - 1.0);
            const M3 rs = mul3(rm, s);
            const M3 sigma = mul3(rs, transpose3(rs));
            c3[0] = sigma.m[0][0]; c3[1] = sigma.m[1][0]; c3[2] = sigma.m[2][0];
            c3[3] = sigma.m[1][1]; c3[4] = sigma.m[2][1]; c3[5] = sigma.m[2][2];
        }

        // EWA projection (computeCov2D)
        float4 t = mat4_vec4(view, mean.x, mean.y, mean.z, 1.0f);
        const float limx = 1.3f * p.tan_fovx, limy = 1.3f * p.tan_fovy;
        const float txtz = t.x / t.z, tytz = t.y / t.z;
        t.x = fminr(limx, fmaxr(-limx, txtz)) * t.z;
        t.y = fminr(limy, fmaxr(-limy, tytz)) * t.z;
        M3 j;
        j.m[0][0] = p.focal / t.z; j.m[0][1] = 0.0f; j.m[0][2] = (-p.focal * t.x) / (t.z * t.z);
        j.m[1][0] = 0.0f; j.m[1][1] = p.focal / t.z; j.m[1][2] = (-p.focal * t.y) / (t.z * t.z);
        j.m[2][0] = 0.0f; j.m[2][1] = 0.0f; j.m[2][2] = 0.0f;
        M3 wv;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) wv.m[c][r] = view[4 * r + c];
        const M3 tm = mul3(wv, j);
        M3 vrk;
        vrk.m[0][0] = c3[0]; vrk.m[0][1] = c3[1]; vrk.m[0][2] = c3[2];
        vrk.m[1][0] = c3[1]; vrk.m[1][1] = c3[3]; vrk.m[1][2] = c3[4];
        vrk.m[2][0] = c3[2]; vrk.m[2][1] = c3[4]; vrk.m[2][2] = c3[5];
        const M3 cv = mul3(mul3(transpose3(tm), vrk), tm);
        const float ca = cv.m[0][0] + 0.3f, cb = cv.m[0][1], cc = cv.m[1][1] + 0.3f;

        const float det = ca * cc - cb * cb;
        // The rectangle first: it decides whether the Gaussian is visible, and only a visible one needs its opacity
        // and DC triple (a 128-byte line each: they are not fetched for the Gaussians that end here).
        float det_inv = 0.0f, my_radius = 0.0f, pix = 0.0f, piy = 0.0f;
        int ex = 0, ey = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        uint32_t band_area = 0;
        if (det != 0.0f) {
            det_inv = 1.0f / det;
            const float mid = 0.5f * (ca + cc);
            const float root = sqrtf(fmaxr(0.1f, mid * mid - det));
            const float lambda1 = mid + root, lambda2 = mid - root;
            my_radius = ceilf(3.0f * sqrtf(fmaxr(lambda1, lambda2)));
            pix = (prx * 0.5f + 0.5f) * (float)p.dims.width;
            piy = (pry * 0.5f + 0.5f) * (float)p.dims.height;
            if (p.rects) {
                ex = (int)ceilf(3.0f * sqrtf(ca));
                ey = (int)ceilf(3.0f * cc);            // sic, reference GSCuda.cu:352
            } else {
                ex = ey = (int)my_radius;
            }
            tile_rect(pix, piy, ex, ey, p.dims, x0, y0, x1, y1);
            // Visibility (reference :356: rectangle area != 0) is decided on the rectangle clipped to this
            // call's tile-row band — the whole grid when the call is not sharded, which is then exactly
            // the reference's test. In a sharded call a Gaussian without a tile in the band is treated as
            // invisible (radius 0, nothing written): the rank that owns the band never looks at it.
            band_area = (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0);
        }
        float opacity = 0.0f, dc0 = 0.0f, dc1 = 0.0f, dc2 = 0.0f;
        if (band_area != 0) {
            opacity = __builtin_nontemporal_load(p.opacities + idx);
            if (!p.skip_colors) {
                const float* sh = p.shs + 48 * (size_t)idx;
                dc0 = sh[0]; dc1 = sh[1]; dc2 = sh[2];
            }
        }

        // ---- what this Gaussian stores (GSCuda.cu:189-194 cov3D for every Gaussian inside the frustum, :353 rects once det != 0,
        // :362-374 the rest once it has a tile) ----
#pragma unroll
        for (int i = 0; i < 6; ++i) o_c3[i] = c3[i];
        if (det != 0.0f) {
            o_ex = ex; o_ey = ey;
            if (band_area != 0) {
                o_rgb[0] = 0.5f + 0.4f * dc0; o_rgb[1] = 0.5f + 0.4f * dc1; o_rgb[2] = 0.5f + 0.4f * dc2;
                o_depth = prz;
                o_pix = pix; o_piy = piy;
                o_co[0] = cc * det_inv; o_co[1] = -cb * det_inv; o_co[2] = ca * det_inv; o_co[3] = opacity;
                out_radius = (int)my_radius;
                out_tiles = band_area;
                out_rect = pack_rect(x0, y0, x1, y1);
            }
        }
    }
    // ---- stores from here on ----
    // EVERY Gaussian stores every record, zeros where the reference stores nothing (it leaves those entries of its chunk
    // as they were; nothing reads them: a culled Gaussian is in no list). A store that skips half the lanes of a wave
    // leaves half-written lines, and a partial line costs the memory a read-modify-write: with the stores under the
    // visibility tests this kernel took 0.33 ms on the bench frame and 2.8 ms at 50 M, with whole lines 0.25 and 2.4 ms
    // (`gpurun_out/r02_pp_exp10.txt`) — for MORE bytes written. The records leave as streaming stores (0.46 GB that the
    // blend reads a few per cent of, much later: 0.357 -> 0.333 ms before this); what the next kernels read at once —
    // radii, tilesTouched, depth keys, packed rectangles — stays cached.
    {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        typedef int i32x2 __attribute__((ext_vector_type(2)));
        if (!p.cov3D_precomp) {
            f32x2* dst = reinterpret_cast<f32x2*>(p.cov3Ds + 6 * (size_t)idx);
            __builtin_nontemporal_store((f32x2){o_c3[0], o_c3[1]}, dst);
            __builtin_nontemporal_store((f32x2){o_c3[2], o_c3[3]}, dst + 1);
            __builtin_nontemporal_store((f32x2){o_c3[4], o_c3[5]}, dst + 2);
        }
        if (p.rects) __builtin_nontemporal_store((i32x2){o_ex, o_ey}, reinterpret_cast<i32x2*>(p.rects + idx));
        if (!p.skip_colors) {
            float* o = p.rgb + 3 * (size_t)idx;
            __builtin_nontemporal_store(o_rgb[0], o); __builtin_nontemporal_store(o_rgb[1], o + 1); __builtin_nontemporal_store(o_rgb[2], o + 2);
        }
        __builtin_nontemporal_store(o_depth, p.depths + idx);
        __builtin_nontemporal_store((f32x2){o_pix, o_piy}, reinterpret_cast<f32x2*>(p.means2D + idx));
        __builtin_nontemporal_store((f32x4){o_co[0], o_co[1], o_co[2], o_co[3]}, reinterpret_cast<f32x4*>(p.conic_opacity + idx));
    }
    p.radii[idx] = out_radius;
    p.tiles_touched[idx] = out_tiles;
    const uint32_t dkey = out_tiles ? __float_as_uint(prz) : 0xFFFFFFFFu;
    p.depth_keys[idx] = dkey;
    if (p.rect_packed) p.rect_packed[idx] = out_rect;
    // (the depth order's side way, radix_sort.hip: the scan wants to know how many visible keys are not "main" keys)
    if (p.wave_sums) store_wave_sums(p.wave_sums, idx, out_tiles, (dkey >> 24) != kDepthMainTop, p.big_from);
}

// colour = 0.5 + 0.4 DC (GSCuda.cu:362-366), the same two float32 operations as the preprocess kernel above (this file
// is compiled without contraction): the colours a caller precomputes with it are bit-equal to geomState.rgb.
__global__ __launch_bounds__(256) void colors_from_dc_kernel(int n, const float* __restrict__ shs, float* __restrict__ colors) {
    // lane = one float of the output; the three floats of a Gaussian sit at a 192-byte stride in the input (a one-time
    // pass per scene: one 128-byte line per Gaussian is what the input layout costs)
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= 3 * (size_t)n) return;
    const size_t g = f / 3;
    colors[f] = 0.5f + 0.4f * shs[48 * g + (f - 3 * g)];
}

}  // namespace

// geomState.rgb (GSCuda.cu:362-366) for the Gaussians that got a tile, zeros for the others — what preprocess_kernel writes
// when it computes the colours itself, bit for bit. On its own it is a strided read (12 useful bytes of a 128-byte line per
// visible Gaussian) that costs the preprocess 0.10 of its 0.27 ms on the bench frame; nothing needs the colours before the
// blend, and on scenes of a few million Gaussians the kernels between — scan, depth sort, block lists — wait on latency,
// not on HBM: launched on the library's second stream once tilesTouched is final, it runs in their shadow (they take 0.05
// ms longer for it). At 50 M those kernels are bound by HBM themselves: the caller (api.hip) keeps the colours in the
// preprocess there.
__global__ __launch_bounds__(256) void colors_visible_kernel(int n, const uint32_t* __restrict__ tiles_touched,
                                                             const float* __restrict__ shs, float* __restrict__ rgb) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= 3 * (size_t)n) return;
    const size_t g = f / 3;
    // (streaming loads and stores: the lines of the SH array are read once, and the depth sort beside this kernel lives in
    // the L2 — with ordinary ones it took 0.022 ms longer, bench frame 1.248 -> 1.227 ms)
    const float v = tiles_touched[g] != 0u ? 0.5f + 0.4f * __builtin_nontemporal_load(shs + 48 * g + (f - 3 * g)) : 0.0f;
    __builtin_nontemporal_store(v, rgb + f);
}

int launch_colors_visible(int n, const uint32_t* tiles_touched, const float* shs, float* rgb, hipStream_t stream) {
    const size_t floats = 3 * (size_t)n;
    if (floats == 0) return GSR_OK;
    hipLaunchKernelGGL(colors_visible_kernel, dim3((unsigned)((floats + 255) / 256)), dim3(256), 0, stream, n, tiles_touched, shs, rgb);
    GSR_LAUNCH_CHECK("colors_visible_kernel");
    return GSR_OK;
}

int launch_colors_from_dc(int n, const float* shs, float* colors, hipStream_t stream) {
    if (n <= 0) return GSR_OK;
    if (!shs || !colors) return GSR_ERR_INVALID_ARG;
    const size_t floats = 3 * (size_t)n;
    hipLaunchKernelGGL(colors_from_dc_kernel, dim3((unsigned)((floats + 255) / 256)), dim3(256), 0, stream, n, shs, colors);
    GSR_LAUNCH_CHECK("colors_from_dc_kernel");
    return GSR_OK;
}

int launch_preprocess(const gsr_forward_args& a, const gsr_geometry_state& g, int32_t* radii,
                      uint32_t* depth_keys, uint32_t* rect_packed, const FrameDims& d, hipStream_t stream, uint4* wave_sums,
                      bool colors_elsewhere, uint32_t big_from) {
    PreprocessParams p;
    p.skip_colors = a.colors_precomp != nullptr || colors_elsewhere;
    fill_preprocess_params(p, a, g, radii, depth_keys, rect_packed, d, wave_sums, big_from);
    p.focal = (float)a.height / (2.0f * a.tan_fovy);   // GSCuda.cu:721
    p.rects = reinterpret_cast<int2*>(a.rects);
    const unsigned blocks = (unsigned)((a.num_gaussians + 255) / 256);
    hipLaunchKernelGGL(preprocess_kernel, dim3(blocks), dim3(256), 0, stream, p);
    GSR_LAUNCH_CHECK("preprocess_kernel");
    return GSR_OK;
}

}  // namespace gsr
