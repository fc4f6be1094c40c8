// Adaptive density control over the raw parameters (include/gsrast_amd.h states the arithmetic, the classes and the order
// of the output rows):
//   gsr_densify_accumulate   a frame's statistics: |dL_dmean2D| in upstream's NDC convention, how often seen, the largest radius
//   gsr_densify_plan         which rows are kept, cloned, split and pruned -> src_of (the source row of every output row), counts
//   gsr_densify_apply        the five arrays and their Adam moments gathered into arrays of the new row count, in one launch
//
// All three are bound by their bytes, so they are about the shape of their accesses.
//   accumulate: rows are narrow (a word, a float2), so lanes run along rows; a wave takes 256 consecutive rows, four per lane,
// the radii words first: a culled row loads nothing else. No atomics: a row belongs to one lane.
//   plan: a classify kernel writes three flag arrays back to back (kept | clone | split-and-surviving, u32[3 n]); ONE run of the
// reduce-then-scan of scan.hip over all 3 n turns them, in place, into their inclusive prefix (a tile of the scan is loaded whole
// before it is stored and belongs to one workgroup: in == out is allowed, include/gsrast_amd.h); a scatter kernel writes
// src_of. The prefix running through the three arrays IS upstream's concatenation order: a clone's position already
// includes K, a child's K + C; child 1 of a parent lies S rows behind its child 0. No kernel waits for another workgroup.
//   apply: output-major. A wave takes one UNIT, `rows` consecutive OUTPUT rows of one array (64, or 16 of the 48-float
// array, as adam.hip), reads their src_of words once — lane r reads row r's — and gathers: writes are whole 16-byte vectors
// and contiguous, reads are monotone within each of the four segments. An array of three floats per row is gathered by plain
// float loads, a lane per row, and leaves through the wave's LDS region as 16-byte vectors (wave_triples.hpp). All of a
// unit's loads come before its first store.
#include "activation_math.hpp"
#include "gsr_common.hpp"
#include "rotation_math.hpp"
#include "wave_triples.hpp"

namespace gsr {
namespace {

// ---- accumulate ------------------------------------------------------------------------------------------------------------
constexpr int kAccRows = 4;               // per lane: a wave takes 4 x 64 consecutive rows

__global__ __launch_bounds__(256) void densify_accumulate_kernel(long long n, const float2* __restrict__ grad,
                                                                  const int32_t* __restrict__ radii, float half_width, float half_height,
                                                                  float* __restrict__ grad_accum, int32_t* __restrict__ denom,
                                                                  int32_t* __restrict__ max_radii) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long base = ((long long)blockIdx.x * 4 + wave) * (kAccRows * kWave) + lane;
    int32_t rad[kAccRows], den[kAccRows], big[kAccRows];
    float2 g[kAccRows];
    float acc[kAccRows];
    // ---- loads: the radii words first ----
#pragma unroll
    for (int k = 0; k < kAccRows; ++k) {
        const long long i = base + k * kWave;
        rad[k] = i < n ? radii[i] : 0;
    }
#pragma unroll
    for (int k = 0; k < kAccRows; ++k) {
        const long long i = base + k * kWave;
        if (rad[k] > 0) { g[k] = grad[i]; acc[k] = grad_accum[i]; den[k] = denom[i]; big[k] = max_radii[i]; }
    }
    // ---- arithmetic and stores ----
#pragma unroll
    for (int k = 0; k < kAccRows; ++k) {
        const long long i = base + k * kWave;
        if (rad[k] > 0) {
            const float gx = g[k].x * half_width, gy = g[k].y * half_height;
            grad_accum[i] = acc[k] + sqrtf(gx * gx + gy * gy);
            denom[i] = den[k] + 1;
            max_radii[i] = big[k] > rad[k] ? big[k] : rad[k];
        }
    }
}

// ---- plan ------------------------------------------------------------------------------------------------------------------
struct PlanScalars {
    float max_grad, log_dense, logit_min_opacity, log_world, log_shrink;
    int32_t max_screen;
};

__global__ __launch_bounds__(256) void densify_classify_kernel(long long n, const float* __restrict__ opacity_logit,
                                                                const float* __restrict__ log_scale, const float* __restrict__ grad_accum,
                                                                const int32_t* __restrict__ denom, const int32_t* __restrict__ max_radii,
                                                                const PlanScalars s, uint32_t* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float o = opacity_logit[i];
    const float s0 = log_scale[3 * i], s1 = log_scale[3 * i + 1], s2 = log_scale[3 * i + 2];
    const float ga = grad_accum[i];
    const int32_t d = denom[i], mr = max_radii[i];
    float g = d > 0 ? ga / (float)d : 0.0f;
    if (!(g == g)) g = 0.0f;
    float m = s0;
    if (s1 > m) m = s1;
    if (s2 > m) m = s2;
    const bool hot = g >= s.max_grad, big = m > s.log_dense;
    const bool clone = hot && !big, split = hot && big;
    const bool faint = o < s.logit_min_opacity, sized = s.max_screen > 0;
    const bool doomed = faint || (sized && (mr > s.max_screen || m > s.log_world));
    const float mc = m - s.log_shrink;
    const bool child_doomed = faint || (sized && (mr > s.max_screen || mc > s.log_world));
    flags[i] = (!split && !doomed) ? 1u : 0u;
    flags[n + i] = (clone && !doomed) ? 1u : 0u;
    flags[2 * n + i] = (split && !child_doomed) ? 1u : 0u;
}

// scan: the inclusive prefix of the 3 n flags. Element e is a flag that was set iff scan[e] != scan[e - 1], and its output
// row is scan[e - 1]; a split parent's child 1 lies S rows further on.
__global__ __launch_bounds__(256) void densify_scatter_kernel(long long n, const uint32_t* __restrict__ scan, int32_t* __restrict__ src_of,
                                                               int32_t* __restrict__ counts) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * n) return;
    const uint32_t kept = scan[n - 1], with_clones = scan[2 * n - 1], with_splits = scan[3 * n - 1];
    const uint32_t splits = with_splits - with_clones;
    if (e == 0) {
        counts[0] = (int32_t)kept;
        counts[1] = (int32_t)(with_clones - kept);
        counts[2] = (int32_t)splits;
        counts[3] = (int32_t)(with_splits + splits);
    }
    const uint32_t here = scan[e], before = e ? scan[e - 1] : 0u;
    if (here == before) return;
    const int32_t row = (int32_t)(e < n ? e : (e < 2 * n ? e - n : e - 2 * n));
    src_of[before] = row;
    if (e >= 2 * n) src_of[before + splits] = row;
}

// ---- apply -----------------------------------------------------------------------------------------------------------------
enum { kXyz = 0, kOpacity = 1, kLogScale = 2, kRotation = 3, kShs = 4, kArrays = 5 };
constexpr int kShsVecs = 12;              // float4 per row of 48 floats
constexpr int kShsRows = 16;              // rows per unit: 192 vectors, three per lane

struct ApplyArray {
    const float *src, *src_m, *src_v;
    float *dst, *dst_m, *dst_v;
    long long unit_end;                   // this array's units end here, in the launch's numbering
};

struct ApplyParams {
    long long n_src, n_out;
    long long kept_end, clone_end, child0_end;      // K, K + C, K + C + S
    const int32_t* src_of;
    const float* noise;
    float log_shrink;
    ApplyArray a[kArrays];
};

// xyz of child k of a split parent: the header's arithmetic.
__device__ __forceinline__ void child_position(float (&p)[3], const float* __restrict__ ls, const float4 rot,
                                               const float* __restrict__ z) {
    const float4 sd = activate_scale(ls[0], ls[1], ls[2]);
    const Rotation3 R = rotation_matrix(activate_rotation(rot.x, rot.y, rot.z, rot.w));
    const float d[3] = {sd.x * z[0], sd.y * z[1], sd.z * z[2]};
    float moved[3];
    rotate(R, d, moved);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = p[a] + moved[a];
}

__global__ __launch_bounds__(256) void densify_apply_kernel(const ApplyParams q) {
    __shared__ __attribute__((aligned(16))) float lds[4][3][kTriple];       // per wave: p | m | v of an array of triples
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const long long unit = (long long)blockIdx.x * 4 + wave;
    int t = 0;
    while (t < kArrays && unit >= q.a[t].unit_end) ++t;
    if (t >= kArrays) return;
    const ApplyArray& a = q.a[t];
    const int rows = t == kShs ? kShsRows : kWave;
    const long long first = (unit - (t ? q.a[t - 1].unit_end : 0ll)) * rows;
    if (first >= q.n_out) return;
    const int count = (int)min((long long)rows, q.n_out - first);
    const bool moments = a.src_m != nullptr;
    // the rows' sources: lane r reads row r's word (kept inside the source arrays whatever the word says)
    const long long r = first + lane;
    long long s = 0;
    if (lane < count) {
        s = q.src_of[r];
        s = s < 0 ? 0 : (s >= q.n_src ? q.n_src - 1 : s);
    }
    if (t == kShs) {
        const float4* __restrict__ P = reinterpret_cast<const float4*>(a.src);
        const float4* __restrict__ M = reinterpret_cast<const float4*>(a.src_m);
        const float4* __restrict__ V = reinterpret_cast<const float4*>(a.src_v);
        const int total = count * kShsVecs;
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4* __restrict__ DP = reinterpret_cast<float4*>(a.dst) + first * kShsVecs;
        float4* __restrict__ DM = reinterpret_cast<float4*>(a.dst_m) + first * kShsVecs;
        float4* __restrict__ DV = reinterpret_cast<float4*>(a.dst_v) + first * kShsVecs;
        // (named registers, a call per vector: as arrays indexed in a loop around the shuffle the nine vectors went through scratch)
        auto load = [&](int k, float4& p, float4& m, float4& v) {
            const int e = k * kWave + lane;
            const int row = e / kShsVecs;                                    // (<= 15)
            const long long sr = __shfl(s, row, kWave);
            p = zero; m = zero; v = zero;
            if (e < total) {
                const long long at = sr * kShsVecs + (e - row * kShsVecs);
                p = P[at];
                if (moments && first + row < q.kept_end) { m = M[at]; v = V[at]; }
            }
        };
        auto store = [&](int k, const float4& p, const float4& m, const float4& v) {
            const int e = k * kWave + lane;
            if (e < total) {
                DP[e] = p;
                if (moments) { DM[e] = m; DV[e] = v; }
            }
        };
        float4 p0, m0, v0, p1, m1, v1, p2, m2, v2;
        // ---- loads ----
        load(0, p0, m0, v0);
        load(1, p1, m1, v1);
        load(2, p2, m2, v2);
        // ---- stores ----
        store(0, p0, m0, v0);
        store(1, p1, m1, v1);
        store(2, p2, m2, v2);
        return;
    }
    const bool kept = r < q.kept_end, child = r >= q.clone_end;
    if (t == kRotation) {
        if (lane >= count) return;
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 p = reinterpret_cast<const float4*>(a.src)[s];
        float4 m = zero, v = zero;
        if (moments && kept) { m = reinterpret_cast<const float4*>(a.src_m)[s]; v = reinterpret_cast<const float4*>(a.src_v)[s]; }
        reinterpret_cast<float4*>(a.dst)[r] = p;
        if (moments) { reinterpret_cast<float4*>(a.dst_m)[r] = m; reinterpret_cast<float4*>(a.dst_v)[r] = v; }
        return;
    }
    if (t == kOpacity) {
        if (lane >= count) return;
        const float p = a.src[s];
        float m = 0.0f, v = 0.0f;
        if (moments && kept) { m = a.src_m[s]; v = a.src_v[s]; }
        a.dst[r] = p;
        if (moments) { a.dst_m[r] = m; a.dst_v[r] = v; }
        return;
    }
    // xyz or log_scale: a lane per row, out through the wave's LDS region
    float (*w)[kTriple] = lds[wave];
    if (lane < count) {
        float p[3], m[3] = {0.0f, 0.0f, 0.0f}, v[3] = {0.0f, 0.0f, 0.0f};
        // ---- loads ----
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = a.src[3 * s + c];
        if (moments && kept) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { m[c] = a.src_m[3 * s + c]; v[c] = a.src_v[3 * s + c]; }
        }
        if (child) {
            if (t == kLogScale) {
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = p[c] - q.log_shrink;
            } else {
                const bool second = r >= q.child0_end;
                const long long j = r - (second ? q.child0_end : q.clone_end);
                float ls[3], z[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { ls[c] = q.a[kLogScale].src[3 * s + c]; z[c] = q.noise[(2 * j + (second ? 1 : 0)) * 3 + c]; }
                const float4 rot = reinterpret_cast<const float4*>(q.a[kRotation].src)[s];
                child_position(p, ls, rot, z);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { w[0][3 * lane + c] = p[c]; w[1][3 * lane + c] = m[c]; w[2][3 * lane + c] = v[c]; }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- stores ----
    flush_triples(a.dst + 3 * first, count, w[0], lane);
    if (moments) {
        flush_triples(a.dst_m + 3 * first, count, w[1], lane);
        flush_triples(a.dst_v + 3 * first, count, w[2], lane);
    }
}

constexpr long long kPlanMaxRows = 0x7FFFFFFFll / 3;                        // 3 n flags, their sums and the counts in 32 bits

inline size_t plan_flag_bytes(long long n) { return ((size_t)n * 3 * sizeof(uint32_t) + 127) / 128 * 128; }

}  // namespace
}  // namespace gsr

using namespace gsr;

static int densify_accumulate_impl(int64_t n, const float* dL_dmean2D, const int32_t* radii, float half_width, float half_height,
                                   float* grad_accum, int32_t* denom, int32_t* max_radii, void* stream) {
    if (n < 0 || !dL_dmean2D || !radii || !grad_accum || !denom || !max_radii) return GSR_ERR_INVALID_ARG;
    if (misaligned(dL_dmean2D, 8) || misaligned(radii, 4) || misaligned(grad_accum, 4) || misaligned(denom, 4) || misaligned(max_radii, 4))
        return GSR_ERR_INVALID_ARG;
    if (n == 0) return GSR_OK;
    const long long per_block = 4ll * kAccRows * kWave;
    const long long blocks = (n + per_block - 1) / per_block;
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    hipLaunchKernelGGL(densify_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long long)n,
                       reinterpret_cast<const float2*>(dL_dmean2D), radii, half_width, half_height, grad_accum, denom, max_radii);
    GSR_LAUNCH_CHECK("densify_accumulate_kernel");
    return GSR_OK;
}
extern "C" int gsr_densify_accumulate(int64_t n, const float* dL_dmean2D, const int32_t* radii, float half_width, float half_height,
                                      float* grad_accum, int32_t* denom, int32_t* max_radii, void* stream) {
    return entry_point(densify_accumulate_impl, n, dL_dmean2D, radii, half_width, half_height, grad_accum, denom, max_radii, stream);
}

extern "C" size_t gsr_densify_plan_temp_bytes(int64_t n) {
    if (n < 0 || n > kPlanMaxRows) return 0;
    return plan_flag_bytes(n) + scan_temp_bytes((size_t)n * 3);
}

static int densify_plan_impl(int64_t n, const float* opacity_logit, const float* log_scale, const float* grad_accum, const int32_t* denom,
                             const int32_t* max_radii, float max_grad, float log_dense, float logit_min_opacity, float log_world,
                             float log_shrink, int32_t max_screen, void* temp, int32_t* src_of, int32_t* counts, void* stream) {
    if (n < 0 || !opacity_logit || !log_scale || !grad_accum || !denom || !max_radii || !temp || !src_of || !counts)
        return GSR_ERR_INVALID_ARG;
    if (misaligned(opacity_logit, 4) || misaligned(log_scale, 4) || misaligned(grad_accum, 4) || misaligned(denom, 4) ||
        misaligned(max_radii, 4) || misaligned(temp, 16) || misaligned(src_of, 4) || misaligned(counts, 4))
        return GSR_ERR_INVALID_ARG;
    if (n > kPlanMaxRows) return GSR_ERR_TOO_LARGE;
    const hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        GSR_HIP_TRY(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), st));
        return GSR_OK;
    }
    uint32_t* flags = reinterpret_cast<uint32_t*>(temp);
    char* scan_temp = reinterpret_cast<char*>(temp) + plan_flag_bytes(n);
    const PlanScalars s{max_grad, log_dense, logit_min_opacity, log_world, log_shrink, max_screen};
    hipLaunchKernelGGL(densify_classify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (long long)n, opacity_logit,
                       log_scale, grad_accum, denom, max_radii, s, flags);
    GSR_LAUNCH_CHECK("densify_classify_kernel");
    GSR_TRY(launch_inclusive_scan(flags, flags, (size_t)n * 3, scan_temp, st));
    hipLaunchKernelGGL(densify_scatter_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, st, (long long)n, flags, src_of, counts);
    GSR_LAUNCH_CHECK("densify_scatter_kernel");
    return GSR_OK;
}
extern "C" int gsr_densify_plan(int64_t n, const float* opacity_logit, const float* log_scale, const float* grad_accum, const int32_t* denom,
                                const int32_t* max_radii, float max_grad, float log_dense, float logit_min_opacity, float log_world,
                                float log_shrink, int32_t max_screen, void* temp, int32_t* src_of, int32_t* counts, void* stream) {
    return entry_point(densify_plan_impl, n, opacity_logit, log_scale, grad_accum, denom, max_radii, max_grad, log_dense, logit_min_opacity,
                       log_world, log_shrink, max_screen, temp, src_of, counts, stream);
}

static int densify_apply_impl(const gsr_densify_apply_args* args) {
    if (!args || args->struct_size != sizeof(gsr_densify_apply_args)) return GSR_ERR_INVALID_ARG;
    const long long n = args->n_src, K = args->counts[0], C = args->counts[1], S = args->counts[2], total = args->counts[3];
    if (n < 0 || K < 0 || C < 0 || S < 0 || total != K + C + 2 * S || K + S > n || C + S > n) return GSR_ERR_INVALID_ARG;
    if (!args->src_of || misaligned(args->src_of, 4) || (S > 0 && !args->noise) || misaligned(args->noise, 4))
        return GSR_ERR_INVALID_ARG;
    const gsr_densify_array* in[kArrays] = {&args->xyz, &args->opacity_logit, &args->log_scale, &args->rotation, &args->shs};
    for (int k = 0; k < kArrays; ++k) {
        const gsr_densify_array& a = *in[k];
        if (!a.src || !a.dst) return GSR_ERR_INVALID_ARG;
        const int set = (a.src_exp_avg != nullptr) + (a.src_exp_avg_sq != nullptr) + (a.dst_exp_avg != nullptr) + (a.dst_exp_avg_sq != nullptr);
        if (set != 0 && set != 4) return GSR_ERR_INVALID_ARG;
        if (misaligned(a.src, 16) || misaligned(a.dst, 16) || misaligned(a.src_exp_avg, 16) || misaligned(a.src_exp_avg_sq, 16) ||
            misaligned(a.dst_exp_avg, 16) || misaligned(a.dst_exp_avg_sq, 16))
            return GSR_ERR_INVALID_ARG;
    }
    if (total == 0) return GSR_OK;
    ApplyParams q;
    q.n_src = n;
    q.n_out = total;
    q.kept_end = K;
    q.clone_end = K + C;
    q.child0_end = K + C + S;
    q.src_of = args->src_of;
    q.noise = args->noise;
    q.log_shrink = args->log_shrink;
    long long units = 0;
    for (int k = 0; k < kArrays; ++k) {
        const gsr_densify_array& a = *in[k];
        const int rows = k == kShs ? kShsRows : kWave;
        units += (total + rows - 1) / rows;
        q.a[k] = ApplyArray{a.src, a.src_exp_avg, a.src_exp_avg_sq, a.dst, a.dst_exp_avg, a.dst_exp_avg_sq, units};
    }
    const long long blocks = (units + 3) / 4;
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    hipLaunchKernelGGL(densify_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)args->stream, q);
    GSR_LAUNCH_CHECK("densify_apply_kernel");
    return GSR_OK;
}
extern "C" int gsr_densify_apply(const gsr_densify_apply_args* args) { return entry_point(densify_apply_impl, args); }
