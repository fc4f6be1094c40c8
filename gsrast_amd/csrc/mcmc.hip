// The three steps of 3DGS-MCMC over the raw parameters (include/gsrast_amd_mcmc.h states the arithmetic operation by
// operation):
//   gsr_mcmc_noise      every step: xyz += covariance x (gated noise), in place, one launch
//   gsr_mcmc_plan       the dead rows in ascending order, the sampling weights of the live ones, the two counts
//   gsr_mcmc_relocate   multiplicities of the sampled rows -> their new opacity and scale -> copies onto the dead rows
//
// All of them are bound by their bytes, so they are about the shape of their accesses.
//   noise: a wave takes 64 consecutive rows. The three arrays of triples (xyz, log_scale, noise) enter the wave's LDS
// region as 16-byte vectors and xyz leaves the same way (wave_triples.hpp); rotation is one float4 per lane, the opacity a
// word. 68 bytes per row, no row is touched by two waves, so in place needs no care beyond load-before-store in the wave.
//   plan: a classify kernel writes a flag per row and the weight; ONE run of the reduce-then-scan of scan.hip turns the
// flags, in place, into their inclusive prefix; a scatter kernel writes dead_idx and the counts (as the densify plan).
//   relocate: three launches behind a memset of temp. count: a thread per sample, integer atomics. update: a thread per
// ROW (two samples of a row would race on the old value): the few rows that were sampled evaluate the header's double
// arithmetic; the 2 x 192 bytes of a row's shs moments are zeroed by 24 lanes of the wave, a vector each. copy: a lane per
// pair for the four narrow arrays (a row of three floats moves as ONE 12-byte vector: the destination rows are scattered, so
// there is no contiguous run of them to gather in LDS), lanes along the 12 vectors of a row for shs, 16 pairs per wave, as
// densify_apply_kernel. No kernel waits for another workgroup.
#include "activation_math.hpp"
#include "gsr_common.hpp"
#include "rotation_math.hpp"
#include "wave_triples.hpp"

#include "../../include/gsrast_amd_mcmc.h"

namespace gsr {
namespace {

// ---- noise -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mcmc_noise_kernel(long long n, float* xyz, const float* __restrict__ opacity_logit,
                                                          const float* __restrict__ log_scale, const float* __restrict__ rotation,
                                                          const float* __restrict__ noise, float scaler) {
    __shared__ __attribute__((aligned(16))) float lds[4][3][kTriple];       // per wave: xyz | log_scale | noise
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const long long first = ((long long)blockIdx.x * 4 + wave) * kWave;
    if (first >= n) return;
    const int count = (int)min((long long)kWave, n - first);
    float (*w)[kTriple] = lds[wave];
    // ---- loads ----
    stage_triples(xyz + 3 * first, count, w[0], lane, ~0ull);
    stage_triples(log_scale + 3 * first, count, w[1], lane, ~0ull);
    stage_triples(noise + 3 * first, count, w[2], lane, ~0ull);
    float4 rot = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    float logit = 0.0f;
    if (lane < count) {
        rot = reinterpret_cast<const float4*>(rotation)[first + lane];
        logit = opacity_logit[first + lane];
    }
    __builtin_amdgcn_wave_barrier();
    // ---- arithmetic: the header's, in its order ----
    if (lane < count) {
        const float o = activate_opacity(logit);
        const float t = 100.0f * ((1.0f - o) - 0.995f);
        const float c = activate_opacity(t) * scaler;
        float v[3], u[3], sq[3], moved[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = w[2][3 * lane + k] * c;
        const float4 sd = activate_scale(w[1][3 * lane], w[1][3 * lane + 1], w[1][3 * lane + 2]);
        const float s[3] = {sd.x, sd.y, sd.z};
        const Rotation3 R = rotation_matrix(activate_rotation(rot.x, rot.y, rot.z, rot.w));
        rotate_transposed(R, v, u);
#pragma unroll
        for (int j = 0; j < 3; ++j) { u[j] = s[j] * u[j]; sq[j] = s[j] * u[j]; }     // S R^T v, then S S R^T v
        rotate(R, sq, moved);
#pragma unroll
        for (int a = 0; a < 3; ++a) w[0][3 * lane + a] = w[0][3 * lane + a] + moved[a];
    }
    __builtin_amdgcn_wave_barrier();
    // ---- stores ----
    flush_triples(xyz + 3 * first, count, w[0], lane);
}

// ---- plan ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mcmc_classify_kernel(long long n, const float* __restrict__ opacity_logit, float logit_min_opacity,
                                                             uint32_t* __restrict__ flags, float* __restrict__ weights) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = opacity_logit[i];
    const bool dead = x <= logit_min_opacity;
    flags[i] = dead ? 1u : 0u;
    weights[i] = dead ? 0.0f : activate_opacity(x);
}

// scan: the inclusive prefix of the flags. Row e is dead iff scan[e] != scan[e - 1], and its place in dead_idx is scan[e - 1].
__global__ __launch_bounds__(256) void mcmc_scatter_kernel(long long n, const uint32_t* __restrict__ scan, int32_t* __restrict__ dead_idx,
                                                            int32_t* __restrict__ counts) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (e == 0) {
        const uint32_t dead = scan[n - 1];
        counts[0] = (int32_t)dead;
        counts[1] = (int32_t)((uint32_t)n - dead);
    }
    const uint32_t here = scan[e], before = e ? scan[e - 1] : 0u;
    if (here != before) dead_idx[before] = (int32_t)e;
}

inline size_t plan_flag_bytes(long long n) { return ((size_t)n * sizeof(uint32_t) + 127) / 128 * 128; }

// ---- relocate --------------------------------------------------------------------------------------------------------------
enum { kXyz = 0, kOpacity = 1, kLogScale = 2, kRotation = 3, kShs = 4, kArrays = 5 };
constexpr int kShsVecs = 12;              // float4 per row of 48 floats
constexpr int kShsRows = 16;              // pairs per wave of the shs copy: 192 vectors, three per lane
constexpr size_t kRelocateHead = 16;      // bytes of temp ahead of c[n]: `rejected` in the first word

struct RelocateArray {
    float *p, *m, *v;
};

struct RelocateParams {
    long long n, m;
    const int32_t *sampled, *dst;
    uint32_t* rejected;
    int32_t* c;
    float min_opacity;
    long long narrow_units;                // the copy's waves that take 64 pairs of the four narrow arrays; the rest take shs
    RelocateArray a[kArrays];
};

// A row of three floats, a lane per row: three adjacent words, which the compiler moves as one 12-byte vector.
struct Triple {
    float x, y, z;
};
__device__ __forceinline__ Triple load_triple(const float* p) { return Triple{p[0], p[1], p[2]}; }
__device__ __forceinline__ void store_triple(float* p, const Triple t) { p[0] = t.x; p[1] = t.y; p[2] = t.z; }

// the pair j as every step sees it: false = ignored
__device__ __forceinline__ bool pair_of(const RelocateParams& q, long long j, long long& s, long long& d) {
    s = q.sampled[j];
    d = q.dst ? (long long)q.dst[j] : 0ll;
    return s >= 0 && s < q.n && d >= 0 && d < q.n;
}

__global__ __launch_bounds__(256) void mcmc_count_kernel(const RelocateParams q) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= q.m) return;
    long long s, d;
    if (pair_of(q, j, s, d)) atomicAdd(&q.c[s], 1);
    else atomicAdd(q.rejected, 1u);
}

// The header's step 2 for one row, in double. -> the new opacity_logit, the float added to each log-scale
__device__ __forceinline__ void relocated_values(float logit, int count, float min_opacity, float& new_logit, float& log_shift) {
    const int ratio = count + 1 < GSR_MCMC_MAX_RATIO ? count + 1 : GSR_MCMC_MAX_RATIO;
    const double o = (double)activate_opacity(logit);
    const double o_new = -expm1(log1p(-o) / (double)ratio);
    double D = 0.0;
    for (int i = 1; i <= ratio; ++i) {
        double p = 1.0, binom = 1.0;                                         // binom = C(i - 1, k)
        for (int k = 0; k < i; ++k) {
            p = p * o_new;
            const double term = (binom * p) / sqrt((double)(k + 1));
            D = (k & 1) ? D - term : D + term;
            binom = (binom * (double)(i - 1 - k)) / (double)(k + 1);
        }
    }
    const double top = 1.0 - 1.1920928955078125e-07;                         // 1 - 2^-23
    const double o_c = fmin(fmax(o_new, (double)min_opacity), top);
    new_logit = (float)log(o_c / (1.0 - o_c));
    log_shift = (float)log(o / D);
}

__global__ __launch_bounds__(256) void mcmc_update_kernel(const RelocateParams q) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int count = i < q.n ? q.c[i] : 0;
    const bool hit = count > 0;
    if (hit) {
        float new_logit, shift;
        relocated_values(q.a[kOpacity].p[i], count, q.min_opacity, new_logit, shift);
        Triple ls = load_triple(q.a[kLogScale].p + 3 * i);
        ls.x = ls.x + shift; ls.y = ls.y + shift; ls.z = ls.z + shift;
        q.a[kOpacity].p[i] = new_logit;
        store_triple(q.a[kLogScale].p + 3 * i, ls);
        const Triple zero3{0.0f, 0.0f, 0.0f};
        const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q.a[kXyz].m) { store_triple(q.a[kXyz].m + 3 * i, zero3); store_triple(q.a[kXyz].v + 3 * i, zero3); }
        if (q.a[kOpacity].m) { q.a[kOpacity].m[i] = 0.0f; q.a[kOpacity].v[i] = 0.0f; }
        if (q.a[kLogScale].m) { store_triple(q.a[kLogScale].m + 3 * i, zero3); store_triple(q.a[kLogScale].v + 3 * i, zero3); }
        if (q.a[kRotation].m) { reinterpret_cast<float4*>(q.a[kRotation].m)[i] = zero4; reinterpret_cast<float4*>(q.a[kRotation].v)[i] = zero4; }
    }
    // the shs moments of the wave's updated rows: 24 lanes, a vector each (every lane of the wave arrives here)
    if (q.a[kShs].m) {
        const long long wave_first = i - lane;
        for (unsigned long long todo = __ballot(hit); todo != 0ull; todo &= todo - 1ull) {
            const long long row = wave_first + (__ffsll((long long)todo) - 1);
            if (lane < 2 * kShsVecs) {
                float* to = lane < kShsVecs ? q.a[kShs].m : q.a[kShs].v;
                reinterpret_cast<float4*>(to)[row * kShsVecs + (lane % kShsVecs)] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
}

__global__ __launch_bounds__(256) void mcmc_copy_kernel(const RelocateParams q) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const long long unit = (long long)blockIdx.x * 4 + wave;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (unit < q.narrow_units) {
        const long long j = unit * kWave + lane;
        long long s, d;
        if (j >= q.m || !pair_of(q, j, s, d)) return;
        // ---- loads ----
        const Triple pos = load_triple(q.a[kXyz].p + 3 * s);
        const float op = q.a[kOpacity].p[s];
        const Triple ls = load_triple(q.a[kLogScale].p + 3 * s);
        const float4 rot = reinterpret_cast<const float4*>(q.a[kRotation].p)[s];
        // ---- stores ----
        const Triple zero3{0.0f, 0.0f, 0.0f};
        store_triple(q.a[kXyz].p + 3 * d, pos);
        q.a[kOpacity].p[d] = op;
        store_triple(q.a[kLogScale].p + 3 * d, ls);
        reinterpret_cast<float4*>(q.a[kRotation].p)[d] = rot;
        if (q.a[kXyz].m) { store_triple(q.a[kXyz].m + 3 * d, zero3); store_triple(q.a[kXyz].v + 3 * d, zero3); }
        if (q.a[kOpacity].m) { q.a[kOpacity].m[d] = 0.0f; q.a[kOpacity].v[d] = 0.0f; }
        if (q.a[kLogScale].m) { store_triple(q.a[kLogScale].m + 3 * d, zero3); store_triple(q.a[kLogScale].v + 3 * d, zero3); }
        if (q.a[kRotation].m) { reinterpret_cast<float4*>(q.a[kRotation].m)[d] = zero4; reinterpret_cast<float4*>(q.a[kRotation].v)[d] = zero4; }
        return;
    }
    // shs: 16 pairs, lanes along the 12 vectors of a row
    const long long first = (unit - q.narrow_units) * kShsRows;
    if (first >= q.m) return;
    const int count = (int)min((long long)kShsRows, q.m - first);
    long long s = -1, d = -1;
    if (lane < count && !pair_of(q, first + lane, s, d)) s = -1;
    const float4* P = reinterpret_cast<const float4*>(q.a[kShs].p);
    float4* DP = reinterpret_cast<float4*>(q.a[kShs].p);
    float4* DM = reinterpret_cast<float4*>(q.a[kShs].m);
    float4* DV = reinterpret_cast<float4*>(q.a[kShs].v);
    const int total = count * kShsVecs;
    // (named registers, a call per vector, as densify_apply_kernel)
    auto load = [&](int k, float4& p, long long& to) {
        const int e = k * kWave + lane;
        const int row = e / kShsVecs;                                        // (<= 15)
        const long long sr = __shfl(s, row, kWave), dr = __shfl(d, row, kWave);
        to = -1;
        p = zero4;
        if (e < total && sr >= 0) {
            p = P[sr * kShsVecs + (e - row * kShsVecs)];
            to = dr * kShsVecs + (e - row * kShsVecs);
        }
    };
    auto store = [&](const float4& p, long long to) {
        if (to >= 0) {
            DP[to] = p;
            if (DM) { DM[to] = zero4; DV[to] = zero4; }
        }
    };
    float4 p0, p1, p2;
    long long to0, to1, to2;
    // ---- loads ----
    load(0, p0, to0);
    load(1, p1, to1);
    load(2, p2, to2);
    // ---- stores ----
    store(p0, to0);
    store(p1, to1);
    store(p2, to2);
}

inline size_t relocate_count_bytes(long long n) { return ((size_t)n * sizeof(int32_t) + 15) / 16 * 16; }

}  // namespace
}  // namespace gsr

using namespace gsr;

static int mcmc_noise_impl(const gsr_mcmc_noise_args* args) {
    if (!args || args->struct_size != sizeof(gsr_mcmc_noise_args)) return GSR_ERR_INVALID_ARG;
    const long long n = args->n;
    if (n < 0) return GSR_ERR_INVALID_ARG;
    if (n > 0 && (!args->xyz || !args->opacity_logit || !args->log_scale || !args->rotation || !args->noise)) return GSR_ERR_INVALID_ARG;
    if (misaligned(args->xyz, 16) || misaligned(args->log_scale, 16) || misaligned(args->rotation, 16) || misaligned(args->noise, 16) ||
        misaligned(args->opacity_logit, 4))
        return GSR_ERR_INVALID_ARG;
    if (n > GSR_MCMC_MAX_ROWS) return GSR_ERR_TOO_LARGE;
    if (n == 0) return GSR_OK;
    const long long blocks = (n + 4 * kWave - 1) / (4 * kWave);
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)args->stream, n, args->xyz,
                       args->opacity_logit, args->log_scale, args->rotation, args->noise, args->scaler);
    GSR_LAUNCH_CHECK("mcmc_noise_kernel");
    return GSR_OK;
}
extern "C" int gsr_mcmc_noise(const gsr_mcmc_noise_args* args) { return entry_point(mcmc_noise_impl, args); }

extern "C" size_t gsr_mcmc_plan_temp_bytes(int64_t n) {
    if (n < 0 || n > GSR_MCMC_MAX_ROWS) return 0;
    return plan_flag_bytes(n) + scan_temp_bytes((size_t)n);
}

static int mcmc_plan_impl(int64_t n, const float* opacity_logit, float logit_min_opacity, void* temp, int32_t* dead_idx, float* weights,
                          int32_t* counts, void* stream) {
    if (n < 0 || !counts) return GSR_ERR_INVALID_ARG;
    if (n > 0 && (!opacity_logit || !temp || !dead_idx || !weights)) return GSR_ERR_INVALID_ARG;
    if (misaligned(opacity_logit, 4) || misaligned(temp, 16) || misaligned(dead_idx, 4) || misaligned(weights, 4) || misaligned(counts, 4))
        return GSR_ERR_INVALID_ARG;
    if (n > GSR_MCMC_MAX_ROWS) return GSR_ERR_TOO_LARGE;
    const hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        GSR_HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st));
        return GSR_OK;
    }
    const long long blocks = (n + 255) / 256;
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    uint32_t* flags = reinterpret_cast<uint32_t*>(temp);
    char* scan_temp = reinterpret_cast<char*>(temp) + plan_flag_bytes(n);
    hipLaunchKernelGGL(mcmc_classify_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (long long)n, opacity_logit, logit_min_opacity,
                       flags, weights);
    GSR_LAUNCH_CHECK("mcmc_classify_kernel");
    GSR_TRY(launch_inclusive_scan(flags, flags, (size_t)n, scan_temp, st));
    hipLaunchKernelGGL(mcmc_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (long long)n, flags, dead_idx, counts);
    GSR_LAUNCH_CHECK("mcmc_scatter_kernel");
    return GSR_OK;
}
extern "C" int gsr_mcmc_plan(int64_t n, const float* opacity_logit, float logit_min_opacity, void* temp, int32_t* dead_idx, float* weights,
                             int32_t* counts, void* stream) {
    return entry_point(mcmc_plan_impl, n, opacity_logit, logit_min_opacity, temp, dead_idx, weights, counts, stream);
}

extern "C" size_t gsr_mcmc_relocate_temp_bytes(int64_t n) {
    if (n < 0 || n > GSR_MCMC_MAX_ROWS) return 0;
    return kRelocateHead + relocate_count_bytes(n);
}

static int mcmc_relocate_impl(const gsr_mcmc_relocate_args* args) {
    if (!args || args->struct_size != sizeof(gsr_mcmc_relocate_args)) return GSR_ERR_INVALID_ARG;
    const long long n = args->n, m = args->m;
    if (n < 0 || m < 0) return GSR_ERR_INVALID_ARG;
    if (!(args->min_opacity > 0.0f && args->min_opacity < 1.0f)) return GSR_ERR_INVALID_ARG;
    const gsr_mcmc_array* in[kArrays] = {&args->xyz, &args->opacity_logit, &args->log_scale, &args->rotation, &args->shs};
    RelocateParams q;
    for (int k = 0; k < kArrays; ++k) {
        const gsr_mcmc_array& a = *in[k];
        if (n > 0 && !a.param) return GSR_ERR_INVALID_ARG;
        if ((a.exp_avg != nullptr) != (a.exp_avg_sq != nullptr)) return GSR_ERR_INVALID_ARG;
        if (misaligned(a.param, 16) || misaligned(a.exp_avg, 16) || misaligned(a.exp_avg_sq, 16)) return GSR_ERR_INVALID_ARG;
        q.a[k] = RelocateArray{a.param, a.exp_avg, a.exp_avg_sq};
    }
    if (m > 0 && (!args->sampled || !args->temp)) return GSR_ERR_INVALID_ARG;
    if (misaligned(args->sampled, 4) || misaligned(args->dst, 4) || misaligned(args->temp, 16)) return GSR_ERR_INVALID_ARG;
    if (n > GSR_MCMC_MAX_ROWS || m > GSR_MCMC_MAX_ROWS) return GSR_ERR_TOO_LARGE;
    if (m == 0) return GSR_OK;
    const hipStream_t st = (hipStream_t)args->stream;
    q.n = n;
    q.m = m;
    q.sampled = args->sampled;
    q.dst = args->dst;
    q.rejected = reinterpret_cast<uint32_t*>(args->temp);
    q.c = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(args->temp) + kRelocateHead);
    q.min_opacity = args->min_opacity;
    q.narrow_units = (m + kWave - 1) / kWave;
    const long long count_blocks = (m + 255) / 256, update_blocks = (n + 255) / 256;
    const long long copy_blocks = (q.narrow_units + (m + kShsRows - 1) / kShsRows + 3) / 4;
    if (exceeds_grid(count_blocks) || exceeds_grid(update_blocks) || exceeds_grid(copy_blocks)) return GSR_ERR_TOO_LARGE;
    GSR_HIP_TRY(hipMemsetAsync(args->temp, 0, kRelocateHead + relocate_count_bytes(n), st));
    hipLaunchKernelGGL(mcmc_count_kernel, dim3((unsigned)count_blocks), dim3(256), 0, st, q);
    GSR_LAUNCH_CHECK("mcmc_count_kernel");
    if (n == 0) return GSR_OK;                                               // (every pair was rejected)
    hipLaunchKernelGGL(mcmc_update_kernel, dim3((unsigned)update_blocks), dim3(256), 0, st, q);
    GSR_LAUNCH_CHECK("mcmc_update_kernel");
    if (args->dst) {
        hipLaunchKernelGGL(mcmc_copy_kernel, dim3((unsigned)copy_blocks), dim3(256), 0, st, q);
        GSR_LAUNCH_CHECK("mcmc_copy_kernel");
    }
    return GSR_OK;
}
extern "C" int gsr_mcmc_relocate(const gsr_mcmc_relocate_args* args) { return entry_point(mcmc_relocate_impl, args); }
