// gsr_adam_step: one in-place Adam update of up to eight arrays that share a row count, gated row by row by the frame's
// radii (include/gsrast_amd.h states the arithmetic and its order).
//
// The step is bound by its bytes: 28 per float updated (p, g, m, v read; p, m, v written), 4 per row for the visibility
// word. So the kernel is about the shape of its accesses, and lanes run along the floats of a wave's rows, never one row
// per lane (a row of 48 floats is 192 bytes: a row per lane would be the strided read gsr_colors_from_dc once paid for).
//   One launch covers every array. A wave takes one UNIT: `rows` consecutive rows of one array (a power of two, 64 at the
// most, chosen on the host so that a unit is at most 256 accesses: 16 rows of 48 floats, 64 of any width up to 4); a
// workgroup is four waves with consecutive units. The wave reads its rows' visibility words once — lane r reads row r's —
// and shares them as a ballot; a unit without a visible row ends there.
//   row_floats % 4 == 0   the unit is a run of float4: lane l takes vectors l, l + 64, l + 128, l + 192 of it
//   row_floats == 3       the wave-private LDS staging of wave_triples.hpp (a 16-byte vector straddles two rows: one with
//                         a visible row is loaded and stored whole, its culled neighbour's floats going back as they
//                         came — the same wave owns both, so nothing races; one without is neither loaded nor stored)
//   any other width       the same run, of single floats
// Memory schedule (the rule above preprocess_backward_kernel, backward.hip): all of a unit's loads come before its first
// store. A row wider than 1024 floats (no array of a Gaussian is) takes several such passes. No atomics, and every float
// is computed from its own p, g, m, v and its array's six scalars alone: the result does not depend on the launch shape.
#include "gsr_common.hpp"
#include "wave_triples.hpp"

namespace gsr {
namespace {

constexpr int kUnitAccesses = 4;          // per lane, array and pass: 4 x 64 lanes = 256 accesses

struct AdamScalars {
    float step_size, rs, b1c, b2, b2c, eps;
};

struct AdamArray {
    float* p;
    const float* g;
    float* m;
    float* v;
    int row_floats;
    int rows;                             // rows per unit
    long long unit_end;                   // this array's units end here, in the launch's numbering (they begin where the one before ends)
    AdamScalars s;
};

struct AdamParams {
    long long n;
    int count;
    const int32_t* visible;
    AdamArray a[GSR_ADAM_MAX_TENSORS];
};

// The arithmetic of the header, one float. (-ffp-contract=off: no fused multiply-add; sqrtf and / correctly rounded.)
__device__ __forceinline__ void adam_float(const AdamScalars& s, float& p, float g, float& m, float& v) {
    m = m + s.b1c * (g - m);
    v = s.b2 * v + s.b2c * (g * g);
    const float den = sqrtf(v) / s.rs + s.eps;
    p = p - s.step_size * (m / den);
}

__device__ __forceinline__ void adam_update(const AdamScalars& s, float& p, const float& g, float& m, float& v) { adam_float(s, p, g, m, v); }
__device__ __forceinline__ void adam_update(const AdamScalars& s, float4& p, const float4& g, float4& m, float4& v) {
    adam_float(s, p.x, g.x, m.x, v.x);
    adam_float(s, p.y, g.y, m.y, v.y);
    adam_float(s, p.z, g.z, m.z, v.z);
    adam_float(s, p.w, g.w, m.w, v.w);
}

// A unit as a run of T (float4 or float): `count` rows of `width` Ts each, beginning at T index `base` of the arrays.
template <typename T>
__device__ __forceinline__ void update_run(const AdamArray& a, long long base, int count, int width, int lane, unsigned long long wanted) {
    T* __restrict__ P = reinterpret_cast<T*>(a.p) + base;
    const T* __restrict__ G = reinterpret_cast<const T*>(a.g) + base;
    T* __restrict__ M = reinterpret_cast<T*>(a.m) + base;
    T* __restrict__ V = reinterpret_cast<T*>(a.v) + base;
    const int total = count * width;                                         // (<= 256 unless one row alone is wider: several passes)
    for (int pass = 0; pass < total; pass += kUnitAccesses * kWave) {
        T p[kUnitAccesses], g[kUnitAccesses], m[kUnitAccesses], v[kUnitAccesses];
        bool on[kUnitAccesses];
        // ---- loads ----
#pragma unroll
        for (int k = 0; k < kUnitAccesses; ++k) {
            const int e = pass + k * kWave + lane;
            on[k] = e < total && ((wanted >> (e / width)) & 1ull);
            if (on[k]) { p[k] = P[e]; g[k] = G[e]; m[k] = M[e]; v[k] = V[e]; }
        }
        // ---- arithmetic ----
#pragma unroll
        for (int k = 0; k < kUnitAccesses; ++k)
            if (on[k]) adam_update(a.s, p[k], g[k], m[k], v[k]);
        // ---- stores ----
#pragma unroll
        for (int k = 0; k < kUnitAccesses; ++k) {
            const int e = pass + k * kWave + lane;
            if (on[k]) { P[e] = p[k]; M[e] = m[k]; V[e] = v[k]; }
        }
    }
}

// A unit of an array of three floats per row: 64 rows, every lane its own row's three floats in the wave's LDS region.
__device__ __forceinline__ void update_triples(const AdamArray& a, long long first, int count, int lane, unsigned long long wanted,
                                               float (*w)[kTriple]) {
    const long long base = 3 * first;
    // ---- loads ----
    stage_triples(a.p + base, count, w[0], lane, wanted);
    stage_triples(a.g + base, count, w[1], lane, wanted);
    stage_triples(a.m + base, count, w[2], lane, wanted);
    stage_triples(a.v + base, count, w[3], lane, wanted);
    __builtin_amdgcn_wave_barrier();
    // ---- arithmetic: in place, a culled row's floats stay what was loaded ----
    if ((wanted >> lane) & 1ull) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = 3 * lane + k;
            adam_float(a.s, w[0][e], w[1][e], w[2][e], w[3][e]);
        }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- stores ----
    flush_triples(a.p + base, count, w[0], lane, wanted);
    flush_triples(a.m + base, count, w[2], lane, wanted);
    flush_triples(a.v + base, count, w[3], lane, wanted);
}

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamParams q) {
    __shared__ __attribute__((aligned(16))) float lds[4][4][kTriple];       // per wave: p | g | m | v of an array of triples
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const long long unit = (long long)blockIdx.x * 4 + wave;                // (wave-uniform, and the compiler knows it)
    int t = 0;
    while (t < q.count && unit >= q.a[t].unit_end) ++t;
    if (t >= q.count) return;
    const AdamArray& a = q.a[t];
    const long long first = (unit - (t ? q.a[t - 1].unit_end : 0ll)) * a.rows;      // first row of this unit
    if (first >= q.n) return;
    const int count = (int)min((long long)a.rows, q.n - first);
    // the visibility words first: a culled row loads nothing else
    const bool visible = lane < count && (q.visible == nullptr || q.visible[first + lane] > 0);
    const unsigned long long wanted = __ballot(visible);
    if (wanted == 0ull) return;
    const int rf = a.row_floats;
    if (rf == 3) update_triples(a, first, count, lane, wanted, lds[wave]);
    else if ((rf & 3) == 0) update_run<float4>(a, first * (rf >> 2), count, rf >> 2, lane, wanted);
    else update_run<float>(a, first * rf, count, rf, lane, wanted);
}

}  // namespace
}  // namespace gsr

using namespace gsr;

static int adam_step_impl(const gsr_adam_args* args) {
    if (!args || args->struct_size != sizeof(gsr_adam_args)) return GSR_ERR_INVALID_ARG;
    if (args->num_rows < 0 || args->num_tensors < 1 || args->num_tensors > GSR_ADAM_MAX_TENSORS) return GSR_ERR_INVALID_ARG;
    for (int k = 0; k < args->num_tensors; ++k) {
        const gsr_adam_tensor& t = args->tensors[k];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || t.row_floats <= 0) return GSR_ERR_INVALID_ARG;
        if (misaligned(t.param, 16) || misaligned(t.grad, 16) || misaligned(t.exp_avg, 16) || misaligned(t.exp_avg_sq, 16))
            return GSR_ERR_INVALID_ARG;
    }
    if (args->num_rows == 0) return GSR_OK;
    AdamParams q;
    q.n = args->num_rows;
    q.count = args->num_tensors;
    q.visible = args->visible;
    long long units = 0;
    for (int k = 0; k < GSR_ADAM_MAX_TENSORS; ++k) {
        AdamArray& a = q.a[k];
        if (k >= args->num_tensors) { a = AdamArray{}; a.unit_end = units; continue; }
        const gsr_adam_tensor& t = args->tensors[k];
        a.p = t.param; a.g = t.grad; a.m = t.exp_avg; a.v = t.exp_avg_sq;
        a.row_floats = t.row_floats;
        a.s = AdamScalars{t.step_size, t.rs, t.b1c, t.b2, t.b2c, t.eps};
        // rows per unit: 64 (one visibility word per lane), halved until the unit is at most 256 accesses
        const long long width = t.row_floats == 3 ? 1 : ((t.row_floats & 3) == 0 ? t.row_floats >> 2 : t.row_floats);
        a.rows = kWave;
        while (a.rows > 1 && a.rows * width > kUnitAccesses * kWave) a.rows >>= 1;
        units += (q.n + a.rows - 1) / a.rows;
        a.unit_end = units;
    }
    const long long blocks = (units + 3) / 4;
    if (exceeds_grid(blocks)) return GSR_ERR_TOO_LARGE;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)args->stream, q);
    GSR_LAUNCH_CHECK("adam_step_kernel");
    return GSR_OK;
}
extern "C" int gsr_adam_step(const gsr_adam_args* args) { return entry_point(adam_step_impl, args); }
