// Initialisation from a point cloud: the mean squared distance of every point to its three nearest neighbours
// (include/gsrast_amd_init.h states the result operation by operation; upstream: simple_knn's distCUDA2).
//
//   knn_bounds_kernel / knn_bounds_final_kernel   min and max of xyz, the cell size per axis
//   knn_code_kernel                               a 63-bit Morton code per point (21 bits an axis), sorted with value = index
//                                                 by eight onesweep passes (radix_sort.hip)
//   knn_gather_kernel                             the sorted points as (x, y, z, index) and the box of every 64 of them (a leaf)
//   knn_node_kernel                               the box of every GSR_KNN_NODE leaves (a node)
//   knn_search_kernel                             one wave per leaf, one query per lane: the exact search
//
// The code only ORDERS the work: whatever order the points get, the search below is exact, so the arithmetic of the code is
// free. No kernel here waits for another workgroup and none uses an atomic; the sort's look-back is the library's own.
#include "../../include/gsrast_amd_init.h"
#include "gsr_common.hpp"
#include "radix_sort.hpp"

namespace gsr {
namespace {

constexpr int kLeaf = GSR_KNN_LEAF;
constexpr int kNode = GSR_KNN_NODE;
static_assert(kLeaf == kWave, "a leaf is one wavefront's queries");
static_assert(kNode >= 1 && kNode <= kWave, "the leaves of a node are tested one per lane");
constexpr long long kKnnMaxPoints = GSR_KNN_MAX_POINTS;
constexpr int kBoundsBlocks = 1024;            // partial boxes at most
constexpr int kBoundsPerThread = 8;
constexpr uint32_t kCells = 1u << GSR_KNN_MORTON_BITS;
constexpr int kSearchWaves = 4;                // independent waves per workgroup of the search

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// temp, carved in this order (every part from a 128-byte boundary)
struct KnnTemp {
    float* partial;        // [kBoundsBlocks][8]: lo xyz, -, hi xyz, -
    float* grid;           // [8]: lo xyz, -, cells per unit xyz, -
    uint64_t *keys_a, *keys_b;
    uint32_t *vals_a, *vals_b;
    char* sweep;
    float4* sorted;        // [n]: x, y, z, the bits of the original index
    float4* leaf_box;      // [leaves][2]: lo, hi
    float4* node_box;      // [nodes][2]
    size_t bytes;
};

inline long long leaves_of(long long n) { return (n + kLeaf - 1) / kLeaf; }
inline long long nodes_of(long long n) { return (leaves_of(n) + kNode - 1) / kNode; }

// (base as an integer: gsr_knn_temp_bytes carves from 0 for the size alone)
KnnTemp carve_knn(uintptr_t base, long long n) {
    KnnTemp t;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = reinterpret_cast<char*>(base + off); off += align_up(bytes, 128); return p; };
    t.partial = reinterpret_cast<float*>(take((size_t)kBoundsBlocks * 8 * sizeof(float)));
    t.grid = reinterpret_cast<float*>(take(8 * sizeof(float)));
    t.keys_a = reinterpret_cast<uint64_t*>(take((size_t)n * sizeof(uint64_t)));
    t.keys_b = reinterpret_cast<uint64_t*>(take((size_t)n * sizeof(uint64_t)));
    t.vals_a = reinterpret_cast<uint32_t*>(take((size_t)n * sizeof(uint32_t)));
    t.vals_b = reinterpret_cast<uint32_t*>(take((size_t)n * sizeof(uint32_t)));
    t.sweep = take(sweep_scratch_bytes((size_t)n));
    t.sorted = reinterpret_cast<float4*>(take((size_t)n * sizeof(float4)));
    t.leaf_box = reinterpret_cast<float4*>(take((size_t)leaves_of(n) * 2 * sizeof(float4)));
    t.node_box = reinterpret_cast<float4*>(take((size_t)nodes_of(n) * 2 * sizeof(float4)));
    t.bytes = off;
    return t;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// The box of a workgroup's six per-lane values (lo xyz, hi xyz), left in out[0..7] by thread 0.
__device__ __forceinline__ void block_box(float lo[3], float hi[3], float* __restrict__ out) {
    __shared__ float part[4][8];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[wave][a] = lo[a]; part[wave][4 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out[a] = fminf(fminf(part[0][a], part[1][a]), fminf(part[2][a], part[3][a]));
            out[4 + a] = fmaxf(fmaxf(part[0][4 + a], part[1][4 + a]), fmaxf(part[2][4 + a], part[3][4 + a]));
        }
        out[3] = 0.0f;
        out[7] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void knn_bounds_kernel(const float* __restrict__ xyz, long long n, float* __restrict__ partial) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3 * i + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
    block_box(lo, hi, partial + 8 * (size_t)blockIdx.x);
}

// One workgroup: the box of the `blocks` partial boxes -> grid = {lo xyz, -, cells per unit xyz, -}. An axis without extent
// (or with one that is not finite) gets 0 cells per unit: all of its points fall into cell 0.
__global__ __launch_bounds__(256) void knn_bounds_final_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ grid) {
    __shared__ float box[8];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < blocks; b += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], partial[8 * b + a]);
            hi[a] = fmaxf(hi[a], partial[8 * b + 4 + a]);
        }
    }
    block_box(lo, hi, box);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float extent = box[4 + a] - box[a];
            const float per_unit = (float)kCells / extent;
            grid[a] = box[a];
            grid[4 + a] = (extent > 0.0f && per_unit < INFINITY) ? per_unit : 0.0f;      // (a NaN fails both comparisons)
        }
        grid[3] = 0.0f;
        grid[7] = 0.0f;
    }
}

// bit i of v -> bit 3 i (v < 2^21)
__device__ __forceinline__ unsigned long long spread3(uint32_t v) {
    unsigned long long x = v & 0x1FFFFFull;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// The cell of a coordinate: clamped as a float first, so that what is converted lies in [0, kCells - 1] whatever came in
// (fmaxf(NaN, 0) is 0).
__device__ __forceinline__ uint32_t cell_of(float v, float lo, float per_unit) {
    const float c = fminf(fmaxf((v - lo) * per_unit, 0.0f), (float)(kCells - 1u));
    return (uint32_t)c;
}

__global__ __launch_bounds__(256) void knn_code_kernel(const float* __restrict__ xyz, long long n, const float* __restrict__ grid,
                                                        unsigned long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t cx = cell_of(xyz[3 * i + 0], grid[0], grid[4]);
    const uint32_t cy = cell_of(xyz[3 * i + 1], grid[1], grid[5]);
    const uint32_t cz = cell_of(xyz[3 * i + 2], grid[2], grid[6]);
    keys[i] = spread3(cx) | (spread3(cy) << 1) | (spread3(cz) << 2);
}

// One wave per leaf: the points in sorted order and the leaf's box. The index is clamped: a sort whose bounded look-back gave
// up would leave words of temp as it found them, and nothing here may be used as an index unchecked.
__global__ __launch_bounds__(256) void knn_gather_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ order, long long n,
                                                          float4* __restrict__ sorted, float4* __restrict__ leaf_box) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long leaf = i >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const uint32_t last = (uint32_t)(n - 1);
        uint32_t src = order[i];
        src = src > last ? last : src;
        const float x = xyz[3 * (size_t)src + 0], y = xyz[3 * (size_t)src + 1], z = xyz[3 * (size_t)src + 2];
        sorted[i] = make_float4(x, y, z, __uint_as_float(src));
        lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
    }
    if (leaf * kLeaf >= n) return;             // (whole waves only: a leaf's first point exists or the wave has none)
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if ((threadIdx.x & 63) == 0) {
        leaf_box[2 * leaf] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        leaf_box[2 * leaf + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// One wave per node, one leaf per lane.
__global__ __launch_bounds__(256) void knn_node_kernel(const float4* __restrict__ leaf_box, long long leaves, long long nodes,
                                                        float4* __restrict__ node_box) {
    const long long node = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (node >= nodes) return;
    const int lane = threadIdx.x & 63;
    const long long leaf = node * kNode + lane;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (lane < kNode && leaf < leaves) {
        const float4 l = leaf_box[2 * leaf], h = leaf_box[2 * leaf + 1];
        lo[0] = l.x; lo[1] = l.y; lo[2] = l.z;
        hi[0] = h.x; hi[1] = h.y; hi[2] = h.z;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if (lane == 0) {
        node_box[2 * node] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        node_box[2 * node + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// The three smallest distances a lane has met, ascending; +inf where there is none yet.
struct Best3 {
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    // (b0 <= b1 <= b2 before and after: the smallest, the median of {b0, b1, d} and the median of {b1, b2, d})
    __device__ __forceinline__ void insert(float d) {
        const float n0 = fminf(b0, d), n1 = __builtin_amdgcn_fmed3f(b0, b1, d), n2 = __builtin_amdgcn_fmed3f(b1, b2, d);
        b0 = n0; b1 = n1; b2 = n2;
    }
};

// d2 of include/gsrast_amd_init.h. The library is built without contraction; the pragma says so once more where it matters.
__device__ __forceinline__ float dist2(float qx, float qy, float qz, float cx, float cy, float cz) {
#pragma clang fp contract(off)
    const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

// Why skipping a box is exact. Let Q = [qlo, qhi] be the box of the wave's 64 queries and B = [lo, hi] a box of candidates.
// Per axis, g = max(0, lo - qhi, qlo - hi), the two differences rounded to float32. For any query q in Q and candidate c in
// B the exact |q - c| is at least both exact differences, and rounding to nearest is monotone, so the ROUNDED |q - c| that
// dist2 squares is >= g >= 0. Rounded products and sums of non-negative floats are monotone in each operand as well, and
// gap2 below squares and sums the three g in the same order as dist2 does the three differences: gap2 <= d2(q, c) for every
// pair, in the computed values and not only in the real ones. `bound` is the largest third-best distance of the wave's
// queries at that moment, and a lane's third-best only shrinks. So with gap2 >= bound every candidate of B is >= the
// third-best of every query; inserting one that is EQUAL leaves the multiset {b0, b1, b2} as it is, which is why >= (and
// not >) may skip — and why a cloud of identical points prunes everything once bound is 0. An epsilon, another order of
// the sum or a fused multiply-add in gap2 would break the inequality in the last bit: there is none.
__device__ __forceinline__ float gap2(const float4 lo, const float4 hi, const float4 qlo, const float4 qhi) {
#pragma clang fp contract(off)
    const float gx = fmaxf(0.0f, fmaxf(lo.x - qhi.x, qlo.x - hi.x));
    const float gy = fmaxf(0.0f, fmaxf(lo.y - qhi.y, qlo.y - hi.y));
    const float gz = fmaxf(0.0f, fmaxf(lo.z - qhi.z, qlo.z - hi.z));
    return (gx * gx + gy * gy) + gz * gz;
}

// The same test per lane, behind the wave's: the box [lo, hi] (the same in every lane) against the lane's own point — Q is the
// point, qlo = qhi = q, and the argument above holds word for word — and the lane's OWN third-best. The box is skipped when
// no query lane has gap2 < b2. Needed where a leaf straddles a seam of the Morton order: its 64 points lie in two or more
// far-apart groups, Q spans what lies between and the wave's test alone lets everything through (measured: DESIGN_HISTORY.md).
__device__ __forceinline__ bool some_lane_may_gain(const float4 lo, const float4 hi, const float4 q, bool is_query, const Best3& best) {
    const float g = gap2(lo, hi, q, q);
    return __ballot(is_query && !(g >= best.b2)) != 0ull;
}

// All lanes walk the `count` points from `leaf_points` on: the address is the same in every lane, so the loads are scalar.
// kOwn: the wave's own leaf, where position j is lane j's own point (indices are compared, never positions).
template <bool kOwn>
__device__ __forceinline__ void scan_leaf(const float4* __restrict__ leaf_points, int count, int lane, float qx, float qy, float qz,
                                          Best3& best) {
    if (count == kLeaf) {
#pragma unroll 8
        for (int j = 0; j < kLeaf; ++j) {
            const float4 c = leaf_points[j];
            float d = dist2(qx, qy, qz, c.x, c.y, c.z);
            if (kOwn) d = j == lane ? INFINITY : d;
            best.insert(d);
        }
    } else {
        for (int j = 0; j < count; ++j) {
            const float4 c = leaf_points[j];
            float d = dist2(qx, qy, qz, c.x, c.y, c.z);
            if (kOwn) d = j == lane ? INFINITY : d;
            best.insert(d);
        }
    }
}

struct SearchArgs {
    const float4* sorted;
    const float4* leaf_box;
    const float4* node_box;
    float* mean_dist2;
    int n, leaves, nodes;
};

// The largest third-best distance of the wave's queries, the same value in every lane and known to be so.
__device__ __forceinline__ float wave_bound(bool is_query, const Best3& best) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wave_max(is_query ? best.b2 : 0.0f))));
}

__global__ __launch_bounds__(64 * kSearchWaves) void knn_search_kernel(const SearchArgs a) {
    // everything that steers a loop below is the same in all lanes of a wave: the leaf, the ballots, the bound
    const int leaf = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kSearchWaves + (threadIdx.x >> 6)));
    if (leaf >= a.leaves) return;
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ sorted = a.sorted;
    const float4* __restrict__ leaf_box = a.leaf_box;
    const float4* __restrict__ node_box = a.node_box;
    const int first = leaf * kLeaf;
    const bool is_query = first + lane < a.n;
    const float4 q = sorted[is_query ? first + lane : a.n - 1];        // (a lane without a query computes on, and writes nothing)
    const float4 qlo = leaf_box[2 * leaf], qhi = leaf_box[2 * leaf + 1];
    auto count_of = [&](int l) { const int left = a.n - l * kLeaf; return left < kLeaf ? left : kLeaf; };
    Best3 best;

    // the seed: the wave's own leaf and its two neighbours in sorted order, unconditionally
    const int seed_lo = leaf > 0 ? leaf - 1 : 0, seed_hi = leaf + 1 < a.leaves ? leaf + 1 : a.leaves - 1;
    scan_leaf<true>(sorted + (size_t)first, count_of(leaf), lane, q.x, q.y, q.z, best);
    if (seed_lo != leaf) scan_leaf<false>(sorted + (size_t)seed_lo * kLeaf, kLeaf, lane, q.x, q.y, q.z, best);
    if (seed_hi != leaf) scan_leaf<false>(sorted + (size_t)seed_hi * kLeaf, count_of(seed_hi), lane, q.x, q.y, q.z, best);
    float bound = wave_bound(is_query, best);

    // The leaves of one node, one per lane: those outside the seed whose box may hold something nearer, in ascending order.
    // The gap of a leaf is tested again against the bound as it is when its turn comes.
    auto visit_node = [&](int node) {
        const int l = node * kNode + lane;
        const bool there = lane < kNode && l < a.leaves && (l < seed_lo || l > seed_hi);
        float g = INFINITY;
        if (there) g = gap2(leaf_box[2 * l], leaf_box[2 * l + 1], qlo, qhi);
        // (`there` stands beside the comparison: with a NaN about, no comparison may be what keeps an index inside the arrays)
        for (unsigned long long m = __ballot(there && !(g >= bound)); m != 0ull; m &= m - 1ull) {
            const int bit = __ffsll((long long)m) - 1;
            const float gl = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(g), bit));
            if (gl >= bound) continue;
            const int cl = node * kNode + bit;
            if (!some_lane_may_gain(leaf_box[2 * cl], leaf_box[2 * cl + 1], q, is_query, best)) continue;
            scan_leaf<false>(sorted + (size_t)cl * kLeaf, count_of(cl), lane, q.x, q.y, q.z, best);
            bound = wave_bound(is_query, best);
        }
    };

    // the wave's own node first: it shrinks the bound the most
    const int own_node = leaf / kNode;
    visit_node(own_node);
    // then every other node, 64 tested at a time
    for (int base = 0; base < a.nodes; base += kWave) {
        const int nd = base + lane;
        const bool there = nd < a.nodes && nd != own_node;
        float g = INFINITY;
        if (there) g = gap2(node_box[2 * nd], node_box[2 * nd + 1], qlo, qhi);
        for (unsigned long long m = __ballot(there && !(g >= bound)); m != 0ull; m &= m - 1ull) {
            const int bit = __ffsll((long long)m) - 1;
            const float gn = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(g), bit));
            if (gn >= bound) continue;
            const int nd_u = base + bit;
            if (!some_lane_may_gain(node_box[2 * nd_u], node_box[2 * nd_u + 1], q, is_query, best)) continue;
            visit_node(nd_u);
        }
    }

    if (!is_query) return;
    float r;
    if (a.n >= 4) r = ((best.b0 + best.b1) + best.b2) / 3.0f;
    else if (a.n == 3) r = (best.b0 + best.b1) / 2.0f;
    else if (a.n == 2) r = best.b0;
    else r = 0.0f;
    a.mean_dist2[__float_as_uint(q.w)] = r;                            // (the index was clamped to n - 1 by the gather)
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" size_t gsr_knn_temp_bytes(int64_t n) {
    if (n < 0 || n > kKnnMaxPoints) return 0;
    return carve_knn(0, n > 0 ? n : 1).bytes;
}

static int knn_mean_dist2_impl(int64_t n, const float* xyz, float* mean_dist2, void* temp, void* stream) {
    if (n < 0 || (n > 0 && (!xyz || !mean_dist2 || !temp))) return GSR_ERR_INVALID_ARG;
    if (misaligned(xyz, 4) || misaligned(mean_dist2, 4) || misaligned(temp, 16)) return GSR_ERR_INVALID_ARG;
    if (n > kKnnMaxPoints) return GSR_ERR_TOO_LARGE;
    if (n == 0) return GSR_OK;
    const hipStream_t st = (hipStream_t)stream;
    const KnnTemp t = carve_knn(reinterpret_cast<uintptr_t>(temp), n);
    const long long leaves = leaves_of(n), nodes = nodes_of(n);
    const auto blocks_of = [](long long threads) { return dim3((unsigned)((threads + 255) / 256)); };

    const long long want = (n + 256ll * kBoundsPerThread - 1) / (256ll * kBoundsPerThread);
    const int bounds_blocks = (int)(want < kBoundsBlocks ? want : kBoundsBlocks);
    hipLaunchKernelGGL(knn_bounds_kernel, dim3(bounds_blocks), dim3(256), 0, st, xyz, (long long)n, t.partial);
    GSR_LAUNCH_CHECK("knn_bounds_kernel");
    hipLaunchKernelGGL(knn_bounds_final_kernel, dim3(1), dim3(256), 0, st, t.partial, bounds_blocks, t.grid);
    GSR_LAUNCH_CHECK("knn_bounds_final_kernel");
    hipLaunchKernelGGL(knn_code_kernel, blocks_of(n), dim3(256), 0, st, xyz, (long long)n, t.grid,
                       reinterpret_cast<unsigned long long*>(t.keys_a));
    GSR_LAUNCH_CHECK("knn_code_kernel");

    // eight stable 8-bit passes, a -> b -> a ...: the order ends in vals_a (the first pass's value is the point's index)
    SweepScratch sc = carve_sweep_scratch(t.sweep, (size_t)n);
    GSR_HIP_TRY(hipMemsetAsync(sc.error_word, 0, sizeof(uint32_t), st));
    GSR_TRY(histogram_bits_u64(t.keys_a, (size_t)n, 0, 64, sc.hist, st));
    for (int p = 0; p < 8; ++p) {
        const bool from_a = (p % 2) == 0;
        DigitSpec spec;
        spec.mode = kDigitBits;
        spec.shift = 8 * p;
        spec.nbins = 256;
        spec.grid_x = 1;
        spec.inv_grid_x = 1.0f;
        GSR_TRY(sweep_pass_u64(from_a ? t.keys_a : t.keys_b, p == 0 ? nullptr : (from_a ? t.vals_a : t.vals_b),
                               from_a ? t.keys_b : t.keys_a, from_a ? t.vals_b : t.vals_a, (uint32_t)n, spec, sc.hist + 256 * p, sc, st));
    }

    hipLaunchKernelGGL(knn_gather_kernel, blocks_of(leaves * kLeaf), dim3(256), 0, st, xyz, t.vals_a, (long long)n, t.sorted, t.leaf_box);
    GSR_LAUNCH_CHECK("knn_gather_kernel");
    hipLaunchKernelGGL(knn_node_kernel, blocks_of(nodes * kWave), dim3(256), 0, st, t.leaf_box, leaves, nodes, t.node_box);
    GSR_LAUNCH_CHECK("knn_node_kernel");
    const SearchArgs sa{t.sorted, t.leaf_box, t.node_box, mean_dist2, (int)n, (int)leaves, (int)nodes};
    hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)((leaves + kSearchWaves - 1) / kSearchWaves)), dim3(64 * kSearchWaves), 0, st, sa);
    GSR_LAUNCH_CHECK("knn_search_kernel");
    return GSR_OK;
}
extern "C" int gsr_knn_mean_dist2(int64_t n, const float* xyz, float* mean_dist2, void* temp, void* stream) {
    return entry_point(knn_mean_dist2_impl, n, xyz, mean_dist2, temp, stream);
}
