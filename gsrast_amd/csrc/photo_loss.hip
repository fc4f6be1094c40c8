// gsr_photo_loss_forward / _backward: (1 - lambda) * L1 + lambda * (1 - SSIM) of an image against a target, and its gradient
// with respect to the image (include/gsrast_amd.h states the arithmetic and its order).
//
// A workgroup of 256 threads owns a tile of kTH x kTW = 16 x 64 pixels of one channel. It stages the tile with its halo of
// five pixels in LDS — rows in 16-byte vectors from the 16-byte boundary left of the halo when the image's rows are whole
// vectors (width % 4 == 0), float by float otherwise; what lies outside the image is stored as 0.0f, so a tap there adds
// g[k] * 0 — runs the horizontal pass from LDS into LDS (one thread per float: lanes along a row, no bank conflict) and the
// vertical pass from LDS into registers (a thread owns four rows of one column: fourteen reads feed four sums).
//   forward   convolves x, y, x*x, y*y, x*y (the products are formed per tap, never stored), forms the SSIM map and its
//             three derivative maps per pixel, sums |x - y| and m in double (thread, wave, workgroup: one partial pair per
//             workgroup, no atomics) and, when a backward will follow, stores t_mu, d_s11, d_s12 to scratch.
//   finalize  one workgroup sums the partial pairs in a fixed order and writes (loss, l1, ssim).
//   backward  the same two passes over the three stored maps, then dL_dimage per pixel; `up` is read from device memory.
// The maps make a round trip through HBM (36 bytes per image float in all) rather than being recomputed from a halo of ten:
// without contraction the passes are bound by their VALU work, which a recompute would repeat 2.6 times per tile.
// No result depends on the tile shape: every float is a fixed sequence of operations on the image, and between workgroups
// only the double partial sums are combined.
#include "gsr_common.hpp"

namespace gsr {
namespace {

constexpr int kTW = 64, kTH = 16;         // the tile
constexpr int kRadius = 5, kTaps = 11;
constexpr int kRows = kTH + 2 * kRadius;  // staged rows: image rows r0 - 5 ..
constexpr int kLW = kTW + 16;             // staged columns: image columns c0 - 8 .. (the halo begins at LDS column 3)
constexpr int kHalo0 = 8 - kRadius;
constexpr int kThreads = 256;
constexpr int kRowsPerThread = kTH / (kThreads / kTW);        // 4
constexpr int kSpan = kRowsPerThread + kTaps - 1;             // 14

__device__ __forceinline__ float tap(int k) {
    constexpr float g[kTaps] = GSR_PHOTO_LOSS_WINDOW;
    return g[k];
}

struct PhotoParams {
    int width, height;
    long long plane;                      // width * height
    const float* image;
    const float* target;
    double* partials;                     // [workgroup][2]
    float* maps;                          // t_mu | d_s11 | d_s12, each channels * plane floats
    long long map_floats;                 // channels * plane
    int want_backward;
    const float* up;
    float* dL_dimage;
    float cs, cl;
};

// Stages image rows r0 - 5 .. r0 + kTH + 4, columns c0 - 8 .. c0 + kTW + 7 of the plane at `src`; zeros outside the image.
template <bool VEC>
__device__ __forceinline__ void stage_tile(float (*dst)[kLW], const float* __restrict__ src, int width, int height, int r0, int c0, int tid) {
    if (VEC) {
        constexpr int kVecs = kLW / 4;
        for (int v = tid; v < kRows * kVecs; v += kThreads) {
            const int i = v / kVecs, j = 4 * (v % kVecs);
            const int r = r0 - kRadius + i, c = c0 - 8 + j;
            float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            // (width % 4 == 0 and c % 4 == 0: a vector lies wholly inside a row or wholly outside)
            if (r >= 0 && r < height && c >= 0 && c < width) val = *reinterpret_cast<const float4*>(src + (long long)r * width + c);
            *reinterpret_cast<float4*>(&dst[i][j]) = val;
        }
    } else {
        for (int e = tid; e < kRows * kLW; e += kThreads) {
            const int i = e / kLW, j = e % kLW;
            const int r = r0 - kRadius + i, c = c0 - 8 + j;
            float val = 0.0f;
            if (r >= 0 && r < height && c >= 0 && c < width) val = src[(long long)r * width + c];
            dst[i][j] = val;
        }
    }
}

// The vertical pass of one quantity for this thread's four rows: hs rows base .. base + 13 of column col.
__device__ __forceinline__ void vertical(const float (*hs)[kTW], int base, int col, float (&out)[kRowsPerThread]) {
    float v[kSpan];
#pragma unroll
    for (int j = 0; j < kSpan; ++j) v[j] = hs[base + j][col];
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) acc = acc + tap(k) * v[j + k];
        out[j] = acc;
    }
}

// The workgroup's sum of (a, b), in a fixed order: lanes by halving, then the four waves in turn. Valid in thread 0.
__device__ __forceinline__ void block_sum(double& a, double& b, double (*red)[kThreads / kWave], int tid) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a = a + __shfl_down(a, off, kWave);
        b = b + __shfl_down(b, off, kWave);
    }
    if ((tid & (kWave - 1)) == 0) { red[0][tid / kWave] = a; red[1][tid / kWave] = b; }
    __syncthreads();
    if (tid == 0) {
        a = red[0][0]; b = red[1][0];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; ++w) { a = a + red[0][w]; b = b + red[1][w]; }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void photo_loss_forward_kernel(const PhotoParams q) {
    __shared__ __attribute__((aligned(16))) float xs[kRows][kLW];
    __shared__ __attribute__((aligned(16))) float ys[kRows][kLW];
    __shared__ float hs[5][kRows][kTW];                                      // conv_h of x, y, x*x, y*y, x*y
    __shared__ double red[2][kThreads / kWave];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kTW, r0 = blockIdx.y * kTH;
    const long long channel = (long long)blockIdx.z * q.plane;
    stage_tile<VEC>(xs, q.image + channel, q.width, q.height, r0, c0, tid);
    stage_tile<VEC>(ys, q.target + channel, q.width, q.height, r0, c0, tid);
    __syncthreads();
    // ---- horizontal ----
    for (int i = tid; i < kRows * kTW; i += kThreads) {
        const int row = i / kTW, col = i % kTW;
        const float* xr = &xs[row][col + kHalo0];
        const float* yr = &ys[row][col + kHalo0];
        float ax = 0.0f, ay = 0.0f, axx = 0.0f, ayy = 0.0f, axy = 0.0f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float x = xr[k], y = yr[k], g = tap(k);
            ax = ax + g * x;
            ay = ay + g * y;
            axx = axx + g * (x * x);
            ayy = ayy + g * (y * y);
            axy = axy + g * (x * y);
        }
        hs[0][row][col] = ax; hs[1][row][col] = ay; hs[2][row][col] = axx; hs[3][row][col] = ayy; hs[4][row][col] = axy;
    }
    __syncthreads();
    // ---- vertical, then the pixel ----
    const int col = tid % kTW, base = kRowsPerThread * (tid / kTW);
    float mu1[kRowsPerThread], mu2[kRowsPerThread], cxx[kRowsPerThread], cyy[kRowsPerThread], cxy[kRowsPerThread];
    vertical(hs[0], base, col, mu1);
    vertical(hs[1], base, col, mu2);
    vertical(hs[2], base, col, cxx);
    vertical(hs[3], base, col, cyy);
    vertical(hs[4], base, col, cxy);
    constexpr float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);                               // (double products, rounded once)
    const int c = c0 + col;
    double l1 = 0.0, ssim = 0.0;
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
        const int r = r0 + base + j;
        if (r >= q.height || c >= q.width) continue;
        const float x = xs[base + j + kRadius][col + 8], y = ys[base + j + kRadius][col + 8];
        const float m1 = mu1[j], m2 = mu2[j];
        const float s11 = cxx[j] - m1 * m1, s22 = cyy[j] - m2 * m2, s12 = cxy[j] - m1 * m2;
        const float a1 = 2.0f * (m1 * m2) + C1, a2 = 2.0f * s12 + C2;
        const float b1 = (m1 * m1 + m2 * m2) + C1, b2 = (s11 + s22) + C2;
        const float b12 = b1 * b2;
        const float m = (a1 * a2) / b12;
        l1 = l1 + (double)fabsf(x - y);
        ssim = ssim + (double)m;
        if (q.want_backward) {
            const float d_s12 = (2.0f * a1) / b12;
            const float d_s11 = -(m / b2);
            const float d_mu1 = (2.0f * m2 * a2) / b12 - (2.0f * m1 * m) / b1;
            const float t_mu = (d_mu1 - 2.0f * m1 * d_s11) - m2 * d_s12;
            float* at = q.maps + channel + (long long)r * q.width + c;
            at[0] = t_mu;
            at[q.map_floats] = d_s11;
            at[2 * q.map_floats] = d_s12;
        }
    }
    block_sum(l1, ssim, red, tid);
    if (tid == 0) {
        const long long wg = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        q.partials[2 * wg] = l1;
        q.partials[2 * wg + 1] = ssim;
    }
}

__global__ __launch_bounds__(kThreads) void photo_loss_finalize_kernel(const double* __restrict__ partials, long long workgroups, double n,
                                                                       double lambda, float* __restrict__ out) {
    __shared__ double red[2][kThreads / kWave];
    const int tid = threadIdx.x;
    double l1 = 0.0, ssim = 0.0;
    for (long long i = tid; i < workgroups; i += kThreads) {
        l1 = l1 + partials[2 * i];
        ssim = ssim + partials[2 * i + 1];
    }
    block_sum(l1, ssim, red, tid);
    if (tid == 0) {
        l1 = l1 / n;
        ssim = ssim / n;
        const double loss = (1.0 - lambda) * l1 + lambda * (1.0 - ssim);
        out[0] = (float)loss;
        out[1] = (float)l1;
        out[2] = (float)ssim;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void photo_loss_backward_kernel(const PhotoParams q) {
    __shared__ __attribute__((aligned(16))) float ms[3][kRows][kLW];         // t_mu, d_s11, d_s12
    __shared__ float hs[3][kRows][kTW];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kTW, r0 = blockIdx.y * kTH;
    const long long channel = (long long)blockIdx.z * q.plane;
#pragma unroll
    for (int t = 0; t < 3; ++t) stage_tile<VEC>(ms[t], q.maps + t * q.map_floats + channel, q.width, q.height, r0, c0, tid);
    __syncthreads();
    for (int i = tid; i < kRows * kTW; i += kThreads) {
        const int row = i / kTW, col = i % kTW;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const float* mr = &ms[t][row][col + kHalo0];
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) acc = acc + tap(k) * mr[k];
            hs[t][row][col] = acc;
        }
    }
    __syncthreads();
    const int col = tid % kTW, base = kRowsPerThread * (tid / kTW);
    float c_mu[kRowsPerThread], c_s11[kRowsPerThread], c_s12[kRowsPerThread];
    vertical(hs[0], base, col, c_mu);
    vertical(hs[1], base, col, c_s11);
    vertical(hs[2], base, col, c_s12);
    const float up = *q.up;
    const int c = c0 + col;
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
        const int r = r0 + base + j;
        if (r >= q.height || c >= q.width) continue;
        const long long at = channel + (long long)r * q.width + c;
        const float x = q.image[at], y = q.target[at];
        const float S = (c_mu[j] + 2.0f * x * c_s11[j]) + y * c_s12[j];
        const float d = x - y;
        const float sgn = (float)(d > 0.0f) - (float)(d < 0.0f);
        q.dL_dimage[at] = up * (q.cs * S + q.cl * sgn);
    }
}

struct PhotoShape {
    long long tiles_x, tiles_y, workgroups, floats;
};

// GSR_OK, or why a call with these sizes is refused.
int photo_shape(int channels, int width, int height, PhotoShape* s) {
    if (channels < 1 || width < 1 || height < 1) return GSR_ERR_INVALID_ARG;
    const long long plane = (long long)width * height;
    if (plane > 0x7FFFFFFFll) return GSR_ERR_TOO_LARGE;          // (and the next product cannot overflow)
    s->floats = plane * channels;
    s->tiles_x = (width + kTW - 1) / kTW;
    s->tiles_y = (height + kTH - 1) / kTH;
    s->workgroups = s->tiles_x * s->tiles_y * channels;
    if (s->floats > 0x7FFFFFFFll || s->tiles_y > 65535 || channels > 65535) return GSR_ERR_TOO_LARGE;
    return GSR_OK;
}

// What both calls refuse, and the parameters both kernels take.
int photo_params(const gsr_photo_loss_args* a, PhotoShape* s, PhotoParams* q) {
    if (!a || a->struct_size != sizeof(gsr_photo_loss_args)) return GSR_ERR_INVALID_ARG;
    if (!(a->lambda_dssim >= 0.0 && a->lambda_dssim <= 1.0)) return GSR_ERR_INVALID_ARG;
    if (!a->image || !a->target || !a->scratch) return GSR_ERR_INVALID_ARG;
    if (misaligned(a->image, 16) || misaligned(a->target, 16) || misaligned(a->scratch, 16)) return GSR_ERR_INVALID_ARG;
    GSR_TRY(photo_shape(a->channels, a->width, a->height, s));
    q->width = a->width;
    q->height = a->height;
    q->plane = (long long)a->width * a->height;
    q->image = a->image;
    q->target = a->target;
    q->partials = static_cast<double*>(a->scratch);
    q->maps = reinterpret_cast<float*>(static_cast<char*>(a->scratch) + 16 * s->workgroups);
    q->map_floats = s->floats;
    q->want_backward = a->want_backward;
    q->up = a->dL_dloss;
    q->dL_dimage = a->dL_dimage;
    const double n = (double)s->floats;
    q->cs = (float)(-a->lambda_dssim / n);
    q->cl = (float)((1.0 - a->lambda_dssim) / n);
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" size_t gsr_photo_loss_scratch_bytes(int channels, int width, int height) {
    PhotoShape s;
    if (photo_shape(channels, width, height, &s) != GSR_OK) return 0;
    return (size_t)(16 * s.workgroups + 3 * 4 * s.floats);        // partial pairs, then the three maps (16-byte aligned: the pairs are)
}

static int photo_loss_forward_impl(const gsr_photo_loss_args* args) {
    PhotoShape s;
    PhotoParams q;
    GSR_TRY(photo_params(args, &s, &q));
    if (!args->out || misaligned(args->out, 4)) return GSR_ERR_INVALID_ARG;
    const hipStream_t stream = (hipStream_t)args->stream;
    const dim3 grid((unsigned)s.tiles_x, (unsigned)s.tiles_y, (unsigned)args->channels);
    if ((args->width & 3) == 0) hipLaunchKernelGGL(photo_loss_forward_kernel<true>, grid, dim3(kThreads), 0, stream, q);
    else hipLaunchKernelGGL(photo_loss_forward_kernel<false>, grid, dim3(kThreads), 0, stream, q);
    GSR_LAUNCH_CHECK("photo_loss_forward_kernel");
    hipLaunchKernelGGL(photo_loss_finalize_kernel, dim3(1), dim3(kThreads), 0, stream, q.partials, s.workgroups, (double)s.floats,
                       args->lambda_dssim, args->out);
    GSR_LAUNCH_CHECK("photo_loss_finalize_kernel");
    return GSR_OK;
}
extern "C" int gsr_photo_loss_forward(const gsr_photo_loss_args* args) { return entry_point(photo_loss_forward_impl, args); }

static int photo_loss_backward_impl(const gsr_photo_loss_args* args) {
    PhotoShape s;
    PhotoParams q;
    GSR_TRY(photo_params(args, &s, &q));
    if (!args->dL_dloss || misaligned(args->dL_dloss, 4) || !args->dL_dimage || misaligned(args->dL_dimage, 16))
        return GSR_ERR_INVALID_ARG;
    const hipStream_t stream = (hipStream_t)args->stream;
    const dim3 grid((unsigned)s.tiles_x, (unsigned)s.tiles_y, (unsigned)args->channels);
    if ((args->width & 3) == 0) hipLaunchKernelGGL(photo_loss_backward_kernel<true>, grid, dim3(kThreads), 0, stream, q);
    else hipLaunchKernelGGL(photo_loss_backward_kernel<false>, grid, dim3(kThreads), 0, stream, q);
    GSR_LAUNCH_CHECK("photo_loss_backward_kernel");
    return GSR_OK;
}
extern "C" int gsr_photo_loss_backward(const gsr_photo_loss_args* args) { return entry_point(photo_loss_backward_impl, args); }
