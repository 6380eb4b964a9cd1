// StyleGAN2's projector (dge_amd.projector): Adam with a first moment as one multi-tensor launch, the single W code broadcast to
// the rows of W+ with its adjoint, the statistics of mapped samples (w_avg, w_std) and the adjoint of the area pooling in front of
// LPIPS.  All f32.  Nothing here uses atomics or a pre-zeroed buffer: partial sums go to slots of their own and are added in a
// fixed order, so the bits are the same from run to run, in both reduction modes, and for a row alone or inside a batch.
#include "common.h"
#include "../../include/dge_hip.h"

namespace {

// ------------------------------------------------------------------ Adam
#define PADAM_MAX_TENSORS 48
struct PAdamTable {
    float* p[PADAM_MAX_TENSORS];
    const float* g[PADAM_MAX_TENSORS];
    float* m[PADAM_MAX_TENSORS];
    float* v[PADAM_MAX_TENSORS];
    long n[PADAM_MAX_TENSORS];
};

// one element of torch.optim.Adam's update; the host's two step scalars: step = lr / (1 - beta1^t), isb = 1 / sqrt(1 - beta2^t)
struct AdamCoef { float b1, omb1, b2, omb2, eps; };          // omb = 1 - beta, rounded from the double
// Every rounding is spelled out (the compiler contracts a * b + c differently in the two loops below): an element gets the same
// bits whichever loop takes it, i.e. wherever its tensor starts and whatever shares the launch.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamCoef& c, float step, float isb) {
    m = __fmaf_rn(c.b1, m, __fmul_rn(c.omb1, g));
    v = __fmaf_rn(c.b2, v, __fmul_rn(__fmul_rn(c.omb2, g), g));
    p = __fmaf_rn(-step, __fdiv_rn(m, __fmaf_rn(__fsqrt_rn(v), isb, c.eps)), p);
}

__global__ __launch_bounds__(256) void adam_multi_kernel(PAdamTable t, AdamCoef c, float step, float isb, const float* __restrict__ scalars) {
    const int ti = blockIdx.y;
    float* __restrict__ p = t.p[ti]; const float* __restrict__ g = t.g[ti];
    float* __restrict__ m = t.m[ti]; float* __restrict__ v = t.v[ti];
    const long n = t.n[ti];
    if (scalars) { step = scalars[0]; isb = scalars[1]; }
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
    const long n4 = vec ? n >> 2 : 0;
    const long stride = gridDim.x * 256L, first = blockIdx.x * 256L + threadIdx.x;
    for (long i = first; i < n4; i += stride) {
        float4 pp = ((float4*)p)[i], mm = ((float4*)m)[i], vv = ((float4*)v)[i];
        const float4 gg = ((const float4*)g)[i];
        adam_elem(pp.x, gg.x, mm.x, vv.x, c, step, isb);
        adam_elem(pp.y, gg.y, mm.y, vv.y, c, step, isb);
        adam_elem(pp.z, gg.z, mm.z, vv.z, c, step, isb);
        adam_elem(pp.w, gg.w, mm.w, vv.w, c, step, isb);
        ((float4*)p)[i] = pp; ((float4*)m)[i] = mm; ((float4*)v)[i] = vv;
    }
    for (long i = (n4 << 2) + first; i < n; i += stride) {          // the ragged tail, or a tensor that is not 16-byte aligned
        float pp = p[i], mm = m[i], vv = v[i];
        adam_elem(pp, g[i], mm, vv, c, step, isb);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

// ------------------------------------------------------------------ W -> W+ and back
// a * b rounded, then + c rounded: torch's `w + noise * scale`.  (__fadd_rn(__fmul_rn()) are plain operators to the compiler, which
// contracts them into one fma under the default -ffp-contract=fast; the pragma takes the contraction off for this body.)
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
    const float p = a * b;
    return p + c;
}
__global__ __launch_bounds__(256) void w_broadcast_kernel(const float* __restrict__ w, const float* __restrict__ noise, float scale,
                                                           const float* __restrict__ scale_dev, float* __restrict__ ws, int L, int D, long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const long b = i / ((long)L * D);
    const int d = (int)(i % D);
    if (scale_dev) scale = scale_dev[0];
    float v = w[b * D + d];
    if (noise) v = mul_then_add(noise[b * D + d], scale, v);
    ws[i] = v;
}

__global__ __launch_bounds__(256) void w_broadcast_bwd_kernel(const float* __restrict__ g_ws, float* __restrict__ g_w, int L, int D, long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;          // (b, d)
    if (i >= n) return;
    const long b = i / D;
    const int d = (int)(i % D);
    const float* q = g_ws + b * L * D + d;
    float acc = 0.f;
    for (int l = 0; l < L; l++) acc = __fadd_rn(acc, q[(long)l * D]);
    g_w[i] = acc;
}

// ------------------------------------------------------------------ w_avg / w_std
constexpr int kRows = 64;          // rows of a chunk; a workgroup takes 1024 of its columns (256 threads x 4)

// slot[chunk][d] <- sum of column d over the chunk's rows, ascending
__global__ __launch_bounds__(256) void rows_colsum_kernel(const float* __restrict__ x, long long N, int D, float* __restrict__ slots) {
    const int c4 = blockIdx.y * 256 + threadIdx.x;
    if (c4 * 4 >= D) return;
    const long long r0 = (long long)blockIdx.x * kRows, r1 = r0 + kRows < N ? r0 + kRows : N;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long r = r0; r < r1; r++) {
        const float4 v = *(const float4*)(x + r * D + c4 * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *(float4*)(slots + (size_t)blockIdx.x * D + c4 * 4) = s;
}
// mean[d] <- (sum of the chunk slots of column d, in slot order) / N
__global__ __launch_bounds__(256) void rows_mean_kernel(const float* __restrict__ slots, int nch, long long N, int D, float* __restrict__ mean) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    float s = 0.f;
    for (int c = 0; c < nch; c++) s += slots[(size_t)c * D + d];
    mean[d] = s / (float)N;
}
// dev[chunk][column block] <- sum over the chunk's rows and the block's columns of (x - mean)^2: the thread's four columns row by
// row in one accumulator, the threads by the butterfly, the waves in index order
__global__ __launch_bounds__(256) void rows_sqdev_kernel(const float* __restrict__ x, const float* __restrict__ mean, long long N, int D,
                                                          float* __restrict__ dev) {
    __shared__ float red[4];
    const int c4 = blockIdx.y * 256 + threadIdx.x;
    const long long r0 = (long long)blockIdx.x * kRows, r1 = r0 + kRows < N ? r0 + kRows : N;
    float s = 0.f;
    if (c4 * 4 < D) {
        const float4 mu = *(const float4*)(mean + c4 * 4);
        for (long long r = r0; r < r1; r++) {
            const float4 v = *(const float4*)(x + r * D + c4 * 4);
            const float a = v.x - mu.x, b = v.y - mu.y, c = v.z - mu.z, e = v.w - mu.w;
            s += (a * a + b * b) + (c * c + e * e);
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) dev[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = (red[0] + red[1]) + (red[2] + red[3]);
}
// std[0] <- sqrt(sum of the n deviations / N): one workgroup, thread-strided partial sums, butterfly, waves in index order
__global__ __launch_bounds__(256) void rows_std_kernel(const float* __restrict__ dev, long long n, long long N, float* __restrict__ std) {
    __shared__ float red[4];
    float s = 0.f;
    for (long long k = threadIdx.x; k < n; k += 256) s += dev[k];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) std[0] = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)N);
}

inline long long mean_std_chunks(long long N) { return (N + kRows - 1) / kRows; }
inline int mean_std_colblocks(int D) { return (D / 4 + 255) / 256; }

// ------------------------------------------------------------------ area pooling, adjoint
__global__ __launch_bounds__(256) void area_pool_bwd_kernel(const float* __restrict__ gp, float* __restrict__ g, int H, int W, int k, long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const long bc = i / ((long)W * H);
    const int hp = H / k, wp = W / k;
    g[i] = __fdiv_rn(gp[(bc * hp + y / k) * wp + x / k], (float)(k * k));
}

}  // namespace

// =================================================================== C ABI
extern "C" int dge_adam_multi(int ntensors, float* const* host_p, const float* const* host_g, float* const* host_m, float* const* host_v,
                              const long* host_n, double beta1, double beta2, float eps, float step, float inv_sqrt_bc2,
                              const float* scalars_dev, hipStream_t s) {
    DGE_CHECK(ntensors >= 0 && (ntensors == 0 || (host_p && host_g && host_m && host_v && host_n)), "adam_multi: bad tensor table");
    DGE_CHECK(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps > 0.f, "adam_multi: betas in [0, 1), eps > 0");
    const AdamCoef c = {(float)beta1, (float)(1. - beta1), (float)beta2, (float)(1. - beta2), eps};
    for (int base = 0; base < ntensors; base += PADAM_MAX_TENSORS) {
        PAdamTable t;
        const int cnt = ntensors - base < PADAM_MAX_TENSORS ? ntensors - base : PADAM_MAX_TENSORS;
        long maxn = 0;
        for (int i = 0; i < cnt; i++) {
            t.p[i] = host_p[base + i]; t.g[i] = host_g[base + i]; t.m[i] = host_m[base + i]; t.v[i] = host_v[base + i];
            t.n[i] = host_n[base + i];
            DGE_CHECK(t.n[i] >= 0 && (t.n[i] == 0 || (t.p[i] && t.g[i] && t.m[i] && t.v[i])), "adam_multi: tensor %d: null pointer or negative size", base + i);
            if (t.n[i] > maxn) maxn = t.n[i];
        }
        long gx = (maxn / 4 + 255) / 256; if (gx > 2048) gx = 2048; if (gx < 1) gx = 1;
        hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)gx, cnt), dim3(256), 0, s, t, c, step, inv_sqrt_bc2, scalars_dev);
        DGE_LAUNCH_CHECK("adam_multi");
    }
    dge_note_kernel("adam_multi");
    return 0;
}

extern "C" int dge_w_broadcast(const float* w, const float* noise, float scale, const float* scale_dev, float* ws, int B, int L, int D,
                               hipStream_t s) {
    DGE_CHECK(w && ws && B >= 1 && L >= 1 && D >= 1, "w_broadcast: bad arguments (B %d, L %d, D %d)", B, L, D);
    const long n = (long)B * L * D;
    DGE_CHECK((n + 255) / 256 < (1L << 31), "w_broadcast: too many elements");
    hipLaunchKernelGGL(w_broadcast_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, noise, scale, scale_dev, ws, L, D, n);
    DGE_LAUNCH_CHECK("w_broadcast");
    dge_note_kernel("w_broadcast");
    return 0;
}

extern "C" int dge_w_broadcast_bwd(const float* g_ws, float* g_w, int B, int L, int D, hipStream_t s) {
    DGE_CHECK(g_ws && g_w && B >= 1 && L >= 1 && D >= 1, "w_broadcast_bwd: bad arguments (B %d, L %d, D %d)", B, L, D);
    const long n = (long)B * D;
    DGE_CHECK((n + 255) / 256 < (1L << 31), "w_broadcast_bwd: too many elements");
    hipLaunchKernelGGL(w_broadcast_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g_ws, g_w, L, D, n);
    DGE_LAUNCH_CHECK("w_broadcast_bwd");
    dge_note_kernel("w_broadcast_bwd");
    return 0;
}

extern "C" int dge_rows_mean_std_work_bytes(long long N, int D) {
    DGE_CHECK(N >= 1 && D >= 4 && D % 4 == 0, "rows_mean_std: N >= 1 rows of D (a multiple of 4) columns, got %lld x %d", N, D);
    const long long nch = mean_std_chunks(N);
    DGE_CHECK(nch <= 65535 * 32LL && mean_std_colblocks(D) <= 65535, "rows_mean_std: too many rows or columns");
    const long long nb = 4 * (nch * D + nch * mean_std_colblocks(D));
    DGE_CHECK(nb < (1LL << 31), "rows_mean_std: a workspace of 2 GiB or more");
    return (int)nb;
}

extern "C" int dge_rows_mean_std(const float* x, long long N, int D, float* mean, float* std, void* work, long long work_bytes,
                                 hipStream_t s) {
    const int need = dge_rows_mean_std_work_bytes(N, D);
    if (need < 0) return -1;
    DGE_CHECK(x && mean && std && work, "rows_mean_std: null argument");
    DGE_CHECK(((((uintptr_t)x) | ((uintptr_t)mean) | ((uintptr_t)work)) & 15) == 0, "rows_mean_std: x, mean and work must be 16-byte aligned");
    DGE_CHECK(work_bytes >= need, "rows_mean_std: the workspace holds %lld bytes, %d needed", work_bytes, need);
    const long long nch = mean_std_chunks(N);
    const int ncb = mean_std_colblocks(D);
    float* slots = (float*)work;
    float* dev = slots + nch * D;
    const dim3 grid((unsigned)nch, ncb);
    hipLaunchKernelGGL(rows_colsum_kernel, grid, dim3(256), 0, s, x, N, D, slots);
    hipLaunchKernelGGL(rows_mean_kernel, dim3((D + 255) / 256), dim3(256), 0, s, slots, (int)nch, N, D, mean);
    hipLaunchKernelGGL(rows_sqdev_kernel, grid, dim3(256), 0, s, x, mean, N, D, dev);
    hipLaunchKernelGGL(rows_std_kernel, dim3(1), dim3(256), 0, s, dev, nch * ncb, N, std);
    DGE_LAUNCH_CHECK("rows_mean_std");
    dge_note_kernel("rows_mean_std");
    return 0;
}

extern "C" int dge_area_pool_bwd(const float* g_pooled, float* g, int BC, int H, int W, int k, hipStream_t s) {
    DGE_CHECK(g_pooled && g && BC >= 1 && H >= 1 && W >= 1, "area_pool_bwd: bad arguments (BC %d, H %d, W %d)", BC, H, W);
    DGE_CHECK(k >= 1 && k <= 1024 && H % k == 0 && W % k == 0, "area_pool_bwd: k = %d must divide H = %d and W = %d", k, H, W);
    const long n = (long)BC * H * W;
    DGE_CHECK((n + 255) / 256 < (1L << 31), "area_pool_bwd: too many elements");
    hipLaunchKernelGGL(area_pool_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g_pooled, g, H, W, k, n);
    DGE_LAUNCH_CHECK("area_pool_bwd");
    dge_note_kernel("area_pool_bwd");
    return 0;
}
