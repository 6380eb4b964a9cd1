// Evaluation metrics on 8-bit images (comparing-baseline.py:21-45 per image pair) and the 8-bit quantisation of a saved image.
// Everything the five metrics need from two uint8 images is an integer: the pixel sums fit int64, every 7x7 window sum fits
// int32, so PSNR / MSE / cosine / the skimage SSIM are evaluated in f64 from exact integers and nothing cancels.
#include "common.h"
#include "../../include/dge_hip.h"

namespace {

// ------------------------------------------------------------------ quantise: [B,C,H,W] f32 / bf16 in [-1,1] -> [B,H,W,C] uint8
// torchvision.utils.save_image / infer.save_image_grid: t = x*0.5 + 0.5, clamp to [0,1], t*255 + 0.5, truncate - as SEPARATE
// round-to-nearest f32 operations (a contracted x*127.5 + 128 lands on the other side of a rounding boundary now and then).
__device__ __forceinline__ uint32_t quant_u8(float x) {
    float t = __fadd_rn(__fmul_rn(x, 0.5f), 0.5f);
    t = fminf(fmaxf(t, 0.f), 1.f);
    t = __fadd_rn(__fmul_rn(t, 255.f), 0.5f);
    return (uint32_t)(int)t;                    // 0 .. 255 for every finite x
}

template <typename T>
__global__ __launch_bounds__(256) void quantize_u8_kernel(const T* __restrict__ x, unsigned char* __restrict__ out, int C, long HW, long n) {
    const long o0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;          // this thread's four output bytes (HWC order)
    if (o0 >= n) return;
    long pixb = o0 / C;                                                   // b * HW + pixel
    int c = (int)(o0 - pixb * C);
    long b = pixb / HW, pix = pixb - b * HW;
    uint32_t v[4];
    const int cnt = n - o0 < 4 ? (int)(n - o0) : 4;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = 0;
        if (k < cnt) v[k] = quant_u8(Elem<T>::ld(x + (b * C + c) * HW + pix));
        if (++c == C) { c = 0; if (++pix == HW) { pix = 0; b++; } }
    }
    if (cnt == 4) *(uint32_t*)(out + o0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);   // o0 % 4 == 0: one packed dword
    else for (int k = 0; k < cnt; k++) out[o0 + k] = (unsigned char)v[k];
}

// ------------------------------------------------------------------ metrics
// A row of an [H,W,3] uint8 image is 3W bytes; channel c of pixel x is byte column q = 3x + c, and the 7-pixel horizontal
// window of (x, c) is the byte columns q, q+3, .. q+18.  The kernel therefore works on byte columns and never separates channels.
constexpr int TH = 16, TQ = 96;                    // window origins per tile: 16 rows x 96 byte columns (32 pixels)
constexpr int RH = TH + 6, RQ = TQ + 18;           // bytes loaded per tile: 22 rows x 114 byte columns
constexpr int WORK_WORDS = 6;                      // per slot: int64 sum a, sum b, sum a^2, sum b^2, sum ab; f64 sum of the SSIM map

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {        // fixed butterfly: the same bits every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (tiles_x, tiles_y, B).  work [B][tiles_y * tiles_x][6] 8-byte words, every slot WRITTEN by its workgroup.
__global__ __launch_bounds__(256) void image_metrics_u8_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                                int H, int W, long long* __restrict__ work, double k1, double k2) {
    __shared__ unsigned char sa[RH][RQ + 2], sb[RH][RQ + 2];
    __shared__ uint32_t hs[RH][TQ], hxx[RH][TQ], hyy[RH][TQ], hxy[RH][TQ];   // horizontal 7-sums; hs = sum a | (sum b << 16)
    __shared__ uint32_t redi[4][5];
    __shared__ double redd[4];
    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * TH, q0 = blockIdx.x * TQ, Q = 3 * W;
    const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
    const size_t img = (size_t)blockIdx.z * H * Q;
    const unsigned char* pa = a + img; const unsigned char* pb = b + img;

    // the tile and its 6-pixel halo, once; the pixel sums of the pixels this tile OWNS come from the same load (rows
    // y0 .. y0+TH-1 and byte columns q0 .. q0+TQ-1; the last tile of a direction also owns what lies beyond its window origins)
    uint32_t s[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < RH * RQ; i += 256) {
        const int r = i / RQ, q = i - r * RQ, gy = y0 + r, gq = q0 + q;
        const bool in = gy < H && gq < Q;
        uint32_t va = 0, vb = 0;
        if (in) { const size_t o = (size_t)gy * Q + gq; va = pa[o]; vb = pb[o]; }
        sa[r][q] = (unsigned char)va; sb[r][q] = (unsigned char)vb;
        if (in && (r < TH || last_y) && (q < TQ || last_x)) { s[0] += va; s[1] += vb; s[2] += va * va; s[3] += vb * vb; s[4] += va * vb; }
    }
    __syncthreads();
    for (int i = tid; i < RH * TQ; i += 256) {
        const int r = i / TQ, q = i - r * TQ;
        uint32_t x = 0, y = 0, xx = 0, yy = 0, xy = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const uint32_t va = sa[r][q + 3 * j], vb = sb[r][q + 3 * j];
            x += va; y += vb; xx += va * va; yy += vb * vb; xy += va * vb;
        }
        hs[r][q] = x | (y << 16); hxx[r][q] = xx; hyy[r][q] = yy; hxy[r][q] = xy;
    }
    __syncthreads();
    double ssum = 0.0;
    for (int i = tid; i < TH * TQ; i += 256) {
        const int r = i / TQ, q = i - r * TQ;
        if (y0 + r >= H - 6 || q0 + q >= Q - 18) continue;
        uint32_t p = 0, xx = 0, yy = 0, xy = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) { p += hs[r + j][q]; xx += hxx[r + j][q]; yy += hyy[r + j][q]; xy += hxy[r + j][q]; }
        // ux = Sx/49, vx = (49/48)(Sxx/49 - ux^2) = (49 Sxx - Sx^2)/(48*49): every factor of the map times 49^2 or 48*49, in integers
        const int sx = (int)(p & 0xffffu), sy = (int)(p >> 16), pxy = sx * sy;
        const double A1 = (double)(2 * pxy) + k1, B1 = (double)(sx * sx + sy * sy) + k1;
        const double A2 = (double)(2 * (49 * (int)xy - pxy)) + k2;
        const double B2 = (double)((49 * (int)xx - sx * sx) + (49 * (int)yy - sy * sy)) + k2;
        ssum += (A1 * A2) / (B1 * B2);
    }
    ssum = wave_sum_f64(ssum);
#pragma unroll
    for (int k = 0; k < 5; k++) s[k] = wave_sum_u32(s[k]);        // a workgroup's sums stay below 22*114*255^2 < 2^32
    if ((tid & 63) == 0) {
        redd[tid >> 6] = ssum;
        for (int k = 0; k < 5; k++) redi[tid >> 6][k] = s[k];
    }
    __syncthreads();
    if (tid < WORK_WORDS) {
        long long* slot = work + ((size_t)blockIdx.z * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * WORK_WORDS;
        if (tid < 5) slot[tid] = (long long)redi[0][tid] + (long long)redi[1][tid] + (long long)redi[2][tid] + (long long)redi[3][tid];
        else slot[5] = __double_as_longlong(((redd[0] + redd[1]) + redd[2]) + redd[3]);
    }
}

// grid (B): adds a row's slots in a fixed order (thread-strided, wave butterfly, waves in index order) and evaluates the metrics
__global__ __launch_bounds__(256) void image_metrics_u8_finalize_kernel(const long long* __restrict__ work, int nslots, int H, int W,
                                                                         long long* __restrict__ isums, double* __restrict__ ssim,
                                                                         double* __restrict__ out) {
    __shared__ long long ri[4][5];
    __shared__ double rd[4];
    const int tid = threadIdx.x, row = blockIdx.x;
    const long long* base = work + (size_t)row * nslots * WORK_WORDS;
    long long s[5] = {0, 0, 0, 0, 0};
    double d = 0.0;
    for (int k = tid; k < nslots; k += 256) {
        const long long* slot = base + (size_t)k * WORK_WORDS;
#pragma unroll
        for (int j = 0; j < 5; j++) s[j] += slot[j];
        d += __longlong_as_double(slot[5]);
    }
    d = wave_sum_f64(d);
#pragma unroll
    for (int j = 0; j < 5; j++) s[j] = wave_sum_i64(s[j]);
    if ((tid & 63) == 0) {
        rd[tid >> 6] = d;
        for (int j = 0; j < 5; j++) ri[tid >> 6][j] = s[j];
    }
    __syncthreads();
    if (tid != 0) return;
    long long t[5];
    for (int j = 0; j < 5; j++) { t[j] = ri[0][j] + ri[1][j] + ri[2][j] + ri[3][j]; isums[(size_t)row * 5 + j] = t[j]; }
    const long long N = 3LL * H * W, Sa = t[0], Sb = t[1], Saa = t[2], Sbb = t[3], Sab = t[4];
    const double sm = (((rd[0] + rd[1]) + rd[2]) + rd[3]) / (double)(3LL * (H - 6) * (W - 6));
    const long long sq = Saa - 2 * Sab + Sbb;                               // sum (a - b)^2
    const double mse = (double)sq / (double)N;
    const double psnr = sq == 0 ? __longlong_as_double(0x7ff0000000000000LL) : 10.0 * log10(65025.0 / mse);
    // cosine of x/255*2 - 1, numerator and both squared norms times 255^2: sum (2a - 255)(2b - 255) and so on, in integers
    const long long num = 4 * Sab - 510 * (Sa + Sb) + 65025 * N;
    const long long da = 4 * Saa - 1020 * Sa + 65025 * N, db = 4 * Sbb - 1020 * Sb + 65025 * N;    // > 0: 2a - 255 is odd
    ssim[row] = sm;
    out[(size_t)row * 4 + 0] = psnr;
    out[(size_t)row * 4 + 1] = sm;
    out[(size_t)row * 4 + 2] = mse;
    out[(size_t)row * 4 + 3] = (double)num / sqrt((double)da * (double)db);
}

// H, W <= 65536 keeps 4 * 255^2 * 3HW (the largest integer formed) below 2^52 and the tile grid inside the launch limits
// ------------------------------------------------------------------ min-max normalisation of a whole array
// y = (x - min x) / (max x - min x): the guided-gradient picture of the mis-align scripts (E_mis_align_cropping_s1.py:292-293,
// `grads -= np.max(np.min(grads), 0); grads /= np.max(grads)` - the 0 is an axis, so this is the global minimum, then the new
// maximum).  Launch 1: workgroup k writes the extrema of its grid-strided elements to slot k.  Launch 2: every workgroup reduces
// the <= 1024 slots in the same fixed order (four per thread, then an LDS tree) and applies (x - mn) / (mx - mn) as a subtraction
// and a correctly rounded division, the two numpy operations.
constexpr int MMU_MAX_SLOTS = 1024;

__device__ __forceinline__ void mmu_tree(float* lo, float* hi, int t) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { lo[t] = fminf(lo[t], lo[t + o]); hi[t] = fmaxf(hi[t], hi[t + o]); }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void minmax_slots_kernel(const float* __restrict__ x, float* __restrict__ slots, long n) {
    __shared__ float lo[256], hi[256];
    const int t = threadIdx.x;
    float a = INFINITY, z = -INFINITY;
    for (long i = blockIdx.x * 256L + t; i < n; i += (long)gridDim.x * 256) { const float v = x[i]; a = fminf(a, v); z = fmaxf(z, v); }
    lo[t] = a; hi[t] = z;
    mmu_tree(lo, hi, t);
    if (t == 0) { slots[2 * blockIdx.x] = lo[0]; slots[2 * blockIdx.x + 1] = hi[0]; }
}

__global__ __launch_bounds__(256) void minmax_unit_apply_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 const float* __restrict__ slots, int nslots, long n) {
    __shared__ float lo[256], hi[256];
    const int t = threadIdx.x;
    float a = INFINITY, z = -INFINITY;
    for (int k = t; k < nslots; k += 256) { a = fminf(a, slots[2 * k]); z = fmaxf(z, slots[2 * k + 1]); }
    lo[t] = a; hi[t] = z;
    mmu_tree(lo, hi, t);
    const float mn = lo[0], span = hi[0] - mn;
    for (long i = blockIdx.x * 256L + t; i < n; i += (long)gridDim.x * 256) y[i] = (x[i] - mn) / span;
}

inline bool metrics_shape_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 7 && W >= 7 && H <= 65536 && W <= 65536; }
inline long long metrics_slots(int H, int W) { return (long long)((H - 6 + TH - 1) / TH) * ((3 * (W - 6) + TQ - 1) / TQ); }

}  // namespace

// =================================================================== C ABI
extern "C" int dge_quantize_u8(const void* x, int dtype, unsigned char* out, int B, int C, int H, int W, hipStream_t s) {
    DGE_CHECK(x && out && B >= 1 && C >= 1 && H >= 1 && W >= 1, "quantize_u8: bad arguments (B %d, C %d, H %d, W %d)", B, C, H, W);
    DGE_CHECK(dtype == DGE_F32 || dtype == DGE_BF16, "quantize_u8: dtype %d (f32 or bf16)", dtype);
    DGE_CHECK(((uintptr_t)out & 3) == 0, "quantize_u8: out must be 4-byte aligned");
    const long HW = (long)H * W, n = (long)B * C * HW;
    const long blocks = ((n + 3) / 4 + 255) / 256;
    DGE_CHECK(blocks < (1L << 31), "quantize_u8: too many elements (%ld)", n);
    if (dtype == DGE_BF16) hipLaunchKernelGGL(quantize_u8_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)x, out, C, HW, n);
    else hipLaunchKernelGGL(quantize_u8_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)x, out, C, HW, n);
    dge_note_kernel("quantize_u8<%s>", dtype == DGE_BF16 ? "bf16" : "f32");
    DGE_LAUNCH_CHECK("quantize_u8");
    return 0;
}

extern "C" int dge_image_metrics_u8_work_bytes(int B, int H, int W) {
    DGE_CHECK(metrics_shape_ok(B, H, W), "image_metrics_u8: images must be 7x7 .. 65536x65536 and B 1 .. 65535 (got B %d, %dx%d)", B, H, W);
    const long long bytes = (long long)B * metrics_slots(H, W) * WORK_WORDS * 8;
    DGE_CHECK(bytes < (1LL << 31), "image_metrics_u8: workspace of %lld bytes (B %d, %dx%d): split the batch", bytes, B, H, W);
    return (int)bytes;
}

extern "C" int dge_image_metrics_u8(const unsigned char* a, const unsigned char* b, int B, int H, int W, void* work, long long* isums,
                                    double* ssim, double* out, hipStream_t s) {
    if (dge_image_metrics_u8_work_bytes(B, H, W) < 0) return -1;
    DGE_CHECK(a && b && work && isums && ssim && out, "image_metrics_u8: null argument");
    DGE_CHECK(((uintptr_t)work & 7) == 0, "image_metrics_u8: work must be 8-byte aligned");
    const int tx = (3 * (W - 6) + TQ - 1) / TQ, ty = (H - 6 + TH - 1) / TH;
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
    hipLaunchKernelGGL(image_metrics_u8_kernel, dim3(tx, ty, B), dim3(256), 0, s, a, b, H, W, (long long*)work, c1 * 2401.0, c2 * 2352.0);
    DGE_LAUNCH_CHECK("image_metrics_u8");
    hipLaunchKernelGGL(image_metrics_u8_finalize_kernel, dim3(B), dim3(256), 0, s, (const long long*)work, tx * ty, H, W, isums, ssim, out);
    dge_note_kernel("image_metrics_u8");
    DGE_LAUNCH_CHECK("image_metrics_u8_finalize");
    return 0;
}

extern "C" int dge_minmax_unit_slots(long n) {
    const long g = (n + 1023) / 1024;                   // four elements per thread before a second slot is opened
    return (int)(g < 1 ? 1 : (g > MMU_MAX_SLOTS ? MMU_MAX_SLOTS : g));
}

extern "C" int dge_minmax_unit(const float* x, float* y, long n, float* slots, hipStream_t s) {
    DGE_CHECK(x && y && slots && n >= 1, "minmax_unit: bad arguments (n %ld)", n);
    const int nslots = dge_minmax_unit_slots(n);
    hipLaunchKernelGGL(minmax_slots_kernel, dim3(nslots), dim3(256), 0, s, x, slots, n);
    DGE_LAUNCH_CHECK("minmax_slots");
    long g = (n + 255) / 256;
    g = g > 4096 ? 4096 : g;
    hipLaunchKernelGGL(minmax_unit_apply_kernel, dim3((unsigned)g), dim3(256), 0, s, x, y, (const float*)slots, nslots, n);
    dge_note_kernel("minmax_unit");
    DGE_LAUNCH_CHECK("minmax_unit_apply");
    return 0;
}
