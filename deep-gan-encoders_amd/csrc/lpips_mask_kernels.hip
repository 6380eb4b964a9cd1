// Masked LPIPS (dge_amd.lpips.LPIPS.value_and_grad(mask=...), the projector's --mask_dir): the mask pyramid, the masked input
// preparation and its adjoint, the mask-weighted perceptual head with its finaliser, and the mask blend of the written images.
//   m_0 = m, m_k = avg_pool2d(m_{k-1}, 2) (floor: an odd trailing row or column is dropped, as nn.MaxPool2d(2,2) drops it)
//   dist_b = sum_k ( sum_p m_k[b,p] d_k[b,p] ) / ( sum_p m_k[b,p] ),  a level of sum 0 contributes 0 and no gradient
// No atomics and nothing pre-zeroed: every partial sum goes to its own slot of a caller-provided workspace and the slots are added
// in a fixed order, so the bits are the same run to run and in both reduction modes, and a row has the bits of its batch-1 call
// (no grid or slot layout depends on B).
#include "common.h"
#include "lpips_prep.h"
#include "../../include/dge_hip.h"

namespace {

constexpr int kLevels = 5;           // LPIPS-VGG taps
constexpr int kTile = 32;            // level-0 pixels of a pyramid tile side: 16, 8, 4, 2 pixels of levels 1..4

__host__ __device__ inline long long pyr_level_off(int B, int H, int W, int k) {          // floats in front of level k
    long long o = 0;
    for (int j = 0; j < k; j++) o += (long long)B * (H >> j) * (W >> j);
    return o;
}

// One workgroup per 32 x 32 tile of m_0: the tile goes through LDS, every level is pooled from the level below it
// ((a + b) + (c + d)) * 0.25, the in-range values are written, and the tile's sum of every level goes to slot [b][tile][level].
// A level-k value is in range when y < H >> k and x < W >> k; its 2^k x 2^k block of m_0 then lies inside the image.
__global__ __launch_bounds__(256) void mask_pyramid_kernel(const float* __restrict__ m, float* __restrict__ levels, float* __restrict__ slots,
                                                            int B, int H, int W) {
    __shared__ float s0[kTile][kTile + 1], s1[16][17], s2[8][9], s3[4][5], s4[2][2];
    const int t = threadIdx.x, b = blockIdx.z;
    const int y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;
    const float* mb = m + (size_t)b * H * W;
    float* l0 = levels + (size_t)b * H * W;
    for (int i = t; i < kTile * kTile; i += 256) {
        const int ty = i / kTile, tx = i % kTile, y = y0 + ty, x = x0 + tx;
        float v = 0.f;
        if (y < H && x < W) { v = mb[(size_t)y * W + x]; l0[(size_t)y * W + x] = v; }
        s0[ty][tx] = v;
    }
    __syncthreads();
#define PYR_LEVEL(K, SRC, DST, SIDE)                                                                                              \
    {                                                                                                                             \
        const int hk = H >> K, wk = W >> K;                                                                                       \
        if (t < SIDE * SIDE) {                                                                                                    \
            const int ty = t / SIDE, tx = t % SIDE, y = (y0 >> K) + ty, x = (x0 >> K) + tx;                                       \
            float v = ((SRC[2 * ty][2 * tx] + SRC[2 * ty][2 * tx + 1]) + (SRC[2 * ty + 1][2 * tx] + SRC[2 * ty + 1][2 * tx + 1])) * 0.25f; \
            if (y < hk && x < wk) levels[pyr_level_off(B, H, W, K) + ((size_t)b * hk + y) * wk + x] = v; else v = 0.f;            \
            DST[ty][tx] = v;                                                                                                      \
        }                                                                                                                         \
        __syncthreads();                                                                                                          \
    }
    PYR_LEVEL(1, s0, s1, 16)
    PYR_LEVEL(2, s1, s2, 8)
    PYR_LEVEL(3, s2, s3, 4)
    PYR_LEVEL(4, s3, s4, 2)
#undef PYR_LEVEL
    // the tile's five sums, each in a fixed order: lane-strided partial sums, then the xor butterfly of one wave
    const int lane = t & 63, wave = t >> 6;
    float* slot = slots + ((size_t)b * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * kLevels;
    if (wave == 0) {
        float a = 0.f;
        for (int i = lane; i < kTile * kTile; i += 64) a += s0[i / kTile][i % kTile];
        a = wave_sum(a);
        if (lane == 0) slot[0] = a;
    } else if (wave == 1) {
        float a = 0.f;
        for (int i = lane; i < 256; i += 64) a += s1[i / 16][i % 16];
        a = wave_sum(a);
        if (lane == 0) slot[1] = a;
    } else if (wave == 2) {
        float a = wave_sum(s2[lane / 8][lane % 8]);
        float c = wave_sum(lane < 4 ? s4[lane / 2][lane % 2] : 0.f);
        if (lane == 0) { slot[2] = a; slot[4] = c; }
    } else {
        float a = wave_sum(lane < 16 ? s3[lane / 4][lane % 4] : 0.f);
        if (lane == 0) slot[3] = a;
    }
}

// one wave per (row, level): the tile slots in lane-strided order, then the butterfly; inv_sum = 1 / sum, or 0 where the sum is 0
__global__ __launch_bounds__(64) void mask_pyramid_finalize_kernel(const float* __restrict__ slots, int ntiles, float* __restrict__ inv_sum,
                                                                    float* __restrict__ sums) {
    const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const float* sb = slots + (size_t)b * ntiles * kLevels + k;
    float a = 0.f;
    for (int i = lane; i < ntiles; i += 64) a += sb[(size_t)i * kLevels];
    a = wave_sum(a);
    if (lane == 0) {
        inv_sum[b * kLevels + k] = a > 0.f ? 1.f / a : 0.f;
        if (sums) sums[b * kLevels + k] = a;
    }
}

// lanes per pixel and pixels per workgroup of the head: lpips_head_kernel's layout (lpips_kernels.hip)
template <typename T> inline void head_w_layout(int C, int& lpp, int& nj, int& ppb) {
    constexpr int EP = Elem<T>::PER16;
    const int chunks = C / EP;
    lpp = chunks >= 64 ? 64 : chunks;
    nj = chunks / lpp;
    ppb = 4 * (64 / lpp) * 8;                             // 8 iterations per wave
}

// The weighted head of one tap.  f: [2B,h,w,C] T (samples [0,B) = image a, [B,2B) = image b), lin [C] f32, mk [B,HW] the mask level,
// inv [B,5] the pyramid's inv_sum (column `tap` is read).  slots[b][blockIdx.x] = sum over the workgroup's pixels of m_k[p] d[p];
// g1 (optional, [B,h,w,C] T) = gscale * m_k[p] * inv[b,tap] * d d[p] / d f[B+b].  Lane layout of lpips_head_kernel: LPP lanes
// on one pixel with 16-byte loads, xor butterflies inside the LPP lanes.
template <typename T, int NJ>
__global__ __launch_bounds__(256) void lpips_head_w_kernel(const T* __restrict__ f, const float* __restrict__ lin, const float* __restrict__ mk,
                                                            const float* __restrict__ inv, int tap, float* __restrict__ slots,
                                                            T* __restrict__ g1, int B, int HW, int C, float gscale, int lpp, int pix_per_block) {
    constexpr int EP = Elem<T>::PER16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int ppw = 64 / lpp, sub = lane / lpp, li = lane % lpp;
    const int p_begin = blockIdx.x * pix_per_block, p_end = min(HW, p_begin + pix_per_block);
    float linv[NJ][EP];
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
        for (int e = 0; e < EP; e++) linv[j][e] = lin[(j * lpp + li) * EP + e];
    const float gs_inv = gscale * inv[b * kLevels + tap];
    const float* mb = mk + (size_t)b * HW;
    float dacc = 0.f;
    for (int p0 = p_begin + wave * ppw; p0 < p_end; p0 += 4 * ppw) {
        const int p = p0 + sub;
        const bool ok = p < p_end;
        const int pc = ok ? p : p_begin;
        const size_t o0 = ((size_t)b * HW + pc) * C, o1 = ((size_t)(B + b) * HW + pc) * C;
        const float mp = mb[pc];
        float a[NJ][EP], bv[NJ][EP];
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            unpack16(*(const uint4*)(f + o0 + (j * lpp + li) * EP), a[j], (T*)nullptr);
            unpack16(*(const uint4*)(f + o1 + (j * lpp + li) * EP), bv[j], (T*)nullptr);
#pragma unroll
            for (int e = 0; e < EP; e++) { s0 += a[j][e] * a[j][e]; s1 += bv[j][e] * bv[j][e]; }
        }
        for (int m = lpp >> 1; m > 0; m >>= 1) { s0 += __shfl_xor(s0, m, 64); s1 += __shfl_xor(s1, m, 64); }
        const float n1 = sqrtf(s1), r0 = 1.f / (sqrtf(s0) + 1e-10f), r1 = 1.f / (n1 + 1e-10f);
        float d = 0.f, dot = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; j++)
#pragma unroll
            for (int e = 0; e < EP; e++) {
                const float u = a[j][e] * r0 - bv[j][e] * r1;
                d += linv[j][e] * u * u;
                dot += (-2.f * linv[j][e] * u) * bv[j][e];
            }
        for (int m = lpp >> 1; m > 0; m >>= 1) { d += __shfl_xor(d, m, 64); dot += __shfl_xor(dot, m, 64); }
        if (ok && li == 0 && mp != 0.f) dacc += mp * d;
        if (g1 && ok) {
            const float wgt = gs_inv * mp;                // 0 under the mask and on an empty level: the gradient is exactly 0 there
            const float k = n1 > 0.f ? dot * r1 * r1 / n1 : 0.f;
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                float g[EP];
#pragma unroll
                for (int e = 0; e < EP; e++) {
                    const float u = a[j][e] * r0 - bv[j][e] * r1;
                    g[e] = wgt != 0.f ? wgt * ((-2.f * linv[j][e] * u) * r1 - bv[j][e] * k) : 0.f;
                }
                *(uint4*)(g1 + ((size_t)b * HW + p) * C + (j * lpp + li) * EP) = pack16(g, (T*)nullptr);
            }
        }
    }
    dacc = wave_sum(dacc);
    __shared__ float wred[4];
    if (lane == 0) wred[wave] = dacc;
    __syncthreads();
    if (threadIdx.x == 0) slots[(size_t)b * gridDim.x + blockIdx.x] = (wred[0] + wred[1]) + (wred[2] + wred[3]);
}

struct HeadWTaps { long long off[kLevels]; int nslots[kLevels]; };

// one wave per row: per tap the slots in lane-strided order and the butterfly, times inv_sum; the taps in tap order
__global__ __launch_bounds__(64) void lpips_head_w_finalize_kernel(const float* __restrict__ slots, HeadWTaps taps, const float* __restrict__ inv,
                                                                    float* __restrict__ dist) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float total = 0.f;
    for (int k = 0; k < kLevels; k++) {
        const int n = taps.nslots[k];
        const float* sb = slots + taps.off[k] + (size_t)b * n;
        float a = 0.f;
        for (int i = lane; i < n; i += 64) a += sb[i];
        a = wave_sum(a);
        const float iv = inv[b * kLevels + k];
        total += iv != 0.f ? a * iv : 0.f;
    }
    if (lane == 0) dist[b] = total;
}

// out[b,c,p] = m[b,p] * a[b,c,p] + (1 - m[b,p]) * b[b,c,p], the two products and the sum rounded one by one (torch's expression)
__global__ __launch_bounds__(256) void mask_blend_kernel(const float* __restrict__ m, const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ out, int HW, long n) {
#pragma clang fp contract(off)
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const long row = i / (3L * HW);
    const float mv = m[row * HW + i % HW];
    const float t0 = mv * a[i];
    const float om = 1.f - mv;
    const float t1 = om * b[i];
    out[i] = t0 + t1;
}

template <typename T>
int head_w_launch(const void* feat, const float* lin, const float* mk, const float* inv, int tap, float* slots, void* g1, int B, int HW, int C,
                  float gscale, hipStream_t s) {
    int lpp, nj, ppb;
    head_w_layout<T>(C, lpp, nj, ppb);
    dim3 grid((HW + ppb - 1) / ppb, B);
#define LH(NJ) hipLaunchKernelGGL((lpips_head_w_kernel<T, NJ>), grid, dim3(256), 0, s, (const T*)feat, lin, mk, inv, tap, slots, (T*)g1, B, HW, C, gscale, lpp, ppb)
    if (nj == 1) LH(1); else if (nj == 2) LH(2); else if (nj == 4) LH(4); else { dge_set_error("lpips_head_w: unsupported C=%d", C); return -1; }
#undef LH
    return 0;
}

bool head_w_shape_ok(int C, int dtype) {
    const int ep = dtype == DGE_BF16 ? 8 : 4;
    return C >= ep && C % ep == 0 && ((C / ep) & (C / ep - 1)) == 0 && C / ep <= 256;
}

}  // namespace

// =================================================================== C ABI
extern "C" int dge_mask_pyramid_work_bytes(int B, int H, int W) {
    DGE_CHECK(B >= 1 && H >= 1 && W >= 1 && B <= 65535, "mask_pyramid: bad sizes (B %d, H %d, W %d)", B, H, W);
    const long long tiles = (long long)((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile);
    DGE_CHECK((H + kTile - 1) / kTile <= 65535 && tiles * B * kLevels * 4 < (1LL << 31), "mask_pyramid: the image is too large");
    return (int)(tiles * B * kLevels * 4);
}

extern "C" int dge_mask_pyramid(const float* m, float* levels, float* inv_sum, float* sums, int B, int H, int W, void* work,
                                long long work_bytes, hipStream_t s) {
    const int need = dge_mask_pyramid_work_bytes(B, H, W);
    if (need < 0) return -1;
    DGE_CHECK(m && levels && inv_sum && work, "mask_pyramid: null argument");
    DGE_CHECK(m != levels, "mask_pyramid: level 0 is a copy of m in the levels' own storage, not m itself");
    DGE_CHECK(work_bytes >= need, "mask_pyramid: the workspace holds %lld bytes, %d needed", work_bytes, need);
    const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile, B);
    hipLaunchKernelGGL(mask_pyramid_kernel, grid, dim3(256), 0, s, m, levels, (float*)work, B, H, W);
    hipLaunchKernelGGL(mask_pyramid_finalize_kernel, dim3(B, kLevels), dim3(64), 0, s, (const float*)work, (int)(grid.x * grid.y), inv_sum, sums);
    DGE_LAUNCH_CHECK("mask_pyramid");
    dge_note_kernel("mask_pyramid");
    return 0;
}

extern "C" int dge_lpips_prep_masked(const float* img, const float* mask, void* x, int B, int HW, int cpad, const float* host_shift3,
                                     const float* host_scale3, int dtype, hipStream_t s) {
    DGE_CHECK(img && mask && x && cpad >= 3, "lpips_prep_masked: null argument or cpad < 3");
    const long n = (long)B * HW;
    const float i0 = 1.f / host_scale3[0], i1 = 1.f / host_scale3[1], i2 = 1.f / host_scale3[2];
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == DGE_BF16) hipLaunchKernelGGL((lpips_prep_kernel<bf16_t, true>), grid, dim3(256), 0, s, img, mask, (bf16_t*)x, B, HW, cpad, host_shift3[0], host_shift3[1], host_shift3[2], i0, i1, i2);
    else hipLaunchKernelGGL((lpips_prep_kernel<float, true>), grid, dim3(256), 0, s, img, mask, (float*)x, B, HW, cpad, host_shift3[0], host_shift3[1], host_shift3[2], i0, i1, i2);
    DGE_LAUNCH_CHECK("lpips_prep_masked");
    dge_note_kernel("lpips_prep_masked");
    return 0;
}

extern "C" int dge_lpips_prep_bwd_masked(const void* gx, const float* mask, float* gimg, int B, int HW, int cpad, const float* host_scale3,
                                         float factor, int accumulate, int dtype, hipStream_t s) {
    DGE_CHECK(gx && mask && gimg && cpad >= 3, "lpips_prep_bwd_masked: null argument or cpad < 3");
    const long n = (long)B * HW;
    const float i0 = 1.f / host_scale3[0], i1 = 1.f / host_scale3[1], i2 = 1.f / host_scale3[2];
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == DGE_BF16) hipLaunchKernelGGL((lpips_prep_bwd_kernel<bf16_t, true>), grid, dim3(256), 0, s, (const bf16_t*)gx, mask, gimg, B, HW, cpad, i0, i1, i2, factor, accumulate);
    else hipLaunchKernelGGL((lpips_prep_bwd_kernel<float, true>), grid, dim3(256), 0, s, (const float*)gx, mask, gimg, B, HW, cpad, i0, i1, i2, factor, accumulate);
    DGE_LAUNCH_CHECK("lpips_prep_bwd_masked");
    dge_note_kernel("lpips_prep_bwd_masked");
    return 0;
}

extern "C" int dge_lpips_head_w_slots(int HW, int C, int dtype) {
    DGE_CHECK(HW >= 1 && head_w_shape_ok(C, dtype), "lpips_head_w: HW=%d, C=%d must be a power-of-two multiple of %d (at most 256 chunks)", HW, C,
              dtype == DGE_BF16 ? 8 : 4);
    int lpp, nj, ppb;
    if (dtype == DGE_BF16) head_w_layout<bf16_t>(C, lpp, nj, ppb); else head_w_layout<float>(C, lpp, nj, ppb);
    return (HW + ppb - 1) / ppb;
}

extern "C" int dge_lpips_head_w(const void* feat, const float* lin, const float* mk, const float* inv_sum, int tap, float* slots, void* g1,
                                int B, int HW, int C, float gscale, int dtype, hipStream_t s) {
    DGE_CHECK(feat && lin && mk && inv_sum && slots, "lpips_head_w: null argument");
    DGE_CHECK(tap >= 0 && tap < kLevels && B >= 1 && B <= 65535, "lpips_head_w: tap %d of 5, B %d", tap, B);
    if (dge_lpips_head_w_slots(HW, C, dtype) < 0) return -1;
    const int rc = dtype == DGE_BF16 ? head_w_launch<bf16_t>(feat, lin, mk, inv_sum, tap, slots, g1, B, HW, C, gscale, s)
                                      : head_w_launch<float>(feat, lin, mk, inv_sum, tap, slots, g1, B, HW, C, gscale, s);
    if (rc) return rc;
    DGE_LAUNCH_CHECK("lpips_head_w");
    dge_note_kernel("lpips_head_w");
    return 0;
}

extern "C" int dge_lpips_head_w_finalize(const float* slots, const long long* host_off5, const int* host_nslots5, const float* inv_sum,
                                         float* dist, int B, hipStream_t s) {
    DGE_CHECK(slots && host_off5 && host_nslots5 && inv_sum && dist && B >= 1, "lpips_head_w_finalize: null argument or B < 1");
    HeadWTaps t;
    for (int k = 0; k < kLevels; k++) {
        DGE_CHECK(host_off5[k] >= 0 && host_nslots5[k] >= 1, "lpips_head_w_finalize: tap %d: offset %lld, %d slots", k, host_off5[k], host_nslots5[k]);
        t.off[k] = host_off5[k]; t.nslots[k] = host_nslots5[k];
    }
    hipLaunchKernelGGL(lpips_head_w_finalize_kernel, dim3(B), dim3(64), 0, s, slots, t, inv_sum, dist);
    DGE_LAUNCH_CHECK("lpips_head_w_finalize");
    dge_note_kernel("lpips_head_w_finalize");
    return 0;
}

extern "C" int dge_mask_blend(const float* m, const float* a, const float* b, float* out, int B, int HW, hipStream_t s) {
    DGE_CHECK(m && a && b && out && B >= 1 && HW >= 1, "mask_blend: bad arguments (B %d, HW %d)", B, HW);
    const long n = 3L * B * HW;
    DGE_CHECK((n + 255) / 256 < (1L << 31), "mask_blend: too many elements");
    hipLaunchKernelGGL(mask_blend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m, a, b, out, HW, n);
    DGE_LAUNCH_CHECK("mask_blend");
    dge_note_kernel("mask_blend");
    return 0;
}
