// LPIPS input preparation (ScalingLayer + NCHW -> NHWC) and its adjoint, one body for the plain entry points
// (lpips_kernels.hip, MASKED = false) and the masked ones (lpips_mask_kernels.hip, MASKED = true: a per-pixel factor m [B,HW]).
// MASKED = false compiles to the code the plain kernels always had: the mask pointer is never read.
#pragma once
#include "common.h"

// a * b as one rounded f32 product that a following add cannot absorb into an fma (torch rounds `m * a` before it subtracts)
__device__ __forceinline__ float lpips_mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    const float p = a * b;
    return p;
}

// img [B,3,h,w] f32 -> x [B,h,w,CP] T (CP >= 3, extra channels zero): (img - shift[c]) / scale[c]; MASKED: (m * img - shift[c]) / scale[c]
template <typename T, bool MASKED>
__global__ void lpips_prep_kernel(const float* __restrict__ img, const float* __restrict__ mask, T* __restrict__ x, int B, int HW, int CP,
                                  float s0, float s1, float s2, float i0, float i1, float i2) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)B * HW) return;
    const int b = idx / HW, p = idx % HW;
    const float* ib = img + (size_t)b * 3 * HW;
    T* xp = x + (size_t)idx * CP;
    float v0 = ib[p], v1 = ib[HW + p], v2 = ib[2 * HW + p];
    if (MASKED) {
        const float m = mask[idx];
        v0 = lpips_mul_rounded(m, v0); v1 = lpips_mul_rounded(m, v1); v2 = lpips_mul_rounded(m, v2);
    }
    Elem<T>::st(xp + 0, (v0 - s0) * i0);
    Elem<T>::st(xp + 1, (v1 - s1) * i1);
    Elem<T>::st(xp + 2, (v2 - s2) * i2);
    for (int c = 3; c < CP; c++) Elem<T>::st(xp + c, 0.f);
}
// adjoint: gimg[b,c,p] (+)= factor * gx[b,p,c] * inv_scale[c]; MASKED: that value times m[b,p], rounded before the add
template <typename T, bool MASKED>
__global__ void lpips_prep_bwd_kernel(const T* __restrict__ gx, const float* __restrict__ mask, float* __restrict__ gimg, int B, int HW, int CP,
                                      float i0, float i1, float i2, float factor, int accumulate) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)B * HW) return;
    const int b = idx / HW, p = idx % HW;
    const T* xp = gx + (size_t)idx * CP;
    float* gb = gimg + (size_t)b * 3 * HW;
    float v0 = Elem<T>::ld(xp) * i0 * factor, v1 = Elem<T>::ld(xp + 1) * i1 * factor, v2 = Elem<T>::ld(xp + 2) * i2 * factor;
    if (MASKED) {
        const float m = mask[idx];
        v0 = lpips_mul_rounded(v0, m); v1 = lpips_mul_rounded(v1, m); v2 = lpips_mul_rounded(v2, m);
    }
    if (accumulate) { gb[p] += v0; gb[HW + p] += v1; gb[2 * HW + p] += v2; }
    else { gb[p] = v0; gb[HW + p] = v1; gb[2 * HW + p] = v2; }
}
