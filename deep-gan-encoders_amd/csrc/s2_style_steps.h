// The first two steps of a modulated block's style gradient, shared by dge_s2_style_grads (which contracts g_s onto g_wp) and
// dge_s2_style_grads_s (which stores it):
//   t[b,o]   = -(P0 - bias[o]*bscale*P1) * d[b,o]^2                      (demodulation gradient from the fused tail sums)
//   g_s[b,c] = st[b,c,0] + s[b,c] * sum_o t[b,o] * wsq[o,c]              (direct part from the data-gradient statistics)
// Entry: dge_s2_grad_entry or dge_s2_sgrad_entry (the same operand names).  t: 512 floats of LDS.  put(c, g_s[b,c]) takes the
// result; the caller synchronises behind it where it reads the results across threads.
#pragma once
#include "common.h"

template <class Entry, class Put>
__device__ __forceinline__ void s2_conv_block_gs(const Entry& e, int b, int B, float* t, Put put) {
    const int tid = threadIdx.x;
    for (int o = tid; o < e.out_c; o += 512) {
        const int idx = b * e.out_c + o;
        const float2 pp = sum_slot_pairs(e.P + (size_t)idx * 2, (size_t)B * e.out_c * 2, e.nslot_p);
        const float dv = e.d[idx];
        t[o] = -(pp.x - e.bias[o] * e.bscale * pp.y) * dv * dv;
    }
    __syncthreads();
    for (int c = tid; c < e.in_c; c += 512) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int o = 0;
        for (; o + 3 < e.out_c; o += 4) {
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] = fmaf(t[o + j], e.wsq[(size_t)(o + j) * e.in_c + c], acc[j]);
        }
        for (; o < e.out_c; o++) acc[0] = fmaf(t[o], e.wsq[(size_t)o * e.in_c + c], acc[0]);
        const int idx = b * e.in_c + c;
        const float2 ss = sum_slot_pairs(e.st + (size_t)idx * 2, (size_t)B * e.in_c * 2, e.nslot_s);
        put(c, ss.x + e.s[idx] * ((acc[0] + acc[1]) + (acc[2] + acc[3])));
    }
}
