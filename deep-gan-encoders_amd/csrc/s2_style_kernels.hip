// StyleSpace codes of StyleGAN2 (dge_amd.style_codes): the S-space ending of the synthesis backward, which stores the style
// gradients dge_s2_style_grads contracts onto g_wp, and the per-column mean / std of sampled style codes (the sigma unit of a
// StyleSpace edit).  All f32.  Neither uses atomics or a pre-zeroed buffer: every output element has one writer, and partial sums
// go to slots of their own and are added in slot order, so the same operands give the same bits, for a row alone or in a batch.
#include "common.h"
#include "s2_style_steps.h"
#include "../../include/dge_hip.h"

namespace {

// ------------------------------------------------------------------ every style gradient of a synthesis backward, stored
// One workgroup per (block, b), as in s2_style_grads_kernel, whose first two steps (s2_style_steps.h) it shares; the third, the
// contraction with the style DenseBlock, is what an S code does not have.  Three kinds of block:
//   conv block (P):        out[b,c] = st[b,c,0] + s[b,c] * sum_o t[b,o] * wsq[o,c]
//   finished block (st):   out[b,c] = st[b,c,0], its nslot_s copies added (a layer whose tail ran as a pass of its own)
//   toRGB block (gs):      out[b,c] = gs[b,c]
struct S2SGradTable { dge_s2_sgrad_entry e[32]; };
__global__ __launch_bounds__(512) void s2_style_grads_s_kernel(S2SGradTable tab, int B) {
    __shared__ float t[512];
    const dge_s2_sgrad_entry e = tab.e[blockIdx.x];
    const int b = blockIdx.y, tid = threadIdx.x;
    float* __restrict__ out = e.out + (size_t)b * e.in_c;
    if (e.P) {
        s2_conv_block_gs(e, b, B, t, [&](int c, float v) { out[c] = v; });
    } else if (e.st) {
        for (int c = tid; c < e.in_c; c += 512)
            out[c] = sum_slot_pairs(e.st + ((size_t)b * e.in_c + c) * 2, (size_t)B * e.in_c * 2, e.nslot_s).x;
    } else {
        for (int c = tid; c < e.in_c; c += 512) out[c] = e.gs[(size_t)b * e.in_c + c];
    }
}

// ------------------------------------------------------------------ per-column mean and std over the rows
constexpr int kRows = 64;          // rows of a chunk; a workgroup takes 256 of its columns, one per thread (any D: scalar loads,
                                   // consecutive threads on consecutive columns)

// slot[chunk][d] <- sum over the chunk's rows, ascending, of x[r,d] (mean == nullptr) or of (x[r,d] - mean[d])^2
__global__ __launch_bounds__(256) void cols_chunk_sum_kernel(const float* __restrict__ x, const float* __restrict__ mean, long long N, int D,
                                                              float* __restrict__ slots) {
    const int d = blockIdx.y * 256 + threadIdx.x;
    if (d >= D) return;
    const long long r0 = (long long)blockIdx.x * kRows, r1 = r0 + kRows < N ? r0 + kRows : N;
    float s = 0.f;
    if (mean) {
        const float mu = mean[d];
        for (long long r = r0; r < r1; r++) { const float a = x[r * D + d] - mu; s = fmaf(a, a, s); }
    } else {
        for (long long r = r0; r < r1; r++) s += x[r * D + d];
    }
    slots[(size_t)blockIdx.x * D + d] = s;
}
// out[d] <- (sum of the chunk slots of column d, in slot order) / N, or its square root
__global__ __launch_bounds__(256) void cols_finish_kernel(const float* __restrict__ slots, long long nch, long long N, int D, int root,
                                                           float* __restrict__ out) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    float s = 0.f;
    for (long long c = 0; c < nch; c++) s += slots[(size_t)c * D + d];
    s = s / (float)N;
    out[d] = root ? sqrtf(s) : s;
}

}  // namespace

// =================================================================== C ABI
extern "C" int dge_s2_style_grads_s(const dge_s2_sgrad_entry* entries, int n, int B, hipStream_t s) {
    DGE_CHECK(entries && n >= 1 && n <= 32 && B >= 1 && B <= 65535, "s2_style_grads_s: 1..32 blocks, 1..65535 rows");
    S2SGradTable tab;
    for (int i = 0; i < n; i++) {
        const dge_s2_sgrad_entry& e = entries[i];
        DGE_CHECK(e.in_c >= 1 && e.in_c <= 512 && e.out, "s2_style_grads_s: bad block %d (1..512 channels, an `out` slice)", i);
        if (e.P)
            DGE_CHECK(e.st && e.d && e.s && e.bias && e.wsq && e.out_c >= 1 && e.out_c <= 512 && e.nslot_p >= 1 && e.nslot_s >= 1,
                      "s2_style_grads_s: conv block %d needs P, st, d, s, bias, wsq, 1..512 output channels and slot counts >= 1", i);
        else
            DGE_CHECK(e.st ? e.nslot_s >= 1 : e.gs != nullptr,
                      "s2_style_grads_s: block %d is neither a conv block (P), a finished block (st) nor a toRGB block (gs)", i);
        tab.e[i] = e;
    }
    hipLaunchKernelGGL(s2_style_grads_s_kernel, dim3(n, B), dim3(512), 0, s, tab, B);
    DGE_LAUNCH_CHECK("s2_style_grads_s");
    dge_note_kernel("s2_style_grads_s");
    return 0;
}

extern "C" int dge_cols_mean_std_work_bytes(long long N, int D) {
    DGE_CHECK(N >= 1 && D >= 1, "cols_mean_std: N >= 1 rows of D >= 1 columns, got %lld x %d", N, D);
    const long long nch = (N + kRows - 1) / kRows;
    DGE_CHECK(nch <= 0x7fffffffLL && (D + 255) / 256 <= 65535, "cols_mean_std: too many rows or columns");
    const long long nb = 4 * nch * D;
    DGE_CHECK(nb < (1LL << 31), "cols_mean_std: a workspace of 2 GiB or more");
    return (int)nb;
}

extern "C" int dge_cols_mean_std(const float* x, long long N, int D, float* mean, float* std, void* work, long long work_bytes,
                                 hipStream_t s) {
    const int need = dge_cols_mean_std_work_bytes(N, D);
    if (need < 0) return -1;
    DGE_CHECK(x && mean && std && work, "cols_mean_std: null argument");
    DGE_CHECK(work_bytes >= need, "cols_mean_std: the workspace holds %lld bytes, %d needed", work_bytes, need);
    const long long nch = (N + kRows - 1) / kRows;
    float* slots = (float*)work;
    const dim3 grid((unsigned)nch, (D + 255) / 256), fin((D + 255) / 256);
    hipLaunchKernelGGL(cols_chunk_sum_kernel, grid, dim3(256), 0, s, x, (const float*)nullptr, N, D, slots);
    hipLaunchKernelGGL(cols_finish_kernel, fin, dim3(256), 0, s, slots, nch, N, D, 0, mean);
    hipLaunchKernelGGL(cols_chunk_sum_kernel, grid, dim3(256), 0, s, x, (const float*)mean, N, D, slots);
    hipLaunchKernelGGL(cols_finish_kernel, fin, dim3(256), 0, s, slots, nch, N, D, 1, std);
    DGE_LAUNCH_CHECK("cols_mean_std");
    dge_note_kernel("cols_mean_std");
    return 0;
}
