// Data gradient of the StyleGAN1 mapping network (reference model/stylegan1/net.py:441-466, pixel_norm :28-29) in ONE launch:
//   w+ = lerp(buffer1, broadcast_L(chain(pixel_norm(z))), coefs)      (or the plain broadcast when there is no truncation centre)
//   dz = pixel_norm'(z)^T . chain'^T . sum_l coefs[l] * dW+[b, l, :]
// One 1024-thread workgroup per sample, the layout of dense_chain_kernel (s2_kernels.hip).  The layer outputs the forward saved
// (`acts`, the per-layer dge_linear results) are read into LDS, so every leaky-relu mask is the one the forward applied; without
// them the forward is recomputed into LDS with dense_chain_kernel's arithmetic (lane-strided partial sums, wave_sum, scale /
// bias / act / gain, bit-identical to the per-layer launches).  The backward then walks the chain: the transposed product of layer l is split over
// eight groups of the output index (128 threads each, four consecutive input elements per thread, 16-byte reads of W rows), and
// the eight partial sums are added in a fixed order.  No atomics: the same bits every run, deterministic mode or not.
// dge_mapping_bwd_wide (second half of the file) is the same adjoint on saved activations as one chip-wide launch per layer.
#include "common.h"
#include "../../include/dge_hip.h"

namespace {

constexpr int kMapThreads = 1024;
constexpr int kMapWaves = kMapThreads / 64;
constexpr int kMapMaxWidth = 512;
constexpr int kMapMaxLayers = 8;
constexpr int kMapGroups = kMapThreads / (kMapMaxWidth / 4);   // output-index groups of the transposed product (8)

struct MapChain {
    const float* w[kMapMaxLayers];
    const float* bias[kMapMaxLayers];
    int I[kMapMaxLayers], O[kMapMaxLayers], act[kMapMaxLayers];
    float wscale[kMapMaxLayers], bscale[kMapMaxLayers], add[kMapMaxLayers], gain[kMapMaxLayers];
    const float* act_out[kMapMaxLayers];       // saved layer outputs [B, O_l], or all null (recompute)
    int n;
};

__global__ __launch_bounds__(kMapThreads) void mapping_bwd_kernel(const float* __restrict__ z, int ldz, MapChain c,
                                                                  const float* __restrict__ g, int L, const float* __restrict__ coefs,
                                                                  float* __restrict__ dz, int lddz, int pixelnorm, float eps) {
    __shared__ float h[kMapMaxLayers + 1][kMapMaxWidth];    // h[0]: chain input, h[l + 1]: output of layer l (18 KB)
    __shared__ float gr[2][kMapMaxWidth];                    // running gradient, ping-pong
    __shared__ float part[kMapGroups][kMapMaxWidth];         // the partial sums of a transposed product (16 KB)
    __shared__ float rnorm;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int I0 = c.I[0], D = c.O[c.n - 1];
    const float* __restrict__ zb = z + (size_t)b * ldz;

    // ---- forward, dense_chain_kernel's arithmetic
    if (pixelnorm) {
        if (wave == 0) {
            float s = 0.f;
            for (int i = lane; i < I0; i += 64) { const float v = zb[i]; s += v * v; }
            s = wave_sum(s);
            const float r = rsqrtf(s / I0 + eps);
            for (int i = lane; i < I0; i += 64) h[0][i] = zb[i] * r;
            if (lane == 0) rnorm = r;
        }
    } else {
        for (int i = tid; i < I0; i += kMapThreads) h[0][i] = zb[i];
    }
    if (c.act_out[0]) {
        for (int l = 0; l < c.n; l++)
            for (int o = tid; o < c.O[l]; o += kMapThreads) h[l + 1][o] = c.act_out[l][(size_t)b * c.O[l] + o];
    }
    __syncthreads();
    for (int l = 0; l < c.n && !c.act_out[0]; l++) {
        const int I = c.I[l], O = c.O[l];
        const float* __restrict__ W = c.w[l];
        const float* __restrict__ bias = c.bias[l];
        for (int o = wave; o < O; o += kMapWaves) {
            const float* wr = W + (size_t)o * I;
            float s = 0.f;
#pragma unroll 8
            for (int i = lane; i < I; i += 64) s += h[l][i] * wr[i];
            s = wave_sum(s);
            if (lane == 0) {
                float v = s * c.wscale[l] + (bias ? bias[o] * c.bscale[l] : 0.f) + c.add[l];
                if (c.act[l] == DGE_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
                else if (c.act[l] == DGE_ACT_RELU) v = v > 0.f ? v : 0.f;
                v *= c.gain[l];
                h[l + 1][o] = v;
            }
        }
        __syncthreads();
    }

    // ---- W+ -> w: the lerp's (or the broadcast's) adjoint, a fixed-order sum over the L rows
    const float* __restrict__ gb = g + (size_t)b * L * D;
    for (int d = tid; d < D; d += kMapThreads) {
        float s = 0.f;
        for (int l = 0; l < L; l++) s += (coefs ? coefs[l] : 1.f) * gb[(size_t)l * D + d];
        gr[0][d] = s;
    }
    __syncthreads();

    // ---- the chain, last layer first
    int cur = 0;
    const int i4 = (tid % (kMapMaxWidth / 4)) * 4, grp = tid / (kMapMaxWidth / 4);
    for (int l = c.n - 1; l >= 0; l--) {
        const int I = c.I[l], O = c.O[l];
        const float* __restrict__ W = c.w[l];
        // gradient of the pre-activation sum s (v = act(s*wscale + ...)*gain; h > 0 exactly where the pre-activation is, gain > 0)
        for (int o = tid; o < O; o += kMapThreads) {
            const float hv = h[l + 1][o];
            const float slope = c.act[l] == DGE_ACT_LRELU ? (hv > 0.f ? 1.f : 0.2f) : (c.act[l] == DGE_ACT_RELU ? (hv > 0.f ? 1.f : 0.f) : 1.f);
            gr[cur][o] *= c.gain[l] * slope * c.wscale[l];
        }
        __syncthreads();
        const int og = (O + kMapGroups - 1) / kMapGroups, o0 = grp * og, o1 = min(O, o0 + og);
        if (i4 < I) {                                   // I % 4 == 0, W 16-byte aligned (checked at the C ABI)
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
            for (int o = o0; o < o1; o++) {
                const float go = gr[cur][o];
                const float4 w = *reinterpret_cast<const float4*>(W + (size_t)o * I + i4);
                s.x += go * w.x; s.y += go * w.y; s.z += go * w.z; s.w += go * w.w;
            }
            part[grp][i4] = s.x; part[grp][i4 + 1] = s.y; part[grp][i4 + 2] = s.z; part[grp][i4 + 3] = s.w;
        }
        __syncthreads();
        if (tid < I) {
            float v = part[0][tid];
#pragma unroll
            for (int k = 1; k < kMapGroups; k++) v += part[k][tid];
            gr[cur ^ 1][tid] = v;
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- pixel norm: y = x*r, r = rsqrt(mean(x^2) + eps)  ->  dx = r*dy - x * r^3/I0 * sum(dy*x)
    float* __restrict__ dzb = dz + (size_t)b * lddz;
    if (pixelnorm) {
        if (wave == 0) {
            float s = 0.f;
            for (int k = lane; k < I0; k += 64) s += gr[cur][k] * zb[k];
            s = wave_sum(s);
            const float r = rnorm;
            const float k3 = r * r * r * s / I0;
            for (int k = lane; k < I0; k += 64) dzb[k] = r * gr[cur][k] - zb[k] * k3;
        }
    } else {
        for (int k = tid; k < I0; k += kMapThreads) dzb[k] = gr[cur][k];
    }
}

// ---- the chip-wide form: one launch per layer (a layer boundary is a launch boundary; nothing waits on another workgroup) ----------
// Launch of layer l: workgroup (x, y, z) owns the input columns [128 x, 128 x + 128), the output rows [32 y, 32 y + 32) and the batch
// rows [8 z, 8 z + 8).  Prologue: the gradient of its 32 x 8 pre-activation sums - the head (sum_l coefs[l] * g[b, l, o]) in the first
// launch, the slots of the launch before it added in slot order otherwise - times gain * slope(h) * wscale, into LDS.  Main loop: a
// thread holds the float4 accumulators of one 16-byte chunk of a W row for the 8 batch rows and walks 4 output rows, so W is read
// once per batch tile; the 8 row sub-groups of the workgroup are added through LDS in a fixed order and the result goes, with plain
// stores, to slot y of the workspace ([slot][B][512] floats, two such buffers used alternately; nothing is zeroed beforehand).  The
// tail launch (one workgroup per sample) adds layer 0's slots and applies the pixel-norm adjoint with mapping_bwd_kernel's
// arithmetic.  Every sum has one fixed order and a batch row never meets another row's values: the same bits every run, in either
// reduction mode, and for a row alone or inside a batch.
constexpr int kWideThreads = 256;
constexpr int kWideCols = 128;                               // input columns of a workgroup: 32 chunks of 16 bytes
constexpr int kWideSubs = kWideThreads / (kWideCols / 4);    // row sub-groups of a workgroup (8)
constexpr int kWideSubRows = 4;                              // output rows a thread walks
constexpr int kWideRows = kWideSubs * kWideSubRows;          // output rows of a workgroup (32) = rows behind one slot
constexpr int kWideBT = 8;                                   // batch rows whose accumulators a thread holds
constexpr int kWideMaxSlots = (kMapMaxWidth + kWideRows - 1) / kWideRows;   // 16
static_assert(kWideRows * kWideBT == kWideThreads, "the prologue maps one thread to one (row, batch row) pair");

struct WideLayer {
    const float* w; const float* h;      // W [O][I]; h: the saved output of this layer [B][O]
    int I, O, act; float gain, wscale;
    const float* g; const float* coefs; int L;      // head (first launch): g [B][L][O], coefs [L] or null
    const float* in; int slots_in;                   // otherwise: the slots the launch before wrote
    float* out; int B;
};

template <bool HEAD>
__global__ __launch_bounds__(kWideThreads) void mapping_bwd_wide_layer_kernel(WideLayer p) {
    __shared__ float gs[kWideRows][kWideBT];
    __shared__ float part[kWideSubs][kWideBT][kWideCols];     // 32 KB
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kWideCols, o0 = blockIdx.y * kWideRows, b0 = blockIdx.z * kWideBT;
    const int nb = min(kWideBT, p.B - b0);
    {
        const int r = tid % kWideRows, bb = tid / kWideRows, o = o0 + r, b = b0 + bb;
        float v = 0.f;
        if (o < p.O && bb < nb) {
            if (HEAD) {
                const float* __restrict__ gb = p.g + (size_t)b * p.L * p.O;
                for (int l = 0; l < p.L; l++) v += (p.coefs ? p.coefs[l] : 1.f) * gb[(size_t)l * p.O + o];
            } else {
                for (int s = 0; s < p.slots_in; s++) v += p.in[((size_t)s * p.B + b) * kMapMaxWidth + o];
            }
            const float hv = p.h[(size_t)b * p.O + o];
            const float slope = p.act == DGE_ACT_LRELU ? (hv > 0.f ? 1.f : 0.2f) : (p.act == DGE_ACT_RELU ? (hv > 0.f ? 1.f : 0.f) : 1.f);
            v *= p.gain * slope * p.wscale;
        }
        gs[r][bb] = v;
    }
    __syncthreads();
    const int ch = tid % (kWideCols / 4), sub = tid / (kWideCols / 4), i4 = c0 + ch * 4;
    float4 acc[kWideBT];
#pragma unroll
    for (int bb = 0; bb < kWideBT; bb++) acc[bb] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i4 < p.I) {                                   // I % 4 == 0, W 16-byte aligned (checked at the C ABI)
#pragma unroll
        for (int k = 0; k < kWideSubRows; k++) {
            const int r = sub * kWideSubRows + k, o = o0 + r;
            if (o < p.O) {
                const float4 w = *reinterpret_cast<const float4*>(p.w + (size_t)o * p.I + i4);
#pragma unroll
                for (int bb = 0; bb < kWideBT; bb++) {
                    if (bb < nb) {
                        const float go = gs[r][bb];
                        acc[bb].x += go * w.x; acc[bb].y += go * w.y; acc[bb].z += go * w.z; acc[bb].w += go * w.w;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int bb = 0; bb < kWideBT; bb++) *reinterpret_cast<float4*>(&part[sub][bb][ch * 4]) = acc[bb];
    __syncthreads();
    for (int e = tid; e < nb * kWideCols; e += kWideThreads) {
        const int bb = e / kWideCols, c = e % kWideCols;
        float v = part[0][bb][c];
#pragma unroll
        for (int k = 1; k < kWideSubs; k++) v += part[k][bb][c];
        if (c0 + c < p.I) p.out[((size_t)blockIdx.y * p.B + b0 + bb) * kMapMaxWidth + c0 + c] = v;
    }
}

__global__ __launch_bounds__(kWideThreads) void mapping_bwd_wide_tail_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ in,
                                                                             int slots_in, int I0, int B, float* __restrict__ dz, int lddz,
                                                                             int pixelnorm, float eps) {
    __shared__ float gr[kMapMaxWidth];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* __restrict__ zb = z + (size_t)b * ldz;
    float* __restrict__ dzb = dz + (size_t)b * lddz;
    for (int i = tid; i < I0; i += kWideThreads) {
        float v = 0.f;
        for (int s = 0; s < slots_in; s++) v += in[((size_t)s * B + b) * kMapMaxWidth + i];
        gr[i] = v;
    }
    __syncthreads();
    if (!pixelnorm) {
        for (int k = tid; k < I0; k += kWideThreads) dzb[k] = gr[k];
    } else if (wave == 0) {          // y = x*r, r = rsqrt(mean(x^2) + eps)  ->  dx = r*dy - x * r^3/I0 * sum(dy*x)
        float q = 0.f, s = 0.f;
        for (int i = lane; i < I0; i += 64) { const float v = zb[i]; q += v * v; }
        q = wave_sum(q);
        const float r = rsqrtf(q / I0 + eps);
        for (int k = lane; k < I0; k += 64) s += gr[k] * zb[k];
        s = wave_sum(s);
        const float k3 = r * r * r * s / I0;
        for (int k = lane; k < I0; k += 64) dzb[k] = r * gr[k] - zb[k] * k3;
    }
}

}  // namespace

extern "C" int dge_mapping_bwd(const float* z, int ldz, const dge_dense_layer* layers, int n, const float* const* acts, const float* g,
                               int L, const float* coefs, float* dz, int lddz, int B, int pixelnorm, float eps, hipStream_t s) {
    DGE_CHECK(z && g && dz && layers && n >= 1 && n <= kMapMaxLayers && B >= 1 && L >= 1, "mapping_bwd: 1 .. %d layers, B >= 1, L >= 1",
              kMapMaxLayers);
    MapChain c;
    c.n = n;
    for (int l = 0; l < n; l++) {
        const dge_dense_layer& Ly = layers[l];
        DGE_CHECK(Ly.w && Ly.I >= 1 && Ly.I <= kMapMaxWidth && Ly.O >= 1 && Ly.O <= kMapMaxWidth && (l == 0 || Ly.I == layers[l - 1].O),
                  "mapping_bwd: layer %d: widths up to %d, I = previous O", l, kMapMaxWidth);
        DGE_CHECK(Ly.I % 4 == 0 && ((uintptr_t)Ly.w & 15) == 0, "mapping_bwd: layer %d: input width a multiple of 4, weight 16-byte aligned", l);
        DGE_CHECK(Ly.act == DGE_ACT_NONE || Ly.act == DGE_ACT_LRELU || Ly.act == DGE_ACT_RELU, "mapping_bwd: activation %d", Ly.act);
        DGE_CHECK(Ly.gain > 0.f, "mapping_bwd: layer %d: gain must be positive (the activation mask is read off the output)", l);
        c.w[l] = Ly.w; c.bias[l] = Ly.bias; c.I[l] = Ly.I; c.O[l] = Ly.O; c.act[l] = Ly.act;
        c.wscale[l] = Ly.wscale; c.bscale[l] = Ly.bscale; c.add[l] = Ly.add; c.gain[l] = Ly.gain;
        c.act_out[l] = acts ? acts[l] : nullptr;
        DGE_CHECK(!acts || acts[l], "mapping_bwd: saved output of layer %d missing", l);
    }
    DGE_CHECK(ldz >= c.I[0] && lddz >= c.I[0], "mapping_bwd: row strides below the input width");
    hipLaunchKernelGGL(mapping_bwd_kernel, dim3(B), dim3(kMapThreads), 0, s, z, ldz, c, g, L, coefs, dz, lddz, pixelnorm ? 1 : 0, eps);
    DGE_LAUNCH_CHECK("mapping_bwd");
    return 0;
}

extern "C" int dge_mapping_bwd_wide_work_bytes(int B) {
    const long long n = (long long)2 * kWideMaxSlots * kMapMaxWidth * sizeof(float) * B;      // two [16][B][512] f32 slot buffers
    if (B < 1 || n >= (1ll << 31)) { dge_set_error("mapping_bwd_wide_work_bytes: B = %d out of range", B); return -1; }
    return (int)n;
}

extern "C" int dge_mapping_bwd_wide(const float* z, int ldz, const dge_dense_layer* layers, int n, const float* const* acts, const float* g,
                                    int L, const float* coefs, float* dz, int lddz, int B, int pixelnorm, float eps, void* work,
                                    long long work_bytes, hipStream_t s) {
    DGE_CHECK(z && g && dz && layers && n >= 1 && n <= kMapMaxLayers && B >= 1 && L >= 1, "mapping_bwd_wide: 1 .. %d layers, B >= 1, L >= 1",
              kMapMaxLayers);
    DGE_CHECK(acts, "mapping_bwd_wide: the saved layer outputs are required (dge_mapping_bwd has the recompute form)");
    DGE_CHECK(B <= 32767, "mapping_bwd_wide: B up to 32767");
    DGE_CHECK(work && ((uintptr_t)work & 15) == 0 && work_bytes >= dge_mapping_bwd_wide_work_bytes(B),
              "mapping_bwd_wide: workspace of dge_mapping_bwd_wide_work_bytes(B) bytes, 16-byte aligned");
    for (int l = 0; l < n; l++) {
        const dge_dense_layer& Ly = layers[l];
        DGE_CHECK(Ly.w && Ly.I >= 1 && Ly.I <= kMapMaxWidth && Ly.O >= 1 && Ly.O <= kMapMaxWidth && (l == 0 || Ly.I == layers[l - 1].O),
                  "mapping_bwd_wide: layer %d: widths up to %d, I = previous O", l, kMapMaxWidth);
        DGE_CHECK(Ly.I % 4 == 0 && ((uintptr_t)Ly.w & 15) == 0, "mapping_bwd_wide: layer %d: input width a multiple of 4, weight 16-byte aligned", l);
        DGE_CHECK(Ly.act == DGE_ACT_NONE || Ly.act == DGE_ACT_LRELU || Ly.act == DGE_ACT_RELU, "mapping_bwd_wide: activation %d", Ly.act);
        DGE_CHECK(Ly.gain > 0.f, "mapping_bwd_wide: layer %d: gain must be positive (the activation mask is read off the output)", l);
        DGE_CHECK(acts[l], "mapping_bwd_wide: saved output of layer %d missing", l);
    }
    DGE_CHECK(ldz >= layers[0].I && lddz >= layers[0].I, "mapping_bwd_wide: row strides below the input width");
    float* buf[2] = {static_cast<float*>(work), static_cast<float*>(work) + (size_t)kWideMaxSlots * B * kMapMaxWidth};
    const int btiles = (B + kWideBT - 1) / kWideBT;
    int slots = 0, cur = 0;
    for (int l = n - 1; l >= 0; l--) {
        const dge_dense_layer& Ly = layers[l];
        WideLayer p;
        p.w = Ly.w; p.h = acts[l]; p.I = Ly.I; p.O = Ly.O; p.act = Ly.act; p.gain = Ly.gain; p.wscale = Ly.wscale;
        p.g = g; p.coefs = coefs; p.L = L; p.in = buf[cur ^ 1]; p.slots_in = slots; p.out = buf[cur]; p.B = B;
        slots = (Ly.O + kWideRows - 1) / kWideRows;
        const dim3 grid((Ly.I + kWideCols - 1) / kWideCols, slots, btiles);
        if (l == n - 1) hipLaunchKernelGGL(mapping_bwd_wide_layer_kernel<true>, grid, dim3(kWideThreads), 0, s, p);
        else hipLaunchKernelGGL(mapping_bwd_wide_layer_kernel<false>, grid, dim3(kWideThreads), 0, s, p);
        DGE_LAUNCH_CHECK("mapping_bwd_wide_layer");
        cur ^= 1;
    }
    hipLaunchKernelGGL(mapping_bwd_wide_tail_kernel, dim3(B), dim3(kWideThreads), 0, s, z, ldz, buf[cur ^ 1], slots, layers[0].I, B, dz, lddz,
                       pixelnorm ? 1 : 0, eps);
    DGE_LAUNCH_CHECK("mapping_bwd_wide_tail");
    return 0;
}
