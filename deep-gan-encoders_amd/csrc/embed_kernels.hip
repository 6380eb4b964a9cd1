// Device work of the W+ / encoder inversion loop (embedding_v2.py; reference embedding_v2_styleGAN1.py:71-189,
// embedding_v2_styleGAN2.py:82-210) that would otherwise need host round trips inside a captured iteration:
//   - the latent norm penalty beta*||w1||_p (Tensor.norm(p) over the whole tensor) and its gradient,
//   - the truncation lerp of a W+ code, avg + psi*(w - avg), and its gradient,
//   - the best-loss / best-norm trackers of the reference's `if` chains, kept on the device.
// All small: one workgroup for the reductions (a fixed-order LDS tree, so the same bits every run), a flat grid for the
// element-wise passes.  No atomics.
// The norm and tracker kernels take the row of a batch from the grid (row r works on w + r*n and on element / block r of every
// output and state array): the whole-tensor entry points launch one row, the *_rows ones a row per sample (independent inversions).
#include "common.h"
#include "../../include/dge_hip.h"

namespace {

constexpr int kRedThreads = 256;

__device__ __forceinline__ float ipow_abs(float x, int p) {      // |x|^p for an integer p >= 0
    const float a = fabsf(x);
    float r = 1.f;
    for (int i = 0; i < p; i++) r *= a;
    return r;
}

// row r = blockIdx.x: out[r] = (sum |w[r]|^p)^(1/p); out_l2[r] = sqrt(sum w[r]^2) when out_l2 != nullptr (either output may be null)
__global__ void __launch_bounds__(kRedThreads) pnorm_fwd_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                                float* __restrict__ out_l2, long n, int p) {
    __shared__ float sp[kRedThreads];
    __shared__ float s2[kRedThreads];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    w += row * n;
    float ap = 0.f, a2 = 0.f;
    for (long i = t; i < n; i += kRedThreads) {
        const float v = w[i];
        ap += ipow_abs(v, p);
        a2 += v * v;
    }
    sp[t] = ap;
    s2[t] = a2;
    __syncthreads();
    for (int h = kRedThreads / 2; h > 0; h >>= 1) {
        if (t < h) {
            sp[t] += sp[t + h];
            s2[t] += s2[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float s = sp[0];
        if (out) out[row] = p == 1 ? s : (p == 2 ? sqrtf(s) : powf(s, 1.f / (float)p));
        if (out_l2) out_l2[row] = sqrtf(s2[0]);
    }
}

// row r = blockIdx.y: g[r][i] += beta * gout[r] * sign(w)|w|^(p-1) / ||w[r]||_p^(p-1); 0 where ||w[r]||_p == 0
__global__ void pnorm_bwd_kernel(const float* __restrict__ w, const float* __restrict__ norm, const float* __restrict__ gout,
                                 float* __restrict__ g, long n, int p, float beta) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = blockIdx.y;
    w += row * n;
    g += row * n;
    const float nrm = norm[row];
    const float scale = beta * (gout ? gout[row] : 1.f);
    const float v = w[i];
    float d = 0.f;
    if (nrm > 0.f) {
        const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
        if (p == 1) d = sg;
        else if (p == 2) d = v / nrm;
        else d = sg * ipow_abs(v, p - 1) / ipow_abs(nrm, p - 1);
    }
    g[i] += scale * d;
}

// out[b,l,d] = avg[l*avg_stride + d] + psi*(w[b,l,d] - avg[...])
__global__ void wplus_lerp_kernel(const float* __restrict__ w, const float* __restrict__ avg, int avg_stride, float psi,
                                  float* __restrict__ out, long n, int L, int D) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int d = (int)(i % D), l = (int)((i / D) % L);
    const float a = avg[(size_t)l * avg_stride + d];
    out[i] = a + psi * (w[i] - a);
}

// gw = psi * g (accumulate: gw += psi * g)
__global__ void wplus_lerp_bwd_kernel(const float* __restrict__ g, float psi, float* __restrict__ gw, long n, int accumulate) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = psi * g[i];
    gw[i] = accumulate ? gw[i] + v : v;
}

// One call per iteration, after the second optimizer step.  istate: [iteration, events written (total), events dropped, armed];
// fstate: [min_loss, min_norm].  Iteration k (0-based, as `iteration` in the reference) is istate[0] on entry.
//   rule DGE_TRACK_ARM_AT:    at k == arm_iter: min_loss := loss; checks from k on       (embedding_v2_styleGAN1.py:128-131)
//   rule DGE_TRACK_ARM_AFTER: checks for k > arm_iter                                   (embedding_v2_styleGAN2.py:153-166)
// check: min_loss > loss*loss_hyst -> min_loss := loss, event kind 0, best_loss_w := w;
//        (norm_hyst > 0) min_norm > norm*norm_hyst -> min_norm := norm, event kind 1, best_norm_w := w.
// Event e goes to ring slot e % cap as (iteration, kind, loss, norm); slots of dropped events are overwritten by later ones.
// Row r = blockIdx.x has a tracker of its own: loss[r], norm[r], w[r][n], istate[r][4], fstate[r][2], events[r][cap][4], best_*[r][n].
__global__ void __launch_bounds__(kRedThreads) embed_track_kernel(const float* __restrict__ loss, const float* __restrict__ norm,
                                                                  const float* __restrict__ w, long n, int* istate, float* fstate,
                                                                  float* best_loss_w, float* best_norm_w, float* events, int cap,
                                                                  int arm_rule, int arm_iter, float loss_hyst, float norm_hyst) {
    __shared__ int take[2];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    loss += row; norm += row; w += row * n;
    istate += row * 4; fstate += row * 2; events += row * (size_t)cap * 4;
    best_loss_w += row * n; best_norm_w += row * n;
    if (t == 0) {
        const int it = istate[0];
        const float l = loss[0], nr = norm[0];
        int armed;
        if (arm_rule == DGE_TRACK_ARM_AT) {
            if (it == arm_iter) fstate[0] = l;
            armed = it >= arm_iter;
        } else {
            armed = it > arm_iter;
        }
        int tl = 0, tn = 0;
        if (armed) {
            if (fstate[0] > l * loss_hyst) {
                fstate[0] = l;
                tl = 1;
            }
            if (norm_hyst > 0.f && fstate[1] > nr * norm_hyst) {
                fstate[1] = nr;
                tn = 1;
            }
        }
        int cnt = istate[1];
        for (int k = 0; k < 2; k++) {
            if (!(k == 0 ? tl : tn)) continue;
            float* e = events + (size_t)(cnt % cap) * 4;
            e[0] = (float)it;
            e[1] = (float)k;
            e[2] = l;
            e[3] = nr;
            cnt++;
        }
        istate[1] = cnt;
        istate[2] = cnt > cap ? cnt - cap : 0;
        istate[3] = armed;
        istate[0] = it + 1;
        take[0] = tl;
        take[1] = tn;
    }
    __syncthreads();
    const int tl = take[0], tn = take[1];
    if (!tl && !tn) return;
    for (long i = t; i < n; i += kRedThreads) {
        const float v = w[i];
        if (tl) best_loss_w[i] = v;
        if (tn) best_norm_w[i] = v;
    }
}

inline unsigned grid_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// =================================================================== C ABI
extern "C" int dge_latent_pnorm_fwd(const float* w, float* out, float* out_l2, long n, int p, hipStream_t s) {
    DGE_CHECK(n > 0, "latent_pnorm_fwd: n = %ld", n);
    DGE_CHECK(p >= 1 && p <= 16, "latent_pnorm_fwd: p = %d (integer 1..16)", p);
    DGE_CHECK(out || out_l2, "latent_pnorm_fwd: no output");
    hipLaunchKernelGGL(pnorm_fwd_kernel, dim3(1), dim3(kRedThreads), 0, s, w, out, out_l2, n, p);
    DGE_LAUNCH_CHECK("latent_pnorm_fwd");
    return 0;
}

extern "C" int dge_latent_pnorm_bwd(const float* w, const float* norm, const float* gout, float* g, long n, int p, float beta,
                                    hipStream_t s) {
    DGE_CHECK(n > 0, "latent_pnorm_bwd: n = %ld", n);
    DGE_CHECK(p >= 1 && p <= 16, "latent_pnorm_bwd: p = %d (integer 1..16)", p);
    hipLaunchKernelGGL(pnorm_bwd_kernel, dim3(grid_of(n)), dim3(256), 0, s, w, norm, gout, g, n, p, beta);
    DGE_LAUNCH_CHECK("latent_pnorm_bwd");
    return 0;
}

extern "C" int dge_wplus_lerp(const float* w, const float* avg, int avg_stride, float psi, float* out, int B, int L, int D,
                              hipStream_t s) {
    DGE_CHECK(B > 0 && L > 0 && D > 0, "wplus_lerp: bad shape [%d,%d,%d]", B, L, D);
    DGE_CHECK(avg_stride == 0 || avg_stride == D, "wplus_lerp: avg_stride %d (0 for avg [D], D for avg [L,D])", avg_stride);
    const long n = (long)B * L * D;
    hipLaunchKernelGGL(wplus_lerp_kernel, dim3(grid_of(n)), dim3(256), 0, s, w, avg, avg_stride, psi, out, n, L, D);
    DGE_LAUNCH_CHECK("wplus_lerp");
    return 0;
}

extern "C" int dge_wplus_lerp_bwd(const float* g, float psi, float* gw, long n, int accumulate, hipStream_t s) {
    DGE_CHECK(n > 0, "wplus_lerp_bwd: n = %ld", n);
    hipLaunchKernelGGL(wplus_lerp_bwd_kernel, dim3(grid_of(n)), dim3(256), 0, s, g, psi, gw, n, accumulate);
    DGE_LAUNCH_CHECK("wplus_lerp_bwd");
    return 0;
}

extern "C" int dge_embed_track(const float* loss, const float* norm, const float* w, long n, int* istate, float* fstate,
                               float* best_loss_w, float* best_norm_w, float* events, int cap, int arm_rule, int arm_iter,
                               float loss_hyst, float norm_hyst, hipStream_t s) {
    DGE_CHECK(n > 0 && cap > 0, "embed_track: n = %ld, cap = %d", n, cap);
    DGE_CHECK(arm_rule == DGE_TRACK_ARM_AT || arm_rule == DGE_TRACK_ARM_AFTER, "embed_track: arm_rule %d", arm_rule);
    hipLaunchKernelGGL(embed_track_kernel, dim3(1), dim3(kRedThreads), 0, s, loss, norm, w, n, istate, fstate, best_loss_w,
                       best_norm_w, events, cap, arm_rule, arm_iter, loss_hyst, norm_hyst);
    DGE_LAUNCH_CHECK("embed_track");
    return 0;
}

// ---- a row per sample: B independent inversions in one batch
extern "C" int dge_latent_pnorm_rows_fwd(const float* w, float* out, float* out_l2, int B, long n, int p, hipStream_t s) {
    DGE_CHECK(B >= 1 && n > 0, "latent_pnorm_rows_fwd: B = %d, n = %ld", B, n);
    DGE_CHECK(p >= 1 && p <= 16, "latent_pnorm_rows_fwd: p = %d (integer 1..16)", p);
    DGE_CHECK(w && (out || out_l2), "latent_pnorm_rows_fwd: no input or no output");
    hipLaunchKernelGGL(pnorm_fwd_kernel, dim3(B), dim3(kRedThreads), 0, s, w, out, out_l2, n, p);
    dge_note_kernel("latent_pnorm_rows_fwd");
    DGE_LAUNCH_CHECK("latent_pnorm_rows_fwd");
    return 0;
}

extern "C" int dge_latent_pnorm_rows_bwd(const float* w, const float* norm, const float* gout, float* g, int B, long n, int p,
                                         float beta, hipStream_t s) {
    DGE_CHECK(B >= 1 && B <= 65535 && n > 0, "latent_pnorm_rows_bwd: B = %d, n = %ld", B, n);
    DGE_CHECK(p >= 1 && p <= 16, "latent_pnorm_rows_bwd: p = %d (integer 1..16)", p);
    DGE_CHECK(w && norm && g, "latent_pnorm_rows_bwd: null argument");
    hipLaunchKernelGGL(pnorm_bwd_kernel, dim3(grid_of(n), B), dim3(256), 0, s, w, norm, gout, g, n, p, beta);
    dge_note_kernel("latent_pnorm_rows_bwd");
    DGE_LAUNCH_CHECK("latent_pnorm_rows_bwd");
    return 0;
}

extern "C" int dge_embed_track_rows(const float* loss, const float* norm, const float* w, int B, long n, int* istate, float* fstate,
                                    float* best_loss_w, float* best_norm_w, float* events, int cap, int arm_rule, int arm_iter,
                                    float loss_hyst, float norm_hyst, hipStream_t s) {
    DGE_CHECK(B >= 1 && n > 0 && cap > 0, "embed_track_rows: B = %d, n = %ld, cap = %d", B, n, cap);
    DGE_CHECK(arm_rule == DGE_TRACK_ARM_AT || arm_rule == DGE_TRACK_ARM_AFTER, "embed_track_rows: arm_rule %d", arm_rule);
    DGE_CHECK(loss && norm && w && istate && fstate && best_loss_w && best_norm_w && events, "embed_track_rows: null argument");
    hipLaunchKernelGGL(embed_track_kernel, dim3(B), dim3(kRedThreads), 0, s, loss, norm, w, n, istate, fstate, best_loss_w,
                       best_norm_w, events, cap, arm_rule, arm_iter, loss_hyst, norm_hyst);
    dge_note_kernel("embed_track_rows");
    DGE_LAUNCH_CHECK("embed_track_rows");
    return 0;
}
