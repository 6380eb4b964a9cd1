// Noise-map optimisation of a StyleGAN2 inversion: the gradient w.r.t. the per-layer noise inputs, the noise regulariser of
// StyleGAN2's projector with its gradient, and the renormalisation of the maps after the optimiser step.
// Nothing here uses atomics or a pre-zeroed buffer: partial sums go to slots of their own and are added in a fixed order, so the
// bits are the same from run to run, in both reduction modes, and for a row alone or inside a batch.
#include "common.h"
#include "../../include/dge_hip.h"

namespace {

// ------------------------------------------------------------------ g_noise
// Forward (stylegan2_generator.py:905-921): z = yraw*d + noise*ns + bias ; x = lrelu(z)*gain, so
//   g_noise[n, p] = ns * sum_{b reads map n} sum_c g_z[b, p, c],   g_z = g_x * gain * lrelu'(x).
// FORM_B: g is g_x and the kernel applies gain * lrelu'(x); else g is g_z.  Thread t owns the 16-byte chunk (t % cpt) of pixel slot
// (t / cpt), as in modconv_bwd_prep_kernel; a shared map (gridDim.y == 1 < B) takes the rows in ascending b in the thread's own
// accumulator.  The chunks of a pixel combine by an xor butterfly inside the wave; a pixel of more than 64 chunks (512 f32
// channels) spans 2 or 4 whole waves, whose totals meet in LDS and are added in wave order.
template <typename T, bool FORM_B>
__global__ __launch_bounds__(256) void s2_noise_grad_kernel(const T* __restrict__ g, const T* __restrict__ x, const float* __restrict__ nsp,
                                                             float* __restrict__ out, int B, int HW, int C, float gain, int accumulate) {
    constexpr int EP = Elem<T>::PER16;
    __shared__ float red[4];
    const int cpt = C / EP, ppi = 256 / cpt;
    const int chunk = threadIdx.x % cpt, slot = threadIdx.x / cpt;
    const int b0 = gridDim.y == 1 ? 0 : blockIdx.y, b1 = gridDim.y == 1 ? B : b0 + 1;
    const float ns = nsp[0], gpos = gain, gneg = 0.2f * gain;
    for (int p0 = blockIdx.x * ppi; p0 < HW; p0 += gridDim.x * ppi) {          // (trip count uniform over the workgroup)
        const int p = p0 + slot;
        const bool live = p < HW;
        float acc = 0.f;
        if (live) {
            for (int b = b0; b < b1; b++) {
                const size_t o = ((size_t)b * HW + p) * C + chunk * EP;
                float gv[EP];
                unpack16(*(const uint4*)(g + o), gv, (T*)nullptr);
                if (FORM_B) {
                    float xv[EP];
                    unpack16(*(const uint4*)(x + o), xv, (T*)nullptr);
#pragma unroll
                    for (int e = 0; e < EP; e++) acc = fmaf(gv[e], xv[e] > 0.f ? gpos : gneg, acc);
                } else {
#pragma unroll
                    for (int e = 0; e < EP; e++) acc += gv[e];
                }
            }
        }
        if (cpt <= 64) {
            for (int o = cpt >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        } else {
            acc = wave_sum(acc);
            __syncthreads();
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
            __syncthreads();
            const int wpp = cpt >> 6;
            acc = 0.f;
            for (int w = 0; w < wpp; w++) acc += red[slot * wpp + w];
        }
        if (live && chunk == 0) {
            const size_t oi = (size_t)blockIdx.y * HW + p;
            const float v = ns * acc;
            out[oi] = accumulate ? out[oi] + v : v;
        }
    }
}

// ------------------------------------------------------------------ regulariser / renormalisation over a table of maps
constexpr int kChunk = 1024;          // elements of a moment / gradient / normalise job: 256 threads x 4

struct Plan {
    const dge_noise_map* maps;
    const dge_noise_job* jobs;
    int nmaps;
    long long n_total, lev_total;
};

// the map of a job with the extents it may touch checked against the buffers (a table that does not fit touches nothing)
__device__ __forceinline__ bool job_map(const Plan& pl, const dge_noise_job& j, int Bn, dge_noise_map& m) {
    if (j.map < 0 || j.map >= pl.nmaps) return false;
    m = pl.maps[j.map];
    if (m.R < 4 || m.R > 1024 || (m.R & (m.R - 1)) || m.nlev < 1 || m.nlev > 8 || (m.R >> (m.nlev - 1)) < 4) return false;
    long long lev = 0;
    for (int l = 1; l < m.nlev; l++) lev += (long long)(m.R >> l) * (m.R >> l);
    return m.off >= 0 && m.off + (long long)Bn * m.R * m.R <= pl.n_total && m.work_off >= 0 && m.work_off + (long long)Bn * lev <= pl.lev_total;
}
// level l of row b of a map: the leaf for l == 0, else the pooled copy in the workspace
__device__ __forceinline__ const float* level_ptr(const dge_noise_map& m, int b, int l, const float* n, const float* work) {
    if (l == 0) return n + m.off + (size_t)b * m.R * m.R;
    size_t lev = 0, o = 0;
    for (int k = 1; k < m.nlev; k++) { const size_t a = (size_t)(m.R >> k) * (m.R >> k); if (k < l) o += a; lev += a; }
    return work + m.work_off + (size_t)b * lev + o;
}

// total of v over the workgroup in a fixed order (xor butterfly, waves in index order), to every thread; red: 4 floats
__device__ __forceinline__ float block_total(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// ordered total of `count` floats `stride` apart, to every thread
__device__ __forceinline__ float slots_total(const float* base, int count, int stride, float* red) {
    float s = 0.f;
    for (int k = threadIdx.x; k < count; k += 256) s += base[(size_t)k * stride];
    return block_total(s, red);
}

// job = (map, source level, tile y, tile x): a tile of up to 32 x 32 of the source level gives its share of up to five pooled
// levels, each from the one before through LDS
__global__ __launch_bounds__(256) void noise_pool_kernel(Plan pl, int job0, const float* __restrict__ n, float* __restrict__ work) {
    __shared__ float buf[2][1024];
    const dge_noise_job j = pl.jobs[job0 + blockIdx.x];
    const int b = blockIdx.y;
    dge_noise_map m;
    if (!job_map(pl, j, gridDim.y, m) || j.level < 0 || j.level >= m.nlev - 1) return;
    const int S = m.R >> j.level, T = S < 32 ? S : 32;
    if (j.a < 0 || j.b < 0 || (j.a + 1) * T > S || (j.b + 1) * T > S) return;
    const float* src = level_ptr(m, b, j.level, n, work);
    for (int i = threadIdx.x; i < T * T; i += 256) buf[0][i] = src[(size_t)(j.a * T + i / T) * S + j.b * T + i % T];
    __syncthreads();
    int cur = 0;
    for (int k = 1; (T >> k) > 0 && j.level + k < m.nlev; k++) {
        const int t = T >> k, s = S >> k;
        float* dst = (float*)level_ptr(m, b, j.level + k, n, work);
        for (int i = threadIdx.x; i < t * t; i += 256) {
            const int yy = i / t, xx = i % t;
            const float* q = &buf[cur][(2 * yy) * (2 * t) + 2 * xx];
            const float v = 0.25f * ((q[0] + q[1]) + (q[2 * t] + q[2 * t + 1]));
            buf[cur ^ 1][i] = v;
            dst[(size_t)(j.a * t + yy) * s + j.b * t + xx] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
}

// job = (map, level, chunk, slot): slot <- (sum n_l * roll(n_l, 1, w), sum n_l * roll(n_l, 1, h)) over the chunk's pixels
__global__ __launch_bounds__(256) void noise_moments_kernel(Plan pl, int job0, int nslots, const float* __restrict__ n,
                                                             const float* __restrict__ work, float* __restrict__ slots) {
    __shared__ float red[4];
    const dge_noise_job j = pl.jobs[job0 + blockIdx.x];
    const int b = blockIdx.y;
    dge_noise_map m;
    if (!job_map(pl, j, gridDim.y, m) || j.level < 0 || j.level >= m.nlev || j.b < 0 || j.b >= nslots) return;
    const int S = m.R >> j.level, N = S * S;
    const float* src = level_ptr(m, b, j.level, n, work);
    float pw = 0.f, ph = 0.f;
    for (int k = 0; k < kChunk / 256; k++) {
        const int i = j.a * kChunk + k * 256 + threadIdx.x;
        if (j.a >= 0 && i < N) {
            const int y = i / S, xx = i % S;
            const float v = src[i];
            pw = fmaf(v, src[y * S + ((xx + S - 1) & (S - 1))], pw);
            ph = fmaf(v, src[((y + S - 1) & (S - 1)) * S + xx], ph);
        }
    }
    pw = block_total(pw, red);
    ph = block_total(ph, red);
    if (threadIdx.x == 0) *(float2*)(slots + ((size_t)b * nslots + j.b) * 2) = make_float2(pw, ph);
}

// one workgroup per row; job = (map, level, first slot, slots) per (map, level) pair: a wave adds a pair's slots in a fixed
// order -> mom[b][pair] = (m_w, m_h); reg[b] = sum over the pairs, in pair order, of m_w^2 + m_h^2
__global__ __launch_bounds__(256) void noise_reg_finalize_kernel(Plan pl, int job0, int npairs, int nslots, const float* __restrict__ slots,
                                                                  float* __restrict__ mom, float* __restrict__ reg) {
    __shared__ float val[256];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    for (int p = threadIdx.x >> 6; p < npairs; p += 4) {
        const dge_noise_job j = pl.jobs[job0 + p];
        float sw = 0.f, sh = 0.f, N = 1.f;
        if (j.map >= 0 && j.map < pl.nmaps && j.level >= 0 && j.level < 8 && j.a >= 0 && j.b >= 0 && j.a + j.b <= nslots) {
            for (int k = lane; k < j.b; k += 64) {
                const float2 v = *(const float2*)(slots + ((size_t)b * nslots + j.a + k) * 2);
                sw += v.x; sh += v.y;
            }
            const int S = pl.maps[j.map].R >> j.level;
            N = (float)S * (float)S;
        }
        sw = wave_sum(sw) / N; sh = wave_sum(sh) / N;
        if (lane == 0) {
            *(float2*)(mom + ((size_t)b * npairs + p) * 2) = make_float2(sw, sh);
            val[p] = sw * sw + sh * sh;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = 0.f;
        for (int p = 0; p < npairs; p++) r += val[p];
        reg[b] = r;
    }
}

// job = (map, 0, chunk, -): grad (+)= scale * d reg / d n at the chunk's pixels; a level's neighbours are taken at the pooled pixel
// that contains the fine one, and 2 / (N_l * 4^l) = 2 / R^2 at every level
__global__ __launch_bounds__(256) void noise_reg_grad_kernel(Plan pl, int job0, int npairs, const float* __restrict__ n,
                                                              const float* __restrict__ work, const float* __restrict__ mom,
                                                              float* __restrict__ grad, float scale, int accumulate) {
    const dge_noise_job j = pl.jobs[job0 + blockIdx.x];
    const int b = blockIdx.y;
    dge_noise_map m;
    if (!job_map(pl, j, gridDim.y, m) || j.a < 0 || m.pair0 < 0 || m.pair0 + m.nlev > npairs) return;
    const int R = m.R, N = R * R;
    const float c = scale * 2.f / (float)N;
    for (int k = 0; k < kChunk / 256; k++) {
        const int i = j.a * kChunk + k * 256 + threadIdx.x;
        if (i >= N) continue;
        const int y = i / R, xx = i % R;
        float acc = 0.f;
        for (int l = 0; l < m.nlev; l++) {
            const int S = R >> l, yl = y >> l, xl = xx >> l;
            const float* q = level_ptr(m, b, l, n, work);
            const float2 mm = *(const float2*)(mom + ((size_t)b * npairs + m.pair0 + l) * 2);
            const float hw = q[yl * S + ((xl + S - 1) & (S - 1))] + q[yl * S + ((xl + 1) & (S - 1))];
            const float hh = q[((yl + S - 1) & (S - 1)) * S + xl] + q[((yl + 1) & (S - 1)) * S + xl];
            acc += mm.x * hw + mm.y * hh;
        }
        const size_t o = (size_t)m.off + (size_t)b * N + i;
        grad[o] = accumulate ? grad[o] + c * acc : c * acc;
    }
}

// job = (map, 0, chunk, slot).  MODE 0: sa[slot] <- sum of the chunk; MODE 1: mean from sa (every workgroup adds the map's slots
// in the same order), sb[slot] <- sum (n - mean)^2; MODE 2: n <- (n - mean) * rsqrt(mean square of n - mean), in place
template <int MODE>
__global__ __launch_bounds__(256) void noise_normalize_kernel(Plan pl, int job0, int nslots, float* __restrict__ n, float* __restrict__ sa,
                                                               float* __restrict__ sb) {
    __shared__ float red[4];
    const dge_noise_job j = pl.jobs[job0 + blockIdx.x];
    const int b = blockIdx.y;
    dge_noise_map m;
    if (!job_map(pl, j, gridDim.y, m) || j.a < 0 || j.b < 0 || j.b >= nslots) return;
    const int N = m.R * m.R, nch = (N + kChunk - 1) / kChunk;
    if (m.cslot0 < 0 || m.cslot0 + nch > nslots || j.a >= nch) return;
    float* p = n + m.off + (size_t)b * N;
    float mean = 0.f, rstd = 1.f;
    if (MODE >= 1) mean = slots_total(sa + (size_t)b * nslots + m.cslot0, nch, 1, red) / (float)N;
    if (MODE == 2) rstd = 1.f / sqrtf(slots_total(sb + (size_t)b * nslots + m.cslot0, nch, 1, red) / (float)N);
    float s = 0.f;
    for (int k = 0; k < kChunk / 256; k++) {
        const int i = j.a * kChunk + k * 256 + threadIdx.x;
        if (i >= N) continue;
        const float v = p[i] - mean;
        if (MODE == 0) s += v;
        if (MODE == 1) s = fmaf(v, v, s);
        if (MODE == 2) p[i] = v * rstd;
    }
    if (MODE < 2) {
        s = block_total(s, red);
        if (threadIdx.x == 0) (MODE == 0 ? sa : sb)[(size_t)b * nslots + j.b] = s;
    }
}

inline int plan_check(const dge_noise_plan* p, const char* what) {
    DGE_CHECK(p && p->maps && p->jobs, "%s: null plan", what);
    DGE_CHECK(p->nmaps >= 1 && p->nmaps <= 32 && p->Bn >= 1 && p->Bn <= 65535, "%s: 1..32 maps, 1..65535 rows", what);
    DGE_CHECK(p->n_pool0 >= 0 && p->n_pool1 >= 0 && p->n_mom >= 1 && p->npairs >= 1 && p->npairs <= 256 && p->n_chunk >= 1,
              "%s: bad job counts", what);
    DGE_CHECK(p->n_total > 0 && p->lev_total >= 0, "%s: bad totals", what);
    return 0;
}
inline long long lev_floats(const dge_noise_plan* p) { return (p->lev_total + 3) & ~3LL; }          // (the slots behind stay 16-byte aligned)
inline long long slot_floats(const dge_noise_plan* p) { return (long long)p->Bn * 2 * (p->n_mom > p->n_chunk ? p->n_mom : p->n_chunk); }
inline Plan device_plan(const dge_noise_plan* p) { return Plan{p->maps, p->jobs, p->nmaps, p->n_total, p->lev_total}; }

}  // namespace

// =================================================================== C ABI
extern "C" int dge_s2_noise_grad(const void* g, const void* x, const float* ns, float* out, int B, int Bn, int HW, int C, float gain,
                                 int accumulate, int dtype, hipStream_t s) {
    const int ep = dtype == DGE_BF16 ? 8 : 4;
    DGE_CHECK(dtype == DGE_BF16 || dtype == DGE_F32, "s2_noise_grad: bad dtype %d", dtype);
    DGE_CHECK(g && ns && out, "s2_noise_grad: null argument");
    DGE_CHECK(B >= 1 && HW >= 1 && (Bn == 1 || Bn == B) && Bn <= 65535, "s2_noise_grad: B = %d, HW = %d, out rows %d (1 or B)", B, HW, Bn);
    DGE_CHECK(C > 0 && C % ep == 0 && C / ep <= 256 && 256 % (C / ep) == 0, "s2_noise_grad: unsupported channel count %d", C);
    DGE_CHECK(!x || gain > 0.f, "s2_noise_grad: gain must be positive");
    const int ppi = 256 / (C / ep);
    int gx = (HW + ppi - 1) / ppi;
    if (gx > 4096) gx = 4096;
    const dim3 grid(gx, Bn);
    const bool bf = dtype == DGE_BF16;
    if (bf && x) hipLaunchKernelGGL((s2_noise_grad_kernel<bf16_t, true>), grid, dim3(256), 0, s, (const bf16_t*)g, (const bf16_t*)x, ns, out, B, HW, C, gain, accumulate);
    else if (bf) hipLaunchKernelGGL((s2_noise_grad_kernel<bf16_t, false>), grid, dim3(256), 0, s, (const bf16_t*)g, (const bf16_t*)nullptr, ns, out, B, HW, C, gain, accumulate);
    else if (x) hipLaunchKernelGGL((s2_noise_grad_kernel<float, true>), grid, dim3(256), 0, s, (const float*)g, (const float*)x, ns, out, B, HW, C, gain, accumulate);
    else hipLaunchKernelGGL((s2_noise_grad_kernel<float, false>), grid, dim3(256), 0, s, (const float*)g, (const float*)nullptr, ns, out, B, HW, C, gain, accumulate);
    dge_note_kernel("s2_noise_grad<%s,%s>", bf ? "bf16" : "f32", x ? "B" : "A");
    DGE_LAUNCH_CHECK("s2_noise_grad");
    return 0;
}

extern "C" int dge_noise_map_size(void) { return (int)sizeof(dge_noise_map); }
extern "C" int dge_noise_job_size(void) { return (int)sizeof(dge_noise_job); }

extern "C" int dge_noise_reg_work_bytes(const dge_noise_plan* p) {
    if (plan_check(p, "noise_reg_work_bytes")) return -1;
    const long long nb = 4 * (lev_floats(p) + slot_floats(p) + (long long)p->Bn * p->npairs * 2);
    DGE_CHECK(nb < (1LL << 31), "noise_reg_work_bytes: a workspace of 2 GiB or more");
    return (int)nb;
}

extern "C" int dge_noise_reg(const dge_noise_plan* p, const float* n, float* reg, float* grad, float scale, int accumulate, void* work,
                             long long work_bytes, hipStream_t s) {
    if (const int rc = plan_check(p, "noise_reg")) return rc;
    DGE_CHECK(n && reg && work && ((uintptr_t)work & 15) == 0, "noise_reg: null argument or unaligned workspace");
    const int need = dge_noise_reg_work_bytes(p);
    if (need < 0) return -1;
    DGE_CHECK(work_bytes >= need, "noise_reg: the workspace holds %lld bytes, %d needed", work_bytes, need);
    const Plan pl = device_plan(p);
    float* lev = (float*)work;
    float* slots = lev + lev_floats(p);
    float* mom = slots + slot_floats(p);
    int job0 = 0;
    if (p->n_pool0) hipLaunchKernelGGL(noise_pool_kernel, dim3(p->n_pool0, p->Bn), dim3(256), 0, s, pl, job0, n, lev);
    job0 += p->n_pool0;
    if (p->n_pool1) hipLaunchKernelGGL(noise_pool_kernel, dim3(p->n_pool1, p->Bn), dim3(256), 0, s, pl, job0, n, lev);
    job0 += p->n_pool1;
    hipLaunchKernelGGL(noise_moments_kernel, dim3(p->n_mom, p->Bn), dim3(256), 0, s, pl, job0, p->n_mom, n, lev, slots);
    job0 += p->n_mom;
    hipLaunchKernelGGL(noise_reg_finalize_kernel, dim3(p->Bn), dim3(256), 0, s, pl, job0, p->npairs, p->n_mom, slots, mom, reg);
    job0 += p->npairs;
    if (grad)
        hipLaunchKernelGGL(noise_reg_grad_kernel, dim3(p->n_chunk, p->Bn), dim3(256), 0, s, pl, job0, p->npairs, n, lev, mom, grad, scale, accumulate);
    dge_note_kernel("noise_reg");
    DGE_LAUNCH_CHECK("noise_reg");
    return 0;
}

extern "C" int dge_noise_normalize_work_bytes(const dge_noise_plan* p) {
    if (plan_check(p, "noise_normalize_work_bytes")) return -1;
    const long long nb = 4 * slot_floats(p);
    DGE_CHECK(nb < (1LL << 31), "noise_normalize_work_bytes: a workspace of 2 GiB or more");
    return (int)nb;
}

extern "C" int dge_noise_normalize(const dge_noise_plan* p, float* n, void* work, long long work_bytes, hipStream_t s) {
    if (const int rc = plan_check(p, "noise_normalize")) return rc;
    DGE_CHECK(n && work, "noise_normalize: null argument");
    const int need = dge_noise_normalize_work_bytes(p);
    if (need < 0) return -1;
    DGE_CHECK(work_bytes >= need, "noise_normalize: the workspace holds %lld bytes, %d needed", work_bytes, need);
    const Plan pl = device_plan(p);
    float* sa = (float*)work;
    float* sb = sa + (size_t)p->Bn * p->n_chunk;
    const int job0 = p->n_pool0 + p->n_pool1 + p->n_mom + p->npairs;
    const dim3 grid(p->n_chunk, p->Bn);
    hipLaunchKernelGGL(noise_normalize_kernel<0>, grid, dim3(256), 0, s, pl, job0, p->n_chunk, n, sa, sb);
    hipLaunchKernelGGL(noise_normalize_kernel<1>, grid, dim3(256), 0, s, pl, job0, p->n_chunk, n, sa, sb);
    hipLaunchKernelGGL(noise_normalize_kernel<2>, grid, dim3(256), 0, s, pl, job0, p->n_chunk, n, sa, sb);
    dge_note_kernel("noise_normalize");
    DGE_LAUNCH_CHECK("noise_normalize");
    return 0;
}
