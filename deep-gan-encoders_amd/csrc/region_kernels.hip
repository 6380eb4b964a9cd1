// Kernels behind the region directions of StyleGAN2 (dge_amd.region_directions, ReSeFa): the W+ codes of a group of finite-
// difference pairs, the pooled image difference that is a row of the Jacobian operand X [K,N], the two mask-weighted Gram matrices
// of X from one read of it, and the small matrix products of the generalised eigensolve.  All f32 in and out.  Nothing here uses
// atomics or a pre-zeroed buffer: the Gram's partial tiles go to slots of the caller's workspace and are added in chunk order by a
// second launch, so the bits are the same from run to run and in both reduction modes.  No workgroup waits for another one.
#include "common.h"
#include "../../include/dge_hip.h"

namespace {

// ------------------------------------------------------------------ weighted Gram matrices of a K-major operand
constexpr int kTile = 64;            // a workgroup owns a 64 x 64 tile of the upper triangle, a thread 4 x 4 of it
constexpr int kStage = 32;           // columns staged in LDS at a time: a row's 32 consecutive floats are one 128-byte read
constexpr int kLd = kStage + 4;      // LDS row stride: rows stay 16-byte aligned, and the 16 rows a 16-lane group reads with
                                     // ds_read_b128 fall on 16 different 16-byte slots (9 * tx mod 16 is a bijection)
constexpr long long kChunkMin = 4096, kChunksMax = 256;

// columns of a chunk: 4096 up to N = 2^20, beyond that N / 256 rounded up to whole stages (at most 256 chunks: the workspace of
// K = 512 stays near 300 MB at N = 3 * 1024^2)
inline long long cols_chunk(long long N) {
    const long long c = (N + kChunksMax - 1) / kChunksMax;
    return c <= kChunkMin ? kChunkMin : (c + kStage - 1) / kStage * kStage;
}
inline int cols_tiles(int K) { const int T = (K + kTile - 1) / kTile; return T * (T + 1) / 2; }

// (ti, tj), ti <= tj, of upper-triangle tile number t in row-major order over T tile columns
__device__ __forceinline__ void tile_of(int t, int T, int& ti, int& tj) {
    int i = 0;
    while (t >= T - i) { t -= T - i; i++; }
    ti = i; tj = i + t;
}

// part[o][chunk][tile][64][64] <- sum over the chunk's columns n of x[i,n] * (w_o[n] * x[j,n]), w_0 = w, w_1 = 1.0f - w, columns
// ascending in one f32 accumulator per element and output.  WGT = false: the one output with w = 1 (the product is x[i,n] * x[j,n]).
// Thread (tx, ty) owns rows 4 ty .. 4 ty + 3 of the i side and rows tx, tx + 16, tx + 32, tx + 48 of the j side.
template <bool WGT>
__global__ __launch_bounds__(256) void gram_cols_partial_kernel(const float* __restrict__ x, int K, unsigned N, long long ldx,
                                                                 const float* __restrict__ wgt, unsigned P, unsigned chunk, int T,
                                                                 float* __restrict__ part, size_t out_stride) {
    __shared__ __attribute__((aligned(16))) float sA[kTile * kLd];
    __shared__ __attribute__((aligned(16))) float sF[kTile * kLd];
    __shared__ __attribute__((aligned(16))) float sB[WGT ? kTile * kLd : 4];
    int ti, tj;
    tile_of(blockIdx.x, T, ti, tj);
    const bool diag = ti == tj;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, sc = tid & 31, sr = tid >> 5;
    const unsigned c0 = blockIdx.y * chunk, c1 = (N - c0 > chunk) ? c0 + chunk : N;
    float accF[4][4], accB[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { accF[i][j] = 0.f; accB[i][j] = 0.f; }
    for (unsigned n0 = c0; n0 < c1; n0 += kStage) {
        const unsigned n = n0 + sc;
        const bool inside = n < c1;
        float w = 1.f, wb = 0.f;
        if (WGT) { w = inside ? wgt[n % P] : 0.f; wb = __fsub_rn(1.0f, w); }
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const int row = sr + 8 * m, gi = ti * kTile + row, gj = tj * kTile + row;
            const float a = (inside && gi < K) ? x[(size_t)gi * ldx + n] : 0.f;
            const float b = diag ? a : ((inside && gj < K) ? x[(size_t)gj * ldx + n] : 0.f);
            sA[row * kLd + sc] = a;
            if (WGT) { sF[row * kLd + sc] = __fmul_rn(w, b); sB[row * kLd + sc] = __fmul_rn(wb, b); }
            else if (!diag) sF[row * kLd + sc] = b;
        }
        __syncthreads();
        const float* pF = (!WGT && diag) ? sA : sF;
#pragma unroll
        for (int k4 = 0; k4 < kStage; k4 += 4) {
            float av[4][4], fv[4][4], bv[4][4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float4 a = *(const float4*)&sA[(ty * 4 + i) * kLd + k4];
                av[i][0] = a.x; av[i][1] = a.y; av[i][2] = a.z; av[i][3] = a.w;
                const float4 f = *(const float4*)&pF[(tx + 16 * i) * kLd + k4];
                fv[i][0] = f.x; fv[i][1] = f.y; fv[i][2] = f.z; fv[i][3] = f.w;
                if (WGT) {
                    const float4 b = *(const float4*)&sB[(tx + 16 * i) * kLd + k4];
                    bv[i][0] = b.x; bv[i][1] = b.y; bv[i][2] = b.z; bv[i][3] = b.w;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        accF[i][j] = __fmaf_rn(av[i][k], fv[j][k], accF[i][j]);
                        if (WGT) accB[i][j] = __fmaf_rn(av[i][k], bv[j][k], accB[i][j]);
                    }
        }
        __syncthreads();
    }
    float* dst = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kTile * kTile);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            dst[(ty * 4 + i) * kTile + tx + 16 * j] = accF[i][j];
            if (WGT) dst[out_stride + (ty * 4 + i) * kTile + tx + 16 * j] = accB[i][j];
        }
}

// out_o[i,j] = out_o[j,i] = scale * (the chunks' partial sums of (i,j), i <= j, in chunk order); blockIdx.y = o
__global__ __launch_bounds__(256) void gram_cols_reduce_kernel(const float* __restrict__ part, int nchunks, int ntiles, int K, int T, float scale,
                                                                float* __restrict__ out_a, float* __restrict__ out_b, size_t out_stride) {
    int ti, tj;
    tile_of(blockIdx.x, T, ti, tj);
    float* out = blockIdx.y ? out_b : out_a;
    part += blockIdx.y * out_stride;
    for (int e = threadIdx.x; e < kTile * kTile; e += 256) {
        const int li = e >> 6, lj = e & 63, gi = ti * kTile + li, gj = tj * kTile + lj;
        if (gi >= K || gj >= K || gi > gj) continue;
        const float* q = part + (size_t)blockIdx.x * (kTile * kTile) + e;
        float s = 0.f;
        for (int c = 0; c < nchunks; c++) s = __fadd_rn(s, q[(size_t)c * ntiles * (kTile * kTile)]);
        s = __fmul_rn(s, scale);
        out[(size_t)gi * K + gj] = s;
        out[(size_t)gj * K + gi] = s;
    }
}

// ------------------------------------------------------------------ pooled finite difference
// x[j, (c, y, x)] = scale * sum over the s x s window of (img[2j] - img[2j+1]), the window in row-major order in one f32 accumulator
// that starts from the window's first difference (s = 1: (a - b) * scale, each operation rounded)
__global__ __launch_bounds__(256) void fd_pool_diff_kernel(const float* __restrict__ img, int C, int H, int W, int s, float scale,
                                                            float* __restrict__ x, long long ldx, long long per_row, long long total) {
#pragma clang fp contract(off)
    const long long e = blockIdx.x * 256LL + threadIdx.x;
    if (e >= total) return;
    const int w = W / s, h = H / s;
    const long long j = e / per_row, r = e % per_row;
    const int px = (int)(r % w), py = (int)((r / w) % h), c = (int)(r / ((long long)w * h));
    const size_t plane = (size_t)H * W, img_elems = (size_t)C * plane;
    const float* a = img + (size_t)(2 * j) * img_elems + (size_t)c * plane + (size_t)(py * s) * W + (size_t)px * s;
    const float* b = a + img_elems;
    float acc = __fsub_rn(a[0], b[0]);
    for (int dy = 0; dy < s; dy++)
        for (int dx = (dy == 0 ? 1 : 0); dx < s; dx++) {
            const size_t o = (size_t)dy * W + dx;
            acc = __fadd_rn(acc, __fsub_rn(a[o], b[o]));
        }
    x[(size_t)j * ldx + r] = __fmul_rn(acc, scale);
}

// ------------------------------------------------------------------ the W+ codes of a group of axis pairs
// out[2j] = fma(h, q_j, wp), out[2j+1] = fma(-h, q_j, wp) on W+ rows r0 .. r1 - 1; the other rows are copies of wp
__global__ __launch_bounds__(256) void wp_axis_pairs_kernel(const float* __restrict__ wp, const float* __restrict__ q, long long ldq, int L, int D,
                                                             int r0, int r1, float h, float* __restrict__ out, long long total) {
    const long long e = blockIdx.x * 256LL + threadIdx.x;
    if (e >= total) return;
    const int d = (int)(e % D), l = (int)((e / D) % L);
    const long long row = e / ((long long)L * D);
    float v = wp[(size_t)l * D + d];
    if (l >= r0 && l < r1) v = __fmaf_rn((row & 1) ? -h : h, q[(size_t)(row >> 1) * ldq + d], v);
    out[e] = v;
}

// ------------------------------------------------------------------ small matrix product, f64 accumulation
// out[m,n] = float(sum_k double(a[m,k]) * double(b(k,n))), k ascending; b(k,n) = b[k*ldb + n] or, trans_b, b[n*ldb + k].  The f64
// product of two f32 values is exact, so the fma is the sum's one rounding per term.
constexpr int kMT = 16;
__global__ __launch_bounds__(256) void matmul_f64acc_kernel(const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
                                                             int trans_b, float* __restrict__ out, long long ldo, int M, int N, int Kk) {
    __shared__ float sA[kMT][kMT + 1], sB[kMT][kMT + 1];          // sA[m][k], sB[k][n]
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m = blockIdx.y * kMT + ty, n = blockIdx.x * kMT + tx;
    double acc = 0.;
    for (int k0 = 0; k0 < Kk; k0 += kMT) {
        sA[ty][tx] = (m < M && k0 + tx < Kk) ? a[(size_t)m * lda + k0 + tx] : 0.f;
        if (trans_b) {
            const int nn = blockIdx.x * kMT + ty;                  // row nn of b, k along the lanes
            sB[tx][ty] = (nn < N && k0 + tx < Kk) ? b[(size_t)nn * ldb + k0 + tx] : 0.f;
        } else {
            sB[ty][tx] = (k0 + ty < Kk && n < N) ? b[(size_t)(k0 + ty) * ldb + n] : 0.f;
        }
        __syncthreads();
        const int kn = Kk - k0 < kMT ? Kk - k0 : kMT;
        for (int k = 0; k < kn; k++) acc = fma((double)sA[ty][k], (double)sB[k][tx], acc);
        __syncthreads();
    }
    if (m < M && n < N) out[(size_t)m * ldo + n] = (float)acc;
}

}  // namespace

// =================================================================== C ABI
extern "C" long long dge_gram_cols_chunk(long long N) {
    DGE_CHECK(N >= 1 && N < (1LL << 31), "gram_cols: 1 <= N < 2^31 columns, got %lld", N);
    return cols_chunk(N);
}

extern "C" long long dge_gram_cols_work_bytes(int K, long long N) {
    DGE_CHECK(K >= 1 && K <= 1024 && N >= 1 && N < (1LL << 31), "gram_cols: 1 <= K <= 1024 rows of 1 <= N < 2^31 columns, got %d x %lld", K, N);
    const long long c = cols_chunk(N), nch = (N + c - 1) / c;
    return 2LL * 4 * nch * cols_tiles(K) * (kTile * kTile);
}

extern "C" int dge_gram_cols(const float* x, int K, long long N, long long ldx, const float* wgt, long long P, float scale, float* out_a,
                             float* out_b, void* work, long long work_bytes, hipStream_t s) {
    const long long need = dge_gram_cols_work_bytes(K, N);
    if (need < 0) return -1;
    DGE_CHECK(x && out_a && work, "gram_cols: null argument");
    DGE_CHECK(ldx >= N, "gram_cols: the row stride %lld is below N = %lld", ldx, N);
    DGE_CHECK(wgt || !out_b, "gram_cols: out_b without a weight is refused (it would be zero)");
    DGE_CHECK(!wgt || (P >= 1 && N % P == 0), "gram_cols: the weight's period P = %lld must divide N = %lld", P, N);
    DGE_CHECK((((uintptr_t)work) & 15) == 0, "gram_cols: work must be 16-byte aligned");
    DGE_CHECK(work_bytes >= need, "gram_cols: the workspace holds %lld bytes, %lld needed", work_bytes, need);
    const int T = (K + kTile - 1) / kTile, ntiles = cols_tiles(K);
    const long long c = cols_chunk(N), nch = (N + c - 1) / c;
    float* part = (float*)work;
    const size_t out_stride = (size_t)nch * ntiles * (kTile * kTile);
    const dim3 grid(ntiles, (unsigned)nch);
    if (wgt)
        hipLaunchKernelGGL(gram_cols_partial_kernel<true>, grid, dim3(256), 0, s, x, K, (unsigned)N, ldx, wgt, (unsigned)P, (unsigned)c, T, part,
                           out_stride);
    else
        hipLaunchKernelGGL(gram_cols_partial_kernel<false>, grid, dim3(256), 0, s, x, K, (unsigned)N, ldx, wgt, 1u, (unsigned)c, T, part,
                           out_stride);
    hipLaunchKernelGGL(gram_cols_reduce_kernel, dim3(ntiles, out_b ? 2 : 1), dim3(256), 0, s, part, (int)nch, ntiles, K, T, scale, out_a, out_b,
                       out_stride);
    DGE_LAUNCH_CHECK("gram_cols");
    dge_note_kernel("gram_cols");
    return 0;
}

extern "C" int dge_fd_pool_diff(const float* img, int n, int C, int H, int W, int s, float scale, float* x, long long ldx, hipStream_t st) {
    DGE_CHECK(img && x, "fd_pool_diff: null argument");
    DGE_CHECK(n >= 1 && C >= 1 && H >= 1 && W >= 1, "fd_pool_diff: n, C, H, W must be positive, got %d %d %d %d", n, C, H, W);
    DGE_CHECK(s >= 1 && H % s == 0 && W % s == 0, "fd_pool_diff: the window %d must divide H = %d and W = %d", s, H, W);
    const long long per_row = (long long)C * (H / s) * (W / s), total = per_row * n;
    DGE_CHECK(ldx >= per_row, "fd_pool_diff: the row stride %lld is below C * (H/s) * (W/s) = %lld", ldx, per_row);
    DGE_CHECK((total + 255) / 256 < (1LL << 31), "fd_pool_diff: too many elements (%lld)", total);
    hipLaunchKernelGGL(fd_pool_diff_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, img, C, H, W, s, scale, x, ldx, per_row,
                       total);
    DGE_LAUNCH_CHECK("fd_pool_diff");
    dge_note_kernel("fd_pool_diff");
    return 0;
}

extern "C" int dge_wp_axis_pairs(const float* wp, const float* q, long long ldq, int n, int L, int D, int r0, int r1, float h, float* out,
                                 hipStream_t s) {
    DGE_CHECK(wp && q && out, "wp_axis_pairs: null argument");
    DGE_CHECK(n >= 1 && L >= 1 && D >= 1, "wp_axis_pairs: n, L, D must be positive, got %d %d %d", n, L, D);
    DGE_CHECK(ldq >= D, "wp_axis_pairs: the row stride %lld of q is below D = %d", ldq, D);
    DGE_CHECK(0 <= r0 && r0 <= r1 && r1 <= L, "wp_axis_pairs: the rows [%d, %d) are outside the %d rows of the code", r0, r1, L);
    const long long total = 2LL * n * L * D;
    DGE_CHECK((total + 255) / 256 < (1LL << 31), "wp_axis_pairs: too many elements (%lld)", total);
    hipLaunchKernelGGL(wp_axis_pairs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wp, q, ldq, L, D, r0, r1, h, out, total);
    DGE_LAUNCH_CHECK("wp_axis_pairs");
    dge_note_kernel("wp_axis_pairs");
    return 0;
}

extern "C" int dge_matmul_f64acc(const float* a, long long lda, const float* b, long long ldb, int trans_b, float* out, long long ldo, int M,
                                 int N, int Kk, hipStream_t s) {
    DGE_CHECK(a && b && out, "matmul_f64acc: null argument");
    DGE_CHECK(M >= 1 && N >= 1 && Kk >= 1 && M <= 1024 && N <= 1024 && Kk <= 1024, "matmul_f64acc: 1 <= M, N, K <= 1024, got %d %d %d", M, N, Kk);
    DGE_CHECK(lda >= Kk && ldo >= N && ldb >= (trans_b ? Kk : N), "matmul_f64acc: a leading dimension is below its row length");
    hipLaunchKernelGGL(matmul_f64acc_kernel, dim3((N + kMT - 1) / kMT, (M + kMT - 1) / kMT), dim3(256), 0, s, a, lda, b, ldb, trans_b, out, ldo, M,
                       N, Kk);
    DGE_LAUNCH_CHECK("matmul_f64acc");
    dge_note_kernel("matmul_f64acc");
    return 0;
}
