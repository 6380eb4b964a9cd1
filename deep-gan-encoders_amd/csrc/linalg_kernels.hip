// Dense linear algebra behind the semantic directions of StyleGAN2 (dge_amd.directions): the Gram matrix of a tall f32 operand
// (SeFa's A^T A over unit rows, GANSpace's covariance of mapped samples) and the eigendecomposition of a symmetric f32 matrix by
// parallel-ordered two-sided Jacobi on an f64 working copy.  Nothing here uses atomics or a pre-zeroed buffer: partial sums go to
// slots of the caller's workspace and are added in a fixed order, so the bits are the same from run to run and in both reduction
// modes.  No workgroup ever waits for another one: every point where all of them must have finished is a launch boundary, and the
// sweep loop is bounded on the host.
#include "common.h"
#include "../../include/dge_hip.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------ Gram matrix
constexpr int kTile = 64;           // a workgroup owns a 64 x 64 tile of the upper triangle, a thread 4 x 4 of it
constexpr int kStep = 16;           // rows staged in LDS at a time
constexpr int kChunk = 512;         // rows of a chunk: one partial tile per (chunk, tile), chunks added in chunk order

// norm[n] = sqrt(sum_d x[n,d]^2): one wave per row, lane-strided f32 sums, the butterfly
__global__ __launch_bounds__(256) void gram_rownorm_kernel(const float* __restrict__ x, long long N, int D, long long ldx,
                                                            float* __restrict__ norm) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;
    const float* q = x + r * ldx;
    float s = 0.f;
    for (int d = threadIdx.x & 63; d < D; d += 64) s = __fmaf_rn(q[d], q[d], s);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) norm[r] = __fsqrt_rn(s);
}

// (ti, tj), ti <= tj, of upper-triangle tile number t in row-major order over T tile columns
__device__ __forceinline__ void gram_tile_of(int t, int T, int& ti, int& tj) {
    int i = 0;
    while (t >= T - i) { t -= T - i; i++; }
    ti = i; tj = i + t;
}

// the f32 operand u[row, col] of the product: x / |x| (a zero row gives zeros), or x - mean, or x; zero outside the matrix
__device__ __forceinline__ float gram_operand(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ norm,
                                              long long row, long long r1, int col, int D, long long ldx) {
    if (row >= r1 || col >= D) return 0.f;
    float v = x[row * ldx + col];
    if (norm) { const float nr = norm[row]; v = nr > 0.f ? __fdiv_rn(v, nr) : 0.f; }
    if (mean) v = __fsub_rn(v, mean[col]);
    return v;
}

// part[chunk][tile][64][64] <- sum over the chunk's rows of u[n, i] * u[n, j], rows ascending in one f32 accumulator per element
__global__ __launch_bounds__(256) void gram_partial_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ norm, long long N, int D, long long ldx, int T,
                                                            float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sA[kStep][kTile];
    __shared__ __attribute__((aligned(16))) float sB[kStep][kTile];
    int ti, tj;
    gram_tile_of(blockIdx.x, T, ti, tj);
    const bool diag = ti == tj;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long r0 = (long long)blockIdx.y * kChunk, r1 = r0 + kChunk < N ? r0 + kChunk : N;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
    for (long long rb = r0; rb < r1; rb += kStep) {
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int e = tid + 256 * m, k = e >> 6, c = e & 63;
            sA[k][c] = gram_operand(x, mean, norm, rb + k, r1, ti * kTile + c, D, ldx);
            if (!diag) sB[k][c] = gram_operand(x, mean, norm, rb + k, r1, tj * kTile + c, D, ldx);
        }
        __syncthreads();
        const float (*pB)[kTile] = diag ? sA : sB;
#pragma unroll
        for (int k = 0; k < kStep; k++) {
            const float4 a = *(const float4*)&sA[k][ty * 4];
            const float4 b = *(const float4*)&pB[k][tx * 4];
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = __fmaf_rn(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
    float* dst = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kTile * kTile);
#pragma unroll
    for (int i = 0; i < 4; i++)
        *(float4*)(dst + (ty * 4 + i) * kTile + tx * 4) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
}

// out[i,j] = out[j,i] = scale * (the chunks' partial sums of (i,j), i <= j, in chunk order)
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ part, int nchunks, int ntiles, int D, int T, float scale,
                                                           float* __restrict__ out) {
    int ti, tj;
    gram_tile_of(blockIdx.x, T, ti, tj);
    for (int e = threadIdx.x; e < kTile * kTile; e += 256) {
        const int li = e >> 6, lj = e & 63, gi = ti * kTile + li, gj = tj * kTile + lj;
        if (gi >= D || gj >= D || gi > gj) continue;
        const float* q = part + (size_t)blockIdx.x * (kTile * kTile) + e;
        float s = 0.f;
        for (int c = 0; c < nchunks; c++) s = __fadd_rn(s, q[(size_t)c * ntiles * (kTile * kTile)]);
        s = __fmul_rn(s, scale);
        out[(size_t)gi * D + gj] = s;
        out[(size_t)gj * D + gi] = s;
    }
}

inline int gram_tiles(int D) { const int T = (D + kTile - 1) / kTile; return T * (T + 1) / 2; }
inline long long gram_chunks(long long N) { return (N + kChunk - 1) / kChunk; }

// ------------------------------------------------------------------ symmetric eigendecomposition
// Two-sided Jacobi in the round-robin order: n = D rounded up to even players, n - 1 rounds of n / 2 disjoint pairs a sweep.  The
// rotations of a round commute, so one launch applies all of them: A' = J^T A J and V' = J^T V (the rows of V are the vectors), out
// of place from one f64 copy into the other.  Every workgroup recomputes the rotation parameters of the rows and columns of its
// tile from the unchanged source copy (the same inputs and the same code: the same bits in every workgroup).
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// every thread of the 256 calls; the total to all threads: butterfly inside a wave, waves in index order
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the partner of index i in round r: player n - 1 stays, the others turn; an index without a partner inside the matrix (odd D:
// the bye) gets itself
__device__ __forceinline__ int jacobi_partner(int i, int r, int n, int D) {
    const int m = n - 1;
    int p;
    if (i == m) p = r;
    else if (i == r) p = m;
    else { p = (2 * r - i) % m; if (p < 0) p += m; }
    return p < D ? p : i;
}

struct JacobiParam { double alpha, beta, dnew; int partner; };
// row i of J^T A = alpha * row i + beta * row partner; dnew = the rotated diagonal element of i
__device__ __forceinline__ JacobiParam jacobi_param(const double* __restrict__ A, int i, int r, int n, int D) {
    JacobiParam q;
    q.alpha = 1.; q.beta = 0.; q.partner = i; q.dnew = 0.;
    if (i >= D) { q.partner = 0; return q; }
    q.dnew = A[(size_t)i * D + i];
    const int p = jacobi_partner(i, r, n, D);
    if (p == i) return q;
    const int lo = i < p ? i : p, hi = i < p ? p : i;
    const double app = A[(size_t)lo * D + lo], aqq = A[(size_t)hi * D + hi], apq = A[(size_t)lo * D + hi];
    q.partner = p;
    if (apq == 0.) return q;
    const double theta = (aqq - app) / (2. * apq);
    const double t = copysign(1., theta) / (fabs(theta) + sqrt(1. + theta * theta));
    const double c = 1. / sqrt(1. + t * t), s = t * c;
    q.alpha = c;
    q.beta = i == lo ? -s : s;
    q.dnew = i == lo ? app - t * apq : aqq + t * apq;
    return q;
}

__global__ __launch_bounds__(256) void jacobi_init_kernel(const float* __restrict__ a, int D, double* __restrict__ A, double* __restrict__ V) {
    const long long e = blockIdx.x * 256LL + threadIdx.x;
    if (e >= (long long)D * D) return;
    const int i = (int)(e / D), j = (int)(e % D);
    A[e] = (double)(i <= j ? a[(size_t)i * D + j] : a[(size_t)j * D + i]);          // the upper triangle only
    V[e] = i == j ? 1. : 0.;
}

constexpr int kJR = 16, kJC = 64;          // rows and columns of a workgroup's tile
__global__ __launch_bounds__(256) void jacobi_round_kernel(const double* __restrict__ A, const double* __restrict__ V, double* __restrict__ A2,
                                                            double* __restrict__ V2, int D, int n, int r) {
    __shared__ double s_alpha[kJR + kJC], s_beta[kJR + kJC], s_dnew[kJR];
    __shared__ int s_part[kJR + kJC];
    const int tid = threadIdx.x, i0 = blockIdx.y * kJR, j0 = blockIdx.x * kJC;
    if (tid < kJR + kJC) {
        const JacobiParam q = jacobi_param(A, tid < kJR ? i0 + tid : j0 + tid - kJR, r, n, D);
        s_alpha[tid] = q.alpha; s_beta[tid] = q.beta; s_part[tid] = q.partner;
        if (tid < kJR) s_dnew[tid] = q.dnew;
    }
    __syncthreads();
    const int lj = tid & 63, j = j0 + lj;
    if (j >= D) return;
    const double aj = s_alpha[kJR + lj], bj = s_beta[kJR + lj];
    const int pj = s_part[kJR + lj];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const int li = (tid >> 6) + 4 * m, i = i0 + li;
        if (i >= D) continue;
        const double ai = s_alpha[li], bi = s_beta[li];
        const int pi = s_part[li];
        const size_t ri = (size_t)i * D, rp = (size_t)pi * D;
        double v;
        if (j == i) v = s_dnew[li];
        else if (j == pi) v = 0.;                                       // the element the rotation annihilates
        else v = ai * (aj * A[ri + j] + bj * A[ri + pj]) + bi * (aj * A[rp + j] + bj * A[rp + pj]);
        A2[ri + j] = v;
        V2[ri + j] = ai * V[ri + j] + bi * V[rp + j];
    }
}

// rowsum[i] = sum_{j > i} A[i,j]^2 and rowsum[D + i] = A[i,i]^2
__global__ __launch_bounds__(256) void jacobi_off_rows_kernel(const double* __restrict__ A, int D, double* __restrict__ rowsum) {
    __shared__ double red[4];
    const int i = blockIdx.x;
    double s = 0.;
    for (int j = i + 1 + threadIdx.x; j < D; j += 256) { const double v = A[(size_t)i * D + j]; s += v * v; }
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) { rowsum[i] = s; const double d = A[(size_t)i * D + i]; rowsum[D + i] = d * d; }
}
// stat[0] = sum of the strict upper triangle's squares, stat[1] = sum of the diagonal's squares: one workgroup, a fixed order
__global__ __launch_bounds__(256) void jacobi_off_total_kernel(const double* __restrict__ rowsum, int D, double* __restrict__ stat) {
    __shared__ double red[4];
    double s = 0., d = 0.;
    for (int i = threadIdx.x; i < D; i += 256) { s += rowsum[i]; d += rowsum[D + i]; }
    s = block_sum_d(s, red);
    d = block_sum_d(d, red);
    if (threadIdx.x == 0) { stat[0] = s; stat[1] = d; }
}

// Workgroup i: the rank of A[i,i] in descending order (equal values by index), then row i of V to row `rank` of evecs in f32 with
// its component of largest magnitude positive (of the f32 values; ties to the lowest index)
__global__ __launch_bounds__(256) void jacobi_finish_kernel(const double* __restrict__ A, const double* __restrict__ V, int D,
                                                             float* __restrict__ evals, float* __restrict__ evecs) {
    __shared__ int s_cnt[256];
    __shared__ float s_val[256];
    __shared__ int s_idx[256];
    __shared__ int s_rank;
    __shared__ float s_sign;
    const int i = blockIdx.x, tid = threadIdx.x;
    const double di = A[(size_t)i * D + i];
    int cnt = 0, bidx = D;
    float best = -1.f;
    for (int j = tid; j < D; j += 256) {
        const double dj = A[(size_t)j * D + j];
        cnt += (dj > di || (dj == di && j < i)) ? 1 : 0;
        const float m = fabsf((float)V[(size_t)i * D + j]);
        if (m > best) { best = m; bidx = j; }
    }
    s_cnt[tid] = cnt; s_val[tid] = best; s_idx[tid] = bidx;
    __syncthreads();
    if (tid == 0) {
        int total = 0, at = D;
        float top = -1.f;
        for (int t = 0; t < 256; t++) {
            total += s_cnt[t];
            if (s_val[t] > top || (s_val[t] == top && s_idx[t] < at)) { top = s_val[t]; at = s_idx[t]; }
        }
        if (at >= D) at = 0;                                           // a row of NaNs: keep the index inside the row
        if (total >= D) total = D - 1;
        s_rank = total;
        s_sign = V[(size_t)i * D + at] < 0. ? -1.f : 1.f;
        evals[total] = (float)di;
    }
    __syncthreads();
    const int rank = s_rank;
    const float sg = s_sign;
    for (int j = tid; j < D; j += 256) evecs[(size_t)rank * D + j] = sg * (float)V[(size_t)i * D + j];
}

constexpr double kJacobiTol = 9.094947017729282e-13;          // 2^-40: off(A) <= tol * |A|_F ends the sweeps

}  // namespace

// =================================================================== C ABI
extern "C" int dge_gram_work_bytes(long long N, int D) {
    DGE_CHECK(N >= 1 && D >= 1 && D <= 1024, "gram: N >= 1 rows of 1 <= D <= 1024 columns, got %lld x %d", N, D);
    const long long nch = gram_chunks(N);
    DGE_CHECK(nch <= 65535, "gram: too many rows (%lld)", N);
    const long long nb = 4 * (nch * gram_tiles(D) * (long long)(kTile * kTile) + ((N + 3) & ~3LL));
    DGE_CHECK(nb < (1LL << 31), "gram: a workspace of 2 GiB or more");
    return (int)nb;
}

extern "C" int dge_gram(const float* x, long long N, int D, long long ldx, const float* mean, int row_norm, float scale, float* out,
                        void* work, long long work_bytes, hipStream_t s) {
    const int need = dge_gram_work_bytes(N, D);
    if (need < 0) return -1;
    DGE_CHECK(x && out && work, "gram: null argument");
    DGE_CHECK(ldx >= D, "gram: the row stride %lld is below D = %d", ldx, D);
    DGE_CHECK(!(row_norm && mean), "gram: row_norm together with mean is refused");
    DGE_CHECK((((uintptr_t)work) & 15) == 0, "gram: work must be 16-byte aligned");
    DGE_CHECK(work_bytes >= need, "gram: the workspace holds %lld bytes, %d needed", work_bytes, need);
    const int T = (D + kTile - 1) / kTile, ntiles = gram_tiles(D);
    const long long nch = gram_chunks(N);
    float* part = (float*)work;
    float* norm = part + (size_t)nch * ntiles * (kTile * kTile);
    if (row_norm) hipLaunchKernelGGL(gram_rownorm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, x, N, D, ldx, norm);
    hipLaunchKernelGGL(gram_partial_kernel, dim3(ntiles, (unsigned)nch), dim3(256), 0, s, x, mean, row_norm ? norm : nullptr, N, D, ldx, T,
                       part);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3(ntiles), dim3(256), 0, s, part, (int)nch, ntiles, D, T, scale, out);
    DGE_LAUNCH_CHECK("gram");
    dge_note_kernel("gram");
    return 0;
}

extern "C" int dge_eigh_sym_work_bytes(int D) {
    DGE_CHECK(D >= 1 && D <= 1024, "eigh_sym: 1 <= D <= 1024, got %d", D);
    return (int)(8LL * (4LL * D * D + 2LL * D + 2));
}

extern "C" int dge_eigh_sym(const float* a, int D, float* evals, float* evecs, double* host_status, void* work, long long work_bytes,
                            int max_sweeps, hipStream_t s) {
    const int need = dge_eigh_sym_work_bytes(D);
    if (need < 0) return -1;
    DGE_CHECK(a && evals && evecs && host_status && work, "eigh_sym: null argument");
    DGE_CHECK(max_sweeps >= 1 && max_sweeps <= 1000, "eigh_sym: 1 <= max_sweeps <= 1000, got %d", max_sweeps);
    DGE_CHECK((((uintptr_t)work) & 7) == 0, "eigh_sym: work must be 8-byte aligned");
    DGE_CHECK(work_bytes >= need, "eigh_sym: the workspace holds %lld bytes, %d needed", work_bytes, need);
    const size_t dd = (size_t)D * D;
    double* A[2] = {(double*)work, (double*)work + dd};
    double* V[2] = {(double*)work + 2 * dd, (double*)work + 3 * dd};
    double* rowsum = (double*)work + 4 * dd;
    double* stat = rowsum + 2 * (size_t)D;
    const int n = D + (D & 1);
    const dim3 rgrid((D + kJC - 1) / kJC, (D + kJR - 1) / kJR);
    int cur = 0, sweeps = 0;
    double off = 0., fro = 0.;
    // the one host read of a sweep: off(A) of the current copy
    auto read_off = [&]() -> int {
        double h[2] = {0., 0.};
        hipLaunchKernelGGL(jacobi_off_rows_kernel, dim3(D), dim3(256), 0, s, A[cur], D, rowsum);
        hipLaunchKernelGGL(jacobi_off_total_kernel, dim3(1), dim3(256), 0, s, rowsum, D, stat);
        DGE_LAUNCH_CHECK("eigh_sym");
        hipError_t e = hipMemcpyAsync(h, stat, sizeof(h), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { dge_set_error("eigh_sym: reading the convergence test failed: %s", hipGetErrorString(e)); return -3; }
        off = sqrt(2. * h[0]);
        fro = sqrt(h[1] + 2. * h[0]);
        return 0;
    };
    hipLaunchKernelGGL(jacobi_init_kernel, dim3((unsigned)((dd + 255) / 256)), dim3(256), 0, s, a, D, A[0], V[0]);
    int rc = read_off();
    if (rc) return rc;
    const double bound = kJacobiTol * fro;          // |A|_F does not change under the rotations
    bool done = off <= bound;
    while (!done && sweeps < max_sweeps) {
        for (int r = 0; r < n - 1; r++) {
            hipLaunchKernelGGL(jacobi_round_kernel, rgrid, dim3(256), 0, s, A[cur], V[cur], A[cur ^ 1], V[cur ^ 1], D, n, r);
            cur ^= 1;
        }
        sweeps++;
        rc = read_off();
        if (rc) return rc;
        done = off <= bound;
    }
    hipLaunchKernelGGL(jacobi_finish_kernel, dim3(D), dim3(256), 0, s, A[cur], V[cur], D, evals, evecs);
    DGE_LAUNCH_CHECK("eigh_sym");
    dge_note_kernel("eigh_sym");
    host_status[0] = (double)sweeps;
    host_status[1] = off;
    if (!done) {
        dge_set_error("eigh_sym: not converged after %d sweeps: off(A) = %.3e, bound %.3e (the results hold the last iterate)", sweeps, off, bound);
        return -2;
    }
    return 0;
}
