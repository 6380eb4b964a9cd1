// Streaming data gradient of the StyleGAN2 up layer at the narrow top of the generator (64 <- 32 channels, 1024^2 -> 512^2; bf16),
// gfx950: the adjoint of upconv_stream.hip, built from that kernel's parts.
// Reference math: model/stylegan2_generator.py:879-896 (conv_transpose2d stride 2 + 4x4 FIR) differentiated, and :908-921 (noise,
// bias, lrelu * sqrt 2 of the layer below) for the fused tail backward.  CPU definitions: oracle/conv_ref.py up_dgrad,
// oracle/elem_ref.py modconv_tail_bwd.
//
// The forward evaluates t = conv_transpose2d(x, w) on the (2H+1)^2 grid, then the separable [1,3,3,1]/4 FIR to 2H x 2W.  Backwards:
//   g_t = FIR^T g_z            (a zero-padded "full" correlation with the same symmetric filter, on the VALU)
//   g_x[m, n, ci] = sum_{ky, kx, co} w[co, ci, 2 - ky, 2 - kx] * g_t[2m + ky, 2n + kx, co]      (9 taps x 32 channels on the MFMAs)
// i.e. 9 tap-MACs per input pixel where the folded space-to-depth form (conv_igemm mode 33) spends 36, and one pass over memory:
// g_z (fine grid) in, the stored activation of the layer below (dot_src) and the toRGB addend in, g_x - or, with `prep`, g_z of the
// layer below - out.
//   * a 2-wave team owns a strip of 32 input-pixel columns and marches down the image one INPUT row per step; the two fine-grid rows
//     of g_z a step needs (68 fine columns = 34 x 128 B: exactly the ring row of upconv_stream) arrive by LDS-DMA through one-row
//     buffer descriptors (zero padding = out-of-range lanes), as do this wave's halves of the dot_src / addend rows and the noise row;
//   * FIR^T: lane (16-byte channel chunk, column pair) runs the horizontal filter on the two new rows and the vertical filter on a
//     three-row register history (f32), rounds g_t to bf16 ONCE and writes the two new t rows to a 4-row LDS ring whose even and odd
//     t columns are separate planes, so that the three column taps of the GEMM read 32 consecutive 64-byte pixels each;
//   * GEMM per wave: M = its 32 input channels, N = 32 pixels, K = 9 taps x 32 = 18 MFMAs 32x32x16, the weights resident in
//     registers (72 VGPRs; the demodulation factor d[b, co] multiplies g_t in f32 before its rounding);
//   * the M rows are permuted (conv_stream's chan_of_row) so that a lane stores two 16-byte runs of consecutive channels.
#include <type_traits>
#include <stdlib.h>
#include "common.h"
#include "../../include/dge_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned rsrc_t;
typedef __attribute__((ext_vector_type(2))) float f2_t;

__device__ __forceinline__ unsigned rfl(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned lds_off(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)p;
}
__device__ __forceinline__ rsrc_t make_rsrc(unsigned long long base, unsigned bytes) {
    rsrc_t r;
    r[0] = rfl((unsigned)base); r[1] = rfl((unsigned)(base >> 32) & 0xffffu); r[2] = rfl(bytes); r[3] = 0x00020000u;
    return r;
}

struct UpbParams {
    const void* gz; const void* w; void* y; const void* addend; const void* dot_src;
    const float* d_in; const float* out_scale;
    float* stats; float* prep_stats; int stats_slots;
    const float* prep_noise; const float* prep_ns; int prep_noise_bstride; float prep_gain;
    int B, H, W;
    int nstrips, nseg, seg_rows, njobs, jobs_per_xcd;
    int dbg;                  // ablation switches for tuning (DGE_UP_DBG: 1 no stores, 2 no MFMAs, 8 no FIR^T), 0 in production
};

constexpr int CIN = 64, COUT = 32;                // of the FORWARD layer: the launch maps 32 gradient channels to 64
constexpr int ZRB = 34 * 128;                     // one g_z ring row: 68 fine pixels x 64 B = 4 full 1 KB pieces + 16 lanes
constexpr int NS = 3, D = 2;                      // ring slots (steps), steps in flight ahead of the live one
constexpr int ZPAIR = 2 * ZRB;                    // a step consumes two fine rows
constexpr int Z_OFF = 0;
constexpr int T_OFF = (NS * ZPAIR + 255) / 256 * 256;
constexpr int T_ODD = 34 * 64;                    // t row: even columns (33 pixels x 64 B), then odd columns (32 pixels)
constexpr int TRB = T_ODD + 32 * 64, NT = 4;
constexpr int D_OFF = T_OFF + NT * TRB;           // per wave: dot_src ring, NS rows of 32 pixels x 32 channels
constexpr int DROWB = 2048, DRING = NS * DROWB;
constexpr int A_OFF = D_OFF + 2 * DRING;          // per wave: addend ring, same shape
constexpr int N_OFF = A_OFF + 2 * DRING;          // per wave: noise ring, NS rows of 64 f32 (32 used)
constexpr int NRING = NS * 256;
constexpr int DUMMY_OFF = (N_OFF + 2 * NRING + 255) / 256 * 256;
constexpr int LDS_BYTES = DUMMY_OFF + 1024;
constexpr int LPR = 6 + 2 + 2 + 1;                // loads per wave and step: 2 x 3 g_z pieces, 2 dot, 2 addend, 1 noise
static_assert((D - 1) * LPR < 64, "vmcnt range");

__device__ __forceinline__ int swz8(int px) { return (px >> 1) & 7; }     // g_z ring: 8 chunks per 128-byte pixel pair (upconv_stream)
__device__ __forceinline__ int swz4(int px) { return (px >> 2) & 3; }     // 64-byte pixels: conflict-free ds_read_b128 of 16 consecutive ones

#define UPB_P(off) "buffer_load_dwordx4 %1, %3, 0 offen offset:" #off " lds\n\t"
#define UPB_M0 "s_mov_b32 m0, %2\n\ts_nop 0\n\t"
// one g_z ring row (upconv_stream's dma_row): pieces 0, 2, 4 by wave 0 (piece 4 = the last 16 lanes' worth, under an EXEC mask),
// pieces 1, 3 + a zero-length piece by wave 1 (both waves count 3 loads per row)
__device__ __forceinline__ void dma_row(int wave, unsigned voff, unsigned voff_b, unsigned voff_c, rsrc_t rs, rsrc_t rs_null,
                                        unsigned m0v, unsigned m0_dummy) {
    unsigned long long keep;
    if (wave == 0)
        asm volatile(UPB_M0 UPB_P(0) UPB_P(2048)
                     "s_mov_b32 m0, %5\n\ts_mov_b64 %0, exec\n\ts_mov_b64 exec, 0xffff\n\tbuffer_load_dwordx4 %4, %3, 0 offen lds\n\ts_mov_b64 exec, %0"
                     : "=&s"(keep) : "v"(voff), "s"(m0v), "s"(rs), "v"(voff_c), "s"(m0v + 4096u) : "memory");
    else
        asm volatile(UPB_M0 UPB_P(1024) UPB_P(3072) "s_mov_b32 m0, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %4, 0 offen lds"
                     : "=&s"(keep) : "v"(voff_b), "s"(m0v), "s"(rs), "s"(rs_null), "s"(m0_dummy) : "memory");
}
// a 2 KB row of 32 pixels x 64 B: two pieces of 16 pixels (the source advances 2048 B per piece, the ring 1024 B)
__device__ __forceinline__ void dma_half(unsigned voff, unsigned voff1, rsrc_t rs, unsigned m0v) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds\n\t"
                 "buffer_load_dwordx4 %3, %2, 0 offen offset:1024 lds" : : "v"(voff), "s"(m0v), "s"(rs), "v"(voff1) : "memory");
}
__device__ __forceinline__ void dma_f32(unsigned voff, rsrc_t rs, unsigned m0v) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dword %0, %2, 0 offen lds" : : "v"(voff), "s"(m0v), "s"(rs) : "memory");
}

// channel of row m of the permuted M tile (conv_stream.hip): the accumulator of lane (pixel, kh) holds channels 8 kh .. 8 kh + 7
// in registers 0-7 and 16 + 8 kh .. in registers 8-15
__device__ __forceinline__ int chan_of_row(int m) {
    const int j = m >> 3, k = (m >> 2) & 1, i = m & 3;
    return 16 * (j >> 1) + 8 * k + 4 * (j & 1) + i;
}
__device__ __forceinline__ int chan_of_reg(int kh, int r) { return (r < 8 ? 8 * kh + r : 16 + 8 * kh + (r - 8)); }

template <bool PREP>
__global__ __launch_bounds__(128, 1) void upconv_stream_bwd_kernel(UpbParams p) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = (int)rfl(threadIdx.x >> 6);
    const unsigned lds0 = lds_off(lds);
    const int n31 = lane & 31, kh = lane >> 5;

    // ---- job: the teams of one XCD take a contiguous range of (sample, segment, strip)
    int job = (blockIdx.x & 7) * p.jobs_per_xcd + (blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= p.jobs_per_xcd || job >= p.njobs) return;
    const int strip = job % p.nstrips; job /= p.nstrips;
    const int seg = job % p.nseg;
    const int b = job / p.nseg;
    const int r0 = seg * p.seg_rows;                                   // input rows [r0, r1)
    const int r1 = min(r0 + p.seg_rows, p.H);
    const int nsteps = r1 - r0 + 2;                                    // step t: input row m = r0 - 2 + t (two warm-up steps fill the FIR history)
    const int x0 = 32 * strip;
    const int FH = 2 * p.H;

    const unsigned zrow_bytes = (unsigned)(2 * p.W) * (COUT * 2);
    const unsigned yrow_bytes = (unsigned)p.W * (CIN * 2);
    const unsigned long long Zb = (unsigned long long)p.gz + (unsigned long long)b * FH * zrow_bytes;
    const unsigned long long DOTb = (unsigned long long)p.dot_src + (unsigned long long)b * p.H * yrow_bytes;
    const unsigned long long ADDb = p.addend ? (unsigned long long)p.addend + (unsigned long long)b * p.H * yrow_bytes : Zb;
    const bool has_nz = PREP && p.prep_noise != nullptr;
    const unsigned long long NZb = has_nz ? (unsigned long long)(p.prep_noise + (size_t)b * p.prep_noise_bstride) : Zb;
    const unsigned nzrow_bytes = (unsigned)p.W * 4;

    // ---- DMA lane offsets.  g_z row: 16-byte unit = (pixel pair, chunk), source chunk swizzled; pair 0 = fine columns 2 x0 - 2, - 1
    unsigned voff, voff_b, voff_c;
    {
        const int px = lane >> 3, cs = lane & 7;
        const int gx = x0 - 1 + px;
        voff = (unsigned)(gx * 128 + ((cs ^ swz8(px)) << 4));                   // negative / beyond the row = out of range = zeros
        voff_b = (unsigned)(gx * 128 + ((cs ^ swz8(px + 8)) << 4));
        voff_c = voff + 4096;
    }
    // dot_src / addend row: this wave's 32 channels (4 chunks) of 16 pixels per piece
    unsigned dvoff, dvoff1;
    {
        const int px = lane >> 2, cs = lane & 3;
        dvoff = (unsigned)((x0 + px) * 128 + wave * 64 + ((cs ^ swz4(px)) << 4));
        dvoff1 = dvoff + 2048u - 1024u;
    }
    const unsigned nvoff = lane < 32 ? (unsigned)((x0 + lane) * 4) : 0x80000000u;
    const rsrc_t rs_null = make_rsrc(Zb, 0);

    // step tt: fine rows 2 (r0 - 1 + tt) and + 1 into ring slot `slot`; dot / addend / noise row r0 - 2 + tt (none for the warm-up steps)
    auto issue = [&](int tt, int slot) {
        const int gy = 2 * (r0 - 1 + tt);
        const bool live = tt < nsteps;
        const bool zv = live && gy >= 0 && gy < FH;                    // (both rows of the pair are inside the image, or neither)
        const unsigned long long zp = Zb + (unsigned long long)(zv ? gy : 0) * zrow_bytes;
        const unsigned m0z = lds0 + Z_OFF + (unsigned)slot * ZPAIR;
        dma_row(wave, voff, voff_b, voff_c, make_rsrc(zp, zv ? zrow_bytes : 0u), rs_null, m0z, lds0 + DUMMY_OFF);
        dma_row(wave, voff, voff_b, voff_c, make_rsrc(zp + zrow_bytes, zv ? zrow_bytes : 0u), rs_null, m0z + ZRB, lds0 + DUMMY_OFF);
        const bool ov = live && tt >= 2;
        const unsigned long long ro = (unsigned long long)(ov ? r0 - 2 + tt : 0);
        dma_half(dvoff, dvoff1, make_rsrc(DOTb + ro * yrow_bytes, ov ? yrow_bytes : 0u), lds0 + D_OFF + (unsigned)(wave * DRING + slot * DROWB));
        dma_half(dvoff, dvoff1, make_rsrc(ADDb + ro * yrow_bytes, (ov && p.addend) ? yrow_bytes : 0u), lds0 + A_OFF + (unsigned)(wave * DRING + slot * DROWB));
        dma_f32(nvoff, make_rsrc(NZb + ro * nzrow_bytes, (ov && has_nz) ? nzrow_bytes : 0u), lds0 + N_OFF + (unsigned)(wave * NRING + slot * 256));
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int h = 0; h < D; h++) issue(h, h);                           // steps 0 .. D - 1 start before the weights are touched

    // ---- weights -> registers: A[tap][ks] of row r = n31: w[tap][ci][co], co = 16 ks + 8 kh + e (the demodulation factor stays out of
    // them: it multiplies g_t in f32 before its one rounding, so that the weights are the shared bf16 copy, exact)
    uint4 wf[9][2];
    {
        const bf16_t* __restrict__ Wp = (const bf16_t*)p.w;
        const int ci = wave * 32 + chan_of_row(n31);
#pragma unroll
        for (int tap = 0; tap < 9; tap++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++) wf[tap][ks] = *(const uint4*)(Wp + ((size_t)(tap * CIN + ci) * COUT + ks * 16 + kh * 8));
    }
    // epilogue constants of this lane's 16 channels
    float oscv[16];
#pragma unroll
    for (int r = 0; r < 16; r++) oscv[r] = p.out_scale ? p.out_scale[b * CIN + wave * 32 + chan_of_reg(kh, r)] : 1.f;
    const float pg_pos = p.prep_gain, pg_neg = 0.2f * p.prep_gain, pz_pos = 1.f / p.prep_gain, pz_neg = 1.f / (0.2f * p.prep_gain);
    const float pns = (has_nz && p.prep_ns) ? p.prep_ns[0] : 0.f;

    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(3))) u32x4_t* lds_u4p;
    typedef __attribute__((address_space(3))) u32x4_t* lds_u4wp;
    typedef const __attribute__((address_space(3))) float* lds_fp;
    auto lds_u4 = [&](unsigned a) { const u32x4_t t = *(lds_u4p)(size_t)a; return make_uint4(t[0], t[1], t[2], t[3]); };
    auto lds_st4 = [&](unsigned a, unsigned v0, unsigned v1, unsigned v2, unsigned v3) { u32x4_t t; t[0] = v0; t[1] = v1; t[2] = v2; t[3] = v3; *(lds_u4wp)(size_t)a = t; };

    // ---- FIR^T lane = (chunk c of 8 channels, column pair j): t columns X0 = 32 wave + 2 j, X0 + 1 and X0 + 2 of the strip's 65; the
    // third one repeats the neighbour lane's first except in the last lane pair of wave 1 (column 64), the only one that writes it.
    // t column X reads fine ring pixels X .. X + 3 (ring pixel 0 = fine column 2 x0 - 2).
    const int fc = lane & 3, fj = lane >> 2;
    unsigned zoff[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int sp = 16 * wave + fj + (k >> 1);                      // pixel pair of ring pixel X0 + k
        zoff[k] = lds0 + Z_OFF + (unsigned)(sp * 128 + ((((k & 1) * 4 + fc) ^ swz8(sp)) << 4));
    }
    const int tj = 16 * wave + fj;                                     // plane position of columns X0 (even plane) and X0 + 1 (odd plane)
    const unsigned toff_e = lds0 + T_OFF + (unsigned)(tj * 64 + ((fc ^ swz4(tj)) << 4));
    const unsigned toff_o = toff_e + T_ODD;
    const unsigned toff_x = lds0 + T_OFF + (unsigned)((tj + 1) * 64 + ((fc ^ swz4(tj + 1)) << 4));
    const bool wr_x = tj == 31;
    f2_t dsc[4];                                                       // demodulation factor of this lane's 8 gradient channels
#pragma unroll
    for (int i = 0; i < 4; i++) dsc[i] = p.d_in ? f2_t{p.d_in[b * COUT + 8 * fc + 2 * i], p.d_in[b * COUT + 8 * fc + 2 * i + 1]} : f2_t{1.f, 1.f};
    f2_t hist[3][3][4];                                                // horizontally filtered fine rows 2m - 1, 2m, 2m + 1: [row][column][channel pair]
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) hist[r][c][i] = f2_t{0.f, 0.f};

    // ---- B-fragment lane offsets: tap column kx reads plane kx & 1 at position n31 + (kx >> 1), chunk 2 ks + kh
    unsigned boff[3][2];
#pragma unroll
    for (int kx = 0; kx < 3; kx++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const int jj = n31 + (kx >> 1);
            boff[kx][ks] = lds0 + T_OFF + (unsigned)((kx & 1) * T_ODD + jj * 64 + (((2 * ks + kh) ^ swz4(jj)) << 4));
        }
    // epilogue: chunks kh and 2 + kh of pixel n31 of this wave's dot / addend rows
    unsigned eoff[2];
#pragma unroll
    for (int q = 0; q < 2; q++) eoff[q] = (unsigned)(wave * DRING + n31 * 64 + (((2 * q + kh) ^ swz4(n31)) << 4));
    const unsigned nzoff = lds0 + N_OFF + (unsigned)(wave * NRING + n31 * 4);

    const bool pv = x0 + n31 < p.W;
    const bool stv = pv && !(p.dbg & 1);
    unsigned char* __restrict__ Yb = (unsigned char*)p.y + (size_t)b * p.H * yrow_bytes + (size_t)(x0 + n31) * (CIN * 2) + wave * 64 + kh * 16;
    float s0[16], s1[16], s2[PREP ? 16 : 1];
#pragma unroll
    for (int r = 0; r < 16; r++) { s0[r] = 0.f; s1[r] = 0.f; if (PREP) s2[r] = 0.f; }
    f32x16_t zero16;
#pragma unroll
    for (int r = 0; r < 16; r++) zero16[r] = 0.f;

    int slot = 0, slot_pf = D % NS;
    for (int t = 0; t < nsteps; t++) {
        // the rows of step t have landed when at most the loads of the D - 1 later steps are still in flight (stores count in vmcnt
        // too and only make this wait conservative)
        asm volatile("s_waitcnt vmcnt(%0)" :: "i"((D - 1) * LPR) : "memory");
        __builtin_amdgcn_s_barrier();                                  // the partner's pieces landed; it finished step t - 1 (t ring reads included)
        issue(t + D, slot_pf);

        // ---- FIR^T: fine rows 2m + 2, 2m + 3 -> horizontal -> with the history: t rows 2m + 1, 2m + 2
        if (!(p.dbg & 8)) {
            f2_t hn[2][3][4];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                f2_t g[6][4];
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const uint4 v = lds_u4(zoff[k] + (unsigned)(slot * ZPAIR + r * ZRB));
                    const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) g[k][i] = f2_t{__uint_as_float(w4[i] << 16), __uint_as_float(w4[i] & 0xffff0000u)};
                }
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int i = 0; i < 4; i++) hn[r][c][i] = (g[c][i] + g[c + 3][i]) * 0.25f + (g[c + 1][i] + g[c + 2][i]) * 0.75f;
            }
            const unsigned ta = (unsigned)(((2 * t + 1) & (NT - 1)) * TRB), tb = (unsigned)(((2 * t + 2) & (NT - 1)) * TRB);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                unsigned oa[4], ob[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const f2_t va = ((hist[0][c][i] + hn[0][c][i]) * 0.25f + (hist[1][c][i] + hist[2][c][i]) * 0.75f) * dsc[i];
                    const f2_t vb = ((hist[1][c][i] + hn[1][c][i]) * 0.25f + (hist[2][c][i] + hn[0][c][i]) * 0.75f) * dsc[i];
                    oa[i] = pack2bf(va[0], va[1]); ob[i] = pack2bf(vb[0], vb[1]);
                    hist[0][c][i] = hist[2][c][i]; hist[1][c][i] = hn[0][c][i]; hist[2][c][i] = hn[1][c][i];
                }
                const unsigned o = c == 0 ? toff_e : (c == 1 ? toff_o : toff_x);
                if (c < 2 || wr_x) { lds_st4(o + ta, oa[0], oa[1], oa[2], oa[3]); lds_st4(o + tb, ob[0], ob[1], ob[2], ob[3]); }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                  // both halves of the two new t rows are in the ring

        if (t >= 2) {
            // ---- GEMM: taps (ky, kx) x 2 K slices in consumption order, PF fragments requested ahead of their MFMAs
            constexpr int NQ = 18, PF = 6;
            unsigned rowb[3];
#pragma unroll
            for (int ky = 0; ky < 3; ky++) rowb[ky] = (unsigned)(((2 * t + ky) & (NT - 1)) * TRB);
            f32x16_t acc = zero16;
            if (!(p.dbg & 2)) {
                uint4 bq[PF];
                StaticFor<PF>::run([&](auto qc) { constexpr int q = decltype(qc)::value; bq[q] = lds_u4(boff[(q >> 1) % 3][q & 1] + rowb[(q >> 1) / 3]); });
                StaticFor<NQ>::run([&](auto qc) {
                    constexpr int q = decltype(qc)::value;
                    constexpr int tap = q >> 1, ks = q & 1;
                    const bf16x8_t bf = *(const bf16x8_t*)&bq[q % PF];
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8_t*)&wf[tap][ks], bf, acc, 0, 0, 0);
                    if constexpr (q + PF < NQ) { constexpr int q2 = q + PF; bq[q % PF] = lds_u4(boff[(q2 >> 1) % 3][q2 & 1] + rowb[(q2 >> 1) / 3]); }
                });
            }
            // ---- epilogue: this lane = pixel x0 + n31, channels chan_of_reg(kh, 0 .. 15) of this wave's 32
            const unsigned so = (unsigned)(slot * DROWB);
            uint4 dd[2], aa[2];
#pragma unroll
            for (int q = 0; q < 2; q++) { dd[q] = lds_u4(lds0 + D_OFF + eoff[q] + so); aa[q] = lds_u4(lds0 + A_OFF + eoff[q] + so); }
            float nzs = 0.f;
            if (PREP) nzs = pns * *(lds_fp)(size_t)(nzoff + (unsigned)(slot * 256));
            float v[16];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                float dv[8], av[8];
                unpack16(dd[q], dv, (bf16_t*)nullptr);
                unpack16(aa[q], av, (bf16_t*)nullptr);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int r = 8 * q + e;
                    const float a = acc[r];
                    s0[r] = fmaf(a, dv[e], s0[r]);
                    const float g = fmaf(a, oscv[r], av[e]);
                    if (PREP) {
                        // x = lrelu(z) * gain of the layer below -> g_z = g * gain * lrelu'(x), z = x / (gain * lrelu'(x))
                        const bool pos = dv[e] > 0.f;
                        const float gz = g * (pos ? pg_pos : pg_neg);
                        const float zt = dv[e] * (pos ? pz_pos : pz_neg) - nzs;
                        s2[PREP ? r : 0] = fmaf(gz, zt, s2[PREP ? r : 0]); s1[r] += gz;
                        v[r] = gz;
                    } else {
                        s1[r] += a;
                        v[r] = g;
                    }
                }
            }
            if (stv) {
                unsigned char* dst = Yb + (size_t)(r0 - 2 + t) * yrow_bytes;
                *(uint4*)dst = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
                *(uint4*)(dst + 32) = make_uint4(pack2bf(v[8], v[9]), pack2bf(v[10], v[11]), pack2bf(v[12], v[13]), pack2bf(v[14], v[15]));
            }
        }
        slot = slot + 1 == NS ? 0 : slot + 1;
        slot_pf = slot_pf + 1 == NS ? 0 : slot_pf + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // no DMA may land after the wave has given its LDS back

    // ---- statistics: reduce over the 32 pixel lanes; lane n31 = r keeps the totals of register r, so that one atomic instruction
    // carries all 16 channels (conv_stream.hip).  Lanes right of the image accumulated pixels that do not exist: dropped here.
    if (p.stats) {
        float* __restrict__ ST = p.stats + ((size_t)(blockIdx.x % p.stats_slots) * p.B + b) * CIN * 2;
        float* __restrict__ PST = (PREP && p.prep_stats) ? p.prep_stats + ((size_t)(blockIdx.x % p.stats_slots) * p.B + b) * CIN * 2 : nullptr;
        float va = 0.f, vc = 0.f, vt = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            float a = pv ? s0[r] : 0.f, c = pv ? s1[r] : 0.f, t2 = (PREP && pv) ? s2[PREP ? r : 0] : 0.f;
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) {
                a += __shfl_xor(a, m, 64); c += __shfl_xor(c, m, 64);
                if (PREP) t2 += __shfl_xor(t2, m, 64);
            }
            if (n31 == r) { va = a; vc = c; vt = t2; }
        }
        if (n31 < 16) {
            const int ch = wave * 32 + chan_of_reg(kh, n31);
            atomicAdd(ST + ch * 2, va);
            if (PREP) { if (PST) { atomicAdd(PST + ch * 2, vt); atomicAdd(PST + ch * 2 + 1, vc); } }
            else atomicAdd(ST + ch * 2 + 1, vc);
        }
    }
}

template <bool PREP>
int launch(UpbParams& p, hipStream_t s) {
    auto kern = upconv_stream_bwd_kernel<PREP>;
    static int caps[16] = {0};                                   // resident teams, per device (the attribute is per device too)
    int dev = 0;
    (void)hipGetDevice(&dev);
    int& cap = caps[dev >= 0 && dev < 16 ? dev : 0];
    if (!cap) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        int occ = 0, ncu = 256;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)kern, 128, LDS_BYTES) != hipSuccess || occ < 1) occ = 1;
        cap = occ * ncu;
    }
    p.nstrips = (p.W + 31) / 32;
    int nseg = cap / (p.B * p.nstrips);
    int maxseg = p.H / 16; if (maxseg < 1) maxseg = 1;
    if (nseg > maxseg) nseg = maxseg;
    if (nseg < 1) nseg = 1;
    p.seg_rows = (p.H + nseg - 1) / nseg;
    p.nseg = (p.H + p.seg_rows - 1) / p.seg_rows;
    p.njobs = p.B * p.nstrips * p.nseg;
    p.jobs_per_xcd = (p.njobs + 7) / 8;
    dge_note_kernel(PREP ? "upconv_stream_bwd<bf16,%d,%d>+prep" : "upconv_stream_bwd<bf16,%d,%d>", CIN, COUT);
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.jobs_per_xcd * 8)), dim3(128), LDS_BYTES, s, p);
    DGE_LAUNCH_CHECK("upconv_stream_bwd");
    return 0;
}

}  // namespace

extern "C" int dge_up_dgrad_stream_supported(int B, int H, int W, int Cin, int Cout, int dtype) {
    if (dtype != DGE_BF16 || Cin != CIN || Cout != COUT || B < 1 || H < 1 || W < 1) return 0;
    if ((long)W * 128 >= (1L << 31) || (long)B * H * W * 128 >= (1L << 40)) return 0;
    return 1;
}

extern "C" int dge_up_dgrad_stream(const void* g_z, const void* w_packed, void* y, const float* d_in, const float* out_scale,
                                   const void* addend, const void* dot_src, float* stats, int stats_slots, int prep, float prep_gain,
                                   const float* prep_noise, int prep_noise_bstride, const float* prep_ns, float* prep_stats,
                                   int B, int H, int W, int Cin, int Cout, int dtype, hipStream_t s) {
    DGE_CHECK(dge_up_dgrad_stream_supported(B, H, W, Cin, Cout, dtype), "up_dgrad_stream: bf16, %d -> %d channels only (got %d -> %d)", CIN, COUT, Cin, Cout);
    DGE_CHECK(dot_src && stats && stats_slots >= 1, "up_dgrad_stream: needs dot_src and stats");
    DGE_CHECK(!prep || (prep_stats && prep_gain > 0.f), "up_dgrad_stream: prep needs its stats and a positive gain");
    UpbParams p;
    p.gz = g_z; p.w = w_packed; p.y = y; p.addend = addend; p.dot_src = dot_src; p.d_in = d_in; p.out_scale = out_scale;
    p.stats = stats; p.prep_stats = prep ? prep_stats : nullptr; p.stats_slots = stats_slots;
    p.prep_noise = prep ? prep_noise : nullptr; p.prep_ns = prep_ns; p.prep_noise_bstride = prep_noise_bstride; p.prep_gain = prep ? prep_gain : 1.f;
    p.B = B; p.H = H; p.W = W;
    p.dbg = dge_env().up_dbg;
    return prep ? launch<true>(p, s) : launch<false>(p, s);
}
