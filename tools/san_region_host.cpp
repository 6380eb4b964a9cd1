// Stand-alone host check of the argument refusals of csrc/region_kernels.hip: every call below returns before a launch, so the
// program needs no device and runs under the host sanitizers on a CPU-only machine.  It supplies the error plumbing of capi.hip
// itself and links nothing else of the library:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         deep-gan-encoders_amd/csrc/region_kernels.hip tools/san_region_host.cpp -o /tmp/san_region && /tmp/san_region
#include <cstdio>
#include <cstdarg>
#include <cstdint>
#include <cstring>
#include "../include/dge_hip.h"
struct DgeDet;
static char g_err[512];
void dge_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
void dge_note_kernel(const char*, ...) {}
void dge_det_register(void (*)(const DgeDet*)) {}
int dge_det_upload_failed = 0;
#define EXPECT(e) do { if (!(e)) { printf("FAILED: %s\n", #e); return 1; } } while (0)
int main() {
    alignas(16) static float buf[64];
    float* p = buf;
    EXPECT(dge_gram_cols_chunk(0) == -1 && dge_gram_cols_chunk(1LL << 31) == -1 && dge_gram_cols_chunk(1) == 4096);
    EXPECT(dge_gram_cols_chunk(1 << 20) == 4096 && dge_gram_cols_chunk((1 << 20) + 1) == 4128 && dge_gram_cols_chunk(3LL << 20) == 12288);
    EXPECT(dge_gram_cols_chunk((1LL << 31) - 1) == 8388608);
    EXPECT(dge_gram_cols_work_bytes(0, 8) == -1 && dge_gram_cols_work_bytes(1025, 8) == -1 && dge_gram_cols_work_bytes(4, 0) == -1);
    EXPECT(dge_gram_cols_work_bytes(1024, (1LL << 31) - 1) == 2LL * 4 * 256 * 136 * 4096);
    long long nb = dge_gram_cols_work_bytes(4, 8);
    EXPECT(nb == 2 * 4 * 4096);
    EXPECT(dge_gram_cols(p, 4, 8, 7, p, 4, 1.f, p, p, p, nb, nullptr) == -1 && strstr(g_err, "row stride"));
    EXPECT(dge_gram_cols(p, 4, 8, 8, p, 3, 1.f, p, p, p, nb, nullptr) == -1 && strstr(g_err, "must divide"));
    EXPECT(dge_gram_cols(p, 4, 8, 8, p, 0, 1.f, p, p, p, nb, nullptr) == -1);
    EXPECT(dge_gram_cols(p, 4, 8, 8, nullptr, 4, 1.f, p, p, p, nb, nullptr) == -1 && strstr(g_err, "out_b"));
    EXPECT(dge_gram_cols(p, 4, 8, 8, p, 4, 1.f, p, p, p, nb - 4, nullptr) == -1 && strstr(g_err, "workspace"));
    EXPECT(dge_gram_cols(p, 4, 8, 8, p, 4, 1.f, p, p, p + 1, nb, nullptr) == -1 && strstr(g_err, "aligned"));
    EXPECT(dge_gram_cols(nullptr, 4, 8, 8, p, 4, 1.f, p, p, p, nb, nullptr) == -1);
    EXPECT(dge_fd_pool_diff(p, 1, 3, 8, 8, 3, 1.f, p, 48, nullptr) == -1 && strstr(g_err, "window"));
    EXPECT(dge_fd_pool_diff(p, 1, 3, 8, 8, 0, 1.f, p, 48, nullptr) == -1);
    EXPECT(dge_fd_pool_diff(p, 1, 3, 8, 8, 2, 1.f, p, 47, nullptr) == -1 && strstr(g_err, "row stride"));
    EXPECT(dge_fd_pool_diff(p, 0, 3, 8, 8, 2, 1.f, p, 48, nullptr) == -1);
    EXPECT(dge_wp_axis_pairs(p, p, 8, 1, 2, 8, -1, 1, .1f, p, nullptr) == -1 && strstr(g_err, "outside"));
    EXPECT(dge_wp_axis_pairs(p, p, 8, 1, 2, 8, 0, 3, .1f, p, nullptr) == -1);
    EXPECT(dge_wp_axis_pairs(p, p, 8, 1, 2, 8, 2, 1, .1f, p, nullptr) == -1);
    EXPECT(dge_wp_axis_pairs(p, p, 7, 1, 2, 8, 0, 1, .1f, p, nullptr) == -1);
    EXPECT(dge_matmul_f64acc(p, 4, p, 4, 0, p, 4, 1025, 4, 4, nullptr) == -1);
    EXPECT(dge_matmul_f64acc(p, 3, p, 4, 0, p, 4, 4, 4, 4, nullptr) == -1 && strstr(g_err, "leading"));
    EXPECT(dge_matmul_f64acc(p, 4, p, 3, 1, p, 4, 4, 2, 4, nullptr) == -1);
    EXPECT(dge_matmul_f64acc(nullptr, 4, p, 4, 0, p, 4, 4, 4, 4, nullptr) == -1);
    printf("host refusals OK\n");
    return 0;
}
