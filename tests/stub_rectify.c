/*
 * stub_rectify.c -- TEST INFRASTRUCTURE ONLY (tests/test_rectify_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_rectify.hip: sgmd_remap, which csrc/sgm_host.c references weakly.  A host linked without this file
 * has no rectification.  It keeps a log of its own (the launch log of stub_device.c stays what it is without rectification): the
 * five pointers and the batch of every call, and it can be told to refuse the n-th call.  While the buffers fit the allocator's
 * cap of stub_device.c (1 MiB) it samples for real, so that a sanitizer build sees every map entry, tap and output byte the
 * product's kernel would touch.
 */
#include "sgm_device.h"

#include <string.h>

#define REMAP_LOG_MAX 256
static struct { const void* p[5]; int frames; } g_calls[REMAP_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_remap_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_remap_count(void) { return g_calls_n; }
/* which: 0 maps, 1 left, 2 right, 3 out_left, 4 out_right */
const void* stub_remap_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 5) ? g_calls[call].p[which] : NULL; }
int stub_remap_frames(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].frames : -1; }
/* the nth (0-based) call from now on returns an error */
void stub_remap_fail_at(int nth) { g_refuse_countdown = nth; }

static unsigned tap(const unsigned char* src, int W, int H, int y, int x)
{
    return (y >= 0 && y < H && x >= 0 && x < W) ? src[(size_t)y * W + x] : 0u;
}

int sgmd_remap(int o, void* st, const sgmd_geom* g, const void* maps, const void* left, const void* right, void* out_left, void* out_right)
{
    (void)o; (void)st;
    if (g_calls_n < REMAP_LOG_MAX) {
        const void* p[5] = {maps, left, right, out_left, out_right};
        memcpy(g_calls[g_calls_n].p, p, sizeof p);
        g_calls[g_calls_n++].frames = g->B;
    }
    if (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) return 719;
    const size_t n = (size_t)g->W * g->H, pitch = SGMD_REMAP_PITCH(n);
    if (4 * pitch * sizeof(int32_t) > (1u << 20) || n * (size_t)g->B > (1u << 20)) return 0;
    for (int view = 0; view < 2; ++view) {
        const int32_t* xq = (const int32_t*)maps + (size_t)view * 2 * pitch;
        const int32_t* yq = xq + pitch;
        for (int f = 0; f < g->B; ++f) {
            const unsigned char* src = (const unsigned char*)(view ? right : left) + (size_t)f * n;
            unsigned char* dst = (unsigned char*)(view ? out_right : out_left) + (size_t)f * n;
            for (size_t p = 0; p < n; ++p) {
                const int x0 = xq[p] >> 5, y0 = yq[p] >> 5;
                const unsigned ax = (unsigned)xq[p] & 31u, ay = (unsigned)yq[p] & 31u;
                dst[p] = (unsigned char)(((32 - ax) * (32 - ay) * tap(src, g->W, g->H, y0, x0) + ax * (32 - ay) * tap(src, g->W, g->H, y0, x0 + 1) +
                                          (32 - ax) * ay * tap(src, g->W, g->H, y0 + 1, x0) + ax * ay * tap(src, g->W, g->H, y0 + 1, x0 + 1) + 512) >> 10);
            }
        }
    }
    return 0;
}
