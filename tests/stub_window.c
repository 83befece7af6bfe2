/*
 * stub_window.c -- TEST INFRASTRUCTURE ONLY (tests/test_window_cpu.py builds it beside tests/stub_device.c and, for the driver,
 * the other volume stand-ins).
 *
 * The stand-in for the launcher of csrc/sgm_window.hip, sgmd_volume_window, which csrc/sgm_host.c references weakly: a host linked
 * without this file keeps the volume and refuses sgm_volume_window.  It keeps a log of its own -- the source volume, the offset,
 * the dims and the four pointers of every call -- and it can be told to refuse the n-th call.  While both volumes fit 1 MiB it
 * windows for real, the copy rule of include/sgm_mi355x.h in plain C, every destination word written exactly once, so that a
 * sanitizer build sees every word read and written and the tests can compare with the restatement.
 */
#include "sgm_device.h"

#include <string.h>

#define WIN_LOG_MAX 256
#define CAP ((size_t)1 << 20)
static struct {
    sgmd_volume v;
    int offset[3], dims[3];
    const void* p[4];
} g_calls[WIN_LOG_MAX];
static int g_calls_n, g_total, g_refuse_countdown = -1;             /* the log keeps the first WIN_LOG_MAX calls, the count all */

void stub_window_clear(void) { g_calls_n = g_total = 0; g_refuse_countdown = -1; }
int stub_window_count(void) { return g_total; }
/* which: 0 source voxels, 1 source colours, 2 destination voxels, 3 destination colours */
const void* stub_window_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 4) ? g_calls[call].p[which] : NULL; }
/* which: 0..2 the offset, 3..5 the dims */
int stub_window_int(int call, int which)
{
    if (call < 0 || call >= g_calls_n || which < 0 || which >= 6) return -1;
    return which < 3 ? g_calls[call].offset[which] : g_calls[call].dims[which - 3];
}
const sgmd_volume* stub_window_volume(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].v : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_window_fail_at(int nth) { g_refuse_countdown = nth; }

static void copy_words(const sgmd_volume* v, const int* o, const int* d, const uint32_t* src, uint32_t* dst)
{
    for (int k = 0; k < d[2]; ++k)
        for (int j = 0; j < d[1]; ++j)
            for (int i = 0; i < d[0]; ++i) {
                const int si = i + o[0], sj = j + o[1], sk = k + o[2];
                const int inside = si >= 0 && si < v->nx && sj >= 0 && sj < v->ny && sk >= 0 && sk < v->nz;
                dst[((size_t)k * (size_t)d[1] + (size_t)j) * (size_t)d[0] + (size_t)i] =
                    inside ? src[((size_t)sk * (size_t)v->ny + (size_t)sj) * (size_t)v->nx + (size_t)si] : 0u;
            }
}

int sgmd_volume_window(int o, void* st, const sgmd_volume* v, const int* offset, const int* dims, const void* src_voxels,
                       const void* src_colors, void* dst_voxels, void* dst_colors)
{
    (void)o; (void)st;
    ++g_total;
    if (g_calls_n < WIN_LOG_MAX) {
        g_calls[g_calls_n].v = *v;
        memcpy(g_calls[g_calls_n].offset, offset, 3 * sizeof(int));
        memcpy(g_calls[g_calls_n].dims, dims, 3 * sizeof(int));
        g_calls[g_calls_n].p[0] = src_voxels; g_calls[g_calls_n].p[1] = src_colors;
        g_calls[g_calls_n].p[2] = dst_voxels; g_calls[g_calls_n].p[3] = dst_colors;
        ++g_calls_n;
    }
    if (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) return 719;
    if ((size_t)v->nx * v->ny * v->nz * 4 > CAP || (size_t)dims[0] * dims[1] * dims[2] * 4 > CAP) return 0;
    copy_words(v, offset, dims, (const uint32_t*)src_voxels, (uint32_t*)dst_voxels);
    if (src_colors) copy_words(v, offset, dims, (const uint32_t*)src_colors, (uint32_t*)dst_colors);
    return 0;
}
