/*
 * stub_distance.c -- TEST INFRASTRUCTURE ONLY (tests/test_distance_cpu.py builds it beside tests/stub_device.c and, for the driver,
 * the other volume stand-ins).
 *
 * The stand-ins for the launchers of csrc/sgm_distance.hip, sgmd_volume_distance and sgmd_volume_distance_field, which
 * csrc/sgm_host.c references weakly: a host linked without this file keeps the volume and refuses the two calls.  It keeps a log of
 * its own -- the kind of call, the volume, the four integers of the distance spec and the pointers -- and it can be told to refuse
 * the n-th call.  While the volume fits 1 MiB it computes for real, the rules of include/sgm_mi355x.h in plain C: the transform by
 * brute force over a window of the sites (no separable passes, so that it is no copy of the kernels' route), the field as written,
 * every output word written exactly once, so that a sanitizer build sees every word read and written and the tests can compare with
 * the restatement.
 */
#include "sgm_device.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#define DIST_LOG_MAX 256
#define CAP ((size_t)1 << 20)
#define FAR 0xFFFFu
static struct {
    int kind;                   /* 0: sgmd_volume_distance, 1: sgmd_volume_distance_field */
    sgmd_volume v;
    int n[4];                   /* min_weight, radius, side, unknown */
    const void* p[3];
} g_calls[DIST_LOG_MAX];
static int g_calls_n, g_total, g_refuse_countdown = -1;             /* the log keeps the first DIST_LOG_MAX calls, the count all */

void stub_distance_clear(void) { g_calls_n = g_total = 0; g_refuse_countdown = -1; }
int stub_distance_count(void) { return g_total; }
int stub_distance_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }
/* which: distance 0 voxels, 1 dist2; field 0 out2, 1 in2, 2 field */
const void* stub_distance_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 3) ? g_calls[call].p[which] : NULL; }
/* which: 0 min_weight, 1 radius, 2 side, 3 unknown */
int stub_distance_int(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 4) ? g_calls[call].n[which] : -1; }
const sgmd_volume* stub_distance_volume(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].v : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_distance_fail_at(int nth) { g_refuse_countdown = nth; }

static int record(int kind, const sgmd_volume* v, unsigned mw, int r, int side, int unknown, const void* a, const void* b, const void* c)
{
    ++g_total;
    if (g_calls_n < DIST_LOG_MAX) {
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].v = *v;
        g_calls[g_calls_n].n[0] = (int)mw; g_calls[g_calls_n].n[1] = r; g_calls[g_calls_n].n[2] = side; g_calls[g_calls_n].n[3] = unknown;
        g_calls[g_calls_n].p[0] = a; g_calls[g_calls_n].p[1] = b; g_calls[g_calls_n].p[2] = c;
        ++g_calls_n;
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

int sgmd_volume_distance(int o, void* st, const sgmd_volume* v, unsigned min_weight, int radius, int side, int unknown, const void* voxels,
                         void* dist2)
{
    (void)o; (void)st;
    const int refused = record(0, v, min_weight, radius, side, unknown, voxels, dist2, NULL);
    if (refused) return refused;
    const size_t n = (size_t)v->nx * v->ny * v->nz;
    if (n * 4 > CAP) return 0;
    const uint32_t* words = (const uint32_t*)voxels;
    uint16_t* out = (uint16_t*)dist2;
    unsigned char* site = (unsigned char*)malloc(n);
    if (!site) return 720;
    for (size_t i = 0; i < n; ++i) {
        const int observed = (words[i] >> 16) >= min_weight;
        const int in_o = observed ? (int16_t)(words[i] & 0xFFFFu) < 0 : unknown;
        site[i] = (unsigned char)(side ? !in_o : in_o);
    }
    for (int k = 0; k < v->nz; ++k)
        for (int j = 0; j < v->ny; ++j)
            for (int i = 0; i < v->nx; ++i) {
                long best = (long)radius * radius + 1;
                for (int c = k - radius < 0 ? 0 : k - radius; c <= k + radius && c < v->nz; ++c)
                    for (int b = j - radius < 0 ? 0 : j - radius; b <= j + radius && b < v->ny; ++b)
                        for (int a = i - radius < 0 ? 0 : i - radius; a <= i + radius && a < v->nx; ++a)
                            if (site[((size_t)c * v->ny + b) * v->nx + a]) {
                                const long m = (long)(i - a) * (i - a) + (long)(j - b) * (j - b) + (long)(k - c) * (k - c);
                                if (m < best) best = m;
                            }
                out[((size_t)k * v->ny + j) * v->nx + i] = (uint16_t)(best <= (long)radius * radius ? best : (long)FAR);
            }
    free(site);
    return 0;
}

int sgmd_volume_distance_field(int o, void* st, const sgmd_volume* v, const void* out2, const void* in2, void* field)
{
    (void)o; (void)st;
    const int refused = record(1, v, 0, 0, 0, 0, out2, in2, field);
    if (refused) return refused;
    const size_t n = (size_t)v->nx * v->ny * v->nz;
    if (n * 4 > CAP) return 0;
    const uint16_t *a = (const uint16_t*)out2, *b = (const uint16_t*)in2;
    float* f = (float*)field;
    for (size_t i = 0; i < n; ++i) {
        if (a[i] == FAR) f[i] = INFINITY;
        else if (a[i] > 0) f[i] = v->voxel * sqrtf((float)a[i]);
        else if (!b || b[i] == 0) f[i] = 0.0f;
        else if (b[i] == FAR) f[i] = -INFINITY;
        else f[i] = -(v->voxel * sqrtf((float)b[i]));
    }
    return 0;
}
