/*
 * stub_cloud.c -- TEST INFRASTRUCTURE ONLY (tests/test_cloud_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_cloud.hip: sgmd_cloud_scratch_bytes, sgmd_cloud_organized and sgmd_cloud_points, which csrc/sgm_host.c
 * references weakly.  A host linked without this file has no point clouds.  It keeps a log of its own (the launch log of
 * stub_device.c stays what it is without clouds): the kind, the spec and the pointers of every call, and it can be told to refuse
 * the n-th call.  While the buffers fit the allocator's cap of stub_device.c (1 MiB) it computes for real -- plain C float
 * arithmetic, built with -ffp-contract=off -- so that a sanitizer build sees every map entry read and every record written, and the
 * tests can follow a cloud from the device buffers to the caller.  It also writes its scratch the way the kernels do (one word per
 * tile, twice), so that a scratch sized too small is an access the sanitizer reports.
 */
#include "sgm_device.h"

#include <math.h>
#include <string.h>

#define CLOUD_LOG_MAX 256
#define CAP ((size_t)1 << 20)
static struct { int kind; sgmd_cloud c; const void* p[6]; } g_calls[CLOUD_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_cloud_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_cloud_count(void) { return g_calls_n; }
int stub_cloud_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }       /* 0 organised, 1 point list */
/* which: 0 disp, 1 mask, 2 conf, 3 xyz / points, 4 offsets, 5 scratch */
const void* stub_cloud_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 6) ? g_calls[call].p[which] : NULL; }
const sgmd_cloud* stub_cloud_spec(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].c : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_cloud_fail_at(int nth) { g_refuse_countdown = nth; }

static int note(int kind, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, const void* out, const void* offsets,
                const void* scratch)
{
    if (g_calls_n < CLOUD_LOG_MAX) {
        const void* p[6] = {disp, mask, conf, out, offsets, scratch};
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].c = *c;
        memcpy(g_calls[g_calls_n++].p, p, sizeof p);
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

static size_t tile_of(size_t npx)
{
    size_t t = 1;
    while (t < 2048 && t < npx) t <<= 1;
    return t;
}

size_t sgmd_cloud_scratch_bytes(int W, int H, int B)
{
    if (W < 1 || H < 1 || B < 1) return 0;
    const size_t npx = (size_t)W * H, t = tile_of(npx);
    return 2 * sizeof(unsigned) * ((npx + t - 1) / t) * (size_t)B;
}

static int finite_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

/* the predicate and the formulas of include/sgm_mi355x.h for pixel (y, x) at linear index i of the batch */
static int point_of(const sgmd_cloud* c, const float* disp, const uint8_t* mask, const uint16_t* conf, size_t i, int y, int x, float* out)
{
    const float d = disp[i];
    if (!finite_bits(d) || (mask && !mask[i]) || (conf && conf[i] < c->min_conf)) return 0;
    const float den = d + c->doffs;
    if (!finite_bits(den) || !(den > 0.0f)) return 0;
    const float Z = c->fb / den;
    if (!finite_bits(Z) || !(c->z_min <= Z && Z <= c->z_max)) return 0;
    out[0] = (((float)x - c->cx) * Z) / c->fx;
    out[1] = (((float)y - c->cy) * Z) / c->fy;
    out[2] = Z;
    return 1;
}

int sgmd_cloud_organized(int o, void* st, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, void* xyz)
{
    (void)o; (void)st;
    const int rc = note(0, c, disp, mask, conf, xyz, NULL, NULL);
    if (rc != 0) return rc;
    const size_t npx = (size_t)c->W * c->H, n = npx * (size_t)c->B;
    if (n * 3 * sizeof(float) > CAP) return 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t p = i % npx;
        uint32_t* out = (uint32_t*)xyz + 3 * i;
        float v[3];
        if (point_of(c, (const float*)disp, (const uint8_t*)mask, (const uint16_t*)conf, i, (int)(p / (size_t)c->W), (int)(p % (size_t)c->W), v))
            memcpy(out, v, sizeof v);
        else
            out[0] = out[1] = out[2] = 0x7FC00000u;
    }
    return 0;
}

int sgmd_cloud_points(int o, void* st, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, void* scratch,
                      void* points, void* offsets)
{
    (void)o; (void)st;
    const int rc = note(1, c, disp, mask, conf, points, offsets, scratch);
    if (rc != 0) return rc;
    const size_t npx = (size_t)c->W * c->H, n = npx * (size_t)c->B;
    if (n * 16 > CAP) return 0;
    const size_t t = tile_of(npx), tpf = (npx + t - 1) / t, ntiles = tpf * (size_t)c->B;
    unsigned* kept = (unsigned*)scratch;
    unsigned* base = kept + ntiles;
    uint32_t* off = (uint32_t*)offsets;
    unsigned char* rec = (unsigned char*)points;
    uint32_t total = 0;
    for (int f = 0; f < c->B; ++f) {
        off[f] = total;
        for (size_t p = 0; p < npx; ++p) {
            const size_t tile = (size_t)f * tpf + p / t;
            if (p % t == 0) { base[tile] = total; kept[tile] = 0; }
            float v[3];
            const int y = (int)(p / (size_t)c->W), x = (int)(p % (size_t)c->W);
            if (!point_of(c, (const float*)disp, (const uint8_t*)mask, (const uint16_t*)conf, (size_t)f * npx + p, y, x, v)) continue;
            const uint32_t pixel = ((uint32_t)y << 16) | (uint32_t)x;
            memcpy(rec + (size_t)total * 16, v, 12);
            memcpy(rec + (size_t)total * 16 + 12, &pixel, 4);
            ++total;
            ++kept[tile];
        }
    }
    off[c->B] = total;
    return 0;
}
