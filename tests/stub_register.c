/*
 * stub_register.c -- TEST INFRASTRUCTURE ONLY (tests/test_register_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_register.hip: sgmd_register_scratch_bytes, sgmd_register_depth and sgmd_register_gather, which
 * csrc/sgm_host.c references weakly.  A host linked without this file has no registration.  It keeps a log of its own (the launch
 * log of stub_device.c stays what it is without it): the kind, the two specs and the pointers of every call, and it can be told to
 * refuse the n-th call.  While the buffers fit the allocator's cap of stub_device.c (1 MiB) it computes for real -- plain C float
 * arithmetic, built with -ffp-contract=off -- so that a sanitizer build sees every map entry read and every output written, and
 * the tests can follow a registration from the device buffers to the caller.  It touches its scratch the way the kernels do: every
 * 16-byte pair of keys is set to all ones, every admitted candidate takes the minimum of one key, every pair is read back; a
 * scratch sized too small is an access the sanitizer reports.
 */
#include "sgm_device.h"

#include <math.h>
#include <string.h>

#define REG_LOG_MAX 256
#define CAP ((size_t)1 << 20)
static struct { int kind, elem_bytes; unsigned fill; sgmd_cloud c; sgmd_register r; const void* p[7]; } g_calls[REG_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_register_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_register_count(void) { return g_calls_n; }
int stub_register_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }       /* 0 depth, 1 gather */
/* which: depth -- 0 disp, 1 mask, 2 conf, 3 keys, 4 depth, 5 source;  gather -- 0 source, 1 map, 2 out */
const void* stub_register_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 7) ? g_calls[call].p[which] : NULL; }
const sgmd_cloud* stub_register_src(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].c : NULL; }
const sgmd_register* stub_register_dst(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].r : NULL; }
int stub_register_elem(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].elem_bytes : -1; }
unsigned stub_register_fill(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].fill : 0; }
/* the nth (0-based) call from now on returns an error */
void stub_register_fail_at(int nth) { g_refuse_countdown = nth; }

static int note(int kind, const sgmd_cloud* c, const sgmd_register* r, int elem_bytes, unsigned fill, const void* const* p, int np)
{
    if (g_calls_n < REG_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].elem_bytes = elem_bytes;
        g_calls[g_calls_n].fill = fill;
        g_calls[g_calls_n].c = *c;
        g_calls[g_calls_n].r = *r;
        memcpy(g_calls[g_calls_n++].p, p, (size_t)np * sizeof *p);
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

size_t sgmd_register_scratch_bytes(int W, int H, int B)
{
    if (W < 1 || H < 1 || B < 1) return 0;
    return 16 * (((size_t)W * H * B + 1) / 2);
}

static uint32_t bits_of(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static int finite_bits(float v) { return (bits_of(v) & 0x7F800000u) != 0x7F800000u; }

static void vote(uint64_t* keys, const sgmd_register* r, float uf, float vf, uint64_t k)
{
    if (!(0.0f <= uf && uf < (float)r->W && 0.0f <= vf && vf < (float)r->H)) return;
    uint64_t* at = keys + (size_t)(unsigned)vf * (size_t)r->W + (unsigned)uf;
    if (k < *at) *at = k;
}

int sgmd_register_depth(int o, void* st, const sgmd_cloud* c, const sgmd_register* r, const void* disp_, const void* mask_,
                        const void* conf_, void* keys_, void* depth_, void* source_)
{
    (void)o; (void)st;
    const void* p[6] = {disp_, mask_, conf_, keys_, depth_, source_};
    const int rc = note(0, c, r, 0, 0, p, 6);
    if (rc != 0) return rc;
    const size_t npx = (size_t)c->W * c->H, tpx = (size_t)r->W * r->H, nk = tpx * (size_t)c->B, n2 = (nk + 1) / 2;
    if (npx * (size_t)c->B * 4 > CAP || n2 * 16 > CAP) return 0;
    const float* disp = (const float*)disp_;
    const uint8_t* mask = (const uint8_t*)mask_;
    const uint16_t* conf = (const uint16_t*)conf_;
    uint64_t* keys = (uint64_t*)keys_;
    for (size_t i = 0; i < 2 * n2; ++i) keys[i] = ~(uint64_t)0;                                   /* clear: whole pairs */
    for (int f = 0; f < c->B; ++f)
        for (size_t q = 0; q < npx; ++q) {
            const size_t i = (size_t)f * npx + q;
            const unsigned y = (unsigned)(q / (size_t)c->W), x = (unsigned)(q % (size_t)c->W);
            const float d = disp[i];
            if (!finite_bits(d) || (mask && !mask[i]) || (conf && conf[i] < c->min_conf)) continue;
            const float den = d + c->doffs;
            if (!finite_bits(den) || !(den > 0.0f)) continue;
            const float Z = c->fb / den;
            if (!finite_bits(Z) || !(c->z_min <= Z && Z <= c->z_max)) continue;
            const float X = (((float)x - c->cx) * Z) / c->fx, Y = (((float)y - c->cy) * Z) / c->fy;
            const float Xp = ((r->R[0] * X + r->R[1] * Y) + r->R[2] * Z) + r->t[0];
            const float Yp = ((r->R[3] * X + r->R[4] * Y) + r->R[5] * Z) + r->t[1];
            const float Zp = ((r->R[6] * X + r->R[7] * Y) + r->R[8] * Z) + r->t[2];
            if (!finite_bits(Zp) || !(Zp > 0.0f && r->z_min <= Zp && Zp <= r->z_max)) continue;
            const float a = Xp / Zp, b = Yp / Zp, aa = a * a, bb = b * b, ab = a * b, r2 = aa + bb;
            const float rad = ((r->dist[4] * r2 + r->dist[1]) * r2 + r->dist[0]) * r2 + 1.0f;
            const float xd = (a * rad + (2.0f * r->dist[2]) * ab) + r->dist[3] * (r2 + 2.0f * aa);
            const float yd = (b * rad + r->dist[2] * (r2 + 2.0f * bb)) + (2.0f * r->dist[3]) * ab;
            const float u = r->fx * xd + r->cx, v = r->fy * yd + r->cy;
            if (!finite_bits(u) || !finite_bits(v)) continue;
            const uint64_t k = ((uint64_t)bits_of(Zp) << 32) | (uint64_t)((y << 16) | x);
            uint64_t* fk = keys + (size_t)f * tpx;
            if (r->splat == 1) vote(fk, r, floorf(u + 0.5f), floorf(v + 0.5f), k);
            else {
                const float u0 = floorf(u), v0 = floorf(v), u1 = u0 + 1.0f, v1 = v0 + 1.0f;
                vote(fk, r, u0, v0, k); vote(fk, r, u1, v0, k); vote(fk, r, u0, v1, k); vote(fk, r, u1, v1, k);
            }
        }
    uint32_t* depth = (uint32_t*)depth_;
    uint32_t* source = (uint32_t*)source_;
    for (size_t g = 0; g < 2 * n2; ++g) {                                                         /* resolve: reads whole pairs */
        const uint64_t k = keys[g];
        if (g >= nk) continue;
        const int hit = (uint32_t)(k >> 32) != 0xFFFFFFFFu;
        depth[g] = hit ? (uint32_t)(k >> 32) : 0x7FC00000u;
        if (source) source[g] = hit ? (uint32_t)k : 0xFFFFFFFFu;
    }
    return 0;
}

int sgmd_register_gather(int o, void* st, const sgmd_cloud* c, const sgmd_register* r, const void* source_, int elem_bytes,
                         const void* map, unsigned fill, void* out)
{
    (void)o; (void)st;
    const void* p[3] = {source_, map, out};
    const int rc = note(1, c, r, elem_bytes, fill, p, 3);
    if (rc != 0) return rc;
    const size_t npx = (size_t)c->W * c->H, tpx = (size_t)r->W * r->H, n = tpx * (size_t)c->B;
    if (n * 4 > CAP || npx * (size_t)c->B * (size_t)elem_bytes > CAP) return 0;
    const uint32_t* source = (const uint32_t*)source_;
    for (size_t g = 0; g < n; ++g) {
        const uint32_t s = source[g];
        const unsigned y = s >> 16, x = s & 0xFFFFu;
        unsigned char* to = (unsigned char*)out + g * (size_t)elem_bytes;
        if (s != 0xFFFFFFFFu && y < (unsigned)c->H && x < (unsigned)c->W)
            memcpy(to, (const unsigned char*)map + ((g / tpx) * npx + (size_t)y * (size_t)c->W + x) * (size_t)elem_bytes, (size_t)elem_bytes);
        else
            memcpy(to, &fill, (size_t)elem_bytes);
    }
    return 0;
}
