/*
 * stub_raycast.c -- TEST INFRASTRUCTURE ONLY (tests/test_raycast_cpu.py builds it beside tests/stub_device.c and tests/stub_volume.c).
 *
 * The stand-in for the ray-cast launcher of csrc/sgm_volume.hip, sgmd_volume_raycast, which csrc/sgm_host.c references weakly and on
 * its own: a host linked without this file keeps the volume and refuses the ray-cast.  It keeps a log of its own (the launch log of
 * stub_device.c and the log of stub_volume.c stay what they are without it): the specs, the poses and the pointers of every call,
 * and it can be told to refuse the n-th call.  While the buffers fit the allocator's cap of stub_device.c (1 MiB) it computes for
 * real -- the contract of include/sgm_mi355x.h (sgm_raycast_spec) in plain C float arithmetic, built with -ffp-contract=off -- so
 * that a sanitizer build sees every word read and every pixel written and the tests can compare its maps with the restatement's.
 */
#include "sgm_device.h"

#include <math.h>
#include <string.h>

#define RAY_LOG_MAX 256
#define CAP ((size_t)1 << 20)
static struct {
    sgmd_volume v;
    sgmd_raycast r;
    float poses[SGMD_MAX_POSES * 12];
    const void* p[4];
} g_calls[RAY_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_raycast_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_raycast_count(void) { return g_calls_n; }
/* which: 0 voxels, 1 depth, 2 normal, 3 the poses as given */
const void* stub_raycast_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 4) ? g_calls[call].p[which] : NULL; }
const sgmd_volume* stub_raycast_volume(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].v : NULL; }
const sgmd_raycast* stub_raycast_view(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].r : NULL; }
const float* stub_raycast_poses(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].poses : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_raycast_fail_at(int nth) { g_refuse_countdown = nth; }

static uint32_t bits_of(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static float float_of(uint32_t u)
{
    float v;
    memcpy(&v, &u, 4);
    return v;
}
static int finite_bits(float v) { return (bits_of(v) & 0x7F800000u) != 0x7F800000u; }
static int tq_of(uint32_t word) { return (int)(int16_t)(word & 0xFFFFu); }

typedef struct {
    const sgmd_volume* v;
    const uint32_t* voxels;
    unsigned min_weight;
} grid;

/* the nearest sample at g: 0 invalid, 1 valid and non-negative, 2 valid and negative */
static int nearest(const grid* G, const float g[3])
{
    const int n[3] = {G->v->nx, G->v->ny, G->v->nz};
    for (int i = 0; i < 3; ++i)
        if (!finite_bits(g[i]) || !(0.0f <= g[i] && g[i] < (float)n[i])) return 0;
    const size_t at = ((size_t)floorf(g[2]) * (size_t)n[1] + (size_t)floorf(g[1])) * (size_t)n[0] + (size_t)floorf(g[0]);
    const uint32_t word = G->voxels[at];
    if ((word >> 16) < G->min_weight) return 0;
    return tq_of(word) < 0 ? 2 : 1;
}

static float lerp(float p, float q, float s) { return p + s * (q - p); }

/* F(g): the trilinear value of tq at g - 0.5; 0 where it is not valid */
static int trilinear(const grid* G, const float g[3], float* F)
{
    const int n[3] = {G->v->nx, G->v->ny, G->v->nz};
    float i0[3], f[3];
    for (int i = 0; i < 3; ++i) {
        const float h = g[i] - 0.5f;
        if (!finite_bits(h)) return 0;
        i0[i] = floorf(h);
        if (!(0.0f <= i0[i] && i0[i] + 1.0f < (float)n[i])) return 0;
        f[i] = h - i0[i];
    }
    float t[2][2][2];
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const size_t at = (((size_t)i0[2] + (size_t)dz) * (size_t)n[1] + (size_t)i0[1] + (size_t)dy) * (size_t)n[0] + (size_t)i0[0] + (size_t)dx;
                const uint32_t word = G->voxels[at];
                if ((word >> 16) < G->min_weight) return 0;
                t[dz][dy][dx] = (float)tq_of(word);
            }
    float c[2];
    for (int dz = 0; dz < 2; ++dz) c[dz] = lerp(lerp(t[dz][0][0], t[dz][0][1], f[0]), lerp(t[dz][1][0], t[dz][1][1], f[0]), f[1]);
    *F = lerp(c[0], c[1], f[2]);
    return 1;
}

static void at_z(const float go[3], const float gd[3], float Z, float g[3])
{
    for (int i = 0; i < 3; ++i) g[i] = go[i] + Z * gd[i];
}

int sgmd_volume_raycast(int o, void* st, const sgmd_volume* v, const sgmd_raycast* r, const float* poses, const void* voxels_,
                        void* depth_, void* normal_)
{
    (void)o; (void)st;
    if (g_calls_n < RAY_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].v = *v;
        g_calls[g_calls_n].r = *r;
        if (poses && r->B >= 1 && r->B <= SGMD_MAX_POSES) memcpy(g_calls[g_calls_n].poses, poses, (size_t)r->B * 12 * sizeof(float));
        const void* p[4] = {voxels_, depth_, normal_, poses};
        memcpy(g_calls[g_calls_n++].p, p, sizeof p);
    }
    if (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) return 719;
    const size_t npx = (size_t)r->W * r->H;
    if ((size_t)v->nx * v->ny * v->nz * 4 > CAP || npx * (size_t)r->B * 12 > CAP) return 0;
    const grid G = {v, (const uint32_t*)voxels_, r->min_weight};
    float* depth = (float*)depth_;
    float* normal = (float*)normal_;
    const float nan = float_of(0x7FC00000u);
    for (int f = 0; f < r->B; ++f) {
        const float* P = poses + 12 * f;
        float c[3];
        for (int i = 0; i < 3; ++i) c[i] = -((P[i] * P[9] + P[3 + i] * P[10]) + P[6 + i] * P[11]);
        for (int y = 0; y < r->H; ++y)
            for (int x = 0; x < r->W; ++x) {
                const size_t px = (size_t)f * npx + (size_t)y * (size_t)r->W + (size_t)x;
                const float a = ((float)x - r->cx) / r->fx, b = ((float)y - r->cy) / r->fy;
                float go[3], gd[3], g[3];
                for (int i = 0; i < 3; ++i) {
                    const float d = (P[i] * a + P[3 + i] * b) + P[6 + i];
                    go[i] = (c[i] - v->origin[i]) / v->voxel;
                    gd[i] = d / v->voxel;
                }
                float Z = nan, n[3] = {nan, nan, nan}, Zp = 0.0f, Zc = 0.0f;
                int prev = 0, front = 0;
                for (unsigned k = 0;; ++k) {
                    Zc = r->z_min + (float)k * r->step;
                    if (!(Zc <= r->z_max)) break;
                    at_z(go, gd, Zc, g);
                    const int cur = nearest(&G, g);
                    if (prev == 1 && cur == 2) { front = 1; break; }
                    if (prev == 2 && cur == 1) break;
                    prev = cur;
                    Zp = Zc;
                }
                float Fp = 0.0f, Fc = 0.0f;
                int ok = 0;
                if (front) {
                    at_z(go, gd, Zp, g);
                    ok = trilinear(&G, g, &Fp);
                    at_z(go, gd, Zc, g);
                    ok = trilinear(&G, g, &Fc) && ok;
                }
                if (ok && Fp - Fc > 0.0f) {
                    const float s = fminf(fmaxf(Fp / (Fp - Fc), 0.0f), 1.0f);
                    Z = Zp + s * r->step;
                    if (normal) {
                        float nw[3], up = 0.0f, dn = 0.0f;
                        int all = 1;
                        at_z(go, gd, Z, g);
                        for (int ax = 0; ax < 3; ++ax) {
                            float e[3] = {g[0], g[1], g[2]};
                            e[ax] = g[ax] + 1.0f;
                            all = trilinear(&G, e, &up) && all;
                            e[ax] = g[ax] - 1.0f;
                            all = trilinear(&G, e, &dn) && all;
                            nw[ax] = up - dn;
                        }
                        if (all) {
                            float m[3];
                            for (int q = 0; q < 3; ++q) m[q] = (P[3 * q] * nw[0] + P[3 * q + 1] * nw[1]) + P[3 * q + 2] * nw[2];
                            const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
                            if (finite_bits(len) && len > 0.0f)
                                for (int q = 0; q < 3; ++q) n[q] = m[q] / len;
                        }
                    }
                }
                depth[px] = Z;
                if (normal) memcpy(normal + 3 * px, n, sizeof n);
            }
    }
    return 0;
}
