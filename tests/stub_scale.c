/*
 * stub_scale.c -- TEST INFRASTRUCTURE ONLY (tests/test_scaled_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_scale.hip: sgmd_downscale and sgmd_upscale, which csrc/sgm_host.c references weakly.  A host linked
 * without this file has no scaled match.  It keeps a log of its own (the launch log of stub_device.c stays what it is without it):
 * the kind, the spec, the pointers of every call and how long stub_device.c's log was at that moment, which places the call among
 * the other launches; and it can be told to refuse the n-th call.  While the buffers fit the allocator's cap of stub_device.c
 * (1 MiB) it computes for real -- plain C loops over the definition of include/sgm_mi355x.h, built with -ffp-contract=off -- so
 * that a sanitizer build sees every sample, word and map entry read and written, and the tests can follow a map from the device
 * buffers to the caller.
 */
#include "sgm_device.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

int stub_log_size(void);                                         /* stub_device.c */

#define SCALE_LOG_MAX 256
#define CAP ((size_t)1 << 20)
static struct { int kind, at; sgmd_scale c; const void* p[7]; } g_calls[SCALE_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_scale_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_scale_count(void) { return g_calls_n; }
int stub_scale_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }     /* 0 downscale, 1 upscale */
int stub_scale_at(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].at : -1; }
/* downscale: 0 in, 1 out; upscale: 0 small map, 1 small guide, 2 full guide, 3 census ref, 4 census other, 5 full map */
const void* stub_scale_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 7) ? g_calls[call].p[which] : NULL; }
const sgmd_scale* stub_scale_spec(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].c : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_scale_fail_at(int nth) { g_refuse_countdown = nth; }

static int note(int kind, const sgmd_scale* c, const void* a, const void* b, const void* d, const void* e, const void* f, const void* g)
{
    if (g_calls_n < SCALE_LOG_MAX) {
        const void* p[7] = {a, b, d, e, f, g, NULL};
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].at = stub_log_size();
        g_calls[g_calls_n].c = *c;
        memcpy(g_calls[g_calls_n++].p, p, sizeof p);
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

static unsigned sample(const void* img, size_t i, int wide) { return wide ? ((const uint16_t*)img)[i] : ((const uint8_t*)img)[i]; }

int sgmd_downscale(int o, void* st, const sgmd_scale* c, const void* in, void* out)
{
    (void)o; (void)st;
    const int rc = note(0, c, in, out, NULL, NULL, NULL, NULL);
    if (rc != 0) return rc;
    const int f = c->f, w = c->W / f, h = c->H / f, wide = c->bits > 8, shift = f == 2 ? 2 : 4;
    if ((size_t)c->B * c->W * c->H * (wide ? 2 : 1) > CAP) return 0;
    for (int b = 0; b < c->B; ++b)
        for (int j = 0; j < h; ++j)
            for (int i = 0; i < w; ++i) {
                unsigned sum = (unsigned)(f * f / 2);
                for (int r = 0; r < f; ++r)
                    for (int k = 0; k < f; ++k) sum += sample(in, ((size_t)b * c->H + (size_t)(f * j + r)) * c->W + (size_t)(f * i + k), wide);
                const size_t at = ((size_t)b * h + j) * w + i;
                if (wide) ((uint16_t*)out)[at] = (uint16_t)(sum >> shift);
                else ((uint8_t*)out)[at] = (uint8_t)(sum >> shift);
            }
    return 0;
}

static int finite_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

static int floor_div(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* the prior of pixel (y, x) of frame b; +INF where no candidate is finite */
static float prior_of(const sgmd_scale* c, const float* small, const void* gs, const void* gf, int b, int y, int x)
{
    const int f = c->f, w = c->W / f, h = c->H / f, wide = c->bits > 8;
    const int ny = 2 * y + 1 - f, nx = 2 * x + 1 - f;
    const int jf = floor_div(ny, 2 * f), fi = floor_div(nx, 2 * f), ay = ny - 2 * f * jf, ax = nx - 2 * f * fi;
    const int js[2] = {clampi(jf, 0, h - 1), clampi(jf + 1, 0, h - 1)}, is[2] = {clampi(fi, 0, w - 1), clampi(fi + 1, 0, w - 1)};
    const int wy[2] = {2 * f - ay, ay}, wx[2] = {2 * f - ax, ax};
    const int g = (int)sample(gf, ((size_t)b * c->H + y) * c->W + x, wide);
    float best = INFINITY;
    int best_diff = 0, best_w = 0, have = 0;
    for (int k = 0; k < 4; ++k) {
        const size_t at = ((size_t)b * h + js[k >> 1]) * w + is[k & 1];
        const float d = small[at];
        if (!finite_bits(d)) continue;
        const int diff = abs((int)sample(gs, at, wide) - g), wgt = wy[k >> 1] * wx[k & 1];
        if (!have || diff < best_diff || (diff == best_diff && wgt > best_w)) { have = 1; best = d; best_diff = diff; best_w = wgt; }
    }
    return have ? (float)f * best : INFINITY;
}

static int popcount32(uint32_t v)
{
    int n = 0;
    for (; v; v &= v - 1) ++n;
    return n;
}

int sgmd_upscale(int o, void* st, const sgmd_scale* c, const void* disp_small, const void* guide_small, const void* guide_full,
                 const void* census_ref, const void* census_oth, void* disp_full)
{
    (void)o; (void)st;
    const int rc = note(1, c, disp_small, guide_small, guide_full, census_ref, census_oth, disp_full);
    if (rc != 0) return rc;
    const size_t npx = (size_t)c->W * c->H;
    if (npx * c->B * 4 > CAP) return 0;
    const int f = c->f, r = c->radius, win = (2 * r + 1) * (2 * r + 1);
    const uint32_t *cr = (const uint32_t*)census_ref, *co = (const uint32_t*)census_oth;
    float* out = (float*)disp_full;
    for (int b = 0; b < c->B; ++b)
        for (int y = 0; y < c->H; ++y)
            for (int x = 0; x < c->W; ++x) {
                float* dst = out + (size_t)b * npx + (size_t)y * c->W + x;
                const float prior = prior_of(c, (const float*)disp_small, guide_small, guide_full, b, y, x);
                *dst = prior;
                if (r < 0 || !finite_bits(prior)) continue;
                const int p = (int)rintf(fminf(fmaxf(prior, -1048576.0f), 1048576.0f));
                long cost[9];
                int adm[9], best = -1;
                for (int k = 0; k <= 2 * f; ++k) {
                    const int off = k - f, d = p + off;
                    adm[k] = c->d_lo <= d && d <= c->d_hi;
                    long A = 0;
                    for (int dy = -r; dy <= r; ++dy)
                        for (int dx = -r; dx <= r; ++dx) {
                            const int qy = y + dy, qx = x + dx, xo = c->right ? qx + d : qx - d;
                            if (qy < 0 || qy >= c->H || qx < 0 || qx >= c->W || xo < 0 || xo >= c->W) { A += 24; continue; }
                            const size_t row = (size_t)b * npx + (size_t)qy * c->W;
                            A += popcount32(cr[row + qx] ^ co[row + xo]);
                        }
                    cost[k] = 2 * A + (long)c->penalty * abs(off) * win;
                }
                for (int k = 0; k <= 2 * f; ++k) {
                    if (!adm[k]) continue;
                    const int ok = k - f, ob = best - f;
                    if (best < 0 || cost[k] < cost[best] || (cost[k] == cost[best] && (abs(ok) < abs(ob) || (abs(ok) == abs(ob) && ok < ob)))) best = k;
                }
                if (best < 0) continue;
                float v = (float)(p + best - f);
                if (best >= 1 && best < 2 * f && adm[best - 1] && adm[best + 1]) {
                    const long den = cost[best - 1] + cost[best + 1] - 2 * cost[best];
                    if (den > 0) v = v + (float)(cost[best - 1] - cost[best + 1]) / (float)(2 * den);
                }
                *dst = v;
            }
    return 0;
}
