/*
 * stub_track.c -- TEST INFRASTRUCTURE ONLY (tests/test_track_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for the launcher of csrc/sgm_track.hip, sgmd_track_sums, which csrc/sgm_host.c references weakly and on its own: a
 * host linked without this file refuses sgm_track_sums and sgm_track and keeps the rest.  It keeps a log of its own (the launch
 * log of stub_device.c stays what it is without it): the source, the model, the poses and the pointers of every call, and it can
 * be told to refuse the n-th call.  It computes for real -- the contract of include/sgm_mi355x.h (sgm_track_spec) in plain C float
 * arithmetic, built with -ffp-contract=off -- so that a sanitizer build sees every element read and every sum written and the
 * tests can compare its sums with the restatement's.
 */
#include "sgm_device.h"

#include <math.h>
#include <string.h>

#define TRACK_LOG_MAX 256
static struct {
    sgmd_cloud c;
    sgmd_track t;
    float poses[SGMD_MAX_POSES * 12];
    const void* p[7];
} g_calls[TRACK_LOG_MAX];
static int g_calls_n, g_total, g_refuse_countdown = -1;           /* g_total: every call, also those past the log's end */

void stub_track_clear(void) { g_calls_n = g_total = 0; g_refuse_countdown = -1; }
int stub_track_count(void) { return g_total; }
/* which: 0 disp, 1 mask, 2 conf, 3 model depth, 4 model normal, 5 sums, 6 the poses as given */
const void* stub_track_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 7) ? g_calls[call].p[which] : NULL; }
const sgmd_cloud* stub_track_source(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].c : NULL; }
const sgmd_track* stub_track_model(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].t : NULL; }
const float* stub_track_poses(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].poses : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_track_fail_at(int nth) { g_refuse_countdown = nth; }

static int finite_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}

int sgmd_track_sums(int o, void* st, const sgmd_cloud* c, const sgmd_track* t, const float* poses, const void* disp_, const void* mask_,
                    const void* conf_, const void* depth_, const void* normal_, void* sums_)
{
    (void)o; (void)st;
    ++g_total;
    if (g_calls_n < TRACK_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].c = *c;
        g_calls[g_calls_n].t = *t;
        if (poses && c->B >= 1 && c->B <= SGMD_MAX_POSES) memcpy(g_calls[g_calls_n].poses, poses, (size_t)c->B * 12 * sizeof(float));
        const void* p[7] = {disp_, mask_, conf_, depth_, normal_, sums_, poses};
        memcpy(g_calls[g_calls_n++].p, p, sizeof p);
    }
    if (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) return 719;
    const float* disp = (const float*)disp_;
    const uint8_t* mask = (const uint8_t*)mask_;
    const uint16_t* conf = (const uint16_t*)conf_;
    int64_t* sums = (int64_t*)sums_;
    const size_t npx = (size_t)c->W * c->H, mpx = (size_t)t->W * t->H;
    const float gate = t->dist_max * t->dist_max;
    memset(sums, 0, (size_t)c->B * 29 * sizeof(int64_t));
    for (int f = 0; f < c->B; ++f) {
        const float* P = poses + 12 * f;
        const float* depth = (const float*)depth_ + (size_t)f * mpx;
        const float* normal = (const float*)normal_ + 3 * (size_t)f * mpx;
        int64_t* out = sums + 29 * f;
        for (int y = 0; y < c->H; ++y)
            for (int x = 0; x < c->W; ++x) {
                const size_t px = (size_t)f * npx + (size_t)y * (size_t)c->W + (size_t)x;
                const float d = disp[px], den = d + c->doffs, Z = c->fb / den;
                if (!(finite_bits(d) && (!mask || mask[px] != 0) && (!conf || conf[px] >= c->min_conf) && finite_bits(den) && den > 0.0f &&
                      finite_bits(Z) && c->z_min <= Z && Z <= c->z_max))
                    continue;
                const float X = (((float)x - c->cx) * Z) / c->fx, Y = (((float)y - c->cy) * Z) / c->fy;
                const float Px = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[9];
                const float Py = ((P[3] * X + P[4] * Y) + P[5] * Z) + P[10];
                const float Pz = ((P[6] * X + P[7] * Y) + P[8] * Z) + P[11];
                if (!finite_bits(Pz) || !(Pz > 0.0f)) continue;
                const float u = t->fx * (Px / Pz) + t->cx, v = t->fy * (Py / Pz) + t->cy;
                if (!finite_bits(u) || !finite_bits(v)) continue;
                const float uf = floorf(u + 0.5f), vf = floorf(v + 0.5f);
                if (!(0.0f <= uf && uf < (float)t->W && 0.0f <= vf && vf < (float)t->H)) continue;
                const size_t at = (size_t)vf * (size_t)t->W + (size_t)uf;
                const float Zm = depth[at];
                if (!finite_bits(Zm) || !(Zm > 0.0f)) continue;
                const float n0 = normal[3 * at], n1 = normal[3 * at + 1], n2 = normal[3 * at + 2];
                if (!finite_bits(n0) || !finite_bits(n1) || !finite_bits(n2)) continue;
                const float e0 = ((uf - t->cx) * Zm) / t->fx - Px, e1 = ((vf - t->cy) * Zm) / t->fy - Py, e2 = Zm - Pz;
                const float d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                if (!finite_bits(d2) || !(d2 <= gate)) continue;
                const float r = (n0 * e0 + n1 * e1) + n2 * e2;
                const float c0 = Py * n2 - Pz * n1, c1 = Pz * n0 - Px * n2, c2 = Px * n1 - Py * n0;
                const float val[7] = {c0 / t->span, c1 / t->span, c2 / t->span, n0, n1, n2, r / t->dist_max};
                int ok = 1;
                int64_t q[7];
                for (int i = 0; i < 7; ++i) {
                    if (!finite_bits(val[i]) || !(fabsf(val[i]) <= 8.0f)) { ok = 0; break; }
                    q[i] = (int64_t)rintf(val[i] * 65536.0f);
                }
                if (!ok) continue;
                int k = 0;
                for (int i = 0; i < 7; ++i)
                    for (int j = i; j < 7; ++j) out[k++] += q[i] * q[j];
                out[28] += 1;
            }
    }
    return 0;
}
