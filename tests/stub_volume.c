/*
 * stub_volume.c -- TEST INFRASTRUCTURE ONLY (tests/test_volume_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_volume.hip: sgmd_volume_scratch_bytes, sgmd_volume_integrate and sgmd_volume_points, which
 * csrc/sgm_host.c references weakly.  A host linked without this file has no volume.  It keeps a log of its own (the launch log of
 * stub_device.c stays what it is without it): the kind, the specs, the poses and the pointers of every call, and it can be told to
 * refuse the n-th call.  While the buffers fit the allocator's cap of stub_device.c (1 MiB) it computes for real -- plain C float
 * arithmetic, built with -ffp-contract=off -- so that a sanitizer build sees every map entry read and every word written, and the
 * tests can follow a volume from the caller's maps to the surface list.  It touches its scratch the way the kernels do: a count and
 * a base per tile of 2048 voxels; a scratch sized too small is an access the sanitizer reports.
 */
#include "sgm_device.h"

#include <math.h>
#include <string.h>

#define VOL_LOG_MAX 256
#define CAP ((size_t)1 << 20)
#define TILE 2048
static struct {
    int kind;
    unsigned min_weight;
    size_t capacity;
    sgmd_volume v;
    sgmd_cloud c;
    float poses[SGMD_MAX_POSES * 12];
    const void* p[6];
} g_calls[VOL_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_volume_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_volume_count(void) { return g_calls_n; }
int stub_volume_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }         /* 0 integrate, 1 points */
/* which: integrate -- 0 disp, 1 mask, 2 conf, 3 voxels, 4 the poses as given;  points -- 0 voxels, 1 scratch, 2 points, 3 count */
const void* stub_volume_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 6) ? g_calls[call].p[which] : NULL; }
const sgmd_volume* stub_volume_spec(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].v : NULL; }
const sgmd_cloud* stub_volume_src(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].c : NULL; }
const float* stub_volume_poses(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].poses : NULL; }
unsigned stub_volume_min_weight(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].min_weight : 0; }
size_t stub_volume_capacity(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].capacity : 0; }
/* the nth (0-based) call from now on returns an error */
void stub_volume_fail_at(int nth) { g_refuse_countdown = nth; }

static int note(int kind, const sgmd_volume* v, const sgmd_cloud* c, const float* poses, unsigned min_weight, size_t capacity,
                const void* const* p, int np)
{
    if (g_calls_n < VOL_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].min_weight = min_weight;
        g_calls[g_calls_n].capacity = capacity;
        g_calls[g_calls_n].v = *v;
        if (c) g_calls[g_calls_n].c = *c;
        if (c && poses && c->B >= 1 && c->B <= SGMD_MAX_POSES) memcpy(g_calls[g_calls_n].poses, poses, (size_t)c->B * 12 * sizeof(float));
        memcpy(g_calls[g_calls_n++].p, p, (size_t)np * sizeof *p);
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

size_t sgmd_volume_scratch_bytes(int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    return 2 * sizeof(unsigned) * (((size_t)nx * ny * nz + TILE - 1) / TILE);
}

static uint32_t bits_of(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static int finite_bits(float v) { return (bits_of(v) & 0x7F800000u) != 0x7F800000u; }
static float centre(float o, int i, float voxel) { return o + ((float)i + 0.5f) * voxel; }
static int tq_of(uint32_t word) { return (int)(int16_t)(word & 0xFFFFu); }

int sgmd_volume_integrate(int o, void* st, const sgmd_volume* v, const sgmd_cloud* c, const float* poses, const void* disp_,
                          const void* mask_, const void* conf_, void* voxels_)
{
    (void)o; (void)st;
    const void* p[5] = {disp_, mask_, conf_, voxels_, poses};
    const int rc = note(0, v, c, poses, 0, 0, p, 5);
    if (rc != 0) return rc;
    const size_t n = (size_t)v->nx * v->ny * v->nz, npx = (size_t)c->W * c->H;
    if (n * 4 > CAP || npx * (size_t)c->B * 4 > CAP) return 0;
    const float* disp = (const float*)disp_;
    const uint8_t* mask = (const uint8_t*)mask_;
    const uint16_t* conf = (const uint16_t*)conf_;
    uint32_t* voxels = (uint32_t*)voxels_;
    for (size_t g = 0; g < n; ++g) {                              /* a voxel's word is read once and written at most once */
        const int i = (int)(g % (size_t)v->nx), j = (int)((g / (size_t)v->nx) % (size_t)v->ny), k = (int)(g / ((size_t)v->nx * v->ny));
        const float px = centre(v->origin[0], i, v->voxel), py = centre(v->origin[1], j, v->voxel), pz = centre(v->origin[2], k, v->voxel);
        int64_t tq = tq_of(voxels[g]), w = voxels[g] >> 16;
        int touched = 0;
        for (int f = 0; f < c->B; ++f) {
            const float* P = poses + 12 * f;
            const float Xp = ((P[0] * px + P[1] * py) + P[2] * pz) + P[9];
            const float Yp = ((P[3] * px + P[4] * py) + P[5] * pz) + P[10];
            const float Zp = ((P[6] * px + P[7] * py) + P[8] * pz) + P[11];
            if (!finite_bits(Zp) || !(Zp > 0.0f)) continue;
            const float u = c->fx * (Xp / Zp) + c->cx, vv = c->fy * (Yp / Zp) + c->cy;
            if (!finite_bits(u) || !finite_bits(vv)) continue;
            const float uf = floorf(u + 0.5f), vf = floorf(vv + 0.5f);
            if (!(0.0f <= uf && uf < (float)c->W && 0.0f <= vf && vf < (float)c->H)) continue;
            const size_t at = (size_t)f * npx + (size_t)(unsigned)vf * (size_t)c->W + (unsigned)uf;
            const float d = disp[at];
            if (!finite_bits(d) || (mask && !mask[at]) || (conf && conf[at] < c->min_conf)) continue;
            const float den = d + c->doffs;
            if (!finite_bits(den) || !(den > 0.0f)) continue;
            const float Z = c->fb / den;
            if (!finite_bits(Z) || !(c->z_min <= Z && Z <= c->z_max)) continue;
            const float sdf = Z - Zp;
            if (sdf < -v->trunc) continue;
            const int64_t q = (int64_t)rintf((fminf(sdf, v->trunc) / v->trunc) * 32767.0f);
            const int64_t num = tq * w + q, dn = w + 1, a = 2 * num + dn, b = 2 * dn;
            tq = a / b - ((a % b != 0 && a < 0) ? 1 : 0);          /* floor */
            w = w + 1 < (int64_t)v->max_weight ? w + 1 : (int64_t)v->max_weight;
            touched = 1;
        }
        if (touched) voxels[g] = ((uint32_t)w << 16) | ((uint32_t)tq & 0xFFFFu);
    }
    return 0;
}

/* the crossings of voxel g, bit a: axis a; *tm: the neighbours' tq */
static unsigned crossings_of(const sgmd_volume* v, const uint32_t* voxels, size_t g, unsigned min_weight, int* tm)
{
    const size_t step[3] = {1, (size_t)v->nx, (size_t)v->nx * v->ny};
    const int at[3] = {(int)(g % (size_t)v->nx), (int)((g / (size_t)v->nx) % (size_t)v->ny), (int)(g / ((size_t)v->nx * v->ny))};
    const int lim[3] = {v->nx, v->ny, v->nz};
    unsigned flags = 0;
    if ((voxels[g] >> 16) < min_weight) return 0;
    for (int a = 0; a < 3; ++a) {
        if (at[a] + 1 >= lim[a]) continue;
        const uint32_t other = voxels[g + step[a]];
        tm[a] = tq_of(other);
        if ((other >> 16) >= min_weight && (tq_of(voxels[g]) < 0) != (tm[a] < 0)) flags |= 1u << a;
    }
    return flags;
}

int sgmd_volume_points(int o, void* st, const sgmd_volume* v, const void* voxels_, unsigned min_weight, void* scratch, void* points_,
                       size_t capacity, void* count_)
{
    (void)o; (void)st;
    const void* p[4] = {voxels_, scratch, points_, count_};
    const int rc = note(1, v, NULL, NULL, min_weight, capacity, p, 4);
    if (rc != 0) return rc;
    const size_t n = (size_t)v->nx * v->ny * v->nz, ntiles = (n + TILE - 1) / TILE;
    if (n * 4 > CAP) return 0;
    const uint32_t* voxels = (const uint32_t*)voxels_;
    unsigned* kept = (unsigned*)scratch;
    unsigned* base = kept + ntiles;
    int tm[3] = {0, 0, 0};
    for (size_t t = 0; t < ntiles; ++t) {                         /* count */
        kept[t] = 0;
        for (size_t g = t * TILE; g < n && g < (t + 1) * TILE; ++g) kept[t] += (unsigned)__builtin_popcount(crossings_of(v, voxels, g, min_weight, tm));
    }
    unsigned run = 0;
    for (size_t t = 0; t < ntiles; ++t) { base[t] = run; run += kept[t]; }      /* scan */
    *(uint32_t*)count_ = run;
    struct point { float c[3]; uint32_t id; }* points = (struct point*)points_;
    for (size_t t = 0; t < ntiles && capacity; ++t) {             /* emit */
        size_t to = base[t];
        for (size_t g = t * TILE; g < n && g < (t + 1) * TILE; ++g) {
            const unsigned flags = crossings_of(v, voxels, g, min_weight, tm);
            const int i = (int)(g % (size_t)v->nx), j = (int)((g / (size_t)v->nx) % (size_t)v->ny), k = (int)(g / ((size_t)v->nx * v->ny));
            const float tn = (float)tq_of(voxels[g]);
            for (int a = 0; a < 3; ++a) {
                if (!(flags & (1u << a))) continue;
                struct point q = {{centre(v->origin[0], i, v->voxel), centre(v->origin[1], j, v->voxel), centre(v->origin[2], k, v->voxel)},
                                  (uint32_t)(g * 4 + (size_t)a)};
                const float s = tn / (tn - (float)tm[a]);
                q.c[a] = q.c[a] + s * v->voxel;
                if (to < capacity) points[to] = q;
                ++to;
            }
        }
    }
    return 0;
}
