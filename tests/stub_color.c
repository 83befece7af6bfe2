/*
 * stub_color.c -- TEST INFRASTRUCTURE ONLY (tests/test_color_cpu.py builds it beside tests/stub_device.c, tests/stub_volume.c,
 * tests/stub_raycast.c and, for the driver, tests/stub_mesh.c).
 *
 * The stand-in for the coloured launchers of csrc/sgm_volume.hip -- sgmd_volume_integrate_color, sgmd_volume_raycast_color and
 * sgmd_volume_colors -- which csrc/sgm_host.c references weakly, each on its own: a host linked without this file keeps the volume
 * and refuses the three entry points.  It keeps a log of its own: the kind, the specs, the poses, the pointers and the integers of
 * every call, and it can be told to refuse the n-th call.  While the buffers fit the allocator's cap of stub_device.c (1 MiB) it
 * computes for real -- the colour section of include/sgm_mi355x.h in plain C, built with -ffp-contract=off -- so that a sanitizer
 * build sees every word read and written and the tests can compare with the restatement.  The geometry is the plain stand-ins':
 * the voxels come from sgmd_volume_integrate (stub_volume.c) and depth and normals from sgmd_volume_raycast (stub_raycast.c), which
 * therefore log a call of their own for every coloured call that computes.
 */
#include "sgm_device.h"

#include <math.h>
#include <string.h>

#define COL_LOG_MAX 256
#define CAP ((size_t)1 << 20)
static struct {
    int kind;
    sgmd_volume v;
    sgmd_cloud c;
    sgmd_raycast r;
    float poses[SGMD_MAX_POSES * 12];
    const void* p[9];
    long long n[2];
} g_calls[COL_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_color_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_color_count(void) { return g_calls_n; }
int stub_color_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }   /* 0 integrate, 1 ray-cast, 2 colours */
/* which: integrate -- 0 disp, 1 mask, 2 conf, 3 image, 4 voxels, 5 colours, 6 the poses as given;  ray-cast -- 0 voxels, 1 colours,
 * 2 depth, 3 normal, 4 rgba, 5 the poses as given;  colours -- 0 voxels, 1 colours, 2 records, 3 count, 4 rgba */
const void* stub_color_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 9) ? g_calls[call].p[which] : NULL; }
/* which: integrate -- 0 channels;  colours -- 0 capacity, 1 id_kinds */
long long stub_color_int(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 2) ? g_calls[call].n[which] : -1; }
const sgmd_volume* stub_color_volume(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].v : NULL; }
const sgmd_cloud* stub_color_src(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].c : NULL; }
const sgmd_raycast* stub_color_view(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].r : NULL; }
const float* stub_color_poses(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].poses : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_color_fail_at(int nth) { g_refuse_countdown = nth; }

static int note(int kind, const sgmd_volume* v, const sgmd_cloud* c, const sgmd_raycast* r, const float* poses, int frames,
                const void* const* p, int np, long long n0, long long n1)
{
    if (g_calls_n < COL_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].v = *v;
        if (c) g_calls[g_calls_n].c = *c;
        if (r) g_calls[g_calls_n].r = *r;
        if (poses && frames >= 1 && frames <= SGMD_MAX_POSES) memcpy(g_calls[g_calls_n].poses, poses, (size_t)frames * 12 * sizeof(float));
        g_calls[g_calls_n].n[0] = n0;
        g_calls[g_calls_n].n[1] = n1;
        memcpy(g_calls[g_calls_n++].p, p, (size_t)np * sizeof *p);
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
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
static float lerp(float p, float q, float s) { return p + s * (q - p); }
static uint32_t average(uint32_t c, uint32_t cw, uint32_t p) { return (2u * (c * cw + p) + (cw + 1u)) / (2u * (cw + 1u)); }

int sgmd_volume_integrate_color(int o, void* st, const sgmd_volume* v, const sgmd_cloud* c, const float* poses, const void* disp_,
                                const void* mask_, const void* conf_, const void* image_, int channels, void* voxels_, void* colors_)
{
    const void* p[7] = {disp_, mask_, conf_, image_, voxels_, colors_, poses};
    const int rc = note(0, v, c, NULL, poses, c->B, p, 7, channels, 0);
    if (rc != 0) return rc;
    const size_t n = (size_t)v->nx * v->ny * v->nz, npx = (size_t)c->W * c->H;
    if (n * 4 > CAP || npx * (size_t)c->B * 4 > CAP) return 0;
    const float* disp = (const float*)disp_;
    const uint8_t* mask = (const uint8_t*)mask_;
    const uint16_t* conf = (const uint16_t*)conf_;
    uint32_t* colors = (uint32_t*)colors_;
    const uint32_t cap = v->max_weight < 255u ? v->max_weight : 255u;
    for (size_t g = 0; g < n; ++g) {                              /* a colour word is read once and written at most once */
        const int i = (int)(g % (size_t)v->nx), j = (int)((g / (size_t)v->nx) % (size_t)v->ny), k = (int)(g / ((size_t)v->nx * v->ny));
        const float px = centre(v->origin[0], i, v->voxel), py = centre(v->origin[1], j, v->voxel), pz = centre(v->origin[2], k, v->voxel);
        uint32_t col = colors[g];
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
            if (sdf < -v->trunc || !(sdf <= v->trunc)) continue;  /* updated, and not far in front of the surface */
            uint32_t pix;
            if (channels == 4) {
                pix = ((const uint32_t*)image_)[at] & 0xFFFFFFu;
            } else {
                pix = ((const uint8_t*)image_)[at];
                pix |= (pix << 8) | (pix << 16);
            }
            const uint32_t cw = col >> 24;
            uint32_t next = (cw + 1u < cap ? cw + 1u : cap) << 24;
            for (int ch = 0; ch < 3; ++ch) next |= average((col >> (8 * ch)) & 0xFFu, cw, (pix >> (8 * ch)) & 0xFFu) << (8 * ch);
            col = next;
            touched = 1;
        }
        if (touched) colors[g] = col;
    }
    return sgmd_volume_integrate(o, st, v, c, poses, disp_, mask_, conf_, voxels_);
}

/* the colour at g: trilinear, else nearest, else 0 */
static uint32_t color_at(const sgmd_volume* v, const uint32_t* colors, const float g[3])
{
    const int n[3] = {v->nx, v->ny, v->nz};
    float i0[3], f[3];
    int cell = 1;
    for (int i = 0; i < 3 && cell; ++i) {
        const float h = g[i] - 0.5f;
        cell = finite_bits(h);
        if (!cell) break;
        i0[i] = floorf(h);
        cell = 0.0f <= i0[i] && i0[i] + 1.0f < (float)n[i];
        f[i] = h - i0[i];
    }
    if (cell) {
        uint32_t word[2][2][2];
        for (int dz = 0; dz < 2; ++dz)
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) {
                    word[dz][dy][dx] = colors[(((size_t)i0[2] + (size_t)dz) * (size_t)n[1] + (size_t)i0[1] + (size_t)dy) * (size_t)n[0] + (size_t)i0[0] + (size_t)dx];
                    if ((word[dz][dy][dx] >> 24) == 0u) cell = 0;
                }
        if (cell) {
            uint32_t out = 0xFF000000u;
            for (int ch = 0; ch < 3; ++ch) {
                float c[2];
                for (int dz = 0; dz < 2; ++dz) {
                    float t[2][2];
                    for (int dy = 0; dy < 2; ++dy)
                        for (int dx = 0; dx < 2; ++dx) t[dy][dx] = (float)((word[dz][dy][dx] >> (8 * ch)) & 0xFFu);
                    c[dz] = lerp(lerp(t[0][0], t[0][1], f[0]), lerp(t[1][0], t[1][1], f[0]), f[1]);
                }
                out |= (uint32_t)rintf(fminf(fmaxf(lerp(c[0], c[1], f[2]), 0.0f), 255.0f)) << (8 * ch);
            }
            return out;
        }
    }
    for (int i = 0; i < 3; ++i)
        if (!finite_bits(g[i]) || !(0.0f <= g[i] && g[i] < (float)n[i])) return 0u;
    const uint32_t word = colors[((size_t)floorf(g[2]) * (size_t)n[1] + (size_t)floorf(g[1])) * (size_t)n[0] + (size_t)floorf(g[0])];
    return (word >> 24) ? (0xFF000000u | word) : 0u;
}

int sgmd_volume_raycast_color(int o, void* st, const sgmd_volume* v, const sgmd_raycast* r, const float* poses, const void* voxels_,
                              const void* colors_, void* depth_, void* normal_, void* rgba_)
{
    const void* p[6] = {voxels_, colors_, depth_, normal_, rgba_, poses};
    const int rc = note(1, v, NULL, r, poses, r->B, p, 6, 0, 0);
    if (rc != 0) return rc;
    const size_t npx = (size_t)r->W * r->H;
    if ((size_t)v->nx * v->ny * v->nz * 4 > CAP || npx * (size_t)r->B * 12 > CAP) return 0;
    const int plain = sgmd_volume_raycast(o, st, v, r, poses, voxels_, depth_, normal_);
    if (plain != 0) return plain;
    const float* depth = (const float*)depth_;
    uint32_t* rgba = (uint32_t*)rgba_;
    for (int f = 0; f < r->B; ++f) {
        const float* P = poses + 12 * f;
        for (int y = 0; y < r->H; ++y)
            for (int x = 0; x < r->W; ++x) {
                const size_t px = (size_t)f * npx + (size_t)y * (size_t)r->W + (size_t)x;
                const float Z = depth[px];
                if (!finite_bits(Z)) { rgba[px] = 0u; continue; }
                const float a = ((float)x - r->cx) / r->fx, b = ((float)y - r->cy) / r->fy;
                float g[3];
                for (int i = 0; i < 3; ++i) {
                    const float c = -((P[i] * P[9] + P[3 + i] * P[10]) + P[6 + i] * P[11]);
                    const float d = (P[i] * a + P[3 + i] * b) + P[6 + i];
                    g[i] = (c - v->origin[i]) / v->voxel + Z * (d / v->voxel);
                }
                rgba[px] = color_at(v, (const uint32_t*)colors_, g);
            }
    }
    return 0;
}

int sgmd_volume_colors(int o, void* st, const sgmd_volume* v, const void* voxels_, const void* colors_, const void* records_,
                       size_t capacity, const void* count_, int id_kinds, void* rgba_)
{
    (void)o; (void)st;
    const void* p[5] = {voxels_, colors_, records_, count_, rgba_};
    const int rc = note(2, v, NULL, NULL, NULL, 0, p, 5, (long long)capacity, id_kinds);
    if (rc != 0) return rc;
    const size_t n = (size_t)v->nx * v->ny * v->nz;
    if (n * 4 > CAP || capacity * 16 > CAP) return 0;
    static const int step[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
    const uint32_t* voxels = (const uint32_t*)voxels_;
    const uint32_t* colors = (const uint32_t*)colors_;
    const uint32_t* records = (const uint32_t*)records_;
    uint32_t* rgba = (uint32_t*)rgba_;
    const size_t count = count_ ? *(const uint32_t*)count_ : capacity;
    for (size_t r = 0; r < capacity && r < count; ++r) {
        const uint32_t id = records[4 * r + 3];
        const size_t g = id / (uint32_t)id_kinds;
        const int e = (int)(id % (uint32_t)id_kinds);
        uint32_t out = 0;
        if (g < n && e < id_kinds - 1) {
            const int i = (int)(g % (size_t)v->nx), j = (int)((g / (size_t)v->nx) % (size_t)v->ny), k = (int)(g / ((size_t)v->nx * v->ny));
            if (i + step[e][0] < v->nx && j + step[e][1] < v->ny && k + step[e][2] < v->nz) {
                const size_t m = ((size_t)(k + step[e][2]) * (size_t)v->ny + (size_t)(j + step[e][1])) * (size_t)v->nx + (size_t)(i + step[e][0]);
                const uint32_t cn = colors[g], cm = colors[m];
                const float tn = (float)tq_of(voxels[g]), tm = (float)tq_of(voxels[m]), den = tn - tm;
                const float s = den != 0.0f ? fminf(fmaxf(tn / den, 0.0f), 1.0f) : 0.0f;
                if ((cn >> 24) && (cm >> 24)) {
                    out = 0xFF000000u;
                    for (int ch = 0; ch < 3; ++ch)
                        out |= (uint32_t)rintf(lerp((float)((cn >> (8 * ch)) & 0xFFu), (float)((cm >> (8 * ch)) & 0xFFu), s)) << (8 * ch);
                } else if (cn >> 24) {
                    out = 0xFF000000u | cn;
                } else if (cm >> 24) {
                    out = 0xFF000000u | cm;
                }
            }
        }
        rgba[r] = out;
    }
    return 0;
}
