/*
 * stub_components.c -- TEST INFRASTRUCTURE ONLY (tests/test_zz_components_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-ins for the launchers of csrc/sgm_components.hip -- sgmd_components_scratch_bytes, sgmd_volume_components and
 * sgmd_volume_component_of -- which csrc/sgm_host.c references weakly: a host linked without this file keeps the volume and refuses
 * the calls.  It keeps a log of its own -- the kind of call, the volume, the spec, the capacities and the pointers -- and it can be
 * told to refuse the n-th call.  While the volume fits 1 MiB it computes for real, the rules of include/sgm_mi355x.h in plain C:
 * the components by breadth-first search in index order (no tiles, no union-find: not the kernels' route), so that a sanitizer build
 * sees every word read and written and the tests can compare with the restatement.  The scratch is logged and never touched.
 */
#include "sgm_device.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#define COMP_LOG_MAX 256
#define CAP ((size_t)1 << 20)
typedef struct { uint32_t first, voxels; uint16_t lo[3], hi[3]; uint32_t reserved; uint64_t sum[3]; } component;
typedef struct { float x, y, z; uint32_t id; } record16;

static struct {
    int kind;                   /* 0: sgmd_volume_components, 1: sgmd_volume_component_of */
    sgmd_volume v;
    sgmd_components c;          /* kind 0 */
    size_t capacity, records_capacity;
    int id_kinds;
    const void* p[6];
} g_calls[COMP_LOG_MAX];
static int g_calls_n, g_total, g_refuse_countdown = -1;             /* the log keeps the first COMP_LOG_MAX calls, the count all */

void stub_components_clear(void) { g_calls_n = g_total = 0; g_refuse_countdown = -1; }
int stub_components_count(void) { return g_total; }
int stub_components_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }
/* which: components 0 voxels, 1 scratch, 2 labels, 3 objects, 4 counts; component_of 0 labels, 1 objects, 2 counts, 3 records,
 * 4 records_count, 5 index */
const void* stub_components_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 6) ? g_calls[call].p[which] : NULL; }
size_t stub_components_capacity(int call, int records) { return (call >= 0 && call < g_calls_n) ? (records ? g_calls[call].records_capacity : g_calls[call].capacity) : 0; }
int stub_components_id_kinds(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].id_kinds : -1; }
const sgmd_volume* stub_components_volume(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].v : NULL; }
const sgmd_components* stub_components_spec(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].c : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_components_fail_at(int nth) { g_refuse_countdown = nth; }

static int record(int kind, const sgmd_volume* v, const sgmd_components* c, size_t capacity, size_t records_capacity, int id_kinds,
                  const void* const p[6])
{
    ++g_total;
    if (g_calls_n < COMP_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].v = *v;
        if (c) g_calls[g_calls_n].c = *c;
        g_calls[g_calls_n].capacity = capacity; g_calls[g_calls_n].records_capacity = records_capacity; g_calls[g_calls_n].id_kinds = id_kinds;
        memcpy(g_calls[g_calls_n].p, p, sizeof g_calls[0].p);
        ++g_calls_n;
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

size_t sgmd_components_scratch_bytes(int nx, int ny, int nz, size_t capacity)
{
    const size_t n = (size_t)nx * ny * nz;
    return 4 * n + 12 * ((n + 2047) / 2048) + 24 * (capacity < n ? capacity : n);
}

static int finite_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x7F800000u) != 0x7F800000u; }

int sgmd_volume_components(int o, void* st, const sgmd_volume* v, const sgmd_components* c, const void* voxels, void* scratch, void* labels,
                           void* objects, size_t capacity, void* counts)
{
    (void)o; (void)st;
    const void* const p[6] = {voxels, scratch, labels, objects, counts, NULL};
    const int refused = record(0, v, c, capacity, 0, 0, p);
    if (refused) return refused;
    const int nx = v->nx, ny = v->ny, nz = v->nz;
    const size_t n = (size_t)nx * ny * nz;
    if (n * 4 > CAP) return 0;
    const uint32_t* words = (const uint32_t*)voxels;
    uint32_t *lab = (uint32_t*)labels, *cnt = (uint32_t*)counts;
    component* obj = (component*)objects;
    unsigned char* in = (unsigned char*)malloc(n);
    uint32_t* queue = (uint32_t*)malloc(n * sizeof(uint32_t));
    if (!in || !queue) { free(in); free(queue); return 720; }
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const size_t at = ((size_t)k * ny + j) * nx + i;
                const int observed = (words[at] >> 16) >= c->min_weight, neg = (int16_t)(words[at] & 0xFFFFu) < 0;
                int member = observed ? (c->set ? !neg : neg) : c->unknown;
                const float C[3] = {v->origin[0] + ((float)i + 0.5f) * v->voxel, v->origin[1] + ((float)j + 0.5f) * v->voxel,
                                    v->origin[2] + ((float)k + 0.5f) * v->voxel};
                for (int q = 0; q < c->planes && member; ++q) {
                    const float* nr = c->normal[q];
                    const float* a = c->anchor[q];
                    if (nr[0] == 0.0f && nr[1] == 0.0f && nr[2] == 0.0f) continue;
                    const float s = ((nr[0] * (C[0] - a[0]) + nr[1] * (C[1] - a[1])) + nr[2] * (C[2] - a[2]));
                    if (finite_bits(s) && s <= c->clearance[q]) member = 0;
                }
                in[at] = (unsigned char)member;
                lab[at] = 0;
            }
    uint32_t survivors = 0, all = 0;
    for (size_t seed = 0; seed < n; ++seed) {
        if (in[seed] != 1) continue;                               /* 0: outside, 2: visited */
        size_t head = 0, tail = 0;
        component r;
        memset(&r, 0, sizeof r);
        r.first = (uint32_t)seed;
        r.lo[0] = r.lo[1] = r.lo[2] = 0xFFFF;
        queue[tail++] = (uint32_t)seed;
        in[seed] = 2;
        while (head < tail) {
            const uint32_t at = queue[head++];
            const int i = (int)(at % (uint32_t)nx), j = (int)(at / (uint32_t)nx % (uint32_t)ny), k = (int)(at / ((uint32_t)nx * (uint32_t)ny));
            const int at3[3] = {i, j, k};
            for (int a = 0; a < 3; ++a) {
                if (at3[a] < r.lo[a]) r.lo[a] = (uint16_t)at3[a];
                if (at3[a] > r.hi[a]) r.hi[a] = (uint16_t)at3[a];
                r.sum[a] += (uint64_t)at3[a];
            }
            for (int dk = -1; dk <= 1; ++dk)
                for (int dj = -1; dj <= 1; ++dj)
                    for (int di = -1; di <= 1; ++di) {
                        const int steps = (di != 0) + (dj != 0) + (dk != 0);
                        if (steps == 0 || (c->connectivity == 6 && steps != 1)) continue;
                        const int a = i + di, b = j + dj, d = k + dk;
                        if (a < 0 || b < 0 || d < 0 || a >= nx || b >= ny || d >= nz) continue;
                        const size_t to = ((size_t)d * ny + b) * nx + a;
                        if (in[to] == 1) { in[to] = 2; queue[tail++] = (uint32_t)to; }
                    }
        }
        r.voxels = (uint32_t)tail;
        ++all;
        if (r.voxels < c->min_voxels) continue;
        for (size_t q = 0; q < tail; ++q) lab[queue[q]] = r.first + 1u;
        if (survivors < capacity) obj[survivors] = r;
        ++survivors;
    }
    cnt[0] = survivors; cnt[1] = all;
    free(in); free(queue);
    return 0;
}

int sgmd_volume_component_of(int o, void* st, const sgmd_volume* v, const void* labels, const void* objects, size_t capacity, const void* counts,
                             const void* records, size_t records_capacity, const void* records_count, int id_kinds, void* index)
{
    (void)o; (void)st;
    static const int step[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
    const void* const p[6] = {labels, objects, counts, records, records_count, index};
    const int refused = record(1, v, NULL, capacity, records_capacity, id_kinds, p);
    if (refused) return refused;
    const size_t n = (size_t)v->nx * v->ny * v->nz;
    if (n * 4 > CAP || records_capacity * 16 > CAP) return 0;
    const uint32_t *lab = (const uint32_t*)labels, *cnt = (const uint32_t*)counts, *rc = (const uint32_t*)records_count;
    const component* obj = (const component*)objects;
    const record16* rec = (const record16*)records;
    uint32_t* out = (uint32_t*)index;
    const size_t todo = rc && rc[0] < records_capacity ? rc[0] : records_capacity, written = cnt[0] < capacity ? cnt[0] : capacity;
    for (size_t r = 0; r < todo; ++r) {
        const uint32_t id = rec[r].id, at = id / (uint32_t)id_kinds, e = id % (uint32_t)id_kinds;
        out[r] = 0;
        if (at >= n || e >= (uint32_t)id_kinds - 1u) continue;
        uint32_t l = lab[at];
        if (l == 0) {
            const int i = (int)(at % (uint32_t)v->nx) + step[e][0], j = (int)(at / (uint32_t)v->nx % (uint32_t)v->ny) + step[e][1],
                      k = (int)(at / ((uint32_t)v->nx * (uint32_t)v->ny)) + step[e][2];
            if (i < v->nx && j < v->ny && k < v->nz) l = lab[((size_t)k * v->ny + j) * v->nx + i];
        }
        if (l == 0) continue;
        for (size_t q = 0; q < written; ++q)                      /* (a linear search: not the kernel's) */
            if (obj[q].first == l - 1u) { out[r] = (uint32_t)q + 1u; break; }
    }
    return 0;
}
