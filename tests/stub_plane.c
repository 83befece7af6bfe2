/*
 * stub_plane.c -- TEST INFRASTRUCTURE ONLY (tests/test_plane_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-ins for the launchers of csrc/sgm_plane.hip -- sgmd_plane_votes, sgmd_plane_best, sgmd_plane_sums, sgmd_plane_label --
 * which csrc/sgm_host.c references weakly, each on its own: a host linked without this file refuses the entry points.  It keeps a
 * log of its own (the kind of call, the spec as the host validated it, the capacity, the label or K, the pointers), it can be told
 * to refuse the n-th call, and it computes for real, the rules of include/sgm_mi355x.h in plain C, one record and one candidate at
 * a time (build it with -ffp-contract=off), so that a sanitizer build sees every byte read and written and the tests can compare
 * with the restatement.
 */
#include "sgm_device.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct { float normal[3], offset, anchor[3]; uint32_t votes; } plane_t;
typedef struct { float x, y, z; uint32_t tag; } record_t;

#define PLANE_LOG_MAX 256
static struct {
    int kind;                   /* 0 votes, 1 best, 2 sums, 3 label */
    sgmd_plane p;
    size_t capacity;
    int n;                      /* best: K;  label: the label */
    const void* ptr[5];
} g_calls[PLANE_LOG_MAX];
static int g_calls_n, g_total, g_refuse_countdown = -1;

void stub_plane_clear(void) { g_calls_n = g_total = 0; g_refuse_countdown = -1; }
int stub_plane_count(void) { return g_total; }
int stub_plane_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }
int stub_plane_int(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].n : -1; }
size_t stub_plane_capacity(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].capacity : 0; }
/* which: votes records, count, labels, planes;  best planes, best;  sums records, count, labels, plane, sums;  label records, count,
 * plane, labels */
const void* stub_plane_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 5) ? g_calls[call].ptr[which] : NULL; }
const sgmd_plane* stub_plane_spec(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].p : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_plane_fail_at(int nth) { g_refuse_countdown = nth; }

static int record(int kind, const sgmd_plane* p, size_t capacity, int n, const void* a, const void* b, const void* c, const void* d, const void* e)
{
    ++g_total;
    if (g_calls_n < PLANE_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].kind = kind;
        if (p) g_calls[g_calls_n].p = *p;
        g_calls[g_calls_n].capacity = capacity;
        g_calls[g_calls_n].n = n;
        const void* ptrs[5] = {a, b, c, d, e};
        memcpy(g_calls[g_calls_n].ptr, ptrs, sizeof ptrs);
        ++g_calls_n;
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

static uint32_t mix(uint32_t seed, uint32_t k, uint32_t j)
{
    uint32_t x = (seed ^ (k * 0x9E3779B9u)) ^ ((j + 1u) * 0x85EBCA6Bu);
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

static uint64_t list_size(size_t capacity, const void* count)
{
    const uint64_t c = count ? *(const uint32_t*)count : (uint64_t)capacity;
    return c < capacity ? c : (uint64_t)capacity;
}

static int takes_part(const record_t* r, const uint8_t* labels, uint64_t at)
{
    return isfinite(r[at].x) && isfinite(r[at].y) && isfinite(r[at].z) && (!labels || labels[at] == 0);
}

static int is_void(const plane_t* pl) { return pl->normal[0] == 0.0f && pl->normal[1] == 0.0f && pl->normal[2] == 0.0f; }

static int inlier(const record_t* r, const plane_t* pl, float dist)
{
    const float s = (pl->normal[0] * (r->x - pl->anchor[0]) + pl->normal[1] * (r->y - pl->anchor[1])) + pl->normal[2] * (r->z - pl->anchor[2]);
    return isfinite(s) && fabsf(s) <= dist;
}

static void candidate(const sgmd_plane* p, const record_t* r, uint64_t n, const uint8_t* labels, uint32_t k, plane_t* out)
{
    memset(out, 0, sizeof *out);
    uint64_t at[3];
    for (uint32_t j = 0; j < 3; ++j) at[j] = ((uint64_t)mix(p->seed, k, j) * n) >> 32;
    if (at[0] == at[1] || at[0] == at[2] || at[1] == at[2]) return;
    for (int j = 0; j < 3; ++j)
        if (!takes_part(r, labels, at[j])) return;
    const record_t *P0 = &r[at[0]], *P1 = &r[at[1]], *P2 = &r[at[2]];
    const float u[3] = {P1->x - P0->x, P1->y - P0->y, P1->z - P0->z}, v[3] = {P2->x - P0->x, P2->y - P0->y, P2->z - P0->z};
    const float c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const float len2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    if (!isfinite(len2) || !(len2 > 0.0f)) return;
    const float len = sqrtf(len2);
    float nrm[3] = {c[0] / len, c[1] / len, c[2] / len};
    if (!isfinite(nrm[0]) || !isfinite(nrm[1]) || !isfinite(nrm[2]) || (nrm[0] == 0.0f && nrm[1] == 0.0f && nrm[2] == 0.0f)) return;
    float t = (nrm[0] * P0->x + nrm[1] * P0->y) + nrm[2] * P0->z;
    if (!isfinite(t)) return;
    int flip;
    if (p->prior) {
        float d = (nrm[0] * p->axis[0] + nrm[1] * p->axis[1]) + nrm[2] * p->axis[2];
        if (!isfinite(d)) return;
        flip = d < 0.0f;
        if (flip) d = -d;
        if (!(d >= p->threshold)) return;
    } else {
        flip = t > 0.0f;
    }
    if (flip) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; t = -t; }
    memcpy(out->normal, nrm, sizeof nrm);
    out->offset = 0.0f - t;
    out->anchor[0] = P0->x; out->anchor[1] = P0->y; out->anchor[2] = P0->z;
}

int sgmd_plane_votes(int o, void* st, const sgmd_plane* p, const void* records, size_t capacity, const void* count, const void* labels,
                     void* planes)
{
    (void)o; (void)st;
    const int refused = record(0, p, capacity, 0, records, count, labels, planes, NULL);
    if (refused) return refused;
    const record_t* r = (const record_t*)records;
    const uint64_t n = list_size(capacity, count);
    plane_t* out = (plane_t*)planes;
    for (int k = 0; k < p->hypotheses; ++k) {
        plane_t pl;
        candidate(p, r, n, (const uint8_t*)labels, (uint32_t)k, &pl);
        if (!is_void(&pl))
            for (uint64_t at = 0; at < n; ++at)
                if (takes_part(r, (const uint8_t*)labels, at) && inlier(&r[at], &pl, p->dist)) ++pl.votes;
        out[k] = pl;
    }
    return 0;
}

int sgmd_plane_best(int o, void* st, const void* planes, int K, void* best)
{
    (void)o; (void)st;
    const int refused = record(1, NULL, 0, K, planes, best, NULL, NULL, NULL);
    if (refused) return refused;
    const plane_t* in = (const plane_t*)planes;
    int pick = -1;
    for (int k = 0; k < K; ++k)
        if (!is_void(&in[k]) && (pick < 0 || in[k].votes > in[pick].votes)) pick = k;
    if (pick < 0) memset(best, 0, sizeof(plane_t));
    else memcpy(best, &in[pick], sizeof(plane_t));
    return 0;
}

int sgmd_plane_sums(int o, void* st, const sgmd_plane* p, const void* records, size_t capacity, const void* count, const void* labels,
                    const void* plane, void* sums)
{
    (void)o; (void)st;
    const int refused = record(2, p, capacity, 0, records, count, labels, plane, sums);
    if (refused) return refused;
    const record_t* r = (const record_t*)records;
    const uint64_t n = list_size(capacity, count);
    plane_t pl;
    memcpy(&pl, plane, sizeof pl);
    int64_t acc[10] = {0};
    for (uint64_t at = 0; at < n && !is_void(&pl); ++at) {
        if (!takes_part(r, (const uint8_t*)labels, at) || !inlier(&r[at], &pl, p->dist)) continue;
        const float e[3] = {(r[at].x - pl.anchor[0]) / p->span, (r[at].y - pl.anchor[1]) / p->span, (r[at].z - pl.anchor[2]) / p->span};
        if (!isfinite(e[0]) || !isfinite(e[1]) || !isfinite(e[2]) || !(fabsf(e[0]) <= 8.0f) || !(fabsf(e[1]) <= 8.0f) || !(fabsf(e[2]) <= 8.0f))
            continue;
        const int64_t q[4] = {(int32_t)rintf(e[0] * 65536.0f), (int32_t)rintf(e[1] * 65536.0f), (int32_t)rintf(e[2] * 65536.0f), 1};
        int k = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = i; j < 4; ++j) acc[k++] += q[i] * q[j];
    }
    memcpy(sums, acc, sizeof acc);
    return 0;
}

int sgmd_plane_label(int o, void* st, const sgmd_plane* p, const void* records, size_t capacity, const void* count, const void* plane,
                     int label, void* labels)
{
    (void)o; (void)st;
    const int refused = record(3, p, capacity, label, records, count, plane, labels, NULL);
    if (refused) return refused;
    const record_t* r = (const record_t*)records;
    const uint64_t n = list_size(capacity, count);
    plane_t pl;
    memcpy(&pl, plane, sizeof pl);
    uint8_t* out = (uint8_t*)labels;
    for (uint64_t at = 0; at < n && !is_void(&pl); ++at)
        if (takes_part(r, out, at) && inlier(&r[at], &pl, p->dist)) out[at] = (uint8_t)label;
    return 0;
}
