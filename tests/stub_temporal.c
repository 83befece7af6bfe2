/*
 * stub_temporal.c -- TEST INFRASTRUCTURE ONLY (tests/test_temporal_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_temporal.hip: sgmd_temporal, sgmd_temporal_scratch_bytes and sgmd_temporal_clear, which csrc/sgm_host.c references weakly.  A host
 * linked without this file has no temporal filter.  It keeps a log of its own (the launch log of stub_device.c stays what it is
 * without the filter): the kind, the geometry, the parameters, the pointers and the stream of every call, and how long the launch
 * log of stub_device.c was at that moment, which places the call among the other launches; it can be told to refuse the n-th call.
 * While the maps fit the cap below (the allocator's cap of stub_device.c, 1 MiB, unless a test that brings its own buffers raises
 * it) it computes for real -- plain C float arithmetic, built with -ffp-contract=off -- so that a sanitizer build sees every
 * entry read and written, and the tests can follow a filtered map from the device buffers to the caller.
 */
#include "sgm_device.h"

#include <string.h>

#define TP_LOG_MAX 256
static struct { int kind, at; sgmd_temporal_params p; size_t streams, steps, pixels; const void* ptr[5]; const void* stream; } g_calls[TP_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;
static size_t g_cap = (size_t)1 << 20;

void stub_temporal_clear_log(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_temporal_count(void) { return g_calls_n; }
int stub_temporal_kind(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].kind : -1; }      /* 0 filter, 1 clear */
/* which: 0 streams, 1 steps, 2 pixels (a clear: its count) */
size_t stub_temporal_geometry(int call, int which)
{
    if (call < 0 || call >= g_calls_n) return 0;
    return which == 0 ? g_calls[call].streams : (which == 1 ? g_calls[call].steps : g_calls[call].pixels);
}
/* which: 0 maps, 1 conf, 2 hist_value, 3 hist_bits, 4 stats */
const void* stub_temporal_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 5) ? g_calls[call].ptr[which] : NULL; }
const sgmd_temporal_params* stub_temporal_params(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].p : NULL; }
/* the nth (0-based) call from now on returns an error */
void stub_temporal_fail_at(int nth) { g_refuse_countdown = nth; }
/* maps of more bytes than this are logged and not computed */
void stub_temporal_cap(size_t bytes) { g_cap = bytes; }

int stub_log_size(void);                                     /* stub_device.c: entries of its launch log */
/* entries of the launch log of stub_device.c in front of the call, and the stream it was queued on */
int stub_temporal_at(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].at : -1; }
const void* stub_temporal_stream(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].stream : NULL; }

static int note(int kind, const void* st, const sgmd_temporal_params* p, size_t streams, size_t steps, size_t pixels, const void* maps, const void* conf,
                const void* hv, const void* hb, const void* stats)
{
    if (g_calls_n < TP_LOG_MAX) {
        const void* ptr[5] = {maps, conf, hv, hb, stats};
        g_calls[g_calls_n].kind = kind;
        g_calls[g_calls_n].at = stub_log_size();
        g_calls[g_calls_n].stream = st;
        if (p) g_calls[g_calls_n].p = *p;
        g_calls[g_calls_n].streams = streams; g_calls[g_calls_n].steps = steps; g_calls[g_calls_n].pixels = pixels;
        memcpy(g_calls[g_calls_n++].ptr, ptr, sizeof ptr);
    }
    return (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) ? 719 : 0;
}

static uint32_t bits_of(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static float float_of(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
static int finite_bits(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }
static int popcount8(unsigned v) { int n = 0; for (; v; v >>= 1) n += (int)(v & 1u); return n; }

/* one step of one pixel (include/sgm_mi355x.h): the output's bits; *hv and *hb become hv' and hb', *cls the decision */
static uint32_t step(const sgmd_temporal_params* p, uint32_t x, int conf_ok, uint32_t* hv, uint8_t* hb, int* cls)
{
    const int valid = finite_bits(x) && conf_ok, hfin = finite_bits(*hv);
    uint32_t out;
    if (valid && !hfin) { *cls = 0; out = x; }
    else if (valid) {
        const float xf = float_of(x), hf = float_of(*hv);
        float d = xf - hf;
        if (d < 0) d = -d;
        if (d <= p->delta) {
            const float ax = p->a * xf, bh = p->b * hf;
            *cls = 1;
            out = bits_of(ax + bh);
        } else { *cls = 2; out = x; }
    }
    else if (p->n > 0 && hfin && popcount8(*hb & ((1u << p->n) - 1u)) >= p->k) { *cls = 3; out = *hv; }
    else { *cls = 4; out = 0x7F800000u; }
    *hb = (uint8_t)(((unsigned)*hb << 1 | (unsigned)valid) & 0xFFu);
    if (finite_bits(out)) *hv = out;
    else if (*hb == 0) *hv = 0x7F800000u;
    return out;
}

size_t sgmd_temporal_scratch_bytes(void) { return 4096; }     /* (deliberately not the kernel's: the host takes whatever the device says) */

int sgmd_temporal(int o, void* st, const sgmd_temporal_params* p, size_t streams, size_t steps, size_t pixels, void* maps, const void* conf,
                  void* hist_value, void* hist_bits, void* stats, void* scratch)
{
    (void)o;
    if (stats && scratch) memset(scratch, 0xA5, sgmd_temporal_scratch_bytes());         /* as the kernel: the scratch is written */
    const int rc = note(0, st, p, streams, steps, pixels, maps, conf, hist_value, hist_bits, stats);
    if (rc != 0) return rc;
    if (streams * steps * pixels * sizeof(float) > g_cap) return 0;
    uint32_t* m = (uint32_t*)maps;
    const uint16_t* k = (const uint16_t*)conf;
    uint32_t* hv = (uint32_t*)hist_value;
    uint8_t* hb = (uint8_t*)hist_bits;
    uint32_t* cnt = (uint32_t*)stats;
    if (cnt) memset(cnt, 0, streams * steps * 5 * sizeof(uint32_t));
    for (size_t s = 0; s < streams; ++s)
        for (size_t t = 0; t < steps; ++t)
            for (size_t i = 0; i < pixels; ++i) {
                const size_t at = (s * steps + t) * pixels + i;
                int cls;
                /* the four bytes of a map or history value may sit at any 4-byte boundary of the caller's, nothing more */
                m[at] = step(p, m[at], !k || p->min_conf == 0 || k[at] >= p->min_conf, &hv[s * pixels + i], &hb[s * pixels + i], &cls);
                if (cnt) ++cnt[(s * steps + t) * 5 + (size_t)cls];
            }
    return 0;
}

int sgmd_temporal_clear(int o, void* st, size_t count, void* hist_value, void* hist_bits)
{
    (void)o;
    const int rc = note(1, st, NULL, 0, 0, count, NULL, NULL, hist_value, hist_bits, NULL);
    if (rc != 0) return rc;
    if (count * sizeof(float) > g_cap) return 0;
    for (size_t i = 0; i < count; ++i) ((uint32_t*)hist_value)[i] = 0x7F800000u;
    memset(hist_bits, 0, count);
    return 0;
}
