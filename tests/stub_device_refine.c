/*
 * stub_device_refine.c -- TEST INFRASTRUCTURE ONLY (tests/test_refine_cpu.py).
 *
 * The refinement launcher of csrc/sgm_device.h (sgmd_refine_pass) for the stand-in device of tests/stub_device.c: it computes
 * nothing and appends its flags (vertical | first << 1 | last << 2 | keep_invalid << 3), the guide and confidence pointers, the
 * table's first entry and its position in stub_device.c's log (stub_log_size() at the call) to a log of its own.  Linked with
 * sgm_host.c, stub_device.c and stub_device_conf.c into a test-only library; sgm_host.c linked without it has no refinement.
 * The two hole-filling launchers are here as no-ops too, so that the host offers hole filling (and refuses the combination).
 */
#include "sgm_device.h"

int stub_log_size(void);

#define RLOG_MAX 256
static int g_flags[RLOG_MAX], g_pos[RLOG_MAX];
static const void *g_guide[RLOG_MAX], *g_conf[RLOG_MAX];
static float g_l0[RLOG_MAX];
static int g_n;

void stubr_clear(void) { g_n = 0; }
int stubr_log_size(void) { return g_n; }
int stubr_log_flags(int i) { return (i >= 0 && i < g_n) ? g_flags[i] : -1; }
int stubr_log_pos(int i) { return (i >= 0 && i < g_n) ? g_pos[i] : -1; }
const void* stubr_log_guide(int i) { return (i >= 0 && i < g_n) ? g_guide[i] : (const void*)0; }
const void* stubr_log_conf(int i) { return (i >= 0 && i < g_n) ? g_conf[i] : (const void*)0; }
float stubr_log_l0(int i) { return (i >= 0 && i < g_n) ? g_l0[i] : -1.0f; }

int sgmd_refine_pass(int o, void* st, const sgmd_geom* g, int vertical, const float* table, const void* guide, const void* disp,
                     const void* conf, void* U, void* V, void* Q, int first, int last, int keep_invalid, void* out)
{
    (void)o; (void)st; (void)g; (void)disp; (void)U; (void)V; (void)Q; (void)out;
    if (g_n < RLOG_MAX) {
        g_flags[g_n] = vertical | (first << 1) | (last << 2) | (keep_invalid << 3);
        g_guide[g_n] = guide;
        g_conf[g_n] = conf;
        g_l0[g_n] = table[0];
        g_pos[g_n] = stub_log_size();
        ++g_n;
    }
    return 0;
}

int sgmd_fill_classify(int o, void* st, const sgmd_geom* g, const void* ref, const void* oth, float th, int right, int chk, void* cls)
{ (void)o; (void)st; (void)g; (void)ref; (void)oth; (void)th; (void)right; (void)chk; (void)cls; return 0; }
int sgmd_fill_pass(int o, void* st, const sgmd_geom* g, int R, const void* in, void* out, const void* cls, int pass)
{ (void)o; (void)st; (void)g; (void)R; (void)in; (void)out; (void)cls; (void)pass; return 0; }
