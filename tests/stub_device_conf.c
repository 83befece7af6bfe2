/*
 * stub_device_conf.c -- TEST INFRASTRUCTURE ONLY (tests/test_confidence_cpu.py).
 *
 * The confidence launchers of csrc/sgm_device.h (sgmd_sum_wta_conf, sgmd_sum_wta_lr_conf, sgmd_wta_right_conf) for the
 * stand-in device of tests/stub_device.c: they compute nothing and append their name, an argument the tests look at, the
 * confidence destination and their position in stub_device.c's log (stub_log_size() at the call) to a log of their own.
 * Linked with sgm_host.c and stub_device.c into a test-only library; sgm_host.c linked without it has no confidence.
 */
#include "sgm_device.h"

#include <stdio.h>

int stub_log_size(void);

#define CLOG_MAX 256
static char g_name[CLOG_MAX][32];
static int g_arg[CLOG_MAX], g_pos[CLOG_MAX];
static const void* g_dst[CLOG_MAX];
static int g_n;

void stubc_clear(void) { g_n = 0; }
int stubc_log_size(void) { return g_n; }
const char* stubc_log_name(int i) { return (i >= 0 && i < g_n) ? g_name[i] : ""; }
int stubc_log_arg(int i) { return (i >= 0 && i < g_n) ? g_arg[i] : -1; }
int stubc_log_pos(int i) { return (i >= 0 && i < g_n) ? g_pos[i] : -1; }
const void* stubc_log_dst(int i) { return (i >= 0 && i < g_n) ? g_dst[i] : NULL; }

static int note(const char* name, int arg, const void* dst)
{
    if (g_n < CLOG_MAX) {
        snprintf(g_name[g_n], sizeof g_name[g_n], "%s", name);
        g_arg[g_n] = arg;
        g_dst[g_n] = dst;
        g_pos[g_n] = stub_log_size();
        ++g_n;
    }
    return 0;
}

int sgmd_sum_wta_conf(int o, void* st, const sgmd_geom* g, int nd, const void* pl, size_t pb, const void* ex, const void* re,
                      const void* rc, int cap, int accumulate, void* S, int cu, float omr, void* dl, void* conf)
{ (void)o; (void)st; (void)g; (void)nd; (void)pl; (void)pb; (void)ex; (void)re; (void)rc; (void)cap; (void)S; (void)cu; (void)omr; (void)dl;
  return note("sum_wta_conf", accumulate, conf); }
int sgmd_sum_wta_lr_conf(int o, void* st, const sgmd_geom* g, int nd, const void* pl, size_t pb, const void* ex, const void* re,
                         const void* rc, int cap, int accumulate, int store_S, int do_right, void* S, int cu, float omr, void* dl,
                         void* dr, void* conf, int conf_right)
{ (void)o; (void)st; (void)g; (void)nd; (void)pl; (void)pb; (void)ex; (void)re; (void)rc; (void)cap; (void)S; (void)cu; (void)omr; (void)dl;
  (void)dr; return note("sum_wta_lr_conf", accumulate | (store_S << 1) | (do_right << 2) | (conf_right << 3), conf); }
int sgmd_wta_right_conf(int o, void* st, const sgmd_geom* g, const void* S, int cu, float omr, void* dr, void* conf)
{ (void)o; (void)st; (void)g; (void)S; (void)cu; (void)omr; (void)dr; return note("wta_right_conf", 0, conf); }
