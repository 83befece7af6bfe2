/*
 * stub_device_both.c -- TEST INFRASTRUCTURE ONLY (tests/test_match_both_cpu.py).
 *
 * The launchers behind sgm_match_both and sgm_depth_from_both (sgmd_lrcheck_both, sgmd_depth_both of csrc/sgm_device.h) for the
 * stand-in device of tests/stub_device.c.  They append their name, an argument the tests look at, their two map pointers and their
 * position in stub_device.c's log to a log of their own; sgmd_lrcheck_both also fills its outputs (1.0 left, 2.0 right, while the
 * maps fit the stand-in allocator's cap) so that the tests can follow the two maps to the caller's buffers.  Linked with
 * sgm_host.c and stub_device.c into a test-only library; sgm_host.c linked without it has no sgm_match_both.
 *
 * It also answers sgmd_host_is_pinned, which stub_device.c answers with "never": the tests compile stub_device.c with
 * -Dsgmd_host_is_pinned=<an unused name> and name here, with stubb_set_pinned, the host buffers that count as page-locked
 * (sgm_host_alloc), so that the pinned, the staged and the mixed hand-over of the two maps can be driven on the stand-in.
 */
#include "sgm_device.h"

#include <stdio.h>

int stub_log_size(void);

#define BLOG_MAX 256
static char g_name[BLOG_MAX][32];
static int g_arg[BLOG_MAX], g_pos[BLOG_MAX];
static const void *g_a[BLOG_MAX], *g_b[BLOG_MAX];
static int g_n;

void stubb_clear(void) { g_n = 0; }
int stubb_log_size(void) { return g_n; }
const char* stubb_log_name(int i) { return (i >= 0 && i < g_n) ? g_name[i] : ""; }
int stubb_log_arg(int i) { return (i >= 0 && i < g_n) ? g_arg[i] : -1; }
int stubb_log_pos(int i) { return (i >= 0 && i < g_n) ? g_pos[i] : -1; }
const void* stubb_log_left(int i) { return (i >= 0 && i < g_n) ? g_a[i] : NULL; }
const void* stubb_log_right(int i) { return (i >= 0 && i < g_n) ? g_b[i] : NULL; }

static int note(const char* name, int arg, const void* a, const void* b)
{
    if (g_n < BLOG_MAX) {
        snprintf(g_name[g_n], sizeof g_name[g_n], "%s", name);
        g_arg[g_n] = arg;
        g_a[g_n] = a;
        g_b[g_n] = b;
        g_pos[g_n] = stub_log_size();
        ++g_n;
    }
    return 0;
}

int sgmd_lrcheck_both(int o, void* st, const sgmd_geom* g, const void* dl, const void* dr, float th, int chk, void* out_l, void* out_r)
{
    (void)o; (void)st; (void)dl; (void)dr; (void)th;
    const size_t px = (size_t)g->B * g->W * g->H;
    if (2 * px * sizeof(float) <= (1u << 20))
        for (size_t i = 0; i < px; ++i) { ((float*)out_l)[i] = 1.0f; ((float*)out_r)[i] = 2.0f; }
    return note("lrcheck_both", chk | (g->B << 8), out_l, out_r);
}

int sgmd_depth_both(int o, void* st, const void* dl, const void* dr, size_t n, float fx_l, float fx_r, float b, float doffs, void* out)
{ (void)o; (void)st; (void)fx_l; (void)fx_r; (void)b; (void)doffs; (void)out; return note("depth_both", (int)n, dl, dr); }

#define PIN_MAX 8
static const void* g_pinned[PIN_MAX];
/* slot 0 .. PIN_MAX-1 <- a host buffer that counts as page-locked from now on (NULL: nothing) */
void stubb_set_pinned(int slot, const void* p) { if (slot >= 0 && slot < PIN_MAX) g_pinned[slot] = p; }
int sgmd_host_is_pinned(int o, const void* p, size_t n)
{
    (void)o; (void)n;
    for (int i = 0; i < PIN_MAX; ++i)
        if (p && g_pinned[i] == p) return 1;
    return 0;
}
