/* TEST INFRASTRUCTURE (tests/test_host_call_trace.py, tests/record_host_call_trace.py): drives one build of the product's C host
 * (csrc/sgm_host.c) on the stand-in device (tests/stub_device.c) through a fixed list of scenarios.
 *
 *   host_trace_driver trace    every scenario once; prints, as JSON, the unfiltered log of device calls of every step (names and
 *                              arguments; the confidence / refinement launches with the owner of their confidence map; the post
 *                              pass -- speckle, median, lrcheck*, fill_*, d2d, memset, remap -- with the ROLE of every map and
 *                              scratch buffer it is handed: "caller" / "caller_r" for the driver's own output buffers, else
 *                              "dev<k>[+<bytes>]" = the k-th device allocation (0-based, the k-th "alloc" entry) of the
 *                              scenario, the instance being opaque here.  A post pass handed the wrong scratch set shows).
 *                              A step is "init" (create / initialize / reset / destroy) or "frame" (everything a match does).
 *   host_trace_driver refuse   every scenario once per allocation it performs, with that allocation refused: the step that meets
 *                              it must return false, a reset at the same shape must then succeed, and the instance is destroyed
 *                              (the caller runs this mode under the sanitizers).  Reports each refusal on stderr, in line with the
 *                              library's own messages.
 */
#include "../include/sgm_mi355x.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void stub_clear(void);
int stub_log_size(void);
const char* stub_log_name(int i);
int stub_log_arg(int i);
void stub_fail_alloc_at(int nth);
int stub_alloc_count(void);
const void* stub_log_ptr(int i, int second);
float stub_log_float(int i);

void stub_set_pinned(int slot, const void* p);
void stub_remap_clear(void);

/* W2 x H2: a map of 300 KiB (handed over in two pieces); B4 frames of W4 x H4: one of 4.1 MiB (four pieces, each above what the
 * stand-in copies for real: its device memory is capped) */
enum { WA = 48, HA = 20, WB = 70, HB = 33, WT = 48, HT = 40, W2 = 320, H2 = 240, W4 = 640, H4 = 424, B4 = 4, MAXPX = B4 * W4 * H4 };
static uint8_t g_img[MAXPX];
static float g_out[MAXPX], g_out_r[4 * 70 * 40];
static uint16_t g_conf[W2 * H2];
static uint8_t g_rows[4 * 3 * 70 * 320];

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

/* ---- the run ---- */
static int g_refuse;                 /* mode */
static const char* g_scenario;
static int g_first_step;
static sgm_instance* g_s;            /* the scenario's instance (NULL: the default instance behind SGM_*) */
static int g_w, g_h;                 /* the shape and options of its last initialize: what the recovery resets to */
static SGMOption g_opt;
static int g_allocs_before;          /* stub_alloc_count() when the scenario began */
static int g_refused;                /* refuse mode: a step has met the refused allocation (the scenario ends there) */

static const char* whose(const void* p) { return p == NULL ? "none" : (p == (const void*)g_conf ? "caller" : "internal"); }


/* ---- notes beside the stand-in's log.  The launchers below are linked with -Wl,--wrap=<name> (tests/record_host_call_trace.py):
 * the host's call lands in __wrap_<name>, which notes the roles of the pointers and calls the stand-in's own launcher.  A note with
 * a name is an entry of its own (launchers the stand-in does not log: fill_*, remap, census_sym; the driver's read_stage answers),
 * printed in front of log entry `at`; one without a name adds its roles to log entry `at`. ---- */
#define ROLE_LEN 40
typedef struct { int at; const char* name; int arg, n; char role[4][ROLE_LEN]; } side_note;
static side_note g_notes[4096];
static int g_notes_n;
static struct { const char* p; size_t bytes; int k; } g_live[256];          /* device allocations alive, k = ordinal in the scenario */
static int g_live_n, g_alloc_k;

static void role_of(const void* p, char* out)
{
    const char* c = (const char*)p;
    int best = -1;
    if (!p) { snprintf(out, ROLE_LEN, "none"); return; }
    if (c >= (const char*)g_out && c < (const char*)g_out + sizeof g_out) { snprintf(out, ROLE_LEN, "caller"); return; }
    if (c >= (const char*)g_out_r && c < (const char*)g_out_r + sizeof g_out_r) { snprintf(out, ROLE_LEN, "caller_r"); return; }
    if (c >= (const char*)g_img && c < (const char*)g_img + sizeof g_img) { snprintf(out, ROLE_LEN, "image"); return; }
    for (int i = 0; i < g_live_n; ++i)              /* (the stand-in caps what it really allocates: the nearest base below wins) */
        if (c >= g_live[i].p && c < g_live[i].p + g_live[i].bytes && (best < 0 || g_live[i].p > g_live[best].p)) best = i;
    if (best < 0) snprintf(out, ROLE_LEN, "other");
    else if (c == g_live[best].p) snprintf(out, ROLE_LEN, "dev%d", g_live[best].k);
    else snprintf(out, ROLE_LEN, "dev%d+%zu", g_live[best].k, (size_t)(c - g_live[best].p));
}

static void side(const char* name, int arg, const void* a, const void* b, const void* c, const void* d, int n)
{
    if (g_refuse || g_notes_n >= (int)(sizeof g_notes / sizeof g_notes[0])) return;
    side_note* s = &g_notes[g_notes_n++];
    const void* p[4] = {a, b, c, d};
    s->at = stub_log_size(); s->name = name; s->arg = arg; s->n = n;
    for (int i = 0; i < n; ++i) role_of(p[i], s->role[i]);
}

int __real_sgmd_alloc(int o, void** p, size_t n);
int __wrap_sgmd_alloc(int o, void** p, size_t n)
{
    const int rc = __real_sgmd_alloc(o, p, n), k = g_alloc_k++;
    if (rc == 0 && g_live_n < (int)(sizeof g_live / sizeof g_live[0])) { g_live[g_live_n].p = (const char*)*p; g_live[g_live_n].bytes = n ? n : 1; g_live[g_live_n++].k = k; }
    return rc;
}
int __real_sgmd_free(int o, void* p);
int __wrap_sgmd_free(int o, void* p)
{
    for (int i = 0; p && i < g_live_n; ++i)
        if (g_live[i].p == (const char*)p) { g_live[i] = g_live[--g_live_n]; break; }
    return __real_sgmd_free(o, p);
}
int __real_sgmd_speckle(int o, void* st, const void* g, void* d, float diff, unsigned area, void* a, void* b, void* c);
int __wrap_sgmd_speckle(int o, void* st, const void* g, void* d, float diff, unsigned area, void* a, void* b, void* c)
{ side(NULL, 0, d, a, b, c, 4); return __real_sgmd_speckle(o, st, g, d, diff, area, a, b, c); }
int __real_sgmd_median(int o, void* st, const void* g, void* d, void* s, void* status);
int __wrap_sgmd_median(int o, void* st, const void* g, void* d, void* s, void* status)
{ side(NULL, 0, d, s, NULL, NULL, 2); return __real_sgmd_median(o, st, g, d, s, status); }
int __real_sgmd_lrcheck(int o, void* st, const void* g, void* dl, const void* dr, float th);
int __wrap_sgmd_lrcheck(int o, void* st, const void* g, void* dl, const void* dr, float th)
{ side(NULL, 0, dl, dr, NULL, NULL, 2); return __real_sgmd_lrcheck(o, st, g, dl, dr, th); }
int __real_sgmd_lrcheck_right(int o, void* st, const void* g, const void* dr, const void* dl, float th, int chk, void* out);
int __wrap_sgmd_lrcheck_right(int o, void* st, const void* g, const void* dr, const void* dl, float th, int chk, void* out)
{ side(NULL, 0, dr, dl, out, NULL, 3); return __real_sgmd_lrcheck_right(o, st, g, dr, dl, th, chk, out); }
int __real_sgmd_d2d_async(int o, void* st, void* d, const void* s, size_t n);
int __wrap_sgmd_d2d_async(int o, void* st, void* d, const void* s, size_t n)
{ side(NULL, 0, d, s, NULL, NULL, 2); return __real_sgmd_d2d_async(o, st, d, s, n); }
int __real_sgmd_fill_classify(int o, void* st, const void* g, const void* ref, const void* oth, float th, int right, int chk, void* cls);
int __wrap_sgmd_fill_classify(int o, void* st, const void* g, const void* ref, const void* oth, float th, int right, int chk, void* cls)
{ side("fill_classify", right | (chk << 1), ref, oth, cls, NULL, 3); return __real_sgmd_fill_classify(o, st, g, ref, oth, th, right, chk, cls); }
int __real_sgmd_fill_pass(int o, void* st, const void* g, int R, const void* in, void* out, const void* cls, int pass);
int __wrap_sgmd_fill_pass(int o, void* st, const void* g, int R, const void* in, void* out, const void* cls, int pass)
{ side("fill_pass", pass, in, out, cls, NULL, 3); return __real_sgmd_fill_pass(o, st, g, R, in, out, cls, pass); }
int __real_sgmd_remap(int o, void* st, const void* g, const void* maps, const void* l, const void* r, void* ol, void* orr);
int __wrap_sgmd_remap(int o, void* st, const void* g, const void* maps, const void* l, const void* r, void* ol, void* orr)
{ side("remap", 0, l, r, ol, orr, 4); return __real_sgmd_remap(o, st, g, maps, l, r, ol, orr); }
/* the symmetric census, which the stand-in lacks (a host linked with the stand-in alone refuses that kind) */
int sgmd_census_sym(int o, void* st, const void* g, int cw, int ch, const void* l, const void* r, void* cl, void* cr, const void* need)
{ (void)o; (void)st; (void)g; side("census_sym", cw * 100 + ch, l, r, need, NULL, 3); (void)cl; (void)cr; return 0; }

static void print_note(const side_note* s, int first)
{
    printf("%s[\"%s\", %d", first ? "" : ", ", s->name, s->arg);
    for (int k = 0; k < s->n; ++k) printf(", \"%s\"", s->role[k]);
    printf("]");
}

static void flush_step(const char* path, const char* what)
{
    const int n = stub_log_size();
    if (!g_refuse) {
        printf("%s\n    {\"path\": \"%s\", \"call\": \"%s\", \"log\": [", g_first_step ? "" : ",", path, what);
        g_first_step = 0;
        /* the confidence launchers with whose map they write, the refinement with whose confidence it reads and its L_t[0] */
        int printed = 0, j = 0;
        for (int i = 0; i < n; ++i) {
            const char* name = stub_log_name(i);
            char role[ROLE_LEN];
            for (; j < g_notes_n && g_notes[j].at <= i && g_notes[j].name; ++j) print_note(&g_notes[j], !printed++);
            printf("%s[\"%s\", %d", printed++ ? ", " : "", name, stub_log_arg(i));
            if (j < g_notes_n && g_notes[j].at == i) {
                for (int k = 0; k < g_notes[j].n; ++k) printf(", \"%s\"", g_notes[j].role[k]);
                ++j;
            } else if (strcmp(name, "lrcheck_both") == 0) {
                role_of(stub_log_ptr(i, 0), role); printf(", \"%s\"", role);
                role_of(stub_log_ptr(i, 1), role); printf(", \"%s\"", role);
            } else if (strcmp(name, "memset") == 0) { role_of(stub_log_ptr(i, 0), role); printf(", \"%s\"", role); }
            if (strcmp(name, "refine_pass") == 0) printf(", \"%s\", \"%.9g\"", whose(stub_log_ptr(i, 0)), (double)stub_log_float(i));
            else if (strstr(name, "_conf")) printf(", \"%s\"", whose(stub_log_ptr(i, 0)));
            printf("]");
        }
        for (; j < g_notes_n; ++j)
            if (g_notes[j].name) print_note(&g_notes[j], !printed++);
        printf("]}");
    }
    g_notes_n = 0;
    stub_clear();
    stub_remap_clear();
}

/* a step of a scenario: in refuse mode a false answer is the refused allocation showing */
#define STEP(path, expr)                                                                                  \
    do {                                                                                                  \
        const bool ok_ = (expr);                                                                          \
        flush_step(path, #expr);                                                                          \
        if (!ok_) {                                                                                       \
            if (!g_refuse) { fprintf(stderr, "host_trace_driver: %s: %s failed\n", g_scenario, #expr); return 1; } \
            fprintf(stderr, "REFUSED %s: %s\n", g_scenario, #expr);                                       \
            g_refused = 1;                                                                                \
            return 0;                                                                                     \
        }                                                                                                 \
    } while (0)

static bool init(int w, int h, const SGMOption* o, bool reset)
{
    g_w = w; g_h = h; g_opt = *o;
    return reset ? sgm_reset(g_s, (uint16_t)w, (uint16_t)h, o) : sgm_initialize(g_s, (uint16_t)w, (uint16_t)h, o);
}
#define INIT(w, h, o) init(w, h, o, false)
#define RESET(w, h, o) init(w, h, o, true)
#define MATCH() sgm_match(g_s, g_img, g_img, g_out)
#define MATCH_DEVICE() (sgm_match_device(g_s, g_img, g_img, g_out) && sgm_synchronize(g_s))

static bool fresh(void)
{
    g_s = sgm_create(0);
    stub_clear();
    return g_s != NULL;
}

static int first_initialize(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    return 0;
}

static int reset_same_shape(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("init", RESET(WA, HA, &o));
    STEP("frame", MATCH());
    return 0;
}

static int reset_larger_smaller(void)
{
    const SGMOption o = options(16), p = options(40);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("init", RESET(WB, HB, &p));
    STEP("frame", MATCH());
    STEP("init", RESET(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("init", RESET(WB, HB, &o));
    STEP("frame", MATCH());
    STEP("init", RESET(WT, HT, &o));                 /* fewer pixels, more rows: the path tables are replaced */
    STEP("frame", MATCH());
    return 0;
}

static int batch_1_to_4(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("init", sgm_set_batch(g_s, 4) && RESET(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    return 0;
}

static int range_300(void)
{
    const SGMOption o = options(300);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    return 0;
}

static int match_without_reset(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    STEP("frame", MATCH_DEVICE());
    STEP("init", RESET(WA, HA, &o));
    STEP("frame", MATCH());
    return 0;
}

static int keep_stages(void)
{
    const SGMOption o = options(16);
    sgm_keep_stages(g_s, 1);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    return 0;
}

static int census_7x7(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_census_window(g_s, 7, 7) && INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    return 0;
}

static int fill_holes(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_fill_holes(g_s, 1) && INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", sgm_fill_holes(g_s, g_out, NULL) && sgm_synchronize(g_s));
    STEP("init", RESET(WB, HB, &o));
    STEP("frame", MATCH());
    return 0;
}

static int refine(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_refine(g_s, 1, 64.0f, 8.0f, 2, 0) && INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", sgm_match_confidence_device(g_s, g_img, g_img, g_out, g_conf) && sgm_synchronize(g_s));
    STEP("frame", MATCH_DEVICE());
    STEP("frame", sgm_match_confidence(g_s, g_img, g_img, g_out, g_conf));
    STEP("init", RESET(WB, HB, &o));
    STEP("frame", MATCH());
    return 0;
}

static int standalone_refinement(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", sgm_set_refine(g_s, 1, 64.0f, 8.0f, 1, 1) && sgm_refine_disparity(g_s, g_out, g_conf, g_img) && sgm_synchronize(g_s));
    return 0;
}

static int confidence_host_pointers(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", sgm_match_confidence(g_s, g_img, g_img, g_out, g_conf));
    STEP("frame", sgm_match_confidence(g_s, g_img, g_img, g_out, g_conf));
    STEP("frame", MATCH());
    STEP("init", RESET(WB, HB, &o));
    STEP("frame", sgm_match_confidence(g_s, g_img, g_img, g_out, g_conf));
    return 0;
}

static int match_planes(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", sgm_match_planes(g_s, g_img, 1000.f, 100.f, 0.f, g_out));
    STEP("frame", sgm_match_planes(g_s, g_img, 1000.f, 100.f, 0.f, g_out));
    return 0;
}

static int row_tile(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_rows(g_s, 7, 13) && INIT(WA, HA, &o));
    for (int frame = 0; frame < 2; ++frame) {
        STEP("frame", sgm_tile_begin(g_s, g_img, g_img));
        for (int fwd = 1; fwd >= 0; --fwd) {
            STEP("frame", sgm_tile_import_boundary(g_s, fwd, g_rows));
            STEP("frame", sgm_tile_sweep(g_s, fwd));
            STEP("frame", sgm_tile_export_boundary(g_s, fwd, g_rows));
        }
        STEP("frame", sgm_tile_finish(g_s, g_out) && sgm_tile_post(g_s, g_out) && sgm_synchronize(g_s));
    }
    return 0;
}

static int overlap_post(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_overlap_post(g_s, 1) && INIT(WA, HA, &o));
    STEP("frame", sgm_match_async(g_s, g_img, g_img, g_out));
    STEP("frame", sgm_match_async(g_s, g_img, g_img, g_out));
    STEP("frame", sgm_match_wait(g_s));
    STEP("frame", sgm_match_planes(g_s, g_img, 1000.f, 100.f, 0.f, g_out));
    return 0;
}

static int stage_cus(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_stage_cus(g_s, SGM_STAGE_SUM, 0, 8) && sgm_set_stage_cus(g_s, SGM_STAGE_POST, 8, 8) && INIT(WA, HA, &o));
    STEP("frame", sgm_match_async(g_s, g_img, g_img, g_out));
    STEP("frame", sgm_match_async(g_s, g_img, g_img, g_out));     /* no reset: S on a cost sum with a stream of its own */
    STEP("frame", sgm_match_wait(g_s));
    return 0;
}

static int fused_last_sweep(void)              /* SGM_UPSUM=1 is in the environment of this scenario's sgm_create */
{
    const SGMOption o = options(128);
    STEP("init", sgm_set_batch(g_s, 2) && INIT(WB, HB, &o));
    STEP("frame", MATCH());
    STEP("frame", sgm_fused_sweep_rows(g_s) > 0);
    STEP("frame", MATCH());                                       /* no reset: the three upward planes are re-created */
    STEP("init", RESET(WB, HB, &o));
    STEP("frame", MATCH());
    return 0;
}

#define MATCH_BOTH() sgm_match_both(g_s, g_img, g_img, g_out, g_out_r)

static int both_pageable(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH_BOTH());
    STEP("frame", MATCH_BOTH());                                  /* no reset: nothing new is allocated, S accumulates once */
    STEP("frame", MATCH());
    STEP("init", RESET(WB, HB, &o));
    STEP("frame", MATCH_BOTH());
    return 0;
}

static int both_left_pinned_right_staged(void)
{
    const SGMOption o = options(16);
    stub_set_pinned(0, g_out);                                    /* (run_scenario unpins it) */
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH_BOTH());
    STEP("frame", sgm_match_both_async(g_s, g_img, g_img, g_out, g_out_r));
    STEP("frame", sgm_match_both_async(g_s, g_img, g_img, g_out, g_out_r));
    STEP("frame", sgm_match_wait(g_s));
    return 0;
}

static int both_device(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", sgm_match_both_device(g_s, g_img, g_img, g_out, g_out_r) && sgm_synchronize(g_s));
    STEP("frame", sgm_match_both_device(g_s, g_img, g_img, g_out, g_out_r) && sgm_synchronize(g_s));
    STEP("frame", MATCH_BOTH());                                  /* the right map's staging comes with the first host form */
    return 0;
}

static int both_keep_stages(void)
{
    const SGMOption o = options(16);
    sgm_keep_stages(g_s, 1);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH_BOTH());
    STEP("frame", MATCH_BOTH());
    return 0;
}

static int result_in_two_pieces(void)
{
    const SGMOption o = options(16);
    STEP("init", INIT(W2, H2, &o));
    STEP("frame", sgm_match_async(g_s, g_img, g_img, g_out));
    STEP("frame", sgm_match_wait(g_s));
    STEP("frame", sgm_match_async(g_s, g_img, g_img, g_out));
    STEP("frame", sgm_match_planes_async(g_s, g_img, 1000.f, 100.f, 0.f, g_out));    /* waits for the pieces itself; comes back whole */
    STEP("frame", sgm_match_wait(g_s));
    STEP("frame", sgm_match_confidence(g_s, g_img, g_img, g_out, g_conf));  /* the map in pieces, the confidence behind it */
    return 0;
}

static int result_in_four_pieces(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_batch(g_s, B4) && INIT(W4, H4, &o));
    STEP("frame", sgm_match_async(g_s, g_img, g_img, g_out));
    STEP("frame", sgm_match_wait(g_s));
    STEP("frame", MATCH());
    return 0;
}

/* ---- scenarios for the paths sgm_host.c's cost-sum state, post pass and stage read-back go through ---- */

/* sgm_read_stage of every id the header documents (and two it does not): each answer is an entry of the step's log.  S (stage 3)
 * exists on every initialized instance: a 0 there is the refused allocation showing */
static bool read_stage_ids(const int* ids, size_t n)
{
    bool ok = true;
    for (size_t i = 0; i < n; ++i) {
        const size_t got = sgm_read_stage(g_s, ids[i], g_out, sizeof g_out);
        if (ids[i] == 3 && got == 0) ok = false;
        side("read_stage", ids[i], NULL, NULL, NULL, NULL, 1);
        if (!g_refuse) snprintf(g_notes[g_notes_n - 1].role[0], ROLE_LEN, "%zu bytes", got);
    }
    return ok;
}
static bool read_stages(void)
{
    static const int ids[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 26, 27, 28, 29};
    return read_stage_ids(ids, sizeof ids / sizeof ids[0]);
}
/* ... but the planes: those of the shapes with 128 disparities are beyond what the stand-in allocates for real */
static bool read_stages_but_planes(void)
{
    static const int ids[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 18, 19, 20, 26, 27, 28};
    return read_stage_ids(ids, sizeof ids / sizeof ids[0]);
}
#define READ_S() (sgm_read_stage(g_s, 3, g_out, sizeof g_out) == (size_t)g_w * g_h * 2 * (size_t)(g_opt.max_disparity - g_opt.min_disparity))

static bool tile_frame(void)
{
    bool ok = sgm_tile_begin(g_s, g_img, g_img);
    for (int fwd = 1; ok && fwd >= 0; --fwd) {
        sgm_tile_import_boundary(g_s, fwd, g_rows);              /* (false at a frame edge) */
        ok = sgm_tile_sweep(g_s, fwd) && (sgm_tile_export_boundary(g_s, fwd, g_rows), true);
    }
    return ok && sgm_tile_finish(g_s, g_out) && sgm_tile_post(g_s, g_out) && sgm_synchronize(g_s);
}

static int right_view(void)
{
    SGMOption o = options(16);
    sgm_set_reference_view(g_s, 1);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    o.is_check_lr = false;
    STEP("init", RESET(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH_DEVICE());
    return 0;
}

static int right_view_batch_2(void)
{
    const SGMOption o = options(16);
    sgm_set_reference_view(g_s, 1);
    STEP("init", sgm_set_batch(g_s, 2) && INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    return 0;
}

static int right_view_row_tile(void)
{
    SGMOption o = options(16);
    sgm_set_reference_view(g_s, 1);
    STEP("init", sgm_set_batch(g_s, 2) && sgm_set_rows(g_s, 7, 13) && INIT(WA, HA, &o));
    STEP("frame", tile_frame());
    STEP("frame", tile_frame());                                  /* no reset */
    STEP("frame", read_stages());                                 /* the planes have storage for the tile's rows */
    o.is_check_lr = false;
    STEP("init", RESET(WA, HA, &o));
    STEP("frame", tile_frame());
    return 0;
}

static int tall_frame(void)                    /* W < H with 8 paths: the diagonal planes are cleared before the aggregation */
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_batch(g_s, 2) && INIT(HA, WA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    STEP("init", sgm_set_rows(g_s, 7, 13) && RESET(HA, WA, &o));
    STEP("frame", tile_frame());
    STEP("frame", tile_frame());
    return 0;
}

static float g_map_x[WA * HA], g_map_y[WA * HA];
static int rectified(void)
{
    const SGMOption o = options(16);
    for (int i = 0; i < WA * HA; ++i) { g_map_x[i] = (float)(i % WA) + 0.25f; g_map_y[i] = (float)(i / WA); }
    STEP("init", sgm_set_rectify(g_s, WA, HA, g_map_x, g_map_y, g_map_x, g_map_y) && INIT(WA, HA, &o));
    STEP("frame", read_stages());                                 /* before any match */
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    STEP("init", RESET(WA, HA, &o));                              /* unchanged maps: nothing is uploaded */
    STEP("frame", MATCH_DEVICE());
    STEP("init", sgm_set_rectify(g_s, 0, 0, NULL, NULL, NULL, NULL) && RESET(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    return 0;
}

static int census_symmetric(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_census_kind(g_s, SGM_CENSUS_SYMMETRIC) && INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    STEP("init", sgm_set_census_window(g_s, 7, 7) && RESET(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    STEP("init", sgm_set_rows(g_s, 7, 13) && RESET(WA, HA, &o));
    STEP("frame", tile_frame());
    return 0;
}

static int fused_sweep_then_read_S(void)       /* SGM_UPSUM=1 */
{
    const SGMOption o = options(128);
    STEP("init", sgm_set_batch(g_s, 2) && INIT(WB, HB, &o));
    STEP("frame", MATCH());
    STEP("frame", sgm_fused_sweep_rows(g_s) > 0 && READ_S());     /* re-creates the three upward planes, then sums */
    STEP("frame", READ_S());                                      /* nothing pending any more */
    STEP("frame", MATCH() && sgm_fused_sweep_rows(g_s) == 0);     /* no reset: adds to the S that was read */
    STEP("frame", MATCH());
    STEP("frame", read_stages_but_planes());
    return 0;
}

static int fused_sweep_then_keep_stages(void)  /* SGM_UPSUM=1 */
{
    const SGMOption o = options(128);
    STEP("init", sgm_set_batch(g_s, 2) && INIT(WB, HB, &o));
    STEP("frame", MATCH());
    sgm_keep_stages(g_s, 1);
    STEP("frame", MATCH() && sgm_fused_sweep_rows(g_s) == 0);     /* no reset */
    STEP("frame", read_stages_but_planes());
    sgm_keep_stages(g_s, 0);
    STEP("init", RESET(WB, HB, &o));
    STEP("frame", MATCH() && sgm_fused_sweep_rows(g_s) > 0);
    STEP("frame", sgm_match_confidence(g_s, g_img, g_img, g_out, g_conf) && sgm_fused_sweep_rows(g_s) == 0);
    return 0;
}

static int three_matches_then_read_S(void)     /* S pending (replacing), pending (adding), stored by the read; also with SGM_FUSED_WTA=0 */
{
    const SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    STEP("frame", MATCH());
    STEP("frame", READ_S());
    STEP("frame", READ_S());
    STEP("frame", MATCH());
    STEP("init", RESET(WA, HA, &o));
    STEP("frame", READ_S());                                      /* S of no match at all */
    STEP("frame", MATCH());
    return 0;
}

static int both_overlap_post(void)
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_overlap_post(g_s, 1) && INIT(WA, HA, &o));
    STEP("frame", MATCH_BOTH());
    STEP("frame", sgm_match_both_async(g_s, g_img, g_img, g_out, g_out_r));
    STEP("frame", sgm_match_both_async(g_s, g_img, g_img, g_out, g_out_r));
    STEP("frame", sgm_match_wait(g_s));
    STEP("frame", MATCH());
    STEP("frame", sgm_match_both_device(g_s, g_img, g_img, g_out, g_out_r) && sgm_synchronize(g_s));
    return 0;
}

static int read_stages_plain(void)
{
    SGMOption o = options(16);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", read_stages());                                 /* before any match */
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    STEP("frame", MATCH());
    sgm_set_honor_num_paths(g_s, 1);
    o.num_paths = 4;
    STEP("init", RESET(WA, HA, &o));                              /* four paths: stages 14 .. 17 do not exist */
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    return 0;
}

static int read_stages_kept_and_filled(void)
{
    const SGMOption o = options(16);
    sgm_keep_stages(g_s, 1);
    STEP("init", sgm_set_fill_holes(g_s, 1) && sgm_set_batch(g_s, 2) && INIT(WA, HA, &o));
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    sgm_select_frame(g_s, 1);
    STEP("frame", read_stages());
    sgm_keep_stages(g_s, 0);
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    return 0;
}

static int read_stages_both(void)
{
    const SGMOption o = options(16);
    sgm_keep_stages(g_s, 1);
    STEP("init", INIT(WA, HA, &o));
    STEP("frame", MATCH_BOTH());
    STEP("frame", read_stages());
    STEP("frame", MATCH());                                       /* another kind of match: stages 26 .. 28 are gone */
    STEP("frame", read_stages());
    sgm_keep_stages(g_s, 0);
    STEP("frame", MATCH_BOTH());                                  /* not kept: 28 alone */
    STEP("frame", read_stages());
    sgm_keep_stages(g_s, 1);
    STEP("frame", read_stages());                                 /* switched on behind the match: its snapshots are not this match's */
    return 0;
}

static int read_stages_wide_census(void)       /* the cost volume exists without sgm_keep_stages */
{
    const SGMOption o = options(16);
    STEP("init", sgm_set_census_window(g_s, 7, 7) && INIT(WA, HA, &o));
    STEP("frame", read_stages());
    STEP("frame", MATCH());
    STEP("frame", read_stages());
    return 0;
}

static bool default_init(int w, int h, const SGMOption* o)
{
    g_w = w; g_h = h; g_opt = *o;
    return SGM_Initialize((uint16_t)w, (uint16_t)h, o);
}

static int default_instance(void)              /* g_s == NULL; its sgm_create happens inside the first SGM_Initialize */
{
    const SGMOption o = options(16);
    STEP("init", default_init(WA, HA, &o));
    STEP("frame", SGM_Match(g_img, g_img, g_out));
    STEP("init", default_init(WB, HB, &o));                       /* Q3: the census words of the first shape are carried over */
    STEP("frame", SGM_Match(g_img, g_img, g_out));
    STEP("frame", SGM_Match(g_img, g_img, g_out));
    return 0;
}

static const struct {
    const char* name;
    int (*run)(void);
    bool own_instance;
    const char* env;             /* set to env_value (NULL: "1") around the scenario's sgm_create */
    int skip;                    /* refuse mode: leading allocations that are not refused (the default instance's sgm_create) */
    const char* env_value;
} k_scenarios[] = {
    {"first_initialize", first_initialize, true, NULL, 0},
    {"reset_same_shape", reset_same_shape, true, NULL, 0},
    {"reset_larger_smaller", reset_larger_smaller, true, NULL, 0},
    {"batch_1_to_4", batch_1_to_4, true, NULL, 0},
    {"range_300", range_300, true, NULL, 0},
    {"match_without_reset", match_without_reset, true, NULL, 0},
    {"keep_stages", keep_stages, true, NULL, 0},
    {"census_7x7", census_7x7, true, NULL, 0},
    {"fill_holes", fill_holes, true, NULL, 0},
    {"refine", refine, true, NULL, 0},
    {"standalone_refinement", standalone_refinement, true, NULL, 0},
    {"confidence_host_pointers", confidence_host_pointers, true, NULL, 0},
    {"match_planes", match_planes, true, NULL, 0},
    {"row_tile", row_tile, true, NULL, 0},
    {"overlap_post", overlap_post, true, NULL, 0},
    {"stage_cus", stage_cus, true, NULL, 0},
    {"fused_last_sweep", fused_last_sweep, true, "SGM_UPSUM", 0},
    {"default_instance", default_instance, false, NULL, 1},
    {"both_pageable", both_pageable, true, NULL, 0},
    {"both_left_pinned_right_staged", both_left_pinned_right_staged, true, NULL, 0},
    {"both_device", both_device, true, NULL, 0},
    {"both_keep_stages", both_keep_stages, true, NULL, 0},
    {"result_in_two_pieces", result_in_two_pieces, true, NULL, 0},
    {"result_in_four_pieces", result_in_four_pieces, true, NULL, 0},
    {"right_view", right_view, true, NULL, 0},
    {"right_view_batch_2", right_view_batch_2, true, NULL, 0},
    {"right_view_row_tile", right_view_row_tile, true, NULL, 0},
    {"tall_frame", tall_frame, true, NULL, 0},
    {"rectified", rectified, true, NULL, 0},
    {"census_symmetric", census_symmetric, true, NULL, 0},
    {"fused_sweep_then_read_S", fused_sweep_then_read_S, true, "SGM_UPSUM", 0},
    {"fused_sweep_then_keep_stages", fused_sweep_then_keep_stages, true, "SGM_UPSUM", 0},
    {"three_matches_then_read_S", three_matches_then_read_S, true, NULL, 0},
    {"three_matches_then_read_S_unfused", three_matches_then_read_S, true, "SGM_FUSED_WTA", 0, "0"},
    {"both_overlap_post", both_overlap_post, true, NULL, 0},
    {"read_stages_plain", read_stages_plain, true, NULL, 0},
    {"read_stages_kept_and_filled", read_stages_kept_and_filled, true, NULL, 0},
    {"read_stages_both", read_stages_both, true, NULL, 0},
    {"read_stages_wide_census", read_stages_wide_census, true, NULL, 0},
};
#define N_SCENARIOS ((int)(sizeof k_scenarios / sizeof k_scenarios[0]))

/* one pass over scenario i; refuse_at >= 0: with that allocation (counted from the scenario's start) refused */
static int run_scenario(int i, int refuse_at)
{
    g_scenario = k_scenarios[i].name;
    g_refused = 0;
    g_s = NULL;
    g_live_n = g_alloc_k = 0;
    if (k_scenarios[i].env) setenv(k_scenarios[i].env, k_scenarios[i].env_value ? k_scenarios[i].env_value : "1", 1);
    g_allocs_before = stub_alloc_count();
    const bool made = !k_scenarios[i].own_instance || fresh();
    if (k_scenarios[i].env) unsetenv(k_scenarios[i].env);
    if (!made) return 1;
    stub_clear();
    if (k_scenarios[i].own_instance) g_allocs_before = stub_alloc_count();      /* else before the sgm_create inside the scenario */
    if (refuse_at >= 0) stub_fail_alloc_at(refuse_at);
    const int rc = k_scenarios[i].run();
    stub_set_pinned(0, NULL);
    if (rc != 0) return 1;
    if (refuse_at >= 0) {
        if (!g_refused) { fprintf(stderr, "host_trace_driver: %s: allocation %d was refused and no call failed\n", g_scenario, refuse_at); return 1; }
        stub_fail_alloc_at(-1);
        const bool again = g_s ? sgm_reset(g_s, (uint16_t)g_w, (uint16_t)g_h, &g_opt) : SGM_Reset((uint16_t)g_w, (uint16_t)g_h, &g_opt);
        fprintf(stderr, "RESET %s: %s\n", g_scenario, again ? "ok" : "failed");
        if (!again) return 1;
    }
    if (g_s) sgm_destroy(g_s);
    else SGM_Shutdown();
    flush_step("init", "destroy");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2 || (strcmp(argv[1], "trace") != 0 && strcmp(argv[1], "refuse") != 0)) {
        fprintf(stderr, "usage: host_trace_driver trace|refuse\n");
        return 2;
    }
    g_refuse = strcmp(argv[1], "refuse") == 0;
    setvbuf(stderr, NULL, _IONBF, 0);
    if (!g_refuse) printf("{");
    for (int i = 0; i < N_SCENARIOS; ++i) {
        if (!g_refuse) { printf("%s\n  \"%s\": [", i ? "," : "", k_scenarios[i].name); g_first_step = 1; }
        if (!g_refuse) {
            if (run_scenario(i, -1) != 0) return 1;
            printf("\n  ]");
            continue;
        }
        /* refuse mode: a clean pass counts the allocations, then one pass per allocation */
        if (run_scenario(i, -1) != 0) return 1;
        const int total = stub_alloc_count() - g_allocs_before;
        fprintf(stderr, "SCENARIO %s: %d allocations\n", k_scenarios[i].name, total);
        for (int k = k_scenarios[i].skip; k < total; ++k)
            if (run_scenario(i, k) != 0) return 1;
    }
    if (!g_refuse) printf("\n}\n");
    else printf("host_trace_driver ok\n");
    return 0;
}
