/* TEST INFRASTRUCTURE (tests/test_temporal_cpu.py): drives the temporal-filter entry points of the product's C host
 * (csrc/sgm_host.c) with the stub device layer (tests/stub_device.c) and the stand-in filter (tests/stub_temporal.c, which computes
 * for real) under AddressSanitizer / UBSan -- the filter alone on the caller's buffers with pixel counts that are no multiple of
 * four, with and without confidence and counters; a sequence of matches with the filter on across Reset, a batch change, a shape
 * change, sequence mode, kept stages and both views, with the history and the counters read back after each; refusals; a refused
 * launch; the default instance; and the lifetime of all of it.  A stand-alone program: nothing is loaded into another process.
 * Results are not checked here (tests/test_temporal_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "temporal_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

void stub_temporal_fail_at(int nth);
void stub_temporal_cap(size_t bytes);

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

static sgm_temporal_spec spec_of(int n, int k, int sequence, unsigned min_conf, int stats)
{
    const sgm_temporal_spec sp = {0.4f, 0.125f, n, k, sequence, min_conf, stats};
    return sp;
}

/* the filter alone on buffers of exactly the sizes the contract names */
static int run_filter(sgm_instance* s, size_t streams, size_t steps, size_t pixels, int with_conf, int with_stats)
{
    const size_t n = streams * steps * pixels, h = streams * pixels;
    float* maps = (float*)malloc(n * sizeof(float));
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* hv = (float*)malloc(h * sizeof(float));
    uint8_t* hb = (uint8_t*)malloc(h);
    uint32_t* stats = (uint32_t*)malloc(streams * steps * 5 * sizeof(uint32_t));
    CHECK(maps && conf && hv && hb && stats);
    const float special[] = {NAN, INFINITY, -INFINITY, -0.0f, 1e-40f, 3e38f, -3e38f, 0.125f};
    for (size_t i = 0; i < n; ++i) {
        maps[i] = (i % 7 == 3) ? special[(i / 7) % 8] : (float)(i % 97) * 0.25f;
        conf[i] = (uint16_t)(i * 7919u);
    }
    for (size_t i = 0; i < h; ++i) {
        hv[i] = (i % 5 == 0) ? special[i % 8] : (float)(i % 89) * 0.25f;
        hb[i] = (uint8_t)(i * 37u);
    }
    const sgm_temporal_spec sp = spec_of(3, 2, 0, with_conf ? 20000u : 0u, 0);
    CHECK(sgm_temporal_filter(s, &sp, streams, steps, pixels, maps, with_conf ? conf : NULL, hv, hb, with_stats ? stats : NULL));
    CHECK(sgm_temporal_clear(s, streams, pixels, hv, hb));
    CHECK(sgm_temporal_filter(s, &sp, streams, steps, pixels, maps, with_conf ? conf : NULL, hv, hb, with_stats ? stats : NULL));
    CHECK(sgm_synchronize(s));
    if (with_stats) {
        size_t total = 0;
        for (size_t i = 0; i < streams * steps * 5; ++i) total += stats[i];
        CHECK(total == n);
    }
    free(maps); free(conf); free(hv); free(hb); free(stats);
    return 0;
}

/* matches with the filter on: every read-back after every kind of match */
static int run_matches(sgm_instance* s, int w, int h, int batch, int sequence, unsigned min_conf)
{
    const size_t px = (size_t)w * h, n = px * batch;
    uint8_t* img = (uint8_t*)malloc(2 * n);
    float* disp = (float*)malloc(2 * n * sizeof(float));
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* frame = (float*)malloc(px * sizeof(float));
    uint8_t* bits = (uint8_t*)malloc(px);
    uint32_t* stats = (uint32_t*)malloc((size_t)2 * batch * 5 * sizeof(uint32_t));
    CHECK(img && disp && conf && frame && bits && stats);
    for (size_t i = 0; i < 2 * n; ++i) img[i] = (uint8_t)(i * 37u + (i >> 5));
    const SGMOption o = options(16);
    const sgm_temporal_spec sp = spec_of(3, 2, sequence, min_conf, 1);
    uint8_t *l = img, *r = img + n;
    CHECK(sgm_set_batch(s, batch) && sgm_set_temporal(s, &sp));
    for (int keep = 0; keep < 2; ++keep) {
        sgm_keep_stages(s, keep);
        for (int overlap = 0; overlap < 2; ++overlap) {
            CHECK(sgm_set_overlap_post(s, overlap));
            for (int k = 0; k < 2; ++k) {
                CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp));
                CHECK(sgm_temporal_stats(s, stats, batch) == batch && sgm_temporal_stats(s, stats, batch - 1) == 0);
                sgm_select_frame(s, batch - 1);
                CHECK(sgm_read_stage(s, 30, frame, px * sizeof(float)) == px * sizeof(float) && sgm_read_stage(s, 31, bits, px) == px);
                CHECK((sgm_read_stage(s, 29, frame, px * sizeof(float)) != 0) == (keep != 0));
                CHECK(sgm_read_stage(s, 33, frame, px * sizeof(float)) == 0);
            }
            CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_confidence(s, l, r, disp, conf));
            CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_async(s, l, r, disp) && sgm_temporal_restart(s) && sgm_match_wait(s));
            if (min_conf) {
                CHECK(!sgm_match_both(s, l, r, disp, disp + n));
                continue;
            }
            for (int k = 0; k < 2; ++k) {
                CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_both(s, l, r, disp, disp + n));
                CHECK(sgm_temporal_stats(s, stats, 2 * batch) == 2 * batch);
                for (int which = 30; which <= 34; ++which) {
                    if (which == 32 && !keep) continue;
                    const size_t bytes = (which == 31 || which == 34) ? px : px * sizeof(float);
                    CHECK(sgm_read_stage(s, which, which == 31 || which == 34 ? (void*)bits : (void*)frame, bytes) == bytes);
                }
            }
        }
    }
    /* a refused filter launch, a refused clear */
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o));
    stub_temporal_fail_at(0);
    CHECK(!sgm_match(s, l, r, disp) && sgm_match(s, l, r, disp));
    CHECK(sgm_temporal_restart(s));
    stub_temporal_fail_at(0);
    CHECK(!sgm_match(s, l, r, disp) && sgm_match(s, l, r, disp));
    CHECK(sgm_set_temporal(s, NULL) && sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp));
    CHECK(sgm_temporal_stats(s, stats, 2 * batch) == 0 && sgm_read_stage(s, 30, frame, px * sizeof(float)) == 0);
    free(img); free(disp); free(conf); free(frame); free(bits); free(stats);
    return 0;
}

int main(void)
{
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    /* streams, steps, pixels: one pixel; pixel counts that are no multiple of four; one that is */
    static const size_t shapes[][3] = {{1, 1, 1}, {1, 2, 3}, {2, 3, 777}, {3, 8, 2310}, {1, 8, 4096}, {5, 1, 5}};
    stub_temporal_cap((size_t)1 << 30);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        for (int variant = 0; variant < 4; ++variant)
            if (run_filter(s, shapes[i][0], shapes[i][1], shapes[i][2], variant & 1, variant >> 1) != 0) return 1;
    stub_temporal_cap((size_t)1 << 20);
    /* refusals queue nothing and touch nothing */
    {
        float m[4] = {1, 2, 3, 4}, hv[4] = {0};
        uint8_t hb[4] = {0};
        sgm_temporal_spec bad = spec_of(3, 2, 0, 0, 0);
        const sgm_temporal_spec good = bad;
        bad.alpha = 0.0f;
        CHECK(!sgm_temporal_filter(s, &bad, 1, 1, 4, m, NULL, hv, hb, NULL) && !sgm_set_temporal(s, &bad));
        bad = good; bad.hold_count = 4;
        CHECK(!sgm_temporal_filter(s, &bad, 1, 1, 4, m, NULL, hv, hb, NULL));
        CHECK(!sgm_temporal_filter(s, &good, 0, 1, 4, m, NULL, hv, hb, NULL) && !sgm_temporal_filter(s, &good, 1, 1, 4, NULL, NULL, hv, hb, NULL));
        CHECK(!sgm_temporal_filter(s, &good, (size_t)1 << 31, 2, 1, m, NULL, hv, hb, NULL));
        CHECK(!sgm_temporal_clear(s, 1, 0, hv, hb) && !sgm_temporal_clear(NULL, 1, 4, hv, hb));
        CHECK(m[0] == 1 && hv[0] == 0);
    }
    /* W, H, batch, sequence, min_conf: grow, a batch change in between, shrink, a frame that is no multiple of four pixels */
    static const int runs[][5] = {{24, 16, 1, 0, 0}, {24, 16, 3, 1, 0}, {24, 16, 1, 0, 0}, {70, 33, 2, 0, 20000}, {7, 9, 2, 1, 0}, {1, 1, 1, 0, 0}, {21, 31, 1, 1, 20000}};
    for (size_t i = 0; i < sizeof runs / sizeof runs[0]; ++i)
        if (run_matches(s, runs[i][0], runs[i][1], runs[i][2], runs[i][3], (unsigned)runs[i][4]) != 0) return 1;
    sgm_destroy(s);

    /* the default instance */
    {
        const int w = 12, h = 10;
        uint8_t img[12 * 10];
        float disp[12 * 10];
        uint32_t stats[5];
        memset(img, 100, sizeof img);
        const SGMOption o = options(8);
        const sgm_temporal_spec sp = spec_of(8, 8, 1, 0, 1);
        CHECK(!SGM_TemporalRestart() && SGM_TemporalStats(stats, 1) == 0);
        CHECK(SGM_SetTemporal(&sp));
        for (int k = 0; k < 3; ++k) CHECK(SGM_Reset((uint16_t)w, (uint16_t)h, &o) && SGM_Match(img, img, disp));
        CHECK(SGM_TemporalStats(stats, 1) == 1 && stats[1] == 120 && SGM_TemporalRestart());
        SGM_Shutdown();
        CHECK(SGM_Initialize((uint16_t)w, (uint16_t)h, &o) && SGM_Match(img, img, disp) && SGM_TemporalStats(stats, 1) == 1 && stats[0] == 120);
        CHECK(SGM_SetTemporal(NULL));
        SGM_Shutdown();
    }
    puts("temporal_sanitize_driver ok");
    return 0;
}
