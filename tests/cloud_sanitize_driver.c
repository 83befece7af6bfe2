/* TEST INFRASTRUCTURE (tests/test_cloud_cpu.py): drives the point-cloud entry points of the product's C host (csrc/sgm_host.c) with
 * the stub device layer (tests/stub_device.c) and the stand-in cloud launchers (tests/stub_cloud.c, which compute for real and
 * write the tile scratch) under AddressSanitizer / UBSan -- the size of the tile scratch for shapes around the tile sizes, the
 * instance's own point and offset buffers across shapes that grow and shrink and batches, a capacity that is too small, the last
 * match's map after every kind of match, refusals, refused launches, the default instance, the valid mask of edge-valued maps, and
 * the lifetime of all of it.  A stand-alone program: nothing is loaded into another process.  Results are not checked here
 * (tests/test_cloud_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "cloud_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_cloud_count(void);
void stub_cloud_fail_at(int nth);

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

static sgm_cloud_spec spec_of(int w, int h, int frames)
{
    const sgm_cloud_spec sp = {w, h, frames, 700.0f, 710.0f, (float)w / 2, (float)h / 2, 160.0f, 0.75f, 100.0f, 1000000.0f, 7};
    return sp;
}

/* the two device forms on the caller's own buffers: no instance shape involved */
static int run_explicit(sgm_instance* s, int w, int h, int frames, int with_maps)
{
    const size_t n = (size_t)w * h * frames;
    float* disp = (float*)malloc(n * sizeof(float));
    uint8_t* mask = (uint8_t*)malloc(n);
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* xyz = (float*)malloc(3 * n * sizeof(float));
    sgm_point* pts = (sgm_point*)malloc(n * sizeof(sgm_point));
    uint32_t* off = (uint32_t*)malloc(((size_t)frames + 1) * sizeof(uint32_t));
    CHECK(disp && mask && conf && xyz && pts && off);
    const float special[] = {NAN, INFINITY, -INFINITY, -0.75f, -1.0f, 0.0f, 1e-38f, 3e38f};
    for (size_t i = 0; i < n; ++i) {
        disp[i] = (i % 11 == 3) ? special[(i / 11) % 8] : (float)(i % 97) * 0.5f;
        mask[i] = (uint8_t)(i % 5 != 0);
        conf[i] = (uint16_t)(i % 13);
    }
    const sgm_cloud_spec sp = spec_of(w, h, frames);
    CHECK(sgm_cloud_organized(s, &sp, disp, with_maps ? mask : NULL, with_maps ? conf : NULL, xyz));
    CHECK(sgm_cloud_points(s, &sp, disp, with_maps ? mask : NULL, with_maps ? conf : NULL, pts, off));
    CHECK(sgm_synchronize(s));
    CHECK(off[0] == 0 && off[frames] <= n);
    free(disp); free(mask); free(conf); free(xyz); free(pts); free(off);
    return 0;
}

/* the last match's map, after every kind of match, through the device forms and sgm_read_cloud */
static int run_instance(sgm_instance* s, int w, int h, int batch)
{
    const size_t n = (size_t)w * h * batch;
    uint8_t* img = (uint8_t*)malloc(2 * n);
    float* disp = (float*)malloc(2 * n * sizeof(float));
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* xyz = (float*)malloc(3 * n * sizeof(float));
    sgm_point* pts = (sgm_point*)malloc(n * sizeof(sgm_point));
    uint32_t* off = (uint32_t*)malloc(((size_t)batch + 1) * sizeof(uint32_t));
    CHECK(img && disp && conf && xyz && pts && off);
    for (size_t i = 0; i < 2 * n; ++i) img[i] = (uint8_t)(i * 37u + (i >> 5));
    const SGMOption o = options(16);
    const sgm_cloud_spec sp = spec_of(w, h, batch);
    CHECK(sgm_set_batch(s, batch) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
    uint8_t *l = img, *r = img + n;
    for (int overlap = 0; overlap < 2; ++overlap) {
        CHECK(sgm_set_overlap_post(s, overlap));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp));
        CHECK(sgm_cloud_organized(s, &sp, NULL, NULL, NULL, xyz) && sgm_cloud_points(s, &sp, NULL, NULL, NULL, pts, off) && sgm_synchronize(s));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_confidence(s, l, r, disp, conf));
        CHECK(sgm_cloud_points(s, &sp, NULL, NULL, conf, pts, off) && sgm_synchronize(s));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_both(s, l, r, disp, disp + n));
        /* the stand-in's maps hold d = 0 or 1: every pixel is kept with this spec's doffs */
        CHECK(!sgm_read_cloud(s, &sp, pts, n - 1, off) && off[batch] == n);
        CHECK(sgm_read_cloud(s, &sp, pts, n, off) && off[batch] == n && pts[n - 1].pixel == (((uint32_t)(h - 1) << 16) | (uint32_t)(w - 1)));
        CHECK(!sgm_read_cloud(s, &sp, NULL, 0, off) && off[batch] == n);
    }
    /* a spec of another shape; a refused launch */
    sgm_cloud_spec other = sp;
    other.width = w + 1;
    CHECK(!sgm_cloud_points(s, &other, NULL, NULL, NULL, pts, off) && !sgm_read_cloud(s, &other, pts, n, off));
    stub_cloud_fail_at(0);
    CHECK(!sgm_read_cloud(s, &sp, pts, n, off));
    stub_cloud_fail_at(0);
    CHECK(!sgm_cloud_organized(s, &sp, NULL, NULL, NULL, xyz));
    CHECK(sgm_read_cloud(s, &sp, pts, n, off));
    free(img); free(disp); free(conf); free(xyz); free(pts); free(off);
    return 0;
}

static int run_mask(int w, int h)
{
    const size_t n = (size_t)w * h;
    float* m = (float*)malloc(2 * n * sizeof(float));
    uint8_t* mask = (uint8_t*)malloc(n);
    CHECK(m && mask);
    const float edge[] = {NAN, INFINITY, -INFINITY, 1e9f, -1e9f, 32768.0f, -32768.0f, 32768.5f, -0.5f, -1.0f, (float)w - 1.0f,
                          (float)w - 1.5f, (float)w - 2.0f, (float)w, -1e-30f, 3.4e38f, -0.015625f, -0.016f};
    const int ne = (int)(sizeof edge / sizeof edge[0]);
    for (size_t i = 0; i < n; ++i) {
        m[i] = (float)(i % (size_t)w) + 0.25f;
        m[n + i] = (float)(i / (size_t)w) - 0.25f;
    }
    for (int i = 0; i < ne; ++i) {
        m[((size_t)i * 7) % n] = edge[i];
        m[n + ((size_t)i * 11 + 3) % n] = edge[ne - 1 - i];
    }
    CHECK(sgm_rectify_valid_mask(w, h, m, m + n, mask));
    for (size_t i = 0; i < n; ++i) CHECK(mask[i] <= 1);
    CHECK(!sgm_rectify_valid_mask(0, h, m, m + n, mask) && !sgm_rectify_valid_mask(w, -1, m, m + n, mask) &&
          !sgm_rectify_valid_mask(w, h, NULL, m + n, mask) && !sgm_rectify_valid_mask(w, h, m, NULL, mask) &&
          !sgm_rectify_valid_mask(w, h, m, m + n, NULL));
    free(m); free(mask);
    return 0;
}

int main(void)
{
    /* W, H, frames: one pixel, under one tile, around 2048 and 4096 pixels, frames that are not a multiple of four pixels */
    static const int shapes[][3] = {{1, 1, 1}, {20, 31, 1}, {70, 33, 1}, {64, 64, 1}, {241, 17, 1}, {130, 40, 3}, {3, 1, 5}, {2047, 1, 2},
                                    {2049, 1, 1}, {64, 32, 2}, {5, 5, 1}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        for (int with_maps = 0; with_maps < 2; ++with_maps)
            if (run_explicit(s, shapes[i][0], shapes[i][1], shapes[i][2], with_maps) != 0) return 1;
    /* refusals queue nothing */
    {
        float d[4] = {1, 2, 3, 4}, xyz[12];
        sgm_point pts[4];
        uint32_t off[2];
        const sgm_cloud_spec good = spec_of(2, 2, 1);
        const int before = stub_cloud_count();
        sgm_cloud_spec bad = good;
        bad.fx = 0.0f;
        CHECK(!sgm_cloud_organized(s, &bad, d, NULL, NULL, xyz) && !sgm_cloud_points(s, &bad, d, NULL, NULL, pts, off));
        bad = good; bad.z_max = bad.z_min;
        CHECK(!sgm_cloud_organized(s, &bad, d, NULL, NULL, xyz));
        bad = good; bad.frames = 0;
        CHECK(!sgm_cloud_points(s, &bad, d, NULL, NULL, pts, off));
        CHECK(!sgm_cloud_organized(NULL, &good, d, NULL, NULL, xyz) && !sgm_cloud_organized(s, NULL, d, NULL, NULL, xyz) &&
              !sgm_cloud_organized(s, &good, d, NULL, NULL, NULL) && !sgm_cloud_points(s, &good, d, NULL, NULL, NULL, off) &&
              !sgm_cloud_points(s, &good, d, NULL, NULL, pts, NULL));
        CHECK(!sgm_cloud_organized(s, &good, NULL, NULL, NULL, xyz));          /* no match yet: nothing to read */
        CHECK(stub_cloud_count() == before);
    }
    /* grow, shrink, batch: the instance's own buffers */
    static const int inst[][3] = {{24, 16, 1}, {70, 33, 2}, {7, 9, 1}, {1, 1, 1}, {64, 32, 3}, {20, 31, 1}};
    for (size_t i = 0; i < sizeof inst / sizeof inst[0]; ++i)
        if (run_instance(s, inst[i][0], inst[i][1], inst[i][2]) != 0) return 1;
    sgm_destroy(s);

    /* the default instance */
    {
        const int w = 12, h = 10;
        uint8_t img[12 * 10];
        float disp[12 * 10];
        sgm_point pts[12 * 10];
        uint32_t off[2] = {9, 9};
        memset(img, 100, sizeof img);
        const SGMOption o = options(8);
        const sgm_cloud_spec sp = spec_of(w, h, 1);
        CHECK(!SGM_ReadCloud(&sp, pts, 120, off));                          /* no default instance yet */
        CHECK(SGM_Initialize((uint16_t)w, (uint16_t)h, &o) && SGM_Match(img, img, disp));
        CHECK(SGM_ReadCloud(&sp, pts, 120, off) && off[1] == 120);
        SGM_Shutdown();
        CHECK(!SGM_ReadCloud(&sp, pts, 120, off));
    }
    static const int masks[][2] = {{1, 1}, {2, 2}, {7, 5}, {70, 33}};
    for (size_t i = 0; i < sizeof masks / sizeof masks[0]; ++i)
        if (run_mask(masks[i][0], masks[i][1]) != 0) return 1;
    puts("cloud_sanitize_driver ok");
    return 0;
}
