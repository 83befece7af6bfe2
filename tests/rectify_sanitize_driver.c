/* TEST INFRASTRUCTURE (tests/test_rectify_cpu.py): drives the rectification of the product's C host (csrc/sgm_host.c) with the stub
 * device layer (tests/stub_device.c) and the stand-in remap (tests/stub_rectify.c, which samples for real) under AddressSanitizer /
 * UBSan -- the quantisation of edge values, the size and lay-out of the map buffer, the rectified images of batches, shapes that
 * grow and shrink, maps replaced and turned off, the default instance's copy, and the lifetime of all of it.  A stand-alone
 * program: nothing is loaded into another process.  Results are not checked here (tests/test_rectify_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "rectify_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_remap_count(void);
void stub_remap_fail_at(int nth);

static SGMOption options(int d, int dmin)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = (uint16_t)dmin; o.max_disparity = (uint16_t)(dmin + d);
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

/* maps of a camera model, then sprinkled with the values the quantisation has to survive */
static int make_maps(int w, int h, float* mx, float* my)
{
    const double K[9] = {(double)w, 0, (w - 1) / 2.0, 0, (double)w, (h - 1) / 2.0, 0, 0, 1};
    const double Knew[9] = {0.7 * w, 0, (w - 1) / 2.0, 0, 0.7 * w, (h - 1) / 2.0, 0, 0, 1};
    const double dist[5] = {-0.3, 0.1, 0.01, -0.005, 0.0};
    const double c = cos(0.05), s = sin(0.05);
    const double R[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    CHECK(sgm_rectify_maps(K, dist, R, Knew, w, h, mx, my));
    const float edge[] = {NAN, INFINITY, -INFINITY, 1e9f, -1e9f, 32768.0f, -32768.0f, 32768.5f, -0.5f, -1.0f, (float)w - 1.0f,
                          (float)w - 0.5f, (float)w, -1e-30f, 3.4e38f};
    const int n = w * h, ne = (int)(sizeof edge / sizeof edge[0]);
    for (int i = 0; i < ne; ++i) {
        mx[(i * 7) % n] = edge[i];
        my[(i * 11 + 3) % n] = edge[ne - 1 - i];
    }
    mx[n - 1] = (float)w - 1.0f;                    /* the last pixel's taps: the last byte of the image and the three beyond it */
    my[n - 1] = (float)h - 1.0f;
    return 0;
}

static int run_shape(sgm_instance* s, int w, int h, int batch)
{
    const size_t n = (size_t)w * h;
    float* m = (float*)malloc(4 * n * sizeof(float));
    uint8_t* img = (uint8_t*)malloc(2 * n * batch);
    uint8_t* rect = (uint8_t*)malloc(2 * n * batch);
    float* disp = (float*)malloc(2 * n * batch * sizeof(float));
    uint16_t* conf = (uint16_t*)malloc(n * batch * sizeof(uint16_t));
    uint8_t* planes = (uint8_t*)malloc(6 * n * batch);
    CHECK(m && img && rect && disp && conf && planes);
    for (size_t i = 0; i < 2 * n * batch; ++i) img[i] = (uint8_t)(i * 37u + (i >> 5));
    memset(planes, 77, 6 * n * batch);
    CHECK(make_maps(w, h, m, m + n) == 0 && make_maps(w, h, m + 2 * n, m + 3 * n) == 0);
    const SGMOption o = options(16, 0);
    CHECK(sgm_set_batch(s, batch));
    CHECK(sgm_set_rectify(s, w, h, m, m + n, m + 2 * n, m + 3 * n));
    memset(m, 0xFF, 4 * n * sizeof(float));        /* the caller's arrays are not borrowed */
    CHECK(sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
    uint8_t *l = img, *r = img + n * batch;
    int before = stub_remap_count();
    CHECK(sgm_match(s, l, r, disp));
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_confidence(s, l, r, disp, conf));
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_both(s, l, r, disp, disp + n * batch));
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_device(s, l, r, disp) && sgm_synchronize(s));
    CHECK(sgm_match_device(s, l, r, disp) && sgm_synchronize(s));          /* without Reset */
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_planes(s, planes, 700.0f, 160.0f, 0.0f, disp));
    CHECK(stub_remap_count() == before + 6);
    CHECK(sgm_rectify(s, l, r, rect, rect + n * batch) && sgm_synchronize(s));
    CHECK(sgm_read_stage(s, 19, rect, n) == n && sgm_read_stage(s, 20, rect, n) == n);
    /* a refused remap fails the match and leaves the instance usable */
    stub_remap_fail_at(0);
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && !sgm_match(s, l, r, disp));
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp));
    /* maps of another shape: the reset is refused; off: the plain match */
    make_maps(w, h, m, m + n); make_maps(w, h, m + 2 * n, m + 3 * n);
    if (h > 1) {
        CHECK(sgm_set_rectify(s, w, h - 1, m, m + n, m + 2 * n, m + 3 * n));
        CHECK(!sgm_reset(s, (uint16_t)w, (uint16_t)h, &o));
    }
    CHECK(sgm_set_rectify(s, 0, 0, NULL, NULL, NULL, NULL));
    before = stub_remap_count();
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp) && stub_remap_count() == before);
    CHECK(!sgm_rectify(s, l, r, rect, rect + n * batch));
    CHECK(sgm_read_stage(s, 19, rect, n) == 0);
    free(m); free(img); free(rect); free(disp); free(conf); free(planes);
    return 0;
}

int main(void)
{
    static const int shapes[][3] = {{24, 16, 1}, {7, 9, 1}, {70, 33, 2}, {1, 1, 1}, {3, 1, 3}, {33, 33, 1}, {20, 31, 2}, {5, 5, 1}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    /* bad arguments change nothing */
    float one[4] = {0, 0, 0, 0};
    CHECK(!sgm_set_rectify(s, 2, 2, one, NULL, one, one) && !sgm_set_rectify(s, 0, 2, one, one, one, one) &&
          !sgm_set_rectify(s, 2, -1, one, one, one, one) && !sgm_set_rectify(NULL, 2, 2, one, one, one, one));
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        if (run_shape(s, shapes[i][0], shapes[i][1], shapes[i][2]) != 0) return 1;
    /* destroyed with maps set */
    CHECK(sgm_set_rectify(s, 2, 2, one, one, one, one));
    sgm_destroy(s);

    /* the default instance: maps set before it exists, kept across a shutdown, replaced, turned off */
    const int w = 12, h = 10;
    float m[4 * 12 * 10];
    uint8_t img[12 * 10];
    float disp[12 * 10];
    memset(img, 100, sizeof img);
    CHECK(make_maps(w, h, m, m + w * h) == 0 && make_maps(w, h, m + 2 * w * h, m + 3 * w * h) == 0);
    const SGMOption o = options(8, 0);
    CHECK(SGM_SetRectify(w, h, m, m + w * h, m + 2 * w * h, m + 3 * w * h));
    int before = stub_remap_count();
    CHECK(SGM_Initialize((uint16_t)w, (uint16_t)h, &o) && SGM_Match(img, img, disp) && stub_remap_count() == before + 1);
    SGM_Shutdown();
    CHECK(SGM_Reset((uint16_t)w, (uint16_t)h, &o) && SGM_Match(img, img, disp) && stub_remap_count() == before + 2);
    CHECK(SGM_SetRectify(w, h, m + 2 * w * h, m + 3 * w * h, m, m + w * h));
    CHECK(SGM_Reset((uint16_t)w, (uint16_t)h, &o) && SGM_Match(img, img, disp) && stub_remap_count() == before + 3);
    CHECK(SGM_SetRectify(0, 0, NULL, NULL, NULL, NULL));
    CHECK(SGM_Reset((uint16_t)w, (uint16_t)h, &o) && SGM_Match(img, img, disp) && stub_remap_count() == before + 3);
    CHECK(SGM_SetRectify(w, h, m, m + w * h, m + 2 * w * h, m + 3 * w * h));
    SGM_Shutdown();
    CHECK(SGM_SetRectify(0, 0, NULL, NULL, NULL, NULL));     /* frees the remembered copy */

    /* the map builder's refusals */
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z3[9] = {0}, d0[5] = {0};
    CHECK(!sgm_rectify_maps(I3, d0, I3, Z3, 2, 2, m, m + 4) && !sgm_rectify_maps(I3, d0, I3, I3, 0, 2, m, m + 4) &&
          !sgm_rectify_maps(NULL, d0, I3, I3, 2, 2, m, m + 4) && !sgm_rectify_maps(I3, d0, I3, I3, 2, 2, m, NULL));
    puts("rectify_sanitize_driver ok");
    return 0;
}
