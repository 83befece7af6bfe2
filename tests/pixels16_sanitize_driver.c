/* TEST INFRASTRUCTURE (tests/test_pixels16_cpu.py): drives the 16-bit front end of the product's C host (csrc/sgm_host.c) with the stub
 * device layer (tests/stub_device.c) and the stand-in launchers (tests/stub_pixels16.c and tests/stub_rectify.c, which compute for
 * real) under AddressSanitizer / UBSan -- the u16 uploads and device images exactly 2 * W * H bytes long, batches whose frames start
 * at odd samples, every census kind and window, the rectified u16 images, the narrowed images, one instance through 8 -> 12 -> 8
 * bits and through growing and shrinking shapes, the refusals, the default instance's remembered setting.  A stand-alone program:
 * nothing is loaded into another process.  Results are not checked here (tests/test_pixels16_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "pixels16_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_p16_count(void);
void stub_p16_fail_at(int nth);

static SGMOption options(int d, int dmin)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = (uint16_t)dmin; o.max_disparity = (uint16_t)(dmin + d);
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

/* every image is malloc'ed with exactly the bytes the host may touch: a read past 2 * n * batch (or n * batch with 8 bits) is caught */
static int run_shape(sgm_instance* s, int w, int h, int batch, int bits, int kind, int cw, int ch, int rectify)
{
    const size_t n = (size_t)w * h * batch, bpp = bits > 8 ? 2 : 1;
    uint8_t* l = (uint8_t*)malloc(n * bpp);
    uint8_t* r = (uint8_t*)malloc(n * bpp);
    uint8_t* ol = (uint8_t*)malloc(n * bpp);
    uint8_t* orr = (uint8_t*)malloc(n * bpp);
    float* disp = (float*)malloc(2 * n * sizeof(float));
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* m = (float*)malloc(2 * (size_t)w * h * sizeof(float));
    uint8_t* planes = (uint8_t*)malloc(6 * n);
    CHECK(l && r && ol && orr && disp && conf && m && planes);
    for (size_t i = 0; i < n * bpp; ++i) { l[i] = (uint8_t)(i * 37u + (i >> 5)); r[i] = (uint8_t)(i * 101u + (i >> 3)); }   /* samples >= 2^bits too */
    memset(planes, 50, 6 * n);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            m[(size_t)y * w + x] = (float)x + 0.4f * (float)((x + y) % 5) - 0.7f;          /* taps beyond every border */
            m[(size_t)w * h + (size_t)y * w + x] = (float)y - 0.3f * (float)(x % 4) + 0.6f;
        }
    const SGMOption o = options(16, 0);
    CHECK(sgm_set_batch(s, batch) && sgm_set_pixel_bits(s, bits) && sgm_set_census_kind(s, kind) && sgm_set_census_window(s, cw, ch));
    CHECK(rectify ? sgm_set_rectify(s, w, h, m, m + (size_t)w * h, m, m + (size_t)w * h) : sgm_set_rectify(s, 0, 0, NULL, NULL, NULL, NULL));
    CHECK(sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
    const int before = stub_p16_count();
    CHECK(sgm_match(s, l, r, disp));
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_confidence(s, l, r, disp, conf));
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_both(s, l, r, disp, disp + n));
    CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_device(s, l, r, disp) && sgm_synchronize(s));
    CHECK(sgm_match_device(s, l, r, disp) && sgm_synchronize(s));                       /* without Reset */
    CHECK(stub_p16_count() == before + (bits > 8 ? 5 * (1 + rectify) : (kind ? 5 : 0)));
    const size_t fpx = (size_t)w * h;
    if (bits > 8) {
        CHECK(sgm_read_stage(s, 21, ol, fpx) == fpx && sgm_read_stage(s, 22, ol, fpx) == fpx);
        CHECK(!sgm_match_planes(s, planes, 700.0f, 160.0f, 0.0f, disp));
        if (n > 1) CHECK(!sgm_match_device(s, l + 1, r, disp) && !sgm_match_device(s, l, r + 1, disp));   /* odd addresses */
        stub_p16_fail_at(0);                                                           /* a refused launch fails the match, no more */
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && !sgm_match(s, l, r, disp));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp));
    } else {
        CHECK(sgm_read_stage(s, 21, ol, fpx) == 0 && sgm_read_stage(s, 22, ol, fpx) == 0);
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_planes(s, planes, 700.0f, 160.0f, 0.0f, disp));
    }
    if (rectify) {
        CHECK(sgm_rectify(s, l, r, ol, orr) && sgm_synchronize(s));
        CHECK(sgm_read_stage(s, 19, ol, fpx * bpp) == fpx * bpp && sgm_read_stage(s, 20, ol, fpx * bpp) == fpx * bpp);
        CHECK(sgm_read_stage(s, 19, ol, fpx * bpp - 1) == 0);
    }
    free(l); free(r); free(ol); free(orr); free(disp); free(conf); free(m); free(planes);
    return 0;
}

int main(void)
{
    /* w, h, batch, bits, census kind, window, rectification */
    static const int runs[][8] = {
        {24, 16, 1, 8, 0, 5, 5, 0},  {24, 16, 1, 12, 0, 5, 5, 0}, {24, 16, 1, 8, 0, 5, 5, 0},     /* 8 -> 12 -> 8 at one shape */
        {7, 9, 3, 16, 1, 7, 7, 1},                                                                /* odd W * H: frame 1 at an odd sample */
        {70, 33, 2, 10, 0, 9, 7, 1}, {5, 9, 1, 12, 0, 5, 5, 0},  {1, 1, 1, 9, 1, 5, 5, 1},        /* grows; window does not fit; one pixel */
        {33, 33, 1, 12, 1, 9, 7, 0}, {20, 31, 2, 8, 0, 7, 7, 1}, {20, 31, 2, 13, 0, 7, 7, 1},     /* wide centre: 8 then 13 bits */
        {3, 1, 3, 16, 0, 1, 3, 0},   {64, 20, 1, 12, 0, 63, 1, 0}, {12, 70, 1, 12, 1, 1, 63, 0},
    };
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    CHECK(!sgm_set_pixel_bits(s, 7) && !sgm_set_pixel_bits(s, 17) && !sgm_set_pixel_bits(s, -1) && !sgm_set_pixel_bits(s, 0) &&
          !sgm_set_pixel_bits(NULL, 12));
    for (size_t i = 0; i < sizeof runs / sizeof runs[0]; ++i) {
        const int* q = runs[i];
        if (run_shape(s, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]) != 0) { fprintf(stderr, "run %zu\n", i); return 1; }
    }
    /* row tiles are refused with more than 8 bits, and come back with 8 */
    const SGMOption o = options(16, 0);
    CHECK(sgm_set_rectify(s, 0, 0, NULL, NULL, NULL, NULL) && sgm_set_batch(s, 1) && sgm_set_pixel_bits(s, 12) && sgm_set_rows(s, 4, 12));
    CHECK(!sgm_reset(s, 24, 16, &o) && !sgm_initialize(s, 24, 16, &o));
    CHECK(sgm_set_pixel_bits(s, 8) && sgm_reset(s, 24, 16, &o));
    sgm_destroy(s);

    /* the default instance: set before it exists, kept across a shutdown */
    enum { W = 12, H = 10 };
    uint16_t img[W * H];
    float disp[W * H];
    for (int i = 0; i < W * H; ++i) img[i] = (uint16_t)(i * 523);
    const SGMOption o8 = options(8, 0);
    CHECK(!SGM_SetPixelBits(17) && SGM_SetPixelBits(12));
    int before = stub_p16_count();
    CHECK(SGM_Initialize(W, H, &o8) && SGM_Match((const uint8_t*)img, (const uint8_t*)img, disp) && stub_p16_count() == before + 1);
    SGM_Shutdown();
    CHECK(SGM_Reset(W, H, &o8) && SGM_Match((const uint8_t*)img, (const uint8_t*)img, disp) && stub_p16_count() == before + 2);
    CHECK(sgm_compute((const uint8_t*)img, (const uint8_t*)img, W, H, &o8, disp) && stub_p16_count() == before + 3);
    CHECK(SGM_SetPixelBits(8));
    uint8_t img8[W * H];
    memset(img8, 9, sizeof img8);
    CHECK(SGM_Reset(W, H, &o8) && SGM_Match(img8, img8, disp) && stub_p16_count() == before + 3);
    SGM_Shutdown();
    puts("pixels16_sanitize_driver ok");
    return 0;
}
