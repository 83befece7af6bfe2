/* TEST INFRASTRUCTURE (tests/test_scaled_cpu.py): drives the scaled entry points of the product's C host (csrc/sgm_host.c) with the
 * stub device layer (tests/stub_device.c), the stand-in scale launchers (tests/stub_scale.c, which compute for real) and the
 * stand-in 16-bit census (tests/stub_pixels16.c) under AddressSanitizer / UBSan -- caller buffers of exactly the documented sizes
 * for shapes with and without remainders, both factors, every radius, 8 and 12 bits, the composed match in its host and device
 * forms across shapes that grow and shrink and batches, refusals, refused launches, the default instance, and the lifetime of all
 * of it.  A stand-alone program: nothing is loaded into another process.  Results are not checked here
 * (tests/test_scaled_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "scaled_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_scale_count(void);
void stub_scale_fail_at(int nth);
void stub_fail_at(const char* name, int nth);

static SGMOption options(int dmin, int dmax)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = (uint16_t)dmin; o.max_disparity = (uint16_t)dmax;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

static sgm_scale_spec spec_of(int w, int h, int frames, int f, int bits, int radius)
{
    const sgm_scale_spec sp = {w, h, frames, f, bits, radius, SGM_SCALE_DEFAULT_PENALTY, 2, 40};
    return sp;
}

/* the two stand-alone device forms on the caller's own buffers, each of exactly its documented size */
static int run_explicit(sgm_instance* s, int w, int h, int frames, int f, int bits, int radius, int right)
{
    const sgm_scale_spec sp = spec_of(w, h, frames, f, bits, radius);
    int ws = 0, hs = 0;
    CHECK(sgm_scaled_shape(&sp, &ws, &hs) && ws == w / f && hs == h / f);
    const size_t es = bits > 8 ? 2 : 1, n = (size_t)w * h * frames, m = (size_t)ws * hs * frames;
    unsigned char* full = (unsigned char*)malloc(n * es);
    unsigned char* small = (unsigned char*)malloc(m * es);
    float* d_small = (float*)malloc(m * sizeof(float));
    float* d_full = (float*)malloc(n * sizeof(float));
    uint32_t* cr = (uint32_t*)malloc(n * 4);
    uint32_t* co = (uint32_t*)malloc(n * 4);
    CHECK(full && small && d_small && d_full && cr && co);
    for (size_t i = 0; i < n * es; ++i) full[i] = (unsigned char)((i * 37u + 11u) >> (es == 2 && (i & 1) ? 4 : 0));
    const float special[] = {NAN, INFINITY, -INFINITY, -3.0f, 1e9f, -1e9f, 3e38f, 0.25f};
    for (size_t i = 0; i < m; ++i) d_small[i] = (i % 7 == 3) ? special[(i / 7) % 8] : (float)(i % 53) * 0.25f;
    for (size_t i = 0; i < n; ++i) { cr[i] = (uint32_t)(i * 2654435761u); co[i] = (uint32_t)((i + 5) * 40503u * 65537u); }
    CHECK(sgm_downscale(s, &sp, full, small));
    CHECK(sgm_upscale_disparity(s, &sp, d_small, small, full, radius < 0 ? NULL : cr, radius < 0 ? NULL : co, right, d_full));
    CHECK(sgm_synchronize(s));
    free(full); free(small); free(d_small); free(d_full); free(cr); free(co);
    return 0;
}

/* the composed match, host and device form, on an instance initialised for the low-resolution shape */
static int run_composed(sgm_instance* s, int w, int h, int batch, int f, int bits, int radius, int symmetric, int right)
{
    const sgm_scale_spec sp = spec_of(w, h, batch, f, bits, radius);
    int ws = 0, hs = 0;
    CHECK(sgm_scaled_shape(&sp, &ws, &hs));
    const SGMOption o = options(1, 12);
    CHECK(sgm_set_batch(s, batch) && sgm_set_pixel_bits(s, bits));
    CHECK(sgm_set_census_kind(s, symmetric ? SGM_CENSUS_SYMMETRIC : SGM_CENSUS_CENTRE) && sgm_set_census_window(s, symmetric ? 7 : 5, symmetric ? 7 : 5));
    sgm_set_reference_view(s, right);
    CHECK(sgm_reset(s, (uint16_t)ws, (uint16_t)hs, &o));
    const size_t es = bits > 8 ? 2 : 1, n = (size_t)w * h * batch;
    uint8_t* left = (uint8_t*)malloc(n * es);
    uint8_t* rightv = (uint8_t*)malloc(n * es);
    float* disp = (float*)malloc(n * sizeof(float));
    CHECK(left && rightv && disp);
    for (size_t i = 0; i < n * es; ++i) { left[i] = (uint8_t)(i * 13u >> (es == 2 && (i & 1) ? 4 : 0)); rightv[i] = (uint8_t)(left[i] ^ 5u); }
    CHECK(sgm_match_scaled(s, &sp, left, rightv, disp));
    CHECK(sgm_match_scaled_device(s, &sp, left, rightv, disp) && sgm_synchronize(s));
    /* a plain match of the small shape in between, then the scaled one again */
    float* small = (float*)malloc((size_t)ws * hs * batch * sizeof(float));
    CHECK(small && sgm_match(s, left, rightv, small));
    CHECK(sgm_match_scaled(s, &sp, left, rightv, disp));
    free(small); free(left); free(rightv); free(disp);
    return 0;
}

int main(void)
{
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    const int shapes[][2] = {{64, 16}, {67, 19}, {70, 23}, {5, 5}, {4, 4}, {9, 131}};
    for (size_t k = 0; k < sizeof shapes / sizeof shapes[0]; ++k)
        for (int f = 2; f <= 4; f += 2)
            for (int radius = -1; radius <= 4; ++radius) {
                const int w = shapes[k][0], h = shapes[k][1];
                if (w / f < 1 || h / f < 1) continue;
                CHECK(run_explicit(s, w, h, 1 + (int)(k % 3), f, (radius & 1) ? 12 : 8, radius, radius & 1) == 0);
            }
    /* shapes that grow and shrink, batches, both census kinds, both views, with and without the re-search */
    CHECK(run_composed(s, 96, 40, 1, 2, 8, 3, 0, 0) == 0);
    CHECK(run_composed(s, 131, 49, 2, 4, 8, 4, 0, 1) == 0);
    CHECK(run_composed(s, 70, 33, 3, 2, 12, 3, 1, 0) == 0);
    CHECK(run_composed(s, 40, 24, 1, 2, 12, 0, 0, 1) == 0);
    CHECK(run_composed(s, 96, 40, 2, 2, 8, -1, 1, 0) == 0);
    CHECK(run_composed(s, 96, 40, 2, 2, 8, 3, 0, 0) == 0);         /* the instance the rest works on: 48x20, batch 2, centre census */

    /* refusals: nothing is queued */
    const int before = stub_scale_count();
    sgm_scale_spec sp = spec_of(96, 40, 2, 2, 8, 3);
    uint8_t* img = (uint8_t*)calloc(96 * 40 * 2, 2);
    float* disp = (float*)malloc(96 * 40 * 2 * sizeof(float));
    CHECK(img && disp);
    CHECK(!sgm_match_scaled(s, NULL, img, img, disp) && !sgm_match_scaled(s, &sp, NULL, img, disp) && !sgm_match_scaled(NULL, &sp, img, img, disp));
    sp.factor = 3;
    CHECK(!sgm_match_scaled(s, &sp, img, img, disp) && !sgm_downscale(s, &sp, img, img));
    sp = spec_of(96, 40, 2, 2, 8, 5);
    CHECK(!sgm_match_scaled(s, &sp, img, img, disp));
    sp = spec_of(96, 40, 3, 2, 8, 3);                             /* another batch than the instance's */
    CHECK(!sgm_match_scaled(s, &sp, img, img, disp));
    sp = spec_of(96, 40, 2, 2, 8, 3);
    const SGMOption small_opt = options(1, 12);
    CHECK(sgm_set_rows(s, 4, 12) && sgm_reset(s, 48, 20, &small_opt) && !sgm_match_scaled(s, &sp, img, img, disp));
    CHECK(sgm_set_rows(s, 0, 0) && sgm_reset(s, 48, 20, &small_opt));
    CHECK(stub_scale_count() == before);
    CHECK(sgm_match_scaled(s, &sp, img, img, disp));

    /* a refused launch anywhere in the sequence fails the call and leaves the instance usable */
    for (int nth = 0; nth < 3; ++nth) {
        stub_scale_fail_at(nth);
        CHECK(!sgm_match_scaled(s, &sp, img, img, disp));
        stub_scale_fail_at(-1);
        CHECK(sgm_match_scaled(s, &sp, img, img, disp));
    }
    stub_fail_at("census", 1);                                    /* the full-resolution census (the small match's is call 0) */
    CHECK(!sgm_match_scaled_device(s, &sp, img, img, disp));
    CHECK(sgm_match_scaled_device(s, &sp, img, img, disp) && sgm_synchronize(s));
    stub_fail_at("aggregate", 0);
    CHECK(!sgm_match_scaled(s, &sp, img, img, disp));
    CHECK(sgm_match_scaled(s, &sp, img, img, disp));
    sgm_destroy(s);

    /* the default instance */
    const SGMOption o = options(0, 16);
    sp = spec_of(96, 40, 1, 4, 8, 3);
    CHECK(!SGM_MatchScaled(&sp, img, img, disp));
    CHECK(SGM_Initialize(24, 10, &o) && SGM_MatchScaled(&sp, img, img, disp));
    SGM_Shutdown();
    free(img); free(disp);
    printf("scaled_sanitize_driver ok\n");
    return 0;
}
