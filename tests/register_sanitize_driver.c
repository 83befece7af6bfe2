/* TEST INFRASTRUCTURE (tests/test_register_cpu.py): drives the registration entry points of the product's C host (csrc/sgm_host.c)
 * with the stub device layer (tests/stub_device.c) and the stand-in registration launchers (tests/stub_register.c, which compute
 * for real and use the key scratch the way the kernels do) under AddressSanitizer / UBSan -- the size of the key scratch for
 * targets with odd and even numbers of pixels, targets that grow and shrink and batches on one instance, both splats, maps with
 * special values, targets every point misses, the gather of every element size, the last match's map after every kind of match,
 * refusals, refused launches, sgm_register_spec_raw, and the lifetime of all of it.  A stand-alone program: nothing is loaded into
 * another process.  Results are not checked here (tests/test_register_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "register_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_register_count(void);
void stub_register_fail_at(int nth);

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

static sgm_cloud_spec source_of(int w, int h, int frames)
{
    const sgm_cloud_spec sp = {w, h, frames, 700.0f, 710.0f, (float)w / 2, (float)h / 2, 160.0f, 0.75f, 100.0f, 1000000.0f, 7};
    return sp;
}

/* a camera beside the source's: scaled to its own size, slightly turned and shifted, with distortion */
static sgm_register_spec target_of(int sw, int w, int h, int splat)
{
    sgm_register_spec t;
    memset(&t, 0, sizeof t);
    t.width = w; t.height = h;
    t.fx = 700.0f * (float)w / (float)sw; t.fy = 710.0f * (float)w / (float)sw; t.cx = (float)w / 2 + 0.2f; t.cy = (float)h / 2 - 0.3f;
    t.dist[0] = -0.08f; t.dist[1] = 0.02f; t.dist[2] = 0.001f; t.dist[3] = -0.001f; t.dist[4] = 0.003f;
    t.R[0] = 0.9994f; t.R[1] = -0.0349f; t.R[3] = 0.0349f; t.R[4] = 0.9994f; t.R[8] = 1.0f;
    t.t[0] = 5.0f; t.t[1] = -1.0f; t.t[2] = 0.5f;
    t.z_min = 0.0f; t.z_max = INFINITY;
    t.splat = splat;
    return t;
}

/* both entry points on the caller's own buffers: no instance shape involved */
static int run_explicit(sgm_instance* s, int w, int h, int frames, int tw, int th, int splat, int with_maps)
{
    const size_t n = (size_t)w * h * frames, tn = (size_t)tw * th * frames;
    float* disp = (float*)malloc(n * sizeof(float));
    uint8_t* mask = (uint8_t*)malloc(n);
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* depth = (float*)malloc(tn * sizeof(float));
    uint32_t* source = (uint32_t*)malloc(tn * sizeof(uint32_t));
    uint32_t* out = (uint32_t*)malloc(tn * sizeof(uint32_t));
    CHECK(disp && mask && conf && depth && source && out);
    const float special[] = {NAN, INFINITY, -INFINITY, -0.75f, -1.0f, 0.0f, 1e-38f, 3e38f};
    for (size_t i = 0; i < n; ++i) {
        disp[i] = (i % 11 == 3) ? special[(i / 11) % 8] : (float)(i % 97) * 0.5f;
        mask[i] = (uint8_t)(i % 5 != 0);
        conf[i] = (uint16_t)(i % 13);
    }
    const sgm_cloud_spec sp = source_of(w, h, frames);
    sgm_register_spec tg = target_of(w, tw, th, splat);
    CHECK(sgm_register_depth(s, &sp, &tg, disp, with_maps ? mask : NULL, with_maps ? conf : NULL, depth, with_maps ? source : NULL));
    CHECK(sgm_register_depth(s, &sp, &tg, disp, NULL, NULL, depth, source) && sgm_synchronize(s));
    /* every element size; the maps are the caller's buffers reread with another element */
    const uint32_t fill = 0xDEADBEEFu;
    CHECK(sgm_register_gather(s, &sp, &tg, source, 1, mask, &fill, out));
    CHECK(sgm_register_gather(s, &sp, &tg, source, 2, conf, &fill, out));
    CHECK(sgm_register_gather(s, &sp, &tg, source, 4, disp, &fill, out) && sgm_synchronize(s));
    /* a source buffer as a caller may leave it: words that name no pixel read nothing */
    for (size_t i = 0; i < tn; ++i) source[i] = (uint32_t)(i * 2654435761u);
    CHECK(sgm_register_gather(s, &sp, &tg, source, 4, disp, &fill, out) && sgm_synchronize(s));
    /* a target every point misses: behind the camera, and far off to the side */
    tg.R[8] = -1.0f;
    CHECK(sgm_register_depth(s, &sp, &tg, disp, NULL, NULL, depth, source));
    for (size_t i = 0; i < tn; ++i) CHECK(source[i] == 0xFFFFFFFFu);
    tg.R[8] = 1.0f; tg.cx = 1e9f;
    CHECK(sgm_register_depth(s, &sp, &tg, disp, NULL, NULL, depth, source));
    for (size_t i = 0; i < tn; ++i) CHECK(source[i] == 0xFFFFFFFFu);
    tg.cx = 3e38f; tg.fx = 3e38f;
    CHECK(sgm_register_depth(s, &sp, &tg, disp, NULL, NULL, depth, source) && sgm_synchronize(s));
    free(disp); free(mask); free(conf); free(depth); free(source); free(out);
    return 0;
}

/* the last match's map, after every kind of match */
static int run_instance(sgm_instance* s, int w, int h, int batch)
{
    const size_t n = (size_t)w * h * batch;
    uint8_t* img = (uint8_t*)malloc(2 * n);
    float* disp = (float*)malloc(2 * n * sizeof(float));
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* depth = (float*)malloc(n * sizeof(float));
    uint32_t* source = (uint32_t*)malloc(n * sizeof(uint32_t));
    CHECK(img && disp && conf && depth && source);
    for (size_t i = 0; i < 2 * n; ++i) img[i] = (uint8_t)(i * 37u + (i >> 5));
    const SGMOption o = options(16);
    const sgm_cloud_spec sp = source_of(w, h, batch);
    sgm_register_spec tg = target_of(w, w, h, 2);
    CHECK(sgm_set_batch(s, batch) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
    uint8_t *l = img, *r = img + n;
    for (int overlap = 0; overlap < 2; ++overlap) {
        CHECK(sgm_set_overlap_post(s, overlap));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp));
        CHECK(sgm_register_depth(s, &sp, &tg, NULL, NULL, NULL, depth, source) && sgm_synchronize(s));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_confidence(s, l, r, disp, conf));
        CHECK(sgm_register_depth(s, &sp, &tg, NULL, NULL, conf, depth, NULL) && sgm_synchronize(s));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_both(s, l, r, disp, disp + n));
        CHECK(sgm_register_depth(s, &sp, &tg, NULL, NULL, NULL, depth, source) && sgm_synchronize(s));
    }
    /* a spec of another shape; a refused launch leaves the instance usable */
    sgm_cloud_spec other = sp;
    other.width = w + 1;
    CHECK(!sgm_register_depth(s, &other, &tg, NULL, NULL, NULL, depth, source));
    stub_register_fail_at(0);
    CHECK(!sgm_register_depth(s, &sp, &tg, NULL, NULL, NULL, depth, source));
    CHECK(sgm_register_depth(s, &sp, &tg, NULL, NULL, NULL, depth, source) && sgm_synchronize(s));
    free(img); free(disp); free(conf); free(depth); free(source);
    return 0;
}

int main(void)
{
    /* source W, H, frames; target W, H: one pixel either side, odd and even numbers of keys, up- and downsampled, grow / shrink / grow */
    static const int shapes[][5] = {{1, 1, 1, 1, 1}, {20, 31, 1, 53, 29}, {70, 33, 3, 35, 17}, {64, 20, 2, 128, 40}, {37, 21, 1, 1, 29},
                                    {37, 21, 1, 53, 1}, {3, 1, 5, 3, 3}, {64, 32, 2, 1, 1}, {130, 40, 3, 131, 41}, {5, 5, 1, 7, 3}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        for (int k = 0; k < 4; ++k)
            if (run_explicit(s, shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], 1 + (k & 1), k >> 1) != 0) return 1;
    /* refusals queue nothing */
    {
        float d[4] = {1, 2, 3, 4}, depth[6];
        uint32_t source[6], fill = 0;
        const sgm_cloud_spec good = source_of(2, 2, 1);
        const sgm_register_spec tg = target_of(2, 3, 2, 1);
        const int before = stub_register_count();
        sgm_cloud_spec bad = good;
        bad.fx = 0.0f;
        CHECK(!sgm_register_depth(s, &bad, &tg, d, NULL, NULL, depth, source));
        sgm_register_spec t2 = tg;
        t2.splat = 3;
        CHECK(!sgm_register_depth(s, &good, &t2, d, NULL, NULL, depth, source));
        t2 = tg; t2.R[4] = NAN;
        CHECK(!sgm_register_depth(s, &good, &t2, d, NULL, NULL, depth, source));
        t2 = tg; t2.z_max = t2.z_min;
        CHECK(!sgm_register_depth(s, &good, &t2, d, NULL, NULL, depth, source));
        t2 = tg; t2.width = 65536;
        CHECK(!sgm_register_gather(s, &good, &t2, source, 4, d, &fill, depth));
        CHECK(!sgm_register_depth(NULL, &good, &tg, d, NULL, NULL, depth, source) && !sgm_register_depth(s, NULL, &tg, d, NULL, NULL, depth, source) &&
              !sgm_register_depth(s, &good, NULL, d, NULL, NULL, depth, source) && !sgm_register_depth(s, &good, &tg, d, NULL, NULL, NULL, source));
        CHECK(!sgm_register_depth(s, &good, &tg, d, NULL, NULL, d, source) && !sgm_register_depth(s, &good, &tg, d, NULL, NULL, depth, (uint32_t*)depth));
        CHECK(!sgm_register_gather(s, &good, &tg, source, 3, d, &fill, depth) && !sgm_register_gather(s, &good, &tg, source, 4, d, NULL, depth) &&
              !sgm_register_gather(s, &good, &tg, source, 4, d, &fill, d));
        CHECK(!sgm_register_depth(s, &good, &tg, NULL, NULL, NULL, depth, source));          /* no match yet: nothing to read */
        CHECK(stub_register_count() == before);
    }
    /* grow, shrink, batch: the instance's own map and keys */
    static const int inst[][3] = {{24, 16, 1}, {70, 33, 2}, {7, 9, 1}, {1, 1, 1}, {64, 32, 3}, {20, 31, 1}};
    for (size_t i = 0; i < sizeof inst / sizeof inst[0]; ++i)
        if (run_instance(s, inst[i][0], inst[i][1], inst[i][2]) != 0) return 1;
    sgm_destroy(s);

    /* the raw camera's spec */
    {
        const double K[9] = {70, 0, 34.5, 0, 70, 16, 0, 0, 1}, dist[5] = {-0.08, 0.02, 0.001, -0.001, 0};
        double R[9] = {0.9996573, -0.0261769, 0, 0.0261769, 0.9996573, 0, 0, 0, 1};
        sgm_register_spec out;
        CHECK(sgm_register_spec_raw(K, dist, R, 70, 33, 2, &out) && out.R[1] == (float)R[3] && out.R[3] == (float)R[1] && out.splat == 2);
        CHECK(!sgm_register_spec_raw(NULL, dist, R, 70, 33, 2, &out) && !sgm_register_spec_raw(K, dist, R, 70, 33, 2, NULL) &&
              !sgm_register_spec_raw(K, dist, R, 0, 33, 2, &out) && !sgm_register_spec_raw(K, dist, R, 70, 33, 0, &out));
        R[2] = NAN;
        CHECK(!sgm_register_spec_raw(K, dist, R, 70, 33, 2, &out));
    }
    puts("register_sanitize_driver ok");
    return 0;
}
