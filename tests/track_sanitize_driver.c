/* TEST INFRASTRUCTURE (tests/test_track_cpu.py): drives sgm_track_sums, sgm_track, sgm_track_solve and sgm_track_world_pose of the
 * product's C host (csrc/sgm_host.c) with the stub device layer (tests/stub_device.c) and the stand-in launcher (tests/stub_track.c,
 * which computes for real) under AddressSanitizer / UBSan -- sources of one pixel, of one row and of one column, models of another
 * size, batches up to the 64 frames a call takes, with and without the side maps, maps full of non-finite and huge entries, poses
 * that throw every pixel out, every number of rounds, with and without traces, behind a match with and without the post pass on a
 * stream of its own, refusals, a refused launch, and the lifetime of all of it.  A stand-alone program: nothing is loaded into
 * another process.  Results are not checked here (tests/test_track_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "track_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_track_count(void);
void stub_track_fail_at(int nth);

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

/* fb = 40: a disparity near 20 is a depth near 2 */
static sgm_cloud_spec source_of(int w, int h, int frames)
{
    const float fx = 40.0f * (float)(w > h ? w : h) / 70.0f;
    const sgm_cloud_spec sp = {w, h, frames, fx, fx, (float)(w - 1) / 2, (float)(h - 1) / 2, 40.0f / fx, 0.0f, 0.1f, 1000.0f, 3};
    return sp;
}

static sgm_track_spec model_of(int w, int h, int iterations)
{
    const float fx = 40.0f * (float)(w > h ? w : h) / 70.0f;
    const sgm_track_spec m = {w, h, fx, fx, (float)(w - 1) / 2, (float)(h - 1) / 2, 0.3f, 4.0f, iterations, 6, 1e-9f};
    return m;
}

static void poses_of(double* p, int frames)
{
    for (int f = 0; f < frames; ++f) {
        const double a = 0.01 * (double)(f % 7), c = cos(a), s = sin(a);
        const double pose[12] = {c, 0, s, 0, 1, 0, -s, 0, c, 0.01 * (double)(f % 3), -0.01, 0.002 * (double)(f % 5)};
        memcpy(p + 12 * f, pose, sizeof pose);
    }
}

static int run(sgm_instance* s, int w, int h, int mw, int mh, int frames)
{
    const size_t px = (size_t)w * h * frames, mpx = (size_t)mw * mh * frames;
    float* disp = (float*)malloc(px * sizeof(float));
    uint8_t* mask = (uint8_t*)malloc(px);
    uint16_t* conf = (uint16_t*)malloc(px * sizeof(uint16_t));
    float* depth = (float*)malloc(mpx * sizeof(float));
    float* normal = (float*)malloc(3 * mpx * sizeof(float));
    double* poses = (double*)malloc((size_t)frames * 12 * sizeof(double));
    float* poses32 = (float*)malloc((size_t)frames * 12 * sizeof(float));
    int64_t* sums = (int64_t*)malloc((size_t)frames * 29 * sizeof(int64_t));
    sgm_track_stats* stats = (sgm_track_stats*)malloc((size_t)frames * sizeof(sgm_track_stats));
    int64_t* trace_sums = (int64_t*)malloc((size_t)64 * frames * 29 * sizeof(int64_t));
    double* trace_poses = (double*)malloc((size_t)65 * frames * 12 * sizeof(double));
    CHECK(disp && mask && conf && depth && normal && poses && poses32 && sums && stats && trace_sums && trace_poses);
    /* a slanted wall near Z = 2 with a step, a model wall with tilted normals */
    for (size_t i = 0; i < px; ++i) {
        disp[i] = 19.0f + (float)(i % 53) * 0.04f + (i % 11 == 0 ? 0.8f : 0.0f);
        mask[i] = (uint8_t)(i % 7 != 0);
        conf[i] = (uint16_t)(i % 9);
    }
    for (size_t i = 0; i < mpx; ++i) {
        depth[i] = 2.0f + (float)(i % 31) * 0.004f;
        normal[3 * i] = 0.1f * (float)((int)(i % 5) - 2); normal[3 * i + 1] = 0.05f * (float)((int)(i % 3) - 1); normal[3 * i + 2] = -0.97f;
    }
    const sgm_cloud_spec sp = source_of(w, h, frames);
    poses_of(poses, frames);
    for (int i = 0; i < 12 * frames; ++i) poses32[i] = (float)poses[i];
    sgm_track_spec m = model_of(mw, mh, 1);
    CHECK(sgm_track_sums(s, &sp, &m, poses32, disp, mask, conf, depth, normal, sums));
    CHECK(sgm_track_sums(s, &sp, &m, poses32, disp, NULL, NULL, depth, normal, sums) && sgm_synchronize(s));
    static const int rounds[] = {1, 2, 5, 64};
    for (size_t k = 0; k < sizeof rounds / sizeof rounds[0]; ++k) {
        m.iterations = rounds[k];
        poses_of(poses, frames);
        CHECK(sgm_track(s, &sp, &m, poses, disp, mask, conf, depth, normal, stats, trace_sums, trace_poses));
        CHECK(sgm_track(s, &sp, &m, poses, disp, NULL, conf, depth, normal, stats, NULL, trace_poses));
        CHECK(sgm_track(s, &sp, &m, poses, disp, mask, NULL, depth, normal, stats, trace_sums, NULL));
    }
    /* every step of the solve by hand, then the pose for the volume */
    for (int f = 0; f < frames; ++f) {
        double next[12];
        float world[12];
        const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        CHECK(sgm_track_solve(&m, sums + 29 * f, poses + 12 * f, next, &stats[f]));
        CHECK(sgm_track_world_pose(identity, next, world));
    }
    /* maps as a caller may leave them: non-finite and huge entries, a gate and a span at the ends of float, poses that look away */
    for (size_t i = 0; i < px; i += 3) disp[i] = i % 2 ? INFINITY : NAN;
    for (size_t i = 0; i < mpx; i += 5) depth[i] = i % 2 ? -1.0f : NAN;
    for (size_t i = 0; i < 3 * mpx; i += 7) normal[i] = i % 2 ? 3e38f : -INFINITY;
    m.iterations = 3;
    poses_of(poses, frames);
    CHECK(sgm_track(s, &sp, &m, poses, disp, mask, conf, depth, normal, stats, trace_sums, trace_poses));
    m.dist_max = 3e38f; m.span = 1e-38f;
    poses_of(poses, frames);
    CHECK(sgm_track(s, &sp, &m, poses, disp, NULL, NULL, depth, normal, stats, trace_sums, trace_poses));
    m.dist_max = 1e-38f; m.span = 3e38f; m.fx = 1e-38f; m.cy = 3e38f;
    poses_of(poses, frames);
    CHECK(sgm_track(s, &sp, &m, poses, disp, NULL, NULL, depth, normal, stats, NULL, NULL));
    m = model_of(mw, mh, 2);
    poses_of(poses, frames);
    for (int f = 0; f < frames; ++f) poses[12 * f + 8] = -1.0, poses[12 * f + 9] = 3e38, poses[12 * f + 2] = -3e38;
    CHECK(sgm_track(s, &sp, &m, poses, disp, NULL, NULL, depth, normal, stats, trace_sums, trace_poses));
    free(disp); free(mask); free(conf); free(depth); free(normal); free(poses); free(poses32); free(sums); free(stats);
    free(trace_sums); free(trace_poses);
    return 0;
}

int main(void)
{
    /* source W, H; model W, H; frames */
    static const int shapes[][5] = {{1, 1, 1, 1, 1}, {24, 16, 24, 16, 1}, {70, 33, 40, 24, 3}, {65, 3, 3, 65, 2}, {3, 65, 129, 2, 1},
                                    {129, 2, 70, 33, 2}, {12, 8, 12, 8, 64}, {257, 65, 70, 33, 1}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        if (run(s, shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4]) != 0) return 1;
    /* refusals queue nothing */
    {
        float disp[4] = {20, 20, 20, 20}, depth[4] = {2, 2, 2, 2}, normal[12] = {0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1}, poses32[65 * 12];
        double poses[65 * 12];
        int64_t sums[65 * 29];
        sgm_track_stats stats[65];
        poses_of(poses, 65);
        for (int i = 0; i < 65 * 12; ++i) poses32[i] = (float)poses[i];
        const sgm_cloud_spec sp = source_of(2, 2, 1);
        const sgm_track_spec good = model_of(2, 2, 2);
        const int before = stub_track_count();
        CHECK(sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, depth, normal, sums));
        sgm_track_spec bad = good;
        bad.width = 0;
        CHECK(!sgm_track_sums(s, &sp, &bad, poses32, disp, NULL, NULL, depth, normal, sums));
        bad = good; bad.dist_max = 0.0f;
        CHECK(!sgm_track_sums(s, &sp, &bad, poses32, disp, NULL, NULL, depth, normal, sums));
        bad = good; bad.span = NAN;
        CHECK(!sgm_track(s, &sp, &bad, poses, disp, NULL, NULL, depth, normal, stats, NULL, NULL));
        bad = good; bad.iterations = 65;
        CHECK(!sgm_track(s, &sp, &bad, poses, disp, NULL, NULL, depth, normal, stats, NULL, NULL));
        bad = good; bad.min_pixels = 5;
        CHECK(!sgm_track_solve(&bad, sums, poses, poses + 12, stats));
        bad = good; bad.min_pivot = -1.0f;
        CHECK(!sgm_track_solve(&bad, sums, poses, poses + 12, stats));
        sgm_cloud_spec many = sp;
        many.frames = 65;
        CHECK(!sgm_track_sums(s, &many, &good, poses32, disp, NULL, NULL, depth, normal, sums));
        sgm_cloud_spec large = sp;
        large.width = 4097; large.height = 4096;
        CHECK(!sgm_track_sums(s, &large, &good, poses32, disp, NULL, NULL, depth, normal, sums));
        poses32[7] = INFINITY; poses[7] = 1e300;
        CHECK(!sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, depth, normal, sums));
        CHECK(!sgm_track(s, &sp, &good, poses, disp, NULL, NULL, depth, normal, stats, NULL, NULL));
        poses32[7] = 0.0f; poses[7] = 0.0;
        CHECK(!sgm_track_sums(NULL, &sp, &good, poses32, disp, NULL, NULL, depth, normal, sums) &&
              !sgm_track_sums(s, NULL, &good, poses32, disp, NULL, NULL, depth, normal, sums) &&
              !sgm_track_sums(s, &sp, NULL, poses32, disp, NULL, NULL, depth, normal, sums) &&
              !sgm_track_sums(s, &sp, &good, NULL, disp, NULL, NULL, depth, normal, sums) &&
              !sgm_track_sums(s, &sp, &good, poses32, NULL, NULL, NULL, depth, normal, sums) &&      /* no match to take a map from */
              !sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, NULL, normal, sums) &&
              !sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, depth, NULL, sums) &&
              !sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, depth, normal, NULL));
        CHECK(!sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, depth, normal, (int64_t*)((char*)sums + 4)) &&
              !sgm_track_sums(s, &sp, &good, poses32, (float*)sums, NULL, NULL, depth, normal, sums) &&
              !sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, (float*)(sums + 1), normal, sums));
        CHECK(!sgm_track(s, &sp, &good, NULL, disp, NULL, NULL, depth, normal, stats, NULL, NULL) &&
              !sgm_track(s, &sp, &good, poses, disp, NULL, NULL, depth, normal, NULL, NULL, NULL));
        CHECK(!sgm_track_solve(NULL, sums, poses, poses + 12, stats) && !sgm_track_solve(&good, NULL, poses, poses + 12, stats) &&
              !sgm_track_world_pose(NULL, poses, poses32) && !sgm_track_world_pose(poses32, NULL, poses32 + 12));
        CHECK(stub_track_count() == before + 1);
        stub_track_fail_at(0);
        CHECK(!sgm_track_sums(s, &sp, &good, poses32, disp, NULL, NULL, depth, normal, sums));
        stub_track_fail_at(1);
        CHECK(!sgm_track(s, &sp, &good, poses, disp, NULL, NULL, depth, normal, stats, NULL, NULL));
        CHECK(sgm_track(s, &sp, &good, poses, disp, NULL, NULL, depth, normal, stats, NULL, NULL) && sgm_synchronize(s));
    }
    /* behind matches, with and without the post pass on a stream of its own, on the instance's own map; the shape changes in between */
    {
        static const int inst[][2] = {{24, 16}, {70, 33}, {7, 9}};
        for (size_t i = 0; i < sizeof inst / sizeof inst[0]; ++i)
            for (int overlap = 0; overlap < 2; ++overlap) {
                const int w = inst[i][0], h = inst[i][1];
                const size_t n = (size_t)w * h;
                uint8_t* img = (uint8_t*)malloc(2 * n);
                float* disp = (float*)malloc(n * sizeof(float));
                float* depth = (float*)malloc(n * sizeof(float));
                float* normal = (float*)malloc(3 * n * sizeof(float));
                int64_t sums[29];
                sgm_track_stats stats;
                double pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.01, 0, 0};
                const float pose32[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.01f, 0, 0};
                CHECK(img && disp && depth && normal);
                for (size_t k = 0; k < 2 * n; ++k) img[k] = (uint8_t)(k * 37u + (k >> 5));
                for (size_t k = 0; k < n; ++k) {
                    depth[k] = 53.3f;
                    normal[3 * k] = 0.1f; normal[3 * k + 1] = -0.1f; normal[3 * k + 2] = -0.98f;
                }
                const SGMOption o = options(16);
                sgm_cloud_spec sp = source_of(w, h, 1);
                sp.doffs = 0.75f;                                 /* the stand-in's map is all 0: Z = 40 / 0.75 everywhere */
                sp.min_conf = 0;
                sgm_track_spec m = model_of(w, h, 2);
                m.span = 50.0f;
                CHECK(sgm_set_overlap_post(s, overlap) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
                CHECK(sgm_match_device(s, img, img + n, disp));
                CHECK(sgm_track_sums(s, &sp, &m, pose32, disp, NULL, NULL, depth, normal, sums));
                CHECK(sgm_track(s, &sp, &m, pose, disp, NULL, NULL, depth, normal, &stats, NULL, NULL));
                CHECK(sgm_match(s, img, img + n, disp));
                CHECK(sgm_track(s, &sp, &m, pose, NULL, NULL, NULL, depth, normal, &stats, NULL, NULL));
                CHECK(sgm_synchronize(s));
                free(img); free(disp); free(depth); free(normal);
            }
    }
    sgm_destroy(s);
    puts("track_sanitize_driver ok");
    return 0;
}
