/* TEST INFRASTRUCTURE (tests/test_volume_cpu.py): drives the TSDF volume entry points of the product's C host (csrc/sgm_host.c) with
 * the stub device layer (tests/stub_device.c) and the stand-in volume launchers (tests/stub_volume.c, which compute for real and use
 * the tile scratch the way the kernels do) under AddressSanitizer / UBSan -- volumes of one voxel, of one tile and of several, that
 * grow and shrink on one instance, batches up to the 64 frames a call takes, maps with special values, poses that look away, lists
 * clipped by their capacity, the last match's map after every kind of match, refusals, refused launches, and the lifetime of all of
 * it.  A stand-alone program: nothing is loaded into another process.  Results are not checked here (tests/test_volume_cpu.py
 * does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "volume_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_volume_count(void);
void stub_volume_fail_at(int nth);

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

/* fb = 40: a disparity near 39 is a depth near 1.03 */
static sgm_cloud_spec source_of(int w, int h, int frames)
{
    const float fx = 40.0f * (float)w / 70.0f;
    const sgm_cloud_spec sp = {w, h, frames, fx, fx, (float)(w - 1) / 2, (float)(h - 1) / 2, 40.0f / fx, 0.75f, 0.1f, 1000.0f, 7};
    return sp;
}

/* a box in front of the camera, 1.8 wide, from Z = 0.5 on */
static sgm_volume_spec volume_of(int nx, int ny, int nz, uint32_t max_weight)
{
    const float voxel = 1.8f / (float)(nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz));
    const sgm_volume_spec v = {nx, ny, nz, voxel, {-0.5f * (float)nx * voxel, -0.5f * (float)ny * voxel, 0.5f}, 0.2f, max_weight};
    return v;
}

static void poses_of(float* p, int frames)
{
    for (int f = 0; f < frames; ++f) {
        const float a = 0.01f * (float)(f % 7), c = cosf(a), s = sinf(a);
        const float pose[12] = {c, 0, s, 0, 1, 0, -s, 0, c, 0.01f * (float)(f % 3), -0.01f, 0.002f * (float)f};
        memcpy(p + 12 * f, pose, sizeof pose);
    }
}

/* both entry points on the caller's own buffers: no instance shape involved */
static int run_explicit(sgm_instance* s, int nx, int ny, int nz, int w, int h, int frames, int with_maps)
{
    const size_t n = (size_t)w * h * frames, nv = (size_t)nx * ny * nz;
    float* disp = (float*)malloc(n * sizeof(float));
    uint8_t* mask = (uint8_t*)malloc(n);
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* poses = (float*)malloc((size_t)frames * 12 * sizeof(float));
    uint32_t* voxels = (uint32_t*)calloc(nv, sizeof(uint32_t));
    sgm_surface_point* points = (sgm_surface_point*)aligned_alloc(16, (3 * nv + 1) * sizeof(sgm_surface_point));
    uint32_t count = 0;
    CHECK(disp && mask && conf && poses && voxels && points);
    const float special[] = {NAN, INFINITY, -INFINITY, -0.75f, -1.0f, 0.0f, 1e-38f, 3e38f};
    for (size_t i = 0; i < n; ++i) {
        disp[i] = (i % 11 == 3) ? special[(i / 11) % 8] : 36.0f + (float)(i % 97) * 0.06f;
        mask[i] = (uint8_t)(i % 5 != 0);
        conf[i] = (uint16_t)(i % 13);
    }
    poses_of(poses, frames);
    const sgm_cloud_spec sp = source_of(w, h, frames);
    sgm_volume_spec v = volume_of(nx, ny, nz, 3);
    CHECK(sgm_volume_bytes(&v) == nv * sizeof(uint32_t));
    for (int round = 0; round < 3; ++round)                       /* past the weight's cap */
        CHECK(sgm_volume_integrate(s, &v, &sp, poses, disp, with_maps ? mask : NULL, with_maps ? conf : NULL, voxels));
    CHECK(sgm_synchronize(s));
    for (uint32_t mw = 1; mw <= 3; ++mw) {
        CHECK(sgm_volume_points(s, &v, voxels, mw, points, 3 * nv, &count) && sgm_synchronize(s) && count <= 3 * nv);
        /* clipped lists: nothing, one short, exactly the count */
        const uint32_t full = count;
        CHECK(sgm_volume_points(s, &v, voxels, mw, NULL, 0, &count) && count == full);
        if (full) CHECK(sgm_volume_points(s, &v, voxels, mw, points, full - 1, &count) && count == full);
        CHECK(sgm_volume_points(s, &v, voxels, mw, points, full, &count) && sgm_synchronize(s) && count == full);
    }
    /* every voxel outside every frame's image: behind the cameras, and far off to the side */
    uint32_t* before = (uint32_t*)malloc(nv * sizeof(uint32_t));
    CHECK(before);
    memcpy(before, voxels, nv * sizeof(uint32_t));
    for (int f = 0; f < frames; ++f) poses[12 * f + 8] = -poses[12 * f + 8], poses[12 * f + 11] = -3.0f;
    CHECK(sgm_volume_integrate(s, &v, &sp, poses, disp, NULL, NULL, voxels) && memcmp(before, voxels, nv * sizeof(uint32_t)) == 0);
    poses_of(poses, frames);
    for (int f = 0; f < frames; ++f) poses[12 * f + 9] = 3e38f;
    CHECK(sgm_volume_integrate(s, &v, &sp, poses, disp, NULL, NULL, voxels) && memcmp(before, voxels, nv * sizeof(uint32_t)) == 0);
    /* a volume as a caller may leave it: any words */
    for (size_t i = 0; i < nv; ++i) voxels[i] = (uint32_t)(i * 2654435761u);
    poses_of(poses, frames);
    v.max_weight = 65535;
    CHECK(sgm_volume_integrate(s, &v, &sp, poses, disp, NULL, NULL, voxels));
    CHECK(sgm_volume_points(s, &v, voxels, 1, points, 3 * nv, &count) && sgm_synchronize(s));
    free(before); free(disp); free(mask); free(conf); free(poses); free(voxels); free(points);
    return 0;
}

/* the last match's map, after every kind of match */
static int run_instance(sgm_instance* s, int w, int h, int batch)
{
    const size_t n = (size_t)w * h * batch, nv = 12 * 6 * 8;
    uint8_t* img = (uint8_t*)malloc(2 * n);
    float* disp = (float*)malloc(2 * n * sizeof(float));
    uint16_t* conf = (uint16_t*)malloc(n * sizeof(uint16_t));
    float* poses = (float*)malloc((size_t)batch * 12 * sizeof(float));
    uint32_t* voxels = (uint32_t*)calloc(nv, sizeof(uint32_t));
    CHECK(img && disp && conf && poses && voxels);
    for (size_t i = 0; i < 2 * n; ++i) img[i] = (uint8_t)(i * 37u + (i >> 5));
    poses_of(poses, batch);
    const SGMOption o = options(16);
    const sgm_cloud_spec sp = source_of(w, h, batch);
    sgm_volume_spec v = volume_of(12, 6, 8, 5);
    v.origin[2] = 52.9f;                                          /* the stand-in's map is all 0: Z = 40 / 0.75 everywhere */
    CHECK(sgm_set_batch(s, batch) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
    uint8_t *l = img, *r = img + n;
    for (int overlap = 0; overlap < 2; ++overlap) {
        CHECK(sgm_set_overlap_post(s, overlap));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match(s, l, r, disp));
        CHECK(sgm_volume_integrate(s, &v, &sp, poses, NULL, NULL, NULL, voxels) && sgm_synchronize(s));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_confidence(s, l, r, disp, conf));
        CHECK(sgm_volume_integrate(s, &v, &sp, poses, NULL, NULL, conf, voxels) && sgm_synchronize(s));
        CHECK(sgm_reset(s, (uint16_t)w, (uint16_t)h, &o) && sgm_match_both(s, l, r, disp, disp + n));
        CHECK(sgm_volume_integrate(s, &v, &sp, poses, NULL, NULL, NULL, voxels) && sgm_synchronize(s));
    }
    /* a spec of another shape; a refused launch leaves the instance usable */
    sgm_cloud_spec other = sp;
    other.width = w + 1;
    CHECK(!sgm_volume_integrate(s, &v, &other, poses, NULL, NULL, NULL, voxels));
    stub_volume_fail_at(0);
    CHECK(!sgm_volume_integrate(s, &v, &sp, poses, NULL, NULL, NULL, voxels));
    CHECK(sgm_volume_integrate(s, &v, &sp, poses, NULL, NULL, NULL, voxels) && sgm_synchronize(s));
    free(img); free(disp); free(conf); free(poses); free(voxels);
    return 0;
}

int main(void)
{
    /* volume nx, ny, nz; source W, H, frames: one voxel, less than a tile, exactly one, one more, many; grow / shrink / grow */
    static const int shapes[][6] = {{1, 1, 1, 1, 1, 1},     {8, 5, 3, 24, 16, 1},   {36, 33, 20, 70, 33, 3}, {64, 8, 4, 64, 20, 2},
                                    {1024, 2, 1, 37, 21, 1}, {683, 3, 1, 37, 21, 1}, {1, 1024, 1, 20, 31, 1}, {1, 1, 1024, 3, 1, 5}, {64, 20, 12, 64, 20, 2},
                                    {5, 5, 5, 12, 8, 64},    {70, 41, 33, 130, 40, 3}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        for (int k = 0; k < 2; ++k)
            if (run_explicit(s, shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], shapes[i][5], k) != 0) return 1;
    /* refusals queue nothing */
    {
        float d[4] = {1, 2, 3, 4}, poses[65 * 12];
        uint32_t voxels[8] = {0}, count;
        sgm_surface_point* points = (sgm_surface_point*)aligned_alloc(16, 24 * sizeof(sgm_surface_point));
        CHECK(points);
        poses_of(poses, 65);
        const sgm_cloud_spec good = source_of(2, 2, 1);
        const sgm_volume_spec v = volume_of(2, 2, 2, 4);
        const int before = stub_volume_count();
        sgm_cloud_spec bad = good;
        bad.fx = 0.0f;
        CHECK(!sgm_volume_integrate(s, &v, &bad, poses, d, NULL, NULL, voxels));
        bad = good; bad.frames = 65;
        CHECK(!sgm_volume_integrate(s, &v, &bad, poses, d, NULL, NULL, voxels));
        sgm_volume_spec v2 = v;
        v2.nx = 1025;
        CHECK(!sgm_volume_integrate(s, &v2, &good, poses, d, NULL, NULL, voxels) && sgm_volume_bytes(&v2) == 0 && sgm_volume_bytes(NULL) == 0);
        v2 = v; v2.trunc = NAN;
        CHECK(!sgm_volume_integrate(s, &v2, &good, poses, d, NULL, NULL, voxels) && !sgm_volume_points(s, &v2, voxels, 1, points, 24, &count));
        v2 = v; v2.max_weight = 0;
        CHECK(!sgm_volume_integrate(s, &v2, &good, poses, d, NULL, NULL, voxels));
        poses[7] = INFINITY;
        CHECK(!sgm_volume_integrate(s, &v, &good, poses, d, NULL, NULL, voxels));
        poses_of(poses, 65);
        CHECK(!sgm_volume_integrate(NULL, &v, &good, poses, d, NULL, NULL, voxels) && !sgm_volume_integrate(s, NULL, &good, poses, d, NULL, NULL, voxels) &&
              !sgm_volume_integrate(s, &v, NULL, poses, d, NULL, NULL, voxels) && !sgm_volume_integrate(s, &v, &good, NULL, d, NULL, NULL, voxels) &&
              !sgm_volume_integrate(s, &v, &good, poses, d, NULL, NULL, NULL));
        CHECK(!sgm_volume_integrate(s, &v, &good, poses, d, NULL, NULL, (uint32_t*)d) && !sgm_volume_integrate(s, &v, &good, poses, d, (uint8_t*)voxels, NULL, voxels));
        CHECK(!sgm_volume_points(s, &v, voxels, 0, points, 24, &count) && !sgm_volume_points(s, &v, voxels, 65536, points, 24, &count) &&
              !sgm_volume_points(s, &v, voxels, 1, NULL, 24, &count) && !sgm_volume_points(s, &v, voxels, 1, points, 24, NULL) &&
              !sgm_volume_points(s, &v, NULL, 1, points, 24, &count) && !sgm_volume_points(s, &v, voxels, 1, points, 24, voxels + 1) &&
              !sgm_volume_points(s, &v, voxels, 1, (sgm_surface_point*)((char*)points + 4), 23, &count) &&
              !sgm_volume_points(s, &v, voxels, 1, points, (size_t)-1, (uint32_t*)(points + 3)));
        CHECK(!sgm_volume_integrate(s, &v, &good, poses, NULL, NULL, NULL, voxels));         /* no match yet: nothing to read */
        CHECK(stub_volume_count() == before);
        free(points);
    }
    /* grow, shrink, batch: the instance's own map */
    static const int inst[][3] = {{24, 16, 1}, {70, 33, 2}, {7, 9, 1}, {1, 1, 1}, {64, 32, 3}, {20, 31, 1}};
    for (size_t i = 0; i < sizeof inst / sizeof inst[0]; ++i)
        if (run_instance(s, inst[i][0], inst[i][1], inst[i][2]) != 0) return 1;
    sgm_destroy(s);
    puts("volume_sanitize_driver ok");
    return 0;
}
