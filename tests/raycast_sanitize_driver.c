/* TEST INFRASTRUCTURE (tests/test_raycast_cpu.py): drives sgm_volume_raycast of the product's C host (csrc/sgm_host.c) with the stub
 * device layer (tests/stub_device.c) and the stand-in launchers (tests/stub_volume.c and tests/stub_raycast.c, which compute for
 * real) under AddressSanitizer / UBSan -- volumes of one voxel and of many, filled by the stand-in's integration or with any words,
 * views of one pixel, of one row and of one column, batches up to the 64 frames a call takes, cameras inside the volume, outside
 * it, looking away and with huge entries, with and without normals, behind matches with and without the post pass on a stream of
 * its own, refusals, a refused launch, and the lifetime of all of it.  A stand-alone program: nothing is loaded into another
 * process.  Results are not checked here (tests/test_raycast_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "raycast_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_raycast_count(void);
void stub_raycast_fail_at(int nth);

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
    const sgm_cloud_spec sp = {w, h, frames, fx, fx, (float)(w - 1) / 2, (float)(h - 1) / 2, 40.0f / fx, 0.0f, 0.1f, 1000.0f, 0};
    return sp;
}

static sgm_raycast_spec view_of(int w, int h, int frames, uint32_t min_weight)
{
    const float fx = 40.0f * (float)(w > h ? w : h) / 70.0f;
    const sgm_raycast_spec vw = {w, h, frames, fx, fx, (float)(w - 1) / 2, (float)(h - 1) / 2, 0.3f, 1.9f, 0.07f, min_weight};
    return vw;
}

/* a box in front of the camera, 1.8 wide, from Z = 0.5 on */
static sgm_volume_spec volume_of(int nx, int ny, int nz)
{
    const float voxel = 1.8f / (float)(nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz));
    const sgm_volume_spec v = {nx, ny, nz, voxel, {-0.5f * (float)nx * voxel, -0.5f * (float)ny * voxel, 0.5f}, 0.2f, 3};
    return v;
}

static void poses_of(float* p, int frames)
{
    for (int f = 0; f < frames; ++f) {
        const float a = 0.03f * (float)(f % 7), c = cosf(a), s = sinf(a);
        const float pose[12] = {c, 0, s, 0, 1, 0, -s, 0, c, 0.01f * (float)(f % 3), -0.01f, 0.002f * (float)f};
        memcpy(p + 12 * f, pose, sizeof pose);
    }
}

static int run(sgm_instance* s, int nx, int ny, int nz, int w, int h, int frames)
{
    const size_t nv = (size_t)nx * ny * nz, px = (size_t)w * h * frames, src_px = 70 * 33;
    float* disp = (float*)malloc(src_px * sizeof(float));
    float* poses = (float*)malloc((size_t)frames * 12 * sizeof(float));
    uint32_t* voxels = (uint32_t*)calloc(nv, sizeof(uint32_t));
    float* depth = (float*)malloc(px * sizeof(float));
    float* normal = (float*)malloc(3 * px * sizeof(float));
    CHECK(disp && poses && voxels && depth && normal);
    for (size_t i = 0; i < src_px; ++i) disp[i] = 36.0f + (float)(i % 97) * 0.06f;
    const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const sgm_cloud_spec sp = source_of(70, 33, 1);
    const sgm_volume_spec v = volume_of(nx, ny, nz);
    for (int round = 0; round < 2; ++round) CHECK(sgm_volume_integrate(s, &v, &sp, identity, disp, NULL, NULL, voxels));
    poses_of(poses, frames);
    for (uint32_t mw = 1; mw <= 3; ++mw) {
        const sgm_raycast_spec vw = view_of(w, h, frames, mw);
        CHECK(sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, normal) && sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, NULL));
    }
    sgm_raycast_spec vw = view_of(w, h, frames, 1);
    /* looking away, far off to the side, from inside the volume, with entries that overflow on the way */
    for (int f = 0; f < frames; ++f) poses[12 * f + 8] = -poses[12 * f + 8], poses[12 * f] = -poses[12 * f];
    CHECK(sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, normal));
    poses_of(poses, frames);
    for (int f = 0; f < frames; ++f) poses[12 * f + 9] = 3e38f, poses[12 * f + 2] = 3e38f;
    CHECK(sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, normal));
    poses_of(poses, frames);
    for (int f = 0; f < frames; ++f) poses[12 * f + 11] = -1.0f;
    vw.z_min = 0.0f; vw.step = 0.013f; vw.z_max = 3.0f;
    CHECK(sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, normal));
    /* a volume as a caller may leave it: any words; a step larger than the volume; intrinsics at the ends of float */
    for (size_t i = 0; i < nv; ++i) voxels[i] = (uint32_t)(i * 2654435761u);
    poses_of(poses, frames);
    CHECK(sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, normal));
    vw.step = 2.5f;
    CHECK(sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, normal));
    vw.step = 0.05f; vw.fx = 1e-38f; vw.cy = 3e38f;
    CHECK(sgm_volume_raycast(s, &v, &vw, poses, voxels, depth, normal) && sgm_synchronize(s));
    free(disp); free(poses); free(voxels); free(depth); free(normal);
    return 0;
}

int main(void)
{
    /* volume nx, ny, nz; view W, H, frames */
    static const int shapes[][6] = {{1, 1, 1, 1, 1, 1},    {8, 5, 3, 24, 16, 1},  {36, 33, 20, 70, 33, 3}, {37, 21, 5, 65, 3, 2}, {2, 2, 2, 3, 65, 1},
                                    {1, 1, 1024, 129, 2, 1}, {1024, 1, 2, 5, 1, 2}, {5, 5, 5, 12, 8, 64},    {2, 1024, 1, 1, 7, 3}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        if (run(s, shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], shapes[i][5]) != 0) return 1;
    /* refusals queue nothing */
    {
        float poses[65 * 12], depth[8], normal[24];
        uint32_t voxels[8] = {0};
        poses_of(poses, 65);
        const sgm_volume_spec v = volume_of(2, 2, 2);
        const sgm_raycast_spec good = view_of(2, 2, 1, 1);
        const int before = stub_raycast_count();
        CHECK(sgm_volume_raycast(s, &v, &good, poses, voxels, depth, normal));
        sgm_raycast_spec bad = good;
        bad.frames = 65;
        CHECK(!sgm_volume_raycast(s, &v, &bad, poses, voxels, depth, normal));
        bad = good; bad.fx = 0.0f;
        CHECK(!sgm_volume_raycast(s, &v, &bad, poses, voxels, depth, normal));
        bad = good; bad.z_max = INFINITY;
        CHECK(!sgm_volume_raycast(s, &v, &bad, poses, voxels, depth, normal));
        bad = good; bad.step = 1e-9f;
        CHECK(!sgm_volume_raycast(s, &v, &bad, poses, voxels, depth, normal));
        bad = good; bad.min_weight = 0;
        CHECK(!sgm_volume_raycast(s, &v, &bad, poses, voxels, depth, normal));
        sgm_volume_spec v2 = v;
        v2.voxel = NAN;
        CHECK(!sgm_volume_raycast(s, &v2, &good, poses, voxels, depth, normal));
        poses[7] = INFINITY;
        CHECK(!sgm_volume_raycast(s, &v, &good, poses, voxels, depth, normal));
        poses_of(poses, 65);
        CHECK(!sgm_volume_raycast(NULL, &v, &good, poses, voxels, depth, normal) && !sgm_volume_raycast(s, NULL, &good, poses, voxels, depth, normal) &&
              !sgm_volume_raycast(s, &v, NULL, poses, voxels, depth, normal) && !sgm_volume_raycast(s, &v, &good, NULL, voxels, depth, normal) &&
              !sgm_volume_raycast(s, &v, &good, poses, NULL, depth, normal) && !sgm_volume_raycast(s, &v, &good, poses, voxels, NULL, normal));
        CHECK(!sgm_volume_raycast(s, &v, &good, poses, voxels, (float*)voxels, normal) && !sgm_volume_raycast(s, &v, &good, poses, voxels, depth, depth) &&
              !sgm_volume_raycast(s, &v, &good, poses, voxels, normal + 8, normal) &&
              !sgm_volume_raycast(s, &v, &good, poses, voxels, (float*)((char*)depth + 2), normal));
        CHECK(stub_raycast_count() == before + 1);
        stub_raycast_fail_at(0);
        CHECK(!sgm_volume_raycast(s, &v, &good, poses, voxels, depth, normal));
        CHECK(sgm_volume_raycast(s, &v, &good, poses, voxels, depth, normal) && sgm_synchronize(s));
    }
    /* behind matches, with and without the post pass on a stream of its own; the instance's shape changes in between */
    {
        static const int inst[][2] = {{24, 16}, {70, 33}, {7, 9}};
        for (size_t i = 0; i < sizeof inst / sizeof inst[0]; ++i)
            for (int overlap = 0; overlap < 2; ++overlap) {
                const int w = inst[i][0], h = inst[i][1];
                const size_t n = (size_t)w * h;
                uint8_t* img = (uint8_t*)malloc(2 * n);
                float* disp = (float*)malloc(n * sizeof(float));
                uint32_t* voxels = (uint32_t*)calloc(12 * 6 * 8, sizeof(uint32_t));
                float* depth = (float*)malloc(n * sizeof(float));
                float* normal = (float*)malloc(3 * n * sizeof(float));
                CHECK(img && disp && voxels && depth && normal);
                for (size_t k = 0; k < 2 * n; ++k) img[k] = (uint8_t)(k * 37u + (k >> 5));
                const SGMOption o = options(16);
                const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
                sgm_cloud_spec sp = source_of(w, h, 1);
                sp.doffs = 0.75f;                                 /* the stand-in's map is all 0: Z = 40 / 0.75 everywhere */
                sgm_volume_spec v = volume_of(12, 6, 8);
                v.origin[2] = 52.9f;
                sgm_raycast_spec vw = view_of(w, h, 1, 1);
                vw.z_min = 52.0f; vw.z_max = 55.0f; vw.step = 0.1f;
                CHECK(sgm_set_overlap_post(s, overlap) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
                CHECK(sgm_match_device(s, img, img + n, disp));
                CHECK(sgm_volume_integrate(s, &v, &sp, identity, disp, NULL, NULL, voxels));
                CHECK(sgm_volume_raycast(s, &v, &vw, identity, voxels, depth, normal) && sgm_volume_raycast(s, &v, &vw, identity, voxels, depth, NULL));
                CHECK(sgm_synchronize(s));
                free(img); free(disp); free(voxels); free(depth); free(normal);
            }
    }
    sgm_destroy(s);
    puts("raycast_sanitize_driver ok");
    return 0;
}
