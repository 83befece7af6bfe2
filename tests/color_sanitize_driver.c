/* TEST INFRASTRUCTURE (tests/test_color_cpu.py): drives sgm_volume_integrate_color, sgm_volume_raycast_color and sgm_volume_colors of
 * the product's C host (csrc/sgm_host.c) with the stub device layer (tests/stub_device.c) and the stand-in launchers
 * (tests/stub_volume.c, stub_raycast.c, stub_mesh.c and stub_color.c, which compute for real) under AddressSanitizer / UBSan --
 * volumes of one voxel and of many, both image kinds, batches, views of one pixel, of a row and of a column, colour volumes with any
 * words, lists of the volume's own vertices and points and of any ids, with and without the count, refusals, refused launches,
 * behind matches with and without the post pass on a stream of its own, and the lifetime of all of it.  A stand-alone program:
 * nothing is loaded into another process.  Results are not checked here (tests/test_color_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "color_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_color_count(void);
void stub_color_fail_at(int nth);

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

static sgm_raycast_spec view_of(int w, int h, int frames)
{
    const float fx = 40.0f * (float)(w > h ? w : h) / 70.0f;
    const sgm_raycast_spec vw = {w, h, frames, fx, fx, (float)(w - 1) / 2, (float)(h - 1) / 2, 0.3f, 1.9f, 0.07f, 1};
    return vw;
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
        const float a = 0.03f * (float)(f % 7), c = cosf(a), s = sinf(a);
        const float pose[12] = {c, 0, s, 0, 1, 0, -s, 0, c, 0.01f * (float)(f % 3), -0.01f, 0.002f * (float)f};
        memcpy(p + 12 * f, pose, sizeof pose);
    }
}

static int run(sgm_instance* s, int nx, int ny, int nz, int w, int h, int frames)
{
    const size_t nv = (size_t)nx * ny * nz, px = (size_t)w * h * frames, src_px = (size_t)70 * 33 * frames;
    float* disp = (float*)malloc(src_px * sizeof(float));
    uint8_t* grey = (uint8_t*)malloc(src_px);
    uint32_t* rgb = (uint32_t*)malloc(src_px * sizeof(uint32_t));
    float* poses = (float*)malloc((size_t)frames * 12 * sizeof(float));
    uint32_t* voxels = (uint32_t*)calloc(nv, sizeof(uint32_t));
    uint32_t* colors = (uint32_t*)calloc(nv, sizeof(uint32_t));
    float* depth = (float*)malloc(px * sizeof(float));
    float* normal = (float*)malloc(3 * px * sizeof(float));
    uint32_t* rgba = (uint32_t*)malloc(px * sizeof(uint32_t));
    const size_t cap = 7 * nv;
    sgm_mesh_vertex* records = (sgm_mesh_vertex*)malloc((cap + 1) * sizeof(sgm_mesh_vertex));
    uint32_t* out = (uint32_t*)malloc((cap + 1) * sizeof(uint32_t));
    uint32_t counts[2] = {0, 0};
    CHECK(disp && grey && rgb && poses && voxels && colors && depth && normal && rgba && records && out);
    for (size_t i = 0; i < src_px; ++i) {
        disp[i] = 36.0f + (float)(i % 97) * 0.06f;
        grey[i] = (uint8_t)(i * 13u);
        rgb[i] = (uint32_t)(i * 2654435761u);
    }
    poses_of(poses, frames);
    const sgm_cloud_spec sp = source_of(70, 33, frames);
    for (uint32_t max_weight = 2; max_weight <= 300; max_weight += 298) {
        const sgm_volume_spec v = volume_of(nx, ny, nz, max_weight);
        CHECK(sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, grey, 1, voxels, colors));
        CHECK(sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, rgb, 4, voxels, colors));
        const sgm_raycast_spec vw = view_of(w, h, frames);
        CHECK(sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, rgba));
        CHECK(sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, NULL, rgba));
        /* the volume's own lists: the vertices (where the mesh takes so large a volume) and the points, with their counts */
        if (sgm_volume_mesh(s, &v, voxels, 1, records, cap, NULL, 0, counts))
            CHECK(sgm_volume_colors(s, &v, voxels, colors, records, cap, counts, 8, out) && sgm_volume_colors(s, &v, voxels, colors, records, cap, NULL, 8, out));
        CHECK(sgm_volume_points(s, &v, voxels, 1, (sgm_surface_point*)records, cap, counts));
        CHECK(sgm_volume_colors(s, &v, voxels, colors, records, cap, counts, 4, out) && sgm_volume_colors(s, &v, voxels, colors, records, 1, counts, 4, out));
        /* any ids, any colours */
        for (size_t i = 0; i < cap; ++i) records[i].id = (uint32_t)(i * 2654435761u) >> (i % 29);
        for (size_t i = 0; i < nv; ++i) colors[i] = (uint32_t)(i * 2246822519u) >> (i % 9);
        CHECK(sgm_volume_colors(s, &v, voxels, colors, records, cap, NULL, 8, out) && sgm_volume_colors(s, &v, voxels, colors, records, cap, NULL, 4, out));
        CHECK(sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, rgba));
        CHECK(sgm_volume_colors(s, &v, voxels, colors, NULL, 0, NULL, 8, NULL) && sgm_synchronize(s));
    }
    free(disp); free(grey); free(rgb); free(poses); free(voxels); free(colors); free(depth); free(normal); free(rgba); free(records); free(out);
    return 0;
}

int main(void)
{
    /* volume nx, ny, nz; view W, H; frames of both */
    static const int shapes[][6] = {{1, 1, 1, 1, 1, 1},      {8, 5, 3, 24, 16, 1},  {36, 33, 20, 70, 33, 3}, {37, 21, 5, 65, 3, 2},
                                    {2, 2, 2, 3, 65, 1},     {1, 1, 1024, 33, 9, 1}, {1024, 1, 2, 5, 1, 2},  {5, 5, 5, 12, 8, 5}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        if (run(s, shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], shapes[i][4], shapes[i][5]) != 0) return 1;
    /* refusals queue nothing */
    {
        float poses[12], disp[4] = {39, 39, 39, 39}, depth[4], normal[12];
        uint32_t voxels[8] = {0}, colors[8] = {0}, image[4] = {0}, rgba[8], count = 8;
        sgm_mesh_vertex records[8];
        memset(records, 0, sizeof records);
        poses_of(poses, 1);
        const sgm_volume_spec v = volume_of(2, 2, 2, 3);
        const sgm_cloud_spec sp = source_of(2, 2, 1);
        const sgm_raycast_spec vw = view_of(2, 2, 1);
        const int before = stub_color_count();
        CHECK(sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 4, voxels, colors));
        CHECK(sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, rgba));
        CHECK(sgm_volume_colors(s, &v, voxels, colors, records, 8, &count, 8, rgba));
        CHECK(!sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, NULL, 4, voxels, colors) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 4, voxels, NULL) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 3, voxels, colors) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, (char*)image + 1, 4, voxels, colors) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 4, voxels, (uint32_t*)((char*)colors + 2)) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 4, voxels, voxels + 7) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 4, voxels, image) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 4, voxels, (uint32_t*)disp) &&
              !sgm_volume_integrate_color(s, &v, &sp, poses, NULL, NULL, NULL, image, 4, voxels, colors));
        CHECK(!sgm_volume_raycast_color(s, &v, &vw, poses, voxels, NULL, depth, normal, rgba) &&
              !sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, NULL) &&
              !sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, (uint32_t*)((char*)rgba + 1)) &&
              !sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, colors) &&
              !sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, voxels + 4) &&
              !sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, (uint32_t*)depth) &&
              !sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, (uint32_t*)normal + 11));
        CHECK(!sgm_volume_colors(s, &v, NULL, colors, records, 8, &count, 8, rgba) && !sgm_volume_colors(s, &v, voxels, NULL, records, 8, &count, 8, rgba) &&
              !sgm_volume_colors(s, &v, voxels, colors, NULL, 8, &count, 8, rgba) && !sgm_volume_colors(s, &v, voxels, colors, records, 8, &count, 8, NULL) &&
              !sgm_volume_colors(s, &v, voxels, colors, records, 8, &count, 5, rgba) &&
              !sgm_volume_colors(s, &v, voxels, colors, (char*)records + 8, 7, &count, 8, rgba) &&
              !sgm_volume_colors(s, &v, voxels, colors, records, 8, &count, 8, (uint32_t*)records) &&
              !sgm_volume_colors(s, &v, voxels, colors, records, 8, &count, 8, colors) && !sgm_volume_colors(s, &v, voxels, colors, records, 8, rgba + 3, 8, rgba));
        CHECK(stub_color_count() == before + 3);
        for (int k = 0; k < 3; ++k) {
            stub_color_fail_at(0);
            CHECK(!(k == 0 ? sgm_volume_integrate_color(s, &v, &sp, poses, disp, NULL, NULL, image, 4, voxels, colors)
                    : k == 1 ? sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, rgba)
                             : sgm_volume_colors(s, &v, voxels, colors, records, 8, &count, 8, rgba)));
        }
        CHECK(sgm_volume_raycast_color(s, &v, &vw, poses, voxels, colors, depth, normal, rgba) && sgm_synchronize(s));
    }
    /* behind matches, with and without the post pass on a stream of its own: the instance's last map and the caller's buffer */
    {
        static const int inst[][2] = {{24, 16}, {70, 33}, {7, 9}};
        for (size_t i = 0; i < sizeof inst / sizeof inst[0]; ++i)
            for (int overlap = 0; overlap < 2; ++overlap) {
                const int w = inst[i][0], h = inst[i][1];
                const size_t n = (size_t)w * h;
                uint8_t* img = (uint8_t*)malloc(2 * n);
                float* disp = (float*)malloc(n * sizeof(float));
                uint32_t* voxels = (uint32_t*)calloc(12 * 6 * 8, sizeof(uint32_t));
                uint32_t* colors = (uint32_t*)calloc(12 * 6 * 8, sizeof(uint32_t));
                float* depth = (float*)malloc(n * sizeof(float));
                uint32_t* rgba = (uint32_t*)malloc(n * sizeof(uint32_t));
                CHECK(img && disp && voxels && colors && depth && rgba);
                for (size_t k = 0; k < 2 * n; ++k) img[k] = (uint8_t)(k * 37u + (k >> 5));
                const SGMOption o = options(16);
                const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
                sgm_cloud_spec sp = source_of(w, h, 1);
                sp.doffs = 0.75f;                                 /* the stand-in's map is all 0: Z = 40 / 0.75 everywhere */
                sgm_volume_spec v = volume_of(12, 6, 8, 3);
                v.origin[2] = 52.9f;
                sgm_raycast_spec vw = view_of(w, h, 1);
                vw.z_min = 52.0f; vw.z_max = 55.0f; vw.step = 0.1f;
                CHECK(sgm_set_overlap_post(s, overlap) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
                CHECK(sgm_match(s, img, img + n, disp));
                CHECK(sgm_volume_integrate_color(s, &v, &sp, identity, NULL, NULL, NULL, img, 1, voxels, colors));
                CHECK(sgm_match_device(s, img, img + n, disp));
                CHECK(sgm_volume_integrate_color(s, &v, &sp, identity, disp, NULL, NULL, img, 1, voxels, colors));
                CHECK(sgm_volume_raycast_color(s, &v, &vw, identity, voxels, colors, depth, NULL, rgba));
                CHECK(sgm_synchronize(s));
                free(img); free(disp); free(voxels); free(colors); free(depth); free(rgba);
            }
    }
    sgm_destroy(s);
    puts("color_sanitize_driver ok");
    return 0;
}
