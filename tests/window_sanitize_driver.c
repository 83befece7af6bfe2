/* TEST INFRASTRUCTURE (tests/test_window_cpu.py): drives sgm_volume_window, sgm_volume_window_spec, sgm_volume_follow and
 * sgm_volume_leaving of the product's C host (csrc/sgm_host.c) with the stub device layer (tests/stub_device.c) and the stand-in
 * launcher (tests/stub_window.c, which windows for real) under AddressSanitizer / UBSan -- arrays allocated to the byte, so that a
 * word read or written outside one is seen; sources and windows of one voxel and of many, every x offset across both edges, with
 * and without colours, the documented loop of a rig that walks away, refusals, a refused launch, behind matches with and without
 * the post pass on a stream of its own, and the lifetime of all of it.  A stand-alone program: nothing is loaded into another
 * process.  The copy rule is checked here as well, word by word (tests/test_window_cpu.py compares with the restatement). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "window_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_window_count(void);
void stub_window_fail_at(int nth);

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

static sgm_volume_spec volume_of(int nx, int ny, int nz)
{
    const sgm_volume_spec v = {nx, ny, nz, 0.0625f, {-1.125f, -1.0f, 0.5f}, 0.25f, 9};
    return v;
}

static uint32_t word_of(size_t i, uint32_t salt) { return (uint32_t)(i * 2654435761u + salt) | 1u; }       /* never 0 */

/* one window of src (n voxels per axis) into exactly allocated arrays, checked word by word */
static int one(sgm_instance* s, const int* n, const int* offset, const int* dims, int color)
{
    const sgm_volume_spec v = volume_of(n[0], n[1], n[2]);
    const size_t ns = (size_t)n[0] * n[1] * n[2], nd = (size_t)dims[0] * dims[1] * dims[2];
    uint32_t* src = (uint32_t*)malloc(ns * sizeof(uint32_t));
    uint32_t* src_col = (uint32_t*)malloc(ns * sizeof(uint32_t));
    uint32_t* dst = (uint32_t*)malloc(nd * sizeof(uint32_t));
    uint32_t* dst_col = (uint32_t*)malloc(nd * sizeof(uint32_t));
    sgm_volume_spec out, want;
    CHECK(src && src_col && dst && dst_col);
    for (size_t i = 0; i < ns; ++i) {
        src[i] = word_of(i, 17u);
        src_col[i] = word_of(i, 99u);
    }
    CHECK(sgm_volume_window(s, &v, offset, dims, src, color ? src_col : NULL, dst, color ? dst_col : NULL, &out) && sgm_synchronize(s));
    CHECK(sgm_volume_window_spec(&v, offset, dims, &want) && memcmp(&out, &want, sizeof out) == 0);
    CHECK(out.nx == dims[0] && out.ny == dims[1] && out.nz == dims[2] && out.voxel == v.voxel && out.trunc == v.trunc && out.max_weight == 9);
    for (int a = 0; a < 3; ++a) CHECK(out.origin[a] == v.origin[a] + (float)offset[a] * 0.0625f);
    for (int k = 0; k < dims[2]; ++k)
        for (int j = 0; j < dims[1]; ++j)
            for (int i = 0; i < dims[0]; ++i) {
                const int si = i + offset[0], sj = j + offset[1], sk = k + offset[2];
                const int inside = si >= 0 && si < n[0] && sj >= 0 && sj < n[1] && sk >= 0 && sk < n[2];
                const size_t at = ((size_t)k * dims[1] + j) * dims[0] + i, from = inside ? ((size_t)sk * n[1] + sj) * n[0] + si : 0;
                CHECK(dst[at] == (inside ? src[from] : 0u));
                if (color) CHECK(dst_col[at] == (inside ? src_col[from] : 0u));
            }
    free(src); free(src_col); free(dst); free(dst_col);
    return 0;
}

/* the documented loop: follow, window what leaves, shift into the other array */
static int walk(sgm_instance* s)
{
    sgm_volume_spec spec = volume_of(20, 17, 12);
    const size_t n = (size_t)20 * 17 * 12;
    uint32_t* vox[2] = {(uint32_t*)malloc(n * 4), (uint32_t*)malloc(n * 4)};
    uint32_t* col[2] = {(uint32_t*)malloc(n * 4), (uint32_t*)malloc(n * 4)};
    CHECK(vox[0] && vox[1] && col[0] && col[1]);
    for (size_t i = 0; i < n; ++i) {
        vox[0][i] = word_of(i, 3u);
        col[0][i] = word_of(i, 5u);
    }
    int cur = 0, moved = 0;
    for (int step = 0; step < 8; ++step) {
        const float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -0.21f * (float)step, 0.11f * (float)step, 0.02f * (float)step};
        int32_t shift[3];
        sgm_volume_box boxes[3];
        CHECK(sgm_volume_follow(&spec, pose, 0.875f, 4, 2, shift));
        const int count = sgm_volume_leaving(&spec, shift, boxes);
        CHECK(count >= 0 && count <= 3);
        for (int b = 0; b < count; ++b) {
            const size_t nb = (size_t)boxes[b].n[0] * boxes[b].n[1] * boxes[b].n[2];
            uint32_t* part = (uint32_t*)malloc(nb * 4);
            uint32_t* part_col = (uint32_t*)malloc(nb * 4);
            sgm_volume_spec part_spec;
            CHECK(part && part_col);
            CHECK(sgm_volume_window(s, &spec, boxes[b].lo, boxes[b].n, vox[cur], col[cur], part, part_col, &part_spec) && sgm_synchronize(s));
            CHECK(sgm_volume_bytes(&part_spec) == nb * 4);
            free(part); free(part_col);
        }
        if (shift[0] || shift[1] || shift[2]) {
            const int32_t dims[3] = {spec.nx, spec.ny, spec.nz};
            CHECK(sgm_volume_window(s, &spec, shift, dims, vox[cur], col[cur], vox[1 - cur], col[1 - cur], &spec) && sgm_synchronize(s));
            cur = 1 - cur;
            ++moved;
        }
    }
    CHECK(moved >= 2);
    free(vox[0]); free(vox[1]); free(col[0]); free(col[1]);
    return 0;
}

int main(void)
{
    static const int shapes[][3] = {{5, 3, 2}, {8, 4, 3}, {13, 5, 3}, {1, 1, 1}, {36, 7, 2}};
    static const int yz[][2] = {{0, 0}, {-1, 1}, {2, -1}, {-9, 0}, {0, 9}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t a = 0; a < sizeof shapes / sizeof shapes[0]; ++a)
        for (size_t b = 0; b < sizeof shapes / sizeof shapes[0]; ++b)
            for (int ox = -shapes[a][0] - 1; ox <= shapes[b][0] + 1; ++ox)
                for (size_t c = 0; c < sizeof yz / sizeof yz[0]; ++c) {
                    const int offset[3] = {ox, yz[c][0], yz[c][1]};
                    if (one(s, shapes[a], offset, shapes[b], (ox + (int)c) & 1) != 0) return 1;
                }
    {   /* the ends of the admitted sizes and offsets */
        static const int long_x[3] = {1024, 2, 2}, long_z[3] = {2, 2, 1024}, small[3] = {4, 4, 4};
        static const int far_off[3] = {1 << 20, -(1 << 20), 0}, back[3] = {-1020, 0, 0}, up[3] = {0, 0, 1021};
        if (one(s, long_x, back, long_x, 1) != 0 || one(s, long_z, up, long_z, 0) != 0 || one(s, small, far_off, small, 1) != 0) return 1;
        if (one(s, long_x, up, small, 0) != 0 || one(s, small, back, long_x, 1) != 0) return 1;
    }
    if (walk(s) != 0) return 1;
    /* refusals queue nothing */
    {
        uint32_t buf[80];                                          /* the four arrays of eight words, and room around them */
        uint32_t *a = buf + 8, *b = buf + 24, *c = buf + 40, *d = buf + 56;
        const sgm_volume_spec v = volume_of(2, 2, 2);
        sgm_volume_spec bad = v, out;
        const int32_t zero[3] = {0, 0, 0}, dims[3] = {2, 2, 2}, too_far[3] = {0, (1 << 20) + 1, 0}, none[3] = {2, 0, 2}, wide[3] = {1025, 1, 1};
        int32_t shift[3];
        sgm_volume_box boxes[3];
        const float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        float nan_pose[12];
        memset(buf, 0, sizeof buf);
        memcpy(nan_pose, pose, sizeof pose);
        nan_pose[4] = nanf("");
        bad.voxel = 0.0f;
        const int before = stub_window_count();
        CHECK(sgm_volume_window(s, &v, zero, dims, a, b, c, d, &out) && sgm_volume_window(s, &v, zero, dims, a, NULL, c, NULL, NULL));
        CHECK(!sgm_volume_window(NULL, &v, zero, dims, a, b, c, d, &out) && !sgm_volume_window(s, NULL, zero, dims, a, b, c, d, &out) &&
              !sgm_volume_window(s, &v, NULL, dims, a, b, c, d, &out) && !sgm_volume_window(s, &v, zero, NULL, a, b, c, d, &out) &&
              !sgm_volume_window(s, &v, zero, dims, NULL, b, c, d, &out) && !sgm_volume_window(s, &v, zero, dims, a, b, NULL, d, &out) &&
              !sgm_volume_window(s, &v, zero, dims, a, NULL, c, d, &out) && !sgm_volume_window(s, &v, zero, dims, a, b, c, NULL, &out) &&
              !sgm_volume_window(s, &bad, zero, dims, a, b, c, d, &out) && !sgm_volume_window(s, &v, zero, none, a, b, c, d, &out) &&
              !sgm_volume_window(s, &v, zero, wide, a, b, c, d, &out) && !sgm_volume_window(s, &v, too_far, dims, a, b, c, d, &out) &&
              !sgm_volume_window(s, &v, zero, dims, (uint32_t*)((char*)a + 2), b, c, d, &out) &&
              !sgm_volume_window(s, &v, zero, dims, a, b, c, (uint32_t*)((char*)d + 1), &out) &&
              !sgm_volume_window(s, &v, zero, dims, a, b, a, d, &out) && !sgm_volume_window(s, &v, zero, dims, a, b, c, c + 7, &out) &&
              !sgm_volume_window(s, &v, zero, dims, a, b, b + 7, d, &out) && !sgm_volume_window(s, &v, zero, dims, a, b, c, a - 7, &out));
        CHECK(!sgm_volume_window_spec(&bad, zero, dims, &out) && !sgm_volume_window_spec(&v, too_far, dims, &out) &&
              !sgm_volume_window_spec(&v, zero, none, &out) && !sgm_volume_window_spec(&v, zero, dims, NULL));
        CHECK(!sgm_volume_follow(&v, nan_pose, 0.0f, 4, 0, shift) && !sgm_volume_follow(&v, pose, 0.0f, 0, 0, shift) &&
              !sgm_volume_follow(&v, pose, 0.0f, 4, -1, shift) && !sgm_volume_follow(&bad, pose, 0.0f, 4, 0, shift) &&
              !sgm_volume_follow(&v, pose, 1e9f, 4, 0, shift) && !sgm_volume_follow(NULL, pose, 0.0f, 4, 0, shift));
        CHECK(sgm_volume_leaving(&bad, zero, boxes) == -1 && sgm_volume_leaving(&v, NULL, boxes) == -1 && sgm_volume_leaving(&v, zero, boxes) == 0);
        { const int32_t all[3] = {-(1 << 30) - (1 << 30), 1 << 30, 1}; CHECK(sgm_volume_leaving(&v, all, boxes) == 1); }
        CHECK(stub_window_count() == before + 2);
        stub_window_fail_at(0);
        CHECK(!sgm_volume_window(s, &v, zero, dims, a, b, c, d, &out));
        CHECK(sgm_volume_window(s, &v, zero, dims, a, b, c, d, &out) && sgm_synchronize(s));
    }
    /* behind matches, with and without the post pass on a stream of its own */
    for (int overlap = 0; overlap < 2; ++overlap) {
        const int w = 24, h = 16;
        const size_t n = (size_t)w * h;
        uint8_t* img = (uint8_t*)malloc(2 * n);
        float* disp = (float*)malloc(n * sizeof(float));
        static const int src_n[3] = {12, 6, 8}, offset[3] = {4, -1, 2};
        CHECK(img && disp);
        for (size_t k = 0; k < 2 * n; ++k) img[k] = (uint8_t)(k * 37u + (k >> 5));
        const SGMOption o = options(16);
        CHECK(sgm_set_overlap_post(s, overlap) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
        CHECK(sgm_match_device(s, img, img + n, disp));
        if (one(s, src_n, offset, src_n, 1) != 0) return 1;
        CHECK(sgm_synchronize(s));
        free(img); free(disp);
    }
    sgm_destroy(s);
    puts("window_sanitize_driver ok");
    return 0;
}
