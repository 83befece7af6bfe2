/* TEST INFRASTRUCTURE (tests/test_distance_cpu.py): drives sgm_volume_distance, sgm_volume_distance_field and
 * sgm_volume_distance_bytes of the product's C host (csrc/sgm_host.c) with the stub device layer (tests/stub_device.c) and the
 * stand-in launchers (tests/stub_distance.c, which compute for real) under AddressSanitizer / UBSan -- arrays allocated to the byte,
 * so that a word read or written outside one is seen; volumes of one voxel and of many, both sides, both readings of unknown space,
 * the smallest and the largest radius, the signed and the unsigned field, refusals, a refused launch, behind matches with and
 * without the post pass on a stream of its own, and the lifetime of all of it.  A stand-alone program: nothing is loaded into
 * another process.  The rules are checked here as well, by a search of its own (tests/test_distance_cpu.py compares with the
 * restatement). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "distance_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_distance_count(void);
void stub_distance_fail_at(int nth);

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

/* weights 0..3 and both signs, about one voxel in `sparse` occupied at min_weight 2 */
static uint32_t word_of(size_t i, uint32_t sparse)
{
    const uint32_t h = (uint32_t)(i * 2654435761u + 12345u) >> 7;
    const uint32_t w = h & 3u, tq = (h >> 2) % sparse == 0 ? 0x8000u | (h & 0x7FFu) : (h >> 9) & 0x7FFFu;
    return w << 16 | tq;
}

static int site_of(uint32_t word, uint32_t min_weight, int side, int unknown)
{
    const int observed = (word >> 16) >= min_weight;
    const int in_o = observed ? (word & 0x8000u) != 0 : unknown;
    return side ? !in_o : in_o;
}

/* both sides and the field of one volume in exactly allocated arrays, every word checked against a search over all voxels */
static int one(sgm_instance* s, const int* n, int radius, int unknown, uint32_t sparse)
{
    const sgm_volume_spec v = volume_of(n[0], n[1], n[2]);
    const size_t count = (size_t)n[0] * n[1] * n[2];
    CHECK(sgm_volume_distance_bytes(&v) == 2 * count);
    uint32_t* vox = (uint32_t*)malloc(count * sizeof(uint32_t));
    uint16_t* side2[2] = {(uint16_t*)malloc(count * sizeof(uint16_t)), (uint16_t*)malloc(count * sizeof(uint16_t))};
    float* field = (float*)malloc(count * sizeof(float));
    CHECK(vox && side2[0] && side2[1] && field);
    for (size_t i = 0; i < count; ++i) vox[i] = word_of(i, sparse);
    for (int side = 0; side < 2; ++side) {
        const sgm_distance_spec d = {2, radius, side, unknown};
        memset(side2[side], 0xA5, count * sizeof(uint16_t));
        CHECK(sgm_volume_distance(s, &v, &d, vox, side2[side]) && sgm_synchronize(s));
        for (int k = 0; k < n[2]; ++k)
            for (int j = 0; j < n[1]; ++j)
                for (int i = 0; i < n[0]; ++i) {
                    long best = -1;
                    for (int c = 0; c < n[2]; ++c)
                        for (int b = 0; b < n[1]; ++b)
                            for (int a = 0; a < n[0]; ++a)
                                if (site_of(vox[((size_t)c * n[1] + b) * n[0] + a], 2, side, unknown)) {
                                    const long m = (long)(i - a) * (i - a) + (long)(j - b) * (j - b) + (long)(k - c) * (k - c);
                                    if (best < 0 || m < best) best = m;
                                }
                    const unsigned want = (best >= 0 && best <= (long)radius * radius) ? (unsigned)best : SGM_DISTANCE_FAR;
                    CHECK(side2[side][((size_t)k * n[1] + j) * n[0] + i] == want);
                }
    }
    for (int is_signed = 1; is_signed >= 0; --is_signed) {
        CHECK(sgm_volume_distance_field(s, &v, side2[0], is_signed ? side2[1] : NULL, field) && sgm_synchronize(s));
        for (size_t i = 0; i < count; ++i) {
            const unsigned o = side2[0][i], in = side2[1][i];
            CHECK(!(o == 0 && in == 0));
            if (o == SGM_DISTANCE_FAR) CHECK(isinf(field[i]) && field[i] > 0);
            else if (o > 0) CHECK(field[i] == v.voxel * sqrtf((float)o));
            else if (!is_signed) CHECK(field[i] == 0.0f);
            else if (in == SGM_DISTANCE_FAR) CHECK(isinf(field[i]) && field[i] < 0);
            else CHECK(field[i] == -(v.voxel * sqrtf((float)in)));
        }
    }
    free(vox); free(side2[0]); free(side2[1]); free(field);
    return 0;
}

int main(void)
{
    static const int shapes[][3] = {{1, 1, 1}, {17, 1, 1}, {1, 17, 1}, {1, 1, 17}, {5, 3, 2}, {13, 5, 3}, {12, 11, 10}};
    static const int radii[] = {1, 2, 3, 255};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t a = 0; a < sizeof shapes / sizeof shapes[0]; ++a)
        for (size_t r = 0; r < sizeof radii / sizeof radii[0]; ++r)
            for (int unknown = 0; unknown < 2; ++unknown)
                if (one(s, shapes[a], radii[r], unknown, (a + r) % 3 == 0 ? 1u : 23u) != 0) return 1;
    /* refusals queue nothing */
    {
        uint32_t vox[12];                                          /* eight voxels, and room around them */
        uint16_t words[48];
        float field[16];
        uint16_t *a = words + 4, *b = words + 20;
        const sgm_volume_spec v = volume_of(2, 2, 2);
        sgm_volume_spec bad = v;
        const sgm_distance_spec d = {1, 3, 0, 0}, light = {0, 3, 0, 0}, heavy = {65536, 3, 0, 0}, near = {1, 0, 0, 0}, wide = {1, 256, 0, 0},
                                other = {1, 3, 2, 0}, dark = {1, 3, 0, -1};
        memset(vox, 0, sizeof vox);
        memset(words, 0, sizeof words);
        bad.voxel = 0.0f;
        const int before = stub_distance_count();
        CHECK(sgm_volume_distance(s, &v, &d, vox + 2, a) && sgm_volume_distance_field(s, &v, a, b, field + 4) &&
              sgm_volume_distance_field(s, &v, a, NULL, field + 4) && sgm_volume_distance_field(s, &v, a, a, field + 4));
        CHECK(!sgm_volume_distance(NULL, &v, &d, vox + 2, a) && !sgm_volume_distance(s, NULL, &d, vox + 2, a) &&
              !sgm_volume_distance(s, &v, NULL, vox + 2, a) && !sgm_volume_distance(s, &v, &d, NULL, a) && !sgm_volume_distance(s, &v, &d, vox + 2, NULL) &&
              !sgm_volume_distance(s, &bad, &d, vox + 2, a) && !sgm_volume_distance(s, &v, &light, vox + 2, a) &&
              !sgm_volume_distance(s, &v, &heavy, vox + 2, a) && !sgm_volume_distance(s, &v, &near, vox + 2, a) &&
              !sgm_volume_distance(s, &v, &wide, vox + 2, a) && !sgm_volume_distance(s, &v, &other, vox + 2, a) &&
              !sgm_volume_distance(s, &v, &dark, vox + 2, a) && !sgm_volume_distance(s, &v, &d, (uint32_t*)((char*)vox + 2), a) &&
              !sgm_volume_distance(s, &v, &d, vox + 2, (uint16_t*)((char*)a + 1)) && !sgm_volume_distance(s, &v, &d, vox + 2, (uint16_t*)(vox + 2)) &&
              !sgm_volume_distance(s, &v, &d, vox + 2, (uint16_t*)(vox + 2) - 3) && !sgm_volume_distance(s, &v, &d, vox + 2, (uint16_t*)(vox + 10) - 1));
        CHECK(!sgm_volume_distance_field(NULL, &v, a, b, field + 4) && !sgm_volume_distance_field(s, NULL, a, b, field + 4) &&
              !sgm_volume_distance_field(s, &v, NULL, b, field + 4) && !sgm_volume_distance_field(s, &v, a, b, NULL) &&
              !sgm_volume_distance_field(s, &bad, a, b, field + 4) && !sgm_volume_distance_field(s, &v, (uint16_t*)((char*)a + 1), b, field + 4) &&
              !sgm_volume_distance_field(s, &v, a, (uint16_t*)((char*)b + 1), field + 4) &&
              !sgm_volume_distance_field(s, &v, a, b, (float*)((char*)field + 18)) && !sgm_volume_distance_field(s, &v, a, b, (float*)a) &&
              !sgm_volume_distance_field(s, &v, a, (uint16_t*)(field + 12) - 1, field + 4) &&
              !sgm_volume_distance_field(s, &v, (uint16_t*)(field + 4) - 7, b, field + 4));
        CHECK(sgm_volume_distance_bytes(&bad) == 0 && sgm_volume_distance_bytes(NULL) == 0 && sgm_volume_distance_bytes(&v) == 16);
        CHECK(stub_distance_count() == before + 4);
        stub_distance_fail_at(0);
        CHECK(!sgm_volume_distance(s, &v, &d, vox + 2, a));
        stub_distance_fail_at(0);
        CHECK(!sgm_volume_distance_field(s, &v, a, b, field + 4));
        CHECK(sgm_volume_distance(s, &v, &d, vox + 2, a) && sgm_volume_distance_field(s, &v, a, b, field + 4) && sgm_synchronize(s));
    }
    /* behind matches, with and without the post pass on a stream of its own */
    for (int overlap = 0; overlap < 2; ++overlap) {
        const int w = 24, h = 16;
        const size_t n = (size_t)w * h;
        uint8_t* img = (uint8_t*)malloc(2 * n);
        float* disp = (float*)malloc(n * sizeof(float));
        static const int dims[3] = {12, 6, 8};
        CHECK(img && disp);
        for (size_t k = 0; k < 2 * n; ++k) img[k] = (uint8_t)(k * 37u + (k >> 5));
        const SGMOption o = options(16);
        CHECK(sgm_set_overlap_post(s, overlap) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &o));
        CHECK(sgm_match_device(s, img, img + n, disp));
        if (one(s, dims, 4, overlap, 11u) != 0) return 1;
        CHECK(sgm_synchronize(s));
        free(img); free(disp);
    }
    sgm_destroy(s);
    puts("distance_sanitize_driver ok");
    return 0;
}
