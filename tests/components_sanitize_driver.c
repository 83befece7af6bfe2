/* TEST INFRASTRUCTURE (tests/test_zz_components_cpu.py): drives sgm_volume_components, sgm_volume_component_of, sgm_component_metric and
 * sgm_volume_components_bytes of the product's C host (csrc/sgm_host.c) with the stub device layer (tests/stub_device.c) and the
 * stand-in launchers (tests/stub_components.c, which compute for real) under AddressSanitizer / UBSan -- arrays allocated to the byte,
 * so that a word read or written outside one is seen; volumes of one voxel and of many, both sets, both connectivities, planes,
 * capacities around the number of components, refusals, a refused launch, behind matches with and without the post pass on a stream
 * of its own, and the lifetime of all of it.  A stand-alone program: nothing is loaded into another process.  The labels are checked
 * here as well, by a rule of their own: neighbours in the set carry the same label, a label names a voxel of its component that is
 * its smallest (tests/test_zz_components_cpu.py compares with the restatement). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "components_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_components_count(void);
void stub_components_fail_at(int nth);

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
    const sgm_volume_spec v = {nx, ny, nz, 0.25f, {0.0f, 0.0f, 0.0f}, 0.5f, 9};
    return v;
}

/* weights 0..3 and both signs, about one voxel in `sparse` occupied at min_weight 2 */
static uint32_t word_of(size_t i, uint32_t sparse)
{
    const uint32_t h = (uint32_t)(i * 2654435761u + 12345u) >> 7;
    const uint32_t w = h & 3u, tq = (h >> 2) % sparse == 0 ? 0x8000u | (h & 0x7FFu) : (h >> 9) & 0x7FFFu;
    return w << 16 | tq;
}

static int member_of(uint32_t word, int set, int unknown)
{
    const int observed = (word >> 16) >= 2u, neg = (word & 0x8000u) != 0;
    return observed ? (set ? !neg : neg) : unknown;
}

/* one volume in exactly allocated arrays: labels, records at three capacities, the objects of a small list */
static int one(sgm_instance* s, const int* n, int set, int unknown, int connectivity, uint32_t sparse)
{
    const sgm_volume_spec v = volume_of(n[0], n[1], n[2]);
    const size_t count = (size_t)n[0] * n[1] * n[2];
    CHECK(sgm_volume_components_bytes(&v) == 4 * count);
    uint32_t* vox = (uint32_t*)malloc(count * sizeof(uint32_t));
    uint32_t* lab = (uint32_t*)malloc(count * sizeof(uint32_t));
    CHECK(vox && lab);
    for (size_t i = 0; i < count; ++i) vox[i] = word_of(i, sparse);
    sgm_component_spec c;
    memset(&c, 0, sizeof c);
    c.min_weight = 2; c.set = set; c.unknown = unknown; c.connectivity = connectivity; c.min_voxels = 1;
    uint32_t counts[2] = {0xA5A5A5A5u, 0xA5A5A5A5u};
    memset(lab, 0xA5, count * sizeof(uint32_t));
    CHECK(sgm_volume_components(s, &v, &c, vox, lab, NULL, 0, counts) && sgm_synchronize(s));
    const uint32_t C = counts[0];
    CHECK(counts[1] == C && C <= count);
    uint32_t roots = 0;
    for (int k = 0; k < n[2]; ++k)
        for (int j = 0; j < n[1]; ++j)
            for (int i = 0; i < n[0]; ++i) {
                const size_t at = ((size_t)k * n[1] + j) * n[0] + i;
                const int in = member_of(vox[at], set, unknown);
                CHECK((lab[at] != 0) == in && lab[at] <= at + 1);
                if (!in) continue;
                roots += lab[at] == at + 1;
                CHECK(lab[lab[at] - 1] == lab[at]);
                for (int dk = -1; dk <= 1; ++dk)
                    for (int dj = -1; dj <= 1; ++dj)
                        for (int di = -1; di <= 1; ++di) {
                            const int steps = (di != 0) + (dj != 0) + (dk != 0), a = i + di, b = j + dj, d = k + dk;
                            if (steps == 0 || (connectivity == 6 && steps != 1) || a < 0 || b < 0 || d < 0 || a >= n[0] || b >= n[1] || d >= n[2]) continue;
                            const size_t to = ((size_t)d * n[1] + b) * n[0] + a;
                            if (member_of(vox[to], set, unknown)) CHECK(lab[to] == lab[at]);
                        }
            }
    CHECK(roots == C);
    for (int extra = -1; extra <= 1; ++extra) {
        if (extra < 0 && C == 0) continue;
        const size_t capacity = (size_t)((long)C + extra);
        sgm_component* obj = (sgm_component*)malloc(capacity ? capacity * sizeof(sgm_component) : 1);
        uint32_t* lab2 = (uint32_t*)malloc(count * sizeof(uint32_t));
        CHECK(obj && lab2);
        memset(obj, 0xA5, capacity * sizeof(sgm_component));
        CHECK(sgm_volume_components(s, &v, &c, vox, lab2, capacity ? obj : NULL, capacity, counts) && sgm_synchronize(s));
        CHECK(counts[0] == C && memcmp(lab, lab2, count * sizeof(uint32_t)) == 0);
        uint64_t voxels = 0;
        for (size_t q = 0; q < capacity && q < C; ++q) {
            CHECK(lab[obj[q].first] == obj[q].first + 1 && (q == 0 || obj[q - 1].first < obj[q].first) && obj[q].reserved == 0 && obj[q].voxels >= 1);
            float lo[3], hi[3], centroid[3];
            sgm_component_metric(&v, &obj[q], lo, hi, centroid);
            for (int a = 0; a < 3; ++a) CHECK(obj[q].lo[a] <= obj[q].hi[a] && obj[q].hi[a] < n[a] && lo[a] < centroid[a] && centroid[a] < hi[a]);
            voxels += obj[q].voxels;
        }
        if (capacity >= C) {
            uint64_t inside = 0;
            for (size_t i = 0; i < count; ++i) inside += lab[i] != 0;
            CHECK(voxels == inside);
            for (size_t q = C; q < capacity; ++q) CHECK(obj[q].first == 0xA5A5A5A5u);
            /* the objects of a list: one record per voxel, along x */
            sgm_surface_point* rec = (sgm_surface_point*)aligned_alloc(16, count * sizeof(sgm_surface_point));
            uint32_t* index = (uint32_t*)malloc(count * sizeof(uint32_t));
            uint32_t rc = (uint32_t)count;
            CHECK(rec && index);
            for (size_t i = 0; i < count; ++i) { rec[i].x = rec[i].y = rec[i].z = 0.0f; rec[i].id = (uint32_t)i * 4u; }
            CHECK(sgm_volume_component_of(s, &v, lab, capacity ? obj : NULL, capacity, counts, rec, count, &rc, 4, index) && sgm_synchronize(s));
            for (size_t i = 0; i < count; ++i) {
                uint32_t l = lab[i];
                if (l == 0 && (int)(i % (size_t)n[0]) + 1 < n[0]) l = lab[i + 1];
                CHECK((index[i] != 0) == (l != 0) && (l == 0 || obj[index[i] - 1].first + 1 == l));
            }
            free(rec); free(index);
        }
        free(obj); free(lab2);
    }
    free(vox); free(lab);
    return 0;
}

int main(void)
{
    static const int shapes[][3] = {{1, 1, 1}, {17, 1, 1}, {1, 17, 1}, {1, 1, 17}, {5, 3, 2}, {13, 5, 3}, {12, 11, 10}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t a = 0; a < sizeof shapes / sizeof shapes[0]; ++a)
        for (int set = 0; set < 2; ++set)
            for (int unknown = 0; unknown < 2; ++unknown)
                for (int conn = 6; conn <= 26; conn += 20)
                    if (one(s, shapes[a], set, unknown, conn, (a + (size_t)set) % 3 == 0 ? 1u : 5u) != 0) return 1;
    /* a floor taken out by its plane; refusals queue nothing */
    {
        enum { NX = 6, NY = 4, NZ = 3, N = NX * NY * NZ };
        uint32_t vox[N + 4], lab[N + 4], counts[4], index[8];
        sgm_component obj[4];
        sgm_surface_point rec[4];
        const sgm_volume_spec v = volume_of(NX, NY, NZ);
        sgm_volume_spec bad = v;
        bad.voxel = 0.0f;
        for (int i = 0; i < N + 4; ++i) vox[i] = 0x00020005u;
        for (int k = 0; k < NZ; ++k)
            for (int i = 0; i < NX; ++i) {
                vox[(k * NY + 0) * NX + i] = 0x00028000u;                                  /* the floor */
                if (i != 2 && i != 3) vox[(k * NY + 1) * NX + i] = vox[(k * NY + 2) * NX + i] = 0x00028000u;   /* two boxes on it */
            }
        sgm_component_spec c;
        memset(&c, 0, sizeof c);
        c.min_weight = 2; c.connectivity = 6; c.min_voxels = 1;
        CHECK(sgm_volume_components(s, &v, &c, vox, lab, obj, 4, counts) && sgm_synchronize(s) && counts[0] == 1 && obj[0].voxels == NZ * (NX + 2 * 4));
        c.planes = 2;                                              /* the first void, the second the floor: s == clearance in layer 0 */
        c.plane[1].normal[1] = 1.0f; c.plane[1].anchor[1] = 0.125f; c.clearance[1] = 0.0f; c.clearance[0] = 100.0f;
        CHECK(sgm_volume_components(s, &v, &c, vox, lab, obj, 4, counts) && sgm_synchronize(s) && counts[0] == 2 && counts[1] == 2);
        CHECK(obj[0].voxels == NZ * 4 && obj[1].voxels == NZ * 4 && obj[0].lo[1] == 1 && obj[1].lo[0] == 4 && lab[0] == 0);
        memset(rec, 0, sizeof rec);
        const int before = stub_components_count();
        sgm_component_spec w = c;
        CHECK(!sgm_volume_components(NULL, &v, &c, vox, lab, obj, 4, counts) && !sgm_volume_components(s, NULL, &c, vox, lab, obj, 4, counts) &&
              !sgm_volume_components(s, &v, NULL, vox, lab, obj, 4, counts) && !sgm_volume_components(s, &v, &c, NULL, lab, obj, 4, counts) &&
              !sgm_volume_components(s, &v, &c, vox, NULL, obj, 4, counts) && !sgm_volume_components(s, &v, &c, vox, lab, NULL, 4, counts) &&
              !sgm_volume_components(s, &v, &c, vox, lab, obj, 4, NULL) && !sgm_volume_components(s, &bad, &c, vox, lab, obj, 4, counts) &&
              !sgm_volume_components(s, &v, &c, vox, vox + 1, obj, 4, counts) && !sgm_volume_components(s, &v, &c, vox, lab, obj, 4, lab + N - 1) &&
              !sgm_volume_components(s, &v, &c, (uint32_t*)((char*)vox + 2), lab, obj, 4, counts) &&
              !sgm_volume_components(s, &v, &c, vox, lab, (sgm_component*)((char*)obj + 4), 3, counts));
        w.min_weight = 0; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts)); w = c;
        w.set = 2; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts)); w = c;
        w.unknown = -1; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts)); w = c;
        w.connectivity = 18; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts)); w = c;
        w.min_voxels = 0; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts)); w = c;
        w.planes = 5; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts)); w = c;
        w.clearance[1] = NAN; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts)); w = c;
        w.plane[0].anchor[2] = INFINITY; CHECK(!sgm_volume_components(s, &v, &w, vox, lab, obj, 4, counts));
        CHECK(!sgm_volume_component_of(NULL, &v, lab, obj, 4, counts, rec, 4, NULL, 4, index) &&
              !sgm_volume_component_of(s, &v, NULL, obj, 4, counts, rec, 4, NULL, 4, index) &&
              !sgm_volume_component_of(s, &v, lab, obj, 4, NULL, rec, 4, NULL, 4, index) &&
              !sgm_volume_component_of(s, &v, lab, obj, 4, counts, NULL, 4, NULL, 4, index) &&
              !sgm_volume_component_of(s, &v, lab, obj, 4, counts, rec, 4, NULL, 4, NULL) &&
              !sgm_volume_component_of(s, &v, lab, obj, 4, counts, rec, 4, NULL, 5, index) &&
              !sgm_volume_component_of(s, &bad, lab, obj, 4, counts, rec, 4, NULL, 4, index) &&
              !sgm_volume_component_of(s, &v, lab, obj, 4, counts, rec, 4, NULL, 4, lab + 2) &&
              !sgm_volume_component_of(s, &v, lab, obj, 4, counts, rec, 4, NULL, 4, (uint32_t*)rec));
        CHECK(sgm_volume_components_bytes(&bad) == 0 && sgm_volume_components_bytes(NULL) == 0 && sgm_volume_components_bytes(&v) == 4 * N);
        CHECK(stub_components_count() == before);
        sgm_component_metric(NULL, &obj[0], NULL, NULL, NULL);
        sgm_component_metric(&v, NULL, NULL, NULL, NULL);
        sgm_component_metric(&v, &obj[0], NULL, NULL, NULL);
        stub_components_fail_at(0);
        CHECK(!sgm_volume_components(s, &v, &c, vox, lab, obj, 4, counts));
        CHECK(sgm_volume_components(s, &v, &c, vox, lab, obj, 4, counts));
        stub_components_fail_at(0);
        CHECK(!sgm_volume_component_of(s, &v, lab, obj, 4, counts, rec, 4, NULL, 4, index));
        CHECK(sgm_volume_component_of(s, &v, lab, obj, 4, counts, rec, 4, NULL, 4, index) && sgm_synchronize(s));
        CHECK(sgm_volume_component_of(s, &v, lab, obj, 4, counts, NULL, 0, NULL, 4, NULL));
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
        if (one(s, dims, overlap, overlap, 26, 3u) != 0) return 1;
        CHECK(sgm_synchronize(s));
        free(img); free(disp);
    }
    sgm_destroy(s);
    puts("components_sanitize_driver ok");
    return 0;
}
