/* TEST INFRASTRUCTURE (tests/test_plane_cpu.py): drives sgm_plane_votes, sgm_plane_best, sgm_plane_sums, sgm_plane_label,
 * sgm_plane_solve and sgm_plane_fit of the product's C host (csrc/sgm_host.c) with the stub device layer (tests/stub_device.c) and
 * the stand-in launchers (tests/stub_plane.c, which compute for real) under AddressSanitizer / UBSan -- lists of 0, 1, 2, 3 and a few
 * thousand records in buffers of exactly their size, with and without a count word and labels, every number of candidates at the
 * ends of its range, records full of non-finite and huge coordinates, collinear and coplanar lists, every number of rounds, with
 * and without traces, a prior, behind a match with the post pass on a stream of its own, refusals, refused launches, and the
 * lifetime of all of it.  A stand-alone program: nothing is loaded into another process.  Results are not checked here
 * (tests/test_plane_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "plane_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_plane_count(void);
void stub_plane_fail_at(int nth);

static SGMOption options(int d)
{
    SGMOption o;
    memset(&o, 0, sizeof o);
    o.num_paths = 8; o.min_disparity = 0; o.max_disparity = (uint16_t)d;
    o.is_check_lr = true; o.lrcheck_thres = 1.0f; o.is_check_unique = true; o.uniqueness_ratio = 0.99;
    o.is_remove_speckles = true; o.min_speckle_area = 20; o.p1 = 10; o.p2_init = 150;
    return o;
}

static sgm_plane_spec spec_of(int k, int iterations, int prior)
{
    const sgm_plane_spec sp = {k, 17u, 0.02f, {0.0f, prior ? 2.0f : 0.0f, prior ? 1.0f : 0.0f}, prior ? 0.3f : 0.0f, 1.5f, iterations, 3u, 1e-9f};
    return sp;
}

/* kind 0: a floor, a wall and stray points; 1: one line; 2: one plane; 3: the floor among non-finite and huge coordinates */
static void fill(sgm_point* r, size_t n, int kind)
{
    for (size_t i = 0; i < n; ++i) {
        const float u = (float)(i % 37) * 0.05f - 0.9f, v = (float)(i % 53) * 0.03f - 0.8f, e = (float)((int)(i % 5) - 2) * 0.004f;
        if (kind == 1) r[i] = (sgm_point){u, 2.0f * u, 1.0f + 0.5f * u, (uint32_t)i};
        else if (kind == 2) r[i] = (sgm_point){u, v, 2.0f, (uint32_t)i};
        else if (i % 10 < 6) r[i] = (sgm_point){u, 0.5f + e, 2.0f + v, (uint32_t)i};
        else if (i % 10 < 9) r[i] = (sgm_point){u, v, 3.0f + e, (uint32_t)i};
        else r[i] = (sgm_point){3.0f * u, 2.0f * v, 1.0f + u * v, (uint32_t)i};
        if (kind == 3 && i % 7 == 0) r[i].x = (i % 3 == 0) ? NAN : (i % 3 == 1 ? INFINITY : 3e38f);
        if (kind == 3 && i % 11 == 0) r[i].z = (i % 2 == 0) ? -INFINITY : 1e-40f;
    }
}

static int run(sgm_instance* s, size_t n, int kind, int k, int iterations, int prior, int with_count, int with_labels)
{
    sgm_point* rec = (sgm_point*)aligned_alloc(16, (n ? n : 1) * sizeof(sgm_point));
    uint8_t* labels = (uint8_t*)malloc(n ? n : 1);
    uint32_t* count = (uint32_t*)malloc(sizeof(uint32_t));
    sgm_plane* planes = (sgm_plane*)aligned_alloc(16, (size_t)k * sizeof(sgm_plane));
    sgm_plane* best = (sgm_plane*)aligned_alloc(16, sizeof(sgm_plane));
    int64_t* sums = (int64_t*)malloc(10 * sizeof(int64_t));
    int64_t* trace_sums = (int64_t*)malloc((size_t)iterations * 10 * sizeof(int64_t));
    sgm_plane* trace_planes = (sgm_plane*)malloc((size_t)(iterations + 1) * sizeof(sgm_plane));
    CHECK(rec && labels && count && planes && best && sums && trace_sums && trace_planes);
    fill(rec, n, kind);
    for (size_t i = 0; i < n; ++i) labels[i] = (uint8_t)(i % 13 == 0 ? 7 : 0);
    *count = (uint32_t)(n > 5 ? n - 5 : n);
    const sgm_plane_spec sp = spec_of(k, iterations, prior);
    const uint32_t* c = with_count ? count : NULL;
    CHECK(sgm_plane_votes(s, &sp, rec, n, c, with_labels ? labels : NULL, planes));
    CHECK(sgm_plane_best(s, planes, k, best));
    CHECK(sgm_plane_sums(s, &sp, rec, n, c, with_labels ? labels : NULL, best, sums));
    CHECK(sgm_plane_label(s, &sp, rec, n, c, best, 200, labels));
    sgm_plane out;
    sgm_plane_stats stats;
    if (best->normal[0] != 0.0f || best->normal[1] != 0.0f || best->normal[2] != 0.0f) CHECK(sgm_plane_solve(&sp, sums, best, &out, &stats));
    CHECK(sgm_plane_fit(s, &sp, rec, n, c, with_labels ? labels : NULL, &out, &stats, trace_sums, trace_planes));
    CHECK(sgm_plane_fit(s, &sp, rec, n, c, NULL, &out, &stats, NULL, NULL));
    CHECK(stats.status >= 0 && stats.status <= 2);
    CHECK(sgm_synchronize(s));
    free(rec); free(labels); free(count); free(planes); free(best); free(sums); free(trace_sums); free(trace_planes);
    return 0;
}

int main(void)
{
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    static const size_t sizes[] = {0, 1, 2, 3, 4, 63, 64, 65, 257, 3000};
    for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; ++i)
        for (int kind = 0; kind < 4; ++kind)
            if (run(s, sizes[i], kind, (int)(1 + 37 * i), 1 + (int)i, kind == 2, (int)(i & 1), kind != 1) != 0) return 1;
    if (run(s, 500, 0, 1024, 64, 1, 1, 1) != 0 || run(s, 500, 3, 1, 1, 0, 0, 0) != 0) return 1;

    /* behind a match whose post pass runs on a stream of its own */
    SGMOption opt = options(16);
    const int w = 24, h = 16;
    uint8_t* img = (uint8_t*)calloc((size_t)w * h, 1);
    float* disp = (float*)calloc((size_t)w * h, sizeof(float));
    CHECK(img && disp && sgm_set_overlap_post(s, 1) && sgm_initialize(s, (uint16_t)w, (uint16_t)h, &opt));
    CHECK(sgm_match_device(s, img, img, disp));
    if (run(s, 300, 0, 16, 3, 0, 1, 1) != 0) return 1;

    /* refusals queue nothing; refused launches fail the calls */
    sgm_point* rec = (sgm_point*)aligned_alloc(16, 128 * sizeof(sgm_point));
    sgm_plane* planes = (sgm_plane*)aligned_alloc(16, 8 * sizeof(sgm_plane));
    uint8_t labels[128] = {0};
    int64_t sums[10];
    sgm_plane out;
    sgm_plane_stats stats;
    CHECK(rec && planes);
    fill(rec, 128, 0);
    sgm_plane_spec sp = spec_of(8, 2, 0);
    const int before = stub_plane_count();
    sgm_plane_spec bad = sp;
    bad.dist = -1.0f;
    CHECK(!sgm_plane_votes(s, &bad, rec, 128, NULL, NULL, planes) && !sgm_plane_votes(s, &sp, NULL, 128, NULL, NULL, planes));
    CHECK(!sgm_plane_votes(s, &sp, rec, 128, NULL, NULL, (sgm_plane*)((char*)planes + 8)));
    CHECK(!sgm_plane_votes(s, &sp, rec, 128, NULL, NULL, (sgm_plane*)(rec + 1)) && !sgm_plane_best(s, planes, 8, planes + 7));
    CHECK(!sgm_plane_best(s, planes, 0, planes) && !sgm_plane_sums(s, &sp, rec, ((size_t)1 << 24) + 1, NULL, NULL, planes, sums));
    CHECK(!sgm_plane_sums(s, &sp, rec, 128, NULL, NULL, planes, (int64_t*)rec) && !sgm_plane_label(s, &sp, rec, 128, NULL, planes, 0, labels));
    CHECK(!sgm_plane_label(s, &sp, rec, 128, NULL, planes, 1, (uint8_t*)rec + 5) && !sgm_plane_fit(s, &sp, rec, 128, NULL, NULL, NULL, &stats, NULL, NULL));
    CHECK(!sgm_plane_solve(&sp, NULL, planes, &out, &stats));
    CHECK(stub_plane_count() == before);
    for (int nth = 0; nth < 4; ++nth) {
        stub_plane_fail_at(nth);
        CHECK(!sgm_plane_fit(s, &sp, rec, 128, NULL, labels, &out, &stats, NULL, NULL));
    }
    stub_plane_fail_at(0);
    CHECK(!sgm_plane_votes(s, &sp, rec, 128, NULL, NULL, planes));
    CHECK(sgm_plane_fit(s, &sp, rec, 128, NULL, labels, &out, &stats, NULL, NULL));
    free(rec); free(planes); free(img); free(disp);
    sgm_destroy(s);
    printf("plane_sanitize_driver ok\n");
    return 0;
}
