/* TEST INFRASTRUCTURE (tests/test_mesh_cpu.py): drives sgm_volume_mesh of the product's C host (csrc/sgm_host.c) with the stub device
 * layer (tests/stub_device.c) and the stand-in mesh launchers (tests/stub_mesh.c, which compute for real and use the tile scratch the
 * way the kernels do) under AddressSanitizer / UBSan -- volumes of one voxel, of one tile and of several, flat ones without a cell,
 * that grow and shrink on one instance, any words a caller may leave in a volume, a volume integrated by the stand-in of
 * sgm_volume_integrate, lists clipped by their capacities, counts-only calls, refusals, a refused launch, and the lifetime of all of
 * it.  A stand-alone program: nothing is loaded into another process.  Results are not checked here (tests/test_mesh_cpu.py does). */
#include "../include/sgm_mi355x.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "mesh_sanitize_driver: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int stub_mesh_count(void);
void stub_mesh_fail_at(int nth);

static sgm_volume_spec volume_of(int nx, int ny, int nz)
{
    const float voxel = 1.8f / (float)(nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz));
    const sgm_volume_spec v = {nx, ny, nz, voxel, {-0.5f * (float)nx * voxel, -0.5f * (float)ny * voxel, 0.5f}, 0.2f, 5};
    return v;
}

/* exactly the arrays the counts ask for: a record past either is an access the sanitizer reports */
static int mesh_exact(sgm_instance* s, const sgm_volume_spec* v, const uint32_t* voxels, uint32_t mw)
{
    uint32_t counts[2] = {0, 0}, again[2];
    CHECK(sgm_volume_mesh(s, v, voxels, mw, NULL, 0, NULL, 0, counts) && sgm_synchronize(s));
    const size_t nv = counts[0], nt = counts[1];
    sgm_mesh_vertex* vert = nv ? (sgm_mesh_vertex*)aligned_alloc(16, nv * sizeof *vert) : NULL;
    sgm_mesh_triangle* tri = nt ? (sgm_mesh_triangle*)aligned_alloc(16, nt * sizeof *tri) : NULL;
    CHECK((vert || !nv) && (tri || !nt));
    CHECK(sgm_volume_mesh(s, v, voxels, mw, vert, nv, tri, nt, again) && sgm_synchronize(s) && again[0] == nv && again[1] == nt);
    for (size_t i = 0; i < nt; ++i) CHECK(tri[i].v[0] < nv && tri[i].v[1] < nv && tri[i].v[2] < nv);
    /* one short of either: the vertex list clipped leaves the triangles alone, so a one-record array is enough for them */
    if (nv) CHECK(sgm_volume_mesh(s, v, voxels, mw, nv > 1 ? vert : NULL, nv - 1, tri, nt, again) && again[0] == nv);
    if (nt) CHECK(sgm_volume_mesh(s, v, voxels, mw, vert, nv, nt > 1 ? tri : NULL, nt - 1, again) && again[1] == nt);
    if (nv) CHECK(sgm_volume_mesh(s, v, voxels, mw, vert, nv, NULL, 0, again) && again[1] == nt);
    free(vert); free(tri);
    return 0;
}

static int run(sgm_instance* s, int nx, int ny, int nz)
{
    const size_t n = (size_t)nx * ny * nz;
    const sgm_volume_spec v = volume_of(nx, ny, nz);
    uint32_t* voxels = (uint32_t*)malloc(n * sizeof(uint32_t));
    CHECK(voxels);
    /* a sphere of negative tq around the middle, weights 1 and 2 in turn */
    for (size_t g = 0; g < n; ++g) {
        const float x = (float)(g % (size_t)nx) - 0.5f * (float)nx, y = (float)((g / (size_t)nx) % (size_t)ny) - 0.5f * (float)ny,
                    z = (float)(g / ((size_t)nx * ny)) - 0.5f * (float)nz;
        const float d = sqrtf(x * x + y * y + z * z) - 0.3f * (float)(nx < ny ? (nx < nz ? nx : nz) : (ny < nz ? ny : nz));
        const int tq = (int)(fmaxf(-1.0f, fminf(1.0f, d / 2.0f)) * 32767.0f);
        voxels[g] = ((uint32_t)(1 + g % 2) << 16) | ((uint32_t)tq & 0xFFFFu);
    }
    for (uint32_t mw = 1; mw <= 3; ++mw)
        if (mesh_exact(s, &v, voxels, mw) != 0) return 1;
    /* any words: every sign pattern, every weight */
    for (size_t g = 0; g < n; ++g) voxels[g] = (uint32_t)(g * 2654435761u) ^ (uint32_t)(g >> 3);
    for (uint32_t mw = 1; mw <= 65535; mw = mw * 16 + 15)
        if (mesh_exact(s, &v, voxels, mw) != 0) return 1;
    free(voxels);
    return 0;
}

/* a frame integrated by the stand-in of the volume, then meshed: the chain */
static int run_chain(sgm_instance* s)
{
    enum { W = 48, H = 20 };
    static const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const sgm_cloud_spec src = {W, H, 1, 27.0f, 27.0f, 23.5f, 9.5f, 40.0f / 27.0f, 0.0f, 0.1f, 100.0f, 0};
    const sgm_volume_spec v = volume_of(24, 12, 16);
    float* disp = (float*)malloc(W * H * sizeof(float));
    uint32_t* voxels = (uint32_t*)calloc(24 * 12 * 16, sizeof(uint32_t));
    CHECK(disp && voxels);
    for (int i = 0; i < W * H; ++i) disp[i] = 40.0f / (1.2f + 0.2f * sinf(0.3f * (float)(i % W)));
    CHECK(sgm_volume_integrate(s, &v, &src, identity, disp, NULL, NULL, voxels) && sgm_synchronize(s));
    if (mesh_exact(s, &v, voxels, 1) != 0) return 1;
    free(disp); free(voxels);
    return 0;
}

int main(void)
{
    /* one voxel, flat grids without a cell, one cell, less than a tile, exactly one, one more, three with the last partial; grow / shrink */
    static const int shapes[][3] = {{1, 1, 1}, {1, 9, 8}, {7, 1, 1}, {2, 2, 2}, {12, 11, 10}, {1024, 2, 1}, {683, 3, 1}, {20, 17, 13},
                                    {3, 2, 2}, {1024, 2, 2}, {9, 13, 7}, {40, 30, 20}};
    sgm_instance* s = sgm_create(0);
    CHECK(s);
    for (size_t i = 0; i < sizeof shapes / sizeof shapes[0]; ++i)
        if (run(s, shapes[i][0], shapes[i][1], shapes[i][2]) != 0) return 1;
    if (run_chain(s) != 0) return 1;
    /* refusals queue nothing; a refused launch leaves the instance usable */
    {
        uint32_t voxels[8] = {0x00010001u, 0x0001FFFFu, 0x00010001u, 0x00010001u, 0x00010001u, 0x00010001u, 0x00010001u, 0x0001FFFFu}, counts[2];
        sgm_mesh_vertex* vert = (sgm_mesh_vertex*)aligned_alloc(16, 56 * sizeof *vert);
        sgm_mesh_triangle* tri = (sgm_mesh_triangle*)aligned_alloc(16, 12 * sizeof *tri);
        CHECK(vert && tri);
        const sgm_volume_spec v = volume_of(2, 2, 2);
        const int before = stub_mesh_count();
        sgm_volume_spec bad = v;
        bad.nx = 1025;
        CHECK(!sgm_volume_mesh(s, &bad, voxels, 1, vert, 56, tri, 12, counts));
        bad = v; bad.nx = 1024; bad.ny = 1024; bad.nz = 129;
        CHECK(!sgm_volume_mesh(s, &bad, voxels, 1, NULL, 0, NULL, 0, counts));
        bad = v; bad.voxel = NAN;
        CHECK(!sgm_volume_mesh(s, &bad, voxels, 1, vert, 56, tri, 12, counts));
        CHECK(!sgm_volume_mesh(NULL, &v, voxels, 1, vert, 56, tri, 12, counts) && !sgm_volume_mesh(s, NULL, voxels, 1, vert, 56, tri, 12, counts) &&
              !sgm_volume_mesh(s, &v, NULL, 1, vert, 56, tri, 12, counts) && !sgm_volume_mesh(s, &v, voxels, 1, vert, 56, tri, 12, NULL) &&
              !sgm_volume_mesh(s, &v, voxels, 1, NULL, 56, tri, 12, counts) && !sgm_volume_mesh(s, &v, voxels, 1, vert, 56, NULL, 12, counts));
        CHECK(!sgm_volume_mesh(s, &v, voxels, 0, vert, 56, tri, 12, counts) && !sgm_volume_mesh(s, &v, voxels, 65536, vert, 56, tri, 12, counts));
        CHECK(!sgm_volume_mesh(s, &v, voxels, 1, (sgm_mesh_vertex*)((char*)vert + 4), 55, tri, 12, counts) &&
              !sgm_volume_mesh(s, &v, voxels, 1, vert, 56, (sgm_mesh_triangle*)((char*)tri + 8), 11, counts) &&
              !sgm_volume_mesh(s, &v, voxels, 1, vert, 56, tri, 12, (uint32_t*)((char*)counts + 2)));
        CHECK(!sgm_volume_mesh(s, &v, voxels, 1, vert, 56, tri, 12, voxels + 7) && !sgm_volume_mesh(s, &v, voxels, 1, vert, 56, tri, 12, (uint32_t*)(vert + 3)) &&
              !sgm_volume_mesh(s, &v, voxels, 1, vert, (size_t)-1, (sgm_mesh_triangle*)(vert + 55), 12, counts));
        CHECK(stub_mesh_count() == before);
        stub_mesh_fail_at(0);
        CHECK(!sgm_volume_mesh(s, &v, voxels, 1, vert, 56, tri, 12, counts));
        CHECK(sgm_volume_mesh(s, &v, voxels, 1, vert, 56, tri, 12, counts) && sgm_synchronize(s) && counts[0] > 0 && counts[1] > 0);
        free(vert); free(tri);
    }
    sgm_destroy(s);
    puts("mesh_sanitize_driver ok");
    return 0;
}
