/*
 * stub_mesh.c -- TEST INFRASTRUCTURE ONLY (tests/test_mesh_cpu.py and tests/test_driver_mesh.py build it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_mesh.hip: sgmd_mesh_scratch_bytes and sgmd_volume_mesh, which csrc/sgm_host.c references weakly.  A host
 * linked without this file has no mesh.  It keeps a log of its own: the spec, the capacities and the pointers of every call, and it
 * can be told to refuse the n-th call.  While the volume fits the allocator's cap of stub_device.c (1 MiB) it computes for real --
 * plain C float arithmetic, built with -ffp-contract=off -- so that a sanitizer build sees every word read and every record
 * written.  It carries no table: the triangles of a tetrahedron and their winding come from the contract's midpoint rule, in
 * integers (midpoints doubled, centroids scaled).  It touches its scratch the way the kernels do: two sets of a count and a base
 * per tile of 2048 voxels; a scratch sized too small is an access the sanitizer reports.
 */
#include "sgm_device.h"

#include <string.h>

#define MESH_LOG_MAX 256
#define CAP ((size_t)1 << 20)
#define TILE 2048
static struct {
    unsigned min_weight;
    size_t capacity[2];
    sgmd_volume v;
    const void* p[5];
} g_calls[MESH_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_mesh_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_mesh_count(void) { return g_calls_n; }
/* which: 0 voxels, 1 scratch, 2 vertices, 3 triangles, 4 counts */
const void* stub_mesh_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 5) ? g_calls[call].p[which] : NULL; }
const sgmd_volume* stub_mesh_spec(int call) { return (call >= 0 && call < g_calls_n) ? &g_calls[call].v : NULL; }
unsigned stub_mesh_min_weight(int call) { return (call >= 0 && call < g_calls_n) ? g_calls[call].min_weight : 0; }
size_t stub_mesh_capacity(int call, int which) { return (call >= 0 && call < g_calls_n && (which == 0 || which == 1)) ? g_calls[call].capacity[which] : 0; }
/* the nth (0-based) call from now on returns an error */
void stub_mesh_fail_at(int nth) { g_refuse_countdown = nth; }

size_t sgmd_mesh_scratch_bytes(int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    return 4 * sizeof(unsigned) * (((size_t)nx * ny * nz + TILE - 1) / TILE);
}

static const int KIND[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
static const int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

static int tq_of(uint32_t word) { return (int)(int16_t)(word & 0xFFFFu); }
static float centre(float o, int i, float voxel) { return o + ((float)i + 0.5f) * voxel; }

typedef struct { const sgmd_volume* v; const uint32_t* voxels; unsigned min_weight; } volume;

static int counts_at(const volume* m, int i, int j, int k)
{
    return i < m->v->nx && j < m->v->ny && k < m->v->nz && (m->voxels[((size_t)k * m->v->ny + j) * m->v->nx + i] >> 16) >= m->min_weight;
}
static int tq_at(const volume* m, int i, int j, int k) { return tq_of(m->voxels[((size_t)k * m->v->ny + j) * m->v->nx + i]); }

/* edge (n, e) carries a vertex */
static int vertex_at(const volume* m, int i, int j, int k, int e)
{
    const int fi = i + KIND[e][0], fj = j + KIND[e][1], fk = k + KIND[e][2];
    return counts_at(m, i, j, k) && counts_at(m, fi, fj, fk) && (tq_at(m, i, j, k) < 0) != (tq_at(m, fi, fj, fk) < 0);
}

static void tet_corners(int t, int p[4][3])
{
    memset(p[0], 0, sizeof p[0]);
    for (int s = 0; s < 3; ++s) {
        memcpy(p[s + 1], p[s], sizeof p[0]);
        p[s + 1][PERM[t][s]] = 1;
    }
}

/* the wound triangles of tetrahedron t with the sign mask: edges as corner pairs (lower first); returns how many */
static int case_triangles(int t, int mask, int tri[2][3][2])
{
    int N[4], P[4], nn = 0, np = 0, p[4][3];
    for (int c = 0; c < 4; ++c) { if (mask >> c & 1) N[nn++] = c; else P[np++] = c; }
    if (nn == 0 || nn == 4) return 0;
    int count = 1;
    if (nn == 1) {
        for (int q = 0; q < 3; ++q) { tri[0][q][0] = N[0]; tri[0][q][1] = P[q]; }
    } else if (nn == 3) {
        for (int q = 0; q < 3; ++q) { tri[0][q][0] = P[0]; tri[0][q][1] = N[q]; }
    } else {
        const int a = N[0], b = N[1], c = P[0], d = P[1];
        const int two[2][3][2] = {{{a, c}, {a, d}, {b, d}}, {{a, c}, {b, d}, {b, c}}};
        memcpy(tri, two, sizeof two);
        count = 2;
    }
    tet_corners(t, p);
    int away[3];                                                  /* nn * np * (centroid(P) - centroid(N)) */
    for (int d = 0; d < 3; ++d) {
        int sp = 0, sn = 0;
        for (int q = 0; q < np; ++q) sp += p[P[q]][d];
        for (int q = 0; q < nn; ++q) sn += p[N[q]][d];
        away[d] = nn * sp - np * sn;
    }
    for (int k = 0; k < count; ++k) {
        int m[3][3];                                              /* twice the midpoints */
        for (int q = 0; q < 3; ++q) {
            if (tri[k][q][0] > tri[k][q][1]) { const int s = tri[k][q][0]; tri[k][q][0] = tri[k][q][1]; tri[k][q][1] = s; }
            for (int d = 0; d < 3; ++d) m[q][d] = p[tri[k][q][0]][d] + p[tri[k][q][1]][d];
        }
        const int u[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]}, w[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
        const int dot = (u[1] * w[2] - u[2] * w[1]) * away[0] + (u[2] * w[0] - u[0] * w[2]) * away[1] + (u[0] * w[1] - u[1] * w[0]) * away[2];
        if (dot < 0) {
            int s[2];
            memcpy(s, tri[k][1], sizeof s); memcpy(tri[k][1], tri[k][2], sizeof s); memcpy(tri[k][2], s, sizeof s);
        }
    }
    return count;
}

/* the triangles of cell (i, j, k) as vertex ids; returns how many (0 where the cell does not exist or is not meshed) */
static int cell_triangles(const volume* m, int i, int j, int k, uint32_t ids[12][3])
{
    int count = 0;
    for (int c = 0; c < 8; ++c)
        if (!counts_at(m, i + (c & 1), j + (c >> 1 & 1), k + (c >> 2))) return 0;
    for (int t = 0; t < 6; ++t) {
        int p[4][3], mask = 0, tri[2][3][2];
        tet_corners(t, p);
        for (int c = 0; c < 4; ++c) mask |= (tq_at(m, i + p[c][0], j + p[c][1], k + p[c][2]) < 0) << c;
        const int here = case_triangles(t, mask, tri);
        for (int q = 0; q < here; ++q, ++count) {
            for (int e = 0; e < 3; ++e) {
                const int* lo = p[tri[q][e][0]];
                const int* hi = p[tri[q][e][1]];
                int kind = 0;
                while (KIND[kind][0] != hi[0] - lo[0] || KIND[kind][1] != hi[1] - lo[1] || KIND[kind][2] != hi[2] - lo[2]) ++kind;
                ids[count][e] = (uint32_t)((((size_t)(k + lo[2]) * m->v->ny + (j + lo[1])) * m->v->nx + (i + lo[0])) * 8 + (size_t)kind);
            }
        }
    }
    return count;
}

typedef struct { float c[3]; uint32_t id; } vertex;
typedef struct { uint32_t v[3], cell; } triangle;

int sgmd_volume_mesh(int o, void* st, const sgmd_volume* v, const void* voxels_, unsigned min_weight, void* scratch, void* vertices_,
                     size_t vertex_capacity, void* triangles_, size_t triangle_capacity, void* counts_)
{
    (void)o; (void)st;
    if (g_calls_n < MESH_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].min_weight = min_weight;
        g_calls[g_calls_n].capacity[0] = vertex_capacity;
        g_calls[g_calls_n].capacity[1] = triangle_capacity;
        g_calls[g_calls_n].v = *v;
        const void* p[5] = {voxels_, scratch, vertices_, triangles_, counts_};
        memcpy(g_calls[g_calls_n++].p, p, sizeof p);
    }
    if (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) return 719;
    const size_t n = (size_t)v->nx * v->ny * v->nz, ntiles = (n + TILE - 1) / TILE;
    if (n * 4 > CAP) return 0;
    const volume m = {v, (const uint32_t*)voxels_, min_weight};
    unsigned* kept_v = (unsigned*)scratch;
    unsigned* base_v = kept_v + ntiles;
    unsigned* kept_t = base_v + ntiles;
    unsigned* base_t = kept_t + ntiles;
    uint32_t ids[12][3];
    for (size_t t = 0; t < ntiles; ++t) {                         /* count */
        kept_v[t] = kept_t[t] = 0;
        for (size_t g = t * TILE; g < n && g < (t + 1) * TILE; ++g) {
            const int i = (int)(g % (size_t)v->nx), j = (int)((g / (size_t)v->nx) % (size_t)v->ny), k = (int)(g / ((size_t)v->nx * v->ny));
            for (int e = 0; e < 7; ++e) kept_v[t] += (unsigned)vertex_at(&m, i, j, k, e);
            kept_t[t] += (unsigned)cell_triangles(&m, i, j, k, ids);
        }
    }
    unsigned run_v = 0, run_t = 0;
    for (size_t t = 0; t < ntiles; ++t) { base_v[t] = run_v; run_v += kept_v[t]; base_t[t] = run_t; run_t += kept_t[t]; }      /* scan */
    ((uint32_t*)counts_)[0] = run_v;
    ((uint32_t*)counts_)[1] = run_t;
    vertex* vertices = (vertex*)vertices_;
    triangle* triangles = (triangle*)triangles_;
    for (size_t t = 0; t < ntiles && vertex_capacity; ++t) {      /* the vertices */
        size_t to = base_v[t];
        for (size_t g = t * TILE; g < n && g < (t + 1) * TILE; ++g) {
            const int i = (int)(g % (size_t)v->nx), j = (int)((g / (size_t)v->nx) % (size_t)v->ny), k = (int)(g / ((size_t)v->nx * v->ny));
            for (int e = 0; e < 7; ++e) {
                if (!vertex_at(&m, i, j, k, e)) continue;
                const float tn = (float)tq_at(&m, i, j, k), tm = (float)tq_at(&m, i + KIND[e][0], j + KIND[e][1], k + KIND[e][2]);
                const float s = tn / (tn - tm), step = s * v->voxel;
                vertex q = {{centre(v->origin[0], i, v->voxel), centre(v->origin[1], j, v->voxel), centre(v->origin[2], k, v->voxel)},
                            (uint32_t)(g * 8 + (size_t)e)};
                for (int d = 0; d < 3; ++d) if (KIND[e][d]) q.c[d] = q.c[d] + step;
                if (to < vertex_capacity) vertices[to] = q;
                ++to;
            }
        }
    }
    if ((size_t)run_v > vertex_capacity) return 0;                /* a truncated vertex list: no triangle */
    for (size_t t = 0; t < ntiles && triangle_capacity; ++t) {    /* the triangles */
        size_t to = base_t[t];
        for (size_t g = t * TILE; g < n && g < (t + 1) * TILE; ++g) {
            const int i = (int)(g % (size_t)v->nx), j = (int)((g / (size_t)v->nx) % (size_t)v->ny), k = (int)(g / ((size_t)v->nx * v->ny));
            const int here = cell_triangles(&m, i, j, k, ids);
            for (int q = 0; q < here; ++q, ++to) {
                if (to >= triangle_capacity) continue;
                triangle r;
                for (int e = 0; e < 3; ++e) {                     /* binary search of the id in the written list */
                    size_t lo = 0, hi = run_v;
                    while (lo + 1 < hi) {
                        const size_t mid = lo + (hi - lo) / 2;
                        if (vertices[mid].id <= ids[q][e]) lo = mid; else hi = mid;
                    }
                    r.v[e] = (uint32_t)lo;
                }
                r.cell = (uint32_t)g;
                triangles[to] = r;
            }
        }
    }
    return 0;
}
