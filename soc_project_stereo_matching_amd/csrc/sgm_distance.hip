#include "sgm_common.hpp"
#include "sgm_volume_common.hpp"

// The distance field of the TSDF volume (include/sgm_mi355x.h, the distance section): per voxel the squared Euclidean distance, in
// voxels, to the nearest site of the lattice, exact integers in uint16, SGM_DISTANCE_FAR beyond the radius.  The transform is
// separable: three passes over the one result array, in place, no scratch and no second array.
//
//   sgm_distance_x_short_k   rows of at most DIST_ROW_WAVE voxels: a wave owns 64 / nx whole rows, one lane per voxel, the rows' sites
//               as one ballot word; nearest site left and right by count-leading / count-trailing zeros.  No LDS.
//   sgm_distance_x_k<V>      longer rows (at most 1024): a wave owns a row, a workgroup DIST_X_WAVES of them.  The site predicate of
//               every voxel goes into 32 words of LDS per row (V == 4: one 16-byte load of four voxels per lane, the nibbles joined
//               across eight lanes by shuffles; V == 1: one voxel per lane and a ballot); then every lane looks its nearest set bit
//               up, left and right, within the radius, and stores dx * dx (V == 4: four results as one 8-byte store).  A row
//               without a site is FAR without a search.  Consecutive lanes write consecutive x.
//   sgm_distance_line_k<TILE, VEC>   the y and the z pass: out[j] = min over |o| <= r of g[j + o] + o * o along lines of length L whose
//               elements lie `stride` apart.  A workgroup owns a strip of `sw` consecutive x over the whole line for one k (y pass) or
//               one j (z pass): it loads the strip into LDS (every row of the strip one contiguous segment; VEC: 16-byte loads),
//               computes from LDS and stores in place.  sw falls with L so that the tile stays within TILE elements of static LDS
//               (DIST_TILE_SMALL, 32 KB, up to DIST_LINE_C; DIST_TILE_LARGE, 64 KB, beyond).  A lane owns one x and a run of
//               consecutive j; it first finds the first and last finite value its run can reach -- none: FAR without a search --
//               and then walks o outward from 0 while o * o < best, which is the pruning g + o * o > r * r with the best so far
//               in r * r's place.  Intermediates above r * r are FAR at once, so every value fits 16 bits.
//   sgm_distance_field_k<V>  the metric, optionally signed field: one item per lane, or four with a 16-byte store.
//
// Bounded grids whose workgroups stride over their items (DIST_MAX_BLOCKS); indices scaled to bytes are 64 bits wide: 2^30 voxels of
// 2 bytes are 2^31 bytes.  No atomics, no waiting between workgroups: the same bytes on every run.

#define DIST_THREADS 256
#define DIST_X_WAVES 4                                        // rows per workgroup of the x pass: DIST_THREADS / 64
#define DIST_MAX_BLOCKS 2048                                  // of every kernel here; the workgroups stride beyond
#define DIST_ROW_WAVE 64                                      // rows up to here take sgm_distance_x_short_k
#define DIST_LINE_A 64                                        // lines up to here: strips of 256 x
#define DIST_LINE_B 128                                       //                   strips of 128
#define DIST_LINE_C 256                                       //                   strips of 64, the last of the small tile
#define DIST_LINE_D 512                                       //                   strips of 64 in the large tile; beyond: 32
#define DIST_TILE_SMALL 16384                                 // uint16 elements of LDS: 32 KB
#define DIST_TILE_LARGE 32768                                 // 64 KB
#define DIST_FAR 0xFFFFu
#define DIST_NONE 0x7FFFFFFF

struct DistanceParams {
    unsigned nx, rows;         // row length and rows (ny * nz)
    unsigned min_weight;
    int r, side, unknown;
};

struct LineParams {
    unsigned nx, L;            // row length of the array; length of a line
    unsigned stride;           // elements between neighbours of a line (nx or nx * ny)
    unsigned outer_stride;     // elements between the strips of consecutive items' outer index (nx * ny or nx)
    unsigned sw, sw_shift;     // strip width, a power of two <= DIST_THREADS
    unsigned strips, items;    // strips of a row; strips * outer
    int r;
    unsigned r2;
};

static __device__ __forceinline__ bool distance_site(const DistanceParams& p, unsigned word)
{
    const bool observed = (word >> 16) >= p.min_weight;
    const bool in_o = observed ? (short)(word & 0xFFFFu) < 0 : p.unknown != 0;
    return (p.side != 0) != in_o;
}

static __device__ __forceinline__ unsigned distance_word(int d, int r) { return d <= r ? (unsigned)(d * d) : DIST_FAR; }

__global__ __launch_bounds__(DIST_THREADS) void sgm_distance_x_short_k(DistanceParams p, const unsigned* __restrict__ voxels,
                                                                       unsigned short* __restrict__ out)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned rpw = 64u / p.nx;                          // whole rows of a wave
    const unsigned units = (p.rows + rpw - 1u) / rpw;
    const unsigned rin = lane / p.nx, x = lane - rin * p.nx;
    const unsigned long long row_mask = p.nx == 64u ? ~0ull : (1ull << p.nx) - 1ull;
    for (unsigned unit = blockIdx.x * DIST_X_WAVES + wave; unit < units; unit += gridDim.x * DIST_X_WAVES) {
        const unsigned row = unit * rpw + rin;
        const bool active = rin < rpw && row < p.rows;
        const size_t at = (size_t)row * p.nx + x;
        const bool site = active && distance_site(p, voxels[active ? at : 0]);
        const unsigned long long all = __ballot(site);
        if (!active) continue;
        const unsigned long long m = (all >> (rin * p.nx)) & row_mask;
        const unsigned long long left = m & (~0ull >> (63u - x)), right = m >> x;
        const int dl = left ? (int)x - (63 - __clzll((long long)left)) : DIST_NONE;
        const int dr = right ? __ffsll((unsigned long long)right) - 1 : DIST_NONE;
        out[at] = (unsigned short)distance_word(dl < dr ? dl : dr, p.r);
    }
}

// the distance from x to the nearest set bit of the row's words within r, DIST_NONE where there is none
static __device__ __forceinline__ int distance_nearest(const unsigned* w, int x, int nx, int r)
{
    int dl = DIST_NONE, dr = DIST_NONE;
    int wi = x >> 5;
    unsigned m = w[wi] & (0xFFFFFFFFu >> (31 - (x & 31)));
    const int first = (x - r > 0 ? x - r : 0) >> 5;
    for (;;) {
        if (m) { dl = x - ((wi << 5) + 31 - __clz((int)m)); break; }
        if (--wi < first) break;
        m = w[wi];
    }
    wi = x >> 5;
    m = w[wi] & (0xFFFFFFFFu << (x & 31));
    const int last = (x + r < nx - 1 ? x + r : nx - 1) >> 5;
    for (;;) {
        if (m) { dr = ((wi << 5) + __ffs((int)m) - 1) - x; break; }
        if (++wi > last) break;
        m = w[wi];
    }
    return dl < dr ? dl : dr;
}

template <int V>
__global__ __launch_bounds__(DIST_THREADS) void sgm_distance_x_k(DistanceParams p, const unsigned* __restrict__ voxels,
                                                                 unsigned short* __restrict__ out)
{
    __shared__ unsigned words[DIST_X_WAVES][32];              // the sites of a row of at most 1024 voxels, one bit each
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned chunks = (p.nx + 64u * V - 1u) / (64u * V);
    // (every wave of a workgroup goes round as often as the others: the barriers are met by all)
    for (unsigned base = blockIdx.x * DIST_X_WAVES; base < p.rows; base += gridDim.x * DIST_X_WAVES) {
        const unsigned row = base + wave;
        const bool live = row < p.rows;
        const size_t at = (size_t)(live ? row : 0u) * p.nx;
        bool any = false;
        __syncthreads();
        for (unsigned c = 0; c < chunks; ++c) {
            const unsigned x0 = (c * 64u + lane) * V;
            if constexpr (V == 4) {
                unsigned nib = 0;
                if (live && x0 < p.nx) {                      // nx % 4 == 0: the whole group inside
                    const uint4 q = *(const uint4*)(voxels + at + x0);
                    nib = (distance_site(p, q.x) ? 1u : 0u) | (distance_site(p, q.y) ? 2u : 0u) | (distance_site(p, q.z) ? 4u : 0u) |
                          (distance_site(p, q.w) ? 8u : 0u);
                }
                unsigned v = nib << (4u * (lane & 7u));
                v |= __shfl_xor(v, 1);
                v |= __shfl_xor(v, 2);
                v |= __shfl_xor(v, 4);
                if ((lane & 7u) == 0u) words[wave][c * 8u + (lane >> 3)] = v;
                any = any || __ballot(nib != 0u) != 0ull;
            } else {
                const bool site = live && x0 < p.nx && distance_site(p, voxels[at + x0]);
                const unsigned long long m = __ballot(site);
                if (lane == 0u) {
                    words[wave][2u * c] = (unsigned)m;
                    words[wave][2u * c + 1u] = (unsigned)(m >> 32);
                }
                any = any || m != 0ull;
            }
        }
        __syncthreads();
        if (!live) continue;
        for (unsigned c = 0; c < chunks; ++c) {
            const unsigned x0 = (c * 64u + lane) * V;
            if (x0 >= p.nx) continue;
            unsigned d[V];
#pragma unroll
            for (int e = 0; e < V; ++e)
                d[e] = any ? distance_word(distance_nearest(words[wave], (int)x0 + e, (int)p.nx, p.r), p.r) : DIST_FAR;
            if constexpr (V == 4)
                *(uint2*)(out + at + x0) = make_uint2(d[0] | d[1] << 16, d[2] | d[3] << 16);
            else
                out[at + x0] = (unsigned short)d[0];
        }
    }
}

template <int TILE, bool VEC>
__global__ __launch_bounds__(DIST_THREADS) void sgm_distance_line_k(LineParams p, unsigned short* __restrict__ d)
{
    __shared__ __attribute__((aligned(16))) unsigned short tile[TILE];
    const unsigned tid = threadIdx.x;
    const unsigned x = tid & (p.sw - 1u), g = tid >> p.sw_shift;
    const unsigned groups = DIST_THREADS >> p.sw_shift;
    const unsigned run = (p.L + groups - 1u) / groups;
    const int j0 = (int)(g * run), j1 = (int)(j0 + run < p.L ? j0 + run : p.L);       // this lane's outputs: [j0, j1)
    const int r = p.r, L = (int)p.L;
    for (unsigned item = blockIdx.x; item < p.items; item += gridDim.x) {
        const unsigned outer = item / p.strips;
        const unsigned x0 = (item - outer * p.strips) * p.sw;
        const unsigned width = p.nx - x0 < p.sw ? p.nx - x0 : p.sw;
        const size_t base = (size_t)outer * p.outer_stride + x0;
        __syncthreads();                                      // the tile of the item before is no longer read
        if constexpr (VEC) {                                  // nx % 8 == 0, sw >= 8 and the array 16-byte aligned: so is every segment
            const unsigned per_row = p.sw >> 3, total = p.L * per_row;
            for (unsigned v = tid; v < total; v += DIST_THREADS) {
                const unsigned j = v >> (p.sw_shift - 3u), c = (v - j * per_row) << 3;
                if (c < width) *(uint4*)(tile + j * p.sw + c) = *(const uint4*)(d + base + (size_t)j * p.stride + c);
            }
        } else {
            const unsigned total = p.L << p.sw_shift;
            for (unsigned e = tid; e < total; e += DIST_THREADS) {
                const unsigned j = e >> p.sw_shift, c = e - (j << p.sw_shift);
                if (c < width) tile[e] = d[base + (size_t)j * p.stride + c];
            }
        }
        __syncthreads();
        if (x >= width || j0 >= j1) continue;
        // the first and the last finite value this run can reach
        const int lo = j0 - r > 0 ? j0 - r : 0, hi = j1 - 1 + r < L - 1 ? j1 - 1 + r : L - 1;
        int fin_lo = 0, fin_hi = -1;
        for (int j = lo; j <= hi; ++j)
            if (tile[(unsigned)j * p.sw + x] != DIST_FAR) {
                if (fin_hi < 0) fin_lo = j;
                fin_hi = j;
            }
        for (int j = j0; j < j1; ++j) {
            unsigned best = p.r2 + 1u;
            if (fin_hi >= 0) {
                const unsigned own = tile[(unsigned)j * p.sw + x];
                best = own < best ? own : best;
                const int up = fin_hi - j, down = j - fin_lo;  // the farthest offsets that can hold a finite value
                int o = fin_lo - j > j - fin_hi ? fin_lo - j : j - fin_hi;
                o = o > 1 ? o : 1;
                const int o_max = up > down ? up : down;
                for (; o <= o_max && (unsigned)(o * o) < best; ++o) {
                    const unsigned oo = (unsigned)(o * o);
                    if (o <= up) {
                        const unsigned t = tile[(unsigned)(j + o) * p.sw + x] + oo;
                        best = t < best ? t : best;
                    }
                    if (o <= down) {
                        const unsigned t = tile[(unsigned)(j - o) * p.sw + x] + oo;
                        best = t < best ? t : best;
                    }
                }
            }
            d[base + (size_t)(unsigned)j * p.stride + x] = (unsigned short)(best <= p.r2 ? best : DIST_FAR);
        }
    }
}

static __device__ __forceinline__ float distance_field_of(unsigned o, unsigned i, bool have_in, float voxel)
{
    if (o == DIST_FAR) return INFINITY;
    if (o > 0u) return voxel * sqrtf((float)o);
    if (!have_in || i == 0u) return 0.0f;
    if (i == DIST_FAR) return -INFINITY;
    return -(voxel * sqrtf((float)i));
}

template <int V>
__global__ __launch_bounds__(DIST_THREADS) void sgm_distance_field_k(unsigned items, float voxel, const unsigned short* __restrict__ out2,
                                                                     const unsigned short* __restrict__ in2, float* __restrict__ field)
{
    const unsigned stride = gridDim.x * DIST_THREADS;         // items <= 2^30 and stride <= 2^19: the sum stays below 2^32
    for (unsigned item = blockIdx.x * DIST_THREADS + threadIdx.x; item < items; item += stride) {
        const size_t at = (size_t)item * V;
        if constexpr (V == 4) {
            const uint2 o = *(const uint2*)(out2 + at);
            const uint2 i = in2 ? *(const uint2*)(in2 + at) : make_uint2(0u, 0u);
            float4 f;
            f.x = distance_field_of(o.x & 0xFFFFu, i.x & 0xFFFFu, in2 != nullptr, voxel);
            f.y = distance_field_of(o.x >> 16, i.x >> 16, in2 != nullptr, voxel);
            f.z = distance_field_of(o.y & 0xFFFFu, i.y & 0xFFFFu, in2 != nullptr, voxel);
            f.w = distance_field_of(o.y >> 16, i.y >> 16, in2 != nullptr, voxel);
            *(float4*)(field + at) = f;
        } else {
            field[at] = distance_field_of(out2[at], in2 ? in2[at] : 0u, in2 != nullptr, voxel);
        }
    }
}

// one min-plus pass along lines of length L: `outer` strips of rows, each `outer_stride` elements after the one before
static int distance_line_pass(hipStream_t stream, unsigned nx, unsigned L, unsigned stride, unsigned outer, unsigned outer_stride, int r,
                              unsigned short* d)
{
    LineParams p;
    p.nx = nx; p.L = L; p.stride = stride; p.outer_stride = outer_stride;
    p.sw = L <= DIST_LINE_A ? 256u : L <= DIST_LINE_B ? 128u : L <= DIST_LINE_D ? 64u : 32u;
    while (p.sw > 1u && p.sw / 2u >= nx) p.sw /= 2u;          // no wider than the row needs
    p.sw_shift = 0;
    while ((1u << p.sw_shift) < p.sw) ++p.sw_shift;
    p.strips = (nx + p.sw - 1u) / p.sw;
    p.items = p.strips * outer;
    p.r = r; p.r2 = (unsigned)(r * r);
    const bool vec = nx % 8u == 0u && p.sw >= 8u && (uintptr_t)d % 16 == 0;
    const dim3 grid(p.items > DIST_MAX_BLOCKS ? DIST_MAX_BLOCKS : p.items);
#define DIST_LINE_LAUNCH(TILE, VEC) hipLaunchKernelGGL((sgm_distance_line_k<TILE, VEC>), grid, dim3(DIST_THREADS), 0, stream, p, d)
    if (L <= DIST_LINE_C) {
        if (vec) DIST_LINE_LAUNCH(DIST_TILE_SMALL, true); else DIST_LINE_LAUNCH(DIST_TILE_SMALL, false);
    } else {
        if (vec) DIST_LINE_LAUNCH(DIST_TILE_LARGE, true); else DIST_LINE_LAUNCH(DIST_TILE_LARGE, false);
    }
#undef DIST_LINE_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int sgmd_volume_distance(int ord, void* stream, const sgmd_volume* v, unsigned min_weight, int radius, int side, int unknown,
                         const void* voxels, void* dist2)
{
    if (!volume_ok(v) || !voxels || !dist2 || min_weight < 1u || min_weight > 65535u || radius < 1 || radius > 255 || (side | unknown) < 0 ||
        side > 1 || unknown > 1 || (uintptr_t)voxels % 4 != 0 || (uintptr_t)dist2 % 2 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_distance: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const unsigned nx = (unsigned)v->nx, ny = (unsigned)v->ny, nz = (unsigned)v->nz;
    DistanceParams p;
    p.nx = nx; p.rows = ny * nz; p.min_weight = min_weight; p.r = radius; p.side = side; p.unknown = unknown;
    unsigned short* d = (unsigned short*)dist2;
    if (nx <= DIST_ROW_WAVE) {
        const unsigned rpw = 64u / nx, units = (p.rows + rpw - 1u) / rpw, blocks = (units + DIST_X_WAVES - 1u) / DIST_X_WAVES;
        hipLaunchKernelGGL(sgm_distance_x_short_k, dim3(blocks > DIST_MAX_BLOCKS ? DIST_MAX_BLOCKS : blocks), dim3(DIST_THREADS), 0,
                           (hipStream_t)stream, p, (const unsigned*)voxels, d);
    } else {
        const unsigned blocks = (p.rows + DIST_X_WAVES - 1u) / DIST_X_WAVES;
        const dim3 grid(blocks > DIST_MAX_BLOCKS ? DIST_MAX_BLOCKS : blocks);
        if (nx % 4u == 0u && (uintptr_t)voxels % 16 == 0 && (uintptr_t)dist2 % 8 == 0)
            hipLaunchKernelGGL(sgm_distance_x_k<4>, grid, dim3(DIST_THREADS), 0, (hipStream_t)stream, p, (const unsigned*)voxels, d);
        else
            hipLaunchKernelGGL(sgm_distance_x_k<1>, grid, dim3(DIST_THREADS), 0, (hipStream_t)stream, p, (const unsigned*)voxels, d);
    }
    HIP_TRY(hipGetLastError());
    // (a line of one element is its own transform)
    if (ny > 1u && distance_line_pass((hipStream_t)stream, nx, ny, nx, nz, nx * ny, radius, d) != 0) return -1;
    if (nz > 1u && distance_line_pass((hipStream_t)stream, nx, nz, nx * ny, ny, nx, radius, d) != 0) return -1;
    return 0;
}

int sgmd_volume_distance_field(int ord, void* stream, const sgmd_volume* v, const void* out2, const void* in2, void* field)
{
    if (!volume_ok(v) || !out2 || !field || (uintptr_t)out2 % 2 != 0 || (uintptr_t)in2 % 2 != 0 || (uintptr_t)field % 4 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_distance_field: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const unsigned n = (unsigned)v->nx * (unsigned)v->ny * (unsigned)v->nz;
    const bool four = v->nx % 4 == 0 && (uintptr_t)out2 % 8 == 0 && (uintptr_t)in2 % 8 == 0 && (uintptr_t)field % 16 == 0;
    const unsigned items = four ? n / 4u : n, blocks = (items + DIST_THREADS - 1u) / DIST_THREADS;
    const dim3 grid(blocks > DIST_MAX_BLOCKS ? DIST_MAX_BLOCKS : blocks);
    if (four)
        hipLaunchKernelGGL(sgm_distance_field_k<4>, grid, dim3(DIST_THREADS), 0, (hipStream_t)stream, items, v->voxel,
                           (const unsigned short*)out2, (const unsigned short*)in2, (float*)field);
    else
        hipLaunchKernelGGL(sgm_distance_field_k<1>, grid, dim3(DIST_THREADS), 0, (hipStream_t)stream, items, v->voxel,
                           (const unsigned short*)out2, (const unsigned short*)in2, (float*)field);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
