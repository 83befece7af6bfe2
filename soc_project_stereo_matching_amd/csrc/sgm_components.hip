#include "sgm_common.hpp"
#include "sgm_cloud_common.hpp"
#include "sgm_volume_common.hpp"

// Connected components of the voxel lattice (include/sgm_mi355x.h, the components section; tests/components_ref.py restates it):
// union-find over the caller's label array, which holds PARENTS (voxel indices, CC_NONE outside the set) until the label launch
// turns them into the words of the contract.  A parent only ever decreases (atomicMin, the larger root under the smaller), so every
// find ends and the final root of a component is its smallest voxel index, the `first` of the contract.  The speckle kernels of
// sgm_post.hip carried into 3-D:
//
//   sgm_components_tile_k    a workgroup labels a 64 x CC_TY x CC_TZ tile entirely in LDS.  One wave = one x-row of 64 voxels: the
//               row's set is one ballot word, a run's first voxel comes from a count of leading zeros, and the union-find joins only
//               runs of neighbouring rows (2 earlier rows at 6-connectivity, 4 at 26), and only where the link is not implied by
//               the voxel to the left -- all decided on the rows' 64-bit words.  One LDS atomic per run gives the voxel count of
//               every tile-local root.  Out: parent[p] = the tile-local root as a voxel index, size[p] = that count at the roots,
//               0 elsewhere.  A tile without a voxel of the set leaves after its first barrier.
//   sgm_components_border_k  voxels with an earlier neighbour in another tile union roots in global memory, under the same
//               implied-by-the-left rule (the set is read back from parent: != CC_NONE).
//   sgm_components_sizes_k   parent[p] = find(p) (a store of an ancestor is harmless to the finds that run beside it) and every
//               tile-local root that is not the final root adds its count to the final root's: one integer atomic per tile-local
//               component, never one per voxel.
//   sgm_components_label_k   the words of the contract, first + 1 where size[first] >= min_voxels, else 0, and per tile of the ordered
//               compaction (sgm_cloud_common.hpp) the surviving roots and all roots.
//   sgm_components_scan_k    one workgroup: the tiles' bases, counts[0] and counts[1].
//   sgm_components_emit_k    a surviving root writes its record (first, voxels; box and sums empty) at its rank, leaves the rank in
//               size[first] and empties the box accumulator of that rank.
//   sgm_components_stats_k   a workgroup reduces a 64 x CC_SY x CC_SZ tile on chip first: a run (one lane knows its ends) goes into
//               an LDS hash table keyed by label -- CC_SLOTS is the largest number of runs of such a tile, so a probe always finds a
//               place -- and every used slot then makes 6 min / max atomics on the accumulators and 3 64-bit adds on the record.
//   sgm_components_box_k     the accumulators into lo[] and hi[] of the records written.
//   sgm_component_of_k       a record list's object indices: the label of voxel n, or of the far end of its edge, looked up in
//               the sorted object list by binary search.
//
// Integer atomics only, no waiting between workgroups; the grids are bounded and stride over their tiles.

#define CC_THREADS 256
#define CC_WAVES (CC_THREADS / 64)
#define CC_TX 64                                              // one tile row = one wave
#ifndef CC_TY                                                 // (the Makefile's CC_TILE_YZ builds another tile for a timing; NOTES.md section 44)
#define CC_TY 8
#define CC_TZ 8
#endif
#define CC_ROWS (CC_TY * CC_TZ)
#define CC_TILE (CC_TX * CC_ROWS)
#define CC_SY 4                                               // the statistics tile: 64 x 4 x 4
#define CC_SZ 4
#define CC_SROWS (CC_SY * CC_SZ)
#define CC_SLOTS 512                                          // at most 32 runs in a row of 64
#define CC_MAX_BLOCKS 2048                                    // of the striding kernels
#define CC_NONE 0xFFFFFFFFu
#define CC_MAX_PLANES 4

struct ComponentPlanes {
    int count;                                                // the non-void planes
    float n[CC_MAX_PLANES][3], a[CC_MAX_PLANES][3], clearance[CC_MAX_PLANES];
};

struct ComponentParams {
    unsigned nx, ny, nz, n;
    unsigned tiles_x, tiles_y, tiles_z, tiles;
    unsigned min_weight, min_voxels;
    int set, unknown, conn26;
    float voxel, ox, oy, oz;
};

struct Component { unsigned first, voxels; unsigned short lo[3], hi[3]; unsigned reserved; unsigned long long sum[3]; };
static_assert(sizeof(Component) == 48, "sgm_component");

static __device__ __forceinline__ unsigned cc_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename P>
static __device__ __forceinline__ unsigned cc_find(P par, unsigned x)
{
    unsigned p = cc_load(par + x);
    while (p != x) { x = p; p = cc_load(par + x); }
    return x;
}

template <typename P>
static __device__ __forceinline__ void cc_union(P par, unsigned a, unsigned b)
{
    for (;;) {
        a = cc_find(par, a);
        b = cc_find(par, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }    // hook the larger root under the smaller
        const unsigned old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

// THE predicate of the contract
static __device__ __forceinline__ bool cc_in_set(const ComponentParams& c, const ComponentPlanes& pl, unsigned word, unsigned i, unsigned j,
                                                 unsigned k)
{
    const bool observed = (word >> 16) >= c.min_weight;
    const bool neg = (short)(word & 0xFFFFu) < 0;
    if (!(observed ? (c.set != 0) != neg : c.unknown != 0)) return false;
    const float cx = volume_centre(c.ox, i, c.voxel), cy = volume_centre(c.oy, j, c.voxel), cz = volume_centre(c.oz, k, c.voxel);
    for (int q = 0; q < pl.count; ++q) {
        const float s = ((pl.n[q][0] * (cx - pl.a[q][0]) + pl.n[q][1] * (cy - pl.a[q][1])) + pl.n[q][2] * (cz - pl.a[q][2]));
        if (cloud_finite(s) && s <= pl.clearance[q]) return false;
    }
    return true;
}

static __device__ __forceinline__ bool cc_bit(unsigned long long m, unsigned x) { return (m >> x) & 1ull; }

// the first voxel of the run of set bits that holds bit x of m
static __device__ __forceinline__ unsigned cc_run_start(unsigned long long m, unsigned x)
{
    const unsigned long long below = ~m & ((1ull << x) - 1ull);
    return below ? 64u - (unsigned)__clzll((long long)below) : 0u;
}

static __device__ __forceinline__ void cc_tile_origin(const ComponentParams& c, unsigned tile, unsigned ty_dim, unsigned tz_dim,
                                                      unsigned tiles_y, unsigned& x0, unsigned& y0, unsigned& z0)
{
    const unsigned tx = tile % c.tiles_x, rest = tile / c.tiles_x;
    const unsigned ty = rest % tiles_y, tz = rest / tiles_y;
    x0 = tx * CC_TX; y0 = ty * ty_dim; z0 = tz * tz_dim;
}

// lanes of row ra (word a) against the earlier row rb (word b): the unions that no voxel to the left implies
static __device__ __forceinline__ void cc_join_rows(unsigned* lab, unsigned long long a, unsigned long long b, unsigned ra, unsigned rb,
                                                    unsigned x, bool diagonals)
{
    if (!cc_bit(a, x)) return;
    const unsigned i = ra * CC_TX + x, o = rb * CC_TX + x;
    const bool al = x > 0u && cc_bit(a, x - 1u), bl = x > 0u && cc_bit(b, x - 1u);
    const bool ar = x < 63u && cc_bit(a, x + 1u), br = x < 63u && cc_bit(b, x + 1u);
    if (cc_bit(b, x)) {
        if (!(al && bl)) cc_union(lab, i, o);
    } else if (diagonals) {
        if (bl && !al) cc_union(lab, i, o - 1u);
        if (br && !ar) cc_union(lab, i, o + 1u);
    }
}

__global__ __launch_bounds__(CC_THREADS) void sgm_components_tile_k(ComponentParams c, ComponentPlanes pl, const unsigned* __restrict__ voxels,
                                                                    unsigned* __restrict__ parent, unsigned* __restrict__ size)
{
    __shared__ unsigned lab[CC_TILE];
    __shared__ unsigned cnt[CC_TILE];
    __shared__ unsigned long long rowset[CC_ROWS];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned tile = blockIdx.x; tile < c.tiles; tile += gridDim.x) {
        unsigned x0, y0, z0;
        cc_tile_origin(c, tile, CC_TY, CC_TZ, c.tiles_y, x0, y0, z0);
        const unsigned x = x0 + lane;
        __syncthreads();                                      // the tile before is no longer read
        // ---- a row per wave: the set as a ballot word, a voxel's label the first voxel of its run ----
        bool any = false;
        for (unsigned r = wave; r < CC_ROWS; r += CC_WAVES) {
            const unsigned y = y0 + (r % CC_TY), z = z0 + (r / CC_TY);
            const bool live = x < c.nx && y < c.ny && z < c.nz;
            const unsigned word = live ? voxels[((size_t)z * c.ny + y) * c.nx + x] : 0u;
            const bool in = live && cc_in_set(c, pl, word, x, y, z);
            const unsigned long long m = __ballot(in);
            if (lane == 0u) rowset[r] = m;
            lab[r * CC_TX + lane] = in ? r * CC_TX + cc_run_start(m, lane) : CC_NONE;
            cnt[r * CC_TX + lane] = 0u;
            any = any || m != 0ull;
        }
#ifdef CC_EVERY_TILE
        __syncthreads();
#else
        // a tile without a voxel of the set -- most tiles of a surface shell -- has nothing to join or to count
        if (!__syncthreads_or(any)) {
            for (unsigned r = wave; r < CC_ROWS; r += CC_WAVES) {
                const unsigned y = y0 + (r % CC_TY), z = z0 + (r / CC_TY);
                if (!(x < c.nx && y < c.ny && z < c.nz)) continue;
                const size_t p = ((size_t)z * c.ny + y) * c.nx + x;
                parent[p] = CC_NONE;
                size[p] = 0u;
            }
            continue;
        }
#endif
        // ---- join the runs of neighbouring rows ----
        for (unsigned r = wave; r < CC_ROWS; r += CC_WAVES) {
            const unsigned ly = r % CC_TY, lz = r / CC_TY;
            const unsigned long long a = rowset[r];
            if (a == 0ull) continue;
            if (ly > 0u) cc_join_rows(lab, a, rowset[r - 1u], r, r - 1u, lane, c.conn26);
            if (lz > 0u) cc_join_rows(lab, a, rowset[r - CC_TY], r, r - CC_TY, lane, c.conn26);
            if (c.conn26 && lz > 0u) {
                if (ly > 0u) {
                    const unsigned long long b = rowset[r - CC_TY - 1u];
                    cc_join_rows(lab, a, b, r, r - CC_TY - 1u, lane, true);
                }
                if (ly + 1u < CC_TY) {
                    const unsigned long long b = rowset[r - CC_TY + 1u];
                    cc_join_rows(lab, a, b, r, r - CC_TY + 1u, lane, true);
                }
            }
        }
        __syncthreads();
        // ---- voxels per tile-local root: one LDS atomic per run, by its last voxel ----
        for (unsigned r = wave; r < CC_ROWS; r += CC_WAVES) {
            const unsigned long long a = rowset[r];
            if (cc_bit(a, lane) && (lane == 63u || !cc_bit(a, lane + 1u))) {
                const unsigned start = cc_run_start(a, lane);
                atomicAdd(&cnt[cc_find(lab, r * CC_TX + start)], lane - start + 1u);
            }
        }
        __syncthreads();
        for (unsigned r = wave; r < CC_ROWS; r += CC_WAVES) {
            const unsigned y = y0 + (r % CC_TY), z = z0 + (r / CC_TY);
            if (!(x < c.nx && y < c.ny && z < c.nz)) continue;
            const unsigned i = r * CC_TX + lane;
            unsigned g = CC_NONE;
            if (lab[i] != CC_NONE) {
                const unsigned root = cc_find(lab, lab[i]), rr = root / CC_TX;
                g = ((z0 + rr / CC_TY) * c.ny + (y0 + rr % CC_TY)) * c.nx + x0 + (root % CC_TX);
            }
            const size_t p = ((size_t)z * c.ny + y) * c.nx + x;
            parent[p] = g;
            size[p] = cnt[i];
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void sgm_components_border_k(ComponentParams c, unsigned* __restrict__ parent)
{
    const unsigned stride = gridDim.x * CC_THREADS;
    for (unsigned p = blockIdx.x * CC_THREADS + threadIdx.x; p < c.n; p += stride) {
        unsigned x, y, z;
        const unsigned row = p / c.nx;
        x = p - row * c.nx; z = row / c.ny; y = row - z * c.ny;
        const unsigned lx = x % CC_TX, ly = y % CC_TY, lz = z % CC_TZ;
        const bool face = lx == 0u || ly == 0u || lz == 0u || (c.conn26 && (lx == CC_TX - 1u || ly == CC_TY - 1u));
        if (!face) continue;
        if (cc_load(parent + p) == CC_NONE) continue;
        // the earlier half of the neighbourhood: (dz, dy, dx) below (0, 0, 0)
        for (int o = 0; o < 13; ++o) {
            const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;     // o = 0..12: dz = -1 (9), dz = 0 dy = -1 (3), (-1,0,0)
            if (!c.conn26 && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
            const int qx = (int)x + dx, qy = (int)y + dy, qz = (int)z + dz;
            if (qx < 0 || qy < 0 || qz < 0 || qx >= (int)c.nx || qy >= (int)c.ny) continue;
            if ((unsigned)qx / CC_TX == x / CC_TX && (unsigned)qy / CC_TY == y / CC_TY && (unsigned)qz / CC_TZ == z / CC_TZ) continue;
            const unsigned q = ((unsigned)qz * c.ny + (unsigned)qy) * c.nx + (unsigned)qx;
            if (cc_load(parent + q) == CC_NONE) continue;
            if (dy != 0 || dz != 0) {
                // implied by the pair one voxel to the left, or by the straight pair of this or the next column
                if (dx == 0) {
                    if (x > 0u && cc_load(parent + p - 1u) != CC_NONE && cc_load(parent + q - 1u) != CC_NONE) continue;
                } else if (dx < 0) {
                    if (cc_load(parent + q + 1u) != CC_NONE || cc_load(parent + p - 1u) != CC_NONE) continue;
                } else {
                    if (cc_load(parent + q - 1u) != CC_NONE || cc_load(parent + p + 1u) != CC_NONE) continue;
                }
            }
            cc_union(parent, p, q);
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void sgm_components_sizes_k(unsigned n, unsigned* __restrict__ parent, unsigned* __restrict__ size)
{
    const unsigned stride = gridDim.x * CC_THREADS;
    for (unsigned p = blockIdx.x * CC_THREADS + threadIdx.x; p < n; p += stride) {
        if (cc_load(parent + p) == CC_NONE) continue;
        const unsigned root = cc_find(parent, p);
        __hip_atomic_store(parent + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (root == p) continue;
        const unsigned mine = size[p];                        // (nobody adds to a voxel that is not a final root)
        if (mine) atomicAdd(size + root, mine);
    }
}

// one pass of the label launch over TILE_THREADS voxels: the root of voxel p and whether it survives (parent is the label array
// the launch then writes at the same place: no __restrict__ on either)
static __device__ __forceinline__ void cc_label_pass(const unsigned* parent, const unsigned* __restrict__ size, unsigned p,
                                                     bool live, unsigned min_voxels, unsigned& root, bool& keep)
{
    root = live ? parent[p] : CC_NONE;
    keep = root != CC_NONE && size[root] >= min_voxels;
}

__global__ __launch_bounds__(TILE_THREADS) void sgm_components_label_k(unsigned n, unsigned tile, unsigned min_voxels,
                                                                       unsigned* labels, const unsigned* __restrict__ size,
                                                                       unsigned* __restrict__ kept, unsigned* __restrict__ roots)
{
    const unsigned first = blockIdx.x * tile, end = min(first + tile, n);
    unsigned survivors = 0, all = 0;                          // of this wave, the same in all of its lanes
    for (unsigned p = first + threadIdx.x; p - threadIdx.x < end; p += TILE_THREADS) {
        unsigned root, lower = 0;
        bool keep;
        cc_label_pass(labels, size, p, p < end, min_voxels, root, keep);
        if (p < end) labels[p] = keep ? root + 1u : 0u;
        wave_rank(keep && root == p, lower, survivors);
        wave_rank(root == p, lower, all);
    }
    __shared__ unsigned s_all[TILE_WAVES];
    if ((threadIdx.x & 63u) == 0) s_all[threadIdx.x >> 6] = all;
    tile_total(survivors, kept + blockIdx.x);                 // (its barrier is also s_all's)
    if (threadIdx.x == 0) {
        unsigned sum = 0;
        for (int w = 0; w < TILE_WAVES; ++w) sum += s_all[w];
        roots[blockIdx.x] = sum;
    }
}

// ONE workgroup: base[i] = kept[0] + .. + kept[i - 1]; counts[0] = the survivors, counts[1] = the roots
__global__ __launch_bounds__(SCAN_THREADS) void sgm_components_scan_k(const unsigned* __restrict__ kept, const unsigned* __restrict__ roots,
                                                                      unsigned ntiles, unsigned* __restrict__ base, unsigned* __restrict__ counts)
{
    __shared__ unsigned s_part[SCAN_THREADS / 64];
    unsigned mine = 0;
    for (unsigned i = threadIdx.x; i < ntiles; i += SCAN_THREADS) mine += roots[i];
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) mine += __shfl_xor(mine, step);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = mine;
    const unsigned total = tile_scan(kept, ntiles, base, [](unsigned, unsigned) {});
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0;
        for (unsigned w = 0; w < SCAN_THREADS / 64; ++w) sum += s_part[w];
        counts[0] = total;
        counts[1] = sum;
    }
}

struct ComponentBox { unsigned lo[3], hi[3]; };

__global__ __launch_bounds__(TILE_THREADS) void sgm_components_emit_k(unsigned n, unsigned tile, const unsigned* __restrict__ labels,
                                                                      unsigned* __restrict__ size, const unsigned* __restrict__ kept,
                                                                      const unsigned* __restrict__ base, Component* __restrict__ objects,
                                                                      ComponentBox* __restrict__ boxes, size_t capacity)
{
    if (kept[blockIdx.x] == 0u) return;                       // (the same in every lane)
    const unsigned first = blockIdx.x * tile, end = min(first + tile, n);
    size_t run = base[blockIdx.x];
    unsigned turn = 0;
    for (unsigned p = first + threadIdx.x; p - threadIdx.x < end; p += TILE_THREADS, turn ^= 1u) {
        const bool root = p < end && labels[p] == p + 1u;
        unsigned lower = 0, wave_total = 0, all;
        wave_rank(root, lower, wave_total);
        const unsigned before = pass_before(wave_total, turn, all);
        if (root) {
            const size_t to = run + before + lower;
            if (to < capacity) {
                Component o;
                o.first = p; o.voxels = size[p];
                o.lo[0] = o.lo[1] = o.lo[2] = o.hi[0] = o.hi[1] = o.hi[2] = 0;
                o.reserved = 0u;
                o.sum[0] = o.sum[1] = o.sum[2] = 0ull;
                objects[to] = o;
                ComponentBox b;
                b.lo[0] = b.lo[1] = b.lo[2] = 0xFFFFFFFFu;
                b.hi[0] = b.hi[1] = b.hi[2] = 0u;
                boxes[to] = b;
            }
            size[p] = to < capacity ? (unsigned)to : CC_NONE; // the rank, where the statistics find it
        }
        run += all;
    }
}

__global__ __launch_bounds__(CC_THREADS) void sgm_components_stats_k(ComponentParams c, unsigned stiles_y, unsigned stiles,
                                                                     const unsigned* __restrict__ labels, const unsigned* __restrict__ rank,
                                                                     Component* __restrict__ objects, ComponentBox* __restrict__ boxes)
{
    __shared__ unsigned key[CC_SLOTS];
    __shared__ unsigned lo[3][CC_SLOTS], hi[3][CC_SLOTS], sum[3][CC_SLOTS];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned tile = blockIdx.x; tile < stiles; tile += gridDim.x) {
        unsigned x0, y0, z0;
        cc_tile_origin(c, tile, CC_SY, CC_SZ, stiles_y, x0, y0, z0);
        const unsigned x = x0 + lane;
        __syncthreads();                                      // the table of the tile before has been flushed
        for (unsigned s = threadIdx.x; s < CC_SLOTS; s += CC_THREADS) {
            key[s] = 0u;
            lo[0][s] = lo[1][s] = lo[2][s] = 0xFFFFFFFFu;
            hi[0][s] = hi[1][s] = hi[2][s] = 0u;
            sum[0][s] = sum[1][s] = sum[2][s] = 0u;
        }
        __syncthreads();
        for (unsigned r = wave; r < CC_SROWS; r += CC_WAVES) {
            const unsigned y = y0 + (r % CC_SY), z = z0 + (r / CC_SY);
            const bool live = x < c.nx && y < c.ny && z < c.nz;
            const unsigned l = live ? labels[((size_t)z * c.ny + y) * c.nx + x] : 0u;
            const unsigned left = __shfl_up(l, 1), right = __shfl_down(l, 1);
            const bool starts = l != 0u && (lane == 0u || left != l);
            const bool ends = l != 0u && (lane == 63u || right != l);
            // the first lane of this lane's run: the highest start at or below it
            const unsigned long long sm = __ballot(starts);
            const unsigned long long below = sm & (~0ull >> (63u - lane));
            if (!ends) continue;
            const unsigned start = 63u - (unsigned)__clzll((long long)below), len = lane - start + 1u;
            unsigned s = (l * 0x9E3779B1u) >> 23;             // 9 bits
            for (;;) {
                const unsigned old = atomicCAS(&key[s], 0u, l);
                if (old == 0u || old == l) break;
                s = (s + 1u) & (CC_SLOTS - 1u);               // (CC_SLOTS holds every run of a tile: a free or an own slot comes)
            }
            atomicMin(&lo[0][s], x0 + start); atomicMax(&hi[0][s], x);
            atomicMin(&lo[1][s], y); atomicMax(&hi[1][s], y);
            atomicMin(&lo[2][s], z); atomicMax(&hi[2][s], z);
            atomicAdd(&sum[0][s], (len * (2u * x0 + start + lane)) / 2u);
            atomicAdd(&sum[1][s], len * y);
            atomicAdd(&sum[2][s], len * z);
        }
        __syncthreads();
        for (unsigned s = threadIdx.x; s < CC_SLOTS; s += CC_THREADS) {
            const unsigned l = key[s];
            if (l == 0u) continue;
            const unsigned at = rank[l - 1u];
            if (at == CC_NONE) continue;                      // an object past the capacity
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(&boxes[at].lo[a], lo[a][s]);
                atomicMax(&boxes[at].hi[a], hi[a][s]);
                atomicAdd(&objects[at].sum[a], (unsigned long long)sum[a][s]);
            }
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void sgm_components_box_k(const unsigned* __restrict__ counts, size_t capacity,
                                                                   const ComponentBox* __restrict__ boxes, Component* __restrict__ objects)
{
    const size_t written = counts[0] < capacity ? counts[0] : capacity;
    for (size_t r = (size_t)blockIdx.x * CC_THREADS + threadIdx.x; r < written; r += (size_t)gridDim.x * CC_THREADS) {
        const ComponentBox b = boxes[r];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            objects[r].lo[a] = (unsigned short)b.lo[a];
            objects[r].hi[a] = (unsigned short)b.hi[a];
        }
    }
}

struct __attribute__((aligned(16))) ListRecord { float x, y, z; unsigned id; };

__global__ __launch_bounds__(CC_THREADS) void sgm_component_of_k(unsigned nx, unsigned ny, unsigned nz, unsigned n,
                                                                 const unsigned* __restrict__ labels, const Component* __restrict__ objects,
                                                                 size_t capacity, const unsigned* __restrict__ counts,
                                                                 const ListRecord* __restrict__ records, size_t records_capacity,
                                                                 const unsigned* __restrict__ records_count, unsigned id_kinds,
                                                                 unsigned* __restrict__ index)
{
    const size_t todo = records_count && records_count[0] < records_capacity ? records_count[0] : records_capacity;
    const size_t written = counts[0] < capacity ? counts[0] : capacity;
    for (size_t r = (size_t)blockIdx.x * CC_THREADS + threadIdx.x; r < todo; r += (size_t)gridDim.x * CC_THREADS) {
        const unsigned id = records[r].id, v = id / id_kinds, e = id - v * id_kinds;
        unsigned out = 0u;
        if (v < n && e < id_kinds - 1u) {
            unsigned l = labels[v];
            if (l == 0u) {
                const unsigned corner = MESH_CORNER_OF(e);
                const unsigned row = v / nx, i = v - row * nx, k = row / ny, j = row - k * ny;
                const unsigned fi = i + (corner & 1u), fj = j + ((corner >> 1) & 1u), fk = k + (corner >> 2);
                if (fi < nx && fj < ny && fk < nz) l = labels[(fk * ny + fj) * nx + fi];
            }
            if (l != 0u) {
                size_t a = 0, b = written;                    // the object whose first is l - 1, in [a, b)
                while (a < b) {
                    const size_t mid = a + (b - a) / 2;
                    if (objects[mid].first < l - 1u) a = mid + 1; else b = mid;
                }
                if (a < written && objects[a].first == l - 1u) out = (unsigned)a + 1u;
            }
        }
        index[r] = out;
    }
}

static unsigned cc_div_up(unsigned a, unsigned b) { return (a + b - 1u) / b; }
static unsigned cc_blocks(size_t items) { return items > CC_MAX_BLOCKS ? CC_MAX_BLOCKS : (unsigned)(items ? items : 1); }

// the scratch: size[n], then the compaction's kept / base / roots per tile of TILE_MAX voxels, then a box per object that can be written
static size_t cc_tiles_max(size_t n) { return (n + TILE_MAX - 1) / TILE_MAX; }
static size_t cc_objects_max(size_t n, size_t capacity) { return capacity < n ? capacity : n; }

extern "C" {

size_t sgmd_components_scratch_bytes(int nx, int ny, int nz, size_t capacity)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    const size_t n = (size_t)nx * ny * nz;
    return 4 * n + 12 * cc_tiles_max(n) + sizeof(ComponentBox) * cc_objects_max(n, capacity);
}

int sgmd_volume_components(int ord, void* stream, const sgmd_volume* v, const sgmd_components* cs, const void* voxels, void* scratch,
                           void* labels, void* objects, size_t capacity, void* counts)
{
    if (!volume_ok(v) || !cs || !voxels || !scratch || !labels || !counts || (!objects && capacity) || cs->min_weight < 1u ||
        cs->min_weight > 65535u || (cs->set | cs->unknown) < 0 || cs->set > 1 || cs->unknown > 1 ||
        (cs->connectivity != 6 && cs->connectivity != 26) || cs->min_voxels < 1u || cs->planes < 0 || cs->planes > CC_MAX_PLANES ||
        (uintptr_t)voxels % 4 != 0 || (uintptr_t)labels % 4 != 0 || (uintptr_t)counts % 4 != 0 || (uintptr_t)objects % 8 != 0 ||
        (uintptr_t)scratch % 8 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_components: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const hipStream_t st = (hipStream_t)stream;
    ComponentParams c;
    c.nx = (unsigned)v->nx; c.ny = (unsigned)v->ny; c.nz = (unsigned)v->nz; c.n = c.nx * c.ny * c.nz;
    c.tiles_x = cc_div_up(c.nx, CC_TX); c.tiles_y = cc_div_up(c.ny, CC_TY); c.tiles_z = cc_div_up(c.nz, CC_TZ);
    c.tiles = c.tiles_x * c.tiles_y * c.tiles_z;
    c.min_weight = cs->min_weight; c.min_voxels = cs->min_voxels;
    c.set = cs->set; c.unknown = cs->unknown; c.conn26 = cs->connectivity == 26;
    c.voxel = v->voxel; c.ox = v->origin[0]; c.oy = v->origin[1]; c.oz = v->origin[2];
    ComponentPlanes pl;
    memset(&pl, 0, sizeof pl);
    for (int q = 0; q < cs->planes; ++q) {
        const float* nrm = cs->normal[q];
        if (nrm[0] == 0.0f && nrm[1] == 0.0f && nrm[2] == 0.0f) continue;      // a void plane excludes nothing
        for (int a = 0; a < 3; ++a) { pl.n[pl.count][a] = nrm[a]; pl.a[pl.count][a] = cs->anchor[q][a]; }
        pl.clearance[pl.count++] = cs->clearance[q];
    }
    // the scratch, 8-byte aligned throughout: the boxes first
    const size_t n = c.n, ntiles_max = cc_tiles_max(n);
    ComponentBox* boxes = (ComponentBox*)scratch;
    unsigned* size = (unsigned*)(boxes + cc_objects_max(n, capacity));
    unsigned* kept = size + n;
    unsigned* base = kept + ntiles_max;
    unsigned* roots = base + ntiles_max;
    unsigned* lab = (unsigned*)labels;

    hipLaunchKernelGGL(sgm_components_tile_k, dim3(cc_blocks(c.tiles)), dim3(CC_THREADS), 0, st, c, pl, (const unsigned*)voxels, lab, size);
    HIP_TRY(hipGetLastError());
    if (c.tiles > 1u) {
        hipLaunchKernelGGL(sgm_components_border_k, dim3(cc_blocks(cc_div_up(c.n, CC_THREADS))), dim3(CC_THREADS), 0, st, c, lab);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(sgm_components_sizes_k, dim3(cc_blocks(cc_div_up(c.n, CC_THREADS))), dim3(CC_THREADS), 0, st, c.n, lab, size);
        HIP_TRY(hipGetLastError());
    }
    const unsigned tile = tile_size(n), ntiles = cc_div_up(c.n, tile);
    hipLaunchKernelGGL(sgm_components_label_k, dim3(ntiles), dim3(TILE_THREADS), 0, st, c.n, tile, c.min_voxels, lab, (const unsigned*)size,
                       kept, roots);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sgm_components_scan_k, dim3(1), dim3(SCAN_THREADS), 0, st, (const unsigned*)kept, (const unsigned*)roots, ntiles, base,
                       (unsigned*)counts);
    HIP_TRY(hipGetLastError());
    if (capacity == 0) return 0;                              // labels and counts are all that was asked for
    hipLaunchKernelGGL(sgm_components_emit_k, dim3(ntiles), dim3(TILE_THREADS), 0, st, c.n, tile, (const unsigned*)lab, size,
                       (const unsigned*)kept, (const unsigned*)base, (Component*)objects, boxes, capacity);
    HIP_TRY(hipGetLastError());
    const unsigned stiles_y = cc_div_up(c.ny, CC_SY), stiles = c.tiles_x * stiles_y * cc_div_up(c.nz, CC_SZ);
    hipLaunchKernelGGL(sgm_components_stats_k, dim3(cc_blocks(stiles)), dim3(CC_THREADS), 0, st, c, stiles_y, stiles, (const unsigned*)lab,
                       (const unsigned*)size, (Component*)objects, boxes);
    HIP_TRY(hipGetLastError());
    const size_t most = cc_objects_max(n, capacity);
    hipLaunchKernelGGL(sgm_components_box_k, dim3(cc_blocks((most + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st,
                       (const unsigned*)counts, capacity, (const ComponentBox*)boxes, (Component*)objects);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_volume_component_of(int ord, void* stream, const sgmd_volume* v, const void* labels, const void* objects, size_t capacity,
                             const void* counts, const void* records, size_t records_capacity, const void* records_count, int id_kinds,
                             void* index)
{
    if (!volume_ok(v) || !labels || !counts || (!objects && capacity) || !records || !index || records_capacity == 0 ||
        (id_kinds != 4 && id_kinds != 8) || (uintptr_t)labels % 4 != 0 || (uintptr_t)objects % 8 != 0 || (uintptr_t)counts % 4 != 0 ||
        (uintptr_t)records % 16 != 0 || (uintptr_t)records_count % 4 != 0 || (uintptr_t)index % 4 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_component_of: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const unsigned nx = (unsigned)v->nx, ny = (unsigned)v->ny, nz = (unsigned)v->nz;
    hipLaunchKernelGGL(sgm_component_of_k, dim3(cc_blocks((records_capacity + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0,
                       (hipStream_t)stream, nx, ny, nz, nx * ny * nz, (const unsigned*)labels, (const Component*)objects, capacity,
                       (const unsigned*)counts, (const ListRecord*)records, records_capacity, (const unsigned*)records_count,
                       (unsigned)id_kinds, (unsigned*)index);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
