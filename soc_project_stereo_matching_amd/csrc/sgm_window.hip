#include "sgm_common.hpp"
#include "sgm_volume_common.hpp"

// A window of the TSDF volume (include/sgm_mi355x.h, the moving-volume section): a box of the voxel lattice copied into another
// volume array at an integer voxel offset, zero where the source has nothing.  The primitive of a volume that follows the rig: the
// shift is one launch, a slab that leaves is one launch into a small array of its own, and every other entry point takes the result
// as it takes any volume.
//
//   sgm_volume_window_k<V, ALIGNED, COLOR>   one launch, no scratch, no LDS, no atomics: the same bytes on every run.  An item is V
//               consecutive destination voxels of one row: V == 4 where dims[0] % 4 == 0 and the destination arrays can be accessed
//               16 bytes at a time (one 16-byte store per array), else V == 1.  Every destination word is written exactly once, by
//               the lane that owns its item; the source is only read.  A row that maps outside the source in y or z is zero-filled
//               without a load.  ALIGNED (V == 4 only): the source row stride and offset[0] are multiples of 4 and the source
//               arrays 16-byte aligned, so every group that lies inside the source is one 16-byte load; otherwise a group is loaded
//               element by element, as is one that straddles the source's edge in x.  COLOR: the colour words travel the same way
//               in the same launch.  A bounded grid of at most WIN_MAX_BLOCKS workgroups whose lanes stride over the items (one lap
//               is WIN_MAX_BLOCKS * WIN_THREADS items); word indices are 64 bits wide where they are scaled to bytes: 2^30 words
//               are 2^32 bytes.

#define WIN_THREADS 256
#define WIN_MAX_BLOCKS 2048                                   // 8 waves on every SIMD of 256 CUs; the lanes stride beyond

struct WindowParams {
    unsigned dnx, dny;         // the destination's row length and rows per layer
    unsigned snx, sny, snz;    // the source grid
    int ox, oy, oz;            // destination (i, j, k) reads source (i + ox, j + oy, k + oz)
    unsigned per_row;          // items of a destination row: dnx / V
    unsigned items;            // per_row * dny * dnz <= 2^30
};

// the words of one item from one source array; row: the first word of the source row, si: the item's first x in the source
template <int V, bool ALIGNED>
static __device__ __forceinline__ void window_load(const WindowParams& w, const unsigned* __restrict__ src, size_t row, int si, unsigned (&out)[V])
{
    if constexpr (V == 4) {
        if (si >= 0 && si + 3 < (int)w.snx) {                 // the whole group inside
            if constexpr (ALIGNED) {
                const uint4 q = *(const uint4*)(src + row + (size_t)si);
                out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) out[e] = src[row + (size_t)(si + e)];
            }
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {                             // one voxel, or a group across the source's edge in x
        const int x = si + e;
        out[e] = (x >= 0 && x < (int)w.snx) ? src[row + (size_t)x] : 0u;
    }
}

template <int V>
static __device__ __forceinline__ void window_store(unsigned* __restrict__ dst, size_t at, const unsigned (&v)[V])
{
    if constexpr (V == 4)
        *(uint4*)(dst + at) = make_uint4(v[0], v[1], v[2], v[3]);
    else
        dst[at] = v[0];
}

template <int V, bool ALIGNED, bool COLOR>
__global__ __launch_bounds__(WIN_THREADS) void sgm_volume_window_k(WindowParams w, const unsigned* __restrict__ src_voxels,
                                                                   const unsigned* __restrict__ src_colors,
                                                                   unsigned* __restrict__ dst_voxels, unsigned* __restrict__ dst_colors)
{
    const unsigned stride = gridDim.x * WIN_THREADS;          // items < 2^30 and stride <= 2^19: the sum stays below 2^32
    for (unsigned item = blockIdx.x * WIN_THREADS + threadIdx.x; item < w.items; item += stride) {
        const unsigned drow = item / w.per_row;
        const unsigned i = (item - drow * w.per_row) * V;
        const unsigned k = drow / w.dny;
        const unsigned j = drow - k * w.dny;
        const int sj = (int)j + w.oy, sk = (int)k + w.oz, si = (int)i + w.ox;
        unsigned vox[V], col[V];
#pragma unroll
        for (int e = 0; e < V; ++e) vox[e] = col[e] = 0u;
        // (a row outside the source in y or z, or a group wholly outside in x: zero-filled without a load)
        if (sj >= 0 && sj < (int)w.sny && sk >= 0 && sk < (int)w.snz && si + (V - 1) >= 0 && si < (int)w.snx) {
            const size_t row = ((size_t)sk * w.sny + (size_t)sj) * w.snx;
            window_load<V, ALIGNED>(w, src_voxels, row, si, vox);
            if constexpr (COLOR) window_load<V, ALIGNED>(w, src_colors, row, si, col);
        }
        const size_t at = (size_t)item * V;                   // == (drow * dnx + i): the rows of the destination are dense
        window_store<V>(dst_voxels, at, vox);
        if constexpr (COLOR) window_store<V>(dst_colors, at, col);
    }
}

extern "C" {

int sgmd_volume_window(int ord, void* stream, const sgmd_volume* src, const int* offset, const int* dims, const void* src_voxels,
                       const void* src_colors, void* dst_voxels, void* dst_colors)
{
    const bool color = src_colors != nullptr;
    bool ok = volume_ok(src) && offset && dims && src_voxels && dst_voxels && (src_colors == nullptr) == (dst_colors == nullptr) &&
              (uintptr_t)src_voxels % 4 == 0 && (uintptr_t)src_colors % 4 == 0 && (uintptr_t)dst_voxels % 4 == 0 && (uintptr_t)dst_colors % 4 == 0;
    for (int a = 0; ok && a < 3; ++a) ok = dims[a] >= 1 && dims[a] <= 1024 && offset[a] >= -(1 << 20) && offset[a] <= (1 << 20);
    if (!ok || (unsigned long long)dims[0] * dims[1] * dims[2] > (1ull << 30)) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_window: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    // four voxels per lane where a destination row is a whole number of them and the destination arrays take 16-byte stores;
    // 16-byte loads where that holds for every group of the launch
    const bool four = dims[0] % 4 == 0 && (uintptr_t)dst_voxels % 16 == 0 && (uintptr_t)dst_colors % 16 == 0;
    const bool aligned = four && src->nx % 4 == 0 && offset[0] % 4 == 0 && (uintptr_t)src_voxels % 16 == 0 && (uintptr_t)src_colors % 16 == 0;
    WindowParams w;
    w.dnx = (unsigned)dims[0]; w.dny = (unsigned)dims[1];
    w.snx = (unsigned)src->nx; w.sny = (unsigned)src->ny; w.snz = (unsigned)src->nz;
    w.ox = offset[0]; w.oy = offset[1]; w.oz = offset[2];
    w.per_row = four ? w.dnx / 4 : w.dnx;
    w.items = w.per_row * w.dny * (unsigned)dims[2];
    const unsigned blocks = (w.items + WIN_THREADS - 1) / WIN_THREADS;
    const dim3 grid(blocks > WIN_MAX_BLOCKS ? WIN_MAX_BLOCKS : blocks);
#define WIN_LAUNCH(V, ALIGNED, COLOR)                                                                                                    \
    hipLaunchKernelGGL((sgm_volume_window_k<V, ALIGNED, COLOR>), grid, dim3(WIN_THREADS), 0, (hipStream_t)stream, w,                     \
                       (const unsigned*)src_voxels, (const unsigned*)src_colors, (unsigned*)dst_voxels, (unsigned*)dst_colors)
    if (color) {
        if (aligned) WIN_LAUNCH(4, true, true); else if (four) WIN_LAUNCH(4, false, true); else WIN_LAUNCH(1, false, true);
    } else {
        if (aligned) WIN_LAUNCH(4, true, false); else if (four) WIN_LAUNCH(4, false, false); else WIN_LAUNCH(1, false, false);
    }
#undef WIN_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
