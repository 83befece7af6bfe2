#include "sgm_common.hpp"
#include "sgm_cloud_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): disparity maps to 3-D points on the device.  The
// contract is written out in include/sgm_mi355x.h (sgm_cloud_spec); tests/cloud_ref.py restates it
// in numpy.
//
// One predicate and one set of formulas (cloud_kept, cloud_xy) feed two products:
//   organised cloud   one element-wise launch, X Y Z or three quiet NaNs per pixel
//   point list        the kept pixels only, packed in raster order: an ORDERED stream compaction
//
// The point list takes three launches, ordered by the stream and by nothing else:
//   count   one workgroup per tile (a power-of-two run of at most 2048 pixels of ONE frame) -> kept[tile]
//   scan    ONE workgroup: exclusive prefix of kept[] -> base[tile]; a frame's first tile gives offsets[f]
//   emit    the tiling of `count`; the predicate is evaluated again (4 B read per pixel against 16 B written
//           per kept point: cheaper than storing it), the rank of a kept pixel inside its wave comes from
//           ballots and mbcnt, the waves' and passes' bases go through LDS; one 16-byte store per kept pixel
// No kernel reads what another workgroup of the same launch writes, nothing waits for another
// workgroup, and no atomic decides a place: the list is the same on every run.
//
// Loads: four consecutive pixels per lane (one 16-byte load of the map) where cloud_vector allows
// it, else one pixel per lane; wave_rank (sgm_cloud_common.hpp) has the rank that follows from it.
//
// (this translation unit is compiled with -fno-honor-nans like the others: a caller's map may hold
// NaN, so "finite" is tested on the bit pattern and NaN is made from bits)
// ============================================================================================

#define CLOUD_THREADS 256                                     // the organised cloud's; the point list's kernels run TILE_THREADS
#define CLOUD_QNAN 0x7FC00000u

// ---- organised cloud: float [frames][H][W][3] ------------------------------------------------------------------------------

template <int V>
__global__ __launch_bounds__(CLOUD_THREADS) void sgm_cloud_organized_k(CloudParams c, size_t n, const float* __restrict__ disp,
                                                                       const uint8_t* __restrict__ mask,
                                                                       const uint16_t* __restrict__ conf, float* __restrict__ xyz)
{
    const size_t g = ((size_t)blockIdx.x * CLOUD_THREADS + threadIdx.x) * V;     // V == 4: npx % 4 == 0, the four share a frame
    if (g >= n) return;
    float d[V];
    unsigned m[V], k[V];
    cloud_load<V>(disp, mask, conf, g, true, d, m, k);
    const unsigned p = (unsigned)(g % c.npx);
    unsigned y = p / c.W, x = p - y * c.W;
    unsigned o[3 * V];                                        // bit patterns: the NaN never passes through a float operation
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float X, Y, Z;
        const bool keep = cloud_kept(c, d[i], m[i], k[i], Z);
        cloud_xy(c, x, y, Z, X, Y);
        o[3 * i] = keep ? __float_as_uint(X) : CLOUD_QNAN;
        o[3 * i + 1] = keep ? __float_as_uint(Y) : CLOUD_QNAN;
        o[3 * i + 2] = keep ? __float_as_uint(Z) : CLOUD_QNAN;
        if (++x == c.W) { x = 0; ++y; }
    }
    unsigned* out = reinterpret_cast<unsigned*>(xyz) + g * 3;
    if constexpr (V == 4) {                                   // 48 bytes at a multiple of 48: three 16-byte stores
        uint4* o4 = reinterpret_cast<uint4*>(out);
        o4[0] = make_uint4(o[0], o[1], o[2], o[3]);
        o4[1] = make_uint4(o[4], o[5], o[6], o[7]);
        o4[2] = make_uint4(o[8], o[9], o[10], o[11]);
    } else {
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    }
}

// ---- point list ------------------------------------------------------------------------------------------------------------

// what a tile is: tiles_per_frame runs of `tile` pixels (a power of two, the last run of a frame shorter), frame-major
struct CloudTiling { unsigned tile, tiles_per_frame; };

// The kept pixels of one pass of a workgroup over its tile: this lane's V pixels start at frame-relative index p (>= end: none).
// Returns the lane's kept flags (bit i: pixel i) and, through the references, how many kept pixels the wave's lower lanes hold
// and the wave's total.
template <int V>
static __device__ __forceinline__ unsigned cloud_pass(const CloudParams& c, const float* __restrict__ disp,
                                                      const uint8_t* __restrict__ mask, const uint16_t* __restrict__ conf,
                                                      size_t frame_base, unsigned p, unsigned end, float (&Z)[V], unsigned& lower,
                                                      unsigned& wave_total)
{
    float d[V];
    unsigned m[V], k[V];
    cloud_load<V>(disp, mask, conf, frame_base + p, p < end, d, m, k);
    unsigned flags = 0;
    lower = wave_total = 0;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const bool keep = cloud_kept(c, d[i], m[i], k[i], Z[i]);
        wave_rank(keep, lower, wave_total);
        flags |= keep ? 1u << i : 0u;
    }
    return flags;
}

template <int V>
__global__ __launch_bounds__(TILE_THREADS) void sgm_cloud_count_k(CloudParams c, CloudTiling t, const float* __restrict__ disp,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const uint16_t* __restrict__ conf, unsigned* __restrict__ kept)
{
    const unsigned frame = blockIdx.x / t.tiles_per_frame, first = (blockIdx.x - frame * t.tiles_per_frame) * t.tile;
    const unsigned end = min(first + t.tile, c.npx);
    const size_t frame_base = (size_t)frame * c.npx;
    unsigned total = 0;                                       // of this wave, the same in all of its lanes
    for (unsigned p = first + threadIdx.x * V; p - threadIdx.x * V < end; p += TILE_THREADS * V) {
        float Z[V];
        unsigned lower, wave_total;
        cloud_pass<V>(c, disp, mask, conf, frame_base, p, end, Z, lower, wave_total);
        total += wave_total;
    }
    tile_total(total, kept + blockIdx.x);
}

// ONE workgroup: base[i] = kept[0] + .. + kept[i - 1]; offsets[f] = base of frame f's first tile, offsets[frames] = the total.
// (tile_scan of sgm_cloud_common.hpp: any number of tiles works)
__global__ __launch_bounds__(SCAN_THREADS) void sgm_cloud_scan_k(const unsigned* __restrict__ kept, unsigned ntiles,
                                                                 unsigned tiles_per_frame, unsigned frames,
                                                                 unsigned* __restrict__ base, unsigned* __restrict__ offsets)
{
    const unsigned total = tile_scan(kept, ntiles, base, [&](unsigned i, unsigned run) {
        const unsigned f = i / tiles_per_frame;
        if (i == f * tiles_per_frame) offsets[f] = run;
    });
    if (threadIdx.x == 0) offsets[frames] = total;
}

struct __attribute__((aligned(16))) CloudPoint { float x, y, z; unsigned pixel; };

template <int V>
__global__ __launch_bounds__(TILE_THREADS) void sgm_cloud_emit_k(CloudParams c, CloudTiling t, const float* __restrict__ disp,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const uint16_t* __restrict__ conf,
                                                                 const unsigned* __restrict__ base, CloudPoint* __restrict__ points)
{
    const unsigned frame = blockIdx.x / t.tiles_per_frame, first = (blockIdx.x - frame * t.tiles_per_frame) * t.tile;
    const unsigned end = min(first + t.tile, c.npx);
    const size_t frame_base = (size_t)frame * c.npx;
    size_t run = base[blockIdx.x];                            // where this pass's first kept pixel goes
    unsigned turn = 0;
    for (unsigned p = first + threadIdx.x * V; p - threadIdx.x * V < end; p += TILE_THREADS * V, turn ^= 1u) {
        float Z[V];
        unsigned lower, wave_total, all;
        const unsigned flags = cloud_pass<V>(c, disp, mask, conf, frame_base, p, end, Z, lower, wave_total);
        const unsigned before = pass_before(wave_total, turn, all);
        if (flags) {
            size_t at = run + before + lower;
            unsigned y = p / c.W, x = p - y * c.W;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (flags & (1u << i)) {
                    CloudPoint q;
                    cloud_xy(c, x, y, Z[i], q.x, q.y);
                    q.z = Z[i];
                    q.pixel = (y << 16) | x;
                    points[at++] = q;
                }
                if (++x == c.W) { x = 0; ++y; }
            }
        }
        run += all;
    }
}

// tiles never span frames: every frame has its own, so that offsets[f] is the base of a tile
static CloudTiling cloud_tiling(int W, int H)
{
    const size_t npx = (size_t)W * H;
    CloudTiling t;
    t.tile = tile_size(npx);
    t.tiles_per_frame = (unsigned)((npx + t.tile - 1) / t.tile);
    return t;
}

extern "C" {

size_t sgmd_cloud_scratch_bytes(int W, int H, int B)
{
    if (W < 1 || H < 1 || B < 1) return 0;
    return tile_scratch_bytes((size_t)cloud_tiling(W, H).tiles_per_frame * (size_t)B);
}

int sgmd_cloud_organized(int ord, void* stream, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, void* xyz)
{
    if (!cloud_shape_ok(c) || !disp || !xyz) {
        fprintf(stderr, "sgm_mi355x: sgmd_cloud_organized: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const size_t n = (size_t)c->W * c->H * c->B;
    const CloudParams p = cloud_params(c);
    if (cloud_vector(c, disp, mask, conf) && (uintptr_t)xyz % 16 == 0)
        hipLaunchKernelGGL(sgm_cloud_organized_k<4>, dim3((unsigned)((n / 4 + CLOUD_THREADS - 1) / CLOUD_THREADS)), dim3(CLOUD_THREADS),
                           0, (hipStream_t)stream, p, n, (const float*)disp, (const uint8_t*)mask, (const uint16_t*)conf, (float*)xyz);
    else
        hipLaunchKernelGGL(sgm_cloud_organized_k<1>, dim3((unsigned)((n + CLOUD_THREADS - 1) / CLOUD_THREADS)), dim3(CLOUD_THREADS), 0,
                           (hipStream_t)stream, p, n, (const float*)disp, (const uint8_t*)mask, (const uint16_t*)conf, (float*)xyz);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_cloud_points(int ord, void* stream, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, void* scratch,
                      void* points, void* offsets)
{
    if (!cloud_shape_ok(c) || !disp || !points || !scratch || !offsets || (uintptr_t)points % 16 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_cloud_points: bad arguments\n");
        return -1;
    }
    const CloudTiling t = cloud_tiling(c->W, c->H);
    const size_t ntiles = (size_t)t.tiles_per_frame * c->B;
    if (ntiles > 0x7FFFFFFFu) {
        fprintf(stderr, "sgm_mi355x: sgmd_cloud_points: %zu tiles are more than one launch takes\n", ntiles);
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const CloudParams p = cloud_params(c);
    const TileScratch s = tile_scratch(scratch, ntiles);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = cloud_vector(c, disp, mask, conf);
    if (vec)
        hipLaunchKernelGGL(sgm_cloud_count_k<4>, dim3((unsigned)ntiles), dim3(TILE_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, s.kept);
    else
        hipLaunchKernelGGL(sgm_cloud_count_k<1>, dim3((unsigned)ntiles), dim3(TILE_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, s.kept);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sgm_cloud_scan_k, dim3(1), dim3(SCAN_THREADS), 0, st, (const unsigned*)s.kept, (unsigned)ntiles, t.tiles_per_frame,
                       (unsigned)c->B, s.base, (unsigned*)offsets);
    HIP_TRY(hipGetLastError());
    if (vec)
        hipLaunchKernelGGL(sgm_cloud_emit_k<4>, dim3((unsigned)ntiles), dim3(TILE_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, (const unsigned*)s.base, (CloudPoint*)points);
    else
        hipLaunchKernelGGL(sgm_cloud_emit_k<1>, dim3((unsigned)ntiles), dim3(TILE_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, (const unsigned*)s.base, (CloudPoint*)points);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
