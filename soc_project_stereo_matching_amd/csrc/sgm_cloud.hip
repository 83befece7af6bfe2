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
// Loads: four pixels per lane (one 16-byte load of the map) where a frame's pixel count and the
// pointers allow it, else one pixel per lane.  A lane's pixels are consecutive, so raster order is
// lane-major, then the lane's own pixels: the rank of pixel k of a lane is the number of kept pixels
// in lower lanes (the sum over k of mbcnt(ballot_k)) plus the kept ones among the lane's first k.
//
// (this translation unit is compiled with -fno-honor-nans like the others: a caller's map may hold
// NaN, so "finite" is tested on the bit pattern and NaN is made from bits)
// ============================================================================================

#define CLOUD_THREADS 256
#define CLOUD_WAVES (CLOUD_THREADS / 64)
#define CLOUD_TILE_MAX 2048
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
        const unsigned long long b = __ballot(keep);
        lower += __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        wave_total += (unsigned)__popcll(b);
        flags |= keep ? 1u << i : 0u;
    }
    return flags;
}

template <int V>
__global__ __launch_bounds__(CLOUD_THREADS) void sgm_cloud_count_k(CloudParams c, CloudTiling t, const float* __restrict__ disp,
                                                                   const uint8_t* __restrict__ mask,
                                                                   const uint16_t* __restrict__ conf, unsigned* __restrict__ kept)
{
    __shared__ unsigned s_wave[CLOUD_WAVES];
    const unsigned frame = blockIdx.x / t.tiles_per_frame, first = (blockIdx.x - frame * t.tiles_per_frame) * t.tile;
    const unsigned end = min(first + t.tile, c.npx);
    const size_t frame_base = (size_t)frame * c.npx;
    unsigned total = 0;                                       // of this wave, the same in all of its lanes
    for (unsigned p = first + threadIdx.x * V; p - threadIdx.x * V < end; p += CLOUD_THREADS * V) {
        float Z[V];
        unsigned lower, wave_total;
        cloud_pass<V>(c, disp, mask, conf, frame_base, p, end, Z, lower, wave_total);
        total += wave_total;
    }
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < CLOUD_WAVES; ++w) sum += s_wave[w];
        kept[blockIdx.x] = sum;
    }
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
__global__ __launch_bounds__(CLOUD_THREADS) void sgm_cloud_emit_k(CloudParams c, CloudTiling t, const float* __restrict__ disp,
                                                                  const uint8_t* __restrict__ mask,
                                                                  const uint16_t* __restrict__ conf,
                                                                  const unsigned* __restrict__ base, CloudPoint* __restrict__ points)
{
    __shared__ unsigned s_wave[2][CLOUD_WAVES];
    const unsigned frame = blockIdx.x / t.tiles_per_frame, first = (blockIdx.x - frame * t.tiles_per_frame) * t.tile;
    const unsigned end = min(first + t.tile, c.npx);
    const size_t frame_base = (size_t)frame * c.npx;
    const unsigned wave = threadIdx.x >> 6;
    size_t run = base[blockIdx.x];                            // where this pass's first kept pixel goes
    unsigned turn = 0;
    for (unsigned p = first + threadIdx.x * V; p - threadIdx.x * V < end; p += CLOUD_THREADS * V, turn ^= 1u) {
        float Z[V];
        unsigned lower, wave_total;
        const unsigned flags = cloud_pass<V>(c, disp, mask, conf, frame_base, p, end, Z, lower, wave_total);
        if ((threadIdx.x & 63u) == 0) s_wave[turn][wave] = wave_total;
        __syncthreads();                                      // (the other half of s_wave is what the previous pass still reads)
        unsigned before = 0, all = 0;
#pragma unroll
        for (unsigned w = 0; w < CLOUD_WAVES; ++w) {
            const unsigned s = s_wave[turn][w];
            before += w < wave ? s : 0u;
            all += s;
        }
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

static CloudParams cloud_params(const sgmd_cloud* c)
{
    CloudParams p;
    p.fx = c->fx; p.fy = c->fy; p.cx = c->cx; p.cy = c->cy; p.fb = c->fb; p.doffs = c->doffs; p.z_min = c->z_min; p.z_max = c->z_max;
    p.min_conf = c->min_conf;
    p.W = (unsigned)c->W;
    p.npx = (unsigned)((size_t)c->W * c->H);
    return p;
}

static bool cloud_args_ok(const sgmd_cloud* c, const void* disp, const void* out)
{
    return c && disp && out && c->W >= 1 && c->H >= 1 && c->W <= 65535 && c->H <= 65535 && c->B >= 1 &&
           (unsigned long long)c->W * c->H * c->B <= (1ull << 31);
}

// four pixels per lane: every frame starts at a multiple of four pixels and the three maps can be read 16 / 4 / 8 bytes at a time
static bool cloud_vector(const sgmd_cloud* c, const void* disp, const void* mask, const void* conf)
{
    return ((size_t)c->W * c->H) % 4 == 0 && (uintptr_t)disp % 16 == 0 && (uintptr_t)mask % 4 == 0 && (uintptr_t)conf % 8 == 0;
}

static CloudTiling cloud_tiling(const sgmd_cloud* c)
{
    const size_t npx = (size_t)c->W * c->H;
    CloudTiling t;
    t.tile = 1;
    while (t.tile < CLOUD_TILE_MAX && t.tile < npx) t.tile <<= 1;
    t.tiles_per_frame = (unsigned)((npx + t.tile - 1) / t.tile);
    return t;
}

extern "C" {

size_t sgmd_cloud_scratch_bytes(int W, int H, int B)
{
    if (W < 1 || H < 1 || B < 1) return 0;
    const sgmd_cloud c = {W, H, B, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return 2 * sizeof(unsigned) * (size_t)cloud_tiling(&c).tiles_per_frame * (size_t)B;      // kept[], base[]
}

int sgmd_cloud_organized(int ord, void* stream, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, void* xyz)
{
    if (!cloud_args_ok(c, disp, xyz)) {
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
    if (!cloud_args_ok(c, disp, points) || !scratch || !offsets || (uintptr_t)points % 16 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_cloud_points: bad arguments\n");
        return -1;
    }
    const CloudTiling t = cloud_tiling(c);
    const size_t ntiles = (size_t)t.tiles_per_frame * c->B;
    if (ntiles > 0x7FFFFFFFu) {
        fprintf(stderr, "sgm_mi355x: sgmd_cloud_points: %zu tiles are more than one launch takes\n", ntiles);
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const CloudParams p = cloud_params(c);
    unsigned* kept = (unsigned*)scratch;
    unsigned* base = kept + ntiles;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = cloud_vector(c, disp, mask, conf);
    if (vec)
        hipLaunchKernelGGL(sgm_cloud_count_k<4>, dim3((unsigned)ntiles), dim3(CLOUD_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, kept);
    else
        hipLaunchKernelGGL(sgm_cloud_count_k<1>, dim3((unsigned)ntiles), dim3(CLOUD_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, kept);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sgm_cloud_scan_k, dim3(1), dim3(SCAN_THREADS), 0, st, (const unsigned*)kept, (unsigned)ntiles, t.tiles_per_frame,
                       (unsigned)c->B, base, (unsigned*)offsets);
    HIP_TRY(hipGetLastError());
    if (vec)
        hipLaunchKernelGGL(sgm_cloud_emit_k<4>, dim3((unsigned)ntiles), dim3(CLOUD_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, (const unsigned*)base, (CloudPoint*)points);
    else
        hipLaunchKernelGGL(sgm_cloud_emit_k<1>, dim3((unsigned)ntiles), dim3(CLOUD_THREADS), 0, st, p, t, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, (const unsigned*)base, (CloudPoint*)points);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
