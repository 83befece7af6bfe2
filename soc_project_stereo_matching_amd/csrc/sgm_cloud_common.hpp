#pragma once
// The predicate, the formulas and the load paths of the point clouds (include/sgm_mi355x.h, sgm_cloud_spec), shared by the
// translation units that turn a disparity map into 3-D points: sgm_cloud.hip, sgm_register.hip and sgm_volume.hip; and the scan of
// the ordered compactions of sgm_cloud.hip and sgm_volume.hip.  Include after sgm_common.hpp.

struct CloudParams {
    float fx, fy, cx, cy, fb, doffs, z_min, z_max;
    unsigned min_conf;
    unsigned W;
    unsigned npx;              // pixels of one frame
};

static __device__ __forceinline__ bool cloud_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// THE predicate.  mask / conf: the pixel's values, 1 / 65535 where the caller gave no map.
static __device__ __forceinline__ bool cloud_kept(const CloudParams& c, float d, unsigned mask, unsigned conf, float& Z)
{
    const float den = d + c.doffs;
    Z = c.fb / den;
    const bool den_ok = cloud_finite(den) && den > 0.0f;
    return cloud_finite(d) && mask != 0u && conf >= c.min_conf && den_ok && cloud_finite(Z) && c.z_min <= Z && Z <= c.z_max;
}

static __device__ __forceinline__ void cloud_xy(const CloudParams& c, unsigned x, unsigned y, float Z, float& X, float& Y)
{
    X = (((float)x - c.cx) * Z) / c.fx;
    Y = (((float)y - c.cy) * Z) / c.fy;
}

// The scan of an ordered compaction's three launches (count per tile, scan, emit), for ONE workgroup of SCAN_THREADS:
// base[i] = kept[0] + .. + kept[i - 1], at_tile(i, base[i]) for every tile, the total as the result (in every thread).
// Chunks of 4 * 1024 tiles with a running carry, so any number of tiles works.
#define SCAN_THREADS 1024
#define SCAN_PER_THREAD 4
template <class AtTile>
static __device__ __forceinline__ unsigned tile_scan(const unsigned* __restrict__ kept, unsigned ntiles, unsigned* __restrict__ base,
                                                     AtTile at_tile)
{
    __shared__ unsigned s_wave[2][SCAN_THREADS / 64];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned carry = 0, turn = 0;
    for (unsigned chunk = 0; chunk < ntiles; chunk += SCAN_THREADS * SCAN_PER_THREAD, turn ^= 1u) {
        const unsigned i0 = chunk + threadIdx.x * SCAN_PER_THREAD;
        unsigned v[SCAN_PER_THREAD], mine = 0;
#pragma unroll
        for (int j = 0; j < SCAN_PER_THREAD; ++j) {
            v[j] = i0 + j < ntiles ? kept[i0 + j] : 0u;
            mine += v[j];
        }
        unsigned incl = mine;                                 // inclusive prefix over the wave's lanes
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const unsigned up = __shfl_up(incl, step);
            if (lane >= (unsigned)step) incl += up;
        }
        if (lane == 63) s_wave[turn][wave] = incl;
        __syncthreads();                                      // (the other half of s_wave is what the previous chunk still reads)
        unsigned before = 0, all = 0;
#pragma unroll
        for (unsigned w = 0; w < SCAN_THREADS / 64; ++w) {
            const unsigned s = s_wave[turn][w];
            before += w < wave ? s : 0u;
            all += s;
        }
        unsigned run = carry + before + incl - mine;
#pragma unroll
        for (int j = 0; j < SCAN_PER_THREAD; ++j) {
            const unsigned i = i0 + j;
            if (i < ntiles) {
                base[i] = run;
                at_tile(i, run);
            }
            run += v[j];
        }
        carry += all;
    }
    return carry;
}

// V consecutive pixels of one frame starting at frame-relative index p (p % V == 0 with V == 4), those at or past `end` read
// as dropped: the map value and the two optional side maps
template <int V>
static __device__ __forceinline__ void cloud_load(const float* __restrict__ disp, const uint8_t* __restrict__ mask,
                                                  const uint16_t* __restrict__ conf, size_t g, bool live, float (&d)[V],
                                                  unsigned (&m)[V], unsigned (&k)[V])
{
#pragma unroll
    for (int i = 0; i < V; ++i) { d[i] = __uint_as_float(0x7F800000u); m[i] = 1u; k[i] = 65535u; }
    if (!live) return;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(disp + g);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
        if (mask) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(mask + g);
            m[0] = w & 255u; m[1] = (w >> 8) & 255u; m[2] = (w >> 16) & 255u; m[3] = w >> 24;
        }
        if (conf) {
            const uint2 w = *reinterpret_cast<const uint2*>(conf + g);
            k[0] = w.x & 0xFFFFu; k[1] = w.x >> 16; k[2] = w.y & 0xFFFFu; k[3] = w.y >> 16;
        }
    } else {
        d[0] = disp[g];
        if (mask) m[0] = mask[g];
        if (conf) k[0] = conf[g];
    }
}
