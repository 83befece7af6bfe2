#pragma once
// The predicate, the formulas and the load paths of the point clouds (include/sgm_mi355x.h, sgm_cloud_spec), shared by the
// translation units that turn a disparity map into 3-D points: sgm_cloud.hip and sgm_register.hip.  Include after sgm_common.hpp.

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
