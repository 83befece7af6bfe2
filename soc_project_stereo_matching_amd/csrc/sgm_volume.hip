#include "sgm_common.hpp"
#include "sgm_cloud_common.hpp"
#include "sgm_volume_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): depth maps with known poses fused into a truncated signed distance volume
// (TSDF), and the surface read back out as points.  The contract is written out in include/sgm_mi355x.h (sgm_volume_spec);
// tests/volume_ref.py restates it in numpy.
//
// Integration   ONE launch, owner-computes: a lane owns its voxels, loads their words once, walks the frames of the batch in
//               order with the words in registers and stores them once -- no atomics and no order between workgroups, so a call
//               over B frames is B calls of one frame, bit for bit.  Per voxel and frame: the voxel centre into the camera
//               (the poses are kernel arguments, read with scalar loads), the pinhole, one gather of the source pixel (the
//               cloud's predicate, cloud_kept, decides whether it contributes and gives Z), the running average in integers.
//               Four consecutive-x voxels per lane with 16-byte loads and stores where nx % 4 == 0 and the pointer allows it,
//               else one voxel per lane.  A lane none of whose voxels was updated does not store.
// Extraction    the ordered compaction of sgm_cloud.hip with a lane contributing 0..3 records (one per axis) instead of 0..1:
//               count per tile, one scan (tile_scan), emit; three ballots give a record's rank inside its wave.  No atomic
//               decides a place: the list is sorted by id and the same on every run.
// Ray-cast      the volume rendered into depth and normal maps of a view (sgm_raycast_spec; tests/raycast_ref.py): one lane per
//               pixel, one launch for all frames; see the block further down.
// Colour        a second array of words beside the volume's, (cw << 24) | (b << 16) | (g << 8) | r (include/sgm_mi355x.h, the
//               colour section; tests/color_ref.py): the COLOR instantiations of the integration and of the ray-cast carry it along
//               -- the lane that owns a voxel owns its colour word, a hit reads eight more words -- and sgm_volume_colors_k gives a
//               colour to every record of a surface list or of a mesh's vertex list, one lane per record.
//
// (this translation unit is compiled with -fno-honor-nans like the others: "finite" is tested on the bit pattern, before any
// comparison)
// ============================================================================================

#define VOL_THREADS 256                                       // the integration's; the surface list's kernels run TILE_THREADS

// the source image as the integration needs it beside CloudParams
struct VolumeSource { float wf, hf; unsigned frames; };

// ---- integration ---------------------------------------------------------------------------------------------------------------

// the image of the coloured integration: u8 grey (channels 1) or u32 r | g << 8 | b << 16 (channels 4), registered to the map
struct VolumeImage { const void* pixels; unsigned channels; };

// c = (c*cw + p) / (cw + 1) rounded, halves up: every operand is below 2^17
static __device__ __forceinline__ unsigned color_average(unsigned c, unsigned cw, unsigned p)
{
    return (2u * (c * cw + p) + (cw + 1u)) / (2u * (cw + 1u));
}

// One frame's say on one voxel whose centre is (px, py, pz); true when the voxel was updated.  The parentheses are the contract's.
// COLOR: col is the voxel's colour word, which takes the source pixel's colour where the update has sdf <= trunc (coloured: it did).
template <bool COLOR>
static __device__ __forceinline__ bool volume_update(const VolumeParams& v, const CloudParams& c, const VolumeSource& s,
                                                     const float* P, size_t frame_base, const float* __restrict__ disp,
                                                     const uint8_t* __restrict__ mask, const uint16_t* __restrict__ conf, float px,
                                                     float py, float pz, int& tq, unsigned& w, const VolumeImage& image, unsigned& col,
                                                     bool& coloured)
{
    float Xp, Yp, Zp, uf, vf;
    pose_move(P, P + 9, px, py, pz, Xp, Yp, Zp);
    if (!pinhole_pixel(c.fx, c.fy, c.cx, c.cy, s.wf, s.hf, Xp, Yp, Zp, uf, vf)) return false;
    const size_t at = frame_base + (size_t)(unsigned)vf * c.W + (unsigned)uf;
    float Z;
    if (!cloud_kept(c, disp[at], mask ? mask[at] : 1u, conf ? conf[at] : 65535u, Z)) return false;
    const float sdf = Z - Zp;
    if (sdf < -v.trunc) return false;
    const int q = (int)rintf((fminf(sdf, v.trunc) / v.trunc) * 32767.0f);
    // num / den rounded to the nearest integer, halves up: |num| < 2^31, but 2 * num + den leaves int32 past w = 32767
    const int num = tq * (int)w + q, den = (int)w + 1;
    int quot = num / den, rem = num - quot * den;
    if (rem < 0) { rem += den; --quot; }
    tq = quot + (2 * rem >= den ? 1 : 0);
    w = min(w + 1u, v.max_weight);
    if constexpr (COLOR) {
        if (sdf <= v.trunc) {                                     // far in front of the surface: distance, no colour
            unsigned p;
            if (image.channels == 4u) {
                p = static_cast<const unsigned*>(image.pixels)[at] & 0xFFFFFFu;
            } else {
                p = static_cast<const uint8_t*>(image.pixels)[at];
                p |= (p << 8) | (p << 16);
            }
            const unsigned cw = col >> 24;
            const unsigned r = color_average(col & 0xFFu, cw, p & 0xFFu), g = color_average((col >> 8) & 0xFFu, cw, (p >> 8) & 0xFFu),
                           b = color_average((col >> 16) & 0xFFu, cw, p >> 16);
            col = (min(cw + 1u, min(v.max_weight, 255u)) << 24) | (b << 16) | (g << 8) | r;
            coloured = true;
        }
    }
    return true;
}

template <int V, bool COLOR>
__global__ __launch_bounds__(VOL_THREADS) void sgm_volume_integrate_k(VolumeParams v, CloudParams c, VolumeSource s, PoseBlock poses,
                                                                      const float* __restrict__ disp, const uint8_t* __restrict__ mask,
                                                                      const uint16_t* __restrict__ conf, unsigned* __restrict__ voxels,
                                                                      VolumeImage image, unsigned* __restrict__ colors)
{
    const unsigned g = (blockIdx.x * VOL_THREADS + threadIdx.x) * V;             // V == 4: nx % 4 == 0, the four share a row
    if (g >= v.n) return;
    unsigned i, j, k;
    volume_ijk(v, g, i, j, k);
    unsigned word[V], col[V];
    if constexpr (V == 4) {
        const uint4 t = *reinterpret_cast<const uint4*>(voxels + g);
        word[0] = t.x; word[1] = t.y; word[2] = t.z; word[3] = t.w;
    } else {
        word[0] = voxels[g];
    }
    if constexpr (COLOR && V == 4) {
        const uint4 t = *reinterpret_cast<const uint4*>(colors + g);
        col[0] = t.x; col[1] = t.y; col[2] = t.z; col[3] = t.w;
    } else if constexpr (COLOR) {
        col[0] = colors[g];
    }
    int tq[V];
    unsigned w[V];
    float px[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        tq[e] = (int)(short)(word[e] & 0xFFFFu);
        w[e] = word[e] >> 16;
        px[e] = volume_centre(v.ox, i + e, v.voxel);
    }
    const float py = volume_centre(v.oy, j, v.voxel), pz = volume_centre(v.oz, k, v.voxel);
    bool touched = false, coloured = false;
    for (unsigned f = 0; f < s.frames; ++f) {                                   // frames take effect in order
        const float* P = poses.p[f];
        const size_t frame_base = (size_t)f * c.npx;
#pragma unroll
        for (int e = 0; e < V; ++e)
            touched |= volume_update<COLOR>(v, c, s, P, frame_base, disp, mask, conf, px[e], py, pz, tq[e], w[e], image, col[e], coloured);
    }
    if (!touched) return;
#pragma unroll
    for (int e = 0; e < V; ++e) word[e] = (w[e] << 16) | ((unsigned)tq[e] & 0xFFFFu);
    if constexpr (V == 4)
        *reinterpret_cast<uint4*>(voxels + g) = make_uint4(word[0], word[1], word[2], word[3]);
    else
        voxels[g] = word[0];
    if constexpr (COLOR) {
        if (!coloured) return;
        if constexpr (V == 4)
            *reinterpret_cast<uint4*>(colors + g) = make_uint4(col[0], col[1], col[2], col[3]);
        else
            colors[g] = col[0];
    }
}

// ---- surface points ------------------------------------------------------------------------------------------------------------

// One pass of a workgroup over its tile: this lane's voxel n (not live: none).  Returns the lane's crossings (bit a: axis a) and,
// through the references, the voxel's place, its tq and its three neighbours', how many records the wave's lower lanes hold and
// the wave's total.
static __device__ __forceinline__ unsigned volume_pass(const VolumeParams& v, const unsigned* __restrict__ voxels, unsigned min_weight,
                                                       unsigned n, bool live, unsigned (&at)[3], int& tn, int (&tm)[3], unsigned& lower,
                                                       unsigned& wave_total)
{
    unsigned flags = 0;
    tn = 0;
    at[0] = at[1] = at[2] = 0;
    tm[0] = tm[1] = tm[2] = 0;
    if (live) {
        const unsigned word = voxels[n];
        volume_ijk(v, n, at[0], at[1], at[2]);
        if ((word >> 16) >= min_weight) {
            tn = (int)(short)(word & 0xFFFFu);
            const unsigned step[3] = {1u, v.nx, v.nx * v.ny};
            const bool inside[3] = {at[0] + 1 < v.nx, at[1] + 1 < v.ny, at[2] + 1 < v.nz};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (inside[a]) {
                    const unsigned other = voxels[n + step[a]];
                    tm[a] = (int)(short)(other & 0xFFFFu);
                    if ((other >> 16) >= min_weight && (tn < 0) != (tm[a] < 0)) flags |= 1u << a;
                }
            }
        }
    }
    lower = wave_total = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) wave_rank((flags >> a) & 1u, lower, wave_total);
    return flags;
}

__global__ __launch_bounds__(TILE_THREADS) void sgm_volume_count_k(VolumeParams v, unsigned tile, unsigned min_weight,
                                                                   const unsigned* __restrict__ voxels, unsigned* __restrict__ kept)
{
    const unsigned first = blockIdx.x * tile, end = min(first + tile, v.n);
    unsigned total = 0;                                       // of this wave, the same in all of its lanes
    for (unsigned p = first + threadIdx.x; p - threadIdx.x < end; p += TILE_THREADS) {
        unsigned at[3], lower, wave_total;
        int tn, tm[3];
        volume_pass(v, voxels, min_weight, p, p < end, at, tn, tm, lower, wave_total);
        total += wave_total;
    }
    tile_total(total, kept + blockIdx.x);
}

// ONE workgroup: base[i] = kept[0] + .. + kept[i - 1]; count[0] = the total
__global__ __launch_bounds__(SCAN_THREADS) void sgm_volume_scan_k(const unsigned* __restrict__ kept, unsigned ntiles,
                                                                  unsigned* __restrict__ base, unsigned* __restrict__ count)
{
    const unsigned total = tile_scan(kept, ntiles, base, [](unsigned, unsigned) {});
    if (threadIdx.x == 0) count[0] = total;
}

struct __attribute__((aligned(16))) SurfacePoint { float x, y, z; unsigned id; };

__global__ __launch_bounds__(TILE_THREADS) void sgm_volume_emit_k(VolumeParams v, unsigned tile, unsigned min_weight,
                                                                  const unsigned* __restrict__ voxels, const unsigned* __restrict__ base,
                                                                  SurfacePoint* __restrict__ points, size_t capacity)
{
    const unsigned first = blockIdx.x * tile, end = min(first + tile, v.n);
    size_t run = base[blockIdx.x];                            // where this pass's first record goes
    unsigned turn = 0;
    for (unsigned p = first + threadIdx.x; p - threadIdx.x < end; p += TILE_THREADS, turn ^= 1u) {
        unsigned at[3], lower, wave_total, all;
        int tn, tm[3];
        const unsigned flags = volume_pass(v, voxels, min_weight, p, p < end, at, tn, tm, lower, wave_total);
        const unsigned before = pass_before(wave_total, turn, all);
        if (flags) {
            size_t to = run + before + lower;
            const float centre[3] = {volume_centre(v.ox, at[0], v.voxel), volume_centre(v.oy, at[1], v.voxel),
                                     volume_centre(v.oz, at[2], v.voxel)};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (flags & (1u << a)) {
                    const float s = (float)tn / ((float)tn - (float)tm[a]);
                    const float moved = centre[a] + s * v.voxel;
                    SurfacePoint q;
                    q.x = a == 0 ? moved : centre[0];
                    q.y = a == 1 ? moved : centre[1];
                    q.z = a == 2 ? moved : centre[2];
                    q.id = p * 4u + (unsigned)a;
                    if (to < capacity) points[to] = q;
                    ++to;
                }
            }
        }
        run += all;
    }
}

// ---- ray-cast ------------------------------------------------------------------------------------------------------------------
// The volume rendered into depth and normal maps of a pinhole view (include/sgm_mi355x.h, sgm_raycast_spec; tests/raycast_ref.py
// restates it).  One lane per pixel, one launch for all frames (blockIdx.z: the frame, whose pose is read from the kernel
// arguments with scalar loads), no LDS, no atomics and no dependence between lanes: a lane marches its ray in Z, reads one word
// per sample, and at a front hit 16 words for the two trilinear values and 48 for the normal.
// A wave covers an 8 x 8 pixel tile, whose rays stay together in the volume, and the march starts and ends at the volume's box
// (ray_box below).
#define RAY_THREADS 256
#define RAY_BLOCK_W 32                                        // four 8 x 8 tiles side by side
#define RAY_BLOCK_H 8

struct RaycastView {
    unsigned W, H;
    float fx, fy, cx, cy, z_min, z_max, step;
    unsigned min_weight;
};

// The nearest sample at g: 0 invalid, 1 valid and non-negative, 2 valid and negative
static __device__ __forceinline__ unsigned ray_nearest(const VolumeParams& v, const unsigned* __restrict__ voxels, unsigned min_weight,
                                                       float gx, float gy, float gz)
{
    if (!cloud_finite(gx) || !cloud_finite(gy) || !cloud_finite(gz)) return 0u;
    // admitted in float, before any conversion to int; floorf of a value in [0, n) is its truncation
    if (!(0.0f <= gx && gx < (float)v.nx && 0.0f <= gy && gy < (float)v.ny && 0.0f <= gz && gz < (float)v.nz)) return 0u;
    const unsigned word = voxels[((unsigned)gz * v.ny + (unsigned)gy) * v.nx + (unsigned)gx];
    if ((word >> 16) < min_weight) return 0u;
    return (word & 0x8000u) ? 2u : 1u;
}

static __device__ __forceinline__ float ray_lerp(float p, float q, float s) { return p + s * (q - p); }

// F(g): the trilinear value of tq at h = g - 0.5, along x first, then y, then z; false where a word is missing or outside the grid
static __device__ __forceinline__ bool ray_trilinear(const VolumeParams& v, const unsigned* __restrict__ voxels, unsigned min_weight,
                                                     float gx, float gy, float gz, float& F)
{
    const float hx = gx - 0.5f, hy = gy - 0.5f, hz = gz - 0.5f;
    if (!cloud_finite(hx) || !cloud_finite(hy) || !cloud_finite(hz)) return false;
    const float ix = floorf(hx), iy = floorf(hy), iz = floorf(hz);
    if (!(0.0f <= ix && ix + 1.0f < (float)v.nx && 0.0f <= iy && iy + 1.0f < (float)v.ny && 0.0f <= iz && iz + 1.0f < (float)v.nz))
        return false;
    const float fx = hx - ix, fy = hy - iy, fz = hz - iz;
    const unsigned* at = voxels + (((unsigned)iz * v.ny + (unsigned)iy) * v.nx + (unsigned)ix);
    const unsigned sy = v.nx, sz = v.nx * v.ny;
    unsigned word[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) word[e] = at[(e & 1) + ((e >> 1) & 1) * sy + (e >> 2) * sz];
    bool ok = true;
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        ok = ok && (word[e] >> 16) >= min_weight;
        t[e] = (float)(int)(short)(word[e] & 0xFFFFu);
    }
    const float c00 = ray_lerp(t[0], t[1], fx), c10 = ray_lerp(t[2], t[3], fx), c01 = ray_lerp(t[4], t[5], fx), c11 = ray_lerp(t[6], t[7], fx);
    F = ray_lerp(ray_lerp(c00, c10, fy), ray_lerp(c01, c11, fy), fz);
    return ok;
}

// The part of the march that can meet the volume: on return every k < k0 and every Z_k > z_end has a sample outside the box, which
// the contract calls invalid -- skipping them changes no bit, and a skipped prefix leaves "no previous sample" as invalid samples
// do.  Per axis the slab [-m, n + m] in grid units, m = 1 voxel + 2^-20 of the magnitudes involved (the float slab test is some
// 2^-23 of them off), then one step on either side; k0 is taken only if Z_k0 itself, as the march computes it, lies below the
// entry (Z_k does not decrease with k).  Anything non-finite on the way: no skip.
static __device__ __forceinline__ void ray_box(const VolumeParams& v, const RaycastView& r, const float (&go)[3], const float (&gd)[3],
                                               unsigned& k0, float& z_end)
{
    const float n[3] = {(float)v.nx, (float)v.ny, (float)v.nz};
    float z_in = r.z_min, z_out = r.z_max;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!cloud_finite(go[i]) || !cloud_finite(gd[i])) return;
        if (gd[i] == 0.0f) continue;                          // (g_i == go_i all the way: the per-sample test decides)
        const float m = 1.0f + (fabsf(go[i]) + n[i]) * 9.5367431640625e-07f;
        const float za = (-m - go[i]) / gd[i], zb = ((n[i] + m) - go[i]) / gd[i];
        if (!cloud_finite(za) || !cloud_finite(zb)) return;
        z_in = fmaxf(z_in, fminf(za, zb) - r.step);
        z_out = fminf(z_out, fmaxf(za, zb) + r.step);
    }
    if (!cloud_finite(z_in) || !cloud_finite(z_out)) return;
    z_end = z_out;
    const float kf = floorf((z_in - r.z_min) / r.step) - 2.0f;
    if (cloud_finite(kf) && kf >= 1.0f && kf < 16777216.0f) {
        const unsigned k = (unsigned)kf;
        if (r.z_min + (float)k * r.step < z_in) k0 = k;
    }
}

// ---- colour ---------------------------------------------------------------------------------------------------------------------
// A colour word is (cw << 24) | (b << 16) | (g << 8) | r; cw == 0: the voxel has none.

// the three channels of p and q blended at s, each rounded to the nearest integer (halves to even), alpha 0xFF; clamp: to 0..255
// first (a blend of three lerps can leave the range by a rounding, one lerp with 0 <= s <= 1 cannot)
template <bool CLAMP, typename F>
static __device__ __forceinline__ unsigned color_pack(F channel)
{
    unsigned out = 0xFF000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float value = channel(8 * ch);
        if constexpr (CLAMP) value = fminf(fmaxf(value, 0.0f), 255.0f);
        out |= (unsigned)rintf(value) << (8 * ch);
    }
    return out;
}

// The colour at g: trilinear over the eight words of F(g)'s cell where all eight have a colour, else the word of the voxel g lies
// in, else 0
static __device__ __forceinline__ unsigned ray_color(const VolumeParams& v, const unsigned* __restrict__ colors, float gx, float gy,
                                                     float gz)
{
    const float hx = gx - 0.5f, hy = gy - 0.5f, hz = gz - 0.5f;
    if (cloud_finite(hx) && cloud_finite(hy) && cloud_finite(hz)) {
        const float ix = floorf(hx), iy = floorf(hy), iz = floorf(hz);
        if (0.0f <= ix && ix + 1.0f < (float)v.nx && 0.0f <= iy && iy + 1.0f < (float)v.ny && 0.0f <= iz && iz + 1.0f < (float)v.nz) {
            const float fx = hx - ix, fy = hy - iy, fz = hz - iz;
            const unsigned* at = colors + (((unsigned)iz * v.ny + (unsigned)iy) * v.nx + (unsigned)ix);
            const unsigned sy = v.nx, sz = v.nx * v.ny;
            unsigned word[8];
            bool all = true;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                word[e] = at[(e & 1) + ((e >> 1) & 1) * sy + (e >> 2) * sz];
                all = all && (word[e] >> 24) != 0u;
            }
            if (all)
                return color_pack<true>([&](int shift) {
                    float t[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) t[e] = (float)((word[e] >> shift) & 0xFFu);
                    const float c00 = ray_lerp(t[0], t[1], fx), c10 = ray_lerp(t[2], t[3], fx), c01 = ray_lerp(t[4], t[5], fx),
                                c11 = ray_lerp(t[6], t[7], fx);
                    return ray_lerp(ray_lerp(c00, c10, fy), ray_lerp(c01, c11, fy), fz);
                });
        }
    }
    // the march's admission of a sample, in float before any conversion
    if (!cloud_finite(gx) || !cloud_finite(gy) || !cloud_finite(gz)) return 0u;
    if (!(0.0f <= gx && gx < (float)v.nx && 0.0f <= gy && gy < (float)v.ny && 0.0f <= gz && gz < (float)v.nz)) return 0u;
    const unsigned word = colors[((unsigned)gz * v.ny + (unsigned)gy) * v.nx + (unsigned)gx];
    return (word >> 24) != 0u ? (0xFF000000u | word) : 0u;
}

template <bool NORMALS, bool COLOR>
__global__ __launch_bounds__(RAY_THREADS) void sgm_volume_raycast_k(VolumeParams v, RaycastView r, PoseBlock poses,
                                                                    const unsigned* __restrict__ voxels, float* __restrict__ depth,
                                                                    float* __restrict__ normal, const unsigned* __restrict__ colors,
                                                                    unsigned* __restrict__ rgba)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned x = blockIdx.x * RAY_BLOCK_W + (threadIdx.x >> 6) * 8u + (lane & 7u), y = blockIdx.y * RAY_BLOCK_H + (lane >> 3);
    if (x >= r.W || y >= r.H) return;
    const float* P = poses.p[blockIdx.z];                     // R row-major, then t: world -> camera
    const float a = ((float)x - r.cx) / r.fx, b = ((float)y - r.cy) / r.fy;
    const float origin[3] = {v.ox, v.oy, v.oz};
    float go[3], gd[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float c = -((P[i] * P[9] + P[3 + i] * P[10]) + P[6 + i] * P[11]);
        const float d = (P[i] * a + P[3 + i] * b) + P[6 + i];
        go[i] = (c - origin[i]) / v.voxel;
        gd[i] = d / v.voxel;
    }
    unsigned k = 0;
    float z_end = r.z_max;
    ray_box(v, r, go, gd, k, z_end);
    const float nan = __uint_as_float(0x7FC00000u);
    float Z = nan, nrm[3] = {nan, nan, nan};
    unsigned prev = 0, color = 0;                             // (color: of the COLOR instantiations; an empty pixel gets 0)
    float Zp = 0.0f;
    bool front = false;
    for (;; ++k) {
        const float Zk = r.z_min + (float)k * r.step;
        if (!(Zk <= z_end)) break;
        const unsigned cur = ray_nearest(v, voxels, r.min_weight, go[0] + Zk * gd[0], go[1] + Zk * gd[1], go[2] + Zk * gd[2]);
        if (prev == 1u && cur == 2u) { front = true; break; }
        if (prev == 2u && cur == 1u) break;                   // a back face: the pixel is empty
        prev = cur;
        Zp = Zk;
    }
    if (front) {
        const float Zc = r.z_min + (float)k * r.step;
        float Fp, Fc;
        const bool okp = ray_trilinear(v, voxels, r.min_weight, go[0] + Zp * gd[0], go[1] + Zp * gd[1], go[2] + Zp * gd[2], Fp);
        const bool okc = ray_trilinear(v, voxels, r.min_weight, go[0] + Zc * gd[0], go[1] + Zc * gd[1], go[2] + Zc * gd[2], Fc);
        if (okp && okc) {
            const float den = Fp - Fc;
            if (den > 0.0f) {
                const float s = fminf(fmaxf(Fp / den, 0.0f), 1.0f);
                Z = Zp + s * r.step;
                if constexpr (COLOR) color = ray_color(v, colors, go[0] + Z * gd[0], go[1] + Z * gd[1], go[2] + Z * gd[2]);
                if constexpr (NORMALS) {
                    const float g[3] = {go[0] + Z * gd[0], go[1] + Z * gd[1], go[2] + Z * gd[2]};
                    float nw[3];
                    bool ok = true;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        float up, dn;
                        ok = ray_trilinear(v, voxels, r.min_weight, ax == 0 ? g[0] + 1.0f : g[0], ax == 1 ? g[1] + 1.0f : g[1],
                                           ax == 2 ? g[2] + 1.0f : g[2], up) && ok;
                        ok = ray_trilinear(v, voxels, r.min_weight, ax == 0 ? g[0] - 1.0f : g[0], ax == 1 ? g[1] - 1.0f : g[1],
                                           ax == 2 ? g[2] - 1.0f : g[2], dn) && ok;
                        nw[ax] = up - dn;
                    }
                    if (ok) {
                        float n[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) n[q] = (P[3 * q] * nw[0] + P[3 * q + 1] * nw[1]) + P[3 * q + 2] * nw[2];
                        const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                        if (cloud_finite(len) && len > 0.0f) {
#pragma unroll
                            for (int q = 0; q < 3; ++q) nrm[q] = n[q] / len;
                        }
                    }
                }
            }
        }
    }
    const size_t at = ((size_t)blockIdx.z * r.H + y) * r.W + x;
    depth[at] = Z;
    if constexpr (NORMALS) {
        normal[3 * at] = nrm[0];
        normal[3 * at + 1] = nrm[1];
        normal[3 * at + 2] = nrm[2];
    }
    if constexpr (COLOR) rgba[at] = color;
}

// ---- the colours of a surface list or of a mesh's vertices ----------------------------------------------------------------------
// One lane per record; only the id, the record's last word, is read.  shift: 3 for ids n*8 + e (sgm_mesh_vertex, kinds 0..6), 2 for
// n*4 + a (sgm_surface_point, axes 0..2).  count (may be NULL) is the list's length as the call before left it on the device, so the
// launch can follow the list's on the stream; records at or beyond it are not written.
__global__ __launch_bounds__(VOL_THREADS) void sgm_volume_colors_k(VolumeParams v, const unsigned* __restrict__ voxels,
                                                                   const unsigned* __restrict__ colors, const uint4* __restrict__ records,
                                                                   size_t capacity, const unsigned* __restrict__ count, unsigned shift,
                                                                   unsigned* __restrict__ rgba)
{
    const size_t r = (size_t)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (r >= capacity || (count && r >= count[0])) return;
    const unsigned id = records[r].w, n = id >> shift, e = id & ((1u << shift) - 1u);
    unsigned out = 0;
    if (n < v.n && e < (shift == 3u ? 7u : 3u)) {
        unsigned i, j, k;
        volume_ijk(v, n, i, j, k);
        const unsigned c = MESH_CORNER_OF(e);
        if (i + (c & 1u) < v.nx && j + ((c >> 1) & 1u) < v.ny && k + (c >> 2) < v.nz) {
            const unsigned m = n + (c & 1u) + ((c >> 1) & 1u) * v.nx + (c >> 2) * (v.nx * v.ny);
            const unsigned cn = colors[n], cm = colors[m];
            if ((cn >> 24) != 0u && (cm >> 24) != 0u) {
                const float tn = (float)(int)(short)(voxels[n] & 0xFFFFu), tm = (float)(int)(short)(voxels[m] & 0xFFFFu);
                const float den = tn - tm;
                const float s = den != 0.0f ? fminf(fmaxf(tn / den, 0.0f), 1.0f) : 0.0f;
                out = color_pack<false>([&](int sh) { return ray_lerp((float)((cn >> sh) & 0xFFu), (float)((cm >> sh) & 0xFFu), s); });
            } else if ((cn >> 24) != 0u) {
                out = 0xFF000000u | cn;
            } else if ((cm >> 24) != 0u) {
                out = 0xFF000000u | cm;
            }
        }
    }
    rgba[r] = out;
}

extern "C" {

// (whole tiles of TILE_MAX voxels: sgmd_volume_points takes a smaller tile only where there is one tile)
size_t sgmd_volume_scratch_bytes(int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    const size_t n = (size_t)nx * ny * nz;
    return tile_scratch_bytes((n + TILE_MAX - 1) / TILE_MAX);
}

// the integration, plain (image, colors NULL) or coloured
static int volume_integrate(const char* entry, int ord, void* stream, const sgmd_volume* v, const sgmd_cloud* c, const float* poses,
                            const void* disp, const void* mask, const void* conf, void* voxels, const void* image, int channels,
                            void* colors)
{
    const bool color = colors != nullptr;
    if (!volume_ok(v) || !cloud_shape_ok(c) || !poses || !disp || !voxels || c->B > SGMD_MAX_POSES || (uintptr_t)voxels % 4 != 0 ||
        (uintptr_t)disp % 4 != 0 || (uintptr_t)conf % 2 != 0 ||
        (color && (!image || (channels != 1 && channels != 4) || (uintptr_t)colors % 4 != 0 || (channels == 4 && (uintptr_t)image % 4 != 0)))) {
        fprintf(stderr, "sgm_mi355x: %s: bad arguments\n", entry);
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const VolumeParams p = volume_params(v);
    const CloudParams q = cloud_params(c);
    VolumeSource s;
    s.wf = (float)c->W; s.hf = (float)c->H;
    s.frames = (unsigned)c->B;
    const PoseBlock pose = pose_block(poses, c->B);
    const hipStream_t st = (hipStream_t)stream;
    VolumeImage im;
    im.pixels = image; im.channels = (unsigned)channels;
    // four voxels per lane where a row is a whole number of them and every array of words can be accessed 16 bytes at a time
    const bool four = p.nx % 4 == 0 && (uintptr_t)voxels % 16 == 0 && (uintptr_t)colors % 16 == 0;
    const dim3 grid(((four ? p.n / 4 : p.n) + VOL_THREADS - 1) / VOL_THREADS);
#define VOL_LAUNCH(V, COLOR)                                                                                                             \
    hipLaunchKernelGGL((sgm_volume_integrate_k<V, COLOR>), grid, dim3(VOL_THREADS), 0, st, p, q, s, pose, (const float*)disp,            \
                       (const uint8_t*)mask, (const uint16_t*)conf, (unsigned*)voxels, im, (unsigned*)colors)
    if (color) {
        if (four) VOL_LAUNCH(4, true); else VOL_LAUNCH(1, true);
    } else {
        if (four) VOL_LAUNCH(4, false); else VOL_LAUNCH(1, false);
    }
#undef VOL_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_volume_integrate(int ord, void* stream, const sgmd_volume* v, const sgmd_cloud* c, const float* poses, const void* disp,
                          const void* mask, const void* conf, void* voxels)
{
    return volume_integrate("sgmd_volume_integrate", ord, stream, v, c, poses, disp, mask, conf, voxels, nullptr, 0, nullptr);
}

int sgmd_volume_integrate_color(int ord, void* stream, const sgmd_volume* v, const sgmd_cloud* c, const float* poses, const void* disp,
                                const void* mask, const void* conf, const void* image, int channels, void* voxels, void* colors)
{
    if (!colors) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_integrate_color: bad arguments\n");
        return -1;
    }
    return volume_integrate("sgmd_volume_integrate_color", ord, stream, v, c, poses, disp, mask, conf, voxels, image, channels, colors);
}

int sgmd_volume_points(int ord, void* stream, const sgmd_volume* v, const void* voxels, unsigned min_weight, void* scratch, void* points,
                       size_t capacity, void* count)
{
    if (!volume_ok(v) || !voxels || !scratch || !count || (!points && capacity) || min_weight < 1 || min_weight > 65535 ||
        (uintptr_t)voxels % 4 != 0 || (uintptr_t)points % 16 != 0 || (uintptr_t)count % 4 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_points: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const VolumeParams p = volume_params(v);
    const unsigned tile = tile_size(p.n), ntiles = (p.n + tile - 1) / tile;
    const TileScratch s = tile_scratch(scratch, ntiles);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sgm_volume_count_k, dim3(ntiles), dim3(TILE_THREADS), 0, st, p, tile, min_weight, (const unsigned*)voxels, s.kept);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sgm_volume_scan_k, dim3(1), dim3(SCAN_THREADS), 0, st, (const unsigned*)s.kept, ntiles, s.base, (unsigned*)count);
    HIP_TRY(hipGetLastError());
    if (capacity == 0) return 0;                              // the count is all that was asked for
    hipLaunchKernelGGL(sgm_volume_emit_k, dim3(ntiles), dim3(TILE_THREADS), 0, st, p, tile, min_weight, (const unsigned*)voxels,
                       (const unsigned*)s.base, (SurfacePoint*)points, capacity);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the ray-cast, plain (colors, rgba NULL) or coloured
static int volume_raycast(const char* entry, int ord, void* stream, const sgmd_volume* v, const sgmd_raycast* r, const float* poses,
                          const void* voxels, void* depth, void* normal, const void* colors, void* rgba)
{
    if (!volume_ok(v) || !r || !poses || !voxels || !depth || r->W < 1 || r->H < 1 || r->W > 65535 || r->H > 65535 || r->B < 1 ||
        r->B > SGMD_MAX_POSES || (unsigned long long)r->W * r->H * r->B > (1ull << 31) || r->min_weight < 1 || r->min_weight > 65535 ||
        (uintptr_t)voxels % 4 != 0 || (uintptr_t)depth % 4 != 0 || (uintptr_t)normal % 4 != 0 || (colors == nullptr) != (rgba == nullptr) ||
        (uintptr_t)colors % 4 != 0 || (uintptr_t)rgba % 4 != 0) {
        fprintf(stderr, "sgm_mi355x: %s: bad arguments\n", entry);
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const VolumeParams p = volume_params(v);
    RaycastView q;
    q.W = (unsigned)r->W; q.H = (unsigned)r->H;
    q.fx = r->fx; q.fy = r->fy; q.cx = r->cx; q.cy = r->cy; q.z_min = r->z_min; q.z_max = r->z_max; q.step = r->step;
    q.min_weight = r->min_weight;
    const PoseBlock pose = pose_block(poses, r->B);
    const dim3 grid((q.W + RAY_BLOCK_W - 1) / RAY_BLOCK_W, (q.H + RAY_BLOCK_H - 1) / RAY_BLOCK_H, (unsigned)r->B);
    const hipStream_t st = (hipStream_t)stream;
#define RAY_LAUNCH(NORMALS, COLOR)                                                                                                       \
    hipLaunchKernelGGL((sgm_volume_raycast_k<NORMALS, COLOR>), grid, dim3(RAY_THREADS), 0, st, p, q, pose, (const unsigned*)voxels,      \
                       (float*)depth, (float*)normal, (const unsigned*)colors, (unsigned*)rgba)
    if (rgba) {
        if (normal) RAY_LAUNCH(true, true); else RAY_LAUNCH(false, true);
    } else {
        if (normal) RAY_LAUNCH(true, false); else RAY_LAUNCH(false, false);
    }
#undef RAY_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_volume_raycast(int ord, void* stream, const sgmd_volume* v, const sgmd_raycast* r, const float* poses, const void* voxels,
                        void* depth, void* normal)
{
    return volume_raycast("sgmd_volume_raycast", ord, stream, v, r, poses, voxels, depth, normal, nullptr, nullptr);
}

int sgmd_volume_raycast_color(int ord, void* stream, const sgmd_volume* v, const sgmd_raycast* r, const float* poses, const void* voxels,
                              const void* colors, void* depth, void* normal, void* rgba)
{
    if (!colors || !rgba) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_raycast_color: bad arguments\n");
        return -1;
    }
    return volume_raycast("sgmd_volume_raycast_color", ord, stream, v, r, poses, voxels, depth, normal, colors, rgba);
}

int sgmd_volume_colors(int ord, void* stream, const sgmd_volume* v, const void* voxels, const void* colors, const void* records,
                       size_t capacity, const void* count, int id_kinds, void* rgba)
{
    if (!volume_ok(v) || !voxels || !colors || (capacity && (!records || !rgba)) || (id_kinds != 4 && id_kinds != 8) ||
        (id_kinds == 8 && (unsigned long long)v->nx * v->ny * v->nz > (1ull << 27)) || capacity > ((size_t)1 << 32) ||
        (uintptr_t)voxels % 4 != 0 || (uintptr_t)colors % 4 != 0 || (uintptr_t)records % 16 != 0 || (uintptr_t)count % 4 != 0 ||
        (uintptr_t)rgba % 4 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_volume_colors: bad arguments\n");
        return -1;
    }
    if (capacity == 0) return 0;
    HIP_TRY(hipSetDevice(ord));
    const VolumeParams p = volume_params(v);
    hipLaunchKernelGGL(sgm_volume_colors_k, dim3((unsigned)((capacity + VOL_THREADS - 1) / VOL_THREADS)), dim3(VOL_THREADS), 0,
                       (hipStream_t)stream, p, (const unsigned*)voxels, (const unsigned*)colors, (const uint4*)records, capacity,
                       (const unsigned*)count, id_kinds == 8 ? 3u : 2u, (unsigned*)rgba);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
