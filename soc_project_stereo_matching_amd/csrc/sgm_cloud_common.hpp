#pragma once
// What sgm_cloud.hip, sgm_register.hip, sgm_volume.hip and sgm_track.hip share.  The source map: the predicate, the formulas and
// the load paths of the point clouds (include/sgm_mi355x.h, sgm_cloud_spec) and, for the launchers, the one reading of a
// sgmd_cloud.  A point into another camera: the rigid move, the pinhole to the nearest admitted pixel and the block of poses a
// launch takes.  The ordered
// compaction of the point list and the surface list: its device pieces, its tile size and its scratch.  Include after sgm_common.hpp.

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

// ---- a point into another camera: the rigid move, the pinhole, the nearest pixel.  The parentheses are the contracts'. --------------

// the poses of a launch's frames, R row-major then t each: 3 KiB of the 4 KiB a kernel's arguments may take, read with scalar loads
struct PoseBlock { float p[SGMD_MAX_POSES][12]; };
static_assert(sizeof(PoseBlock) == 3072, "the poses travel as kernel arguments");

static __device__ __forceinline__ void pose_move(const float* R, const float* t, float x, float y, float z, float& X, float& Y, float& Z)
{
    X = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
    Y = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
    Z = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
}

// (X, Y, Z) in front of a pinhole -> the nearest pixel (uf, vf) of a wf x hf image; false where it has none
static __device__ __forceinline__ bool pinhole_pixel(float fx, float fy, float cx, float cy, float wf, float hf, float X, float Y, float Z,
                                                     float& uf, float& vf)
{
    if (!cloud_finite(Z)) return false;
    if (!(Z > 0.0f)) return false;
    const float u = fx * (X / Z) + cx, v = fy * (Y / Z) + cy;
    if (!cloud_finite(u) || !cloud_finite(v)) return false;
    uf = floorf(u + 0.5f);
    vf = floorf(v + 0.5f);
    // admitted in float, before any conversion to int
    return 0.0f <= uf && uf < wf && 0.0f <= vf && vf < hf;
}

// ---- the ordered compaction: count per tile, scan, emit ---------------------------------------------------------------------------
// A tile is a power-of-two run of at most TILE_MAX items, one workgroup of TILE_THREADS per tile in `count` and `emit`, which pass
// over it TILE_THREADS lanes at a time.  A lane contributes a few flags per pass (the cloud: its V pixels, the volume: three axes).

#define TILE_THREADS 256
#define TILE_WAVES (TILE_THREADS / 64)
#define TILE_MAX 2048

// The wave rank, one flag at a time: adds the kept flags of the lower lanes to `lower` and those of the whole wave to `wave_total`.
// The rank of a lane's flag k is `lower` after all of its flags plus the kept ones among its first k (raster order is lane-major).
static __device__ __forceinline__ void wave_rank(bool keep, unsigned& lower, unsigned& wave_total)
{
    const unsigned long long b = __ballot(keep);
    lower += __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    wave_total += (unsigned)__popcll(b);
}

// The end of `count`: the sum of the waves' totals (each the same in all lanes of its wave) -> *kept, by thread 0.
static __device__ __forceinline__ void tile_total(unsigned wave_total, unsigned* __restrict__ kept)
{
    __shared__ unsigned s_wave[TILE_WAVES];
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < TILE_WAVES; ++w) sum += s_wave[w];
        *kept = sum;
    }
}

// The hand-over of one pass of `emit` (turn: 0, 1, 0, .. over the passes): returns what the lower waves kept in this pass, `all`
// what the workgroup kept.  One barrier per pass.
static __device__ __forceinline__ unsigned pass_before(unsigned wave_total, unsigned turn, unsigned& all)
{
    __shared__ unsigned s_wave[2][TILE_WAVES];
    const unsigned wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) s_wave[turn][wave] = wave_total;
    __syncthreads();                                          // (the other half of s_wave is what the previous pass still reads)
    unsigned before = 0;
    all = 0;
#pragma unroll
    for (unsigned w = 0; w < TILE_WAVES; ++w) {
        const unsigned s = s_wave[turn][w];
        before += w < wave ? s : 0u;
        all += s;
    }
    return before;
}

// The scan of the three launches (count per tile, scan, emit), for ONE workgroup of SCAN_THREADS:
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

// ---- the launchers' side ---------------------------------------------------------------------------------------------------------
// the shapes the kernels take: frame-relative pixel indices and (y << 16) | x fit 32 bits, a launch covers the batch
static bool cloud_shape_ok(const sgmd_cloud* c)
{
    return c && c->W >= 1 && c->H >= 1 && c->W <= 65535 && c->H <= 65535 && c->B >= 1 &&
           (unsigned long long)c->W * c->H * c->B <= (1ull << 31);
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

// four pixels per lane: every frame starts at a multiple of four pixels and the three maps can be read 16 / 4 / 8 bytes at a time
static bool cloud_vector(const sgmd_cloud* c, const void* disp, const void* mask, const void* conf)
{
    return ((size_t)c->W * c->H) % 4 == 0 && (uintptr_t)disp % 16 == 0 && (uintptr_t)mask % 4 == 0 && (uintptr_t)conf % 8 == 0;
}

// the poses of `frames` frames ([frames][12], frames <= SGMD_MAX_POSES) as the kernel argument, the rest zero
static PoseBlock pose_block(const float* poses, int frames)
{
    PoseBlock b;
    memset(&b, 0, sizeof b);
    memcpy(b.p, poses, (size_t)frames * 12 * sizeof(float));
    return b;
}

// the tile of a compaction over runs of n items: a power of two, at most TILE_MAX, at least 1
static unsigned tile_size(size_t n)
{
    unsigned tile = 1;
    while (tile < TILE_MAX && tile < n) tile <<= 1;
    return tile;
}

// the scratch of a compaction over ntiles tiles: kept[ntiles], then base[ntiles]
struct TileScratch { unsigned* kept; unsigned* base; };
static size_t tile_scratch_bytes(size_t ntiles) { return 2 * sizeof(unsigned) * ntiles; }
static TileScratch tile_scratch(void* scratch, size_t ntiles) { return {(unsigned*)scratch, (unsigned*)scratch + ntiles}; }
