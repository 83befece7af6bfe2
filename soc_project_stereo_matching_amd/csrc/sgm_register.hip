#include "sgm_common.hpp"
#include "sgm_cloud_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): depth registered to another camera -- a forward warp with a z-buffer.  The
// contract is written out in include/sgm_mi355x.h (sgm_register_spec); tests/register_ref.py restates it in numpy.
//
// The kept pixels of the cloud contract (cloud_kept, cloud_xy: the same X Y Z sgm_cloud_organized writes) are moved into the
// target camera, projected through its pinhole and distortion and splatted onto one or four target pixels.  Many source pixels
// can land on one target pixel and the nearest must win: per target pixel a 64-bit key (bits(Z') << 32) | source pixel, and the
// smallest key wins.  Z' > 0 makes its bit pattern monotonic, the source pixel breaks ties, and a minimum does not depend on the
// order of arrival: the result is the same on every run.
//
// Three launches, ordered by the stream and by nothing else:
//   clear     the keys of the batch's target pixels to all ones, 16-byte stores
//   scatter   the cloud's load paths (four source pixels per lane from one 16-byte load where the pixel count and the pointers
//             allow it, else one per lane), the projection, one no-return 64-bit minimum per admitted candidate.  Agent scope:
//             the eight XCDs do not share an L2.  It is one global_atomic_umin_x2, no compare-and-swap loop.
//   resolve   element-wise over the target, two keys per lane from one 16-byte load -> depth and, when asked, source
// sgm_register_gather is a fourth, independent element-wise kernel: any map of the source follows the depth through `source`.
//
// (this translation unit is compiled with -fno-honor-nans like the others: "finite" is tested on the bit pattern, before any
// comparison, and NaN is made from bits)
// ============================================================================================

#define REG_THREADS 256
#define REG_QNAN 0x7FC00000u
#define REG_NONE 0xFFFFFFFFu
// The pre-check: read the key first (agent scope, relaxed) and skip the atomic when it is already <= this candidate's.  Keys only
// fall, so a stale read costs one redundant atomic and never a wrong result.  At splat 2 only (NOTES.md section 29): at splat 1 a key
// sees about one candidate and the load is wasted, at splat 2 it sees about four and the later ones are often beaten already.

typedef unsigned long long reg_key;

struct RegisterParams {
    float fx, fy, cx, cy, k1, k2, p1, p2, k3;
    float R[9], t[3];
    float z_min, z_max;
    float wf, hf;              // (float)width, (float)height of the target
    unsigned W;                // target width
    unsigned tpx;              // target pixels of one frame
    int splat;
};

template <bool PRECHECK>
static __device__ __forceinline__ void register_vote(reg_key* __restrict__ keys, const RegisterParams& r, float uf, float vf, reg_key k)
{
    // admitted in float, before any conversion to int (pinhole_pixel's test, written out here: behind a shared helper the four
    // votes of splat 2 compiled to another control flow, 6 % slower -- NOTES.md section 36)
    if (!(0.0f <= uf && uf < r.wf && 0.0f <= vf && vf < r.hf)) return;
    reg_key* at = keys + (size_t)(unsigned)vf * r.W + (unsigned)uf;
    if constexpr (PRECHECK) {
        if (__hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= k) return;
    }
    (void)__hip_atomic_fetch_min(at, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one kept source pixel (x, y) with its point (X, Y, Z) -> its candidates' votes in the keys of its frame.  The parentheses are
// the contract's.
static __device__ __forceinline__ void register_point(reg_key* __restrict__ keys, const RegisterParams& r, unsigned x, unsigned y,
                                                      float X, float Y, float Z)
{
    float Xp, Yp, Zp;
    pose_move(r.R, r.t, X, Y, Z, Xp, Yp, Zp);
    if (!cloud_finite(Zp)) return;
    if (!(Zp > 0.0f && r.z_min <= Zp && Zp <= r.z_max)) return;
    const float a = Xp / Zp, b = Yp / Zp;
    const float aa = a * a, bb = b * b, ab = a * b;
    const float r2 = aa + bb;
    const float rad = ((r.k3 * r2 + r.k2) * r2 + r.k1) * r2 + 1.0f;
    const float xd = (a * rad + (2.0f * r.p1) * ab) + r.p2 * (r2 + 2.0f * aa);
    const float yd = (b * rad + r.p1 * (r2 + 2.0f * bb)) + (2.0f * r.p2) * ab;
    const float u = r.fx * xd + r.cx, v = r.fy * yd + r.cy;
    if (!cloud_finite(u) || !cloud_finite(v)) return;
    const reg_key k = ((reg_key)__float_as_uint(Zp) << 32) | (reg_key)((y << 16) | x);
    if (r.splat == 1) {
        register_vote<false>(keys, r, floorf(u + 0.5f), floorf(v + 0.5f), k);
    } else {
        const float u0 = floorf(u), v0 = floorf(v);
        const float u1 = u0 + 1.0f, v1 = v0 + 1.0f;
        register_vote<true>(keys, r, u0, v0, k);
        register_vote<true>(keys, r, u1, v0, k);
        register_vote<true>(keys, r, u0, v1, k);
        register_vote<true>(keys, r, u1, v1, k);
    }
}

// ---- clear: n2 pairs of keys ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(REG_THREADS) void sgm_register_clear_k(uint4* __restrict__ keys2, size_t n2)
{
    const size_t g = (size_t)blockIdx.x * REG_THREADS + threadIdx.x;
    if (g < n2) keys2[g] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// ---- scatter: n source pixels of the batch -------------------------------------------------------------------------------------

template <int V>
__global__ __launch_bounds__(REG_THREADS) void sgm_register_scatter_k(CloudParams c, RegisterParams r, size_t n,
                                                                      const float* __restrict__ disp, const uint8_t* __restrict__ mask,
                                                                      const uint16_t* __restrict__ conf, reg_key* __restrict__ keys)
{
    const size_t g = ((size_t)blockIdx.x * REG_THREADS + threadIdx.x) * V;       // V == 4: npx % 4 == 0, the four share a frame
    if (g >= n) return;
    float d[V];
    unsigned m[V], k[V];
    cloud_load<V>(disp, mask, conf, g, true, d, m, k);
    const size_t frame = g / c.npx;
    const unsigned p = (unsigned)(g - frame * c.npx);
    unsigned y = p / c.W, x = p - y * c.W;
    reg_key* frame_keys = keys + frame * (size_t)r.tpx;                        // frame f of the source writes frame f of the target
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float X, Y, Z;
        if (cloud_kept(c, d[i], m[i], k[i], Z)) {
            cloud_xy(c, x, y, Z, X, Y);
            register_point(frame_keys, r, x, y, X, Y, Z);
        }
        if (++x == c.W) { x = 0; ++y; }
    }
}

// ---- resolve: nk keys of the batch (the scratch holds an even number of them) ---------------------------------------------------

__global__ __launch_bounds__(REG_THREADS) void sgm_register_resolve_k(const uint4* __restrict__ keys2, size_t nk,
                                                                      unsigned* __restrict__ depth, unsigned* __restrict__ source)
{
    const size_t g = ((size_t)blockIdx.x * REG_THREADS + threadIdx.x) * 2;
    if (g >= nk) return;
    const uint4 t = keys2[g / 2];                             // little endian: .x / .z the source pixel, .y / .w the bits of Z'
    const bool hit0 = t.y != ~0u, hit1 = t.w != ~0u;          // (no candidate's high word is all ones: Z' is finite)
    depth[g] = hit0 ? t.y : REG_QNAN;
    if (source) source[g] = hit0 ? t.x : REG_NONE;
    if (g + 1 < nk) {
        depth[g + 1] = hit1 ? t.w : REG_QNAN;
        if (source) source[g + 1] = hit1 ? t.z : REG_NONE;
    }
}

// ---- gather: n target pixels of the batch --------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(REG_THREADS) void sgm_register_gather_k(size_t n, unsigned tpx, unsigned W, unsigned H, unsigned npx,
                                                                     const unsigned* __restrict__ source, const T* __restrict__ map,
                                                                     T fill, T* __restrict__ out)
{
    const size_t g = (size_t)blockIdx.x * REG_THREADS + threadIdx.x;
    if (g >= n) return;
    const unsigned s = source[g];
    const unsigned y = s >> 16, x = s & 0xFFFFu;
    const size_t frame = g / tpx;
    // (a word that names no pixel of the source -- 0xFFFFFFFF, or anything a caller's buffer may hold -- reads nothing)
    out[g] = (s != REG_NONE && y < H && x < W) ? map[frame * npx + (size_t)y * W + x] : fill;
}

// the source's shape (cloud_shape_ok) and the target's own: its size, the batch's pixels in it, its splat
static bool register_shapes_ok(const sgmd_cloud* c, const sgmd_register* r)
{
    return cloud_shape_ok(c) && r && r->W >= 1 && r->H >= 1 && r->W <= 65535 && r->H <= 65535 &&
           (unsigned long long)r->W * r->H * c->B <= (1ull << 31) && (r->splat == 1 || r->splat == 2);
}

static unsigned register_blocks(size_t items) { return (unsigned)((items + REG_THREADS - 1) / REG_THREADS); }

extern "C" {

size_t sgmd_register_scratch_bytes(int W, int H, int B)
{
    if (W < 1 || H < 1 || B < 1) return 0;
    const size_t nk = (size_t)W * H * B;
    return 16 * ((nk + 1) / 2);                               // one 8-byte key per target pixel, in 16-byte pairs
}

int sgmd_register_depth(int ord, void* stream, const sgmd_cloud* c, const sgmd_register* r, const void* disp, const void* mask,
                        const void* conf, void* keys, void* depth, void* source)
{
    if (!register_shapes_ok(c, r) || !disp || !keys || !depth || (uintptr_t)keys % 16 != 0 || (uintptr_t)depth % 4 != 0 ||
        (uintptr_t)source % 4 != 0 || (uintptr_t)disp % 4 != 0 || (uintptr_t)conf % 2 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_register_depth: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)c->W * c->H * c->B, nk = (size_t)r->W * r->H * c->B, n2 = (nk + 1) / 2;
    const CloudParams p = cloud_params(c);
    RegisterParams q;
    q.fx = r->fx; q.fy = r->fy; q.cx = r->cx; q.cy = r->cy;
    q.k1 = r->dist[0]; q.k2 = r->dist[1]; q.p1 = r->dist[2]; q.p2 = r->dist[3]; q.k3 = r->dist[4];
    for (int i = 0; i < 9; ++i) q.R[i] = r->R[i];
    for (int i = 0; i < 3; ++i) q.t[i] = r->t[i];
    q.z_min = r->z_min; q.z_max = r->z_max;
    q.wf = (float)r->W; q.hf = (float)r->H;
    q.W = (unsigned)r->W;
    q.tpx = (unsigned)((size_t)r->W * r->H);
    q.splat = r->splat;
    hipLaunchKernelGGL(sgm_register_clear_k, dim3(register_blocks(n2)), dim3(REG_THREADS), 0, st, (uint4*)keys, n2);
    HIP_TRY(hipGetLastError());
    if (cloud_vector(c, disp, mask, conf))
        hipLaunchKernelGGL(sgm_register_scatter_k<4>, dim3(register_blocks(n / 4)), dim3(REG_THREADS), 0, st, p, q, n, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, (reg_key*)keys);
    else
        hipLaunchKernelGGL(sgm_register_scatter_k<1>, dim3(register_blocks(n)), dim3(REG_THREADS), 0, st, p, q, n, (const float*)disp,
                           (const uint8_t*)mask, (const uint16_t*)conf, (reg_key*)keys);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sgm_register_resolve_k, dim3(register_blocks(n2)), dim3(REG_THREADS), 0, st, (const uint4*)keys, nk, (unsigned*)depth,
                       (unsigned*)source);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_register_gather(int ord, void* stream, const sgmd_cloud* c, const sgmd_register* r, const void* source, int elem_bytes,
                         const void* map, unsigned fill, void* out)
{
    if (!register_shapes_ok(c, r) || !source || !map || !out || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) ||
        (uintptr_t)source % 4 != 0 || (uintptr_t)map % (unsigned)elem_bytes != 0 || (uintptr_t)out % (unsigned)elem_bytes != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_register_gather: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)r->W * r->H * c->B;
    const unsigned tpx = (unsigned)((size_t)r->W * r->H), W = (unsigned)c->W, H = (unsigned)c->H, npx = (unsigned)((size_t)c->W * c->H);
    const dim3 grid(register_blocks(n)), block(REG_THREADS);
    if (elem_bytes == 1)
        hipLaunchKernelGGL(sgm_register_gather_k<uint8_t>, grid, block, 0, st, n, tpx, W, H, npx, (const unsigned*)source, (const uint8_t*)map,
                           (uint8_t)fill, (uint8_t*)out);
    else if (elem_bytes == 2)
        hipLaunchKernelGGL(sgm_register_gather_k<uint16_t>, grid, block, 0, st, n, tpx, W, H, npx, (const unsigned*)source,
                           (const uint16_t*)map, (uint16_t)fill, (uint16_t*)out);
    else
        hipLaunchKernelGGL(sgm_register_gather_k<uint32_t>, grid, block, 0, st, n, tpx, W, H, npx, (const unsigned*)source,
                           (const uint32_t*)map, (uint32_t)fill, (uint32_t*)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
