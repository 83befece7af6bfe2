#include "sgm_common.hpp"
#include "sgm_cloud_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): the sums of frame-to-model tracking, projective point-to-plane ICP of the current
// frame's depth against the depth and normal maps sgm_volume_raycast rendered.  The contract is written out in
// include/sgm_mi355x.h (sgm_track_spec); tests/track_ref.py restates it in numpy.
//
// One launch for all frames (blockIdx.y: the frame, whose pose is read from the kernel arguments with scalar loads).  Lanes stride
// over the source pixels -- four consecutive pixels per lane with 16-byte map loads where cloud_vector allows it, else one -- and
// decide with the cloud's predicate (cloud_kept) which contribute.  A contributing pixel is moved by the pose, projected into the
// model view, associated with the model pixel it lands on and gated; its seven quantised numbers q_0..q_6 (the six entries of the
// Jacobian row and the residual) add 28 products and a count to the lane's 29 int64 accumulators, which stay in registers.  A wave
// adds its lanes' accumulators with shuffles, a workgroup its waves' through LDS, and 29 lanes add the workgroup's sums to
// sums[frame][0..28] with 64-bit integer atomics.  The sums are exact integers (|q| <= 2^19, at most 2^24 pixels: below 2^62), so
// the order of addition does not show: the result is the same bytes on every run, and one call over B frames is B calls of one.
// sums is zeroed on the stream ahead of the launch.
//
// (this translation unit is compiled with -fno-honor-nans like the others: "finite" is tested on the bit pattern, before any
// comparison)
// ============================================================================================

#define TRACK_THREADS 256
#define TRACK_WAVES (TRACK_THREADS / 64)
#define TRACK_MAX_BLOCKS 128                                  // per frame: 29 atomics each, the lanes stride beyond
#define TRACK_SUMS 29

struct TrackModel {
    unsigned W, H;
    float wf, hf, fx, fy, cx, cy, gate, dist_max, span;       // gate: dist_max * dist_max rounded once
};

// One kept source pixel with its cloud X, Y, Z.  The parentheses are the contract's.
static __device__ __forceinline__ void track_pixel(const TrackModel& m, const float* P, const float* __restrict__ depth,
                                                   const float* __restrict__ normal, float X, float Y, float Z,
                                                   long long (&acc)[TRACK_SUMS])
{
    float Px, Py, Pz, uf, vf;
    pose_move(P, P + 9, X, Y, Z, Px, Py, Pz);
    if (!pinhole_pixel(m.fx, m.fy, m.cx, m.cy, m.wf, m.hf, Px, Py, Pz, uf, vf)) return;
    const size_t at = (size_t)(unsigned)vf * m.W + (unsigned)uf;
    const float Zm = depth[at];
    if (!cloud_finite(Zm)) return;
    if (!(Zm > 0.0f)) return;
    const float n0 = normal[3 * at], n1 = normal[3 * at + 1], n2 = normal[3 * at + 2];
    if (!cloud_finite(n0) || !cloud_finite(n1) || !cloud_finite(n2)) return;
    const float e0 = ((uf - m.cx) * Zm) / m.fx - Px, e1 = ((vf - m.cy) * Zm) / m.fy - Py, e2 = Zm - Pz;
    const float d2 = (e0 * e0 + e1 * e1) + e2 * e2;
    if (!cloud_finite(d2)) return;
    if (!(d2 <= m.gate)) return;
    const float r = (n0 * e0 + n1 * e1) + n2 * e2;
    const float c0 = Py * n2 - Pz * n1, c1 = Pz * n0 - Px * n2, c2 = Px * n1 - Py * n0;
    const float val[7] = {c0 / m.span, c1 / m.span, c2 / m.span, n0, n1, n2, r / m.dist_max};
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i) ok = ok && cloud_finite(val[i]) && fabsf(val[i]) <= 8.0f;
    if (!ok) return;
    int q[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) q[i] = (int)rintf(val[i] * 65536.0f);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = i; j < 7; ++j) acc[k++] += (long long)q[i] * (long long)q[j];
    }
    acc[28] += 1;
}

template <int V>
__global__ __launch_bounds__(TRACK_THREADS) void sgm_track_sums_k(CloudParams c, TrackModel m, PoseBlock poses,
                                                                  const float* __restrict__ disp, const uint8_t* __restrict__ mask,
                                                                  const uint16_t* __restrict__ conf, const float* __restrict__ depth,
                                                                  const float* __restrict__ normal, long long* __restrict__ sums)
{
    __shared__ long long s_wave[TRACK_WAVES][TRACK_SUMS];
    const unsigned f = blockIdx.y;
    const float* P = poses.p[f];                              // R row-major, then t: source camera -> model camera
    const size_t frame_base = (size_t)f * c.npx, model_base = (size_t)f * m.W * m.H;
    const float* fdepth = depth + model_base;
    const float* fnormal = normal + 3 * model_base;
    long long acc[TRACK_SUMS];
#pragma unroll
    for (int k = 0; k < TRACK_SUMS; ++k) acc[k] = 0;
    const unsigned stride = gridDim.x * TRACK_THREADS * V;
    // (V == 4: npx % 4 == 0, so a lane's four pixels are all inside the frame or all outside)
    for (unsigned p = (blockIdx.x * TRACK_THREADS + threadIdx.x) * V; p < c.npx; p += stride) {
        float d[V];
        unsigned mk[V], cf[V];
        cloud_load<V>(disp, mask, conf, frame_base + p, true, d, mk, cf);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float X, Y, Z;
            if (!cloud_kept(c, d[e], mk[e], cf[e], Z)) continue;
            const unsigned y = (p + e) / c.W, x = (p + e) - y * c.W;
            cloud_xy(c, x, y, Z, X, Y);
            track_pixel(m, P, fdepth, fnormal, X, Y, Z, acc);
        }
    }
    // the wave's lanes, then the workgroup's waves, then the grid's workgroups: integer sums, any order gives the same bytes
#pragma unroll
    for (int k = 0; k < TRACK_SUMS; ++k) {
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) acc[k] += __shfl_xor(acc[k], step);
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < TRACK_SUMS; ++k) s_wave[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < TRACK_SUMS) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < TRACK_WAVES; ++w) sum += s_wave[w][threadIdx.x];
        if (sum != 0) atomicAdd(reinterpret_cast<unsigned long long*>(sums + (size_t)f * TRACK_SUMS + threadIdx.x), (unsigned long long)sum);
    }
}

// the workgroups of a frame: one item per lane up to TRACK_MAX_BLOCKS, the lanes stride beyond
static unsigned track_blocks(size_t items)
{
    const size_t blocks = (items + TRACK_THREADS - 1) / TRACK_THREADS;
    return (unsigned)(blocks > TRACK_MAX_BLOCKS ? TRACK_MAX_BLOCKS : blocks);
}

extern "C" {

int sgmd_track_sums(int ord, void* stream, const sgmd_cloud* c, const sgmd_track* t, const float* poses, const void* disp,
                    const void* mask, const void* conf, const void* model_depth, const void* model_normal, void* sums)
{
    if (!cloud_shape_ok(c) || !t || !poses || !disp || !model_depth || !model_normal || !sums || c->B > SGMD_MAX_POSES ||
        (unsigned long long)c->W * c->H > (1ull << 24) || t->W < 1 || t->H < 1 || t->W > 65535 || t->H > 65535 ||
        (uintptr_t)disp % 4 != 0 || (uintptr_t)conf % 2 != 0 || (uintptr_t)model_depth % 4 != 0 || (uintptr_t)model_normal % 4 != 0 ||
        (uintptr_t)sums % 8 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_track_sums: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const CloudParams q = cloud_params(c);
    TrackModel m;
    m.W = (unsigned)t->W; m.H = (unsigned)t->H;
    m.wf = (float)t->W; m.hf = (float)t->H;
    m.fx = t->fx; m.fy = t->fy; m.cx = t->cx; m.cy = t->cy;
    m.gate = t->dist_max * t->dist_max;
    m.dist_max = t->dist_max; m.span = t->span;
    const PoseBlock pose = pose_block(poses, c->B);
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(sums, 0, (size_t)c->B * TRACK_SUMS * sizeof(long long), st));
    const bool vec = cloud_vector(c, disp, mask, conf);
    const unsigned blocks = track_blocks(((size_t)q.npx + (vec ? 3 : 0)) / (vec ? 4 : 1));
    const dim3 grid(blocks, (unsigned)c->B);
    if (vec)
        hipLaunchKernelGGL(sgm_track_sums_k<4>, grid, dim3(TRACK_THREADS), 0, st, q, m, pose, (const float*)disp, (const uint8_t*)mask,
                           (const uint16_t*)conf, (const float*)model_depth, (const float*)model_normal, (long long*)sums);
    else
        hipLaunchKernelGGL(sgm_track_sums_k<1>, grid, dim3(TRACK_THREADS), 0, st, q, m, pose, (const float*)disp, (const uint8_t*)mask,
                           (const uint16_t*)conf, (const float*)model_depth, (const float*)model_normal, (long long*)sums);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
