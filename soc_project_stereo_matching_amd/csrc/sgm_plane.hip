#include "sgm_common.hpp"
#include "sgm_cloud_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): planes in a point list.  The contract is written out in include/sgm_mi355x.h
// (sgm_plane_spec); tests/plane_ref.py restates it in numpy.  A list is what sgm_cloud_points, sgm_volume_points and sgm_volume_mesh
// write: 16-byte records {float x, y, z; uint32 tag} with an optional device count word.
//
// Four launchers.  sgmd_plane_votes: K candidate planes from three hashed records each (one lane per candidate, a small launch of its
// own that writes them to `planes`), then the vote: every workgroup copies the K candidates into LDS, a lane keeps PLANE_RECORDS
// records in registers (16-byte loads, lane-contiguous), and for every candidate -- read back from LDS at one address by the whole
// wave, a broadcast -- a wave turns each of its PLANE_RECORDS tests into a ballot and a population count on the scalar side.  The
// wave's count of candidate k is kept by lane k % 64 in a register; after 64 candidates every lane adds its own to the workgroup's
// LDS counter of its candidate, and the workgroup adds its K counters to planes[k].votes with 32-bit integer atomics: integer sums,
// so the order of addition never shows.  sgmd_plane_best: one wave, the candidate with the
// most votes.  sgmd_plane_sums: the ten integer moments of a plane's inliers, reduced as in sgm_track.hip (registers, shuffles, LDS,
// 64-bit integer atomics).  sgmd_plane_label: a byte per unlabelled inlier.
//
// "|s| <= dist and s finite" is one signed integer comparison on the bit pattern: for a finite dist > 0, bits(s) & 0x7FFFFFFF <=
// bits(dist) holds exactly for the finite s with |s| <= dist (an infinity or NaN has a larger pattern).  A void plane travels with
// the threshold -1, which nothing passes.
//
// (this translation unit is compiled with -fno-honor-nans like the others: "finite" is tested on the bit pattern, before any
// comparison)
// ============================================================================================

#define PLANE_THREADS 256
#define PLANE_WAVES (PLANE_THREADS / 64)
#define PLANE_RECORDS 8                                       // records a lane holds while the candidates pass (NOTES.md 42)
#define PLANE_MAX_BLOCKS 512                                  // the lanes stride beyond; bounds the atomics of a launch
#define PLANE_MAX_K 1024
#define PLANE_SUMS 10

struct PlaneRule {
    unsigned K, seed;
    int dist_bits;                                            // the bits of dist: finite, > 0
    int prior;
    float ax, ay, az, thr;                                    // thr: min_cos * |axis|, rounded as the header says
    float span;
};

// h of the header: a pure uint32 mix (no modulo, no float)
static __device__ __forceinline__ unsigned plane_hash(unsigned seed, unsigned k, unsigned j)
{
    unsigned x = (seed ^ (k * 0x9E3779B9u)) ^ ((j + 1u) * 0x85EBCA6Bu);
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

static __device__ __forceinline__ unsigned long long plane_count(size_t capacity, const unsigned* __restrict__ count)
{
    const unsigned long long c = count ? (unsigned long long)count[0] : (unsigned long long)capacity;
    return c < (unsigned long long)capacity ? c : (unsigned long long)capacity;
}

static __device__ __forceinline__ bool plane_finite3(float x, float y, float z)
{
    return cloud_finite(x) && cloud_finite(y) && cloud_finite(z);
}

// The vote rule on a finite, unlabelled record.  The parentheses are the contract's.
static __device__ __forceinline__ bool plane_inlier(float x, float y, float z, const float4& nrm, const float4& anchor)
{
    const float s = (nrm.x * (x - anchor.x) + nrm.y * (y - anchor.y)) + nrm.z * (z - anchor.z);
    return (int)(__float_as_uint(s) & 0x7FFFFFFFu) <= __float_as_int(nrm.w);
}

static __device__ __forceinline__ bool plane_is_void(const float4& nrm)
{
    return ((__float_as_uint(nrm.x) | __float_as_uint(nrm.y) | __float_as_uint(nrm.z)) & 0x7FFFFFFFu) == 0u;
}

// a plane as the kernels test against it: {n0, n1, n2, threshold bits}, {a0, a1, a2, -}
static __device__ __forceinline__ void plane_load(const float4* __restrict__ plane, int dist_bits, float4& nrm, float4& anchor)
{
    nrm = plane[0];
    anchor = plane[1];
    nrm.w = __int_as_float(plane_is_void(nrm) ? -1 : dist_bits);
}

__global__ __launch_bounds__(64) void sgm_plane_candidates_k(const float4* __restrict__ records, size_t capacity,
                                                             const unsigned* __restrict__ count, const uint8_t* __restrict__ labels,
                                                             float4* __restrict__ planes, PlaneRule p)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    if (k >= p.K) return;
    const unsigned long long n = plane_count(capacity, count);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 nrm = zero, anchor = zero;
    size_t at[3];
#pragma unroll
    for (unsigned j = 0; j < 3; ++j) at[j] = (size_t)(((unsigned long long)plane_hash(p.seed, k, j) * n) >> 32);
    bool ok = at[0] != at[1] && at[0] != at[2] && at[1] != at[2];     // n < 3 ends here: no record is read
    float4 r[3] = {zero, zero, zero};
    if (ok) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            r[j] = records[at[j]];
            ok = ok && plane_finite3(r[j].x, r[j].y, r[j].z) && (labels == nullptr || labels[at[j]] == 0);
        }
    }
    if (ok) {
        const float u0 = r[1].x - r[0].x, u1 = r[1].y - r[0].y, u2 = r[1].z - r[0].z;
        const float v0 = r[2].x - r[0].x, v1 = r[2].y - r[0].y, v2 = r[2].z - r[0].z;
        const float c0 = u1 * v2 - u2 * v1, c1 = u2 * v0 - u0 * v2, c2 = u0 * v1 - u1 * v0;
        const float len2 = (c0 * c0 + c1 * c1) + c2 * c2;
        ok = cloud_finite(len2) && len2 > 0.0f;
        if (ok) {
            const float len = sqrtf(len2);
            float n0 = c0 / len, n1 = c1 / len, n2 = c2 / len;
            float t = (n0 * r[0].x + n1 * r[0].y) + n2 * r[0].z;
            ok = plane_finite3(n0, n1, n2) && cloud_finite(t) && (((__float_as_uint(n0) | __float_as_uint(n1) | __float_as_uint(n2)) & 0x7FFFFFFFu) != 0u);
            bool flip;
            if (p.prior) {
                float d = (n0 * p.ax + n1 * p.ay) + n2 * p.az;
                ok = ok && cloud_finite(d);
                flip = ok && d < 0.0f;
                if (flip) d = -d;
                ok = ok && d >= p.thr;
            } else {
                flip = ok && t > 0.0f;
            }
            if (flip) { n0 = -n0; n1 = -n1; n2 = -n2; t = -t; }
            if (ok) {
                nrm = make_float4(n0, n1, n2, 0.0f - t);
                anchor = make_float4(r[0].x, r[0].y, r[0].z, 0.0f);   // votes = 0: the vote adds to it
            }
        }
    }
    planes[2 * (size_t)k] = nrm;
    planes[2 * (size_t)k + 1] = anchor;
}

__global__ __launch_bounds__(PLANE_THREADS) void sgm_plane_votes_k(const float4* __restrict__ records, size_t capacity,
                                                                   const unsigned* __restrict__ count, const uint8_t* __restrict__ labels,
                                                                   float4* __restrict__ planes, unsigned K, int dist_bits)
{
    __shared__ float4 s_plane[PLANE_MAX_K][2];
    __shared__ unsigned s_votes[PLANE_MAX_K];
    const unsigned long long n = plane_count(capacity, count);
    for (unsigned k = threadIdx.x; k < K; k += PLANE_THREADS) {
        float4 nrm, anchor;
        plane_load(planes + 2 * (size_t)k, dist_bits, nrm, anchor);
        s_plane[k][0] = nrm;
        s_plane[k][1] = anchor;
        s_votes[k] = 0u;
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long trip = (unsigned long long)PLANE_THREADS * PLANE_RECORDS, wave_trip = 64ull * PLANE_RECORDS;
    for (unsigned long long base = blockIdx.x * trip + wave * wave_trip; base < n; base += gridDim.x * trip) {
        float x[PLANE_RECORDS], y[PLANE_RECORDS], z[PLANE_RECORDS];
        unsigned long long ok[PLANE_RECORDS];                 // wave-uniform: the lanes whose record votes at all
#pragma unroll
        for (int r = 0; r < PLANE_RECORDS; ++r) {
            const unsigned long long at = base + (unsigned)r * 64u + lane;
            bool votes = false;
            x[r] = y[r] = z[r] = 0.0f;
            if (at < n) {
                const float4 rec = records[at];
                x[r] = rec.x; y[r] = rec.y; z[r] = rec.z;
                votes = plane_finite3(rec.x, rec.y, rec.z) && (labels == nullptr || labels[at] == 0);
            }
            ok[r] = __ballot(votes);
        }
        // candidate kb + j is lane j's to count: 64 candidates pass, then every lane adds its own to the workgroup's counter
        for (unsigned kb = 0; kb < K; kb += 64u) {
            unsigned mine = 0;
            const unsigned top = K - kb < 64u ? K - kb : 64u;
            for (unsigned j = 0; j < top; ++j) {
                const float4 nrm = s_plane[kb + j][0], anchor = s_plane[kb + j][1];
                unsigned c = 0;
#pragma unroll
                for (int r = 0; r < PLANE_RECORDS; ++r) c += (unsigned)__popcll(__ballot(plane_inlier(x[r], y[r], z[r], nrm, anchor)) & ok[r]);
                mine += lane == j ? c : 0u;
            }
            if (mine != 0u) atomicAdd(&s_votes[kb + lane], mine);
        }
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < K; k += PLANE_THREADS) {
        const unsigned v = s_votes[k];
        if (v != 0u) atomicAdd(reinterpret_cast<unsigned*>(planes + 2 * (size_t)k + 1) + 3, v);
    }
}

// one wave: the non-void candidate with the most votes, ties to the smallest k
__global__ __launch_bounds__(64) void sgm_plane_best_k(const float4* __restrict__ planes, unsigned K, float4* __restrict__ best)
{
    unsigned long long key = 0ull;                            // votes << 32 | ~k of the best non-void candidate so far
    int have = 0;
    for (unsigned k = threadIdx.x; k < K; k += 64u) {
        const float4 nrm = planes[2 * (size_t)k], anchor = planes[2 * (size_t)k + 1];
        if (plane_is_void(nrm)) continue;
        const unsigned long long mine = ((unsigned long long)__float_as_uint(anchor.w) << 32) | (0xFFFFFFFFu - k);
        if (!have || mine > key) key = mine;
        have = 1;
    }
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const unsigned long long other = __shfl_xor(key, step);
        const int other_has = __shfl_xor(have, step);
        if (other_has && (!have || other > key)) key = other;
        have |= other_has;
    }
    if (threadIdx.x == 0) {
        float4 nrm = make_float4(0.0f, 0.0f, 0.0f, 0.0f), anchor = nrm;
        if (have) {
            const unsigned k = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
            nrm = planes[2 * (size_t)k];
            anchor = planes[2 * (size_t)k + 1];
        }
        best[0] = nrm;
        best[1] = anchor;
    }
}

__global__ __launch_bounds__(PLANE_THREADS) void sgm_plane_sums_k(const float4* __restrict__ records, size_t capacity,
                                                                  const unsigned* __restrict__ count, const uint8_t* __restrict__ labels,
                                                                  const float4* __restrict__ plane, int dist_bits, float span,
                                                                  long long* __restrict__ sums)
{
    __shared__ long long s_wave[PLANE_WAVES][PLANE_SUMS];
    const unsigned long long n = plane_count(capacity, count);
    float4 nrm, anchor;
    plane_load(plane, dist_bits, nrm, anchor);
    long long acc[PLANE_SUMS];
#pragma unroll
    for (int k = 0; k < PLANE_SUMS; ++k) acc[k] = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * PLANE_THREADS;
    for (unsigned long long at = (unsigned long long)blockIdx.x * PLANE_THREADS + threadIdx.x; at < n; at += stride) {
        const float4 rec = records[at];
        if (!plane_finite3(rec.x, rec.y, rec.z)) continue;
        if (labels != nullptr && labels[at] != 0) continue;
        if (!plane_inlier(rec.x, rec.y, rec.z, nrm, anchor)) continue;
        const float e[3] = {(rec.x - anchor.x) / span, (rec.y - anchor.y) / span, (rec.z - anchor.z) / span};
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) ok = ok && cloud_finite(e[i]) && fabsf(e[i]) <= 8.0f;
        if (!ok) continue;
        long long q[4];
#pragma unroll
        for (int i = 0; i < 3; ++i) q[i] = (long long)(int)rintf(e[i] * 65536.0f);
        q[3] = 1;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = i; j < 4; ++j) acc[k++] += q[i] * q[j];
        }
    }
    // the wave's lanes, then the workgroup's waves, then the grid's workgroups: integer sums, any order gives the same bytes
#pragma unroll
    for (int k = 0; k < PLANE_SUMS; ++k) {
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) acc[k] += __shfl_xor(acc[k], step);
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < PLANE_SUMS; ++k) s_wave[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < PLANE_SUMS) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < PLANE_WAVES; ++w) sum += s_wave[w][threadIdx.x];
        if (sum != 0) atomicAdd(reinterpret_cast<unsigned long long*>(sums + threadIdx.x), (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(PLANE_THREADS) void sgm_plane_label_k(const float4* __restrict__ records, size_t capacity,
                                                                   const unsigned* __restrict__ count, const float4* __restrict__ plane,
                                                                   int dist_bits, unsigned label, uint8_t* __restrict__ labels)
{
    const unsigned long long n = plane_count(capacity, count);
    float4 nrm, anchor;
    plane_load(plane, dist_bits, nrm, anchor);
    const unsigned long long stride = (unsigned long long)gridDim.x * PLANE_THREADS;
    for (unsigned long long at = (unsigned long long)blockIdx.x * PLANE_THREADS + threadIdx.x; at < n; at += stride) {
        const float4 rec = records[at];
        if (!plane_finite3(rec.x, rec.y, rec.z) || labels[at] != 0) continue;
        if (plane_inlier(rec.x, rec.y, rec.z, nrm, anchor)) labels[at] = (uint8_t)label;
    }
}

// the workgroups of a launch: `per_block` records each up to PLANE_MAX_BLOCKS, the lanes stride beyond
static unsigned plane_blocks(size_t capacity, size_t per_block)
{
    const size_t blocks = (capacity + per_block - 1) / per_block;
    return (unsigned)(blocks > PLANE_MAX_BLOCKS ? PLANE_MAX_BLOCKS : (blocks < 1 ? 1 : blocks));
}

static bool plane_list_ok(const void* records, size_t capacity, const void* count)
{
    return records && capacity <= ((size_t)1 << 32) && (uintptr_t)records % 16 == 0 && (uintptr_t)count % 4 == 0;
}

static bool plane_dist_ok(float dist, int* bits)
{
    memcpy(bits, &dist, sizeof *bits);
    return *bits > 0 && *bits < 0x7F800000;                   // finite and > 0
}

extern "C" {

int sgmd_plane_votes(int ord, void* stream, const sgmd_plane* p, const void* records, size_t capacity, const void* count,
                     const void* labels, void* planes)
{
    PlaneRule r;
    if (!p || !plane_list_ok(records, capacity, count) || !planes || (uintptr_t)planes % 16 != 0 || p->hypotheses < 1 ||
        p->hypotheses > PLANE_MAX_K || !plane_dist_ok(p->dist, &r.dist_bits)) {
        fprintf(stderr, "sgm_mi355x: sgmd_plane_votes: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    r.K = (unsigned)p->hypotheses; r.seed = p->seed; r.prior = p->prior;
    r.ax = p->axis[0]; r.ay = p->axis[1]; r.az = p->axis[2]; r.thr = p->threshold; r.span = p->span;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sgm_plane_candidates_k, dim3((r.K + 63u) / 64u), dim3(64), 0, st, (const float4*)records, capacity,
                       (const unsigned*)count, (const uint8_t*)labels, (float4*)planes, r);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sgm_plane_votes_k, dim3(plane_blocks(capacity, (size_t)PLANE_THREADS * PLANE_RECORDS)), dim3(PLANE_THREADS), 0, st,
                       (const float4*)records, capacity, (const unsigned*)count, (const uint8_t*)labels, (float4*)planes, r.K, r.dist_bits);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_plane_best(int ord, void* stream, const void* planes, int K, void* best)
{
    if (!planes || !best || K < 1 || K > PLANE_MAX_K || (uintptr_t)planes % 16 != 0 || (uintptr_t)best % 16 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_plane_best: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    hipLaunchKernelGGL(sgm_plane_best_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float4*)planes, (unsigned)K, (float4*)best);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_plane_sums(int ord, void* stream, const sgmd_plane* p, const void* records, size_t capacity, const void* count,
                    const void* labels, const void* plane, void* sums)
{
    int dist_bits;
    if (!p || !plane_list_ok(records, capacity, count) || capacity > ((size_t)1 << 24) || !plane || (uintptr_t)plane % 16 != 0 || !sums ||
        (uintptr_t)sums % 8 != 0 || !plane_dist_ok(p->dist, &dist_bits) || !(p->span > 0.0f)) {
        fprintf(stderr, "sgm_mi355x: sgmd_plane_sums: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(sums, 0, PLANE_SUMS * sizeof(long long), st));
    hipLaunchKernelGGL(sgm_plane_sums_k, dim3(plane_blocks(capacity, PLANE_THREADS)), dim3(PLANE_THREADS), 0, st, (const float4*)records,
                       capacity, (const unsigned*)count, (const uint8_t*)labels, (const float4*)plane, dist_bits, p->span, (long long*)sums);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_plane_label(int ord, void* stream, const sgmd_plane* p, const void* records, size_t capacity, const void* count,
                     const void* plane, int label, void* labels)
{
    int dist_bits;
    if (!p || !plane_list_ok(records, capacity, count) || !plane || (uintptr_t)plane % 16 != 0 || !labels || label < 1 || label > 255 ||
        !plane_dist_ok(p->dist, &dist_bits)) {
        fprintf(stderr, "sgm_mi355x: sgmd_plane_label: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    hipLaunchKernelGGL(sgm_plane_label_k, dim3(plane_blocks(capacity, PLANE_THREADS)), dim3(PLANE_THREADS), 0, (hipStream_t)stream,
                       (const float4*)records, capacity, (const unsigned*)count, (const float4*)plane, dist_bits, (unsigned)label,
                       (uint8_t*)labels);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
