#include "sgm_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): the temporal filter of a stream of disparity maps.
// The contract is written out in include/sgm_mi355x.h (sgm_temporal_spec); tests/temporal_ref.py
// restates it in numpy and tests/stub_temporal.c in plain C.
//
// Pure streaming.  A lane owns V consecutive pixels of one stream (V = 4: 16-byte loads and stores
// of the map and of hv, one word of four hb, 8 bytes of confidence; V = 1 where the pixel count or a
// pointer does not allow that) and walks the `steps` maps of that stream in order with hv / hb in
// registers: the history is read once and written once per call however many steps there are.  The
// map (and confidence) values of step t + 1 are loaded before the arithmetic of step t.
//
// Work is cut into chunks of TP_THREADS lane items of ONE stream; a capped grid strides over the
// chunks.  Because a chunk never straddles two streams, the statistics of a wave belong to one map
// per step: ballots per class, the four waves' counts summed through LDS, one atomic add per
// workgroup, step and class.  With few maps those adds would all land on a few cache lines and queue
// up there (8 maps: two lines; one add per WAVE and class straight into them took 0.76 ms for a
// kernel that streams in 13 us), so they go to one of up to TP_REPLICAS copies of the counters in a
// scratch, chosen by chunk, and a second
// small launch sums the copies into the caller's counters; with many maps the rows themselves spread
// the adds and the kernel adds into the caller's counters directly.
//
// (this translation unit is compiled with -fno-honor-nans like the others: a caller's map or history
// may hold NaN, so "finite" is tested on the bit pattern, values travel as bit patterns, and no
// arithmetic ever sees a value that is not finite: an operand that does not count is replaced by 0)
// ============================================================================================

#define TP_THREADS 256
#define TP_GRID_MAX 2048
#define TP_INF 0x7F800000u
#define TP_CLASSES 5
#define TP_STAT_ROWS 16384        // rows of TP_CLASSES counters the scratch holds: replicas x maps
#define TP_REPLICAS 256

struct TemporalParams {
    float a, b, delta;
    unsigned nmask, k, min_conf;
    unsigned steps, pixels;       // maps per stream, pixels of one map
    unsigned items;               // lane items per stream: pixels / V
    unsigned cps, chunks;         // chunks per stream, chunks in all
    unsigned replicas, maps;      // statistics: copies of the counters [replicas][maps][TP_CLASSES] the waves spread their adds over
};

static __device__ __forceinline__ bool tp_finite(unsigned bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

// ONE step of ONE pixel (include/sgm_mi355x.h, "One step"): the output value; hv, hb are updated, cls is the decision
static __device__ __forceinline__ unsigned tp_step(const TemporalParams& c, unsigned xb, bool conf_ok, unsigned& hvb, unsigned& hb,
                                                   unsigned& cls)
{
    const bool valid = tp_finite(xb) && conf_ok;
    const bool hfin = tp_finite(hvb);
    const float x = __uint_as_float(valid ? xb : 0u), h = __uint_as_float(hfin ? hvb : 0u);
    const bool near = fabsf(__fsub_rn(x, h)) <= c.delta;
    const float smooth = __fadd_rn(__fmul_rn(c.a, x), __fmul_rn(c.b, h));
    const bool hold = hfin && (unsigned)__popc(hb & c.nmask) >= c.k;            // (n == 0: k = 9, never)
    cls = valid ? (hfin ? (near ? 1u : 2u) : 0u) : (hold ? 3u : 4u);
    const unsigned out = valid ? (hfin && near ? __float_as_uint(smooth) : xb) : (hold ? hvb : TP_INF);
    hb = ((hb << 1) | (valid ? 1u : 0u)) & 0xFFu;
    hvb = tp_finite(out) ? out : (hb == 0u ? TP_INF : hvb);
    return out;
}

// the V map values (and confidences) of a lane item at element offset `at`
template <int V, bool CONF>
static __device__ __forceinline__ void tp_load(const float* __restrict__ maps, const uint16_t* __restrict__ conf, size_t at,
                                               unsigned (&x)[V], unsigned (&k)[V])
{
    if constexpr (V == 4) {
        const uint4 t = *reinterpret_cast<const uint4*>(maps + at);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
        if constexpr (CONF) {
            const uint2 w = *reinterpret_cast<const uint2*>(conf + at);
            k[0] = w.x & 0xFFFFu; k[1] = w.x >> 16; k[2] = w.y & 0xFFFFu; k[3] = w.y >> 16;
        }
    } else {
        x[0] = __float_as_uint(maps[at]);
        if constexpr (CONF) k[0] = conf[at];
    }
}

template <int V, bool CONF, bool STATS>
__global__ __launch_bounds__(TP_THREADS) void sgm_temporal_k(TemporalParams c, float* __restrict__ maps,
                                                             const uint16_t* __restrict__ conf, float* __restrict__ hist_value,
                                                             uint8_t* __restrict__ hist_bits, unsigned* __restrict__ stats)
{
    __shared__ unsigned s_count[STATS ? 2 : 1][TP_THREADS / 64][TP_CLASSES];
    unsigned turn = 0;
    for (unsigned chunk = blockIdx.x; chunk < c.chunks; chunk += gridDim.x) {
        const unsigned stream = chunk / c.cps;
        const unsigned item = (chunk - stream * c.cps) * TP_THREADS + threadIdx.x;
        const bool live = item < c.items;                     // (only the last chunk of a stream has lanes without an item)
        const size_t hat = (size_t)stream * c.pixels + (size_t)item * V;
        size_t at = (size_t)stream * c.steps * c.pixels + (size_t)item * V;
        unsigned hv[V], hb[V], x[V], k[V];
#pragma unroll
        for (int i = 0; i < V; ++i) { hv[i] = TP_INF; hb[i] = 0u; x[i] = TP_INF; k[i] = 65535u; }
        if (live) {
            if constexpr (V == 4) {
                const uint4 t = *reinterpret_cast<const uint4*>(hist_value + hat);
                hv[0] = t.x; hv[1] = t.y; hv[2] = t.z; hv[3] = t.w;
                const unsigned w = *reinterpret_cast<const unsigned*>(hist_bits + hat);
                hb[0] = w & 255u; hb[1] = (w >> 8) & 255u; hb[2] = (w >> 16) & 255u; hb[3] = w >> 24;
            } else {
                hv[0] = __float_as_uint(hist_value[hat]);
                hb[0] = hist_bits[hat];
            }
            tp_load<V, CONF>(maps, conf, at, x, k);
        }
        for (unsigned t = 0; t < c.steps; ++t, at += c.pixels) {
            unsigned xn[V], kn[V];
#pragma unroll
            for (int i = 0; i < V; ++i) { xn[i] = TP_INF; kn[i] = 65535u; }
            if (live && t + 1 < c.steps) tp_load<V, CONF>(maps, conf, at + c.pixels, xn, kn);      // in flight during this step
            unsigned out[V], cls[V];
#pragma unroll
            for (int i = 0; i < V; ++i) out[i] = tp_step(c, x[i], !CONF || k[i] >= c.min_conf, hv[i], hb[i], cls[i]);
            if (live) {
                if constexpr (V == 4) *reinterpret_cast<uint4*>(maps + at) = make_uint4(out[0], out[1], out[2], out[3]);
                else maps[at] = __uint_as_float(out[0]);
            }
            if constexpr (STATS) {
                // every lane of the workgroup is here (no lane leaves a loop early; chunk and step counts are the workgroup's): the
                // waves' counts for map (stream, t) meet in LDS, one lane per class adds the workgroup's sum.  Two halves of s_count by
                // turns: a half is written again two barriers after it was read
#pragma unroll
                for (unsigned cl = 0; cl < TP_CLASSES; ++cl) {
                    unsigned n = 0;
#pragma unroll
                    for (int i = 0; i < V; ++i) n += (unsigned)__popcll(__ballot(live && cls[i] == cl));
                    if ((threadIdx.x & 63u) == 0) s_count[turn][threadIdx.x >> 6][cl] = n;
                }
                __syncthreads();
                if (threadIdx.x < TP_CLASSES) {
                    unsigned n = 0;
#pragma unroll
                    for (int w = 0; w < TP_THREADS / 64; ++w) n += s_count[turn][w][threadIdx.x];
                    const unsigned copy = chunk % c.replicas;
                    if (n) atomicAdd(stats + ((size_t)copy * c.maps + (size_t)stream * c.steps + t) * TP_CLASSES + threadIdx.x, n);
                }
                turn ^= 1u;
            }
#pragma unroll
            for (int i = 0; i < V; ++i) { x[i] = xn[i]; k[i] = kn[i]; }
        }
        if (live) {
            if constexpr (V == 4) {
                *reinterpret_cast<uint4*>(hist_value + hat) = make_uint4(hv[0], hv[1], hv[2], hv[3]);
                *reinterpret_cast<unsigned*>(hist_bits + hat) = hb[0] | (hb[1] << 8) | (hb[2] << 16) | (hb[3] << 24);
            } else {
                hist_value[hat] = __uint_as_float(hv[0]);
                hist_bits[hat] = (uint8_t)hb[0];
            }
        }
    }
}

// counters[i] = the sum over the copies of copies[r][i], i < n = maps * TP_CLASSES
__global__ __launch_bounds__(TP_THREADS) void sgm_temporal_sum_k(const unsigned* __restrict__ copies, unsigned replicas, unsigned n,
                                                                 unsigned* __restrict__ counters)
{
    const unsigned i = blockIdx.x * TP_THREADS + threadIdx.x;
    if (i >= n) return;
    unsigned sum = 0;
    for (unsigned r = 0; r < replicas; ++r) sum += copies[(size_t)r * n + i];
    counters[i] = sum;
}

// n 32-bit words <- value (the clear of hv: +INF)
__global__ __launch_bounds__(TP_THREADS) void sgm_fill32_k(unsigned* __restrict__ p, unsigned value, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * TP_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * TP_THREADS) p[i] = value;
}

template <int V, bool CONF, bool STATS>
static void tp_launch(hipStream_t st, TemporalParams c, size_t streams, void* maps, const void* conf, void* hv, void* hb, void* stats)
{
    c.items = c.pixels / V;
    c.cps = (c.items + TP_THREADS - 1) / TP_THREADS;
    c.chunks = (unsigned)(streams * c.cps);                   // <= 2^31 items in all
    const unsigned grid = c.chunks < TP_GRID_MAX ? c.chunks : TP_GRID_MAX;
    hipLaunchKernelGGL((sgm_temporal_k<V, CONF, STATS>), dim3(grid), dim3(TP_THREADS), 0, st, c, (float*)maps, (const uint16_t*)conf,
                       (float*)hv, (uint8_t*)hb, (unsigned*)stats);
}

template <int V>
static void tp_dispatch(hipStream_t st, const TemporalParams& c, size_t streams, void* maps, const void* conf, void* hv, void* hb,
                        void* stats)
{
    if (conf && stats) tp_launch<V, true, true>(st, c, streams, maps, conf, hv, hb, stats);
    else if (conf) tp_launch<V, true, false>(st, c, streams, maps, conf, hv, hb, stats);
    else if (stats) tp_launch<V, false, true>(st, c, streams, maps, conf, hv, hb, stats);
    else tp_launch<V, false, false>(st, c, streams, maps, conf, hv, hb, stats);
}

extern "C" {

size_t sgmd_temporal_scratch_bytes(void) { return (size_t)TP_STAT_ROWS * TP_CLASSES * sizeof(unsigned); }

int sgmd_temporal(int ord, void* stream, const sgmd_temporal_params* p, size_t streams, size_t steps, size_t pixels, void* maps,
                  const void* conf, void* hist_value, void* hist_bits, void* stats, void* scratch)
{
    const size_t lim = (size_t)1 << 31;
    if (!p || !maps || !hist_value || !hist_bits || streams < 1 || steps < 1 || pixels < 1 || streams > lim || steps > lim || pixels > lim ||
        streams * steps > lim || streams * steps * pixels > lim || p->n < 0 || p->n > 8 || (p->n > 0 && (p->k < 1 || p->k > p->n)) ||
        ((uintptr_t)maps | (uintptr_t)hist_value | (uintptr_t)stats | (uintptr_t)scratch) % 4 != 0 || (uintptr_t)conf % 2 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_temporal: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const hipStream_t st = (hipStream_t)stream;
    if (p->min_conf == 0) conf = NULL;                        // K >= 0 holds for every K: the instantiation without the loads
    TemporalParams c;
    // the copies of the counters: as many as the scratch holds, none (the caller's counters themselves) without a scratch or with
    // more maps than half its rows
    const size_t nmaps = streams * steps;
    c.maps = (unsigned)nmaps;
    c.replicas = stats && scratch && nmaps <= TP_STAT_ROWS / 2 ? (unsigned)(TP_STAT_ROWS / nmaps < TP_REPLICAS ? TP_STAT_ROWS / nmaps : TP_REPLICAS) : 1u;
    void* counters = c.replicas > 1 ? scratch : stats;
    if (stats) HIP_TRY(hipMemsetAsync(counters, 0, (size_t)c.replicas * nmaps * TP_CLASSES * sizeof(unsigned), st));
    c.a = p->a; c.b = p->b; c.delta = p->delta;
    c.nmask = (1u << p->n) - 1u;
    c.k = p->n > 0 ? (unsigned)p->k : 9u;                     // n == 0: holes are never bridged
    c.min_conf = p->min_conf;
    c.steps = (unsigned)steps;
    c.pixels = (unsigned)pixels;
    c.items = c.cps = c.chunks = 0;
    // four pixels per lane: every map and history row starts at a multiple of four pixels and can be read 16 / 8 / 4 bytes at a time
    const bool vec = pixels % 4 == 0 && (uintptr_t)maps % 16 == 0 && (uintptr_t)hist_value % 16 == 0 && (uintptr_t)hist_bits % 4 == 0 &&
                     (uintptr_t)conf % 8 == 0;
    if (vec) tp_dispatch<4>(st, c, streams, maps, conf, hist_value, hist_bits, stats ? counters : NULL);
    else tp_dispatch<1>(st, c, streams, maps, conf, hist_value, hist_bits, stats ? counters : NULL);
    HIP_TRY(hipGetLastError());
    if (c.replicas > 1) {
        const unsigned n = c.maps * TP_CLASSES;
        hipLaunchKernelGGL(sgm_temporal_sum_k, dim3((n + TP_THREADS - 1) / TP_THREADS), dim3(TP_THREADS), 0, st, (const unsigned*)scratch,
                           c.replicas, n, (unsigned*)stats);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int sgmd_temporal_clear(int ord, void* stream, size_t count, void* hist_value, void* hist_bits)
{
    if (!hist_value || !hist_bits || count < 1 || (uintptr_t)hist_value % 4 != 0) {
        fprintf(stderr, "sgm_mi355x: sgmd_temporal_clear: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const hipStream_t st = (hipStream_t)stream;
    const size_t blocks = (count + TP_THREADS - 1) / TP_THREADS;
    hipLaunchKernelGGL(sgm_fill32_k, dim3((unsigned)(blocks < TP_GRID_MAX ? blocks : TP_GRID_MAX)), dim3(TP_THREADS), 0, st,
                       (unsigned*)hist_value, TP_INF, count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(hist_bits, 0, count, st));
    return 0;
}

}  // extern "C"
