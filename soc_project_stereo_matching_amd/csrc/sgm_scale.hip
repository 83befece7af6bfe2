#include "sgm_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): matching at 1/f scale.  The contract is written out
// in include/sgm_mi355x.h (sgm_scale_spec); tests/scaled_ref.py restates it in numpy.
//
//   downscale   f x f box mean with rounding, u8 or u16 samples: a streaming kernel, one output
//               sample per lane, a lane's f samples of a row in ONE load where the image's address
//               and width allow it (else one load per sample, same results)
//   upscale     per full-resolution pixel: the prior by guided selection among four low-resolution
//               neighbours (compares and selects), then the re-search: Hamming costs of the
//               full-resolution census words over a (2r+1)^2 window for the 2f+1 disparities around
//               the prior, integer arithmetic, one float divide for the sub-pixel term
//
// Layout of the re-search (sgm_upscale_k<F, R>): a workgroup is 64 x 4 pixels, one pixel per lane,
// a wave is one image row of 64 pixels.  The workgroup's (64 + 2R) x (4 + 2R) reference-view words
// sit in LDS (lanes of a wave read adjacent dwords: no bank conflict).  The other view cannot be
// tiled, priors differ per lane: per window row a lane loads the 2R + 1 + 2F contiguous words its
// 2F + 1 candidates share -- word e of them serves every pair (dx, s) with dx - s = e -- so a pixel
// takes (2R+1)(2R+1+2F) loads for (2R+1)^2 (2F+1) terms (77 for 245 at r = 3, f = 2).  Neighbouring
// lanes with equal priors read neighbouring words, so the loads of a wave coalesce where the map is
// smooth.  The costs are summed per shift s = dx - e, which is the candidate offset o for the left
// view and -o for the right one: every register array is indexed by compile-time constants.
// Every column and row is bounds-checked; a lane whose whole footprint is inside the frame takes
// the same body without the per-term checks.  No atomics, nothing waits for another workgroup.
//
// This translation unit is compiled with -fno-honor-nans like the others, and a caller's map may hold
// NaN: "finite" is tested on the bit pattern, and on words that were LOADED as integers -- the same
// test on a float's bits is folded by the compiler into a float compare that is free to call a NaN
// finite (v_cmp_eq_f32 |v|, inf).  A map entry becomes a float only once it is known to be finite.
// ============================================================================================

#define SCALE_BW 64
#define SCALE_BH 4
#define SCALE_THREADS (SCALE_BW * SCALE_BH)
#define SCALE_OUTSIDE 24                     // the cost of a window pixel or a partner outside the frame
#define SCALE_PRIOR_MAX 1048576.0f           // priors are clamped to +-2^20 before rounding (no candidate is admitted out there)

struct ScaleParams {
    int W, H;                                // full resolution
    int w, h;                                // low resolution
    int wide;                                // samples are u16
    int penalty, d_lo, d_hi, right;
};

#define SCALE_INF_BITS 0x7F800000u
static __device__ __forceinline__ bool scale_finite(uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

// ---- downscale -------------------------------------------------------------------------------------------------------------

template <typename T, int F> struct ScaleRow;                           // the F samples of a row of a block, in one load
template <> struct ScaleRow<uint8_t, 2> { typedef uint16_t type; };
template <> struct ScaleRow<uint8_t, 4> { typedef uint32_t type; };
template <> struct ScaleRow<uint16_t, 2> { typedef uint32_t type; };
template <> struct ScaleRow<uint16_t, 4> { typedef uint2 type; };

// grid: (ceil(w / 64), ceil(h / 4), frames); VEC: in + every row start is a multiple of F samples
template <typename T, int F, bool VEC>
__global__ __launch_bounds__(SCALE_THREADS) void sgm_downscale_k(const T* __restrict__ in, T* __restrict__ out, int W, int H, int w, int h)
{
    const int i = blockIdx.x * SCALE_BW + (threadIdx.x & (SCALE_BW - 1));
    const int j = blockIdx.y * SCALE_BH + (threadIdx.x / SCALE_BW);
    if (i >= w || j >= h) return;
    const T* src = in + (size_t)blockIdx.z * W * H + (size_t)(F * j) * W + (size_t)F * i;
    unsigned sum = F * F / 2;
#pragma unroll
    for (int r = 0; r < F; ++r) {
        if constexpr (VEC) {
            typedef typename ScaleRow<T, F>::type row_t;
            const row_t v = *reinterpret_cast<const row_t*>(src + (size_t)r * W);
            T e[F];
            __builtin_memcpy(e, &v, sizeof v);
#pragma unroll
            for (int c = 0; c < F; ++c) sum += e[c];
        } else {
#pragma unroll
            for (int c = 0; c < F; ++c) sum += src[(size_t)r * W + c];
        }
    }
    out[(size_t)blockIdx.z * w * h + (size_t)j * w + i] = (T)(sum / (F * F));
}

// ---- the prior: guided selection among the four low-resolution neighbours ----------------------------------------------------

static __device__ __forceinline__ unsigned scale_sample(const void* img, size_t i, int wide)
{
    return wide ? (unsigned)static_cast<const uint16_t*>(img)[i] : (unsigned)static_cast<const uint8_t*>(img)[i];
}

// the bits of the prior; those of +INF where no candidate is finite
template <int F>
static __device__ __forceinline__ uint32_t scale_prior(const ScaleParams& c, const uint32_t* __restrict__ small, const void* __restrict__ gs,
                                                    const void* __restrict__ gf, size_t frame, int y, int x)
{
    constexpr int F2 = 2 * F, SH = F == 2 ? 2 : 3;                       // 2f = 1 << SH
    const int ny = 2 * y + 1 - F, nx = 2 * x + 1 - F;
    const int jf = ny >> SH, fi = nx >> SH;                              // floor, also of a negative numerator
    const int ay = ny - F2 * jf, ax = nx - F2 * fi;
    const int j0 = min(max(jf, 0), c.h - 1), j1 = min(max(jf + 1, 0), c.h - 1);
    const int i0 = min(max(fi, 0), c.w - 1), i1 = min(max(fi + 1, 0), c.w - 1);
    const size_t sb = frame * (size_t)c.w * c.h;
    const size_t at[4] = {sb + (size_t)j0 * c.w + i0, sb + (size_t)j0 * c.w + i1, sb + (size_t)j1 * c.w + i0, sb + (size_t)j1 * c.w + i1};
    const int wgt[4] = {(F2 - ay) * (F2 - ax), (F2 - ay) * ax, ay * (F2 - ax), ay * ax};
    const int g = (int)scale_sample(gf, frame * (size_t)c.W * c.H + (size_t)y * c.W + x, c.wide);
    uint32_t best = SCALE_INF_BITS;
    int best_diff = 0x7FFFFFFF, best_w = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t d = small[at[k]];
        const int diff = abs((int)scale_sample(gs, at[k], c.wide) - g);
        const bool take = scale_finite(d) && (diff < best_diff || (diff == best_diff && wgt[k] > best_w));
        best = take ? d : best;
        best_diff = take ? diff : best_diff;
        best_w = take ? wgt[k] : best_w;
    }
    if (best_w < 0) return SCALE_INF_BITS;                               // no candidate was finite
    return __float_as_uint((float)F * __uint_as_float(best));            // exact: f is a power of two (a huge entry may overflow to INF)
}

// radius < 0: the guided upscale alone
template <int F>
__global__ __launch_bounds__(SCALE_THREADS) void sgm_upscale_prior_k(ScaleParams c, const uint32_t* __restrict__ small,
                                                                     const void* __restrict__ gs, const void* __restrict__ gf,
                                                                     uint32_t* __restrict__ out)
{
    const int x = blockIdx.x * SCALE_BW + (threadIdx.x & (SCALE_BW - 1));
    const int y = blockIdx.y * SCALE_BH + (threadIdx.x / SCALE_BW);
    if (x >= c.W || y >= c.H) return;
    out[(size_t)blockIdx.z * c.W * c.H + (size_t)y * c.W + x] = scale_prior<F>(c, small, gs, gf, blockIdx.z, y, x);
}

// ---- the re-search -----------------------------------------------------------------------------------------------------------

// A[s + F] += the window's costs at shift s: the other view's column of window pixel (y + dy, x + dx) is base + dx - s
template <int F, int R, bool CHECK>
static __device__ __forceinline__ void scale_costs(const ScaleParams& c, const uint32_t* tile, const uint32_t* __restrict__ oth, int y,
                                                   int x, int tx, int ty, int base, int (&A)[2 * F + 1])
{
    constexpr int TW = SCALE_BW + 2 * R, NW = 2 * R + 1 + 2 * F;
#pragma unroll
    for (int dyi = 0; dyi <= 2 * R; ++dyi) {
        const int yy = y + dyi - R;
        if (yy < 0 || yy >= c.H) {                                       // wave-uniform: a wave is one image row
#pragma unroll
            for (int k = 0; k <= 2 * F; ++k) A[k] += SCALE_OUTSIDE * (2 * R + 1);
            continue;
        }
        const uint32_t* orow = oth + (size_t)yy * c.W;
        uint32_t ov[NW];
        unsigned okm = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int col = base + j - (R + F);
            const bool ok = !CHECK || (unsigned)col < (unsigned)c.W;
            ov[j] = ok ? orow[col] : 0u;
            okm |= (unsigned)ok << j;
        }
#pragma unroll
        for (int dxi = 0; dxi <= 2 * R; ++dxi) {
            const uint32_t ref = tile[(ty + dyi) * TW + tx + dxi];
            const bool qok = !CHECK || (unsigned)(x + dxi - R) < (unsigned)c.W;
#pragma unroll
            for (int k = 0; k <= 2 * F; ++k) {
                const int j = dxi - (k - F) + F;                         // e = dx - s, j = e + R + F, dx = dxi - R, s = k - F
                const int t = __popc(ref ^ ov[j]);
                A[k] += (!CHECK || (qok && ((okm >> j) & 1u))) ? t : SCALE_OUTSIDE;
            }
        }
    }
}

template <int F, int R>
__global__ __launch_bounds__(SCALE_THREADS) void sgm_upscale_k(ScaleParams c, const uint32_t* __restrict__ small, const void* __restrict__ gs,
                                                               const void* __restrict__ gf, const uint32_t* __restrict__ cref,
                                                               const uint32_t* __restrict__ coth, uint32_t* __restrict__ out)
{
    constexpr int TW = SCALE_BW + 2 * R, TH = SCALE_BH + 2 * R, N = 2 * F + 1, WIN = (2 * R + 1) * (2 * R + 1);
    __shared__ uint32_t tile[TW * TH];
    const size_t frame_px = (size_t)blockIdx.z * c.W * c.H;
    const int x0 = blockIdx.x * SCALE_BW, y0 = blockIdx.y * SCALE_BH;
    for (int t = threadIdx.x; t < TW * TH; t += SCALE_THREADS) {
        const int r = t / TW, col = t - r * TW;
        const int yy = y0 + r - R, xx = x0 + col - R;
        const bool in = (unsigned)yy < (unsigned)c.H && (unsigned)xx < (unsigned)c.W;
        tile[t] = in ? cref[frame_px + (size_t)yy * c.W + xx] : 0u;       // outside: never used, those terms cost SCALE_OUTSIDE
    }
    __syncthreads();
    const int tx = threadIdx.x & (SCALE_BW - 1), ty = threadIdx.x / SCALE_BW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= c.W || y >= c.H) return;
    uint32_t* o = out + frame_px + (size_t)y * c.W + x;
    const uint32_t prior_bits = scale_prior<F>(c, small, gs, gf, blockIdx.z, y, x);
    if (!scale_finite(prior_bits)) { *o = prior_bits; return; }
    const int p = (int)rintf(fminf(fmaxf(__uint_as_float(prior_bits), -SCALE_PRIOR_MAX), SCALE_PRIOR_MAX));
    if (p + F < c.d_lo || p - F > c.d_hi) { *o = prior_bits; return; }   // no candidate is admitted
    const int base = c.right ? x + p : x - p;
    int A[N];
#pragma unroll
    for (int k = 0; k < N; ++k) A[k] = 0;
    const bool inside = x - R >= 0 && x + R < c.W && base - (R + F) >= 0 && base + (R + F) < c.W;
    if (inside) scale_costs<F, R, false>(c, tile, coth + frame_px, y, x, tx, ty, base, A);
    else scale_costs<F, R, true>(c, tile, coth + frame_px, y, x, tx, ty, base, A);
    // C[k]: candidate o = k - F; shift s = o for the left view, -o for the right one
    int C[N];
    bool adm[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int oo = k - F, d = p + oo;
        C[k] = 2 * (c.right ? A[N - 1 - k] : A[k]) + c.penalty * abs(oo) * WIN;
        adm[k] = c.d_lo <= d && d <= c.d_hi;
    }
    // smallest C, then smaller |o|, then smaller d: candidates in the order 0, -1, +1, -2, +2, ... with a strict compare
    int best = -1, bc = 0x7FFFFFFF;
#pragma unroll
    for (int m = 0; m < N; ++m) {
        const int oo = (m == 0) ? 0 : ((m & 1) ? -((m + 1) / 2) : m / 2), k = oo + F;
        const bool take = adm[k] && C[k] < bc;
        best = take ? k : best;
        bc = take ? C[k] : bc;
    }
    // its neighbours, picked by compile-time indices (a run-time index would send C[] to scratch)
    int cm = 0, cp = 0;
    bool both = false;
#pragma unroll
    for (int k = 1; k < N - 1; ++k)
        if (best == k) { cm = C[k - 1]; cp = C[k + 1]; both = adm[k - 1] && adm[k + 1]; }
    const int d = p + best - F, den = cm + cp - 2 * bc;
    float v = (float)d;
    if (both && den > 0) v = v + (float)(cm - cp) / (float)(2 * den);
    *o = __float_as_uint(v);
}

template <typename T>
static void downscale_launch(const sgmd_scale* c, hipStream_t st, const void* in, void* out, int w, int h)
{
    const dim3 grid((w + SCALE_BW - 1) / SCALE_BW, (h + SCALE_BH - 1) / SCALE_BH, c->B);
    const T* src = (const T*)in;
    T* dst = (T*)out;
    const bool vec = (uintptr_t)in % (sizeof(T) * c->f) == 0 && c->W % c->f == 0;
    if (c->f == 2) {
        if (vec) hipLaunchKernelGGL((sgm_downscale_k<T, 2, true>), grid, dim3(SCALE_THREADS), 0, st, src, dst, c->W, c->H, w, h);
        else hipLaunchKernelGGL((sgm_downscale_k<T, 2, false>), grid, dim3(SCALE_THREADS), 0, st, src, dst, c->W, c->H, w, h);
    } else {
        if (vec) hipLaunchKernelGGL((sgm_downscale_k<T, 4, true>), grid, dim3(SCALE_THREADS), 0, st, src, dst, c->W, c->H, w, h);
        else hipLaunchKernelGGL((sgm_downscale_k<T, 4, false>), grid, dim3(SCALE_THREADS), 0, st, src, dst, c->W, c->H, w, h);
    }
}

template <int F>
static void upscale_launch(const sgmd_scale* c, const ScaleParams& p, dim3 grid, hipStream_t st, const uint32_t* small, const void* gs,
                           const void* gf, const uint32_t* cref, const uint32_t* coth, uint32_t* out)
{
#define SCALE_CASE(R) case R: hipLaunchKernelGGL((sgm_upscale_k<F, R>), grid, dim3(SCALE_THREADS), 0, st, p, small, gs, gf, cref, coth, out); break
    switch (c->radius) {
        SCALE_CASE(0); SCALE_CASE(1); SCALE_CASE(2); SCALE_CASE(3); SCALE_CASE(4);
        default: hipLaunchKernelGGL((sgm_upscale_prior_k<F>), grid, dim3(SCALE_THREADS), 0, st, p, small, gs, gf, out); break;
    }
#undef SCALE_CASE
}

static bool scale_args_ok(const sgmd_scale* c)
{
    return c && c->W >= 1 && c->H >= 1 && c->B >= 1 && c->B <= 65535 && (c->f == 2 || c->f == 4) && c->W / c->f >= 1 && c->H / c->f >= 1 &&
           c->bits >= 8 && c->bits <= 16 && c->radius <= 4 && (c->H + SCALE_BH - 1) / SCALE_BH <= 65535;
}

extern "C" {

int sgmd_downscale(int ord, void* stream, const sgmd_scale* c, const void* in, void* out)
{
    const bool wide = c && c->bits > 8;
    if (!scale_args_ok(c) || !in || !out || (wide && (((uintptr_t)in | (uintptr_t)out) & 1u))) {
        fprintf(stderr, "sgm_mi355x: sgmd_downscale: bad arguments\n");
        return (int)hipErrorInvalidValue;
    }
    HIP_TRY(hipSetDevice(ord));
    if (wide) downscale_launch<uint16_t>(c, (hipStream_t)stream, in, out, c->W / c->f, c->H / c->f);
    else downscale_launch<uint8_t>(c, (hipStream_t)stream, in, out, c->W / c->f, c->H / c->f);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_upscale(int ord, void* stream, const sgmd_scale* c, const void* disp_small, const void* guide_small, const void* guide_full,
                 const void* census_ref, const void* census_oth, void* disp_full)
{
    const bool wide = c && c->bits > 8;
    if (!scale_args_ok(c) || !disp_small || !guide_small || !guide_full || !disp_full ||
        (c->radius >= 0 && (!census_ref || !census_oth)) || (wide && (((uintptr_t)guide_small | (uintptr_t)guide_full) & 1u)) ||
        (((uintptr_t)disp_small | (uintptr_t)disp_full | (uintptr_t)census_ref | (uintptr_t)census_oth) & 3u)) {
        fprintf(stderr, "sgm_mi355x: sgmd_upscale: bad arguments\n");
        return (int)hipErrorInvalidValue;
    }
    HIP_TRY(hipSetDevice(ord));
    const ScaleParams p = {c->W, c->H, c->W / c->f, c->H / c->f, wide ? 1 : 0, c->penalty, c->d_lo, c->d_hi, c->right ? 1 : 0};
    const dim3 grid((c->W + SCALE_BW - 1) / SCALE_BW, (c->H + SCALE_BH - 1) / SCALE_BH, c->B);
    if (c->f == 2)
        upscale_launch<2>(c, p, grid, (hipStream_t)stream, (const uint32_t*)disp_small, guide_small, guide_full, (const uint32_t*)census_ref,
                          (const uint32_t*)census_oth, (uint32_t*)disp_full);
    else
        upscale_launch<4>(c, p, grid, (hipStream_t)stream, (const uint32_t*)disp_small, guide_small, guide_full, (const uint32_t*)census_ref,
                          (const uint32_t*)census_oth, (uint32_t*)disp_full);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
