#include "sgm_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): occlusion-aware hole filling, the discontinuity-
// preserving interpolation of Hirschmueller's SGM paper.  The contract is written out in
// include/sgm_mi355x.h (sgm_set_fill_holes); tests/fill_holes_ref.py restates it in numpy.
//
//   classify   one byte per pixel from the two WTA maps BEFORE the LR check (0 valid, 1 occluded,
//              2 mismatched) -- the LR check itself runs in place afterwards and is unchanged
//   fill pass  out-of-place (Jacobi): an INF target takes, of the first finite value along each of
//              the 8 rays within R steps, the second smallest (pass 1, occluded) or the upper median
//              (passes 2 and 3).  Compares and selects only: the result is exact.
// ============================================================================================

// Class of pixel x of one row.  Left view: ref = left WTA map, oth = right WTA map, the arithmetic of sgm_lrcheck_k; right
// view: the mirror image, the arithmetic of sgm_lrcheck_right_k (both in sgm_sum_wta.hip).
__global__ __launch_bounds__(256) void sgm_fill_classify_k(const float* __restrict__ ref, const float* __restrict__ oth,
                                                           uint8_t* __restrict__ cls, int W, int H, float thres, int right,
                                                           int do_check)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const float inf = __builtin_inff();
    const size_t row = (size_t)blockIdx.z * W * H + (size_t)y * W;     // batch: z = frame
    uint8_t c = 0;
    if (do_check) {
        const float d = ref[row + x];
        if (d == inf) {
            c = 2;                                                      // WTA rejected it (uniqueness)
        } else {
            const int xo = right ? (int)((double)((float)x + d) + 0.5) : (int)((double)((float)x - d) + 0.5);
            if (xo < 0 || xo >= W) {
                c = 2;
            } else {
                const float o = oth[row + xo];
                if (o != inf && fabs((double)(d - o)) > (double)thres) {
                    // the other view's pixel points back at xb: something nearer (a larger disparity) there = occluded
                    const int xb = right ? (int)((double)((float)xo - o) + 0.5) : (int)((double)((float)xo + o) + 0.5);
                    c = (xb >= 0 && xb < W && ref[row + xb] > d) ? 1 : 2;
                }
            }
        }
    }
    cls[row + x] = c;
}

static __device__ __forceinline__ void cswap(float& a, float& b)
{
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}

// pass 1: INF pixels of class 1 take s[1] (s[0] if only one candidate); pass 2: INF pixels of class 2 take s[k/2];
// pass 3 (cls may be NULL): every INF pixel takes s[k/2].  Every other pixel is copied.
__global__ __launch_bounds__(256) void sgm_fill_pass_k(const float* __restrict__ in, float* __restrict__ out,
                                                       const uint8_t* __restrict__ cls, int W, int H, int R, int pass)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const float inf = __builtin_inff();
    const size_t fo = (size_t)blockIdx.z * W * H;
    const size_t idx = fo + (size_t)y * W + x;
    const float v = in[idx];
    if (v != inf || (pass != 3 && cls[idx] != pass)) {
        out[idx] = v;
        return;
    }
    const float* f = in + fo;
    // the first finite value along each ray (INF: none within R steps of the image); steps to the edge bound every walk
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = (k == 0 || k == 4 || k == 6) ? 1 : ((k == 1 || k == 5 || k == 7) ? -1 : 0);
        const int dy = (k == 2 || k == 4 || k == 7) ? 1 : ((k == 3 || k == 5 || k == 6) ? -1 : 0);
        int lim = R;
        if (dx > 0) lim = min(lim, W - 1 - x);
        if (dx < 0) lim = min(lim, x);
        if (dy > 0) lim = min(lim, H - 1 - y);
        if (dy < 0) lim = min(lim, y);
        const long step = (long)dy * W + dx;
        const float* p = f + (size_t)y * W + x;
        float got = inf;
        for (int m = 1; m <= lim; ++m) {
            const float t = p[step * m];
            if (t != inf) { got = t; break; }
        }
        c[k] = got;
    }
    // Batcher's odd-even merge sort of 8 (19 compare-exchanges); INF (no candidate) sorts last
    cswap(c[0], c[1]); cswap(c[2], c[3]); cswap(c[4], c[5]); cswap(c[6], c[7]);
    cswap(c[0], c[2]); cswap(c[1], c[3]); cswap(c[4], c[6]); cswap(c[5], c[7]);
    cswap(c[1], c[2]); cswap(c[5], c[6]);
    cswap(c[0], c[4]); cswap(c[1], c[5]); cswap(c[2], c[6]); cswap(c[3], c[7]);
    cswap(c[2], c[4]); cswap(c[3], c[5]);
    cswap(c[1], c[2]); cswap(c[3], c[4]); cswap(c[5], c[6]);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) k += c[i] != inf;
    float r;
    if (pass == 1) {
        r = k >= 2 ? c[1] : c[0];                                       // the background: second smallest
    } else {
        const int h = k >> 1;                                           // upper median; k == 0 leaves c[0] = INF
        r = c[0];
        r = h == 1 ? c[1] : r;
        r = h == 2 ? c[2] : r;
        r = h == 3 ? c[3] : r;
        r = h == 4 ? c[4] : r;
    }
    out[idx] = r;
}

extern "C" {

int sgmd_fill_classify(int ord, void* stream, const sgmd_geom* g, const void* ref, const void* oth, float thres, int right,
                       int do_check, void* cls)
{
    HIP_TRY(hipSetDevice(ord));
    const dim3 grid((g->W + 255) / 256, g->H, g->B);
    hipLaunchKernelGGL(sgm_fill_classify_k, grid, dim3(256), 0, (hipStream_t)stream, (const float*)ref, (const float*)oth,
                       (uint8_t*)cls, g->W, g->H, thres, right, do_check);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_fill_pass(int ord, void* stream, const sgmd_geom* g, int R, const void* in, void* out, const void* cls, int pass)
{
    if (pass < 1 || pass > 3 || (pass != 3 && !cls) || R < 1) {
        fprintf(stderr, "sgm_mi355x: sgmd_fill_pass: bad arguments (pass %d, R %d)\n", pass, R);
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const dim3 grid((g->W + 255) / 256, g->H, g->B);
    hipLaunchKernelGGL(sgm_fill_pass_k, grid, dim3(256), 0, (hipStream_t)stream, (const float*)in, (float*)out,
                       (const uint8_t*)cls, g->W, g->H, R, pass);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
