#include "sgm_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): rectification of raw camera pairs ahead of the
// match.  The contract is written out in include/sgm_mi355x.h (SGM_SetRectify);
// tests/rectify_ref.py restates it in numpy.
//
// One launch rectifies both views of all B frames.  The bytes decide the layout: a map entry is
// 8 B per pixel and view (xq, yq as int32, quantised to 1/32 pixel by the host), a pixel is 1 B in
// and 1 B out per frame -- so a thread reads the entries of four adjacent pixels ONCE (two 16-byte
// loads from the xq and the yq plane) and walks the B frames with them in registers: the maps cost
// 2 x 8 B x W x H per batch instead of per frame.  The four outputs of a frame leave as one dword
// where the frame's offset allows it.  The taps are byte gathers; rectification maps are smooth, so
// the 16 taps of a thread and those of its neighbours fall into a few cache lines of two or three
// image rows.
//
// Pixels are addressed by their linear index p = y * W + x: the map planes are padded to a multiple
// of four entries (SGMD_REMAP_PITCH, the padding holds the "outside" entry), so every 16-byte load
// is aligned and in bounds whatever W is, and rows need no special case.
// ============================================================================================

// one output pixel: the four taps around (yq, xq) / 32, 0 outside the frame (decided per tap), weights in 1/32
static __device__ __forceinline__ unsigned remap_pixel(const uint8_t* __restrict__ src, int W, int H, int xq, int yq)
{
    const int x0 = xq >> 5, y0 = yq >> 5;
    const unsigned ax = (unsigned)xq & 31u, ay = (unsigned)yq & 31u;
    const bool r0 = (unsigned)y0 < (unsigned)H, r1 = (unsigned)(y0 + 1) < (unsigned)H;
    const bool c0 = (unsigned)x0 < (unsigned)W, c1 = (unsigned)(x0 + 1) < (unsigned)W;
    // an index is formed only for a tap inside the frame: y0 * W of an entry far outside does not fit 32 bits
    const unsigned p00 = (r0 && c0) ? src[(size_t)y0 * W + x0] : 0u;
    const unsigned p01 = (r0 && c1) ? src[(size_t)y0 * W + (x0 + 1)] : 0u;
    const unsigned p10 = (r1 && c0) ? src[(size_t)(y0 + 1) * W + x0] : 0u;
    const unsigned p11 = (r1 && c1) ? src[(size_t)(y0 + 1) * W + (x0 + 1)] : 0u;
    // at most 1024 * 255 + 512
    return ((32u - ax) * (32u - ay) * p00 + ax * (32u - ay) * p01 + (32u - ax) * ay * p10 + ax * ay * p11 + 512u) >> 10;
}

// grid: x = groups of 4 pixels / 256, y = view (0 left, 1 right)
__global__ __launch_bounds__(256) void sgm_remap_k(const int32_t* __restrict__ maps, const uint8_t* __restrict__ left,
                                                   const uint8_t* __restrict__ right, uint8_t* __restrict__ out_left,
                                                   uint8_t* __restrict__ out_right, int W, int H, int B)
{
    const size_t N = (size_t)W * H, pitch = SGMD_REMAP_PITCH(N);
    const size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;       // first of this thread's four pixels
    if (p >= N) return;
    const int view = blockIdx.y;
    const int32_t* m = maps + (size_t)view * 2 * pitch;
    const int4 xq = *reinterpret_cast<const int4*>(m + p);
    const int4 yq = *reinterpret_cast<const int4*>(m + pitch + p);
    const uint8_t* src = view ? right : left;
    uint8_t* dst = view ? out_right : out_left;
    const bool whole = p + 4 <= N;                                       // false for the last group of a frame with N % 4 != 0
    for (int f = 0; f < B; ++f, src += N, dst += N) {
        const unsigned v0 = remap_pixel(src, W, H, xq.x, yq.x), v1 = remap_pixel(src, W, H, xq.y, yq.y);
        const unsigned v2 = remap_pixel(src, W, H, xq.z, yq.z), v3 = remap_pixel(src, W, H, xq.w, yq.w);
        uint8_t* o = dst + p;
        const unsigned align = (unsigned)(uintptr_t)o & 3u;              // the same for every thread of the launch: p % 4 == 0
        if (whole && align == 0) {
            *reinterpret_cast<uint32_t*>(o) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
        } else if (whole && align == 2) {
            *reinterpret_cast<uint16_t*>(o) = (uint16_t)(v0 | (v1 << 8));
            *reinterpret_cast<uint16_t*>(o + 2) = (uint16_t)(v2 | (v3 << 8));
        } else {
            o[0] = (uint8_t)v0;
            if (p + 1 < N) o[1] = (uint8_t)v1;
            if (p + 2 < N) o[2] = (uint8_t)v2;
            if (p + 3 < N) o[3] = (uint8_t)v3;
        }
    }
}

extern "C" {

int sgmd_remap(int ord, void* stream, const sgmd_geom* g, const void* maps, const void* left, const void* right, void* out_left,
               void* out_right)
{
    if (!maps || !left || !right || !out_left || !out_right || g->W < 1 || g->H < 1 || g->B < 1) {
        fprintf(stderr, "sgm_mi355x: sgmd_remap: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const size_t groups = SGMD_REMAP_PITCH((size_t)g->W * g->H) / 4;
    const dim3 grid((unsigned)((groups + 255) / 256), 2);
    hipLaunchKernelGGL(sgm_remap_k, grid, dim3(256), 0, (hipStream_t)stream, (const int32_t*)maps, (const uint8_t*)left,
                       (const uint8_t*)right, (uint8_t*)out_left, (uint8_t*)out_right, g->W, g->H, g->B);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
