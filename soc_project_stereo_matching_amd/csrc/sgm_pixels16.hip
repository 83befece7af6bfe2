#include "sgm_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): images of 9..16 bits per sample.  The contract is
// written out in include/sgm_mi355x.h (SGM_SetPixelBits); tests/pixels16_ref.py restates it in numpy.
//
// The census is a rank transform: it is evaluated on the u16 samples as they are.  Everything below
// it reads census words, and the three readers of grey values (adaptive P2, the refinement's guide,
// the fused sweep's image copy) read the NARROWED image g8 = min(v >> (bits - 8), 255), which the
// census kernels write on the side: the thread that owns a pixel has its sample in LDS anyway, so no
// separate pass reads the image again.  A translation unit of its own: the 8-bit kernels of
// sgm_census.hip / sgm_rectify.hip compile to what they were.
//
// Blocks as in sgm_census_k: 64 x 16 pixels, z = 2 * frame + image, a thread owns one column of four
// consecutive rows.  The (64 + cw - 1) x (16 + ch - 1) samples a block needs are staged in LDS once.
// Global loads are single u16 loads, so an image needs its element's alignment and nothing more (a
// batch with W * H odd starts every other frame at an odd sample; so may a caller's pointer): there
// is no wider path that could give other results.  LDS rows are an even number of u16 apart, so a
// row starts on a bank; a wave reads ONE tile row per instruction (its 64 lanes are 64 adjacent
// columns, ds_read_u16 is banked (a / 4) % 32 per 32 lanes), i.e. 16 or 17 adjacent dwords with two
// lanes on each half of a dword: no two distinct dwords of a lane group meet on a bank whatever the
// stride is, which the 8-bit tiles (four lanes per dword) also had.
// ============================================================================================

#define C16_BW 64
#define C16_BH 16
#define C16_LDS 4992                                                    // u16 entries; the largest tile: 1 x 63, 64 columns x 78 rows

static __device__ __forceinline__ unsigned narrow8(unsigned v, int shift)
{
    return min(v >> shift, 255u);                                       // samples >= 2^bits saturate
}

// the block's tile: positions outside the image are clamped, only pixels of the zero border ever see them (tw <= 126)
static __device__ __forceinline__ void stage_tile16(uint16_t* tile, const uint16_t* __restrict__ img, int W, int H, int x0, int y0,
                                                    int rx, int ry, int tw, int th, int ld)
{
    const int c = threadIdx.x & 127;
    if (c < tw) {
        const int xx = min(max(x0 + c - rx, 0), W - 1);
        for (int r = threadIdx.x >> 7; r < th; r += 2) {
            const int yy = min(max(y0 + r - ry, 0), H - 1);
            tile[r * ld + c] = img[(size_t)yy * W + xx];
        }
    }
    __syncthreads();
}

// 5x5 centre census (ref :134-159 on u16 samples) -> u32; every word of the frame is written
#define C16_LD5 68                                                      // LDS row stride in u16 (68 used)
__global__ __launch_bounds__(256) void sgm_census16_k(const uint16_t* __restrict__ left, const uint16_t* __restrict__ right,
                                                      uint32_t* __restrict__ cl, uint32_t* __restrict__ cr,
                                                      uint8_t* __restrict__ gl, uint8_t* __restrict__ gr, int W, int H, int shift)
{
    __shared__ uint16_t tile[(C16_BH + 4) * C16_LD5];
    const size_t frame_px = (size_t)(blockIdx.z >> 1) * W * H;         // batch: z = 2 * frame + image
    const uint16_t* img = ((blockIdx.z & 1) ? right : left) + frame_px;
    uint32_t* out = ((blockIdx.z & 1) ? cr : cl) + frame_px;
    uint8_t* g8 = ((blockIdx.z & 1) ? gr : gl) + frame_px;
    const int x0 = blockIdx.x * C16_BW, y0 = blockIdx.y * C16_BH;
    // the 68 x 20 samples in 5.3 loads per thread, every lane busy (stage_tile16 would use 68 lanes of 128 here: 10 loads per
    // thread); positions outside the image are clamped, only the zero border sees them
    for (int t = threadIdx.x; t < (C16_BH + 4) * (C16_BW + 4); t += 256) {
        const int r = t / (C16_BW + 4), c = t % (C16_BW + 4);
        const int yy = min(max(y0 + r - 2, 0), H - 1), xx = min(max(x0 + c - 2, 0), W - 1);
        tile[r * C16_LD5 + c] = img[(size_t)yy * W + xx];
    }
    __syncthreads();
    const int cx = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int x = x0 + cx;
    if (x >= W) return;
    unsigned v[8][5];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 5; ++c) v[r][c] = tile[(rg * 4 + r) * C16_LD5 + cx + c];
    const bool col_ok = W > 5 && H > 5 && x >= 2 && x < W - 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + rg * 4 + i;
        if (y >= H) break;
        const unsigned centre = v[i + 2][2];
        uint32_t bits = 0;
        if (col_ok && y >= 2 && y < H - 2) {
#pragma unroll
            for (int r = 0; r < 5; ++r)
#pragma unroll
                for (int c = 0; c < 5; ++c) bits = (bits << 1) | (unsigned)(v[i + r][c] < centre);   // raster order, ref :146-154
        }
        out[(size_t)y * W + x] = bits;
        g8[(size_t)y * W + x] = (uint8_t)narrow8(centre, shift);
    }
}

// centre-symmetric census over any odd window (sgm_census_sym_k on u16 samples) -> u32
__global__ __launch_bounds__(256) void sgm_census16_sym_k(const uint16_t* __restrict__ left, const uint16_t* __restrict__ right,
                                                          uint32_t* __restrict__ cl, uint32_t* __restrict__ cr,
                                                          uint8_t* __restrict__ gl, uint8_t* __restrict__ gr, int W, int H, int cw,
                                                          int ch, int shift)
{
    __shared__ uint16_t tile[C16_LDS];
    const int rx = cw >> 1, ry = ch >> 1, n = (cw * ch - 1) >> 1;
    const int tw = C16_BW + cw - 1, th = C16_BH + ch - 1;              // tw <= 126
    const int ld = (tw + 1) & ~1;
    const size_t frame_px = (size_t)(blockIdx.z >> 1) * W * H;
    const uint16_t* img = ((blockIdx.z & 1) ? right : left) + frame_px;
    uint32_t* out = ((blockIdx.z & 1) ? cr : cl) + frame_px;
    uint8_t* g8 = ((blockIdx.z & 1) ? gr : gl) + frame_px;
    const int x0 = blockIdx.x * C16_BW, y0 = blockIdx.y * C16_BH;
    stage_tile16(tile, img, W, H, x0, y0, rx, ry, tw, th, ld);
    const int cx = threadIdx.x & 63, li = (threadIdx.x >> 6) * 4;
    const int x = x0 + cx;
    if (x >= W) return;
    uint32_t bits0 = 0, bits1 = 0, bits2 = 0, bits3 = 0;
    for (int c = -rx; c <= rx; ++c) {
        // pixel i of the thread (tile row li + i + ry), window row r = j - ry: a = tile row li + i + j of column c,
        // b = tile row li + i + 2 ry - j of column -c; both slide by one row per step
        const uint16_t* pa = tile + li * ld + (cx + rx + c);
        const uint16_t* pb = tile + (li + 2 * ry) * ld + (cx + rx - c);
        unsigned a0 = pa[0], a1 = pa[ld], a2 = pa[2 * ld];
        unsigned b1 = pb[ld], b2 = pb[2 * ld], b3 = pb[3 * ld];
        const int steps = c < 0 ? ry + 1 : ry;                         // the centre row stops in front of the centre
        int sh = n - 1 - (c + rx);                                     // raster order, first comparison in the highest bit
        for (int j = 0; j < steps; ++j, sh -= cw) {
            const unsigned a3 = pa[(j + 3) * ld], b0 = pb[-j * ld];
            bits0 |= (unsigned)(a0 < b0) << sh;
            bits1 |= (unsigned)(a1 < b1) << sh;
            bits2 |= (unsigned)(a2 < b2) << sh;
            bits3 |= (unsigned)(a3 < b3) << sh;
            a0 = a1; a1 = a2; a2 = a3;
            b3 = b2; b2 = b1; b1 = b0;
        }
    }
    const bool col_ok = W > cw && H > ch && x >= rx && x < W - rx;
    const uint32_t bits[4] = {bits0, bits1, bits2, bits3};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + li + i;
        if (y >= H) break;
        out[(size_t)y * W + x] = (col_ok && y >= ry && y < H - ry) ? bits[i] : 0u;
        g8[(size_t)y * W + x] = (uint8_t)narrow8(tile[(li + i + ry) * ld + cx + rx], shift);
    }
}

// wide centre census (sgm_census_window_k on u16 samples) -> u64.  For one window column the thread walks the ch + 3 tile rows its
// four pixels' windows cover: one LDS read serves up to four comparisons.
__global__ __launch_bounds__(256) void sgm_census16_window_k(const uint16_t* __restrict__ left, const uint16_t* __restrict__ right,
                                                             unsigned long long* __restrict__ cl, unsigned long long* __restrict__ cr,
                                                             uint8_t* __restrict__ gl, uint8_t* __restrict__ gr, int W, int H, int cw,
                                                             int ch, int shift)
{
    __shared__ uint16_t tile[C16_LDS];
    const int rx = cw >> 1, ry = ch >> 1, n = cw * ch;
    const int tw = C16_BW + cw - 1, th = C16_BH + ch - 1;
    const int ld = (tw + 1) & ~1;
    const size_t frame_px = (size_t)(blockIdx.z >> 1) * W * H;
    const uint16_t* img = ((blockIdx.z & 1) ? right : left) + frame_px;
    unsigned long long* out = ((blockIdx.z & 1) ? cr : cl) + frame_px;
    uint8_t* g8 = ((blockIdx.z & 1) ? gr : gl) + frame_px;
    const int x0 = blockIdx.x * C16_BW, y0 = blockIdx.y * C16_BH;
    stage_tile16(tile, img, W, H, x0, y0, rx, ry, tw, th, ld);
    const int cx = threadIdx.x & 63, li = (threadIdx.x >> 6) * 4;
    const int x = x0 + cx;
    if (x >= W) return;
    unsigned centre[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) centre[i] = tile[(li + i + ry) * ld + cx + rx];
    unsigned long long bits[4] = {0, 0, 0, 0};
    for (int c = 0; c < cw; ++c) {
        const uint16_t* p = tile + li * ld + cx + c;
        for (int rr = 0; rr < ch + 3; ++rr) {
            const unsigned v = p[rr * ld];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rr - i;                                  // window row of pixel i (uniform across the wave)
                if (r >= 0 && r < ch) bits[i] |= (unsigned long long)(v < centre[i]) << (n - 1 - (r * cw + c));   // raster order
            }
        }
    }
    const bool col_ok = W > cw && H > ch && x >= rx && x < W - rx;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + li + i;
        if (y >= H) break;
        out[(size_t)y * W + x] = (col_ok && y >= ry && y < H - ry) ? bits[i] : 0ull;
        g8[(size_t)y * W + x] = (uint8_t)narrow8(centre[i], shift);
    }
}

// ============================================================================================
// the remap of sgm_rectify.hip on u16 samples: same maps, taps and rounding; 1024 * 65535 + 512 < 2^32
// ============================================================================================

static __device__ __forceinline__ unsigned remap_pixel16(const uint16_t* __restrict__ src, int W, int H, int xq, int yq)
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
    return ((32u - ax) * (32u - ay) * p00 + ax * (32u - ay) * p01 + (32u - ax) * ay * p10 + ax * ay * p11 + 512u) >> 10;
}

// grid: x = groups of 4 pixels / 256, y = view (0 left, 1 right); the map entries of four pixels are read once for all B frames
__global__ __launch_bounds__(256) void sgm_remap16_k(const int32_t* __restrict__ maps, const uint16_t* __restrict__ left,
                                                     const uint16_t* __restrict__ right, uint16_t* __restrict__ out_left,
                                                     uint16_t* __restrict__ out_right, int W, int H, int B)
{
    const size_t N = (size_t)W * H, pitch = SGMD_REMAP_PITCH(N);
    const size_t p = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= N) return;
    const int view = blockIdx.y;
    const int32_t* m = maps + (size_t)view * 2 * pitch;
    const int4 xq = *reinterpret_cast<const int4*>(m + p);
    const int4 yq = *reinterpret_cast<const int4*>(m + pitch + p);
    const uint16_t* src = view ? right : left;
    uint16_t* dst = view ? out_right : out_left;
    const bool whole = p + 4 <= N;                                       // false for the last group of a frame with N % 4 != 0
    for (int f = 0; f < B; ++f, src += N, dst += N) {
        const unsigned v0 = remap_pixel16(src, W, H, xq.x, yq.x), v1 = remap_pixel16(src, W, H, xq.y, yq.y);
        const unsigned v2 = remap_pixel16(src, W, H, xq.z, yq.z), v3 = remap_pixel16(src, W, H, xq.w, yq.w);
        uint16_t* o = dst + p;
        const unsigned align = (unsigned)(uintptr_t)o & 7u;              // the same for every thread of the launch: p % 4 == 0
        if (whole && align == 0) {
            *reinterpret_cast<uint2*>(o) = make_uint2(v0 | (v1 << 16), v2 | (v3 << 16));
        } else if (whole && align == 4) {
            *reinterpret_cast<uint32_t*>(o) = v0 | (v1 << 16);
            *reinterpret_cast<uint32_t*>(o + 2) = v2 | (v3 << 16);
        } else {
            o[0] = (uint16_t)v0;
            if (p + 1 < N) o[1] = (uint16_t)v1;
            if (p + 2 < N) o[2] = (uint16_t)v2;
            if (p + 3 < N) o[3] = (uint16_t)v3;
        }
    }
}

extern "C" {

int sgmd_census16(int ord, void* stream, const sgmd_geom* g, int bits, int symmetric, int cw, int ch, const void* left,
                  const void* right, void* census_l, void* census_r, void* g8_left, void* g8_right)
{
    const bool odd = (((uintptr_t)left | (uintptr_t)right) & 1u) != 0;
    if (!left || !right || !census_l || !census_r || !g8_left || !g8_right || odd || bits < 9 || bits > 16 || g->W < 1 || g->H < 1 ||
        g->B < 1) {
        fprintf(stderr, "sgm_mi355x: sgmd_census16: bad arguments\n");
        return (int)hipErrorInvalidValue;
    }
    if (cw < 1 || ch < 1 || !(cw & 1) || !(ch & 1) || cw * ch > 64 || (C16_BH + ch - 1) * ((C16_BW + cw - 1 + 1) & ~1) > C16_LDS) {
        fprintf(stderr, "sgm_mi355x: the census needs an odd window of at most 64 pixels (got %dx%d)\n", cw, ch);
        return (int)hipErrorInvalidValue;
    }
    HIP_TRY(hipSetDevice(ord));
    const dim3 grid((g->W + C16_BW - 1) / C16_BW, (g->H + C16_BH - 1) / C16_BH, 2 * g->B);
    const int shift = bits - 8;
    const uint16_t *l = (const uint16_t*)left, *r = (const uint16_t*)right;
    if (symmetric)
        hipLaunchKernelGGL(sgm_census16_sym_k, grid, dim3(256), 0, (hipStream_t)stream, l, r, (uint32_t*)census_l, (uint32_t*)census_r,
                           (uint8_t*)g8_left, (uint8_t*)g8_right, g->W, g->H, cw, ch, shift);
    else if (cw == 5 && ch == 5)
        hipLaunchKernelGGL(sgm_census16_k, grid, dim3(256), 0, (hipStream_t)stream, l, r, (uint32_t*)census_l, (uint32_t*)census_r,
                           (uint8_t*)g8_left, (uint8_t*)g8_right, g->W, g->H, shift);
    else
        hipLaunchKernelGGL(sgm_census16_window_k, grid, dim3(256), 0, (hipStream_t)stream, l, r, (unsigned long long*)census_l,
                           (unsigned long long*)census_r, (uint8_t*)g8_left, (uint8_t*)g8_right, g->W, g->H, cw, ch, shift);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sgmd_remap16(int ord, void* stream, const sgmd_geom* g, const void* maps, const void* left, const void* right, void* out_left,
                 void* out_right)
{
    const bool odd = (((uintptr_t)left | (uintptr_t)right | (uintptr_t)out_left | (uintptr_t)out_right) & 1u) != 0;
    if (!maps || !left || !right || !out_left || !out_right || odd || g->W < 1 || g->H < 1 || g->B < 1) {
        fprintf(stderr, "sgm_mi355x: sgmd_remap16: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    const size_t groups = SGMD_REMAP_PITCH((size_t)g->W * g->H) / 4;
    const dim3 grid((unsigned)((groups + 255) / 256), 2);
    hipLaunchKernelGGL(sgm_remap16_k, grid, dim3(256), 0, (hipStream_t)stream, (const int32_t*)maps, (const uint16_t*)left,
                       (const uint16_t*)right, (uint16_t*)out_left, (uint16_t*)out_right, g->W, g->H, g->B);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
