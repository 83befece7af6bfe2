#include "sgm_common.hpp"

// ============================================================================================
// Extension (parity unpinned by the reference): confidence-guided edge-aware refinement of the
// disparity map, the Fast Global Smoother of Min et al. (2014).  The contract is written out in
// include/sgm_mi355x.h (sgm_set_refine); tests/refine_ref.py restates it in numpy.
//
// One lane per line: a lane walks the Thomas recurrence of its row (horizontal pass) or column
// (vertical pass) in exactly the contract's order, so the result is bit-exact.  U and V (the two
// right-hand sides, sharing m and q) are solved in place; q_i goes to the scratch map Q between the
// forward and the backward sweep.  Lines end at the frame edges; the maps are [B][H][W], so the
// B*H rows of a batch are simply consecutive rows.
//
//   horizontal  one wave = 64 consecutive rows.  Each 32-column slab goes through LDS: the wave
//               loads it with 128-byte row pieces, then every lane walks its own row of the slab
//               (a 64 x 33 tile: lane r reads bank (r + col) % 32, no conflict), then the slab is
//               written back the same way.  The first pass of the refinement builds U and V from
//               the disparity map and the confidence on the fly.
//   vertical    one lane per column of a frame: every step's loads and stores are coalesced.  The
//               last pass of the refinement writes out = U / V (masked) instead of U and V.
// The serial chain per step is a multiply, a subtract and a correctly rounded divide (three
// divides per step, the two of U and V independent of each other): the passes are latency-bound.
// ============================================================================================

namespace {

constexpr int kLines = 64;      // lines per wave (= workgroup) of the horizontal pass
constexpr int kSlab = 32;       // columns per LDS slab of the horizontal pass
constexpr int kPad = kSlab + 1; // LDS row stride in floats

struct RefineTable {
    float L[256];               // L_t[k] of this iteration (host-computed, include/sgm_mi355x.h step 2)
};

__device__ __forceinline__ float edge_weight(const float* lut, int g0, int g1) { return lut[g0 > g1 ? g0 - g1 : g1 - g0]; }

// step 1 of the contract: c, U = c * D (0 where D is +INF), V = c
__device__ __forceinline__ void data_term(float d, uint16_t k, float& u, float& v)
{
    const bool ok = d != __builtin_inff();
    const float c = ok ? (float)k / 65535.0f : 0.0f;
    u = ok ? c * d : 0.0f;
    v = c;
}

// horizontal pass (rows of all B frames).  first: U and V come from disp / conf (step 1) instead of U / V.
__global__ __launch_bounds__(kLines) void sgm_refine_rows_k(RefineTable tab, const uint8_t* __restrict__ guide,
                                                            const float* __restrict__ disp, const uint16_t* __restrict__ conf,
                                                            float* __restrict__ U, float* __restrict__ V, float* __restrict__ Q,
                                                            int W, int rows, int first)
{
    __shared__ float lut[256];
    __shared__ float tq[kLines * kPad], tu[kLines * kPad], tv[kLines * kPad];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += kLines) lut[k] = tab.L[k];
    const int row0 = blockIdx.x * kLines;
    const int my_row = row0 + lane;
    const bool live = my_row < rows;
    // cooperative slab access: element j = i * 64 + lane of the 64 x 32 slab is row j / 32, column j % 32
    const int cr = lane >> 5, cc = lane & 31;

    // ---- forward sweep, slabs left to right
    float a = 0.0f, q = 0.0f, ru = 0.0f, rv = 0.0f;       // e_{i-1}, q_{i-1}, r'_{i-1} of U and V
    for (int x0 = 0; x0 < W; x0 += kSlab) {
        __syncthreads();                                  // the previous slab's stores have read the tiles
        const int x = x0 + cc;
#pragma unroll 4
        for (int i = 0; i < kLines * kSlab / 64; ++i) {
            const int r = i * 2 + cr, gr = row0 + r;
            float e = 0.0f, u = 0.0f, v = 0.0f;
            if (gr < rows && x < W) {
                const size_t idx = (size_t)gr * W + x;
                if (x + 1 < W) e = edge_weight(lut, guide[idx], guide[idx + 1]);
                if (first) data_term(disp[idx], conf[idx], u, v);
                else { u = U[idx]; v = V[idx]; }
            }
            tq[r * kPad + cc] = e;                        // e_i, replaced by q_i in the walk
            tu[r * kPad + cc] = u;
            tv[r * kPad + cc] = v;
        }
        __syncthreads();
        if (live) {
            const int n = min(kSlab, W - x0);
            float* pq = tq + lane * kPad;
            float* pu = tu + lane * kPad;
            float* pv = tv + lane * kPad;
            int j = 0;
            if (x0 == 0) {                                // i = 0: m_0 = b_0, r'_0 = r_0 / m_0
                const float c = pq[0];
                const float m = (1.0f + 0.0f) + c;
                q = c / m;
                ru = pu[0] / m;
                rv = pv[0] / m;
                pq[0] = q; pu[0] = ru; pv[0] = rv;
                a = c;
                j = 1;
            }
            for (; j < n; ++j) {
                const float c = pq[j];
                const float b = (1.0f + a) + c;
                const float m = b - a * q;
                const float nu = pu[j] + a * ru;
                const float nv = pv[j] + a * rv;
                q = c / m;
                ru = nu / m;
                rv = nv / m;
                pq[j] = q; pu[j] = ru; pv[j] = rv;
                a = c;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < kLines * kSlab / 64; ++i) {
            const int r = i * 2 + cr, gr = row0 + r;
            if (gr < rows && x < W) {
                const size_t idx = (size_t)gr * W + x;
                Q[idx] = tq[r * kPad + cc];
                U[idx] = tu[r * kPad + cc];
                V[idx] = tv[r * kPad + cc];
            }
        }
    }

    // ---- backward sweep, slabs right to left: x_{n-1} = r'_{n-1}, x_i = r'_i + q_i * x_{i+1}
    float xu = 0.0f, xv = 0.0f;
    const int last0 = (W - 1) / kSlab * kSlab;
    for (int x0 = last0; x0 >= 0; x0 -= kSlab) {
        __syncthreads();
        const int x = x0 + cc;
#pragma unroll 4
        for (int i = 0; i < kLines * kSlab / 64; ++i) {
            const int r = i * 2 + cr, gr = row0 + r;
            if (gr < rows && x < W) {
                const size_t idx = (size_t)gr * W + x;
                tq[r * kPad + cc] = Q[idx];
                tu[r * kPad + cc] = U[idx];
                tv[r * kPad + cc] = V[idx];
            }
        }
        __syncthreads();
        if (live) {
            const int n = min(kSlab, W - x0);
            float* pq = tq + lane * kPad;
            float* pu = tu + lane * kPad;
            float* pv = tv + lane * kPad;
            int j = n - 1;
            if (x0 == last0) {                            // the line's last sample
                xu = pu[j];
                xv = pv[j];
                --j;
            }
            for (; j >= 0; --j) {
                const float qq = pq[j];
                xu = pu[j] + qq * xu;
                xv = pv[j] + qq * xv;
                pu[j] = xu; pv[j] = xv;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < kLines * kSlab / 64; ++i) {
            const int r = i * 2 + cr, gr = row0 + r;
            if (gr < rows && x < W) {
                const size_t idx = (size_t)gr * W + x;
                U[idx] = tu[r * kPad + cc];
                V[idx] = tv[r * kPad + cc];
            }
        }
    }
}

// vertical pass (columns of each frame; blockIdx.y = frame).  last: out = V > 0 ? U / V : +INF (step 5), and with keep_invalid
// +INF where out (= the input map D, read before it is written) was +INF.
__global__ __launch_bounds__(256) void sgm_refine_cols_k(RefineTable tab, const uint8_t* __restrict__ guide,
                                                         float* __restrict__ U, float* __restrict__ V, float* __restrict__ Q,
                                                         float* __restrict__ out, int W, int H, int last, int keep_invalid)
{
    __shared__ float lut[256];
    for (int k = threadIdx.x; k < 256; k += 256) lut[k] = tab.L[k];
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const size_t fo = (size_t)blockIdx.y * W * H + x;
    const uint8_t* g = guide + fo;
    float* u = U + fo;
    float* v = V + fo;
    float* qs = Q + fo;

    // forward sweep, top to bottom
    int g0 = g[0];
    float a = 0.0f, q, ru, rv;
    {
        const int g1 = H > 1 ? g[W] : g0;
        const float c = H > 1 ? edge_weight(lut, g0, g1) : 0.0f;
        const float m = (1.0f + 0.0f) + c;
        q = c / m;
        ru = u[0] / m;
        rv = v[0] / m;
        qs[0] = q; u[0] = ru; v[0] = rv;
        a = c;
        g0 = g1;
    }
#pragma unroll 4
    for (int y = 1; y < H; ++y) {
        const size_t o = (size_t)y * W;
        const float c = y + 1 < H ? edge_weight(lut, g0, g[o + W]) : 0.0f;
        if (y + 1 < H) g0 = g[o + W];
        const float b = (1.0f + a) + c;
        const float m = b - a * q;
        const float nu = u[o] + a * ru;
        const float nv = v[o] + a * rv;
        q = c / m;
        ru = nu / m;
        rv = nv / m;
        qs[o] = q; u[o] = ru; v[o] = rv;
        a = c;
    }

    // backward sweep, bottom to top
    const float inf = __builtin_inff();
    float* po = out + fo;
    float xu = ru, xv = rv;                               // x_{H-1} = r'_{H-1}
    for (int y = H - 1; y >= 0; --y) {
        const size_t o = (size_t)y * W;
        if (y < H - 1) {
            const float qq = qs[o];
            xu = u[o] + qq * xu;
            xv = v[o] + qq * xv;
        }
        if (last) {
            const float r = xv > 0.0f ? xu / xv : inf;
            po[o] = (keep_invalid && po[o] == inf) ? inf : r;
        } else {
            u[o] = xu;
            v[o] = xv;
        }
    }
}

}  // namespace

extern "C" {

int sgmd_refine_pass(int ord, void* stream, const sgmd_geom* g, int vertical, const float* table, const void* guide,
                     const void* disp, const void* conf, void* U, void* V, void* Q, int first, int last, int keep_invalid,
                     void* out)
{
    if (!table || !guide || !U || !V || !Q || (first && (vertical || !disp || !conf)) || (last && (!vertical || !out))) {
        fprintf(stderr, "sgm_mi355x: sgmd_refine_pass: bad arguments\n");
        return -1;
    }
    HIP_TRY(hipSetDevice(ord));
    RefineTable tab;
    memcpy(tab.L, table, sizeof tab.L);
    if (!vertical) {
        const int rows = g->B * g->H;
        hipLaunchKernelGGL(sgm_refine_rows_k, dim3((rows + kLines - 1) / kLines), dim3(kLines), 0, (hipStream_t)stream, tab,
                           (const uint8_t*)guide, (const float*)disp, (const uint16_t*)conf, (float*)U, (float*)V, (float*)Q,
                           g->W, rows, first);
    } else {
        hipLaunchKernelGGL(sgm_refine_cols_k, dim3((g->W + 255) / 256, g->B), dim3(256), 0, (hipStream_t)stream, tab,
                           (const uint8_t*)guide, (float*)U, (float*)V, (float*)Q, (float*)out, g->W, g->H, last, keep_invalid);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
