/*
 * stub_pixels16.c -- TEST INFRASTRUCTURE ONLY (tests/test_pixels16_cpu.py builds it beside tests/stub_device.c).
 *
 * The stand-in for csrc/sgm_pixels16.hip: sgmd_census16 and sgmd_remap16, which csrc/sgm_host.c references weakly.  A host linked
 * without this file keeps to 8 bits per sample.  It keeps a log of its own (the launch log of stub_device.c stays what it is with
 * 8-bit input): the pointers and arguments of every call and where in stub_device.c's log the call fell, and it can be told to
 * refuse the n-th call.  While the buffers fit the allocator's cap of stub_device.c (1 MiB) both launchers compute for real, in
 * plain loops written from the header's text, so that a sanitizer build sees every sample, word and byte the product's kernels
 * would touch.  It also carries a stand-in for sgmd_census_sym (logged here as kind 2, computes nothing), so that the host accepts the
 * symmetric census kind, whose 16-bit form goes through sgmd_census16.
 */
#include "sgm_device.h"

#include <string.h>

int stub_log_size(void);                       /* stub_device.c */

#define P16_LOG_MAX 256
/* kind: 0 census16, 1 remap16, 2 the 8-bit symmetric census.  census16: p = left, right, census_l, census_r, g8_left, g8_right; remap16: p = maps, left, right,
 * out_left, out_right */
static struct { int kind, bits, symmetric, cw, ch, frames, at; const void* p[6]; } g_calls[P16_LOG_MAX];
static int g_calls_n, g_refuse_countdown = -1;

void stub_p16_clear(void) { g_calls_n = 0; g_refuse_countdown = -1; }
int stub_p16_count(void) { return g_calls_n; }
const void* stub_p16_ptr(int call, int which) { return (call >= 0 && call < g_calls_n && which >= 0 && which < 6) ? g_calls[call].p[which] : NULL; }
/* field: 0 kind, 1 bits, 2 symmetric, 3 cw, 4 ch, 5 frames, 6 size of stub_device.c's log when the call came */
int stub_p16_arg(int call, int field)
{
    if (call < 0 || call >= g_calls_n) return -1;
    const int v[7] = {g_calls[call].kind, g_calls[call].bits, g_calls[call].symmetric, g_calls[call].cw, g_calls[call].ch, g_calls[call].frames,
                      g_calls[call].at};
    return (field >= 0 && field < 7) ? v[field] : -1;
}
/* the nth (0-based) call of either launcher from now on returns an error */
void stub_p16_fail_at(int nth) { g_refuse_countdown = nth; }

static int note16(int kind, int bits, int symmetric, int cw, int ch, int frames, const void* const* p, int n)
{
    if (g_calls_n < P16_LOG_MAX) {
        memset(&g_calls[g_calls_n], 0, sizeof g_calls[0]);
        g_calls[g_calls_n].kind = kind; g_calls[g_calls_n].bits = bits; g_calls[g_calls_n].symmetric = symmetric;
        g_calls[g_calls_n].cw = cw; g_calls[g_calls_n].ch = ch; g_calls[g_calls_n].frames = frames; g_calls[g_calls_n].at = stub_log_size();
        memcpy(g_calls[g_calls_n].p, p, (size_t)n * sizeof *p);
        ++g_calls_n;
    }
    if (g_refuse_countdown >= 0 && g_refuse_countdown-- == 0) return 719;
    return 0;
}

int sgmd_census16(int o, void* st, const sgmd_geom* g, int bits, int symmetric, int cw, int ch, const void* left, const void* right,
                  void* census_l, void* census_r, void* g8_left, void* g8_right)
{
    (void)o; (void)st;
    const void* p[6] = {left, right, census_l, census_r, g8_left, g8_right};
    const int rc = note16(0, bits, symmetric, cw, ch, g->B, p, 6);
    if (rc != 0) return rc;
    const int W = g->W, H = g->H, rx = cw / 2, ry = ch / 2;
    const size_t n = (size_t)W * H, all = n * (size_t)g->B;
    const int wide = !symmetric && !(cw == 5 && ch == 5);                  /* u64 words */
    if (all * 8 > (1u << 20)) return 0;
    for (int view = 0; view < 2; ++view)
        for (int f = 0; f < g->B; ++f) {
            const uint16_t* img = (const uint16_t*)(view ? right : left) + (size_t)f * n;
            uint8_t* g8 = (uint8_t*)(view ? g8_right : g8_left) + (size_t)f * n;
            uint32_t* w32 = (uint32_t*)(view ? census_r : census_l) + (size_t)f * n;
            uint64_t* w64 = (uint64_t*)(view ? census_r : census_l) + (size_t)f * n;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const unsigned v = img[(size_t)y * W + x], narrowed = v >> (bits - 8);
                    g8[(size_t)y * W + x] = (uint8_t)(narrowed > 255u ? 255u : narrowed);
                    uint64_t word = 0;
                    if (W > cw && H > ch && x >= rx && x < W - rx && y >= ry && y < H - ry) {
                        int left_to_do = symmetric ? (cw * ch - 1) / 2 : cw * ch;
                        for (int r = -ry; r <= ry && left_to_do; ++r)
                            for (int c = -rx; c <= rx && left_to_do; ++c, --left_to_do) {
                                const unsigned a = img[(size_t)(y + r) * W + (x + c)];
                                const unsigned b = symmetric ? img[(size_t)(y - r) * W + (x - c)] : v;
                                word = (word << 1) | (uint64_t)(a < b);
                            }
                    }
                    if (wide) w64[(size_t)y * W + x] = word;
                    else w32[(size_t)y * W + x] = (uint32_t)word;
                }
        }
    return 0;
}

int sgmd_census_sym(int o, void* st, const sgmd_geom* g, int cw, int ch, const void* left, const void* right, void* census_l, void* census_r,
                    const void* need)
{
    (void)o; (void)st; (void)need;
    const void* p[4] = {left, right, census_l, census_r};
    return note16(2, 8, 1, cw, ch, g->B, p, 4);
}

static unsigned tap16(const uint16_t* src, int W, int H, int y, int x)
{
    return (y >= 0 && y < H && x >= 0 && x < W) ? src[(size_t)y * W + x] : 0u;
}

int sgmd_remap16(int o, void* st, const sgmd_geom* g, const void* maps, const void* left, const void* right, void* out_left, void* out_right)
{
    (void)o; (void)st;
    const void* p[5] = {maps, left, right, out_left, out_right};
    const int rc = note16(1, 0, 0, 0, 0, g->B, p, 5);
    if (rc != 0) return rc;
    const size_t n = (size_t)g->W * g->H, pitch = SGMD_REMAP_PITCH(n);
    if (4 * pitch * sizeof(int32_t) > (1u << 20) || 2 * n * (size_t)g->B > (1u << 20)) return 0;
    for (int view = 0; view < 2; ++view) {
        const int32_t* xq = (const int32_t*)maps + (size_t)view * 2 * pitch;
        const int32_t* yq = xq + pitch;
        for (int f = 0; f < g->B; ++f) {
            const uint16_t* src = (const uint16_t*)(view ? right : left) + (size_t)f * n;
            uint16_t* dst = (uint16_t*)(view ? out_right : out_left) + (size_t)f * n;
            for (size_t q = 0; q < n; ++q) {
                const int x0 = xq[q] >> 5, y0 = yq[q] >> 5;
                const unsigned ax = (unsigned)xq[q] & 31u, ay = (unsigned)yq[q] & 31u;
                dst[q] = (uint16_t)(((32 - ax) * (32 - ay) * tap16(src, g->W, g->H, y0, x0) + ax * (32 - ay) * tap16(src, g->W, g->H, y0, x0 + 1) +
                                     (32 - ax) * ay * tap16(src, g->W, g->H, y0 + 1, x0) + ax * ay * tap16(src, g->W, g->H, y0 + 1, x0 + 1) + 512u) >> 10);
            }
        }
    }
    return 0;
}
