/*
 * sgm_mi355x.h -- C-ABI of libsgm_mi355x.so, the MI355X (gfx950) drop-in for the reference's
 * Semi-Global-Matching library.
 *
 * Part 1 is the reference boundary itself: the same three entry points with the same SGMOption
 * layout, argument meaning and error behaviour as
 *   /root/reference/SemiGlobalMatching/SemiGlobalMatching/SemiGlobalMatching.h:24-40 (SGMOption)
 *   /root/reference/SemiGlobalMatching/SemiGlobalMatching/SemiGlobalMatching.h:78-80 (functions)
 * so a caller such as the reference's main.c:72,83 links against this library unchanged.
 *
 * Part 2 are extensions the reference does not have (device-resident buffers, several
 * independent instances, stage read-back for parity tests).  Plain C types only.
 *
 * Results: disparity in pixels with sub-pixel fraction, invalid = +INFINITY
 * (SemiGlobalMatching.h:12), bit-identical to the reference's C code for every defined input
 * (see DESIGN.md "Parity contract" for the one undefined behaviour of the reference that is
 * defined here).
 */
#ifndef SGM_MI355X_H
#define SGM_MI355X_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Part 1 -- the reference boundary
 * ---------------------------------------------------------------------------------------- */

/* replaces SemiGlobalMatching.h:24-40; 28 bytes, align 4 on x86-64 SysV */
typedef struct {
    uint8_t  num_paths;          /* ignored by the reference (always 8 directions); see SGM_SetHonorNumPaths */
    uint16_t min_disparity;
    uint16_t max_disparity;      /* search range is [min_disparity, max_disparity) */

    bool     is_check_unique;
    float    uniqueness_ratio;

    bool     is_check_lr;
    float    lrcheck_thres;

    bool     is_remove_speckles;
    uint16_t min_speckle_area;

    int16_t  p1;
    int16_t  p2_init;
} SGMOption;

/* replaces SemiGlobalMatching.h:78 / SemiGlobalMatching.c:37-66.
 * false for width==0, height==0, max_disparity<=min_disparity (as the reference) and, in addition,
 * when no gfx950 device is usable, a HIP call fails, or the disparity range exceeds
 * SGM_MAX_DISPARITY_RANGE (the reason is printed to stderr).  Sizes device buffers for this
 * shape and marks the aggregated-cost volume as zero.
 * Admitted: width and height up to 65535 each with width * height < 2^31, min_disparity up to
 * 65535 - D, and a padded volume width * height * Dp < 2^32 - 1 cells (Dp = D rounded up to 32, 64,
 * 128, 192, 256 or 512); anything beyond is refused.  Also refused: a frame whose per-row table of
 * anomalous-line visits, [height][cap] with cap = the most visits of one row, would pass 2^24
 * entries.  With eight paths that is width == 1 with height > 4096 only (two diagonal lines stay on
 * one row there, cap = height or height + 1; no other width has cap > 6): 1 x 4096 is accepted,
 * 1 x 4097 is not.  tests/test_gpu_limits.py runs every kernel at these ends (DESIGN.md section 2
 * has the table).
 * One deviation past 32768 columns or rows: the reference's RemoveSpeckles keeps neighbour
 * coordinates in int16_t (SemiGlobalMatching.c:618-620), so a neighbour in a column or row >= 32768
 * wraps negative and is rejected, and components are cut there.  This library (and the CPU oracle)
 * grows whole components at every size; up to 32768 x 32768 the two are the same. */
bool SGM_Initialize(uint16_t width, uint16_t height, const SGMOption* option);

/* replaces SemiGlobalMatching.h:79 / SemiGlobalMatching.c:128-132 (clear + Initialize). */
bool SGM_Reset(uint16_t width, uint16_t height, const SGMOption* option);

/* replaces SemiGlobalMatching.h:80 / SemiGlobalMatching.c:68-125.
 * img_left/img_right: host pointers, row-major uint8, stride = width, borrowed for the call.
 * disp_left: host pointer to width*height floats, fully overwritten.  Blocking.
 * false if not initialised or an image pointer is NULL (as the reference) or a HIP call failed.
 * Like the reference a second SGM_Match without SGM_Reset accumulates onto the
 * aggregated costs of the previous frame; call SGM_Reset per frame. */
bool SGM_Match(const uint8_t* img_left, const uint8_t* img_right, float* disp_left);

/* ------------------------------------------------------------------------------------------
 * Part 2 -- extensions
 * ---------------------------------------------------------------------------------------- */

#define SGM_MAX_DISPARITY_RANGE 512

/* The default instance used by Part 1 can be moved to another GPU of the node before
 * SGM_Initialize (default: device 0, or the SGM_DEVICE environment variable). */
bool SGM_SetDevice(int device_ordinal);

/* 0 (default) = reference behaviour: num_paths is ignored, all 8 directions run.
 * 1 = num_paths == 4 runs only the first four directions of SemiGlobalMatching.c:213-216.
 * Takes effect at the next SGM_Initialize / SGM_Reset. */
void SGM_SetHonorNumPaths(int honor);

/* Two options the reference does not have.  Neither is pinned by the reference: the CPU oracle
 * (oracle/sgm_oracle.c) defines them, "parity unpinned by the reference".  Both take effect at the next SGM_Initialize /
 * SGM_Reset; the defaults are the reference's behaviour.
 *   census window: any odd width x height of at most 64 pixels (e.g. 7x7, 9x7) instead of SemiGlobalMatching.c:134-159's
 *     5x5 -- same bit order (raster, first comparison in the highest bit, centre included), border of width/2 columns
 *     and height/2 rows zero, off-image cost 127.  Wide windows take the materialised-cost path (u64 census words, cost
 *     volume, volume-fed aggregation kernels): correct, but not the fused fast path of 5x5 (SGM_SetCensusKind below has a
 *     wide-window census that is).
 *   reference view: 1 = the result is the RIGHT image's disparity map (the right-view winner-take-all of
 *     SemiGlobalMatching.c:395-408), validated by the mirror image of LRCheck (.c:445-470: right pixel x with disparity d
 *     must agree with the left map at column x + d), then speckle removal and median as usual.  0 = left (reference). */
bool SGM_SetCensusWindow(int width, int height);
void SGM_SetReferenceView(int right);

/* Census kind (extension, "parity unpinned by the reference": the reference has the centre census only; defined here and restated
 * by tests/census_sym_ref.py).  SGM_CENSUS_CENTRE (default) compares every pixel of the window with the centre pixel, so all of
 * its bits share one noisy sample.  SGM_CENSUS_SYMMETRIC is the centre-symmetric census (Spangenberg et al. 2013): it compares
 * the pixel pairs mirrored through the centre.  For the window cw x ch of SGM_SetCensusWindow (odd, cw * ch <= 64; the
 * reference's 5x5 when none was set), rx = cw / 2, ry = ch / 2, n = (cw * ch - 1) / 2:
 *   walk the window offsets (r, c) in raster order (r = -ry..ry outer, c = -rx..rx inner) and take the first n of them, those
 *   strictly before the centre; for each, bits = (bits << 1) | (I[y + r][x + c] < I[y - r][x - c])   (strict, as the centre census).
 *   u32 words of n <= 31 bits: 5x5 gives 12, 7x7 gives 24, 9x7 gives 31.  Pixels within rx columns or ry rows of the frame edge
 *   get 0, and every pixel gets 0 when !(W > cw && H > ch).  Every word of the frame is written on every match (the default
 *   instance's stale-border behaviour, SURVEY.md Q3, belongs to the reference's 5x5 centre census only).
 *   The cost is popcount(cl ^ cr), 127 off the image; everything downstream is exactly the path of the reference's 5x5.
 * Because the words are u32 for ANY window, the symmetric kind takes the fast path whatever its window: the cost is recomputed
 * inside the fused aggregation, no u64 words and no cost volume exist (stage 0 / 1 read back u32, stage 2 needs sgm_keep_stages),
 * and batches, four-path mode, negative P1, the right reference view, SGM_MatchBoth, the confidence, hole filling, the
 * refinement, matches without Reset, row tiles and sgm_match_planes compose as they do with 5x5.  Only the opt-in fused last
 * sweep (SGM_UPSUM) is not used.  Takes effect at the next SGM_Initialize / SGM_Reset; the default instance remembers it across
 * SGM_Shutdown, as it does the window.  Returns false and changes nothing for any other kind, or for SGM_CENSUS_SYMMETRIC in a
 * build without the kernel.  Timing: the kernel counts toward "census"; "cost" stays empty.
 * SGM_CENSUS_SYMMETRIC_DEFAULT_W / _H: the window the drivers use with the symmetric kind when none is given -- under sensor
 * noise (sigma = 4 grey levels) 7x7 has the lowest bad-pixel rate on the four image pairs the reference ships (NOTES.md). */
enum { SGM_CENSUS_CENTRE = 0, SGM_CENSUS_SYMMETRIC = 1 };
#define SGM_CENSUS_SYMMETRIC_DEFAULT_W 7
#define SGM_CENSUS_SYMMETRIC_DEFAULT_H 7
bool SGM_SetCensusKind(int kind);

/* Hole filling (extension, "parity unpinned by the reference": SemiGlobalMatching.h:24-40 has no such option; defined here
 * and restated by tests/fill_holes_ref.py).  The discontinuity-preserving interpolation of Hirschmueller's SGM paper: the
 * pixels the LR check, the uniqueness test and speckle removal leave +INF get a disparity from their neighbourhood, occluded
 * pixels from the background.  Off by default (every launch, buffer and result is then the reference's); takes effect at the
 * next SGM_Initialize / sgm_initialize / SGM_Reset / sgm_reset, which return false in row-tile mode (sgm_set_rows) with it on.
 * INF = +INFINITY; ref = the reference view's map after WTA (stage 4, or 5 with the right view), oth = the other view's; R =
 * option.max_disparity.
 *   1. Classes (stage 18, u8 [H][W]), from ref and oth BEFORE the LR check: 0 valid, 1 occluded, 2 mismatched; all 0 when
 *      is_check_lr is off.  Left view, pixel x of row y, d = ref[y][x]: d == INF -> 2; else xr = (int)((double)((float)x - d)
 *      + 0.5) (the LR check's own rounding); xr outside [0, W) -> 2; else r = oth[y][xr]: r == INF -> 0; |d - r| >
 *      lrcheck_thres -> xl = (int)((double)((float)xr + r) + 0.5), class 1 if 0 <= xl < W and ref[y][xl] > d (INF included),
 *      else 2; otherwise 0.  Right view: the mirror image (x + d, then xl - l).  Class != 0 exactly where the LR check
 *      leaves +INF.
 *   2. Filling, on the map after speckle removal, before the median: three Jacobi passes (each reads the map as it was when
 *      the pass started) -- pass 1 the INF pixels of class 1, pass 2 the INF pixels of class 2, pass 3 every pixel still INF.
 *      A target walks each of the 8 directions (+-1,0), (0,+-1), (+-1,+-1) for m = 1..R steps, stopping at the frame edge
 *      or at the first finite value, which it collects.  k <= 8 candidates sorted ascending s[]: k == 0 stays INF; pass 1
 *      takes s[1] if k >= 2 else s[0] (the background), passes 2 and 3 take s[k/2].  Compares and selects only: exact.
 *   3. The median runs unchanged on the filled map.
 * Timing: the classification counts toward "lrcheck", the three passes toward "speckle". */
bool SGM_SetFillHoles(int enable);

/* Matching confidence (extension, "parity unpinned by the reference": SemiGlobalMatching.c:380-426 computes min_cost and
 * sec_min_cost of every pixel but never exposes them; defined here and restated by tests/confidence_ref.py).
 * For each pixel of the REFERENCE view take the aggregated costs S after this match's cost sum (the Q14 accumulation of a
 * Match without Reset included), index k = d - min_disparity in [0, D):
 *   left view:  S[y][x][k];   right view (SGM_SetReferenceView(1)): S[y][x + min_disparity + k][k], columns outside the
 *   image counting as 65535 (.c:397-407).
 *   m1 = the smallest of these costs; d1 = the first index that reaches it (strict '>', .c:390 / .c:401);
 *   m2 = the smallest cost over every index k != d1, 65535 if there is none (.c:381).
 *   conf = (m2 == 0) ? 0 : (uint16_t)(((uint32_t)(m2 - m1) * 65535u) / m2)       (unsigned 32-bit, floor)
 * So a pixel without any candidate (m1 = m2 = 65535) and a tie for the best cost both give 0.  The value describes the
 * winner-take-all result: the LR check, the uniqueness test, speckle removal, hole filling and the median do not change it
 * (mask it with the disparity map's +INF where needed), and it does not depend on is_check_unique / uniqueness_ratio.
 * Layout u16 [B][H][W] like the disparity map.  disp is bit-identical to what the plain match returns for the same instance
 * state.  The sgm_match_confidence* forms mirror sgm_match / sgm_match_async (+ sgm_match_wait) / sgm_match_device;
 * SGM_MatchConfidence is SGM_Match on the default instance.  A NULL conf returns false and queues nothing; so does row-tile
 * mode (sgm_set_rows), and a build without the confidence kernels.  Timing: the store counts toward "sum" / "wta". */
bool SGM_MatchConfidence(const uint8_t* img_left, const uint8_t* img_right, float* disp_left, uint16_t* conf);

/* Both views' disparity maps from ONE match (extension; each map's parity is pinned: the left map is SGM_Match's, the right map is
 * SGM_Match's with SGM_SetReferenceView(1); returning the two together is "parity unpinned by the reference", whose SGM_Match
 * computes the right-view map (.c:105) and drops it).  Census, path aggregation, cost sum and both winner-take-all passes run once;
 * only the post pass differs between the views: one dual LR check reads the two raw WTA maps and writes the left-checked and the
 * right-checked map, then speckle removal and the median run over the 2 B maps as one batch.
 *   disp_left  is bit-identical to what SGM_Match returns for the same instance state with reference view 0,
 *   disp_right is bit-identical to what SGM_Match returns for the same instance state with reference view 1;
 * "the same instance state" includes the Q14 accumulation of a Match without Reset: S is accumulated once per call.  The
 * SGM_SetReferenceView setting is neither read nor changed.  Both maps f32 [B][H][W], +INF invalid.  Batches, the wide census
 * windows, four-path mode, sgm_set_overlap_post / sgm_set_stage_cus / sgm_set_stage_priority and buffers from sgm_host_alloc carry
 * over from the single-view match; the opt-in fused last sweep (SGM_UPSUM) is not used.  The sgm_match_both* forms mirror
 * sgm_match / sgm_match_async (+ sgm_match_wait) / sgm_match_device; SGM_MatchBoth is sgm_match_both on the default instance.
 * Returns false and queues nothing: for a NULL pointer; in row-tile mode (sgm_set_rows); with hole filling (SGM_SetFillHoles) or the
 * refinement (SGM_SetRefine) in effect -- their class map and confidence are defined for one reference view, and no meaning for
 * two is made up here --; in a build without the dual LR check kernel.  The extra device buffers (the raw left map, the two
 * finished maps, the speckle and median scratch of 2 B maps) are allocated at the first such call; an instance that never makes
 * one allocates and launches exactly what it did before.  Timing: the same eight entries, the second view's share counts toward
 * "lrcheck", "speckle" and "median". */
bool SGM_MatchBoth(const uint8_t* img_left, const uint8_t* img_right, float* disp_left, float* disp_right);

/* Refinement (extension, "parity unpinned by the reference": SemiGlobalMatching.h:24-40 has no such option; defined here and
 * restated by tests/refine_ref.py).  A confidence-weighted, edge-aware smoother after the median: the Fast Global Smoother of
 * Min et al. (2014), the weighted-least-squares filter behind OpenCV's DisparityWLSFilter, solved with separable 1-D tridiagonal
 * systems.  Low-confidence and invalid pixels take their value from confident neighbours on the same surface of the grey image;
 * depth edges stay where the image edges are.  Off by default (every launch, buffer and result is then the reference's); takes
 * effect at the next SGM_Initialize / sgm_initialize / SGM_Reset / sgm_reset, which return false with it on in row-tile mode
 * (sgm_set_rows) or together with hole filling (SGM_SetFillHoles: the refinement fills by itself, and a filled pixel would carry
 * the confidence of a disparity the LR check rejected).  Returns false and changes nothing for enable or keep_invalid other than
 * 0 / 1 and, with enable = 1, for a lambda or sigma that is not finite and > 0 or iterations outside 1..SGM_REFINE_MAX_ITERS
 * (with enable = 0 the other arguments are not looked at), or in a build without the kernels.
 * Per frame: D = the map after the median (f32 [H][W], +INF invalid); K = the reference view's confidence exactly as
 * SGM_MatchConfidence defines it (u16); G = the reference view's grey image, the one the census saw (the left image, the right
 * one with SGM_SetReferenceView(1)).  All arithmetic float32, every operation rounded on its own (no contraction, correctly
 * rounded divide, subnormals kept):
 *   1. c = isfinite(D) ? (float)K / 65535.0f : 0;  U = isfinite(D) ? c * D : 0;  V = c.
 *   2. For iteration t = 0..T-1: lam_t = lambda * 1.5 * 4^(T-1-t) / (4^T - 1) and L_t[k] = (float)(lam_t * exp(-k / sigma)),
 *      k = 0..255, in double, rounded once (sgm_refine_table).
 *   3. A line of n samples with guide values g: e_i = L_t[|g[i+1] - g[i]|]; a_i = e_{i-1} (0 at i = 0), c_i = e_i (0 at i = n-1),
 *      b_i = (1 + a_i) + c_i.  Thomas algorithm in this order: m_0 = b_0, m_i = b_i - a_i * q_{i-1}; q_i = c_i / m_i; for U and for
 *      V: r'_0 = r_0 / m_0, r'_i = (r_i + a_i * r'_{i-1}) / m_i; x_{n-1} = r'_{n-1}, x_i = r'_i + q_i * x_{i+1}  (m_i >= 1).
 *   4. Iteration t solves every row (horizontal pass), then every column (vertical pass), each on U and V.  Lines end at the
 *      frame edges; the frames of a batch are independent.
 *   5. out = V > 0 ? U / V : +INF; with keep_invalid the pixels that were +INF in D stay +INF, without it the map is dense
 *      wherever V > 0 (V is 0 where a small sigma makes the weights underflow and cuts a line into pieces without a confident pixel).
 * The result is a weighted average of the valid input disparities of the frame: it never leaves their [min, max] range.
 * Every match of the instance then computes the confidence (into the caller's map for sgm_match_confidence*, else into one of its
 * own; the fused last sweep is not used), and every entry point returns the refined map: SGM_Match, sgm_match*, sgm_compute,
 * the device and pipelined forms, sgm_match_planes* (whose depth is computed from it).  The passes run behind the median on the
 * post-pass stream (sgm_set_overlap_post, sgm_set_stage_cus and batches carry over) and read a private copy of G.
 * Timing: the refinement counts toward "median".  Defaults of the drivers (the best of a sweep on the four image pairs the
 * reference ships, NOTES.md): SGM_REFINE_DEFAULT_*. */
#define SGM_REFINE_MAX_ITERS 8
#define SGM_REFINE_DEFAULT_LAMBDA 16.0f
#define SGM_REFINE_DEFAULT_SIGMA 1.5f
#define SGM_REFINE_DEFAULT_ITERS 1
bool SGM_SetRefine(int enable, float lambda, float sigma, int iterations, int keep_invalid);
/* L_t of step 2 for (lambda, sigma, T = iterations, t) into out[256]; host only, no device needed.  false for arguments outside
 * the ranges of SGM_SetRefine or t outside [0, T). */
bool sgm_refine_table(float lambda, float sigma, int iterations, int t, float* out);

/* Rectification (extension, "parity unpinned by the reference": its image pairs arrive rectified; defined here and restated by
 * tests/rectify_ref.py).  Raw camera pairs are undistorted and row-aligned on the device ahead of the match -- OpenCV's
 * initUndistortRectifyMap -> remap -- so that every entry point can be fed sensor images.  Off by default (every launch, buffer
 * and result is then exactly what it is without); takes effect at the next SGM_Initialize / sgm_initialize / SGM_Reset /
 * sgm_reset, which upload the maps and return false when the maps' shape is not the frame's or in row-tile mode (sgm_set_rows).
 * Maps are as OpenCV's: per camera two float32 arrays map_x, map_y of [height][width]; output pixel (y, x) is sampled from the
 * source image at (map_y[y][x], map_x[y][x]).  Source and output have the same width x height, the instance's shape; one set of
 * maps serves all frames of a batch.
 *   Quantisation (on the host, when the maps are set; the caller's arrays are not borrowed): for a map value m,
 *     q = (int32_t)floor((double)m * 32.0 + 0.5).  If either coordinate of a pixel is not finite or has |m| > 32768, both xq and
 *     yq of that pixel become -64: all four taps fall outside.
 *   Sampling (exact integer arithmetic): x0 = xq >> 5 (arithmetic shift), ax = xq & 31, the same for y0, ay;
 *     p00 = src(y0, x0), p01 = src(y0, x0 + 1), p10 = src(y0 + 1, x0), p11 = src(y0 + 1, x0 + 1), any tap outside
 *     [0, H) x [0, W) counting as 0 (a constant border, decided per tap);
 *     out = ((32-ax)*(32-ay)*p00 + ax*(32-ay)*p01 + (32-ax)*ay*p10 + ax*ay*p11 + 512) >> 10.
 *   Integer maps copy pixels, identity maps reproduce the image exactly; there is no tolerance anywhere.
 * SGM_SetRectify / sgm_set_rectify: map_lx == NULL turns rectification off (the other arguments are then not looked at);
 * false, and nothing changes, for a NULL among the other three maps, width or height < 1, or (maps given) a build without the
 * kernel.  The default instance remembers its maps across SGM_Shutdown, as it does the census window.
 * The remap runs first in every match: census, the grey values of the adaptive P2, the refinement's guide and everything else
 * downstream see the rectified images, so batches, both census kinds and any window, four-path mode, the right reference view,
 * SGM_MatchBoth, the confidence, hole filling, the refinement, matches without Reset, sgm_set_overlap_post / sgm_set_stage_cus
 * and sgm_match_planes (grey conversion, then the remap) compose as they do without it.  The caller's images -- also the device
 * images of sgm_match_device and its twins -- are only read.  The rectified images stay readable as stages 19 / 20.
 * What it does not do: pixels whose taps fall outside the source are 0, and masking their disparities is left to the caller;
 * source images of another size than the frame's, row tiles, and per-frame maps within a batch are not supported.
 * Timing: the remap counts toward "census". */
bool SGM_SetRectify(int width, int height, const float* map_lx, const float* map_ly, const float* map_rx, const float* map_ry);
/* The maps of one camera by the formulas of OpenCV's initUndistortRectifyMap, in double, each value rounded once to float32; host
 * only, no device needed.  K, R, Knew: 3x3 row-major (camera matrix, rectifying rotation, new camera matrix); dist: k1 k2 p1 p2 k3.
 *   iR = (Knew R)^-1;  [X Y W]' = iR [u v 1]';  x = X / W, y = Y / W, r2 = x^2 + y^2;  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3;
 *   xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2);  yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y;
 *   map_x[v][u] = fx xd + cx,  map_y[v][u] = fy yd + cy   with fx, fy, cx, cy of K.
 * false for a NULL pointer, a size < 1 or a singular Knew R. */
bool sgm_rectify_maps(const double K[9], const double dist[5], const double R[9], const double Knew[9], int width, int height,
                      float* map_x, float* map_y);

/* Bits per image sample (extension, "parity unpinned by the reference", whose images are bytes; defined here and restated by
 * tests/pixels16_ref.py).  Sensors deliver 10..16 bits; tone-mapping them to 8 before the match throws away what the census lives
 * on, the order of neighbouring samples.  The census is a rank transform and needs no tone map: with bits in 9..16 it is evaluated
 * on the samples as they are, and everything below it is the 8-bit pipeline unchanged.
 * bits == 8 (default): every launch, buffer and result is exactly what it is without this call.  bits in 9..16 takes effect at the
 * next SGM_Initialize / sgm_initialize / SGM_Reset / sgm_reset.  From then on EVERY image pointer of every match entry point --
 * SGM_Match, sgm_compute, sgm_match[_async|_device], the _confidence* and _both* families, sgm_rectify (inputs and outputs) --
 * refers to width * height uint16_t samples per frame: host byte order, row-major, stride = width, the [B] frames of sgm_set_batch
 * back to back.  The parameter types stay const uint8_t*, so the ABI is unchanged: cast the pointer.  Device images must be 2-byte
 * aligned and nothing more (the kernels read single samples; an odd address returns false and queues nothing).
 *   1. Census: the formulas of the 5x5 centre census, of SGM_SetCensusKind(SGM_CENSUS_SYMMETRIC) and of the wide centre windows
 *      (SGM_SetCensusWindow, u64 words), evaluated on the u16 samples as they are: the same strict <, bit order, zero borders and
 *      "window does not fit -> all 0" rule.  Every word of the frame is written on every match (the default instance's stale-border
 *      behaviour, SURVEY.md Q3, belongs to the 8-bit 5x5 centre census only).
 *   2. Narrowed image, per view: g8 = min(v >> (bits - 8), 255).  A sample >= 2^bits is therefore defined: it saturates.  g8 is
 *      what the adaptive-P2 lookup, the refinement's guide and every other reader of grey values see; it is written by the census
 *      kernel and readable as stages 21 (left) and 22 (right), u8 [H][W] (0 bytes with 8-bit input).
 *   3. Rectification (SGM_SetRectify): the same quantised maps, tap rule and constant-0 border on the u16 samples,
 *      out = (... + 512) >> 10 in unsigned 32-bit arithmetic (1024 * 65535 + 512 < 2^32).  It runs before the census; stages 19 / 20
 *      then hold u16 [H][W].
 *   4. Everything downstream of the census words and g8 is untouched.  So a pair with v = u8 << (bits - 8) gives results
 *      bit-identical to the 8-bit match of u8 -- every stage, every option, the confidence, both views, filled, refined, clouds.
 *   5. Refused with more than 8 bits in effect (false, nothing queued, a message): row-tile mode (sgm_set_rows) at initialize /
 *      reset; sgm_match_planes*, whose planes are bytes by protocol.  The opt-in fused last sweep (SGM_UPSUM) is simply not used.
 * Returns false and changes nothing for any other bits, and for 9..16 in a build without the kernels.  The default instance
 * remembers the setting across SGM_Shutdown, as it does the census window.  Timing: everything new counts toward "census". */
bool SGM_SetPixelBits(int bits);

/* Same as SGM_Match but all three pointers are DEVICE pointers (HBM-resident frames) on the
 * instance's device.  Asynchronous on the instance's stream; SGM_Synchronize waits. */
bool SGM_MatchDevice(const uint8_t* d_left, const uint8_t* d_right, float* d_disp_left);
bool SGM_Synchronize(void);

/* Releases every device resource of the default instance (the reference has no counterpart). */
void SGM_Shutdown(void);

/* The one-call form BASELINE.json's north_star names ("sgm_compute(left, right, params -> disparity)"; the reference
 * itself has no such symbol, its boundary is the three functions above): SGM_Reset(width, height, option) followed by
 * SGM_Match(img_left, img_right, disp_left) on the default instance -- the per-frame sequence of main.c:72,83 and
 * of SURVEY.md Q14.  Host pointers, blocking, same results and the same true/false behaviour as the two calls. */
bool sgm_compute(const uint8_t* img_left, const uint8_t* img_right, uint16_t width, uint16_t height,
                 const SGMOption* option, float* disp_left);

/* ---- explicit instances: several frames in flight on one GPU, one per HIP stream ---- */
typedef struct sgm_instance sgm_instance;

sgm_instance* sgm_create(int device_ordinal);                 /* NULL on failure */
void          sgm_destroy(sgm_instance* s);
void          sgm_set_honor_num_paths(sgm_instance* s, int honor);
bool          sgm_set_census_window(sgm_instance* s, int width, int height);   /* see SGM_SetCensusWindow */
bool          sgm_set_census_kind(sgm_instance* s, int kind);                  /* see SGM_SetCensusKind */
void          sgm_set_reference_view(sgm_instance* s, int right);              /* see SGM_SetReferenceView */
bool          sgm_set_pixel_bits(sgm_instance* s, int bits);                   /* see SGM_SetPixelBits */
bool          sgm_set_fill_holes(sgm_instance* s, int enable);                 /* see SGM_SetFillHoles */
bool          sgm_set_refine(sgm_instance* s, int enable, float lambda, float sigma, int iterations, int keep_invalid);  /* see SGM_SetRefine */
bool          sgm_set_rectify(sgm_instance* s, int width, int height, const float* map_lx, const float* map_ly, const float* map_rx,
                              const float* map_ry);                            /* see SGM_SetRectify */
bool          sgm_initialize(sgm_instance* s, uint16_t width, uint16_t height, const SGMOption* option);
bool          sgm_reset(sgm_instance* s, uint16_t width, uint16_t height, const SGMOption* option);
bool          sgm_match(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left);
bool          sgm_match_device(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, float* d_disp_left);
bool          sgm_synchronize(sgm_instance* s);
/* Pipelined host-pointer matches (SGM_Match's H2D / kernels / D2H of SemiGlobalMatching.c:77-78,122 without the
 * blocking wait): sgm_match_async stages the images, queues the upload, the pipeline and the download on the instance's
 * stream and returns; the three buffers stay borrowed until sgm_match_wait (or the next sgm_match_async / sgm_initialize /
 * sgm_reset / sgm_destroy on the same instance, which wait implicitly) has handed the result over.  A caller that
 * round-robins frames over two or three instances overlaps the copies of one with the kernels of the others.
 * sgm_match == sgm_match_async + sgm_match_wait.  Buffers from sgm_host_alloc (page-locked) are used in place: no
 * staging copy on either side; any other host pointer is staged through the instance's own pinned buffers. */
bool          sgm_match_async(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left);
bool          sgm_match_wait(sgm_instance* s);
/* the matching confidence beside the disparity map (see SGM_MatchConfidence): host blocking, host pipelined (+ sgm_match_wait;
 * buffers from sgm_host_alloc are used in place), device pointers (asynchronous, as sgm_match_device) */
bool          sgm_match_confidence(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left, uint16_t* conf);
bool          sgm_match_confidence_async(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left,
                                         uint16_t* conf);
bool          sgm_match_confidence_device(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, float* d_disp_left,
                                          uint16_t* d_conf);
/* both views' maps from one match (see SGM_MatchBoth): host blocking, host pipelined (+ sgm_match_wait; all four buffers stay
 * borrowed until then, buffers from sgm_host_alloc are used in place), device pointers (asynchronous, as sgm_match_device) */
bool          sgm_match_both(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left, float* disp_right);
bool          sgm_match_both_async(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left,
                                   float* disp_right);
bool          sgm_match_both_device(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, float* d_disp_left,
                                    float* d_disp_right);
void*         sgm_host_alloc(sgm_instance* s, size_t bytes);   /* page-locked host memory on the instance's device; NULL on failure */
void          sgm_host_free(sgm_instance* s, void* p);
/* Throughput option for a stream of matches on ONE instance: with sgm_set_overlap_post(s, 1) the post pass of a match (LR
 * check, speckle removal, median: latency-bound kernels that occupy a fraction of the GPU) runs on a second stream of the
 * instance, ordered behind the match's cost sum by an event, while sgm_stream(s) goes on with the census and aggregation of
 * the next match; the next cost sum waits for the post pass that still reads the shared maps.  Results are unchanged.  What
 * changes: the disparity map of sgm_match_device is complete after sgm_synchronize (or sgm_match_wait for the host-pointer
 * form), no longer in stream order of sgm_stream(s).  Off by default; ignored in row-tile mode. */
bool          sgm_set_overlap_post(sgm_instance* s, int enable);
/* Stage groups on streams -- and compute units -- of their own.  A match is three groups of kernels with different appetites:
 * census + path aggregation (VALU-bound, SemiGlobalMatching.c:82-94), cost sum + both winner-take-all passes (HBM-bound,
 * .c:94-105), LR check + speckle removal + median (latency-bound, a few workgroups, .c:109-120).  When several matches are in
 * flight on one GPU (two instances, or a stream of matches on one with sgm_set_overlap_post) kernels of different groups share
 * compute units and slow each other down far more than they gain from the sharing -- the median's serial kernel runs three
 * times longer next to an aggregation's waves than alone.  sgm_set_stage_cus(s, which, first, count) gives group `which` a HIP
 * stream of its own whose kernels run only on CUs [first, first + count) of EVERY XCD (MI355X: 32 CUs in each of 8 XCDs; each
 * XCD keeps its L2 and its path to HBM in play); the groups are ordered by events, results are unchanged.
 *   count > 0   own stream on those CUs        count == 0  own stream, all CUs       count < 0  back to the default
 *   which = SGM_STAGE_MAIN: the stream census + aggregation (and every group without a stream of its own) run on; re-created,
 *   so sgm_stream(s) changes: a caller that cached the handle (the tile pipeline's slots do) must query it again, the old one
 *   is destroyed.   SGM_STAGE_POST with count == 0 is sgm_set_overlap_post(s, 1).
 * As with sgm_set_overlap_post a result is complete after sgm_synchronize / sgm_match_wait, not in stream order of
 * sgm_stream(s).  Ignored in row-tile mode.  The instance must be idle (the call waits for it). */
enum { SGM_STAGE_MAIN = 0, SGM_STAGE_SUM = 1, SGM_STAGE_POST = 2 };
bool          sgm_set_stage_cus(sgm_instance* s, int which, int first_cu_per_xcd, int cus_per_xcd);
/* The same with a dispatch priority instead of a CU range: the group gets a stream of its own on all CUs whose waiting
 * workgroups the dispatcher serves before (priority < 0) or after (> 0) those of normal streams (clamped to the device's
 * range).  Replaces a CU range set before; a later sgm_set_stage_cus (count >= 0) replaces the priority stream in turn, and
 * count < 0 goes back to the default in either case. */
bool          sgm_set_stage_priority(sgm_instance* s, int which, int priority);
/* The HIP stream (hipStream_t as void*) the instance launches on, e.g. to record events. */
void*         sgm_stream(sgm_instance* s);
/* Whether the LAST match ran the fused last sweep (csrc/sgm_upsum.hip: the three upward directions computed inside the cost-sum /
 * winner-take-all kernel, their planes never written): image rows per workgroup of that kernel, 0 = the separate kernels.  It is used
 * for batches of whole frames with W > H, a padded range of 128, eight paths and P1 >= 0 when SGM_UPSUM allows it, and only by
 * matches that neither add to an earlier S (Q14) nor keep stages; results are identical either way. */
int           sgm_fused_sweep_rows(const sgm_instance* s);

/* Batches: after sgm_set_batch(s, n) and the next sgm_initialize / sgm_reset, every sgm_match /
 * sgm_match_device call processes n frames of the same shape stored back to back ([n][H][W] for the
 * images and the disparity output) -- each kernel of the pipeline covers all n frames in one launch,
 * which is how one GPU is filled when frames are small.  n = 1 (default) is the reference behaviour.
 * n is 1 to 1024; anything else returns false and changes nothing.  The limits of sgm_initialize hold per frame and are unchanged
 * by the batch (width * height below 2^31, width * height * the padded range below 2^32 - 1); the totals of a batch may pass 2^32
 * cells, pixels times frames included: every frame base is 64-bit arithmetic, and only device memory bounds the batch
 * (8 bytes per padded cell of the batch for the path planes, 3 more where S and the cost volume exist).  The entry points that
 * return both views, and the two-view temporal filter, run their post pass on 2 n maps. */
bool          sgm_set_batch(sgm_instance* s, int frames);
/* which frame of the batch sgm_read_stage returns (default 0) */
void          sgm_select_frame(sgm_instance* s, int frame);

/* ---- row tiles: one frame over several GPUs (each GPU one instance, one process per GPU) ----
 * After sgm_set_rows(s, r0, r1) and the next sgm_initialize / sgm_reset the instance computes rows [r0, r1) of
 * the frame (r1 = 0 returns to whole frames).  Per frame, on every GPU (all calls asynchronous on sgm_stream):
 *
 *     sgm_tile_begin(s, d_left, d_right)          census, horizontal paths of the tile, anomalous diagonals
 *     forward sweep, tiles top to bottom:          backward sweep, tiles bottom to top:
 *       [sgm_tile_import_boundary(s, 1, buf)]        [sgm_tile_import_boundary(s, 0, buf)]   not at the frame edge
 *       sgm_tile_sweep(s, 1)                         sgm_tile_sweep(s, 0)
 *       sgm_tile_export_boundary(s, 1, buf)          sgm_tile_export_boundary(s, 0, buf)     -> next GPU
 *     sgm_tile_finish(s, d_disp)                   cost sum, WTA (both views), LR check -> rows [r0, r1) of d_disp
 *     (gather the rows of all GPUs into one [H][W] map)
 *     sgm_tile_post(s, d_disp)                     speckle removal + median on the whole frame
 *
 * d_left / d_right are the whole images (replicated); buf holds sgm_tile_boundary_bytes(s) bytes of device
 * memory: the path costs of one image row for the 3 directions of a sweep (1 with four paths).  The two
 * sweeps are independent of each other.  The result is bit-identical to sgm_match on one GPU.
 * With sgm_set_batch(s, B) every call covers the same rows of B frames ([B][H][W] images and maps; the hand-over buffer holds
 * B such rows, frame-major): one launch per stage for the B tiles -- a tile of a single frame leaves most of a GPU idle. */
bool   sgm_set_rows(sgm_instance* s, int row_begin, int row_end);
bool   sgm_tile_begin(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right);
size_t sgm_tile_boundary_bytes(const sgm_instance* s);
bool   sgm_tile_import_boundary(sgm_instance* s, int forward, const void* d_buf);
bool   sgm_tile_sweep(sgm_instance* s, int forward);
bool   sgm_tile_export_boundary(sgm_instance* s, int forward, void* d_buf);
bool   sgm_tile_finish(sgm_instance* s, float* d_disp_left);
bool   sgm_tile_post(sgm_instance* s, float* d_disp_left);

/* ---- test-platform arithmetic on device buffers ----
 * What the reference's host platform does with a returned map (HostScript_Server/depth_image.py:138-165 disparity_to_depth,
 * :276-319 compare_img), for maps that are already in HBM.  Restated from reading: that module imports cv2, which is not
 * installed where this library is built, so no reference-made vectors exist -- "parity unpinned" (tests compare with the
 * host restatement soc_project_stereo_matching_amd/platform.py).
 *   depth[mm] = float32(fx * baseline) / (disparity + doffs); a non-finite or zero denominator (invalid = +INF) -> NaN.
 *   compare (blocking): over the pixels finite in BOTH images: rmse = sqrt(mean((test - gt)^2)), bad_pixel_rate = share
 *   with |test - gt| > abs_thresh [mm], n_valid; (NaN, NaN, 0) if there is none.  Asynchronous / blocking on sgm_stream(s). */
bool   sgm_disparity_to_depth(sgm_instance* s, const float* d_disparity, size_t count, float fx, float baseline, float doffs,
                              float* d_depth);
bool   sgm_compare_depth(sgm_instance* s, const float* d_ground_truth, const float* d_test, size_t count, float abs_thresh,
                         double* rmse, double* bad_pixel_rate, uint64_t* n_valid);

/* Depth from both views' maps as the test platform combines them (depth_image.py:167-197, depth_from_left_and_right_disp; pinned by
 * tests/golden/platform_depth_both.npz, made by that function itself): depth_l = sgm_disparity_to_depth of d_disp_left with
 * fx_left (cam0[0,0]), depth_r = the same of d_disp_right with fx_right (cam1[0,0]); depth = isfinite(depth_l) ? depth_l : depth_r.
 * The fill is per pixel, without warping the right map into the left view: the reference's behaviour, kept.  (Where the reference's
 * bare formula meets this library's invalid marker +INF it gives depth 0, which counts as finite there; here an invalid left pixel
 * is NaN and takes the right view's depth, as with the NaN-masked maps the platform itself feeds that function.)  Asynchronous on
 * sgm_stream(s), behind the last match; false in a build without the kernel.  host restatement:
 * soc_project_stereo_matching_amd/platform.py. */
bool   sgm_depth_from_both(sgm_instance* s, const float* d_disp_left, const float* d_disp_right, size_t count, float fx_left,
                           float fx_right, float baseline, float doffs, float* d_depth);

/* ---- point clouds: disparity maps to XYZ on the device, organised or compacted ----
 * Extension, "parity unpinned by the reference" (it has no such step); defined here and restated by tests/cloud_ref.py.
 * Per pixel p = (f, y, x) of a map, in float32, every operation rounded on its own (no contraction, correctly rounded divide):
 *   fb = (float)((double)fx * (double)baseline)                       (the value sgm_disparity_to_depth uses)
 *   the pixel is KEPT iff all of:  d = disp[p] is finite (by its bit pattern: a caller's map may hold NaN);
 *     mask == NULL || mask[p] != 0;   conf == NULL || conf[p] >= min_conf;
 *     den = d + doffs is finite and den > 0;   Z = fb / den is finite;   z_min <= Z && Z <= z_max
 *   for a kept pixel  X = (((float)x - cx) * Z) / fx,  Y = (((float)y - cy) * Z) / fy.
 * So Z of a kept pixel is bit-identical to what sgm_disparity_to_depth writes for it.  Two products of the one predicate:
 *   organised cloud   float [frames][height][width][3]: X Y Z of a kept pixel, three quiet NaNs (0x7FC00000) for every other
 *                     (what cv::reprojectImageTo3D and PCL users expect);
 *   point list        the kept pixels only, as sgm_point records packed in raster order -- frame-major, then row, then column --
 *                     with offsets[frames + 1] (u32): frame f's points are points[offsets[f] .. offsets[f + 1]), offsets[frames]
 *                     is the total.  The order is part of the contract: the list is the same on every run (numpy's nonzero
 *                     order).  Records at index offsets[frames] and beyond are not written.
 * sgm_cloud_organized / sgm_cloud_points: all pointers are device pointers on the instance's device; d_mask (u8) and d_conf (u16)
 * may be NULL and, like d_disp, need no alignment beyond their element's (a map that cannot be read 16 bytes at a time takes a
 * one-pixel-per-lane path with the same results); d_points has room for frames * width * height records (nothing is clipped) and
 * is 16-byte aligned.  Asynchronous on sgm_stream(s), behind the last match also where its post pass runs on a stream of its own
 * (sgm_set_overlap_post).
 * d_disp == NULL: the reference-view final map of the instance's last match, the one stage 8 reads back (after sgm_match_device
 * and its twins the result is in the caller's buffer: pass that); the spec's width / height / frames must then be the instance's
 * shape and batch, and row-tile mode (sgm_set_rows) is refused.  With an explicit d_disp the instance need not be initialised.
 * false, and nothing is queued: NULL s, spec or output; a d_points that is not 16-byte aligned; a spec outside the ranges below;
 * fx, fy, baseline or fb not finite and > 0; cx, cy or doffs not finite; z_min NaN or < 0; z_max NaN or not > z_min (+INFINITY is allowed); min_conf > 65535; a build
 * without the kernels.  The point list takes three launches (count per tile, one scan, emit) and a few bytes of scratch per 2048
 * pixels, allocated at the first such call: an instance that never asks for a cloud allocates and launches what it did before.
 * sgm_read_cloud (blocking; SGM_ReadCloud: the default instance): the point list of the last match's final map, no mask and no
 * confidence, made in device buffers of the instance's own.  offsets (frames + 1 entries) is always copied to the host; if
 * offsets[frames] <= capacity exactly that many records are copied to points and the result is true, else no record is copied
 * and the result is false: size a buffer from offsets[frames] and call again (points may be NULL with capacity 0). */
typedef struct {            /* 48 bytes, every field 4 bytes, no padding */
    int32_t  width, height, frames;     /* maps are f32 [frames][height][width]; 1 <= width, height <= 65535, frames >= 1,
                                           frames * width * height <= 2^31 */
    float    fx, fy, cx, cy;            /* pinhole of the rectified reference camera, pixels */
    float    baseline, doffs;           /* as sgm_disparity_to_depth: depth = fx * baseline / (d + doffs) */
    float    z_min, z_max;              /* keep z_min <= Z <= z_max; 0 and +INFINITY keep every finite positive Z */
    uint32_t min_conf;                  /* with a confidence map: keep conf >= min_conf (0..65535) */
} sgm_cloud_spec;
typedef struct { float x, y, z; uint32_t pixel; } sgm_point;     /* 16 bytes; pixel = (y << 16) | x */
bool   sgm_cloud_organized(sgm_instance* s, const sgm_cloud_spec* spec, const float* d_disp, const uint8_t* d_mask,
                           const uint16_t* d_conf, float* d_xyz);
bool   sgm_cloud_points(sgm_instance* s, const sgm_cloud_spec* spec, const float* d_disp, const uint8_t* d_mask,
                        const uint16_t* d_conf, sgm_point* d_points, uint32_t* d_offsets);
bool   sgm_read_cloud(sgm_instance* s, const sgm_cloud_spec* spec, sgm_point* points, size_t capacity, uint32_t* offsets);
bool   SGM_ReadCloud(const sgm_cloud_spec* spec, sgm_point* points, size_t capacity, uint32_t* offsets);
/* The mask SGM_SetRectify leaves to the caller: mask[y][x] = 1 iff all four taps of output pixel (y, x) fall inside
 * [0, height) x [0, width) under exactly the quantisation and tap rule of SGM_SetRectify (a pixel with a coordinate that is not
 * finite or has |m| > 32768 gets 0), else 0 -- a tap with weight 0 counts like any other.  Host only, no device needed; one
 * camera per call: a caller who also wants the right view's footprint combines the two masks itself.  false for a NULL pointer,
 * a size < 1 or more than 2^31 - 1 pixels. */
bool   sgm_rectify_valid_mask(int width, int height, const float* map_x, const float* map_y, uint8_t* mask);

/* ---- depth registered to another camera: a z-buffered forward warp on the device ----
 * Extension, "parity unpinned by the reference" (it has no such step); defined here and restated by tests/register_ref.py.  Every
 * result of a match lives in the rectified reference camera; a caller's pixels live in the raw image that was fed in
 * (SGM_SetRectify) or in a colour camera beside the pair.  This is the "align / register depth to colour" step of a stereo SDK.
 *
 * Points.  The contributing pixels are exactly the KEPT pixels of the cloud contract above -- the same predicate over src, d_mask,
 * d_conf, min_conf and the source's z_min / z_max -- and X, Y, Z are the float32 values sgm_cloud_organized writes for them.
 * Projection.  float32, every operation rounded on its own (no contraction, correctly rounded divide, subnormals kept); the
 * parentheses are the contract:
 *   X' = ((R0*X + R1*Y) + R2*Z) + t0          (Y' with R3..5, t1;  Z' with R6..8, t2)
 *   drop unless Z' is finite (by its bit pattern), Z' > 0, z_min <= Z' && Z' <= z_max
 *   a = X'/Z', b = Y'/Z';  aa = a*a, bb = b*b, ab = a*b;  r2 = aa + bb
 *   rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1
 *   xd  = (a*rad + (2*p1)*ab) + p2*(r2 + 2*aa)
 *   yd  = (b*rad + p1*(r2 + 2*bb)) + (2*p2)*ab
 *   u = fx*xd + cx,  v = fy*yd + cy;  drop unless both are finite
 * Candidates.  splat == 1: the one target pixel (floorf(u + 0.5f), floorf(v + 0.5f)).  splat == 2: with u0 = floorf(u),
 * v0 = floorf(v) the four (u0, v0), (u0 + 1, v0), (u0, v0 + 1), (u0 + 1, v0 + 1).  A candidate (uf, vf) is admitted iff
 * 0 <= uf && uf < (float)width && 0 <= vf && vf < (float)height, tested in float before any conversion to int.
 * Z-buffer.  Per target pixel the winner among all admitted candidates of its frame is the one with the smallest 64-bit key
 * ((uint64)bits(Z') << 32) | pixel, pixel = (y << 16) | x of the source: Z' > 0 makes the bit pattern monotonic, so the nearest
 * surface wins, equal Z' bits go to the smaller source pixel, and the result does not depend on the order of arrival: it is the
 * same on every run.  Frame f of the source writes frame f of the target.
 * Outputs.  d_depth f32 [frames][height][width]: Z' of the winner, the quiet NaN 0x7FC00000 where nothing landed.  d_source u32 of
 * the same shape (may be NULL): the winner's pixel, 0xFFFFFFFF where nothing landed.  Nothing outside these arrays is written.
 *
 * sgm_register_gather: out[f][v][u] = source[f][v][u] == 0xFFFFFFFF ? *fill : map[f][y][x], for a map of 1-, 2- or 4-byte elements
 * of the source's shape: how a confidence, the disparity itself, a grey or colour plane or a mask follows the depth into the
 * target image.  fill is a HOST pointer to one element, read before the call returns; a source word that names no pixel of the
 * source shape reads nothing and gives *fill as well.
 * sgm_register_spec_raw (host only): the target "back into the raw camera that sgm_rectify_maps(K, dist, R, Knew, ..) rectified":
 * pinhole and dist from K / dist, R the transpose of the rectifying rotation, t = 0, z_min = 0, z_max = +INFINITY, every value
 * computed in double and rounded once to float32; the source pinhole a caller pairs with it is Knew's.  false for a NULL pointer,
 * a size outside 1..65535, a splat other than 1 or 2, a non-finite input.
 *
 * All other pointers are device pointers on the instance's device and need no alignment beyond their element's (a map that cannot
 * be read 16 bytes at a time takes the one-pixel-per-lane path with the same results).  Asynchronous on sgm_stream(s), behind the
 * last match also with sgm_set_overlap_post, as for clouds.  d_disp == NULL: the instance's last final map, under the cloud entry
 * points' rules.  false, nothing queued and a message on stderr: a NULL s, spec, d_depth (d_source, d_map, fill, d_out for the
 * gather); an output that aliases d_disp (an input, for the gather) or the other output; a pointer not aligned to its element; a
 * src outside the cloud spec's ranges; a dst with width or height outside 1..65535 or frames * width * height > 2^31; fx or fy
 * not finite and > 0; a non-finite cx, cy, dist, R or t; z_min NaN or < 0; z_max NaN or not > z_min; a splat that is not 1 or 2;
 * an elem_bytes other than 1, 2 or 4; a build without the kernels.  Three launches (clear, scatter, resolve) and 8 bytes of key
 * scratch per target pixel, reserved at the first call: an instance that never calls these entry points allocates and launches
 * exactly what it did before.  Not part of it: closing the holes of the registered map, fisheye or rational distortion models,
 * per-frame extrinsics within a batch, row tiles, sgm_match_planes. */
typedef struct {            /* 104 bytes, every field 4 bytes, no padding */
    int32_t width, height;  /* target image, 1..65535 each; frames * width * height <= 2^31 */
    float   fx, fy, cx, cy; /* target pinhole, pixels */
    float   dist[5];        /* k1 k2 p1 p2 k3 of the target camera (all 0: none) */
    float   R[9], t[3];     /* P' = R P + t: source (rectified reference camera) coordinates -> target camera coordinates; row-major; t in the units of baseline */
    float   z_min, z_max;   /* keep z_min <= Z' <= z_max; 0 and +INFINITY keep every finite positive Z' */
    int32_t splat;          /* 1: the nearest target pixel;  2: the four target pixels around the projection */
} sgm_register_spec;
bool   sgm_register_depth(sgm_instance* s, const sgm_cloud_spec* src, const sgm_register_spec* dst,
                          const float* d_disp, const uint8_t* d_mask, const uint16_t* d_conf,
                          float* d_depth, uint32_t* d_source /* may be NULL */);
bool   sgm_register_gather(sgm_instance* s, const sgm_cloud_spec* src, const sgm_register_spec* dst,
                           const uint32_t* d_source, int elem_bytes /* 1, 2, 4 */,
                           const void* d_map, const void* fill, void* d_out);
bool   sgm_register_spec_raw(const double K[9], const double dist[5], const double R[9],
                             int width, int height, int splat, sgm_register_spec* out);   /* host only */

/* ---- depth from a moving rig fused into a TSDF volume on the device ----
 * Extension, "parity unpinned by the reference" (it has no such step); defined here and restated by tests/volume_ref.py.  Clouds,
 * registration and the temporal filter stop at one camera position; depth maps with known poses are integrated into a truncated
 * signed distance volume and the surface is read back out: the "spatial mapping" of a stereo SDK.
 *
 * The volume.  A caller-owned device array of nx * ny * nz uint32 words, voxel n = (k*ny + j)*nx + i (x fastest), each
 * (w << 16) | (uint16_t)tq: tq an int16, 32767 meaning +trunc, and w the weight.  All-zero bytes are the empty volume (there is no
 * clear entry point: hipMemset it).  sgm_volume_bytes: its size, host only, 0 for a refused spec.
 * Integration.  The contributing pixels are the KEPT pixels of the cloud contract above (src, d_mask, d_conf) and Z is their cloud
 * Z.  For voxel (i, j, k) and frame f, in float32, every operation rounded on its own (no contraction, correctly rounded divide);
 * the parentheses are the contract:
 *   px = ox + ((float)i + 0.5f) * voxel          (py, pz alike)
 *   X' = ((R0*px + R1*py) + R2*pz) + t0          (Y' with R3..5, t1;  Z' with R6..8, t2;  R, t of frame f: world -> camera f)
 *   skip unless Z' is finite (by its bits) and Z' > 0
 *   u = fx*(X'/Z') + cx,  v = fy*(Y'/Z') + cy;   skip unless both finite
 *   uf = floorf(u + 0.5f), vf = floorf(v + 0.5f); skip unless 0 <= uf < (float)width && 0 <= vf < (float)height, tested in float
 *   skip unless source pixel (f, vf, uf) is KEPT;  Z = its cloud Z
 *   sdf = Z - Z';  skip if sdf < -trunc
 *   q   = (int)rintf((fminf(sdf, trunc) / trunc) * 32767.0f)                    (round half to even)
 *   num = tq*w + q;  den = w + 1;  tq = floor_div(2*num + den, 2*den)            (signed, floor: num / den rounded, halves up)
 *   w   = min(w + 1, max_weight)
 * (2*num + den is meant exactly: past w = 32767 it leaves int32, so the kernel takes the floor quotient and remainder of num / den
 * and adds 1 when twice the remainder reaches den, which is the same number.)  Frames take effect in order f = 0 .. frames-1; one
 * call over B frames equals B calls of one frame each, bit for bit; a launch reads and writes each voxel word at most once,
 * whatever B is (a lane owns its voxels and loops over the frames: no atomics, no order between workgroups).
 * Surface points.  For voxel n and axis a = 0, 1, 2 with the neighbour m one step up in x, y or z and inside the grid, a crossing
 * exists iff w[n] >= min_weight && w[m] >= min_weight && (tq[n] < 0) != (tq[m] < 0).  Its point is the centre of voxel n (px, py,
 * pz above) with s * voxel added along the axis, s = (float)tq[n] / ((float)tq[n] - (float)tq[m]), and id = n*4 + a.  The list is
 * sorted by id and the same on every run (count per tile, one scan, emit: no atomics).  d_count[0] always receives the full number
 * of crossings; records with index >= capacity are not written; nothing else is written.
 *
 * poses is a HOST pointer, [src->frames][12]: R row-major, then t, P' = R P + t as in sgm_register_spec, t and the volume in the
 * units of baseline; it is read before the call returns.  All other pointers are device pointers on the instance's device and
 * need no alignment beyond their element's, except d_points (16 bytes): a volume with nx % 4 != 0 or a d_voxels that cannot be
 * accessed 16 bytes at a time takes a one-voxel-per-lane path with the same results.  Asynchronous on sgm_stream(s), behind the
 * last match also with sgm_set_overlap_post, as for clouds.  d_disp == NULL: the instance's last final map, under the cloud entry
 * points' rules.  false, nothing queued and a message on stderr: a NULL s, spec, src, poses, d_voxels (d_count; d_points unless
 * capacity is 0); a spec outside the ranges below; a src outside the cloud spec's ranges or with more than 64 frames (the poses
 * travel as kernel arguments); a non-finite pose entry; a min_weight outside 1..65535; a pointer not aligned as said; a d_voxels
 * that aliases a map (d_points or d_count that alias the volume or each other); a build without the kernels.  The extraction
 * keeps 8 bytes of scratch per tile of 2048 voxels, reserved at its first call: an instance that never calls these entry points
 * allocates and launches exactly what it did before.  Not part of it: meshing and ray-casting the volume into a view, which are
 * entry points of their own (sgm_volume_mesh and sgm_volume_raycast below), confidence-weighted updates, colour, voxel hashing (a
 * volume that moves with the rig is made of windows: sgm_volume_window below), estimating the poses (sgm_track below does that
 * against a ray-cast), row tiles, sgm_match_planes. */
typedef struct {            /* 36 bytes, every field 4 bytes, no padding */
    int32_t  nx, ny, nz;    /* 1..1024 each, nx*ny*nz <= 2^30; voxel n = (k*ny + j)*nx + i, x fastest */
    float    voxel;         /* edge length, units of baseline; finite, > 0 */
    float    origin[3];     /* world position of the corner of voxel (0,0,0); finite */
    float    trunc;         /* truncation distance; finite, > 0 */
    uint32_t max_weight;    /* 1..65535 */
} sgm_volume_spec;
typedef struct { float x, y, z; uint32_t id; } sgm_surface_point;   /* 16 bytes; id = n*4 + axis */
size_t sgm_volume_bytes(const sgm_volume_spec* spec);                /* host only; 0 for a refused spec */
bool   sgm_volume_integrate(sgm_instance* s, const sgm_volume_spec* spec, const sgm_cloud_spec* src,
                            const float* poses /* HOST, [src->frames][12]: R row-major then t; read before return */,
                            const float* d_disp, const uint8_t* d_mask, const uint16_t* d_conf, uint32_t* d_voxels);
bool   sgm_volume_points(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_voxels, uint32_t min_weight /* 1..65535 */,
                         sgm_surface_point* d_points /* 16-byte aligned */, size_t capacity, uint32_t* d_count);

/* ---- the TSDF volume as a triangle mesh: marching tetrahedra on the device ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/mesh_ref.py.  sgm_volume_points hands back an
 * unconnected list of crossings; a viewer, a collision checker or a texture step needs connectivity.  Takes a volume as
 * sgm_volume_integrate leaves it and writes an indexed triangle mesh: a vertex list and a triangle list.  Marching tetrahedra, not
 * cubes: 16 cases per tetrahedron, none ambiguous, so the mesh is closed wherever the cells around it are meshed.  All float
 * arithmetic follows sgm_volume_points: float32, every operation rounded on its own, no contraction.
 *
 * Size limit.  A spec sgm_volume_integrate accepts with, in addition, nx*ny*nz <= 2^27: then n*8 + e, at most 7 vertices per voxel
 * and at most 12 triangles per cell all fit uint32.  A larger volume is refused by this entry point only.
 * Edges.  Edge kind e of voxel n = (i,j,k) runs to the voxel at (i+dx, j+dy, k+dz):
 *   e = 0: (1,0,0)   1: (0,1,0)   2: (0,0,1)   3: (1,1,0)   4: (1,0,1)   5: (0,1,1)   6: (1,1,1)
 * and exists when that far voxel is inside the grid.  Kinds 0..2 are the axes of sgm_volume_points.
 * Vertices.  Edge (n, e) with far voxel m carries a vertex iff w[n] >= min_weight && w[m] >= min_weight && (tq[n] < 0) != (tq[m] < 0),
 * the crossing rule of sgm_volume_points (zero counts as non-negative).  s = (float)tq[n] / ((float)tq[n] - (float)tq[m]); each
 * coordinate in which the edge steps is centre + s * voxel, the others are the centre of voxel n (px, py, pz of the volume
 * contract); id = n*8 + e.  The list is sorted by id and holds every such edge, whether or not a triangle uses it; its records
 * with e < 3 are exactly the records of sgm_volume_points with the same min_weight (same x, y, z; id n*4 + a <-> n*8 + a).
 * Cells and tetrahedra.  Cell n = (i,j,k) exists iff i+1 < nx, j+1 < ny and k+1 < nz, and is meshed iff all eight corners have
 * w >= min_weight.  It is cut into the six tetrahedra around its body diagonal: tetrahedron t has corners p0 = (0,0,0),
 * p1 = p0 + axis a, p2 = p1 + axis b, p3 = (1,1,1) for (a,b,c) = the permutations (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y),
 * (z,y,x), t = 0..5.  Every tetrahedron edge is one of the seven kinds above, taken from its lower corner, so neighbouring cells
 * agree on their shared face diagonals.
 * Triangles of a tetrahedron.  N is the set of corner indices 0..3 with tq < 0, ascending; P the rest, ascending.
 *   |N| = 0 or 4: no triangle
 *   |N| = 1, N = {a}:           one triangle on edges (a,P0), (a,P1), (a,P2)
 *   |N| = 3, P = {c}:           one triangle on edges (c,N0), (c,N1), (c,N2)
 *   |N| = 2, N = {a,b}, P = {c,d}: two triangles, (ac, ad, bd) then (ac, bd, bc)
 * Winding, a constant of (t, sign mask) independent of the data: with each vertex at the midpoint of its edge in the unit cell, the
 * order above is kept if ((v1-v0) x (v2-v0)) . (centroid(P) - centroid(N)) > 0 and the last two vertices are swapped otherwise (the
 * product is a non-zero integer in all 6 x 14 cases).  Normals therefore point towards free space, as the ray-cast's do.
 * Order of the triangle list: by cell n, then t, then first triangle before second.  v[] are ranks in the full vertex list;
 * cell = n.  Triangles with coincident vertices (tq == 0 gives s == 0) are emitted as any other: they keep the mesh closed.
 * Outputs.  d_counts[0] always receives the full vertex count and d_counts[1] the full triangle count.  Vertex records with index
 * >= vertex_capacity are not written.  Triangle records are written only if the vertex count <= vertex_capacity (a truncated
 * vertex list would make the indices meaningless), and only those with index < triangle_capacity.  Nothing else is written.
 * Capacity 0 with a NULL array asks for the counts only.  The result is the same bytes on every run: no atomic decides a place
 * (count per tile, one scan, the vertices, the triangles; a triangle finds its vertices' ranks by binary search of their ids).
 *
 * false, nothing queued and one "sgm_mi355x: sgm_volume_mesh: ..." line on stderr: a NULL s, spec, d_voxels or d_counts; an array
 * that is NULL with a capacity > 0; a spec outside the ranges (the limit above included); a min_weight outside 1..65535; an array
 * not 16-byte aligned, or d_voxels / d_counts not 4-byte aligned; outputs that overlap the volume or each other; a build without
 * the kernels.  Asynchronous on sgm_stream(s) and ordered as sgm_volume_points is.  It keeps 16 bytes of scratch per tile of 2048
 * voxels, reserved at its first call: an instance that never calls it allocates and launches exactly what it did before.  Not part
 * of it: vertex normals, colour, decimation, welding of coincident positions, row tiles. */
typedef struct { float x, y, z; uint32_t id; } sgm_mesh_vertex;      /* 16 bytes; id = n*8 + e */
typedef struct { uint32_t v[3]; uint32_t cell; } sgm_mesh_triangle;  /* 16 bytes; v = indices into the vertex list */
bool sgm_volume_mesh(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_voxels, uint32_t min_weight /* 1..65535 */,
                     sgm_mesh_vertex* d_vertices /* 16-byte aligned */, size_t vertex_capacity,
                     sgm_mesh_triangle* d_triangles /* 16-byte aligned */, size_t triangle_capacity,
                     uint32_t* d_counts /* [2]: vertices, triangles */);

/* ---- the TSDF volume ray-cast into depth and normal maps of any view ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/raycast_ref.py.  The third step of spatial
 * mapping (integrate, extract, render): the fused surface as an image -- the denoised depth of the current frame, a preview from a
 * virtual viewpoint, the model prediction of frame-to-model tracking.  Takes a volume as sgm_volume_integrate leaves it, a pinhole
 * view and one world -> camera pose per frame; per pixel it writes the depth Z of the first front-facing surface along the pixel's
 * ray and, optionally, the unit surface normal in camera coordinates.
 *
 * All arithmetic is float32, every operation rounded on its own (no contraction; divide and sqrt correctly rounded); the
 * parentheses are the contract; "finite" is tested on the bit pattern, before any comparison.  Per frame, R, t its pose (R[r][i] =
 * poses[3*r + i], t_r = poses[9 + r]); the camera centre and the ray directions in world coordinates:
 *   c_i = -((R[0][i]*t0 + R[1][i]*t1) + R[2][i]*t2)            i = 0,1,2        (R^T is a transposition, no arithmetic)
 * Per pixel (x, y):
 *   a = ((float)x - cx) / fx,   b = ((float)y - cy) / fy
 *   d_i  = (R[0][i]*a + R[1][i]*b) + R[2][i]                   world direction per unit of camera Z
 *   go_i = (c_i - origin_i) / voxel,   gd_i = d_i / voxel      grid units: voxel (i,j,k) covers [i,i+1) x [j,j+1) x [k,k+1)
 *   g(Z)_i = go_i + Z * gd_i
 * The march is in Z, not in ray length (the result is the depth itself; the stored distance is projective along Z as well):
 *   Z_k = z_min + (float)k * step,  k = 0, 1, ...  while Z_k <= z_max
 * The nearest sample at g = g(Z_k) is valid iff all three g_i are finite, 0 <= g_i < (float)n_i (tested in float before any
 * conversion) and the word of voxel (floorf g_x, floorf g_y, floorf g_z) has w >= min_weight; its sign is tq < 0, the crossing
 * rule of sgm_volume_points (zero counts as non-negative).  An invalid sample forgets the previous one.  Previous valid and
 * non-negative, current valid and negative: a front hit at k, the march ends.  Previous valid and negative, current valid and
 * non-negative: a back face, the march ends and the pixel is empty.  Reaching z_max without a hit leaves the pixel empty.
 * Refinement at a hit.  F(g) is the trilinear value of tq at h = g - 0.5f, i0 = floorf(h), f = h - i0 per axis; valid iff h is
 * finite, 0 <= i0 and i0 + 1 < n on every axis (in float) and all eight words have w >= min_weight;
 * lerp(p, q, s) = p + s*(q - p) on (float)tq, along x first, then y, then z.
 *   Fp = F(g(Z_{k-1})),  Fc = F(g(Z_k)),  den = Fp - Fc
 *   hit iff both are valid and den > 0;   s = fminf(fmaxf(Fp / den, 0), 1);   Z* = Z_{k-1} + s * step
 * Otherwise the pixel is empty and the march does not resume.  d_depth receives Z*; an empty pixel the quiet NaN 0x7FC00000, as in
 * the other 3-D units.  The normal (written only if d_normal != NULL), at g* = go + Z* * gd:
 *   nw_a = F(g* + e_a) - F(g* - e_a)  for the three unit steps   (g*_a + 1.0f and g*_a - 1.0f, then F's own - 0.5f)
 *   n_r  = (R[r][0]*nw_0 + R[r][1]*nw_1) + R[r][2]*nw_2
 *   len  = sqrtf((n_0*n_0 + n_1*n_1) + n_2*n_2)
 * If all six samples are valid and len is finite and > 0 the normal is n_r / len, else three quiet NaNs (the depth stays).  It
 * points out of the surface towards free space: n_z < 0 for a wall facing the camera.  An empty pixel gets three quiet NaNs.
 *
 * false, nothing queued and one "sgm_mi355x: sgm_volume_raycast: ..." line on stderr: a NULL s, vol, view, poses, d_voxels or
 * d_depth; a volume spec sgm_volume_integrate refuses; a view outside the ranges below; fx, fy not finite and > 0; cx, cy not
 * finite; z_min NaN or < 0; z_max not finite or not > z_min; step not finite or not > 0; (z_max - z_min) / step >= 65536 (in
 * double: k fits and a launch is bounded); a min_weight outside 1..65535; a non-finite pose entry; a pointer not aligned to its
 * element; an output that overlaps the volume or the other output; a build without the kernel.  poses is a HOST pointer, read
 * before the call returns; the others are device pointers.  Asynchronous on sgm_stream(s), ordered as sgm_volume_points is (behind
 * the last match also with sgm_set_overlap_post).  No scratch; nothing outside the two output arrays is written; an instance that
 * never calls it allocates and launches exactly what it did before; one lane per pixel with no dependence between lanes, so the
 * result is the same on every run and one call over B frames equals B calls of one frame.  Not part of it: adaptive step lengths,
 * shading and colour, pose estimation (sgm_track below tracks a frame against these maps), row tiles. */
typedef struct {            /* 44 bytes, every field 4 bytes, no padding */
    int32_t  width, height, frames;   /* 1..65535 each for width/height; 1 <= frames <= 64; frames*width*height <= 2^31 */
    float    fx, fy, cx, cy;          /* pinhole of the view */
    float    z_min, z_max, step;      /* march Z = z_min + k*step while Z <= z_max; units of the volume */
    uint32_t min_weight;              /* 1..65535: a voxel counts iff w >= min_weight */
} sgm_raycast_spec;
bool sgm_volume_raycast(sgm_instance* s, const sgm_volume_spec* vol, const sgm_raycast_spec* view,
                        const float* poses /* HOST [frames][12], R row-major then t, world -> camera, as sgm_volume_integrate */,
                        const uint32_t* d_voxels, float* d_depth /* [frames][height][width] */,
                        float* d_normal /* [frames][height][width][3], may be NULL */);

/* ---- frame-to-model tracking: projective point-to-plane ICP against the ray-cast ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/track_ref.py.  The step that makes spatial
 * mapping work without an outside tracker: given the depth of the current frame and the depth and normal maps sgm_volume_raycast
 * rendered from the last known pose, it estimates the rigid motion between the two, so that a caller can run match -> track ->
 * integrate -> ray-cast on the device.  Conventions are registration's: a pose is [12], R row-major, then t, P' = R P + t.  The
 * tracked pose maps the SOURCE camera (the rectified reference camera of the current frame) into the MODEL camera (the view the
 * maps were ray-cast from).
 *
 * Inputs.  The contributing pixels are the KEPT pixels of the cloud contract above (src, d_disp, d_mask, d_conf) with their cloud
 * X, Y, Z.  The model maps are d_model_depth f32 [frames][mh][mw] and d_model_normal f32 [frames][mh][mw][3] as sgm_volume_raycast
 * writes them (width = mw, height = mh and the pinhole of sgm_track_spec); the model view may differ in size and pinhole from the
 * source.  Frame f of the source meets frame f of the model under pose f.
 * Per source pixel of frame f.  All arithmetic is float32, every operation rounded on its own (no contraction, correctly rounded
 * divide); the parentheses are the contract; "finite" is tested on the bit pattern, before any comparison:
 *   Px = ((R0*X + R1*Y) + R2*Z) + t0          (Py with R3..5, t1;  Pz with R6..8, t2;  R, t of frame f)
 *   skip unless Pz is finite and Pz > 0
 *   u = fx*(Px/Pz) + cx,  v = fy*(Py/Pz) + cy;   skip unless both finite
 *   uf = floorf(u + 0.5f), vf = floorf(v + 0.5f); skip unless 0 <= uf < (float)width && 0 <= vf < (float)height, tested in float
 *   Zm = model_depth[f][vf][uf];  skip unless Zm is finite and Zm > 0
 *   n  = model_normal[f][vf][uf][0..2];  skip unless all three are finite
 *   Q  = (((uf - cx)*Zm)/fx, ((vf - cy)*Zm)/fy, Zm)
 *   e  = Q - P;   skip unless (e0*e0 + e1*e1) + e2*e2 is finite and <= dist_max*dist_max   (the right side rounded once to float)
 *   r  = (n0*e0 + n1*e1) + n2*e2
 *   c  = P x n:   c0 = Py*n2 - Pz*n1,  c1 = Pz*n0 - Px*n2,  c2 = Px*n1 - Py*n0
 *   v[0..6] = c0/span, c1/span, c2/span, n0, n1, n2, r/dist_max
 *   skip unless every v_i is finite and |v_i| <= 8.0f
 *   q_i = (int32)rintf(v_i * 65536.0f)              (the product is exact; round half to even; |q_i| <= 2^19)
 * A pixel that was not skipped is ASSOCIATED.  Why these seven: moving P by w x P + v changes r by -(P x n).w - n.v, so the row of
 * the Jacobian of the six unknowns (w, v) is J = [P x n, n] and J xi = r is the linearised point-to-plane equation; span and
 * dist_max bring the three kinds of entries to order one before they are quantised.
 * Sums.  The result of frame f is int64 sums[f][29]: sums[k], k = 0..27, is the sum over the associated pixels of q_i*q_j for
 * (i, j), i <= j, in row-major order of the upper triangle of the 7 x 7 matrix ((0,0) (0,1) .. (0,6) (1,1) .. (6,6)); sums[28] is
 * the number of associated pixels.  Bound: |q_i| <= 2^19, so a term is at most 2^38; the entry points refuse a source of more
 * than 2^24 pixels per frame (width * height > 2^24), so a sum stays at or below 2^62 and no addition overflows int64.
 * Determinism: the sums are exact integers, so any order of addition gives the same bytes; the result is the same on every run and
 * one call over B frames equals B calls of one frame.
 *
 * The step (sgm_track_solve; host only, double, every operation rounded on its own, no contraction).  sums(i, j), i <= j, is the
 * entry of the pair.  status 1 (too few pixels) if sums[28] < min_pixels.  Else A_ij = A_ji = (double)sums(i, j) for i <= j < 6,
 * b_i = (double)sums(i, 6), and A xi = b is solved by LDL^T without square roots, columns j = 0..5 left to right; every inner sum
 * starts at 0.0 and adds its terms in index order k = 0, 1, ..:
 *   D_j  = A_jj - sum_{k<j} (L_jk*L_jk)*D_k
 *   status 2 (degenerate) unless D_j is finite and D_j > min_pivot * A_jj
 *   L_ij = (A_ij - sum_{k<j} (L_ik*L_jk)*D_k) / D_j                for i = j+1..5
 * then  y_i = b_i - sum_{k<i} L_ik*y_k   (i = 0..5),   z_i = y_i / D_i,   xi_i = z_i - sum_{k=i+1..5} L_ki*xi_k   (i = 5..0).
 * status 2 as well if an xi_i or an entry of the stepped pose is not finite.  The motion, with dist_max and span as doubles:
 *   w_i = xi_i * (dist_max / span),   v_i = xi_{3+i} * dist_max                     i = 0, 1, 2
 * and the rotation is the Cayley map of s = w * 0.5 -- only + - * /, no libm, so numpy and C give the same bits:
 *   ss = (s0*s0 + s1*s1) + s2*s2,   a = 1 - ss,   den = 1 + ss
 *   X  = [s]x:  X01 = -s2, X02 = s1, X10 = s2, X12 = -s0, X20 = -s1, X21 = s0, X_rr = 0
 *   Ri_rc = ((a*I_rc + 2*(s_r*s_c)) + 2*X_rc) / den                                 (I the identity, as 1.0 and 0.0)
 *   R'_rc = (Ri_r0*R_0c + Ri_r1*R_1c) + Ri_r2*R_2c,    t'_r = ((Ri_r0*t0 + Ri_r1*t1) + Ri_r2*t2) + v_r
 * Ri is a rotation exactly in real arithmetic and to rounding here.  stats: pixels = sums[28]; rms = dist_max * sqrt((double)
 * sums[27] / (double)sums[28]) / 65536 (0 without pixels), the root mean square of the point-to-plane residuals that went into the
 * sums, in the units of dist_max; status 0 (pose_out is the stepped pose), 1 or 2 (pose_out is pose_in).
 *
 * sgm_track_sums: asynchronous on sgm_stream(s), ordered as sgm_volume_raycast is (behind the last match also with
 * sgm_set_overlap_post; a ray-cast queued before it on the same instance is finished when it reads the maps).  poses is a HOST
 * pointer, [src->frames][12] float, read before the call returns (the poses travel as kernel arguments: 1..64 frames); d_sums is a
 * device pointer, int64 [frames][29], 8-byte aligned, zeroed on the stream inside the call; the other pointers are device pointers
 * that need no alignment beyond their element's (a map that cannot be read 16 bytes at a time takes a one-pixel-per-lane path with
 * the same result).  d_disp == NULL: the instance's last final map, under the cloud entry points' rules.  Nothing outside d_sums
 * is written and there is no scratch.
 * sgm_track (blocking): model->iterations rounds of { one sgm_track_sums launch for all frames into a buffer of the instance's own
 * (232 bytes per frame, reserved at the first call), that buffer copied to the host, sgm_track_solve per frame }.  poses is a HOST
 * pointer, [frames][12] double: in, the guess; out, the estimate.  The kernel receives each pose rounded once to float32; the
 * solve steps the double pose.  A frame whose solve does not return status 0 keeps its pose, records that status and sits out the
 * remaining rounds (the launches still cover it, at the pose it kept).  stats[f]: the stats of the last solve made for frame f.
 * trace_sums (HOST, int64 [iterations][frames][29], or NULL) receives the sums of every round, trace_poses (HOST, double
 * [iterations + 1][frames][12], or NULL) the poses before the first round and after every round.
 * sgm_track_world_pose (host only): out = rel^-1 o model_pose, the world -> camera pose of the tracked frame, ready for
 * sgm_volume_integrate, for model_pose the world -> camera pose the maps were ray-cast from and rel the tracked pose.  In double,
 * rel^-1 taken as (R^T, -R^T t), every result rounded once to float:
 *   out_R[r][c] = (Rr[0][r]*Rm[0][c] + Rr[1][r]*Rm[1][c]) + Rr[2][r]*Rm[2][c]
 *   out_t[r]    = (Rr[0][r]*(tm0 - tr0) + Rr[1][r]*(tm1 - tr1)) + Rr[2][r]*(tm2 - tr2)
 *
 * false, nothing queued and one "sgm_mi355x: <entry point>: ..." line on stderr: a NULL pointer other than d_disp, d_mask, d_conf
 * and the traces; a src outside the cloud spec's ranges, with more than 64 frames or with width * height > 2^24; a model outside
 * the ranges below; a pose entry that is not finite (for sgm_track: also after rounding to float); a pointer not aligned as
 * said; a d_sums that overlaps a map; a sums[28] outside 0..2^24, which no launch gives (sgm_track_solve); a build without the
 * kernel (sgm_track_sums, sgm_track).  An instance that never calls these entry points allocates and launches exactly what it did
 * before.  Not part of it: image pyramids (a caller can ray-cast and match at a lower scale), robust weights beyond the distance
 * gate, normals of the source frame and a normal-angle gate, photometric terms, loop closure, row tiles, sgm_match_planes. */
typedef struct {            /* 44 bytes, every field 4 bytes, no padding */
    int32_t  width, height;           /* the model maps, 1..65535 each */
    float    fx, fy, cx, cy;          /* pinhole of the model view; fx, fy finite and > 0, cx, cy finite */
    float    dist_max;                /* finite, > 0: the association gate and the unit of the residual */
    float    span;                    /* finite, > 0: the length that normalises the rotational Jacobian; about the scene depth */
    int32_t  iterations;              /* 1..64: rounds of sgm_track */
    uint32_t min_pixels;              /* at least 6: fewer associated pixels are status 1 */
    float    min_pivot;               /* finite, >= 0: a pivot D_j <= min_pivot * A_jj is status 2 */
} sgm_track_spec;
typedef struct { double rms; uint32_t pixels; int32_t status; } sgm_track_stats;   /* 16 bytes; status 0 ok, 1 too few pixels, 2 degenerate */
bool sgm_track_sums(sgm_instance* s, const sgm_cloud_spec* src, const sgm_track_spec* model,
                    const float* poses /* HOST [frames][12], source camera -> model camera; read before return */,
                    const float* d_disp, const uint8_t* d_mask, const uint16_t* d_conf,
                    const float* d_model_depth, const float* d_model_normal,
                    int64_t* d_sums /* device, [frames][29], 8-byte aligned */);
bool sgm_track_solve(const sgm_track_spec* model, const int64_t sums[29], const double pose_in[12], double pose_out[12],
                     sgm_track_stats* stats);                                        /* host only */
bool sgm_track(sgm_instance* s, const sgm_cloud_spec* src, const sgm_track_spec* model,
               double* poses /* HOST [frames][12]; in: the guess, out: the estimate */,
               const float* d_disp, const uint8_t* d_mask, const uint16_t* d_conf,
               const float* d_model_depth, const float* d_model_normal,
               sgm_track_stats* stats /* HOST [frames] */,
               int64_t* trace_sums /* HOST [iterations][frames][29], or NULL */,
               double* trace_poses /* HOST [iterations + 1][frames][12], or NULL */);
bool sgm_track_world_pose(const float model_pose[12], const double rel[12], float out[12]);   /* host only */

/* ---- colour in the TSDF volume: fused with the depth, ray-cast with it, given to the mesh ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/color_ref.py.  The entry points above carry
 * geometry only; these three carry the reference camera's image along, so that the fused model is the left image on the surface: a
 * rendered preview that looks like a picture, a mesh a viewer shows in colour.  Each is the twin of a plain entry point and leaves
 * that one's outputs exactly as the plain call leaves them.  Float arithmetic follows the sections above: float32, every operation
 * rounded on its own, no contraction, "finite" tested on the bit pattern; the averages are exact integers; no atomics, the same
 * bytes on every run.
 *
 * The colour volume.  A second caller-owned device array of nx * ny * nz uint32 words, indexed like the TSDF words, each
 *   (cw << 24) | (b << 16) | (g << 8) | r
 * with cw an 8-bit weight of its own.  All-zero bytes mean "no colour anywhere"; its size is sgm_volume_bytes(spec); there is no
 * clear entry point (hipMemset it, as for the TSDF words).
 *
 * sgm_volume_integrate_color.  d_image is the reference camera's image, registered to the disparity map, [frames][height][width]:
 * channels == 1: uint8 grey, taken as r = g = b;  channels == 4: uint32 per pixel, r | g << 8 | b << 16, the top byte ignored,
 * the pointer 4-byte aligned.  d_voxels is updated exactly as sgm_volume_integrate updates it, word for word (d_disp == NULL: the
 * instance's last final map, under the same rules).  For voxel and frame f the colour word changes iff frame f updated the voxel's
 * TSDF word under every rule of the volume contract AND sdf <= trunc (tested in float: a voxel far in front of the surface gets
 * distance but no colour).  Then, with p the channel value of the source pixel (f, vf, uf) that gave Z, per channel
 *   c = floor_div(2*(c*cw + p) + (cw + 1), 2*(cw + 1))       (all operands non-negative, below 2^31: rounded, halves up)
 * and then
 *   cw = min(cw + 1, min(max_weight, 255))
 * Frames take effect in order; one call over B frames equals B calls of one frame, bit for bit, in both arrays; a launch reads and
 * writes each word of either array at most once (the lane that owns a voxel owns its colour word; it stores the colour words only
 * where one changed).  Both arrays are accessed 16 bytes at a time where nx % 4 == 0 and both pointers allow it, else one voxel per
 * lane, with the same results.
 *
 * sgm_volume_raycast_color.  d_depth and d_normal (may be NULL) receive exactly the bytes sgm_volume_raycast writes.  d_rgba is
 * uint32 [frames][height][width]: 0 for an empty pixel; at a hit, with g* = go + Z* * gd, the first of these rules that applies:
 *   trilinear   the eight voxels of F(g*): h = g* - 0.5f, i0 = floorf(h), f = h - i0, the same in-grid test in float.  Valid iff
 *               all eight colour words have cw >= 1 (the TSDF weight is not asked again).  Per channel, on (float)c,
 *               lerp(p, q, s) = p + s*(q - p) along x, then y, then z;   v = (unsigned)rintf(fminf(fmaxf(value, 0), 255));
 *               the pixel is 0xFF000000 | b << 16 | g << 8 | r
 *   nearest     the voxel (floorf g*_x, floorf g*_y, floorf g*_z), where all three g*_i are finite and 0 <= g*_i < (float)n_i (the
 *               march's own admission test, in float): if its cw >= 1, its colour with alpha 0xFF
 *   else        0
 *
 * sgm_volume_colors: colours for a list the volume produced.  d_records are 16-byte records with the id in the last word:
 * id_kinds == 8: sgm_mesh_vertex, id = n*8 + e, edge kinds 0..6;  id_kinds == 4: sgm_surface_point, id = n*4 + a, axes 0..2.
 * Only the id is read.  Record r is handled iff r < capacity and (d_count == NULL or r < d_count[0]); nothing is written for the
 * other records, so the call can be queued straight behind sgm_volume_mesh (d_count = its d_counts) or sgm_volume_points without
 * reading the count back.  d_rgba is uint32 [capacity].  The edge (n, e) of a record, with far voxel m (the (dx,dy,dz) table of
 * the mesh contract), is valid iff n < nx*ny*nz, e names a kind and m is inside the grid; otherwise d_rgba[r] = 0.  Else
 *   den = (float)tq[n] - (float)tq[m];   s = den != 0 ? fminf(fmaxf((float)tq[n] / den, 0), 1) : 0
 *   both ends have cw >= 1:      per channel rintf(lerp(c_n, c_m, s)), alpha 0xFF
 *   exactly one end has colour:  that end's colour, alpha 0xFF
 *   neither:                     0
 * One launch, one lane per record, no scratch.
 *
 * All three: poses is a HOST pointer as in the plain twins; the others are device pointers.  Asynchronous on sgm_stream(s), behind
 * the last match also with sgm_set_overlap_post, as their twins.  false, nothing queued and one "sgm_mi355x: <entry point>: ..."
 * line on stderr: everything the plain twin refuses (sgm_volume_colors: a NULL s, spec, d_voxels or d_colors; a spec outside the
 * volume's ranges; with id_kinds 8 a spec over the mesh's 2^27 voxels; a capacity above 2^32); a NULL d_image, d_colors or d_rgba
 * (sgm_volume_colors: a NULL d_records or d_rgba with capacity > 0); channels other than 1 or 4; id_kinds other than 4 or 8; a
 * d_image (with channels 4), d_colors, d_rgba or d_count that is not 4-byte aligned, d_records not 16-byte aligned; d_colors that
 * overlaps d_voxels, the image or a map (integration); d_rgba that overlaps the volume, the colours or another output (ray-cast);
 * an output that overlaps an input (sgm_volume_colors); a build without the kernel.  capacity == 0 is a successful no-op.  An
 * instance that never calls these entry points allocates and launches exactly what it did before.  Not part of it: colour spaces
 * and gamma (the bytes are averaged as they are), shading, textures and texture atlases, per-triangle colour, a second camera's
 * image (register it first: sgm_register_gather), row tiles, sgm_match_planes. */
bool sgm_volume_integrate_color(sgm_instance* s, const sgm_volume_spec* spec, const sgm_cloud_spec* src,
                                const float* poses /* HOST, [src->frames][12], as sgm_volume_integrate */,
                                const float* d_disp, const uint8_t* d_mask, const uint16_t* d_conf,
                                const void* d_image /* [frames][height][width] u8 or u32 */, int channels /* 1 or 4 */,
                                uint32_t* d_voxels, uint32_t* d_colors);
bool sgm_volume_raycast_color(sgm_instance* s, const sgm_volume_spec* vol, const sgm_raycast_spec* view,
                              const float* poses /* HOST [frames][12], as sgm_volume_raycast */,
                              const uint32_t* d_voxels, const uint32_t* d_colors, float* d_depth /* [frames][height][width] */,
                              float* d_normal /* [frames][height][width][3], may be NULL */, uint32_t* d_rgba /* [frames][height][width] */);
bool sgm_volume_colors(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_voxels, const uint32_t* d_colors,
                       const void* d_records /* 16-byte records, id in the last word */, size_t capacity,
                       const uint32_t* d_count /* device u32, may be NULL */, int id_kinds /* 8 or 4 */, uint32_t* d_rgba /* u32 [capacity] */);

/* ---- a window of the TSDF volume: a volume that follows the rig and streams out what leaves ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/window_ref.py.  A volume is a dense array with a
 * fixed origin: at 5 cm voxels the largest box is 51 m long, and a car crosses it in seconds.  Every entry point above takes the
 * volume spec per call, so one primitive makes the volume move: copy a box of the voxel lattice into another volume array at an
 * integer voxel offset, zero-filling what was never observed.  Shifting the volume so that the rig stays centred is one call, what
 * is about to fall off the edge is handed out as a small volume of its own by one call per slab, and the same call grows, crops or
 * re-allocates a volume without losing it.  Tolerance 0: words are copied.
 *
 * sgm_volume_window.  The destination is a volume of dims[0] x dims[1] x dims[2] voxels, indexed like every volume.
 *   copy rule   destination voxel (i, j, k), 0 <= i < dims[0], 0 <= j < dims[1], 0 <= k < dims[2], receives the source word of
 *               (i + offset[0], j + offset[1], k + offset[2]) if that lies inside the source grid, otherwise 0, the empty voxel
 *   colours     with d_src_colors and d_dst_colors (both or neither) the colour words travel the same way in the same launch
 *   writes      every destination word is written exactly once; nothing else is written; the source is only read
 *   the spec    voxel, trunc and max_weight are the source's;  nx, ny, nz = dims;
 *               origin_a = src.origin_a + (float)offset_a * src.voxel        (float32: the product, then the sum, each rounded once)
 *               It is written to *dst_out (HOST, may be NULL) and is what sgm_volume_window_spec (host only) gives.
 * The consequence of the origin's rule: if voxel is a power of two and the origin a multiple of it (and the numbers stay within
 * float32's 24 bits), every origin made this way is exact, the voxel centres of source and window are the same floats, and whatever
 * is computed in the window -- an integration, a mesh, a ray-cast -- is word for word what it would have been in the source.
 * Otherwise the centres agree to rounding, and results computed in the window may differ from the source's in isolated words.
 * One launch, no scratch, no atomics: the same bytes on every run.  Four voxels per lane and 16-byte stores where dims[0] % 4 == 0
 * and the destination arrays can be accessed 16 bytes at a time, 16-byte loads where src->nx % 4 == 0, offset[0] % 4 == 0 and
 * the source arrays allow it; else element by element, with the same bytes.  Asynchronous on sgm_stream(s), behind the last match
 * also with sgm_set_overlap_post, as sgm_volume_points.  false, nothing queued and one "sgm_mi355x: sgm_volume_window: ..." line
 * on stderr: a NULL s, src, offset, dims, d_src_voxels or d_dst_voxels; exactly one of the two colour arrays NULL; a source spec
 * that sgm_volume_integrate refuses; dims that do not make a spec it accepts (1..1024 each, product <= 2^30); |offset_a| > 2^20; a
 * resulting origin that is not finite; a pointer that is not 4-byte aligned; a destination array that overlaps any other of the
 * four arrays (so there is no in-place call: keep two arrays and alternate); a build without the kernel.  An instance that never
 * calls it allocates and launches exactly what it did before.
 *
 * sgm_volume_follow (host only): the shift, in voxels, that brings the rig back to the middle of the volume.  In double, every
 * operation on its own, sums left to right; pose is world -> camera (R row-major, then t):
 *   the point to keep centred is (0, 0, focus_z) in camera coordinates: the camera centre for 0, or the middle of the viewed depths
 *   P_i     = (R[0][i]*(0 - t0) + R[1][i]*(0 - t1)) + R[2][i]*(focus_z - t2)                  (the point in the world)
 *   g_a     = (P_a - origin_a) / voxel - n_a / 2                                              (n_a / 2 in double: 16.5 for 33)
 *   shift_a = 0 if |g_a| <= margin, else granule * floor(g_a / granule + 0.5)
 * false and a line on stderr: a NULL argument, a spec outside the volume's ranges, granule < 1, margin < 0, a pose entry or focus_z
 * that is not finite, |g_a| >= 2^20, a shift that rounds to more than 2^20.  A granule that is a multiple of 4 keeps offset[0], and
 * with nx % 4 == 0 the whole shift, on the window's 16-byte load path.
 *
 * sgm_volume_leaving (host only): the parts of the volume that the shift drops, as at most three boxes to hand to sgm_volume_window.
 * Per axis a, with c = n_a - 1 the cells on that axis (a cell is the cube between eight neighbouring voxels) and s = shift_a:
 *   s > 0:  the cells [0, min(s, c)) leave and [min(s, c), c) stay
 *   s < 0:  the cells [max(c + s, 0), c) leave and [0, max(c + s, 0)) stay
 *   s = 0:  none leave and [0, c) stay
 * Box a is the stay range on the axes before a, the leave range on a, and all cells on the axes after; it exists iff all three
 * ranges are non-empty.  It is reported in voxels: lo holds the range starts and n the lengths + 1, so that its last cells are
 * whole.  The boxes come in axis order, absent ones skipped; the return value is their number, 0..3, or -1 (and a line on stderr)
 * for a NULL argument or a refused spec.  The boxes are disjoint in cells, and together with the stay ranges they cover every cell
 * of the volume exactly once: the meshes of what leaves and of what stays tile the mesh of the whole, without gaps or duplicates.
 *
 * The caller's loop, with two arrays A and B of sgm_volume_bytes(spec) (and two of colours) that alternate:
 *   1. sgm_volume_follow(spec, pose, focus_z, granule, margin, shift);  all zero: nothing to do
 *   2. for each box of sgm_volume_leaving(spec, shift, boxes): sgm_volume_window(s, spec, box.lo, box.n, A, ..., small, ..., &part)
 *   3. sgm_volume_mesh / sgm_volume_colors (or sgm_volume_points) on each small array under its spec `part`: the streamed surface
 *   4. sgm_volume_window(s, spec, shift, (nx, ny, nz), A, ..., B, ..., &spec);  swap A and B;  integrate the next frames into A
 * Not part of it: ring-buffer addressing inside the kernels above, shifting in place, voxel hashing, welding the seams between
 * streamed meshes (vertices on a shared face appear in both parts, with equal positions), loop closure. */
typedef struct { int32_t lo[3]; int32_t n[3]; } sgm_volume_box;      /* voxels: a box of n cells-plus-one starting at lo; 24 bytes */
bool sgm_volume_window(sgm_instance* s, const sgm_volume_spec* src, const int32_t offset[3], const int32_t dims[3],
                       const uint32_t* d_src_voxels, const uint32_t* d_src_colors /* or NULL */,
                       uint32_t* d_dst_voxels, uint32_t* d_dst_colors /* NULL iff d_src_colors is */,
                       sgm_volume_spec* dst_out /* HOST, may be NULL */);
bool sgm_volume_window_spec(const sgm_volume_spec* src, const int32_t offset[3], const int32_t dims[3], sgm_volume_spec* dst); /* host only */
bool sgm_volume_follow(const sgm_volume_spec* spec, const float pose[12] /* world -> camera */, float focus_z,
                       int32_t granule /* >= 1 */, int32_t margin /* >= 0, voxels */, int32_t shift[3]);
int  sgm_volume_leaving(const sgm_volume_spec* spec, const int32_t shift[3], sgm_volume_box boxes[3]);   /* 0..3, -1 refused */

/* ---- the distance field of the TSDF volume: the exact Euclidean distance transform of its voxel lattice ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/distance_ref.py.  What a planner reads from a map
 * is the clearance of a voxel: its distance to the nearest obstacle.  The stored tq cannot serve: it is projective along the camera's
 * Z, truncated at trunc, and undefined where no frame looked.  sgm_volume_distance computes, per voxel, the squared Euclidean distance
 * in voxels to the nearest site of the lattice -- exact integers, tolerance 0 -- and sgm_volume_distance_field turns the words of one
 * or both sides into a metric, optionally signed, float field.
 *
 * Sites.  For a voxel word, w = word >> 16 and tq = (int16_t)word.
 *   observed    w >= min_weight
 *   occupied    observed and tq < 0   (the sign rule of sgm_volume_points; zero counts as non-negative)
 *   O           the obstacle set: the occupied voxels, and with unknown == 1 the voxels that are not observed
 *   side 0      the sites are O;   side 1: the sites are every voxel of the grid that is not in O
 * Nothing exists outside the grid: there are no sites there, on either side.
 *
 * sgm_volume_distance.  d_dist2 holds one uint16_t per voxel, indexed like the volume.  For voxel p = (pi, pj, pk)
 *   m = min over sites q of (pi-qi)^2 + (pj-qj)^2 + (pk-qk)^2                                         (an exact integer)
 *   the word written is m if a site exists and m <= r*r, otherwise SGM_DISTANCE_FAR; a site gets 0
 * Every word of d_dist2 is written exactly once per call as far as a reader can tell (the result does not depend on what it held),
 * nothing else is written, the volume is only read, and the result is the same bytes on every run.  The transform is separable --
 * along x the nearest site of the row, then along y and along z out[j] = min over |o| <= r of g[j+o] + o*o -- and runs as three
 * passes over d_dist2 itself: a workgroup owns whole lines, holds them in LDS and stores them in place.  An intermediate above r*r
 * can never become a result and is FAR at once, so every value fits 16 bits.  The call allocates nothing: no instance scratch and
 * no second array.  No atomics.
 *
 * sgm_volume_distance_field.  float32, every operation rounded on its own, sqrtf correctly rounded (as the ray-cast needs it).  With
 * o the word of side 0 (d_out2) and i the word of side 1 (d_in2, which may be NULL: an unsigned field):
 *   o == FAR                              +INFINITY
 *   o > 0                                 spec->voxel * sqrtf((float)o)
 *   o == 0 and (d_in2 == NULL or i == 0)  0.0f
 *   o == 0 and i == FAR                   -INFINITY
 *   o == 0 otherwise                      -(spec->voxel * sqrtf((float)i))
 * Distances are between voxel centres: the surface lies between an occupied voxel and its free neighbour, so against the true
 * surface the field is biased by up to half a voxel (the outside reads too far, the inside too deep, each by half a voxel along an
 * axis); a planner that needs a bound subtracts voxel * sqrt(3) / 2.  One launch, one lane per voxel, or four with a 16-byte store
 * where nx % 4 == 0 and the pointers allow it; no scratch, no atomics.
 *
 * Both calls are asynchronous on sgm_stream(s), behind the last match also with sgm_set_overlap_post, as sgm_volume_points.  false,
 * nothing queued and one "sgm_mi355x: sgm_volume_distance: ..." (or "sgm_volume_distance_field: ...") line on stderr: a NULL s, spec,
 * dist, d_voxels, d_dist2, d_out2 or d_field; a volume spec that sgm_volume_integrate refuses; a min_weight outside 1..65535; a radius
 * outside 1..255; a side or unknown other than 0 or 1; a pointer that is not aligned to its element; an output that overlaps any
 * input; a build without the kernels.  It composes with the window: sgm_volume_window crops the region of interest first (a window
 * with a margin of r voxels around a box gives, on that box, the source's distances), and a moving volume recomputes its field after
 * a shift.  An instance that never calls these allocates and launches exactly what it did before.
 * Not part of it: incremental update of a field after an integration, the identity of the nearest site, a radius above 255, 2-D
 * cost maps, queries at arbitrary points (interpolation is the caller's). */
#define SGM_DISTANCE_FAR 0xFFFFu
typedef struct {            /* 16 bytes, every field 4 bytes, no padding */
    uint32_t min_weight;    /* 1..65535: a voxel is observed iff w >= min_weight */
    int32_t  radius;        /* r, voxels, 1..255: r*r <= 65025 < SGM_DISTANCE_FAR */
    int32_t  side;          /* 0: distance to the obstacle set; 1: distance to its complement */
    int32_t  unknown;       /* 0: unobserved voxels are not obstacles; 1: they are */
} sgm_distance_spec;
size_t sgm_volume_distance_bytes(const sgm_volume_spec* spec);   /* host only; 2 * nx*ny*nz, 0 for a refused spec */
bool sgm_volume_distance(sgm_instance* s, const sgm_volume_spec* spec, const sgm_distance_spec* dist,
                         const uint32_t* d_voxels, uint16_t* d_dist2);
bool sgm_volume_distance_field(sgm_instance* s, const sgm_volume_spec* spec,
                               const uint16_t* d_out2, const uint16_t* d_in2 /* or NULL */, float* d_field);

/* ---- planes in a point list: exact votes on the device, an integer fit ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/plane_ref.py.  Everything above stops at raw
 * geometry; this answers the first question asked of it: where is the floor, where are the walls, which points stand on them.
 * A point list is what sgm_cloud_points, sgm_volume_points and sgm_volume_mesh (its vertices) write: 16-byte records
 * { float x, y, z; uint32 tag } -- sgm_point, sgm_surface_point, sgm_mesh_vertex; the tag is never read -- with an optional device
 * count word, so that a call can be queued behind the list's own call without reading the count back.  Throughout,
 *   n = min(capacity, d_count[0])     (capacity where d_count == NULL)
 * and a record r < n TAKES PART iff x, y, z are finite and it is unlabelled (d_labels == NULL || d_labels[r] == 0).
 *
 * All device arithmetic is float32, every operation rounded on its own (no contraction; divide and sqrt correctly rounded); the
 * parentheses are the contract; "finite" is tested on the bit pattern, before any comparison.
 * A plane (sgm_plane) is normal . (P - anchor) = 0 with offset = -(normal . anchor) carried along; a VOID plane has an all-zero
 * normal (either sign of zero) and, as the entry points write it, 32 zero bytes.  A void plane has no inliers.
 * The vote rule.  A record that takes part is an INLIER of a non-void plane iff
 *   s = ((n0*(x - a0) + n1*(y - a1)) + n2*(z - a2))     is finite and |s| <= dist
 *
 * Candidates (sgm_plane_votes).  Candidate k = 0 .. hypotheses-1 takes the records i_j = ((uint64)h(seed, k, j) * n) >> 32,
 * j = 0, 1, 2, with the uint32 mix (every operation modulo 2^32; no modulo by n, no float)
 *   h(seed, k, j):  x = (seed ^ (k * 0x9E3779B9)) ^ ((j + 1) * 0x85EBCA6B)
 *                   x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 * It is void where two of the three indices coincide (so always for n < 3; no record is read then) or a chosen record does not
 * take part.  Else, with P0, P1, P2 the records:
 *   u = P1 - P0,  v = P2 - P0                                   (per coordinate)
 *   c0 = u1*v2 - u2*v1,  c1 = u2*v0 - u0*v2,  c2 = u0*v1 - u1*v0
 *   len2 = (c0*c0 + c1*c1) + c2*c2;   void unless len2 is finite and len2 > 0
 *   len = sqrtf(len2);   n_i = c_i / len;   void unless every n_i is finite and not all are zero
 *   t = (n0*P0x + n1*P0y) + n2*P0z;   void unless t is finite
 *   with a prior (axis not all zero):  d = (n0*axis0 + n1*axis1) + n2*axis2;  void unless d is finite;
 *                                      if d < 0: n = -n, t = -t, d = -d;   void unless d >= thr,
 *                                      thr = min_cos * sqrtf((axis0*axis0 + axis1*axis1) + axis2*axis2)     (float32, as written)
 *   without:                           if t > 0: n = -n, t = -t                                            (so that offset >= 0)
 *   normal = n,  offset = 0.0f - t,  anchor = P0,  votes = 0
 * The candidates are written to d_planes by a small launch of their own; the vote launch that follows adds to their votes.
 * Votes.  votes of a non-void candidate = the number of its inliers among the records r < n, exact (modulo 2^32, which only
 * n = 2^32 can reach).  A void candidate keeps its 32 zero bytes.  Integer sums: the same bytes on every run.
 * Best (sgm_plane_best).  d_best receives the non-void candidate with the most votes, ties to the smallest k; a void plane where
 * every candidate is void.
 * Sums (sgm_plane_sums).  Over the inliers of *d_plane, per coordinate i:
 *   e_i = (P_i - anchor_i) / span;   skip the record unless every e_i is finite and |e_i| <= 8.0f
 *   q_i = (int32)rintf(e_i * 65536.0f)                        (the product is exact; round half to even; |q_i| <= 2^19)
 * d_sums[0..9] is the upper triangle of the 4 x 4 moment matrix of (q_x, q_y, q_z, 1) in row-major order: sum of q_x*q_x, q_x*q_y,
 * q_x*q_z, q_x, q_y*q_y, q_y*q_z, q_y, q_z*q_z, q_z, 1; the last is the number of records that were not skipped.  Bound: a term
 * is at most 2^38 and the entry points refuse capacity > 2^24, so a sum stays at or below 2^62 and no addition overflows int64;
 * exact integers, so the order of addition does not show.
 * Labels (sgm_plane_label).  d_labels[r] = label for every inlier of *d_plane (an inlier is unlabelled by definition); no other
 * byte is written.  Label the floor, vote again: the second plane.  The records still 0 afterwards are the obstacle points.
 *
 * The fit step (sgm_plane_solve; host only, double, every operation rounded on its own, no contraction, no libm beyond sqrt).
 * Sxx .. N name the ten sums in their order (Sxx Sxy Sxz Sx Syy Syz Sy Szz Sz N) as doubles, M the symmetric 3 x 3 matrix of the
 * second moments and m = (Sx, Sy, Sz).  status 1 (too few inliers) if N < min_inliers.  Else, from plane_in (n, A as doubles):
 *   w = n / sqrt((n0*n0 + n1*n1) + n2*n2)
 *   e = the unit vector of the axis with the smallest |w_i|, ties to the lowest index
 *   t1 = c / sqrt((c0*c0 + c1*c1) + c2*c2),  c = w x e;     t2 = w x t1        (p x r = (p1*r2 - p2*r1, p2*r0 - p0*r2, p0*r1 - p1*r0))
 *   M(p, r) = (p0*Mr_0 + p1*Mr_1) + p2*Mr_2,  Mr_i = (M_i0*r0 + M_i1*r1) + M_i2*r2;      m(p) = (p0*Sx + p1*Sy) + p2*Sz
 * (t1, t2, w) is an orthonormal frame; with u = t1.q, v = t2.q, s = w.q the moments in that frame are exact integers rotated:
 *   Su = m(t1), Sv = m(t2), Ss = m(w), Suu = M(t1,t1), Suv = M(t1,t2), Svv = M(t2,t2), Sus = M(t1,w), Svs = M(t2,w), Sss = M(w,w)
 * The regression s = c + a*u + b*v has the normal equations A x = y, x = (c, a, b), in this order of unknowns:
 *   A = [N Su Sv; Su Suu Suv; Sv Suv Svv],   y = (Ss, Sus, Svs)
 * solved by LDL^T without square roots, columns j = 0..2 left to right, every inner sum starting at 0.0 in index order:
 *   D_j  = A_jj - sum_{k<j} (L_jk*L_jk)*D_k
 *   status 2 (degenerate) unless D_j is finite and D_j > min_pivot * A_jj
 *   L_ij = (A_ij - sum_{k<j} (L_ik*L_jk)*D_k) / D_j                for i = j+1..2
 * then  z_i = y_i - sum_{k<i} L_ik*z_k   (i = 0..2),   x_i = z_i / D_i - sum_{k=i+1..2} L_ki*x_k   (i = 2..0).
 * With the constant first, D_1 and D_2 are the centred second moments: identical inliers fail at D_1, collinear ones at D_1 or D_2.
 *   g = (w - a*t1) - b*t2;   lg = sqrt((g0*g0 + g1*g1) + g2*g2);   nn = g / lg          the stepped unit normal
 *   gq = (Sx/N, Sy/N, Sz/N)                                                              the centroid, in q units
 *   d  = c/lg - ((nn0*gq0 + nn1*gq1) + nn2*gq2);   pq = gq + d*nn                        the centroid lifted onto the new plane
 *   unit = span / 65536;   anchor_i = (float)(A_i + pq_i*unit);   normal_i = (float)nn_i  each rounded to float once
 *   t = (N0*a0 + N1*a1) + N2*a2    on the rounded normal N and anchor a, as doubles
 *   with a prior:  if (N0*axis0 + N1*axis1) + N2*axis2 < 0: N = -N, t = -t;     without:  if t > 0: N = -N, t = -t
 *   offset = (float)(0.0 - t);   votes = N (the count)
 *   SSR = Sss - ((c*Ss + a*Sus) + b*Svs), taken as 0 if negative;   rms = unit * sqrt(SSR / N)      in the units of span
 * status 2 as well if x, lg (which must be > 0) or an output is not finite.  With status 0 plane_out is the stepped plane; else
 * plane_out = plane_in and rms = 0.  stats->inliers = N in every case.  Regressing the offset along the current normal on the
 * in-plane coordinates has total least squares as its fixed point: where the step leaves the normal unchanged, a = b = 0, the
 * in-plane coordinates are uncorrelated with the residual, and the normal is an eigenvector of the inliers' covariance; iterated
 * from a candidate near the plane it converges to the eigenvector of the smallest eigenvalue, the orthogonal-distance fit.
 *
 * sgm_plane_fit (blocking).  First sgm_plane_votes into candidates of the instance's own, sgm_plane_best into a 32-byte device
 * word of the instance's own, and that word copied to the host; a void best plane is status 1 and ends the call.  Then up to
 * spec->iterations rounds, each of which
 *   1. copies the current plane to that device word (from the second round on: in the first it is there already),
 *   2. queues sgm_plane_sums at it into 80 bytes of the instance's own,
 *   3. copies those 80 bytes to the host and waits for them,
 *   4. steps the plane with sgm_plane_solve.
 * The first status other than 0 ends the rounds, and the plane stays the last good one.  *plane
 * and *stats are HOST outputs: the last plane and the stats of the last solve.  trace_sums (HOST, int64 [iterations][10], or
 * NULL) receives the sums of every round made, trace_planes (HOST, sgm_plane [iterations + 1], or NULL) the best candidate and
 * the plane after every round made; rounds not made leave their entries as they were.
 *
 * The device entry points are asynchronous on sgm_stream(s) and ordered as sgm_volume_points is (behind the last match also with
 * sgm_set_overlap_post; a list queued before them on the same instance is finished when they read it).  d_records is 16-byte
 * aligned; d_planes, d_best and d_plane are 16-byte aligned; d_sums is 8-byte aligned and zeroed on the stream inside the call;
 * d_count is 4-byte aligned; d_labels needs no alignment.  No scratch, except the 32 KiB + 112 bytes sgm_plane_fit reserves at
 * its first call: an instance that never calls these entry points allocates and launches exactly what it did before.
 * false, nothing queued and one "sgm_mi355x: <entry point>: ..." line on stderr: a NULL pointer other than d_count, d_labels
 * (sgm_plane_label needs its d_labels) and the traces; a spec outside the ranges below; a label outside 1..255; a K outside 1..1024
 * (sgm_plane_best); a pointer not aligned as said; capacity > 2^32 (> 2^24 for sgm_plane_sums and sgm_plane_fit); an output that
 * overlaps an input or another output; a plane_in that is not finite or is void, or a sums[9] outside 0..2^24
 * (sgm_plane_solve); a build without the kernels.  Not part of it: several planes in one call, plane extents and polygons, a
 * plane at a clicked pixel, region growing on normals, a floor-aligned pose helper, row tiles. */
typedef struct { float normal[3]; float offset; float anchor[3]; uint32_t votes; } sgm_plane;   /* 32 bytes */
typedef struct {            /* 44 bytes, every field 4 bytes, no padding */
    int32_t  hypotheses;    /* K, 1..1024: candidate planes of a vote */
    uint32_t seed;          /* of the hash that picks the candidates' records */
    float    dist;          /* finite, > 0: the inlier half-thickness, units of the records */
    float    axis[3];       /* the orientation prior; all zero: none.  Else finite, with a finite length > 0 as a float */
    float    min_cos;       /* finite, 0..1: with a prior a candidate is kept only if |normal . axis| >= min_cos * |axis| */
    float    span;          /* finite, > 0: the length that normalises coordinates before they are quantised; about the scene size */
    int32_t  iterations;    /* 1..64: rounds of sgm_plane_fit */
    uint32_t min_inliers;   /* at least 3: fewer are status 1 */
    float    min_pivot;     /* finite, >= 0: a pivot D_j <= min_pivot * A_jj is status 2 */
} sgm_plane_spec;
typedef struct { double rms; uint32_t inliers; int32_t status; } sgm_plane_stats;   /* 16 bytes; status 0 ok, 1 too few inliers, 2 degenerate */
bool sgm_plane_votes(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records /* 16-byte records */, size_t capacity,
                     const uint32_t* d_count /* device u32, or NULL */, const uint8_t* d_labels /* device u8 [capacity], or NULL */,
                     sgm_plane* d_planes /* device, [hypotheses], 16-byte aligned */);
bool sgm_plane_best(sgm_instance* s, const sgm_plane* d_planes, int K /* 1..1024 */, sgm_plane* d_best /* device, 16-byte aligned */);
bool sgm_plane_sums(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records, size_t capacity, const uint32_t* d_count,
                    const uint8_t* d_labels, const sgm_plane* d_plane /* device, one plane */,
                    int64_t* d_sums /* device, [10], 8-byte aligned */);
bool sgm_plane_label(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records, size_t capacity, const uint32_t* d_count,
                     const sgm_plane* d_plane, int label /* 1..255 */, uint8_t* d_labels /* device u8 [capacity] */);
bool sgm_plane_solve(const sgm_plane_spec* spec, const int64_t sums[10], const sgm_plane* plane_in, sgm_plane* plane_out,
                     sgm_plane_stats* stats);                                        /* host only */
bool sgm_plane_fit(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records, size_t capacity, const uint32_t* d_count,
                   const uint8_t* d_labels, sgm_plane* plane /* HOST out */, sgm_plane_stats* stats /* HOST out */,
                   int64_t* trace_sums /* HOST [iterations][10], or NULL */, sgm_plane* trace_planes /* HOST [iterations + 1], or NULL */);

/* ---- objects in the TSDF volume: connected components of its voxel lattice ----
 * Extension, "parity unpinned by the reference"; defined here and restated by tests/components_ref.py.  The plane section ends with the
 * obstacle points; what a planner, a tracker or a viewer asks next is which of them belong together: how many objects stand on the
 * floor, where they are and how large, which mesh vertices belong to which, whether one free cell can be reached from another.
 * sgm_volume_components labels the connected components of a set of voxels and lists them; sgm_volume_component_of carries the
 * result to a list the volume produced.  Exact integers throughout, tolerance 0, the same bytes on every run.
 *
 * The set.  For a voxel word, w = word >> 16 and tq = (int16_t)word, as in the distance section; a voxel is observed iff
 * w >= min_weight.  A voxel is IN THE SET iff no plane excludes it (below) and
 *   set == 0 (occupied)   it is observed and tq < 0,   or
 *   set == 1 (free)       it is observed and tq >= 0,  or
 *   unknown == 1          it is not observed           (with either set)
 * Plane exclusion: how the floor sgm_plane_fit found is taken out, so that the things standing on it fall apart.  The spec carries
 * `planes` (0..4) host sgm_plane values and a clearance each.  Per axis the voxel centre is C = o + ((float)i + 0.5f) * voxel, the float
 * the integration uses, and
 *   s = ((n0*(Cx - a0) + n1*(Cy - a1)) + n2*(Cz - a2))       the plane section's vote arithmetic: float32, no contraction
 * A non-void plane excludes the voxel iff s is finite (by its bits) and s <= clearance: the plane's slab and everything behind it.
 * A void plane (an all-zero normal, either sign of zero) excludes nothing.
 * Neighbours.  connectivity 6: the voxels one step away along one axis; 26: along one, two or three axes.  Neighbours exist inside
 * the grid only.  The components are the classes of the symmetric relation "neighbours, both in the set".
 *
 * Outputs, with n the voxel index of the volume.
 *   d_labels   one uint32_t per voxel.  With `first` the smallest voxel index of the voxel's component and `size` its number of
 *              voxels, the word is first + 1 if the voxel is in the set and size >= min_voxels, and 0 otherwise.  Every word is
 *              written whatever the array held.
 *   d_objects  sgm_component records, one per surviving component (size >= min_voxels) in increasing order of first; only the first
 *              `capacity` records are written and nothing beyond min(C, capacity) records.  lo and hi are the inclusive box of the
 *              component in i, j, k; sum holds the sums of i, of j and of k over its voxels.
 *   d_counts   [0] = C, the surviving components, also where C > capacity; [1] = the components before the min_voxels filter.
 * capacity == 0 with d_objects == NULL asks for labels and counts alone.
 *
 * sgm_volume_component_of.  d_records are 16-byte records with the id in the last word; id_kinds 4 (sgm_surface_point, id = n*4 + a)
 * or 8 (sgm_mesh_vertex, id = n*8 + e) as in sgm_volume_colors, and record r is handled iff r < records_capacity and
 * (d_records_count == NULL or r < d_records_count[0]); nothing is written for the others.  The label of a record is that of its voxel
 * n; where that is 0, the label of the other end of its edge (the (dx,dy,dz) table of the mesh contract), where that voxel is inside
 * the grid.  A record whose n is outside the volume or whose kind does not exist has label 0.  d_index[r] is 1 plus the position in
 * d_objects[0 .. min(C, capacity)) of the object whose first + 1 equals the label -- found by binary search, the list is sorted --
 * and 0 where the label is 0 or the object was not written.  d_labels, d_objects, capacity and d_counts are those of the components
 * call, so it can be queued straight behind sgm_volume_mesh and sgm_volume_components with their device count words.
 * sgm_component_metric (host only).  lo[a] = origin[a] + (float)obj->lo[a] * voxel and hi[a] = origin[a] + (float)(obj->hi[a] + 1) *
 * voxel, float32 as written; centroid[a] = (float)(origin[a] + (sum[a] / voxels + 0.5) * voxel) computed in double (the quotient of
 * the two integers as doubles) and rounded once.  Only spec->voxel and spec->origin are read; an output that is NULL is left out, and
 * with voxels == 0 (no record the device writes) the quotient is taken as 0.
 * sgm_volume_components_bytes (host only): the size of d_labels, 4 * nx*ny*nz, 0 for a refused spec.
 *
 * How it runs.  Union-find over d_labels itself, which serves the call as its working array: a workgroup labels a tile of 64 x 8 x 8
 * voxels in LDS (one wave per x-row: runs come from a ballot, unions only between the runs of neighbouring rows), voxels on tile
 * faces union roots across tiles in global memory (parents only ever decrease, so every find ends), then the sizes, the filter, the
 * ordered compaction of the surviving roots (count per tile, one scan, emit) and a statistics pass that reduces a tile on chip
 * before it touches a record.  Integer atomics only; no workgroup waits for another.
 * Scratch: 4 * nx*ny*nz + 12 * ceil(nx*ny*nz / 2048) + 24 * min(capacity, nx*ny*nz) bytes of the instance's own, reserved at the
 * first call and grown when a later call needs more; it depends on the arguments alone, never on a value read back, and the call
 * does not block.  An instance that never calls these entry points allocates and launches exactly what it did before.
 *
 * The device calls are asynchronous on sgm_stream(s) and ordered as sgm_volume_points is.  false, nothing queued and one
 * "sgm_mi355x: <entry point>: ..." line on stderr: a NULL pointer other than d_objects with capacity 0 and d_records_count; a volume
 * spec that sgm_volume_integrate refuses; min_weight outside 1..65535; set or unknown other than 0 or 1; connectivity other than 6 or
 * 26; min_voxels < 1; planes outside 0..4; a plane (normal, offset, anchor) or clearance that is not finite; id_kinds other than 4 or
 * 8, and with 8 a volume over the mesh's 2^27 voxels; records_capacity above 2^32; a pointer that is not aligned (records 16 bytes,
 * objects 8, words 4); an output that overlaps an input or another output; a build without the kernels.  records_capacity == 0 is a
 * successful no-op.
 * Not part of it: 18-connectivity, incremental relabelling after an integration, tracking object identities across frames or window
 * shifts, oriented boxes, clustering of unorganised point lists. */
typedef struct {            /* 168 bytes, every field 4 bytes, no padding */
    uint32_t  min_weight;   /* 1..65535: a voxel is observed iff w >= min_weight */
    int32_t   set;          /* 0: the occupied voxels; 1: the free ones */
    int32_t   unknown;      /* 1: unobserved voxels belong to the set as well */
    int32_t   connectivity; /* 6 or 26 */
    uint32_t  min_voxels;   /* >= 1: smaller components get label 0 and no record */
    int32_t   planes;       /* 0..4: how many of plane[] and clearance[] are in effect */
    sgm_plane plane[4];     /* finite; only normal and anchor take part; a void plane excludes nothing */
    float     clearance[4]; /* finite: a voxel with s <= clearance is excluded */
} sgm_component_spec;
typedef struct {            /* 48 bytes */
    uint32_t first;         /* the smallest voxel index of the component: its label is first + 1 */
    uint32_t voxels;
    uint16_t lo[3], hi[3];  /* the inclusive box in i, j, k */
    uint32_t reserved;      /* 0 */
    uint64_t sum[3];        /* the sums of i, j, k over the component's voxels */
} sgm_component;
size_t sgm_volume_components_bytes(const sgm_volume_spec* spec);   /* host only; 4 * nx*ny*nz, 0 for a refused spec */
bool sgm_volume_components(sgm_instance* s, const sgm_volume_spec* spec, const sgm_component_spec* comp, const uint32_t* d_voxels,
                           uint32_t* d_labels, sgm_component* d_objects /* 8-byte aligned, or NULL */, size_t capacity,
                           uint32_t* d_counts /* [2]: surviving components, all components */);
bool sgm_volume_component_of(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_labels, const sgm_component* d_objects,
                             size_t capacity, const uint32_t* d_counts, const void* d_records /* 16-byte records, id in the last word */,
                             size_t records_capacity, const uint32_t* d_records_count /* device u32, may be NULL */,
                             int id_kinds /* 8 or 4 */, uint32_t* d_index /* u32 [records_capacity] */);
void sgm_component_metric(const sgm_volume_spec* spec, const sgm_component* obj, float lo[3], float hi[3], float centroid[3]); /* host only */

/* ---- matching at half or quarter scale, re-search at full resolution ----
 * Extension, "parity unpinned by the reference" (it has no such step); defined here and restated by tests/scaled_ref.py.  A match at
 * 1/f scale pays for f^3 fewer cells of W x H x D for the same metric range; the result is brought back to the full grid by a guided
 * selection and a small search on the FULL-resolution census words.  Off unless called: an instance that never calls one of these
 * entry points allocates and launches exactly what it did before.
 *
 * The low-resolution shape is w = width / f, h = height / f (floor); sgm_scaled_shape (host only) computes it and is false for a
 * spec outside its ranges or with w < 1 or h < 1.  All images and maps are [frames][rows][columns], frames back to back.
 *
 * sgm_downscale: out[j][i] = (sum of the f x f block of `in` at (f j, f i) + f^2 / 2) >> log2(f^2), exact, on u8 (bits == 8) or u16
 *   samples; trailing rows and columns that do not fill a block are not read.  One image stack per call; no alignment beyond the
 *   element's.
 *
 * sgm_upscale_disparity: for every full-resolution pixel (y, x) of every frame --
 *   Prior by guided selection (compares and selects only).  ny = 2 y + 1 - f, j0 = floor(ny / 2f), j1 = j0 + 1, ay = ny - 2f j0; the
 *   same for x gives i0, i1, ax; j0, j1 are then clamped to [0, h) and i0, i1 to [0, w).  The four candidates, in the order (j0,i0),
 *   (j0,i1), (j1,i0), (j1,i1), carry the weights (2f-ay)(2f-ax), (2f-ay) ax, ay (2f-ax), ay ax.  Among the candidates whose
 *   low-resolution disparity is finite (by its bit pattern: exponent bits not all ones) the one with the smallest
 *   |guide_small[j][i] - guide_full[y][x]| is selected; ties go to the larger weight, then to the earlier candidate.  No finite
 *   candidate: the output is +INF.  prior = f * d_sel (exact).  With radius < 0 the output is prior.
 *   Re-search (integers).  p = (int)rintf(min(max(prior, -2^20), 2^20)) (round to nearest even; the clamp changes no result, no
 *   candidate is admitted out there).  Candidates d = p + o, o = -f .. f; one is admitted iff d_lo <= d <= d_hi.  With no admitted
 *   candidate the output is prior.  A(d) = sum over the (2r+1)^2 window offsets (dy, dx) of t, where q = (y + dy, x + dx),
 *   xo = q.x - d (left view) or q.x + d (right_view != 0), t = popcount(census_ref[q] ^ census_oth[q.y][xo]), and t = 24 where q is
 *   outside the frame or xo is outside [0, width).  C(o) = 2 A + penalty |o| (2r+1)^2.  The winner is the admitted o with the
 *   smallest C; ties go to the smaller |o|, then to the smaller d.
 *   Sub-pixel.  If o-1 and o+1 are both admitted and den = C(o-1) + C(o+1) - 2 C(o) > 0:
 *   out = (float)d + (float)(C(o-1) - C(o+1)) / (float)(2 den), float32 operations each rounded on its own, the divide correctly
 *   rounded; otherwise out = (float)d.
 *   The guides are grey images of `bits` (u8, or u16 with more than 8 bits, 2-byte aligned); the census planes are u32
 *   [frames][height][width] of the reference view (the view the map belongs to) and of the other view, and may be NULL with
 *   radius < 0.  Every column is bounds-checked: nothing outside the planes is read.
 *
 * sgm_downscale, sgm_upscale_disparity and sgm_match_scaled_device take device pointers and are asynchronous on sgm_stream(s);
 * the first two need no initialised instance.  false, nothing queued and a message on stderr: a NULL pointer (but the census planes
 * with radius < 0), a spec outside the ranges below, a misaligned pointer, a build without the kernels.
 *
 * sgm_match_scaled (host pointers, blocking; pinned buffers of sgm_host_alloc are used in place) / sgm_match_scaled_device: the
 * instance must be initialised at (w, h) with the batch spec->frames and the pixel bits spec->bits.  In order: (1) both views are
 * downscaled; (2) the instance's ordinary match runs on the small pair, with every option of the instance (census kind, reference
 * view, four paths, hole filling, refinement, a match without Reset); its final map is the one stage 8 reads back; (3) the census of
 * both FULL-resolution views is computed by the instance's census kind (5x5 centre, or symmetric with its window; on the u16 samples
 * with more than 8 bits), every word written, the border 0, into buffers of the call's own: the instance's census planes are
 * untouched; (4) sgm_upscale_disparity with the reference view's image and its downscaled twin as guides, right_view of the
 * instance, d_lo = f * min_disparity and d_hi = f * max_disparity - 1 of the instance's option (the spec's d_lo / d_hi are ignored).
 * Additionally refused: a shape, batch or bits mismatch; row-tile mode; rectification in effect (its maps are for the small shape
 * and the guide would be unrectified); a wide CENTRE census window (u64 words) with radius >= 0.  Device buffers are reserved at the
 * first call.  A plain sgm_match on the same instance afterwards returns what it would have returned.
 * Not part of it: confidence at full resolution, both views, rectification, row tiles, factors other than 2 and 4,
 * sgm_match_planes. */
typedef struct {            /* 36 bytes, every field 4 bytes, no padding */
    int32_t width, height, frames;   /* FULL resolution; 1 <= width, height <= 65535, 1 <= frames <= 65535, frames * width * height <= 2^31 */
    int32_t factor;                  /* f: 2 or 4 */
    int32_t bits;                    /* 8: samples are u8;  9..16: samples are u16 (as SGM_SetPixelBits) */
    int32_t radius;                  /* r: window radius of the re-search, 0..4; < 0: no re-search (guided upscale only) */
    int32_t penalty;                 /* pull toward the prior, 0..16, in half Hamming bits per window pixel per step */
    int32_t d_lo, d_hi;              /* admitted full-resolution disparities, inclusive, 0 <= d_lo <= d_hi <= 65535 */
} sgm_scale_spec;
#define SGM_SCALE_DEFAULT_RADIUS 3
#define SGM_SCALE_DEFAULT_PENALTY 1
bool   sgm_scaled_shape(const sgm_scale_spec* spec, int* w, int* h);
bool   sgm_downscale(sgm_instance* s, const sgm_scale_spec* spec, const void* d_in, void* d_out);
bool   sgm_upscale_disparity(sgm_instance* s, const sgm_scale_spec* spec, const float* d_disp_small, const void* d_guide_small,
                             const void* d_guide_full, const uint32_t* d_census_ref, const uint32_t* d_census_oth, int right_view,
                             float* d_disp_full);
bool   sgm_match_scaled(sgm_instance* s, const sgm_scale_spec* spec, const uint8_t* img_left, const uint8_t* img_right, float* disp_full);
bool   sgm_match_scaled_device(sgm_instance* s, const sgm_scale_spec* spec, const uint8_t* d_left, const uint8_t* d_right,
                               float* d_disp_full);
bool   SGM_MatchScaled(const sgm_scale_spec* spec, const uint8_t* img_left, const uint8_t* img_right, float* disp_full);   /* the default instance */

/* ---- temporal filter for streams of maps: history, motion gate, hold ----
 * Extension, "parity unpinned by the reference" (it treats every frame as the only one); defined here and restated by
 * tests/temporal_ref.py.  The device matches it bit for bit.  All arithmetic is float32, every operation rounded on its own,
 * subnormals kept.  "Finite" always means by bit pattern, exponent bits not all ones: a caller's map may hold NaN.
 *
 * State per stream and pixel: hv (f32), the last output value, starts at +INF; hb (u8), the validity of the last eight INPUTS,
 * newest in bit 0, starts at 0.  Constants: a = alpha, b = 1.0f - a, rounded once on the host.
 * One step, with input x, optional confidence K, n = hold_window, k = hold_count and cnt = popcount(hb & ((1 << n) - 1)):
 *   1. valid = finite(x) && (no confidence given || min_conf == 0 || K >= min_conf).
 *   2. The decision; the classes are numbered for the statistics.
 *        0 first     valid and hv not finite:                                   out = x
 *        1 smoothed  valid, hv finite and fabsf(x - hv) <= delta:               out = a * x + b * hv   (two products and one sum,
 *                                                                               each rounded; hence alpha == 1 returns x)
 *        2 replaced  valid, hv finite, gate exceeded (motion, an edge):         out = x
 *        3 held      not valid, n > 0, hv finite and cnt >= k:                  out = hv
 *        4 invalid   otherwise:                                                 out = +INF
 *   3. hb' = (hb << 1 | valid) & 0xFF.
 *   4. hv' = out if out is finite; else +INF if hb' == 0 (the history forgets after eight invalid inputs); else hv.
 * The validity bits record inputs, not outputs: a held value cannot keep itself alive.  The steps of a stream run in order,
 * pixels are independent, and the result is a pure function of (state, inputs, spec), also for arbitrary caller-made state.
 * Statistics: uint32_t [maps][5], one exact count per class and map; maps = streams x steps in the order the maps lie in memory.
 *
 * sgm_temporal_filter: the filter on any device maps, in place.  d_maps f32 [streams][steps][pixels]; d_conf u16 of the same
 *   shape, or NULL; the history d_hist_value f32 / d_hist_bits u8 [streams][pixels]; d_stats [streams * steps][5] or NULL, zeroed
 *   by the call on the stream.  spec->sequence and spec->stats are not looked at: the geometry and d_stats say it.  Asynchronous on
 *   sgm_stream(s), behind the last match; needs no initialised instance and no alignment beyond the element's (a map that cannot
 *   be read 16 bytes at a time takes a one-pixel-per-lane path with the same results).  false, nothing queued and a message on
 *   stderr: a NULL required pointer, a pointer that is not aligned to its element, a spec outside its ranges, streams, steps or
 *   pixels < 1 or a product above 2^31, a build without the kernel.
 * sgm_temporal_clear: +INF / 0 into streams x pixels history entries, on the stream.
 * sgm_set_temporal (SGM_SetTemporal: the default instance, remembered across SGM_Shutdown): turns the filter on for matches, NULL
 *   turns it off; takes effect at the next SGM_Initialize / sgm_initialize / SGM_Reset / sgm_reset, which return false in row-tile
 *   mode (sgm_set_rows) with it on.  false, and nothing changes, for a spec outside its ranges, a build without the kernel, or
 *   min_conf > 0 in a build without the confidence kernels.  Every entry point then returns the filtered map: sgm_match, _async,
 *   _device, sgm_compute, sgm_match_confidence*, sgm_match_both* (both maps, each view with a history of its own),
 *   sgm_match_planes* (the depth is computed from the filtered map) and sgm_match_scaled* (its small map, because it runs the
 *   ordinary match).  The filter is the last step of the post pass -- after the median, after hole filling, after the refinement
 *   -- on the post-pass stream; timing: it counts toward "median".  With min_conf > 0 every match computes the confidence the way a
 *   refining instance does (into the caller's map where one is given, else into an internal one; the fused last sweep is not
 *   used) and sgm_match_both* is refused, the confidence being defined for one reference view; with min_conf == 0 no confidence is
 *   computed for the filter's sake.  sequence = 0: the B frames of a batch are B streams; sequence = 1: they are B consecutive
 *   frames of ONE stream.
 * History lifetime.  The history belongs to the instance.  It SURVIVES sgm_reset / sgm_initialize with an unchanged stream
 *   signature -- the per-frame Reset of a stream.  It restarts (a clear queued on the stream the filter runs on, ahead of its next
 *   launch) when the signature of the match about to be filtered differs from that of the last filtered one -- width, height,
 *   batch, reference view, single or both views, sequence --, after every sgm_set_temporal(s, non-NULL), and after
 *   sgm_temporal_restart(s), the caller's scene cut.  A match that fails before or at the filter's launch leaves the history
 *   exactly as it was.
 * sgm_temporal_stats (blocking): the counters of the last match, [B * views][5], into out (room for `capacity` maps); returns the
 *   number of maps written, 0 when stats was off, nothing was filtered yet or capacity is too small.
 * Stage read-back: 8 stays "what the match returned"; 29 the map as it entered the filter (needs sgm_keep_stages); 30 hv and 31 hb
 *   of the selected frame's stream after the last match; 32 / 33 / 34 the same three for the right view after sgm_match_both.  With
 *   sequence = 1 every frame index reads the one stream for 30 / 31 (33 / 34).
 * An instance that never calls sgm_set_temporal with a spec allocates and launches exactly what it did before.
 * Not part of it: motion compensation, filtering the confidence map, row tiles, a history shared between instances. */
typedef struct {            /* 28 bytes, every field 4 bytes, no padding */
    float    alpha;         /* weight of the new measurement, finite, 0 < alpha <= 1 */
    float    delta;         /* gate in disparities, finite, >= 0 */
    int32_t  hold_window;   /* n: 0..8; 0 = holes are never bridged */
    int32_t  hold_count;    /* k: 1..n (not looked at with n == 0) */
    int32_t  sequence;      /* 0: every frame of a batch is a stream of its own; 1: the B frames of a call are consecutive frames of ONE stream */
    uint32_t min_conf;      /* 0..65535; > 0: a measurement whose matching confidence is below it counts as a hole */
    int32_t  stats;         /* 0 / 1: count the decisions */
} sgm_temporal_spec;
bool   sgm_temporal_filter(sgm_instance* s, const sgm_temporal_spec* spec, size_t streams, size_t steps, size_t pixels, float* d_maps,
                           const uint16_t* d_conf, float* d_hist_value, uint8_t* d_hist_bits, uint32_t* d_stats);
bool   sgm_temporal_clear(sgm_instance* s, size_t streams, size_t pixels, float* d_hist_value, uint8_t* d_hist_bits);
bool   sgm_set_temporal(sgm_instance* s, const sgm_temporal_spec* spec);
bool   sgm_temporal_restart(sgm_instance* s);
int    sgm_temporal_stats(sgm_instance* s, uint32_t* out, int capacity);
bool   SGM_SetTemporal(const sgm_temporal_spec* spec);
bool   SGM_TemporalRestart(void);
int    SGM_TemporalStats(uint32_t* out, int capacity);

/* The filling of SGM_SetFillHoles (step 2) on any device map: d_disp, the instance's B frames of its shape, is filled in
 * place with R = the option's max_disparity; d_class (u8 [B][H][W], classes 0/1/2) drives passes 1 and 2, NULL runs pass 3
 * alone.  Asynchronous on sgm_stream(s), behind the last match.  Works whether or not filling is on for matches; the filled
 * map of a match (stage 9) is overwritten. */
bool   sgm_fill_holes(sgm_instance* s, float* d_disp, const uint8_t* d_class);

/* The refinement of SGM_SetRefine (steps 1-5) on any device map: d_disp, the instance's B frames of its shape, is refined in place
 * with the parameters of the last sgm_set_refine(s, 1, ...) (false if there was none), from the u16 confidence d_conf and the u8
 * grey image d_guide ([B][H][W] each).  Asynchronous on sgm_stream(s), behind the last match.  Works whether or not the refinement
 * is on for matches. */
bool   sgm_refine_disparity(sgm_instance* s, float* d_disp, const uint16_t* d_conf, const uint8_t* d_guide);

/* The remap of SGM_SetRectify on any device images: B frames of the instance's shape each, d_out_* = d_* sampled through the maps
 * in effect (those of the last initialize / reset).  No output may alias an input.  Asynchronous on sgm_stream(s).  false when no
 * maps are in effect.  With more than 8 bits per sample in effect (SGM_SetPixelBits) all four images are uint16_t. */
bool   sgm_rectify(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, uint8_t* d_out_left, uint8_t* d_out_right);

/* ---- a test-platform frame end to end (the data formats either side of the path) ----
 * The server hands the board six byte planes per frame -- left B, G, R, right B, G, R, each h rows of w bytes
 * (HostScript_Server/server.py:105-131; received into frame_buffer.h:16-51 by tcp_perf_client.c:181-189) -- and expects h rows
 * of w float32 depth in mm back (message type 3, server.py:148-177).  The firmware's grey conversion is
 * (76 r + 150 g + 29 b) >> 8 (stereo_matching.c:18-25; stb's, behind main.c's image load, uses 77: weight_r selects).
 *   sgm_gray_from_planes   device buffers: three planes B, G, R of `count` bytes each at d_bgr -> d_gray; on sgm_stream(s).
 *   sgm_match_planes_async host buffers: queues H2D of the six planes (B frames of six with sgm_set_batch), both grey
 *                          conversions, the match, disparity -> depth (as sgm_disparity_to_depth) and D2H of the depth map,
 *                          then returns; sgm_match_wait hands the map over.  Pinned buffers (sgm_host_alloc) are used in
 *                          place.  The disparity map itself stays readable with sgm_read_stage(s, 8, ...).
 *   sgm_match_planes       = sgm_match_planes_async + sgm_match_wait. */
bool   sgm_gray_from_planes(sgm_instance* s, const uint8_t* d_bgr, size_t count, int weight_r, uint8_t* d_gray);
bool   sgm_match_planes_async(sgm_instance* s, const uint8_t* planes, float fx, float baseline, float doffs, float* depth);
bool   sgm_match_planes(sgm_instance* s, const uint8_t* planes, float fx, float baseline, float doffs, float* depth);

/* ---- stage read-back (parity tests; copies device -> host, blocking) ----
 * which: 0 census left (u32 [H][W])       1 census right (u32 [H][W])    (u64 words with a wide CENTRE census window)
 *        2 matching cost (u8 [H][W][D])   3 aggregated cost S (u16 [H][W][D])
 *        4 left disparity after WTA       5 right-view disparity
 *        6 after LR check                 7 after speckle removal        8 final (all f32 [H][W])
 *        9 after hole filling (f32 [H][W]; needs sgm_keep_stages and filling on, SGM_SetFillHoles)
 *        18 hole-filling classes (u8 [H][W]; after any match with filling on)
 *        19 rectified left image         20 rectified right image       (u8 [H][W]; 0 bytes with rectification off, SGM_SetRectify;
 *                                                                        u16 [H][W] with more than 8 bits per sample, SGM_SetPixelBits)
 *        21 narrowed left image          22 narrowed right image        (u8 [H][W]; 0 bytes with 8-bit input, SGM_SetPixelBits)
 *        10..17 per-direction path cost L_r of direction (which-10) (u8 [H][W][D]; cells the
 *               direction never visits read 0, cells visited twice hold the last-but-one visit)
 *        after a sgm_match_both (SGM_MatchBoth), where 4, 6, 7, 8 are the LEFT view's maps and 5 the raw right-view map:
 *        26 right view after the LR check   27 right view after speckle removal   (both need sgm_keep_stages during that match)
 *        28 right view, final               (all f32 [H][W]; 0 bytes after any other kind of match or a sgm_match_both that failed)
 *        with the temporal filter on (sgm_set_temporal), after a match it filtered:
 *        29 the map as it entered the filter (f32 [H][W]; needs sgm_keep_stages)   30 hv (f32 [H][W])   31 hb (u8 [H][W])
 *        32 / 33 / 34 the same three for the right view after a sgm_match_both
 * Returns the number of bytes written, 0 on error or if `capacity` is too small. */
size_t sgm_read_stage(sgm_instance* s, int which, void* host_out, size_t capacity);
size_t SGM_ReadStage(int which, void* host_out, size_t capacity);
/* Stages 4, 6 and 7 are overwritten in place by the following stage and stage 2 (the cost volume) is
 * normally never materialised (the aggregation kernel recomputes it from the census images); enable
 * keeping them (one extra kernel + three device-to-device copies per match) before the match whose
 * stages are read. */
void   sgm_keep_stages(sgm_instance* s, int enable);
void   SGM_KeepStages(int enable);

/* Per-kernel device time (ms) of the last match of the instance, measured with HIP events on
 * the instance's stream when timing is enabled.  names[i] points to static strings.
 * Returns the number of entries written (<= max_entries).  With hole filling on (SGM_SetFillHoles) the same eight entries:
 * the classification is part of "lrcheck", the three filling passes are part of "speckle". */
void   sgm_enable_timing(sgm_instance* s, int enable);
int    sgm_last_timing(sgm_instance* s, const char** names, float* ms, int max_entries);
/* Mean and minimum per-kernel time over every match since timing was (re-)enabled and collected by
 * sgm_synchronize (up to 64 matches between two synchronizes are kept); *matches = how many. */
int    sgm_mean_timing(sgm_instance* s, const char** names, float* mean_ms, float* min_ms, int max_entries, long* matches);

/* ---- debugging: guard bands and poison around every device buffer of the library ----
 * Off unless asked for through the environment, read at every allocation (buffers only grow, so that is off the hot path):
 *   SGM_DEBUG_GUARD=<bytes>    every device buffer the library allocates from then on gets a band of that many bytes (rounded up
 *                              to 4096) in front of it and one behind it, the second starting at the buffer's last byte + 1
 *   SGM_DEBUG_POISON=<0..255>  the byte that fills the bands AND the buffer itself before anybody uses it (0xA5 unless given;
 *                              given alone: poisoned buffers without bands)
 * With neither set the library allocates exactly what it always did and keeps no record.
 * sgm_debug_guard_check waits for the device, copies every live band back and compares it with the poison.  Returns the number of
 * violated bands, those of buffers freed (or re-allocated larger) since the last call included -- these are reported once.
 * Every violation is one line on stderr: the buffer's size, the band, the first and last byte that changed, as an offset from the
 * buffer's start (front band: -1 is the byte just in front of it) or its end (back band: +0 is the first byte behind it).
 * live_allocations / live_bytes (either may be NULL): how many buffers are under guard and the sum of their sizes; 0 with the
 * mode off, and the return value is 0 then.  A write of the very poison byte cannot show: run under two different bytes.
 * Caller-owned buffers are not covered.  Thread-safe. */
int    sgm_debug_guard_check(int* live_allocations, size_t* live_bytes);

/* Seeded synthetic stereo pair of SURVEY.md 8(d) (host buffers of width*height bytes each). */
void   SGM_SynthPair(int width, int height, int disparity_range, uint32_t seed, uint8_t* left, uint8_t* right);

/* Library build info, e.g. "sgm_mi355x 0.1 gfx950". */
const char* SGM_Version(void);

#ifdef __cplusplus
}
#endif
#endif /* SGM_MI355X_H */
