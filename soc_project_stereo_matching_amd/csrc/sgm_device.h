/*
 * sgm_device.h -- the thin C interface between the C host (sgm_host.c) and the HIP translation
 * units (sgm_*.hip).  Plain C types only; device memory is passed as void*.
 * Every function returns 0 on success and a non-zero HIP error code otherwise (the message is
 * printed to stderr by the HIP side), except where noted.
 */
#ifndef SGM_DEVICE_H
#define SGM_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device, stream, memory ---- */
int   sgmd_device_count(void);                       /* <= 0: no usable device */
int   sgmd_device_is_gfx950(int ordinal);            /* 1 yes, 0 no, <0 error */
int   sgmd_stream_create(int ordinal, void** stream);
/* a stream whose kernels run only on compute units [first, first + count) of EVERY XCD (hipExtStreamCreateWithCUMask; the mask's
 * bit i is CU i / xcds of XCD i % xcds).  count <= 0: an ordinary stream on all CUs */
int   sgmd_stream_create_cus(int ordinal, void** stream, int first_per_xcd, int count_per_xcd);
int   sgmd_device_cus(int ordinal, int* cus_per_xcd, int* xcds);     /* 32 x 8 on MI355X */
int   sgmd_stream_create_prio(int ordinal, void** stream, int priority);   /* 0 normal, < 0 higher, > 0 lower (clamped) */
int   sgmd_stream_destroy(int ordinal, void* stream);
int   sgmd_stream_sync(int ordinal, void* stream);
/* events without timing, for ordering one stream behind another */
int   sgmd_event_create(int ordinal, void** event);
void  sgmd_event_destroy(int ordinal, void* event);
int   sgmd_event_record(int ordinal, void* event, void* stream);
int   sgmd_stream_wait_event(int ordinal, void* stream, void* event);
int   sgmd_event_sync(int ordinal, void* event);                     /* the host waits */
int   sgmd_set_device(int ordinal);                                  /* the calling thread's current device (for libraries such as RCCL) */
int   sgmd_mem_info(int ordinal, size_t* free_bytes, size_t* total_bytes);
int   sgmd_alloc(int ordinal, void** dptr, size_t bytes);
int   sgmd_free(int ordinal, void* dptr);
/* the debug allocation mode of sgmd_alloc / sgmd_free (sgm_guard.h): the number of violated guard bands, those found at free time
 * since the last call included; 0 with 0 live allocations while the mode is off.  Not an error code.  The C host does not call
 * it (csrc/sgm_runtime.hip exports it as sgm_debug_guard_check itself), so a stand-in device layer need not have it. */
int   sgmd_guard_check(int* live_allocations, size_t* live_bytes);
int   sgmd_alloc_pinned(int ordinal, void** hptr, size_t bytes);
int   sgmd_free_pinned(int ordinal, void* hptr);
int   sgmd_host_is_pinned(int ordinal, const void* hptr, size_t bytes);   /* 1: [hptr, hptr+bytes) is page-locked HIP host memory, else 0 */
int   sgmd_h2d_async(int ordinal, void* stream, void* dst, const void* src, size_t bytes);
int   sgmd_d2h_async(int ordinal, void* stream, void* dst, const void* src, size_t bytes);
int   sgmd_d2d_async(int ordinal, void* stream, void* dst, const void* src, size_t bytes);
/* `rows` pieces of `width` bytes each, `src_pitch` / `dst_pitch` bytes apart (device to device; the row gather of a batch packs the same
 * rows of every map into one message this way) */
int   sgmd_d2d_2d_async(int ordinal, void* stream, void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows);
/* One image row of up to 8 direction planes of every frame of the batch <-> a packed buffer [frame][k][row_bytes] (the row-tile
 * hand-over): plane d = dirs[k] of frame f starts at planes + (f * 8 + d) * plane_bytes; to_buf != 0 gathers, else scatters. */
int   sgmd_plane_rows_copy(int ordinal, void* stream, void* planes, size_t plane_bytes, size_t row_offset, size_t row_bytes,
                           const int* dirs, int ndirs, int frames, void* buf, int to_buf);
int   sgmd_memset_async(int ordinal, void* stream, void* dst, int value, size_t bytes);

/* ---- per-stage timing with HIP events on the stream ---- */
int   sgmd_timer_create(int ordinal, void** timer, int max_marks);
void  sgmd_timer_destroy(int ordinal, void* timer);
int   sgmd_timer_mark(int ordinal, void* timer, void* stream, int index);           /* records event #index */
int   sgmd_timer_elapsed(int ordinal, void* timer, int from, int to, float* ms);    /* after a sync */

/* ---- geometry shared by all launchers ---- */
typedef struct {
    int W, H;          /* image */
    int D;             /* max_disparity - min_disparity */
    int Dp;            /* padded cell stride of the volumes: 16 * DPL >= D */
    int DPL;           /* disparities per lane in the aggregation kernel (2,4,8,12,16,32) */
    int LPP;           /* lanes per pixel in the aggregation kernel: 16 (4 lines per wave) or 8 (8 lines); Dp = LPP*DPL */
    int HL;            /* lanes per pixel of the horizontal lines: 0 = LPP, or 32 / 64 (2 / 1 lines per wave; needs
                          Dp/HL in {2,4,8,16}): the launcher falls back to LPP where the combination does not exist */
    int dmin;          /* min_disparity */
    int B;             /* frames per launch (batch): every buffer is [B][...] frame-major, every kernel
                          processes all B frames */
    int row_begin, row_end;  /* the rows this GPU computes in aggregate / sum_wta / wta_right / lrcheck: [0,H) normally,
                          a row tile when a frame is spread over several GPUs (buffers stay frame-sized) */
} sgmd_geom;

/* one anomalous-line visit that lands on a pixel of row `row` (built by the host) */
typedef struct {
    int32_t col_slot;  /* column | (diagonal slot 0..3) << 16 */
    int32_t step;      /* index k into the slot's extras rows */
} sgmd_row_extra;

typedef struct {
    int ndirs;                 /* 4 or 8, reference order SemiGlobalMatching.c:213-220 */
    int dx[8], dy[8];
    int anom_line[8];          /* line index whose first step trips the wrong edge test, or -1 */
    int ghost_zero;            /* 1: W >= H, the anomalous wave zeroes the cells no line visits */
    int p1;
    int pen_max;               /* largest entry of the adaptive-P2 table = max(P1, P2_init, 0): picks the aggregation step family */
    int allow_fast;            /* 0: never the FAST step family (sgm_aggregate_fast.hip), whatever the penalties (tests run both) */
    int dir_mask;              /* bit d: run direction d in this launch (0xFF normally; a tile sweep runs a subset) */
    int run_anom;              /* 1: run the anomalous diagonal lines in this launch (whole frame, never tiled) */
    int up_fused;              /* 1: the upward directions belong to the fused last sweep (sgmd_upsum): this launch skips (0,-1) and walks
                                  of (-1,-1) / (1,-1) only the H-1 lines that wrap around the image edge, storing their post-wrap cells */
} sgmd_paths;

/* ---- stage launchers (all asynchronous on `stream`) ---- */

/* 5x5 census of both images; border = 0.  SemiGlobalMatching.c:134-159 */
/* need: NULL, or one byte per block of the sgmd_census_blocks grid (row-major): 0 = leave the block's words as they are (a
 * row-tile instance only needs its own rows and the pixels the four anomalous lines read) */
/* keep_border != 0: the words the reference never writes (the 2-pixel border; everything when W <= 5 or H <= 5, .c:136,140-141)
 * are left as they are instead of being written as 0 -- the reference's static buffers keep what an earlier frame of another
 * shape left at the same linear index */
int sgmd_census(int ord, void* stream, const sgmd_geom* g, const void* left, const void* right,
                void* census_l, void* census_r, const void* need, int keep_border);
void sgmd_census_blocks(const sgmd_geom* g, int* blocks_x, int* blocks_y);     /* blocks of 64 x 16 pixels */

/* Hamming matching cost volume, u8 [H][W][Dp].  SemiGlobalMatching.c:161-196 */
int sgmd_cost(int ord, void* stream, const sgmd_geom* g, const void* census_l, const void* census_r, void* cost);

/* Extension: census over an odd cw x ch window of at most 64 pixels into u64 words, and the Hamming cost
 * volume of those words (u8 [H][W][Dp], as sgmd_cost); sgmd_aggregate then takes the volume instead of the census images */
int sgmd_census_window(int ord, void* stream, const sgmd_geom* g, int cw, int ch, const void* left, const void* right,
                       void* census64_l, void* census64_r);
int sgmd_cost64(int ord, void* stream, const sgmd_geom* g, const void* census64_l, const void* census64_r, void* cost);

/* Extension (parity unpinned by the reference), the centre-symmetric census of include/sgm_mi355x.h (SGM_SetCensusKind) over an
 * odd cw x ch window of at most 64 pixels: u32 words of at most 31 bits into the buffers of sgmd_census, for the same
 * aggregation, with the same block grid and `need` map; every word of a block that is not skipped is written (0 on the border).
 * sgm_host.c references it weakly (a host built without it refuses that census kind). */
int sgmd_census_sym(int ord, void* stream, const sgmd_geom* g, int cw, int ch, const void* left, const void* right,
                    void* census_l, void* census_r, const void* need);

/* All directions of the path aggregation in ONE launch.  SemiGlobalMatching.c:198-372.
 * The matching cost (SemiGlobalMatching.c:161-196) is recomputed from the census images inside the
 * kernel; census_r must be preceded by at least sgmd_census_slack(g) readable bytes (disparities that
 * reach left of column 0 read there and are masked to 127) and followed by 64 readable bytes (a wave's
 * census run is loaded in whole 16-byte groups).
 * planes: u8 [ndirs][H][W][Dp] per-direction path costs L_r; extras: u8 [4][H][Dp] path costs of
 * the four anomalous diagonal lines (step-major); lut: u16[256] = (uint16)max(P1, P2/(a+1)). */
size_t sgmd_census_slack(const sgmd_geom* g);
int sgmd_aggregate(int ord, void* stream, const sgmd_geom* g, const sgmd_paths* paths, const void* img_left,
                   const void* census_l, const void* census_r, const void* lut, void* planes, size_t plane_bytes,
                   void* extras);
/* the same aggregation fed from a materialised cost volume (sgmd_cost / sgmd_cost64) instead of recomputing the cost:
 * what the wide census windows use (generic step, 16 lanes per pixel) */
int sgmd_aggregate_volume(int ord, void* stream, const sgmd_geom* g, const sgmd_paths* paths, const void* img_left,
                          const void* cost, const void* lut, void* planes, size_t plane_bytes, void* extras);

/* S = (accumulate ? S : 0) + sum of planes + anomalous-line visits (u16 [H][W][Dp]) and, fused, the LEFT-view
 * winner-take-all with uniqueness and sub-pixel (SemiGlobalMatching.c:374-443, inverse == 0) -> disp_l */
int sgmd_sum_wta(int ord, void* stream, const sgmd_geom* g, int ndirs, const void* planes, size_t plane_bytes,
                 const void* extras, const void* row_extras, const void* row_extra_count, int row_cap, int accumulate,
                 void* S, int check_unique, float one_minus_ratio, void* disp_l);

/* The same sum and BOTH winner-take-all passes in one kernel (Dp <= 256: sgmd_sum_wta_lr_supported): a workgroup
 * walks an image row and keeps the last Dp+32 columns of S in LDS for the right view's diagonal gather, so S is
 * written only if store_S (and read only if accumulate); do_right = 0 skips the right view (no LR check). */
int sgmd_sum_wta_lr_supported(const sgmd_geom* g, int row_cap);   /* row_cap: most anomalous-line visits in one row */
int sgmd_sum_wta_lr(int ord, void* stream, const sgmd_geom* g, int ndirs, const void* planes, size_t plane_bytes,
                    const void* extras, const void* row_extras, const void* row_extra_count, int row_cap, int accumulate,
                    int store_S, int do_right, void* S, int check_unique, float one_minus_ratio, void* disp_l, void* disp_r);

/* The LAST vertical sweep -- directions (0,-1), (-1,-1), (1,-1), SemiGlobalMatching.c:216,218,219 -- fused with the cost sum and both
 * winner-take-all passes (sgm_upsum.hip): reads the five other planes and the post-wrap cells of the two diagonal ones (an
 * aggregation launch with paths->up_fused), writes the two disparity maps; S and the three planes never exist.
 * sgmd_upsum_rows: the most image rows a workgroup may take (sgmd_upsum's rows_per_workgroup: 1 .. that), 0 where the shape keeps the separate kernels (needs W > H, Dp = 128, whole frames).
 * scratch: sgmd_upsum_scratch_bytes(g) bytes, zero when allocated; generation: a different number for every launch on that scratch;
 * status: NULL or a page-locked int set to 1 if a workgroup gave up waiting for the rows below (the maps are then wrong);
 * workgroups_per_frame: 0 = the launcher's choice (a frame's row groups are drawn from a ticket by that many persistent workgroups). */
int sgmd_upsum_rows(const sgmd_geom* g);
size_t sgmd_upsum_scratch_bytes(const sgmd_geom* g);
int sgmd_upsum(int ord, void* stream, const sgmd_geom* g, const sgmd_paths* paths, const void* img_left, const void* census_l,
               const void* census_r, const void* lut, const void* planes, size_t plane_bytes, const void* extras,
               const void* row_extras, const void* row_extra_count, int row_cap, int do_right, int check_unique, float one_minus_ratio,
               void* scratch, unsigned generation, void* status, int rows_per_workgroup, int workgroups_per_frame, void* disp_l, void* disp_r);

/* right-view winner-take-all on S[y][x+d][d] (SemiGlobalMatching.c:395-408) -> disp_r; needed by the LR check only */
int sgmd_wta_right(int ord, void* stream, const sgmd_geom* g, const void* S, int check_unique, float one_minus_ratio,
                   void* disp_r);

/* Extension (parity unpinned by the reference), the matching confidence of include/sgm_mi355x.h (sgm_match_confidence): the
 * launchers above that also store the reference view's confidence of every pixel to conf, u16 [B][H][W].  sgmd_sum_wta_conf: the
 * left view; sgmd_wta_right_conf: the right view; sgmd_sum_wta_lr_conf: the left view, or the right one if conf_right (needs
 * do_right).  conf == NULL: exactly the plain launcher.  sgm_host.c references them weakly (a host built without them answers
 * false to the confidence entry points). */
int sgmd_sum_wta_conf(int ord, void* stream, const sgmd_geom* g, int ndirs, const void* planes, size_t plane_bytes,
                      const void* extras, const void* row_extras, const void* row_extra_count, int row_cap, int accumulate,
                      void* S, int check_unique, float one_minus_ratio, void* disp_l, void* conf);
int sgmd_sum_wta_lr_conf(int ord, void* stream, const sgmd_geom* g, int ndirs, const void* planes, size_t plane_bytes,
                         const void* extras, const void* row_extras, const void* row_extra_count, int row_cap, int accumulate,
                         int store_S, int do_right, void* S, int check_unique, float one_minus_ratio, void* disp_l, void* disp_r,
                         void* conf, int conf_right);
int sgmd_wta_right_conf(int ord, void* stream, const sgmd_geom* g, const void* S, int check_unique, float one_minus_ratio,
                        void* disp_r, void* conf);

/* SemiGlobalMatching.c:445-470 */
int sgmd_lrcheck(int ord, void* stream, const sgmd_geom* g, void* disp_l, const void* disp_r, float thres);

/* Extension: the right view as the reference view.  out = disp_r where the mirrored check against disp_l passes (all of
 * disp_r if !do_check), +INF elsewhere; out must not alias either input */
int sgmd_lrcheck_right(int ord, void* stream, const sgmd_geom* g, const void* disp_r, const void* disp_l, float thres,
                       int do_check, void* out);

/* Extension (sgm_match_both): both checks in one pass.  out_l / out_r = the two raw WTA maps after sgmd_lrcheck / its mirror
 * image (plain copies if !do_check); whole frames only; neither output may alias an input, both raw maps survive.
 * sgm_host.c references it weakly (a host built without it answers false to the sgm_match_both entry points). */
int sgmd_lrcheck_both(int ord, void* stream, const sgmd_geom* g, const void* disp_l, const void* disp_r, float thres, int do_check,
                      void* out_l, void* out_r);

/* connected components (|delta| <= diff, 8-neighbourhood) smaller than min_area -> +INF.
 * labels/sizes/totals: int32 [H][W] scratch each.  SemiGlobalMatching.c:585-642 */
int sgmd_speckle(int ord, void* stream, const sgmd_geom* g, void* disp, float diff, unsigned min_area,
                 void* labels, void* sizes, void* totals);

/* Extension (parity unpinned by the reference), the hole filling of include/sgm_mi355x.h (sgm_set_fill_holes); sgm_fill.hip.
 * classify: one byte per pixel of all B frames, 0 valid / 1 occluded / 2 mismatched, from the reference view's WTA map `ref` and
 * the other view's `oth` as they are BEFORE the LR check (right != 0: the right view is the reference view); all 0 if !do_check.
 * pass: one Jacobi pass (1 occluded, 2 mismatched, 3 every INF pixel; cls may be NULL for pass 3) of the 8-ray fill, walks of at
 * most R steps, `in` -> `out` (distinct buffers).  sgm_host.c references both weakly (a host built without them has no filling). */
int sgmd_fill_classify(int ord, void* stream, const sgmd_geom* g, const void* ref, const void* oth, float thres, int right,
                       int do_check, void* cls);
int sgmd_fill_pass(int ord, void* stream, const sgmd_geom* g, int R, const void* in, void* out, const void* cls, int pass);

/* Extension (parity unpinned by the reference), the refinement of include/sgm_mi355x.h (sgm_set_refine); sgm_refine.hip.
 * One pass of one iteration over all B frames: vertical == 0 solves every row, else every column, of both right-hand sides U and V
 * in place (f32 [B][H][W] each), with Q (f32 [B][H][W]) as scratch for q_i.  table: the iteration's L_t[256] (host memory, passed by
 * value).  first (horizontal only): U and V are built from disp (f32, +INF invalid) and conf (u16) instead of read.  last (vertical
 * only): out = V > 0 ? U / V : +INF, and with keep_invalid +INF where out itself was +INF before (out may be disp).
 * sgm_host.c references it weakly (a host built without it has no refinement). */
int sgmd_refine_pass(int ord, void* stream, const sgmd_geom* g, int vertical, const float* table, const void* guide,
                     const void* disp, const void* conf, void* U, void* V, void* Q, int first, int last, int keep_invalid,
                     void* out);

/* Extension (parity unpinned by the reference), the rectification of include/sgm_mi355x.h (SGM_SetRectify); sgm_rectify.hip.
 * One launch for both views of all B frames: out_left / out_right (u8 [B][H][W]) = left / right sampled through the quantised maps.
 * maps: int32 [view: left, right][plane: xq, yq][SGMD_REMAP_PITCH(W * H)], entry p = y * W + x, the padding holding -64
 * ("outside").  No output may alias an input.  sgm_host.c references it weakly (a host built without it has no rectification). */
#define SGMD_REMAP_PITCH(n) (((size_t)(n) + 3) & ~(size_t)3)
int sgmd_remap(int ord, void* stream, const sgmd_geom* g, const void* maps, const void* left, const void* right, void* out_left,
               void* out_right);

/* Extension (parity unpinned by the reference), images of 9..16 bits per sample (include/sgm_mi355x.h, SGM_SetPixelBits);
 * sgm_pixels16.hip.  left / right (and the outputs of sgmd_remap16) are u16 [B][H][W], 2-byte aligned and nothing more.
 * sgmd_census16: ONE launch for both views of all B frames, with the block grid of sgmd_census: the census of the u16 samples as they
 * are -- symmetric != 0: the centre-symmetric census over cw x ch into u32 words (as sgmd_census_sym); else cw x ch == 5 x 5: the
 * reference's centre census into u32 words (as sgmd_census, every word written); else the wide centre census into u64 words (as
 * sgmd_census_window) -- and, beside it, the narrowed images g8 = min(v >> (bits - 8), 255), u8 [B][H][W], which every reader of
 * grey values downstream takes.  sgmd_remap16: sgmd_remap on u16 samples (same maps, taps and rounding).  sgm_host.c references
 * both weakly (a host built without them refuses more than 8 bits). */
int sgmd_census16(int ord, void* stream, const sgmd_geom* g, int bits, int symmetric, int cw, int ch, const void* left,
                  const void* right, void* census_l, void* census_r, void* g8_left, void* g8_right);
int sgmd_remap16(int ord, void* stream, const sgmd_geom* g, const void* maps, const void* left, const void* right, void* out_left,
                 void* out_right);

/* in-place raster-order 3x3 median (the reference calls MedianFilter with in == out, .c:120).
 * scratch: sgmd_median_scratch_bytes(g) bytes for the pre-sorted neighbourhoods. */
/* status: NULL, or an int in page-locked host memory (sgmd_alloc_pinned) that the chained kernel of tall frames sets to 1 when a
 * band gave up waiting for the rows of the band above (bounded polls): the map is then wrong and the host fails the match */
size_t sgmd_median_scratch_bytes(const sgmd_geom* g);
int sgmd_median(int ord, void* stream, const sgmd_geom* g, void* disp, void* scratch, void* status);

/* SURVEY.md 8f-3 on device buffers: depth[mm] = float32(fx * baseline) / (disparity + doffs), NaN where the denominator is not
 * finite or zero; and (blocking) the sums behind RMSE / bad-pixel rate over the pixels finite in both depth images */
int sgmd_depth(int ord, void* stream, const void* disp, size_t n, float fx, float baseline, float doffs, void* depth);
int sgmd_score(int ord, void* stream, const void* ground_truth, const void* test, size_t n, float abs_thresh, double* sum_sq,
               unsigned long long* n_valid, unsigned long long* n_bad);

/* Extension: depth from both views' maps as the test platform combines them (depth_image.py:167-197): sgmd_depth of disp_l with
 * fx_l where that is finite, else sgmd_depth of disp_r with fx_r at the same pixel (no warping).  Weakly referenced by sgm_host.c. */
int sgmd_depth_both(int ord, void* stream, const void* disp_l, const void* disp_r, size_t n, float fx_l, float fx_r, float baseline,
                    float doffs, void* depth);

/* Extension (parity unpinned by the reference), the point clouds of include/sgm_mi355x.h (sgm_cloud_spec); sgm_cloud.hip.
 * c: the spec as the host validated it, fb = (float)((double)fx * (double)baseline).  disp f32, mask u8 or NULL, conf u16 or NULL,
 * [B][H][W] each.  sgmd_cloud_organized: xyz f32 [B][H][W][3], X Y Z of a kept pixel, three quiet NaNs (0x7FC00000) elsewhere.
 * sgmd_cloud_points: the kept pixels as 16-byte records {x, y, z, pixel = y << 16 | x} packed in raster order into points (room
 * for B * W * H records, 16-byte aligned; records past the total are not written) and offsets u32 [B + 1]; three launches (count,
 * scan, emit) that use scratch, sgmd_cloud_scratch_bytes(W, H, B) bytes, which must not be shared with a call still in flight.
 * sgm_host.c references all three weakly (a host built without them answers false to the cloud entry points). */
typedef struct {
    int W, H, B;
    float fx, fy, cx, cy, fb, doffs, z_min, z_max;
    unsigned min_conf;
} sgmd_cloud;
size_t sgmd_cloud_scratch_bytes(int W, int H, int B);
int sgmd_cloud_organized(int ord, void* stream, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, void* xyz);
int sgmd_cloud_points(int ord, void* stream, const sgmd_cloud* c, const void* disp, const void* mask, const void* conf, void* scratch,
                      void* points, void* offsets);

/* Extension (parity unpinned by the reference), depth registered to another camera (include/sgm_mi355x.h, sgm_register_spec);
 * sgm_register.hip.  c: the source as the cloud entry points take it; r: the target as the host validated it.  disp, mask, conf:
 * the source maps, [B][c->H][c->W].  sgmd_register_depth: depth f32 and source u32 (or NULL), [B][r->H][r->W]; three launches
 * (clear, scatter, resolve) that use keys, sgmd_register_scratch_bytes(r->W, r->H, B) bytes (one 8-byte key per target pixel, an
 * even number of them), 16-byte aligned, which must not be shared with a call still in flight.  sgmd_register_gather:
 * out[f][v][u] = source[f][v][u] names a pixel (y, x) of the source ? map[f][y][x] : fill, elements of elem_bytes (1, 2, 4); fill:
 * the element in the low bytes.  sgm_host.c references all three weakly (a host built without them answers false). */
typedef struct {
    int W, H;
    float fx, fy, cx, cy, dist[5], R[9], t[3], z_min, z_max;
    int splat;
} sgmd_register;
size_t sgmd_register_scratch_bytes(int W, int H, int B);
int sgmd_register_depth(int ord, void* stream, const sgmd_cloud* c, const sgmd_register* r, const void* disp, const void* mask,
                        const void* conf, void* keys, void* depth, void* source);
int sgmd_register_gather(int ord, void* stream, const sgmd_cloud* c, const sgmd_register* r, const void* source, int elem_bytes,
                         const void* map, unsigned fill, void* out);

/* The frames of one call of the volume's integration, its ray-cast and tracking, one pose each: the poses travel as kernel
 * arguments, 3 KiB of the 4 KiB a launch may take */
#define SGMD_MAX_POSES 64

/* Extension (parity unpinned by the reference), depth fused into a TSDF volume (include/sgm_mi355x.h, sgm_volume_spec);
 * sgm_volume.hip.  v: the volume as the host validated it; c: the source as the cloud entry points take it (c->B <= 64).
 * sgmd_volume_integrate: poses (HOST, [c->B][12], read before it returns: they travel as kernel arguments), disp, mask, conf
 * [B][c->H][c->W], voxels u32 [nz][ny][nx] updated in place by one launch.  sgmd_volume_points: three launches (count per tile,
 * one scan, emit) that use scratch, sgmd_volume_scratch_bytes(nx, ny, nz) bytes, which must not be shared with a call still in
 * flight; points: 16-byte records sorted by id, those at index >= capacity not written; count[0]: the number of crossings.
 * sgm_host.c references all three weakly (a host built without them answers false). */
typedef struct {
    int nx, ny, nz;
    float voxel, origin[3], trunc;
    unsigned max_weight;
} sgmd_volume;
size_t sgmd_volume_scratch_bytes(int nx, int ny, int nz);
int sgmd_volume_integrate(int ord, void* stream, const sgmd_volume* v, const sgmd_cloud* c, const float* poses, const void* disp,
                          const void* mask, const void* conf, void* voxels);
int sgmd_volume_points(int ord, void* stream, const sgmd_volume* v, const void* voxels, unsigned min_weight, void* scratch,
                       void* points, size_t capacity, void* count);

/* The volume ray-cast into depth and normal maps of a view (include/sgm_mi355x.h, sgm_raycast_spec); sgm_volume.hip.  r: the view as
 * the host validated it (r->B <= 64 frames, one pose each).  poses: HOST, [r->B][12], read before it returns.  One launch, no
 * scratch: depth f32 [B][H][W], normal f32 [B][H][W][3] or NULL (then not written).  sgm_host.c references it weakly, on its own:
 * a host built without it answers false to sgm_volume_raycast and keeps the rest of the volume. */
typedef struct {
    int W, H, B;
    float fx, fy, cx, cy, z_min, z_max, step;
    unsigned min_weight;
} sgmd_raycast;
int sgmd_volume_raycast(int ord, void* stream, const sgmd_volume* v, const sgmd_raycast* r, const float* poses, const void* voxels,
                        void* depth, void* normal);

/* Colour in the volume (include/sgm_mi355x.h, the colour section); sgm_volume.hip.  colors: u32 [nz][ny][nx] beside the voxels,
 * (cw << 24) | (b << 16) | (g << 8) | r.  sgmd_volume_integrate_color: sgmd_volume_integrate with the source's image (u8 grey with
 * channels 1, u32 r | g << 8 | b << 16 with channels 4, [B][c->H][c->W]) fused into colors by the same launch.
 * sgmd_volume_raycast_color: sgmd_volume_raycast with rgba u32 [B][H][W] written beside depth and normal (NULL: not written).
 * sgmd_volume_colors: one launch, no scratch: rgba[r] for every 16-byte record r < capacity (and < count[0] where count, a device
 * word, is not NULL) whose last word is the id n * id_kinds + e of a mesh vertex (id_kinds 8) or of a surface point (4).
 * sgm_host.c references each weakly, on its own: a host built without one answers false to its entry point and keeps the rest. */
int sgmd_volume_integrate_color(int ord, void* stream, const sgmd_volume* v, const sgmd_cloud* c, const float* poses, const void* disp,
                                const void* mask, const void* conf, const void* image, int channels, void* voxels, void* colors);
int sgmd_volume_raycast_color(int ord, void* stream, const sgmd_volume* v, const sgmd_raycast* r, const float* poses, const void* voxels,
                              const void* colors, void* depth, void* normal, void* rgba);
int sgmd_volume_colors(int ord, void* stream, const sgmd_volume* v, const void* voxels, const void* colors, const void* records,
                       size_t capacity, const void* count, int id_kinds, void* rgba);

/* A window of the volume (include/sgm_mi355x.h, the moving-volume section); sgm_window.hip.  One launch, no scratch: destination
 * voxel (i, j, k) of the dims[0] x dims[1] x dims[2] grid receives the source word of (i + offset[0], j + offset[1], k + offset[2])
 * where that lies inside src's grid, else 0; the colour words alike where src_colors / dst_colors are given (both or neither).
 * src: the source volume as the host validated it; dims 1..1024 each and at most 2^30 voxels, |offset| <= 2^20; the arrays 4-byte
 * aligned and, the destination's against all others, disjoint.  sgm_host.c references it weakly, on its own. */
int sgmd_volume_window(int ord, void* stream, const sgmd_volume* src, const int* offset, const int* dims, const void* src_voxels,
                       const void* src_colors, void* dst_voxels, void* dst_colors);

/* The distance field of the volume (include/sgm_mi355x.h, the distance section); sgm_distance.hip.  v: the volume as the host validated
 * it; min_weight 1..65535, radius 1..255, side and unknown 0 or 1.  sgmd_volume_distance: dist2 u16 [nz][ny][nx], 2-byte aligned and
 * disjoint from voxels, every word written; up to three launches (the x pass, then y and z in place where those axes are longer than
 * one voxel), no scratch.  sgmd_volume_distance_field: field f32 [nz][ny][nx] from the side-0 words out2 and the side-1 words in2 (or
 * NULL), one launch, no scratch.  sgm_host.c references both weakly, on their own. */
int sgmd_volume_distance(int ord, void* stream, const sgmd_volume* v, unsigned min_weight, int radius, int side, int unknown,
                         const void* voxels, void* dist2);
int sgmd_volume_distance_field(int ord, void* stream, const sgmd_volume* v, const void* out2, const void* in2, void* field);

/* The volume as a triangle mesh, marching tetrahedra (include/sgm_mi355x.h, sgm_volume_mesh); sgm_mesh.hip. v: the volume as the
 * host validated it, at most 2^27 voxels.  Four launches (count per tile, one scan, the vertices, the triangles; the last two only
 * where their capacity is not 0) that use scratch, sgmd_mesh_scratch_bytes(nx, ny, nz) bytes -- two sets of tile words -- which
 * must not be shared with a call still in flight.  vertices, triangles: 16-byte records, those at index >= their capacity not
 * written, and no triangle unless the whole vertex list was; counts[0], counts[1]: the full numbers of vertices and triangles.
 * sgm_host.c references both weakly, on their own: a host built without them answers false to sgm_volume_mesh and keeps the rest
 * of the volume. */
size_t sgmd_mesh_scratch_bytes(int nx, int ny, int nz);
int sgmd_volume_mesh(int ord, void* stream, const sgmd_volume* v, const void* voxels, unsigned min_weight, void* scratch,
                     void* vertices, size_t vertex_capacity, void* triangles, size_t triangle_capacity, void* counts);

/* Extension (parity unpinned by the reference), the sums of frame-to-model tracking (include/sgm_mi355x.h, sgm_track_spec);
 * sgm_track.hip.  c: the source as the host validated it (c->B <= 64 frames, one pose each, c->W * c->H <= 2^24); t: the model view.
 * poses: HOST, [c->B][12], source camera -> model camera, read before it returns.  model_depth f32 [B][t->H][t->W], model_normal
 * f32 [B][t->H][t->W][3]; sums int64 [B][29], 8-byte aligned, zeroed on the stream and then added to with integer atomics.
 * One launch, no scratch.  sgm_host.c references it weakly, on its own: a host built without it answers false to sgm_track_sums and
 * sgm_track. */
typedef struct {
    int W, H;
    float fx, fy, cx, cy, dist_max, span;
} sgmd_track;
int sgmd_track_sums(int ord, void* stream, const sgmd_cloud* c, const sgmd_track* t, const float* poses, const void* disp,
                    const void* mask, const void* conf, const void* model_depth, const void* model_normal, void* sums);

/* Extension (parity unpinned by the reference), planes in a point list (include/sgm_mi355x.h, sgm_plane_spec); sgm_plane.hip.
 * p: the spec as the host validated it (threshold = min_cos * |axis| as the header rounds it, prior = the axis is not all zero).
 * records: 16-byte records {x, y, z, tag}, 16-byte aligned, capacity <= 2^32 of them (2^24 for the sums); count: a device u32 or
 * NULL; labels: device u8 [capacity] or NULL (sgmd_plane_label: never NULL); planes / plane / best: device sgm_plane, 16-byte
 * aligned; sums: int64 [10], 8-byte aligned, zeroed on the stream and then added to with integer atomics.  sgmd_plane_votes: two
 * launches (the candidates, the vote); the others one each; no scratch.  sgm_host.c references each weakly, on its own. */
typedef struct {
    int hypotheses;
    unsigned seed;
    float dist, axis[3], threshold, span;
    int prior;
} sgmd_plane;
int sgmd_plane_votes(int ord, void* stream, const sgmd_plane* p, const void* records, size_t capacity, const void* count,
                     const void* labels, void* planes);
int sgmd_plane_best(int ord, void* stream, const void* planes, int K, void* best);
int sgmd_plane_sums(int ord, void* stream, const sgmd_plane* p, const void* records, size_t capacity, const void* count,
                    const void* labels, const void* plane, void* sums);
int sgmd_plane_label(int ord, void* stream, const sgmd_plane* p, const void* records, size_t capacity, const void* count,
                     const void* plane, int label, void* labels);

/* Extension (parity unpinned by the reference), connected components of the volume's voxel lattice (include/sgm_mi355x.h, the
 * components section); sgm_components.hip.  v: the volume as the host validated it; cs: the spec as the host validated it (the planes
 * as normal, anchor and clearance; a void plane is skipped).  sgmd_volume_components: labels u32 [nz][ny][nx], the call's working array
 * and its result; objects: 48-byte records, 8-byte aligned, or NULL with capacity 0; counts u32 [2]; scratch:
 * sgmd_components_scratch_bytes(nx, ny, nz, capacity) bytes, 8-byte aligned, which must not be shared with a call still in flight.
 * Five launches for labels and counts (three where the volume is one tile), three more for the records.  sgmd_volume_component_of: one
 * launch, no scratch: index[r] for every 16-byte record r < records_capacity (and < records_count[0] where that device word is
 * given).  sgm_host.c references all three weakly, on their own. */
typedef struct {
    unsigned min_weight;
    int set, unknown, connectivity;
    unsigned min_voxels;
    int planes;
    float normal[4][3], anchor[4][3], clearance[4];
} sgmd_components;
size_t sgmd_components_scratch_bytes(int nx, int ny, int nz, size_t capacity);
int sgmd_volume_components(int ord, void* stream, const sgmd_volume* v, const sgmd_components* cs, const void* voxels, void* scratch,
                           void* labels, void* objects, size_t capacity, void* counts);
int sgmd_volume_component_of(int ord, void* stream, const sgmd_volume* v, const void* labels, const void* objects, size_t capacity,
                             const void* counts, const void* records, size_t records_capacity, const void* records_count, int id_kinds,
                             void* index);

/* Extension (parity unpinned by the reference), matching at 1/f scale (include/sgm_mi355x.h, sgm_scale_spec); sgm_scale.hip.
 * c: the spec as the host validated it (W, H: FULL resolution; the low resolution is W / f x H / f).  sgmd_downscale: the f x f box
 * mean with rounding of one image stack, u8 (bits == 8) or u16 [B][H][W] -> [B][H / f][W / f]; trailing rows and columns are not
 * read; no alignment beyond the element's.  sgmd_upscale: disp_full f32 [B][H][W] from disp_small f32 and guide_small [B][H / f][W / f],
 * guide_full and the u32 census planes of the reference and the other view [B][H][W] (unused, may be NULL, with radius < 0); every
 * census column is bounds-checked, nothing in front of a plane is read.  sgm_host.c references both weakly (a host built without
 * them answers false to the scaled entry points). */
typedef struct {
    int W, H, B;
    int f, bits, radius, penalty, d_lo, d_hi, right;
} sgmd_scale;
int sgmd_downscale(int ord, void* stream, const sgmd_scale* c, const void* in, void* out);
int sgmd_upscale(int ord, void* stream, const sgmd_scale* c, const void* disp_small, const void* guide_small, const void* guide_full,
                 const void* census_ref, const void* census_oth, void* disp_full);

/* Extension (parity unpinned by the reference), the temporal filter of include/sgm_mi355x.h (sgm_temporal_spec); sgm_temporal.hip.
 * p: the spec as the host validated it -- a = alpha, b = 1.0f - a rounded once by the host, n = 0..8, k = 1..n (n == 0: not looked
 * at).  maps f32 [streams][steps][pixels], filtered in place; conf u16 of that shape or NULL (also with min_conf == 0: the test
 * is then always true); hist_value f32 and hist_bits u8 [streams][pixels], read once and written once per call however many
 * steps; stats u32 [streams * steps][5] or NULL, zeroed by the call on the stream, then counted; scratch: NULL, or
 * sgmd_temporal_scratch_bytes() bytes the call spreads the waves' counter adds over before it sums them into stats (few maps are
 * few cache lines for thousands of adds), which must not be shared with a call still in flight.  No alignment beyond the
 * element's: pointers or a pixel count that do not allow 16-byte accesses take a one-pixel-per-lane path with the same results.
 * streams, steps, pixels >= 1 and streams * steps * pixels <= 2^31.  sgmd_temporal_clear: hist_value <- +INF, hist_bits <- 0,
 * count entries each.  sgm_host.c references both weakly (a host built without them answers false to the temporal entry points). */
typedef struct {
    float a, b, delta;
    int n, k;
    unsigned min_conf;
} sgmd_temporal_params;
int sgmd_temporal(int ord, void* stream, const sgmd_temporal_params* p, size_t streams, size_t steps, size_t pixels, void* maps,
                  const void* conf, void* hist_value, void* hist_bits, void* stats, void* scratch);
size_t sgmd_temporal_scratch_bytes(void);
int sgmd_temporal_clear(int ord, void* stream, size_t count, void* hist_value, void* hist_bits);

/* grey = (weight_r r + 150 g + 29 b) >> 8 of three consecutive n-byte planes B, G, R (the test platform's frame
 * format, server.py:105-131; the firmware's conversion, stereo_matching.c:18-25) */
int sgmd_gray_planes(int ord, void* stream, const void* bgr, size_t n, int weight_r, void* gray);

#ifdef __cplusplus
}
#endif
#endif
