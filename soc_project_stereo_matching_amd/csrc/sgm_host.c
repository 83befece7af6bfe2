/*
 * sgm_host.c -- the C host of libsgm_mi355x.so.
 *
 * Implements the reference's library boundary (SGM_Initialize / SGM_Reset / SGM_Match,
 * /root/reference/SemiGlobalMatching/SemiGlobalMatching/SemiGlobalMatching.h:78-80) plus the
 * extensions of include/sgm_mi355x.h on top of the HIP stage launchers of sgm_device.h.
 * This file owns everything that is not a kernel: option validation, buffer sizing, the
 * adaptive-P2 table, the path-geometry tables for the anomalous diagonal lines and the order
 * of the stages (the body of SGM_Match, SemiGlobalMatching.c:77-122).
 *
 * There is no CPU fallback: without a usable gfx950 device every entry point fails loudly.
 */
#include "../../include/sgm_mi355x.h"
#include "sgm_device.h"

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define SGM_VERSION_STRING "sgm_mi355x 0.3 (gfx950, hand-written HIP)"
#define CENSUS_FRONT_SLACK ((size_t)(65535 + SGM_MAX_DISPARITY_RANGE + 8 + 63) / 64 * 64 * 4)   /* >= sgmd_census_slack() for any options */
/* the aggregation loads a wave's census run in whole 16-byte groups, up to 12 words past the last pixel: readable bytes behind
 * the census-right words (allocated, never written: nothing uses what is read there) */
#define CENSUS_BACK_SLACK ((size_t)64)

#define TIMING_RING 64
enum { T_CENSUS, T_COST, T_AGGREGATE, T_SUM, T_WTA, T_LRCHECK, T_SPECKLE, T_MEDIAN, T_COUNT };
/* event marks of a match: 0 .. T_COUNT bracket the stages in order; one more, M_SUM_BEGIN, sits right in front of the cost sum
 * BEHIND its waits for other streams' events, so that "sum" is the kernel's time and not the wait for the previous post pass */
#define M_END T_COUNT
#define M_SUM_BEGIN (T_COUNT + 1)
#define MARKS_PER_MATCH (T_COUNT + 2)
static const char* const k_stage_names[T_COUNT] = {"census", "cost", "aggregate", "sum", "wta", "lrcheck", "speckle", "median"};

/* reference direction order, SemiGlobalMatching.c:213-220 */
static const int k_dir_dx[8] = {1, -1, 0, 0, 1, -1, 1, -1};
static const int k_dir_dy[8] = {0, 0, 1, -1, 1, -1, -1, 1};

/* A device or page-locked buffer the instance owns, its capacity in bytes beside it: buffers only grow, so a Reset with the same
 * shape allocates nothing.  reserve() sizes them, free_device_buffers() walks k_buffers, nothing else allocates or frees one. */
typedef struct { void* p; size_t cap; } sgm_buf;
typedef struct { void* dst; const void* src; size_t bytes; } handover;     /* a staged output on its way to the caller (sgm_match_wait) */

/* Where S lives, the aggregated-cost sum of the matches since the last Reset (quirk Q14: a Match without Reset adds to it).  The
 * fused kernels do not store it: it stays spread over the direction planes of the last frame until somebody needs it (a Match
 * without Reset, a stage read) and then replaces what d_S holds (the first match behind a Reset) or adds to it; behind a fused last
 * sweep the three upward planes of that frame are missing as well.  Three writers: sum_reset (Initialize / Reset), sum_accepted (a
 * cost-sum launch was accepted: exactly then, so a refused launch leaves the matches that completed described) and materialize_S. */
typedef enum { S_ZERO, S_STORED, S_IN_PLANES, S_IN_PLANES_ADDS } sum_where;
typedef struct { sum_where where; bool up_missing; } sum_state;

/* refinement parameters (sgm_set_refine) and the weight tables L_t of their iterations */
typedef struct {
    float lambda, sigma;
    int iters, keep_invalid;
    float tab[SGM_REFINE_MAX_ITERS][256];
} refine_params;

struct sgm_instance {
    int device;
    void* stream;                /* census and aggregation; and every other stage unless it has a stream of its own (sgm_set_stage_cus) */
    void* sum_stream;            /* cost sum + both WTAs, behind ev_agg (the aggregation is done) */
    void* post_stream;           /* LR check, speckle removal and median, behind ev_sum (cost sum + WTAs done); ev_post = post pass done */
    void *ev_agg, *ev_sum, *ev_post;
    int overlap_post;
    bool sum_pending;            /* a cost sum is (possibly) still reading the planes on sum_stream */
    bool post_pending;           /* a post pass is (possibly) still running on post_stream */
    void* tail_stream;           /* the stream the last match's final kernel was queued on (NULL: stream) */
    int cu_first[3], cu_count[3];/* CUs per XCD of the main / sum / post stream (count 0: all CUs) */
    int up_rows;                 /* > 0: the last vertical sweep (directions (0,-1), (-1,-1), (1,-1)) runs fused with the cost sum and both WTAs
                                    (sgmd_upsum) wherever a match allows it: image rows per workgroup of that kernel */
    sgm_buf d_up_scratch;        /* its hand-over rows, progress words and tickets */
    sgm_buf d_left_keep;         /* copy of the last fused match's left image(s): what re-creating the three planes needs (Q14, stage read-back) */
    unsigned up_gen;             /* launch counter of the fused kernel (its progress words carry it) */
    int up_key[5];               /* B, W, H, Dp, rows per workgroup of the fused launches the scratch's progress words belong to
                                    ([0] == 0: none, the scratch is to be zeroed): ensure_upsum */
    int last_up_rows;            /* rows per workgroup of the fused sweep in the LAST match, 0 if it ran the separate kernels */
    int env_upsum, env_upsum_rows, env_upsum_wgs;   /* SGM_UPSUM, SGM_UPSUM_ROWS, SGM_UPSUM_WGS */
    int env_lanes, env_hl, env_agg_fast, env_fused;   /* SGM_LANES_PER_PIXEL, SGM_HL, SGM_AGG_FAST, SGM_FUSED_WTA as read at sgm_create
                                    (-1: not set) -- tuning / test knobs, not looked up again on the per-frame sgm_reset path */
    bool stage_prio[3];          /* that stream was made by sgm_set_stage_priority (an all-CU request must replace it, not keep it) */
    int* h_status;               /* page-locked word the chained median kernel sets when a band gave up waiting (sgmd_median) */
    void* timer;
    int timing;
    int keep_stages;
    int honor_num_paths;
    int census_w, census_h;      /* census window (sgm_set_census_window); 0 = the reference's 5x5 */
    int census_kind;             /* SGM_CENSUS_CENTRE (reference) or SGM_CENSUS_SYMMETRIC (sgm_set_census_kind) */
    int reference_view;          /* 0 = left (reference), 1 = right (sgm_set_reference_view) */
    int pixel_bits_req;          /* bits per image sample asked for (sgm_set_pixel_bits; 0 = never set = 8); takes effect at the next initialize */
    int pixel_bits;              /* ... and in effect for this shape: 8 = u8 images (reference), 9..16 = u16 images */
    int fill_req;                /* hole filling asked for (sgm_set_fill_holes); takes effect at the next initialize */
    bool fill_on;                /* ... and in effect for this shape: the class map and the ping-pong map exist */
    int refine_req;              /* refinement asked for (sgm_set_refine); takes effect at the next initialize */
    bool refine_on;              /* ... and in effect for this shape: its maps exist */
    int reference_statics;       /* the default instance behind SGM_Initialize / SGM_Reset / SGM_Match: its census buffers behave like
                                    the reference's static arrays (SemiGlobalMatching.h:67-68) -- zero at first, never cleared, the words
                                    census_transform_5x5 does not write (.c:136,140-141) keep what an earlier frame of another shape left
                                    at the same linear index.  Explicit instances (an extension) write those words as 0 */
    int batch;                   /* frames per match call (>= 1); takes effect at the next initialize */
    int read_frame;              /* which frame of the batch sgm_read_stage returns */
    int tile_begin, tile_end;    /* row tile this instance computes (sgm_set_rows); tile_end == 0: the whole frame */
    const void* tile_left;       /* left image of the frame a tile sequence is working on */

    bool initialized;
    sum_state S;                 /* the aggregated-cost volume: logically zero, in d_S, or still in the planes (Q14) */
    int fused_wta;               /* Dp <= 256: cost sum and both WTA passes in one kernel, S not written */
    SGMOption opt;
    sgmd_geom g;
    sgmd_paths paths;
    int need_plane_memset;       /* W < H: diagonal planes are cleared before aggregation */
    int row_cap;
    float last_ms[T_COUNT];
    bool have_ms;
    /* timing history: TIMING_RING event sets, one per match since the last collection */
    int ring_next, ring_pending;          /* next set to record into; sets recorded and not yet read */
    double sum_ms[T_COUNT], min_ms[T_COUNT];
    long n_timed;

    /* device buffers (every sgm_buf of the instance is listed in k_buffers below) */
    int plane_row_lo, plane_rows;        /* image rows a direction plane has storage for: [plane_row_lo, plane_row_lo + plane_rows) --
                                            the whole frame normally, the tile's rows + one hand-over row either side in row-tile mode */
    int tab_W, tab_H, tab_ndirs, tab_p1, tab_p2;   /* what the uploaded tables were built for */
    sgm_buf d_left, d_right, d_census_l, d_census_r_alloc, d_cost, d_planes_alloc, d_extras, d_S;
    void *d_census_r, *d_planes; /* d_census_r = d_census_r_alloc + CENSUS_FRONT_SLACK;
                                    d_planes = d_planes_alloc - plane_row_lo rows: kernels address cells by their frame
                                    position; d_cost and d_S exist only once somebody needs them (stage read-back, Q14, D > 256) */
    sgm_buf d_disp, d_disp_r, d_labels, d_sizes, d_lut, d_row_extras, d_row_count;
    sgm_buf d_snap_wta, d_snap_lr, d_snap_speckle, d_totals, d_median_scratch;
    sgm_buf d_census64_l, d_census64_r;  /* u64 census words of the wide windows (allocated on first use) */
    sgm_buf d_census_need;               /* row tiles: which 64 x 16 blocks of the census this instance reads (sgmd_census) */
    int need_key[7];                     /* W, H, rows, dmin, Dp, ndirs the map was built for */
    sgm_buf d_bgr, d_depth, h_bgr;       /* a test-platform frame's six colour planes, its depth map, pinned staging (first use) */
    sgm_buf d_fill_class, d_fill_map;    /* hole filling: u8 class map and the f32 ping-pong map ([B][H][W] each; only when asked for) */
    sgm_buf d_conf, h_conf;              /* device / page-locked staging of the host-pointer confidence entry points (first use) */
    refine_params rf_req, rf_eff;        /* refinement: the parameters last set (sgm_refine_disparity) and those of the matches */
    sgm_buf d_rf_u, d_rf_v, d_rf_q;      /* its right-hand sides / solutions and the q_i of the line solves, f32 [B][H][W] each */
    sgm_buf d_rf_conf;                   /* the confidence of a match whose caller did not ask for it, u16 [B][H][W] */
    sgm_buf d_rf_guide[2];               /* private copies of the reference image, used by turns (u8 [B][H][W] each) */
    int rf_turn;
    /* rectification (sgm_set_rectify): the host's quantised copy of the maps last set (NULL: none; the layout sgmd_remap reads) and
     * their shape; takes effect at the next initialize, which uploads them when they are new or the device copy is gone */
    int32_t* rect_q;
    int rect_w, rect_h;
    bool rect_dirty;                     /* the device copy is not (or no longer) that of rect_q */
    bool rect_on;                        /* ... and in effect for this shape: every match rectifies its images first */
    sgm_buf d_rect_maps, d_rect_l, d_rect_r;   /* the maps; the rectified images, u8 (u16 with more than 8 bits) [B][H][W] each: what every
                                            stage below the remap reads */
    sgm_buf d_g8_l, d_g8_r;              /* more than 8 bits per sample: the narrowed images the census writes on the side, u8 [B][H][W]
                                            each: what every reader of grey values below the census takes */
    /* both views' maps from one match (sgm_match_both; all allocated at its first use): the raw left WTA map (f32 [B][H][W]; the raw
     * right one is d_disp_r), the two finished maps as ONE batch of 2 B maps (f32 [2 B][H][W]: the left maps, then the right ones),
     * the speckle and median scratch of such a batch, the right view's snapshots for sgm_keep_stages (after the LR check, after
     * speckle removal: f32 [2][B][H][W]) and the page-locked staging of the right map */
    sgm_buf d_both_raw, d_both_maps, d_both_labels, d_both_sizes, d_both_totals, d_both_median, d_both_snap, h_disp_r;
    /* point clouds (sgm_cloud_points / sgm_read_cloud; allocated at the first such call): the tile counts and bases of the point list's
     * three launches, and the list and offsets sgm_read_cloud makes on the device before it copies them */
    sgm_buf d_cloud_scratch, d_cloud_points, d_cloud_offsets;
    /* registration (sgm_register_depth; allocated at the first such call): one 8-byte z-buffer key per target pixel */
    sgm_buf d_register_keys;
    /* TSDF volume (sgm_volume_points; allocated at the first such call): the tile counts and bases of the surface list's three launches */
    sgm_buf d_volume_scratch;
    /* the volume's mesh (sgm_volume_mesh; allocated at the first such call): the two sets of tile words of its four launches */
    sgm_buf d_mesh_scratch;
    /* tracking (allocated at the first such call): the sums of a round of sgm_track, 29 int64 per frame, and whatever scratch the
     * launcher asks for (none in the default build) */
    sgm_buf d_track_sums;
    /* planes in a point list (sgm_plane_fit; allocated at its first call): 1024 candidates, the plane that travels between the
     * rounds and the ten sums of a round */
    sgm_buf d_plane_work;
    /* connected components of the volume (sgm_volume_components; allocated at its first call): the sizes, the compaction's tile words
     * and the boxes of the objects */
    sgm_buf d_components_scratch;
    /* matching at 1/f scale (sgm_match_scaled; allocated at its first use): the downscaled views, the census planes of the
     * FULL-resolution views with the narrowed images sgmd_census16 writes beside them, and for the host-pointer form the full
     * images, the full map and their page-locked staging */
    sgm_buf d_sc_small_l, d_sc_small_r, d_sc_census_l, d_sc_census_r, d_sc_g8_l, d_sc_g8_r, d_sc_full_l, d_sc_full_r, d_sc_disp;
    sgm_buf h_sc_l, h_sc_r, h_sc_disp;
    /* temporal filter (sgm_set_temporal): the spec last set and whether one is; the spec in effect for this shape and whether one is.
     * The history -- hv f32 and hb u8 [views][streams][H][W], streams = B or (sequence) 1 --, the counters u32 [views][B][5], and for
     * sgm_keep_stages the maps as they entered the filter (f32 [views][B][H][W]); the second view's share only once a
     * sgm_match_both ran.  tp_sig: W, H, B, reference view, views, sequence of the last filtered match ([0] == 0: none, the
     * history is to be cleared); tp_restart: a clear is owed for another reason (sgm_set_temporal, sgm_temporal_restart);
     * tp_stat_maps: counter rows the last match filled (0: none) */
    sgm_temporal_spec tp_req, tp_eff;
    bool temporal_req, temporal_on;
    sgm_buf d_tp_value, d_tp_bits, d_tp_stats, d_tp_pre;
    sgm_buf d_tp_scratch;        /* where a filter launch that counts spreads its counter adds (sgmd_temporal_scratch_bytes; first use) */
    int tp_sig[6];
    bool tp_restart;
    int tp_stat_maps;
    bool last_both;              /* the last match was a sgm_match_both that was queued to its end: stage 8 is the first half of d_both_maps */
    bool last_both_kept;         /* ... and it ran with sgm_keep_stages: d_both_snap holds ITS right-view snapshots (stages 26, 27) */
    size_t plane_bytes;
    /* pinned staging for the host-pointer entry point */
    sgm_buf h_left, h_right, h_disp;
    /* a host-pointer match whose result has been queued on the stream and not yet handed to the caller: what sgm_match_wait still
     * has to copy from a staging buffer to the caller's pageable one (nothing for an output that is page-locked: the device writes it) */
    bool async_pending;
    handover async_out[3];       /* the map (or depth), the confidence, the right view's map */
    int async_n;
    /* the first of them may come back in async_chunks pieces, an event behind each but the last: sgm_match_wait copies piece i to the
     * caller while piece i + 1 is still on the bus (a 1242x375 map: 1.86 MB, ~40 us of DMA + ~90 us of memcpy in sequence otherwise) */
    void* ev_chunk[4];
    int async_chunks;
};
/* every buffer of the instance, for free_device_buffers: a new sgm_buf member gets its line here */
#define DEVICE_BUF(member) {offsetof(struct sgm_instance, member), false}
#define PINNED_BUF(member) {offsetof(struct sgm_instance, member), true}
static const struct { size_t offset; bool pinned; } k_buffers[] = {
    DEVICE_BUF(d_left), DEVICE_BUF(d_right), DEVICE_BUF(d_census_l), DEVICE_BUF(d_census_r_alloc), DEVICE_BUF(d_cost),
    DEVICE_BUF(d_planes_alloc), DEVICE_BUF(d_extras), DEVICE_BUF(d_S), DEVICE_BUF(d_disp), DEVICE_BUF(d_disp_r), DEVICE_BUF(d_labels),
    DEVICE_BUF(d_sizes), DEVICE_BUF(d_lut), DEVICE_BUF(d_row_extras), DEVICE_BUF(d_row_count), DEVICE_BUF(d_snap_wta),
    DEVICE_BUF(d_snap_lr), DEVICE_BUF(d_snap_speckle), DEVICE_BUF(d_totals), DEVICE_BUF(d_median_scratch), DEVICE_BUF(d_census64_l),
    DEVICE_BUF(d_census64_r), DEVICE_BUF(d_census_need), DEVICE_BUF(d_bgr), DEVICE_BUF(d_depth), PINNED_BUF(h_bgr),
    DEVICE_BUF(d_up_scratch), DEVICE_BUF(d_left_keep), DEVICE_BUF(d_fill_class), DEVICE_BUF(d_fill_map), DEVICE_BUF(d_conf),
    PINNED_BUF(h_conf), DEVICE_BUF(d_rf_u), DEVICE_BUF(d_rf_v), DEVICE_BUF(d_rf_q), DEVICE_BUF(d_rf_conf), DEVICE_BUF(d_rf_guide[0]),
    DEVICE_BUF(d_rf_guide[1]), PINNED_BUF(h_left), PINNED_BUF(h_right), PINNED_BUF(h_disp), DEVICE_BUF(d_both_raw),
    DEVICE_BUF(d_both_maps), DEVICE_BUF(d_both_labels), DEVICE_BUF(d_both_sizes), DEVICE_BUF(d_both_totals), DEVICE_BUF(d_both_median),
    DEVICE_BUF(d_both_snap), PINNED_BUF(h_disp_r), DEVICE_BUF(d_rect_maps), DEVICE_BUF(d_rect_l), DEVICE_BUF(d_rect_r),
    DEVICE_BUF(d_cloud_scratch), DEVICE_BUF(d_cloud_points), DEVICE_BUF(d_cloud_offsets), DEVICE_BUF(d_g8_l), DEVICE_BUF(d_g8_r),
    DEVICE_BUF(d_sc_small_l), DEVICE_BUF(d_sc_small_r), DEVICE_BUF(d_sc_census_l), DEVICE_BUF(d_sc_census_r), DEVICE_BUF(d_sc_g8_l),
    DEVICE_BUF(d_sc_g8_r), DEVICE_BUF(d_sc_full_l), DEVICE_BUF(d_sc_full_r), DEVICE_BUF(d_sc_disp), PINNED_BUF(h_sc_l), PINNED_BUF(h_sc_r),
    PINNED_BUF(h_sc_disp), DEVICE_BUF(d_tp_value), DEVICE_BUF(d_tp_bits), DEVICE_BUF(d_tp_stats), DEVICE_BUF(d_tp_pre),
    DEVICE_BUF(d_tp_scratch), DEVICE_BUF(d_register_keys), DEVICE_BUF(d_volume_scratch), DEVICE_BUF(d_mesh_scratch), DEVICE_BUF(d_track_sums),
    DEVICE_BUF(d_plane_work), DEVICE_BUF(d_components_scratch),
};
#define UPSUM_DEFAULT 0       /* the fused last sweep is opt-in (SGM_UPSUM=1) until it beats the separate kernels in the timed pipeline */
#define RESULT_CHUNKS 4
#define RESULT_CHUNK_MIN ((size_t)256 << 10)      /* smaller results are not worth the events */
#define RESULT_CHUNK_SPLIT ((size_t)4 << 20)      /* below this: two pieces */

#define FAIL(...)                                  \
    do {                                           \
        fprintf(stderr, "sgm_mi355x: " __VA_ARGS__); \
        fputc('\n', stderr);                       \
        return false;                              \
    } while (0)

/* row-tile mode (sgm_set_rows): the instance computes rows [tile_begin, tile_end) of every frame */
static bool row_tiled(const sgm_instance* s) { return s->tile_end != 0; }

/* The census decides two things.  reference_census: the reference's own 5x5 centre census (sgmd_census: the stale-border
 * quirk, the opt-in fused last sweep).  volume_fed: a wide centre window -- u64 words, a materialised cost volume and the
 * volume-fed aggregation.  Everything else about the fast path only asks for u32 words, i.e. !volume_fed: the symmetric kind
 * (at most 31 bits for any window) takes it whatever its window. */
static bool census_symmetric(const sgm_instance* s) { return s->census_kind == SGM_CENSUS_SYMMETRIC; }
static bool reference_census(const sgm_instance* s) { return !s->census_w && !census_symmetric(s); }
static bool volume_fed(const sgm_instance* s) { return s->census_w && !census_symmetric(s); }

static void sum_reset(sgm_instance* s) { s->S = (sum_state){S_ZERO, false}; }
static void sum_accepted(sgm_instance* s, sum_where where, bool up_missing) { s->S = (sum_state){where, up_missing}; }

/* pixels of one frame and of the batch a match works on (frame-major); maps are f32, images u8 */
static size_t frame_px(const sgm_instance* s) { return (size_t)s->g.W * s->g.H; }
static size_t batch_px(const sgm_instance* s) { return (size_t)s->g.B * frame_px(s); }
static size_t map_bytes(const sgm_instance* s) { return batch_px(s) * sizeof(float); }
/* images of more than 8 bits per sample (sgm_set_pixel_bits) are u16: the bytes of the caller's images of a batch */
static bool wide_pixels(const sgm_instance* s) { return s->pixel_bits > 8; }
static size_t image_bytes(const sgm_instance* s) { return batch_px(s) * (wide_pixels(s) ? 2 : 1); }

/* wait for everything the instance has queued (its stream and, with sgm_set_overlap_post, the post-pass stream) */
static int sync_streams(sgm_instance* s)
{
    int rc = sgmd_stream_sync(s->device, s->stream);
    if (s->sum_stream && sgmd_stream_sync(s->device, s->sum_stream) != 0) rc = -1;
    if (s->post_stream && sgmd_stream_sync(s->device, s->post_stream) != 0) rc = -1;
    if (rc == 0) { s->post_pending = s->sum_pending = false; s->tail_stream = NULL; }
    if (rc == 0 && s->h_status && *s->h_status) {
        *s->h_status = 0;
        fprintf(stderr, "sgm_mi355x: the median of a tall frame gave up waiting for the band above; the result is not valid\n");
        rc = -1;
    }
    return rc;
}

/* ------------------------------------------------------------------ path geometry (host) */

/* The reference's pointer walk (SemiGlobalMatching.c:243-255, 281-323, 359-367)
 * for one line.  Writes visited linear pixel indices, returns their count; a step that leaves
 * the image ends the line (the reference's undefined behaviour, defined away: SURVEY.md Q6). */
static int walk_line(int W, int H, int dx, int dy, int line, int32_t* pix)
{
    const int fwd = (dx == 1 && dy == 0) || (dx == 0 && dy == 1) || (dx == 1 && dy == 1) || (dx == -1 && dy == 1);
    const int s = fwd ? 1 : -1;
    const long long npx = (long long)W * H;
    long long p = (dy == 0) ? (long long)line * W + (fwd ? 0 : W - 1) : (fwd ? 0 : (long long)(H - 1) * W) + line;
    const int steps = (dy == 0 ? W : H) - 1;
    unsigned row = (unsigned)(fwd ? 0 : H - 1) & 0xFFFFu, col = (unsigned)line & 0xFFFFu;
    int n = 0;
    pix[n++] = (int32_t)p;
    for (int j = 0; j < steps; ++j) {
        if (dy == 0) p += s;
        else if (dx == 0) p += (long long)s * W;
        else {
            const int not_last = fwd ? ((int)row < H - 1) : (row > 0);
            if ((int)col == W - 1 && not_last) { p = ((long long)row + s) * W; col = 0; }
            else if (col == 0 && not_last) { p = ((long long)row + s) * W + (W - 1); col = (unsigned)(W - 1); }
            else p += (long long)s * (W + (dx == dy ? 1 : -1));
        }
        if (p < 0 || p >= npx) break;
        pix[n++] = (int32_t)p;
        row = (row + (unsigned)s) & 0xFFFFu;
        col = (col + (unsigned)((dx == dy || dx == 0 || dy == 0) ? s : -s)) & 0xFFFFu;
    }
    return n;
}

/* exported for the host-logic tests (not part of the public header) */
int sgm_host_walk_line(int W, int H, int dx, int dy, int line, int32_t* pix) { return walk_line(W, H, dx, dy, line, pix); }

/* The line of a diagonal direction whose very first step trips the wrong edge test
 * (SemiGlobalMatching.c:297,304 do not look at dx): it starts in column 0 while
 * moving right, or in column W-1 while moving left. */
static int anomalous_line(int W, int dx) { return dx > 0 ? 0 : W - 1; }
int sgm_host_anomalous_line(int W, int dx) { return anomalous_line(W, dx); }

/* (uint16) max(P1, P2 / (a + 1)), a = |grey difference| (SemiGlobalMatching.c:335) */
static void build_p2_table(int p1, int p2_init, uint16_t* lut)
{
    for (int a = 0; a < 256; ++a) {
        int pen = p2_init / (a + 1);
        if (p1 > pen) pen = p1;
        lut[a] = (uint16_t)pen;
    }
}
void sgm_host_p2_table(int p1, int p2_init, uint16_t* lut) { build_p2_table(p1, p2_init, lut); }

static int pick_dpl(int D)
{
    if (D <= 32) return 2;
    if (D <= 64) return 4;
    if (D <= 128) return 8;
    if (D <= 192) return 12;
    if (D <= 256) return 16;
    return 32;
}

/* ------------------------------------------------------------------ instance management */

static bool device_usable(int device)
{
    const int n = sgmd_device_count();
    if (n <= 0) FAIL("no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) FAIL("device %d out of range (%d visible)", device, n);
    if (sgmd_device_is_gfx950(device) != 1) FAIL("device %d is not gfx950 (MI355X); kernels are built for gfx950 only", device);
    return true;
}

static int env_int(const char* name)
{
    const char* e = getenv(name);
    return (e && *e) ? atoi(e) : -1;
}

sgm_instance* sgm_create(int device)
{
    if (!device_usable(device)) return NULL;
    sgm_instance* s = (sgm_instance*)calloc(1, sizeof *s);
    if (!s) return NULL;
    s->device = device;
    s->batch = 1;
    if (sgmd_stream_create(device, &s->stream) != 0) { free(s); return NULL; }
    void* st = NULL;
    if (sgmd_alloc_pinned(device, &st, 64) != 0) { sgmd_stream_destroy(device, s->stream); free(s); return NULL; }
    s->h_status = (int*)st;
    *s->h_status = 0;
    s->env_lanes = env_int("SGM_LANES_PER_PIXEL");
    s->env_hl = env_int("SGM_HL");
    s->env_agg_fast = env_int("SGM_AGG_FAST");
    s->env_fused = env_int("SGM_FUSED_WTA");
    s->env_upsum = env_int("SGM_UPSUM");
    s->env_upsum_rows = env_int("SGM_UPSUM_ROWS");
    s->env_upsum_wgs = env_int("SGM_UPSUM_WGS");
    return s;
}

/* ------------------------------------------------------------------ the instance's buffers */

enum {
    BUF_PINNED = 1,          /* page-locked host memory (a device buffer otherwise) */
    BUF_ZERO = 2,            /* zero-filled on s->stream when (re-)allocated */
    BUF_LAZY_DRAIN = 4       /* no drain in front of a first allocation, where there is nothing to free (every other buffer drains
                                there too, as its hand-written block always did) */
};
typedef struct { sgm_buf* buf; size_t bytes; int flags; } buf_request;

static bool buf_holds(const sgm_buf* b, size_t bytes) { return b->p && bytes <= b->cap; }

static void buf_release(sgm_instance* s, sgm_buf* b, bool pinned)
{
    if (pinned) sgmd_free_pinned(s->device, b->p);
    else sgmd_free(s->device, b->p);
    b->p = NULL;
    b->cap = 0;
}

/* The grow-only idiom, for n buffers that are sized together: nothing to do when all of them exist and are large enough.  Otherwise
 * the instance's streams are drained once (queued work may use what is freed here) and each buffer that is missing or too small
 * is freed and allocated anew; its capacity is recorded only once it is usable, a failure leaves it {NULL, 0} and ends the call. */
static bool reserve_all(sgm_instance* s, const buf_request* req, int n, int flags)
{
    bool grow = false, drain = false;
    for (int i = 0; i < n; ++i)
        if (!buf_holds(req[i].buf, req[i].bytes)) {
            grow = true;
            if (req[i].buf->p || !((req[i].flags | flags) & BUF_LAZY_DRAIN)) drain = true;
        }
    if (!grow) return true;
    if (drain) sync_streams(s);
    for (int i = 0; i < n; ++i) {
        sgm_buf* b = req[i].buf;
        const int f = req[i].flags | flags;
        if (buf_holds(b, req[i].bytes)) continue;
        buf_release(s, b, f & BUF_PINNED);
        const int rc = (f & BUF_PINNED) ? sgmd_alloc_pinned(s->device, &b->p, req[i].bytes) : sgmd_alloc(s->device, &b->p, req[i].bytes);
        if (rc != 0) { b->p = NULL; return false; }
        if ((f & BUF_ZERO) && sgmd_memset_async(s->device, s->stream, b->p, 0, req[i].bytes) != 0) {
            buf_release(s, b, f & BUF_PINNED);
            return false;
        }
        b->cap = req[i].bytes;
    }
    return true;
}

static bool reserve(sgm_instance* s, sgm_buf* b, size_t bytes, int flags)
{
    const buf_request one = {b, bytes, flags};
    return reserve_all(s, &one, 1, 0);
}

static void free_device_buffers(sgm_instance* s)
{
    s->d_census_r = NULL;                                        /* points into d_census_r_alloc */
    s->d_planes = NULL;                                          /* points into (or in front of) d_planes_alloc */
    for (size_t i = 0; i < sizeof k_buffers / sizeof k_buffers[0]; ++i)
        buf_release(s, (sgm_buf*)((char*)s + k_buffers[i].offset), k_buffers[i].pinned);
    s->need_key[0] = 0;
    s->up_key[0] = 0;
    s->tab_W = s->tab_H = 0;
    s->rect_dirty = true;
    s->tp_sig[0] = 0;                                            /* the history went with its buffers */
    s->tp_stat_maps = 0;
}

void sgm_destroy(sgm_instance* s)
{
    if (!s) return;
    sgm_match_wait(s);
    sync_streams(s);
    free_device_buffers(s);
    sgmd_timer_destroy(s->device, s->timer);
    sgmd_event_destroy(s->device, s->ev_agg);
    sgmd_event_destroy(s->device, s->ev_sum);
    sgmd_event_destroy(s->device, s->ev_post);
    for (int i = 0; i < 4; ++i)
        if (s->ev_chunk[i]) sgmd_event_destroy(s->device, s->ev_chunk[i]);
    if (s->sum_stream) sgmd_stream_destroy(s->device, s->sum_stream);
    if (s->post_stream) sgmd_stream_destroy(s->device, s->post_stream);
    sgmd_stream_destroy(s->device, s->stream);
    sgmd_free_pinned(s->device, s->h_status);
    free(s->rect_q);
    free(s);
}

void sgm_set_honor_num_paths(sgm_instance* s, int honor) { if (s) s->honor_num_paths = honor; }

/* the three ordering events exist as soon as any stage has a stream of its own; all or none */
static bool ensure_stage_events(sgm_instance* s)
{
    void** ev[3] = {&s->ev_agg, &s->ev_sum, &s->ev_post};
    for (int i = 0; i < 3; ++i)
        if (!*ev[i] && sgmd_event_create(s->device, ev[i]) != 0) { *ev[i] = NULL; return false; }
    return true;
}

/* Stage groups on streams of their own, optionally on their own compute units (include/sgm_mi355x.h).  The instance is idle
 * while its streams change. */
bool sgm_set_stage_cus(sgm_instance* s, int which, int first_per_xcd, int count_per_xcd)
{
    if (!s || which < SGM_STAGE_MAIN || which > SGM_STAGE_POST) return false;
    if (!sgm_match_wait(s) || sync_streams(s) != 0) return false;
    void** slot = which == SGM_STAGE_MAIN ? &s->stream : (which == SGM_STAGE_SUM ? &s->sum_stream : &s->post_stream);
    if (count_per_xcd < 0) {                                     /* back to the default */
        if (which == SGM_STAGE_MAIN) return sgm_set_stage_cus(s, which, 0, 0);
        if (*slot) sgmd_stream_destroy(s->device, *slot);
        *slot = NULL;
        if (which == SGM_STAGE_POST) s->overlap_post = 0;
        s->cu_first[which] = s->cu_count[which] = 0;
        s->stage_prio[which] = false;
        return true;
    }
    if (*slot && !s->stage_prio[which] && s->cu_first[which] == first_per_xcd && s->cu_count[which] == count_per_xcd) {
        if (which == SGM_STAGE_POST) s->overlap_post = 1;
        return true;
    }
    void* fresh = NULL;
    if (!ensure_stage_events(s) || sgmd_stream_create_cus(s->device, &fresh, first_per_xcd, count_per_xcd) != 0) return false;
    if (*slot) sgmd_stream_destroy(s->device, *slot);
    *slot = fresh;
    s->cu_first[which] = first_per_xcd;
    s->cu_count[which] = count_per_xcd;
    s->stage_prio[which] = false;
    if (which == SGM_STAGE_POST) s->overlap_post = 1;
    return true;
}

/* the group's own stream, on all CUs, with a dispatch priority (include/sgm_mi355x.h) */
bool sgm_set_stage_priority(sgm_instance* s, int which, int priority)
{
    if (!s || which < SGM_STAGE_MAIN || which > SGM_STAGE_POST) return false;
    if (!sgm_match_wait(s) || sync_streams(s) != 0) return false;
    void** slot = which == SGM_STAGE_MAIN ? &s->stream : (which == SGM_STAGE_SUM ? &s->sum_stream : &s->post_stream);
    void* fresh = NULL;
    if (!ensure_stage_events(s) || sgmd_stream_create_prio(s->device, &fresh, priority) != 0) return false;
    if (*slot) sgmd_stream_destroy(s->device, *slot);
    *slot = fresh;
    s->cu_first[which] = s->cu_count[which] = 0;
    s->stage_prio[which] = true;
    if (which == SGM_STAGE_POST) s->overlap_post = 1;
    return true;
}

bool sgm_set_overlap_post(sgm_instance* s, int enable)
{
    if (!s) return false;
    if (enable) return s->post_stream ? (s->overlap_post = 1, true) : sgm_set_stage_cus(s, SGM_STAGE_POST, 0, 0);
    if (s->overlap_post) sync_streams(s);                        /* the next match is ordered on sgm_stream alone again */
    s->overlap_post = 0;
    return true;
}

bool sgm_set_census_window(sgm_instance* s, int width, int height)
{
    if (!s || width < 1 || height < 1 || !(width & 1) || !(height & 1) || width * height > 64) return false;
    if (width == 5 && height == 5) width = height = 0;           /* the reference's window: the fused fast path */
    if (width != s->census_w || height != s->census_h) s->initialized = false;   /* takes effect at the next initialize */
    s->census_w = width; s->census_h = height;
    return true;
}

/* The symmetric census launcher (sgm_census.hip), weakly referenced like the extensions below: a host built without it (the
 * stand-in device of the tests) refuses that kind. */
#pragma weak sgmd_census_sym
static bool census_kind_ok(int kind)
{
    if (kind != SGM_CENSUS_CENTRE && kind != SGM_CENSUS_SYMMETRIC) return false;
    if (kind == SGM_CENSUS_SYMMETRIC && sgmd_census_sym == NULL) FAIL("the symmetric census is not part of this build");
    return true;
}

bool sgm_set_census_kind(sgm_instance* s, int kind)
{
    if (!s || !census_kind_ok(kind)) return false;
    if (kind != s->census_kind) s->initialized = false;          /* takes effect at the next initialize */
    s->census_kind = kind;
    return true;
}

void sgm_set_reference_view(sgm_instance* s, int right) { if (s) s->reference_view = right ? 1 : 0; }

/* The launchers for images of more than 8 bits per sample (sgm_pixels16.hip), weakly referenced like the other extensions: a host
 * built without them (the stand-in device of the tests) keeps to 8 bits. */
#pragma weak sgmd_census16
#pragma weak sgmd_remap16
static bool pixel_bits_ok(int bits)
{
    if (bits < 8 || bits > 16) return false;
    if (bits > 8 && (sgmd_census16 == NULL || sgmd_remap16 == NULL)) FAIL("images of more than 8 bits are not part of this build");
    return true;
}

bool sgm_set_pixel_bits(sgm_instance* s, int bits)
{
    if (!s || !pixel_bits_ok(bits)) return false;
    if (bits != (s->pixel_bits_req ? s->pixel_bits_req : 8)) s->initialized = false;   /* takes effect at the next initialize */
    s->pixel_bits_req = bits;
    return true;
}

/* device images of more than 8 bits are read two bytes at a time */
static bool images_aligned(const sgm_instance* s, const void* a, const void* b)
{
    if (wide_pixels(s) && (((uintptr_t)a | (uintptr_t)b) & 1u)) FAIL("device images of %d bits per sample must be 2-byte aligned", s->pixel_bits);
    return true;
}

/* The hole-filling launchers live in sgm_fill.hip; the host is also built without any HIP (tests link it against a stand-in
 * device), where they are absent: weak references, and no filling there. */
#pragma weak sgmd_fill_classify
#pragma weak sgmd_fill_pass
static bool fill_available(void) { return sgmd_fill_classify != NULL && sgmd_fill_pass != NULL; }

bool sgm_set_fill_holes(sgm_instance* s, int enable)
{
    if (!s) return false;
    if (enable && !fill_available()) FAIL("hole filling is not part of this build");
    s->fill_req = enable ? 1 : 0;                                /* takes effect at the next initialize */
    return true;
}
void sgm_keep_stages(sgm_instance* s, int enable) { if (s) s->keep_stages = enable; }

/* The confidence launchers (sgm_sum_wta.hip): weak references as for the hole filling -- a host built without them (the
 * stand-in device of the tests) answers false to the confidence entry points. */
#pragma weak sgmd_sum_wta_conf
#pragma weak sgmd_sum_wta_lr_conf
#pragma weak sgmd_wta_right_conf
static bool conf_available(void) { return sgmd_sum_wta_conf != NULL && sgmd_sum_wta_lr_conf != NULL && sgmd_wta_right_conf != NULL; }

/* The refinement launcher (sgm_refine.hip), weakly referenced as well; a match with refinement needs the confidence kernels too */
#pragma weak sgmd_refine_pass
static bool refine_available(void) { return sgmd_refine_pass != NULL && conf_available(); }

/* The dual LR check (sgm_sum_wta.hip) behind sgm_match_both and the depth from both maps (sgm_post.hip), weakly referenced as
 * well: a host built without them answers false to those entry points. */
#pragma weak sgmd_lrcheck_both
#pragma weak sgmd_depth_both
static bool both_available(void) { return sgmd_lrcheck_both != NULL; }

bool sgm_refine_table(float lambda, float sigma, int iterations, int t, float* out)
{
    if (!out || !isfinite(lambda) || !isfinite(sigma) || lambda <= 0 || sigma <= 0 || iterations < 1 ||
        iterations > SGM_REFINE_MAX_ITERS || t < 0 || t >= iterations)
        return false;
    const double lam = (double)lambda * 1.5 * ldexp(1.0, 2 * (iterations - 1 - t)) / (ldexp(1.0, 2 * iterations) - 1.0);
    for (int k = 0; k < 256; ++k) out[k] = (float)(lam * exp(-(double)k / (double)sigma));
    return true;
}

static bool refine_params_set(refine_params* p, float lambda, float sigma, int iterations, int keep_invalid)
{
    if (keep_invalid != 0 && keep_invalid != 1) return false;
    for (int t = 0; t < iterations; ++t)
        if (!sgm_refine_table(lambda, sigma, iterations, t, p->tab[t])) return false;
    if (iterations < 1) return false;
    p->lambda = lambda;
    p->sigma = sigma;
    p->iters = iterations;
    p->keep_invalid = keep_invalid;
    return true;
}

bool sgm_set_refine(sgm_instance* s, int enable, float lambda, float sigma, int iterations, int keep_invalid)
{
    if (!s || (enable != 0 && enable != 1)) return false;
    if (!enable) {
        s->refine_req = 0;                                       /* takes effect at the next initialize */
        return true;
    }
    if (!refine_available()) FAIL("the refinement is not part of this build");
    refine_params p;
    if (!refine_params_set(&p, lambda, sigma, iterations, keep_invalid)) return false;
    s->rf_req = p;
    s->refine_req = 1;
    return true;
}

/* ------------------------------------------------------------------ temporal filter (extension) */

/* The launchers of sgm_temporal.hip, weakly referenced like the extensions above: a host built without them has no temporal filter */
#pragma weak sgmd_temporal
#pragma weak sgmd_temporal_clear
#pragma weak sgmd_temporal_scratch_bytes
static bool temporal_available(void) { return sgmd_temporal != NULL && sgmd_temporal_clear != NULL && sgmd_temporal_scratch_bytes != NULL; }

/* the spec as the kernel takes it; false for anything outside the ranges of include/sgm_mi355x.h.  flags: sequence and stats are
 * checked too (sgm_set_temporal; sgm_temporal_filter does not look at them) */
static bool temporal_spec_valid(const sgm_temporal_spec* sp, bool flags, sgmd_temporal_params* c)
{
    if (!isfinite(sp->alpha) || !(sp->alpha > 0.0f) || !(sp->alpha <= 1.0f) || !isfinite(sp->delta) || !(sp->delta >= 0.0f)) return false;
    if (sp->hold_window < 0 || sp->hold_window > 8 || sp->min_conf > 65535u) return false;
    if (sp->hold_window > 0 && (sp->hold_count < 1 || sp->hold_count > sp->hold_window)) return false;
    if (flags && ((sp->sequence != 0 && sp->sequence != 1) || (sp->stats != 0 && sp->stats != 1))) return false;
    const float b = 1.0f - sp->alpha;
    if (c) *c = (sgmd_temporal_params){sp->alpha, b, sp->delta, sp->hold_window, sp->hold_window > 0 ? sp->hold_count : 0, sp->min_conf};
    return true;
}

/* what sgm_set_temporal / SGM_SetTemporal check */
static bool temporal_spec_ok(const sgm_temporal_spec* spec)
{
    if (!temporal_available()) FAIL("the temporal filter is not part of this build");
    if (!temporal_spec_valid(spec, true, NULL)) FAIL("the temporal spec is outside its ranges (include/sgm_mi355x.h, sgm_temporal_spec)");
    if (spec->min_conf > 0 && !conf_available()) FAIL("a temporal filter with min_conf > 0 needs the confidence kernels, which are not part of this build");
    return true;
}

bool sgm_set_temporal(sgm_instance* s, const sgm_temporal_spec* spec)
{
    if (!s) return false;
    if (!spec) {
        s->temporal_req = false;                                 /* takes effect at the next initialize */
        return true;
    }
    if (!temporal_spec_ok(spec)) return false;
    s->tp_req = *spec;
    s->temporal_req = true;
    s->tp_restart = true;                                        /* every spec set starts a new history */
    return true;
}

bool sgm_temporal_restart(sgm_instance* s)
{
    if (!s) return false;
    s->tp_restart = true;
    return true;
}

/* what the standalone entry points check of their geometry */
static bool temporal_geometry_ok(size_t streams, size_t steps, size_t pixels)
{
    const size_t lim = (size_t)1 << 31;
    return streams >= 1 && steps >= 1 && pixels >= 1 && streams <= lim && steps <= lim && pixels <= lim && streams * steps <= lim &&
           streams * steps * pixels <= lim;
}

/* ------------------------------------------------------------------ rectification (extension) */

/* The remap launcher (sgm_rectify.hip), weakly referenced like the extensions above: a host built without it has no rectification */
#pragma weak sgmd_remap
static bool rectify_available(void) { return sgmd_remap != NULL; }

bool sgm_rectify_maps(const double K[9], const double dist[5], const double R[9], const double Knew[9], int width, int height,
                      float* map_x, float* map_y)
{
    if (!K || !dist || !R || !Knew || !map_x || !map_y || width < 1 || height < 1) return false;
    double m[9], iR[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[3 * i + j] = Knew[3 * i] * R[j] + Knew[3 * i + 1] * R[3 + j] + Knew[3 * i + 2] * R[6 + j];
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    if (!isfinite(det) || det == 0.0) return false;
    iR[0] = c0 / det; iR[1] = (m[2] * m[7] - m[1] * m[8]) / det; iR[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    iR[3] = c1 / det; iR[4] = (m[0] * m[8] - m[2] * m[6]) / det; iR[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    iR[6] = c2 / det; iR[7] = (m[1] * m[6] - m[0] * m[7]) / det; iR[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    for (int v = 0; v < height; ++v)
        for (int u = 0; u < width; ++u) {
            const double X = iR[0] * u + iR[1] * v + iR[2], Y = iR[3] * u + iR[4] * v + iR[5], Wz = iR[6] * u + iR[7] * v + iR[8];
            const double x = X / Wz, y = Y / Wz, r2 = x * x + y * y;
            const double rad = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
            const double xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
            const double yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
            map_x[(size_t)v * width + u] = (float)(fx * xd + cx);
            map_y[(size_t)v * width + u] = (float)(fy * yd + cy);
        }
    return true;
}

/* The quantisation of one map entry (include/sgm_mi355x.h): both coordinates become -64, all four taps outside, when either is not
 * finite or has |m| > 32768 (!(<=) also catches NaN) */
static void rectify_quantise_entry(double x, double y, int32_t* xq, int32_t* yq)
{
    const bool ok = fabs(x) <= 32768.0 && fabs(y) <= 32768.0;
    *xq = ok ? (int32_t)floor(x * 32.0 + 0.5) : -64;
    *yq = ok ? (int32_t)floor(y * 32.0 + 0.5) : -64;
}

bool sgm_rectify_valid_mask(int width, int height, const float* map_x, const float* map_y, uint8_t* mask)
{
    if (!map_x || !map_y || !mask || width < 1 || height < 1 || (long long)width * height > 0x7FFFFFFFLL) return false;
    const size_t n = (size_t)width * height;
    for (size_t p = 0; p < n; ++p) {
        int32_t xq, yq;
        rectify_quantise_entry((double)map_x[p], (double)map_y[p], &xq, &yq);
        const int32_t x0 = xq >> 5, y0 = yq >> 5;                 /* the taps are (y0, x0) .. (y0 + 1, x0 + 1) */
        mask[p] = x0 >= 0 && x0 < width - 1 && y0 >= 0 && y0 < height - 1;
    }
    return true;
}

/* The quantised maps of both views in the layout sgmd_remap reads (sgm_device.h), malloc'ed; NULL: bad arguments or out of memory */
static int32_t* rectify_quantise(int width, int height, const float* map_lx, const float* map_ly, const float* map_rx, const float* map_ry)
{
    if (!map_lx || !map_ly || !map_rx || !map_ry || width < 1 || height < 1 || (long long)width * height > 0x7FFFFFFFLL) return NULL;
    const size_t n = (size_t)width * height, pitch = SGMD_REMAP_PITCH(n);
    int32_t* q = (int32_t*)malloc(4 * pitch * sizeof *q);
    if (!q) return NULL;
    const float* const mx[2] = {map_lx, map_rx};
    const float* const my[2] = {map_ly, map_ry};
    for (int view = 0; view < 2; ++view) {
        int32_t* xq = q + (size_t)view * 2 * pitch;
        int32_t* yq = xq + pitch;
        for (size_t p = 0; p < pitch; ++p) {
            const double x = p < n ? (double)mx[view][p] : NAN, y = p < n ? (double)my[view][p] : NAN;
            rectify_quantise_entry(x, y, &xq[p], &yq[p]);
        }
    }
    return q;
}

/* the instance takes q (NULL: rectification off) */
static void rectify_install(sgm_instance* s, int32_t* q, int width, int height)
{
    free(s->rect_q);
    s->rect_q = q;
    s->rect_w = q ? width : 0;
    s->rect_h = q ? height : 0;
    s->rect_dirty = true;                                        /* takes effect at the next initialize */
}

bool sgm_set_rectify(sgm_instance* s, int width, int height, const float* map_lx, const float* map_ly, const float* map_rx,
                     const float* map_ry)
{
    if (!s) return false;
    if (!map_lx) { rectify_install(s, NULL, 0, 0); return true; }
    if (!rectify_available()) FAIL("the rectification is not part of this build");
    int32_t* q = rectify_quantise(width, height, map_lx, map_ly, map_rx, map_ry);
    if (!q) return false;
    rectify_install(s, q, width, height);
    return true;
}

/* the maps on the device and the two rectified images, beside upload_tables: a Reset with unchanged maps uploads nothing */
static bool upload_rectify(sgm_instance* s)
{
    const size_t px = image_bytes(s);
    const size_t bytes = 4 * SGMD_REMAP_PITCH((size_t)s->rect_w * s->rect_h) * sizeof(int32_t);
    const buf_request bufs[] = {{&s->d_rect_maps, bytes, 0}, {&s->d_rect_l, px, 0}, {&s->d_rect_r, px, 0}};
    if (!reserve_all(s, bufs, 3, 0)) FAIL("device allocation failed for the rectification of %dx%d", s->g.W, s->g.H);
    if (!s->rect_dirty) return true;
    /* queued remaps read the maps on s->stream: the upload is behind them; the host copy may be replaced once this returns */
    if (sgmd_h2d_async(s->device, s->stream, s->d_rect_maps.p, s->rect_q, bytes) != 0 || sync_streams(s) != 0)
        FAIL("uploading the rectification maps failed");
    s->rect_dirty = false;
    return true;
}

bool sgm_rectify(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, uint8_t* d_out_left, uint8_t* d_out_right)
{
    if (!s || !s->initialized || !d_left || !d_right || !d_out_left || !d_out_right) return false;
    if (!s->rect_on) FAIL("sgm_rectify: no rectification maps are in effect (sgm_set_rectify, then sgm_initialize / sgm_reset)");
    if (!images_aligned(s, d_left, d_right) || !images_aligned(s, d_out_left, d_out_right)) return false;
    if ((wide_pixels(s) ? sgmd_remap16 : sgmd_remap)(s->device, s->stream, &s->g, s->d_rect_maps.p, d_left, d_right, d_out_left, d_out_right) != 0)
        FAIL("a kernel launch failed");
    return true;
}

bool sgm_set_batch(sgm_instance* s, int frames)
{
    if (!s || frames < 1 || frames > 1024) return false;
    if (frames != s->batch) s->initialized = false;              /* buffers are sized at the next initialize */
    s->batch = frames;
    return true;
}

void sgm_select_frame(sgm_instance* s, int frame)
{
    if (s && frame >= 0 && frame < s->batch) s->read_frame = frame;
}
void* sgm_stream(sgm_instance* s) { return s ? s->stream : NULL; }
int sgm_fused_sweep_rows(const sgm_instance* s) { return s ? s->last_up_rows : 0; }

void sgm_enable_timing(sgm_instance* s, int enable)
{
    if (!s) return;
    if (enable && !s->timer && sgmd_timer_create(s->device, &s->timer, TIMING_RING * MARKS_PER_MATCH) != 0) return;
    s->timing = enable;
    /* (re-)enabling starts a new statistics window: drop what was recorded before */
    sync_streams(s);
    s->ring_next = s->ring_pending = 0;
    s->n_timed = 0;
    for (int i = 0; i < T_COUNT; ++i) { s->sum_ms[i] = 0; s->min_ms[i] = 1e30; }
}

int sgm_mean_timing(sgm_instance* s, const char** names, float* mean_ms, float* min_ms, int max_entries, long* matches)
{
    if (matches) *matches = s ? s->n_timed : 0;
    if (!s || s->n_timed == 0) return 0;
    int n = 0;
    for (int i = 0; i < T_COUNT && n < max_entries; ++i, ++n) {
        if (names) names[n] = k_stage_names[i];
        if (mean_ms) mean_ms[n] = (float)(s->sum_ms[i] / (double)s->n_timed);
        if (min_ms) min_ms[n] = (float)s->min_ms[i];
    }
    return n;
}

int sgm_last_timing(sgm_instance* s, const char** names, float* ms, int max_entries)
{
    if (!s || !s->have_ms) return 0;
    int n = 0;
    for (int i = 0; i < T_COUNT && n < max_entries; ++i, ++n) {
        if (names) names[n] = k_stage_names[i];
        if (ms) ms[n] = s->last_ms[i];
    }
    return n;
}

/* Row tiles: the census words this instance reads are those of its own rows (horizontal lines, the sweeps, the cost sum's
 * recomputation) and, on every row of the frame, the pixel an anomalous line visits with the Dp words to its left.  Everything
 * else of the replicated images is skipped: sgmd_census takes one byte per 64 x 16 block.  (The aggregation's masked and
 * prefetched reads beyond that see whatever the buffer holds, as they always did at row starts.) */
static bool upload_census_need(sgm_instance* s)
{
    const int W = s->g.W, H = s->g.H;
    const int key[7] = {W, H, s->g.row_begin, s->g.row_end, s->g.dmin, s->g.Dp, s->paths.ndirs};
    if (s->d_census_need.p && memcmp(key, s->need_key, sizeof key) == 0) return true;
    int bx, by;
    sgmd_census_blocks(&s->g, &bx, &by);
    const size_t n = (size_t)bx * by;
    uint8_t* need = (uint8_t*)calloc(n, 1);
    int32_t* pix = (int32_t*)malloc(sizeof(int32_t) * (size_t)(W > H ? W : H));
    if (!need || !pix) { free(need); free(pix); FAIL("out of host memory"); }
    const int bw = 64, bh = 16;                               /* sgmd_census_blocks */
    for (int r = s->g.row_begin / bh; r <= (s->g.row_end - 1) / bh; ++r) memset(need + (size_t)r * bx, 1, (size_t)bx);
    if (s->paths.ndirs > 4) {
        const int back = s->g.dmin + s->g.Dp + 64;            /* words left of the pixel: range + the widest vector load */
        for (int d = 4; d < 8; ++d) {
            const int cnt = walk_line(W, H, k_dir_dx[d], k_dir_dy[d], s->paths.anom_line[d], pix);
            for (int k = 0; k < cnt; ++k) {
                const int y = pix[k] / W, x = pix[k] % W;
                const int c0 = (x - back < 0 ? 0 : x - back) / bw, c1 = x / bw;
                memset(need + (size_t)(y / bh) * bx + c0, 1, (size_t)(c1 - c0 + 1));
                /* a window that starts left of column 0 continues at the end of the row above (masked, but keep it defined) */
                if (x - back < 0 && y > 0) need[(size_t)((y - 1) / bh) * bx + bx - 1] = 1;
            }
        }
    }
    free(pix);
    const bool ok = reserve(s, &s->d_census_need, n, 0) && sgmd_h2d_async(s->device, s->stream, s->d_census_need.p, need, n) == 0 && sync_streams(s) == 0;
    free(need);
    if (!ok) FAIL("uploading the census block map failed");
    memcpy(s->need_key, key, sizeof key);
    return true;
}

/* most entries of the per-row table [H][cap] (8 bytes each: 128 MB) */
#define ROW_EXTRAS_MAX ((size_t)1 << 24)

/* Build the per-row table of anomalous-line visits and upload it together with the P2 table. */
static bool upload_tables(sgm_instance* s)
{
    const int W = s->g.W, H = s->g.H;
    uint16_t lut[256];
    build_p2_table(s->opt.p1, s->opt.p2_init, lut);

    int32_t* pix = (int32_t*)malloc(sizeof(int32_t) * (size_t)(W > H ? W : H));
    int* count = (int*)calloc((size_t)H, sizeof(int));
    int32_t* visits = (int32_t*)malloc(sizeof(int32_t) * 4 * (size_t)H);      /* [slot][k] pixel or -1 */
    if (!pix || !count || !visits) { free(pix); free(count); free(visits); FAIL("out of host memory"); }
    for (int i = 0; i < 4 * H; ++i) visits[i] = -1;
    if (s->paths.ndirs > 4) {
        for (int slot = 0; slot < 4; ++slot) {
            const int d = 4 + slot;
            const int n = walk_line(W, H, k_dir_dx[d], k_dir_dy[d], s->paths.anom_line[d], pix);
            for (int k = 0; k < n; ++k) {
                visits[slot * H + k] = pix[k];
                count[pix[k] / W]++;
            }
        }
    }
    int cap = 1;
    for (int r = 0; r < H; ++r) if (count[r] > cap) cap = count[r];
    /* W = 1: for the two directions with dx != dy a diagonal step is W - 1 = 0 pixels and the tracker never finds column 0 again:
     * after its first step the (-1,+1) line stays on row 1 and the (+1,-1) line on row H - 2, H - 1 visits each.  The other two
     * lines move two rows per step, (1,1) over rows 0, 1, 3, 5, ..., (-1,-1) over H - 1, H - 2, H - 4, ...; both meet row 1 where H
     * is odd.  So cap = H for even H and H + 1 for odd H: a table of about H^2 entries (34 GB at H = 65535) that the kernels index
     * with row * cap in int.  The limit admits H * cap <= 2^24: 1 x 4096 (4096 * 4096, exactly the limit) is the tallest such
     * frame, 1 x 4097 (4097 * 4098) is refused.  No other width has more than 6 visits in a row. */
    if ((size_t)H * cap > ROW_EXTRAS_MAX) {
        free(pix); free(count); free(visits);
        FAIL("a frame %d wide and %d rows tall is not supported: its anomalous lines visit one row %d times (a frame one pixel wide "
             "is accepted up to 4096 rows)", W, H, cap);
    }
    sgmd_row_extra* table = (sgmd_row_extra*)calloc((size_t)H * cap, sizeof *table);
    if (!table) { free(pix); free(count); free(visits); FAIL("out of host memory"); }
    memset(count, 0, sizeof(int) * (size_t)H);
    for (int slot = 0; slot < 4; ++slot)
        for (int k = 0; k < H; ++k) {
            const int32_t p = visits[slot * H + k];
            if (p < 0) continue;
            const int r = p / W, c = p % W;
            table[(size_t)r * cap + count[r]].col_slot = c | (slot << 16);
            table[(size_t)r * cap + count[r]].step = k;
            count[r]++;
        }

    /* tables that are replaced may still be read by queued work; the first ones are not */
    const buf_request tables[] = {{&s->d_row_extras, sizeof *table * (size_t)H * cap, 0}, {&s->d_row_count, sizeof(int) * (size_t)H, 0}};
    s->row_cap = cap;
    /* plain blocking-safe uploads: the tables live on the host stack/heap only until the sync below */
    const bool ok = reserve_all(s, tables, 2, BUF_LAZY_DRAIN) && sgmd_h2d_async(s->device, s->stream, s->d_row_extras.p, table, sizeof *table * (size_t)H * cap) == 0 &&
         sgmd_h2d_async(s->device, s->stream, s->d_row_count.p, count, sizeof(int) * (size_t)H) == 0 &&
         sgmd_h2d_async(s->device, s->stream, s->d_lut.p, lut, sizeof lut) == 0 &&
         sync_streams(s) == 0;
    free(table); free(visits); free(count); free(pix);
    if (!ok) FAIL("uploading path tables failed");
    return true;
}

/* Per-pixel buffers (sized for the whole batch) and the per-direction planes.  A plane only has storage for the rows
 * the instance works on: every row of the frame normally; in row-tile mode the tile's rows plus the row either side that
 * a neighbouring GPU's hand-over lands in -- 1/N of the frame, which is what lets N + 2 frames be in flight per GPU. */
static bool ensure_buffers(sgm_instance* s)
{
    const int dev = s->device;
    const size_t px = batch_px(s);          /* all frames of the batch, frame-major */
    if (!buf_holds(&s->d_disp, px * 4)) {
        /* the per-pixel set grows: everything the instance owns goes (the buffers sized below and in sgm_initialize come back at
         * once, S, the cost volume and the others on their first use).
         * The aggregation kernel reads census-right up to dmin + Dp - 1 words left of a row start (masked to 127
         * afterwards); give the buffer that much readable slack in front, sized for the largest options */
        const size_t img = image_bytes(s);
        const buf_request images[] = {{&s->d_left, img, 0}, {&s->d_right, img, 0}, {&s->d_census_l, px * 4, 0},
                                      {&s->d_census_r_alloc, CENSUS_FRONT_SLACK + px * 4 + CENSUS_BACK_SLACK, 0}};
        const buf_request maps[] = {{&s->d_disp, px * 4, 0}, {&s->d_disp_r, px * 4, 0}, {&s->d_labels, px * 4, 0}, {&s->d_sizes, px * 4, 0},
                                    {&s->d_totals, px * 4, 0}, {&s->d_lut, 512, 0}, {&s->d_snap_wta, px * 4, 0}, {&s->d_snap_lr, px * 4, 0},
                                    {&s->d_snap_speckle, px * 4, 0}, {&s->h_left, img, BUF_PINNED}, {&s->h_right, img, BUF_PINNED},
                                    {&s->h_disp, px * 4, BUF_PINNED}};
        sync_streams(s);
        /* the census words of earlier frames outlive a re-allocation (reference_statics): set the old buffers aside */
        const sgm_buf old_l = s->d_census_l, old_r = s->d_census_r_alloc;
        s->d_census_l = s->d_census_r_alloc = (sgm_buf){NULL, 0};
        free_device_buffers(s);
        int rc = reserve_all(s, images, 4, BUF_LAZY_DRAIN) ? 0 : -1;
        if (rc == 0) s->d_census_r = (char*)s->d_census_r_alloc.p + CENSUS_FRONT_SLACK;
        /* zero like the reference's statics; then the words earlier frames left, at their linear indices */
        if (rc == 0) rc |= sgmd_memset_async(dev, s->stream, s->d_census_l.p, 0, px * 4);
        if (rc == 0) rc |= sgmd_memset_async(dev, s->stream, s->d_census_r_alloc.p, 0, CENSUS_FRONT_SLACK + px * 4);
        if (rc == 0 && s->reference_statics && old_l.p && old_r.p) {
            rc |= sgmd_d2d_async(dev, s->stream, s->d_census_l.p, old_l.p, old_l.cap);
            rc |= sgmd_d2d_async(dev, s->stream, s->d_census_r, (char*)old_r.p + CENSUS_FRONT_SLACK, old_l.cap);
        }
        if (rc == 0) rc |= sgmd_stream_sync(dev, s->stream);
        sgmd_free(dev, old_l.p);
        sgmd_free(dev, old_r.p);
        if (rc != 0 || !reserve_all(s, maps, 12, BUF_LAZY_DRAIN)) {
            free_device_buffers(s);
            FAIL("device allocation failed for %dx%dx%d", s->g.W, s->g.H, s->g.D);
        }
    }
    if (wide_pixels(s)) {
        /* the same frames with more bits per sample: the images (and their staging) grow to u16, the narrowed images appear */
        const size_t img = image_bytes(s);
        const buf_request wide[] = {{&s->d_left, img, 0}, {&s->d_right, img, 0}, {&s->h_left, img, BUF_PINNED}, {&s->h_right, img, BUF_PINNED},
                                    {&s->d_g8_l, px, 0}, {&s->d_g8_r, px, 0}};
        if (!reserve_all(s, wide, 6, 0)) FAIL("device allocation failed for the %d-bit images of %dx%d", s->pixel_bits, s->g.W, s->g.H);
    }
    const bool tiled = row_tiled(s);
    s->plane_row_lo = tiled && s->g.row_begin > 0 ? s->g.row_begin - 1 : 0;
    const int row_hi = tiled && s->g.row_end < s->g.H ? s->g.row_end + 1 : s->g.H;
    s->plane_rows = row_hi - s->plane_row_lo;
    s->plane_bytes = (size_t)s->plane_rows * s->g.W * s->g.Dp;
    const size_t need = (size_t)s->g.B * 8 * s->plane_bytes;
    if (!reserve(s, &s->d_planes_alloc, need, 0))
        FAIL("device allocation failed for the path-cost planes of %dx%dx%d (%zu bytes)", s->g.W, s->g.H, s->g.D, need);
    s->d_planes = (void*)((uintptr_t)s->d_planes_alloc.p - (uintptr_t)s->plane_row_lo * s->g.W * s->g.Dp);
    return true;
}

/* S (u16 per cell) and the cost volume (u8 per cell) are frame-sized and rarely needed: the fused kernels neither read
 * nor write them.  They are allocated (S zero-filled) the first time something does: a Match without Reset (Q14), the
 * separate sum / right-view kernels (D > 256, SGM_FUSED_WTA=0), sgm_keep_stages, a stage read-back. */
static int ensure_S(sgm_instance* s)
{
    const size_t need = batch_px(s) * s->g.Dp * 2;
    if (buf_holds(&s->d_S, need)) return 0;
    if (reserve(s, &s->d_S, need, BUF_ZERO) &&
        (!s->sum_stream || sgmd_stream_sync(s->device, s->stream) == 0))   /* the cost sum may run on another stream */
        return 0;
    fprintf(stderr, "sgm_mi355x: device allocation failed for the aggregated-cost volume (%zu bytes)\n", need);
    return -1;
}

static int ensure_cost(sgm_instance* s)
{
    const size_t need = batch_px(s) * s->g.Dp;
    if (reserve(s, &s->d_cost, need, 0)) return 0;
    fprintf(stderr, "sgm_mi355x: device allocation failed for the cost volume (%zu bytes)\n", need);
    return -1;
}

/* the class map and the ping-pong map of the hole filling, [B][H][W] each */
static int ensure_fill(sgm_instance* s)
{
    const size_t px = batch_px(s);
    const buf_request maps[] = {{&s->d_fill_class, px, 0}, {&s->d_fill_map, px * sizeof(float), 0}};
    if (reserve_all(s, maps, 2, 0)) return 0;
    fprintf(stderr, "sgm_mi355x: device allocation failed for the hole-filling maps (%zu pixels)\n", px);
    return -1;
}

/* the maps of the refinement, [B][H][W] each: U, V, Q (f32), the internal confidence (u16), two guide copies (u8) */
static int ensure_refine(sgm_instance* s)
{
    const size_t px = batch_px(s);
    const buf_request maps[] = {{&s->d_rf_u, px * 4, 0}, {&s->d_rf_v, px * 4, 0}, {&s->d_rf_q, px * 4, 0}, {&s->d_rf_conf, px * 2, 0},
                                {&s->d_rf_guide[0], px, 0}, {&s->d_rf_guide[1], px, 0}};
    if (reserve_all(s, maps, 6, 0)) return 0;
    fprintf(stderr, "sgm_mi355x: device allocation failed for the refinement maps (%zu pixels)\n", px);
    return -1;
}

/* streams per view of the filter in effect: the B frames of a batch, or (sequence) one */
static size_t temporal_streams(const sgm_instance* s) { return s->tp_eff.sequence ? 1 : (size_t)s->g.B; }

/* The history, the counters, the internal confidence (min_conf > 0) and, for sgm_keep_stages, the pre-filter maps, for `views` views.
 * A history that has to grow is a new one: its signature goes, the next filtered match clears it. */
static int ensure_temporal(sgm_instance* s, int views, bool keep)
{
    const size_t px = frame_px(s), hist = (size_t)views * temporal_streams(s) * px;
    if (!buf_holds(&s->d_tp_value, hist * sizeof(float)) || !buf_holds(&s->d_tp_bits, hist)) s->tp_sig[0] = 0;
    const buf_request bufs[] = {{&s->d_tp_value, hist * sizeof(float), 0}, {&s->d_tp_bits, hist, 0},
                                {&s->d_tp_stats, (size_t)views * s->g.B * 5 * sizeof(uint32_t), 0},
                                {&s->d_rf_conf, s->tp_eff.min_conf > 0 ? batch_px(s) * sizeof(uint16_t) : 0, 0},
                                {&s->d_tp_pre, keep ? (size_t)views * map_bytes(s) : 0, 0},
                                {&s->d_tp_scratch, s->tp_eff.stats ? sgmd_temporal_scratch_bytes() : 0, 0}};
    buf_request want[6];
    int n = 0;
    for (int i = 0; i < 6; ++i)
        if (bufs[i].bytes) want[n++] = bufs[i];
    if (reserve_all(s, want, n, 0)) return 0;
    fprintf(stderr, "sgm_mi355x: device allocation failed for the temporal filter of %d views of %dx%d\n", views, s->g.W, s->g.H);
    return -1;
}

/* the 2 T passes of the refinement on `disp`, in place (include/sgm_mi355x.h, sgm_set_refine) */
static int refine_passes(sgm_instance* s, void* st, void* disp, const void* conf, const void* guide, const refine_params* p)
{
    int rc = 0;
    for (int t = 0; rc == 0 && t < p->iters; ++t) {
        rc = sgmd_refine_pass(s->device, st, &s->g, 0, p->tab[t], guide, t == 0 ? disp : NULL, t == 0 ? conf : NULL, s->d_rf_u.p,
                              s->d_rf_v.p, s->d_rf_q.p, t == 0, 0, 0, NULL);
        if (rc == 0)
            rc = sgmd_refine_pass(s->device, st, &s->g, 1, p->tab[t], guide, NULL, NULL, s->d_rf_u.p, s->d_rf_v.p, s->d_rf_q.p, 0,
                                  t == p->iters - 1, t == p->iters - 1 ? p->keep_invalid : 0, disp);
    }
    return rc;
}

/* the three Jacobi passes of the hole filling on `disp` (in place, through d_fill_map, which keeps the filled map: stage 9);
 * cls == NULL: pass 3 alone */
static int fill_passes(sgm_instance* s, void* st, void* disp, const void* cls)
{
    const int R = s->opt.max_disparity;
    int rc = 0;
    if (cls) {
        rc = sgmd_fill_pass(s->device, st, &s->g, R, disp, s->d_fill_map.p, cls, 1);                  /* occluded */
        if (rc == 0) rc = sgmd_fill_pass(s->device, st, &s->g, R, s->d_fill_map.p, disp, cls, 2);     /* mismatched */
    }
    if (rc == 0) rc = sgmd_fill_pass(s->device, st, &s->g, R, disp, s->d_fill_map.p, NULL, 3);        /* every hole left */
    if (rc == 0) rc = sgmd_d2d_async(s->device, st, disp, s->d_fill_map.p, map_bytes(s));
    return rc;
}

bool sgm_initialize(sgm_instance* s, uint16_t width, uint16_t height, const SGMOption* option)
{
    if (!s || !option) return false;
    s->initialized = false;
    if (s->async_pending && !sgm_match_wait(s)) return false;    /* its buffers may be re-sized below */
    s->opt = *option;                                            /* SemiGlobalMatching.c:41 */
    if (width == 0 || height == 0) return false;                 /* .c:43 */
    if (option->max_disparity <= option->min_disparity) return false;   /* .c:46 */
    const int D = (uint16_t)(option->max_disparity - option->min_disparity);    /* .c:49 */
    if (D > SGM_MAX_DISPARITY_RANGE) FAIL("disparity range %d exceeds SGM_MAX_DISPARITY_RANGE=%d", D, SGM_MAX_DISPARITY_RANGE);
    if ((long long)width * height > 0x7FFFFFFFLL) FAIL("image too large (width*height must fit in 31 bits)");

    s->g.W = width; s->g.H = height; s->g.D = D;
    s->g.DPL = pick_dpl(D);
    s->g.LPP = 16;
    s->g.Dp = 16 * s->g.DPL;
    /* a batch of frames is VALU-bound: 8 lanes per pixel (twice the disparities per lane, same Dp) spends the
     * fewest instructions per cell; a single frame keeps 16 lanes per pixel for the shorter serial step (measured
     * at KITTI size, one frame: 16 lanes + 32-lane horizontals 0.35 ms, 8 lanes + 32-lane horizontals 0.39 ms, 8 lanes 0.59 ms) */
    {
        const int want = s->env_lanes >= 0 ? s->env_lanes : (s->batch >= 2 ? 8 : 16);      /* SGM_LANES_PER_PIXEL */
        /* negative P1 (defined by the reference's C arithmetic, covered by the parity tests, used by nobody) runs the
         * generic aggregation step, which only exists for 16 lanes per pixel */
        /* the wide census windows feed the aggregation from a cost volume: generic step, 16 lanes per pixel */
        if (want == 8 && option->p1 >= 0 && !volume_fed(s) && s->g.DPL >= 2 && s->g.DPL <= 8 && s->g.DPL != 6) { s->g.LPP = 8; s->g.DPL *= 2; }
    }
    /* one frame per launch: the horizontal lines (W-1 serial steps) are the longest chains of the launch -> spread each
     * pixel of those over 32 lanes (2 lines per wave).  64 lanes (SGM_HL=64, one line per wave) measures the same at
     * KITTI size (0.351 vs 0.349 ms): with one frame the launch is then bound by total VALU issue at ~2 waves per SIMD.
     * Batches with 8 lanes per pixel: 16 lanes on the horizontal lines (4 lines per wave: a third fewer instructions per step of
     * the launch's longest chains for 4 % more instructions in total) -- KITTI 3850 -> 4010 fps through host pointers, aggregation
     * 1.19 -> 1.16 ms per 8 frames alone; 32 and 64 lanes cost more than they shorten (round 2) */
    {
        const int ok64 = (s->g.Dp % 64 == 0) && (s->g.Dp / 64 == 2 || s->g.Dp / 64 == 4 || s->g.Dp / 64 == 8);
        const int ok32 = (s->g.Dp % 32 == 0) && (s->g.Dp / 32 == 2 || s->g.Dp / 32 == 4 || s->g.Dp / 32 == 8 || s->g.Dp / 32 == 16);
        int want = s->env_hl >= 0 ? s->env_hl : ((s->batch == 1 || s->g.LPP == 16) ? 32 : 16);   /* SGM_HL; */   /* D > 128 in batches (16 lanes elsewhere): 32, +2 % at 2880x1988 D=256 */
        const int ok16 = s->g.LPP == 8 && (s->g.Dp / 16 == 2 || s->g.Dp / 16 == 4 || s->g.Dp / 16 == 8 || s->g.Dp / 16 == 16);
        if (want == 64 && !ok64) want = 32;
        if (want == 32 && !ok32) want = 0;
        if (want == 16 && !ok16) want = 0;
        if (want == s->g.LPP || option->p1 < 0 || volume_fed(s)) want = 0;
        s->g.HL = want;
    }
    s->g.dmin = option->min_disparity;
    s->g.B = s->batch;
    s->g.row_begin = 0; s->g.row_end = height;
    if (row_tiled(s)) {
        if (s->tile_begin < 0 || s->tile_begin >= s->tile_end || s->tile_end > height)
            FAIL("row tile [%d,%d) does not fit a frame of %d rows", s->tile_begin, s->tile_end, height);
        s->g.row_begin = s->tile_begin; s->g.row_end = s->tile_end;
    }
    s->tile_left = NULL;
    if (s->read_frame >= s->batch) s->read_frame = 0;
    if ((unsigned long long)width * height * (unsigned)s->g.Dp >= 0xFFFFFFFFull)
        FAIL("cost volume too large: width*height*%d must stay below 2^32 cells (32-bit offsets in the kernels)", s->g.Dp);

    s->paths.ndirs = (s->honor_num_paths && option->num_paths == 4) ? 4 : 8;    /* Q1 */
    s->paths.p1 = option->p1;
    {
        uint16_t lut[256];
        build_p2_table(option->p1, option->p2_init, lut);
        s->paths.pen_max = 0;
        for (int a = 0; a < 256; ++a) if (lut[a] > s->paths.pen_max) s->paths.pen_max = lut[a];
        s->paths.allow_fast = s->env_agg_fast >= 0 ? s->env_agg_fast != 0 : 1;   /* SGM_AGG_FAST=0: keep the plain non-negative-P1 step (parity tests run both) */
    }
    for (int d = 0; d < 8; ++d) {
        s->paths.dx[d] = k_dir_dx[d];
        s->paths.dy[d] = k_dir_dy[d];
        s->paths.anom_line[d] = (d >= 4) ? anomalous_line(width, k_dir_dx[d]) : -1;
    }
    s->paths.ghost_zero = (width >= height);
    s->paths.dir_mask = 0xFF;
    s->paths.run_anom = 1;
    s->need_plane_memset = !s->paths.ghost_zero;

    s->pixel_bits = 8;
    if (s->pixel_bits_req > 8 && row_tiled(s))
        FAIL("images of more than 8 bits (sgm_set_pixel_bits) work on whole frames: not available in row-tile mode (sgm_set_rows)");
    if (s->pixel_bits_req > 8) s->pixel_bits = s->pixel_bits_req;
    s->fill_on = false;
    if (s->fill_req && row_tiled(s))
        FAIL("hole filling (sgm_set_fill_holes) works on whole frames: not available in row-tile mode (sgm_set_rows)");
    s->refine_on = false;
    if (s->refine_req && row_tiled(s))
        FAIL("the refinement (sgm_set_refine) works on whole frames: not available in row-tile mode (sgm_set_rows)");
    if (s->refine_req && s->fill_req)
        FAIL("the refinement (sgm_set_refine) and hole filling (sgm_set_fill_holes) do not combine: the refinement fills by itself, "
             "and a filled pixel would carry the confidence of a disparity the LR check rejected");
    s->temporal_on = false;
    if (s->temporal_req && row_tiled(s))
        FAIL("the temporal filter (sgm_set_temporal) works on whole frames: not available in row-tile mode (sgm_set_rows)");
    s->rect_on = false;
    if (s->rect_q && row_tiled(s))
        FAIL("the rectification (sgm_set_rectify) works on whole frames: not available in row-tile mode (sgm_set_rows)");
    if (s->rect_q && (s->rect_w != width || s->rect_h != height))
        FAIL("the rectification maps (sgm_set_rectify) are %dx%d, the frame is %dx%d", s->rect_w, s->rect_h, width, height);
    if (!ensure_buffers(s)) return false;
    if (s->rect_q) {
        if (!upload_rectify(s)) return false;
        s->rect_on = true;
    }
    if (s->fill_req) {
        if (ensure_fill(s) != 0) return false;
        s->fill_on = true;
    }
    if (s->refine_req) {
        if (ensure_refine(s) != 0) return false;
        s->rf_eff = s->rf_req;
        s->refine_on = true;
    }
    if (s->temporal_req) {
        /* (the history survives this: its buffers only grow, and what restarts it is decided where the filter is launched) */
        s->tp_eff = s->tp_req;
        if (ensure_temporal(s, 1, false) != 0) return false;
        s->temporal_on = true;
    }
    /* extras: 4 anomalous lines x H steps x Dp bytes */
    const size_t extras_bytes = (size_t)s->g.B * 4 * height * s->g.Dp;
    if (!reserve(s, &s->d_extras, extras_bytes, 0)) FAIL("device allocation failed (extras)");
    /* median scratch depends on W and H separately (64-row groups x time slots); the granule rows between the bands of a tall
     * frame carry a generation tag: start from "never written" */
    if (!reserve(s, &s->d_median_scratch, sgmd_median_scratch_bytes(&s->g), BUF_ZERO)) FAIL("device allocation failed (median scratch)");
    /* a Reset with unchanged shape and penalties (the per-frame case, Q14) re-uploads nothing */
    if (s->tab_W != width || s->tab_H != height || s->tab_ndirs != s->paths.ndirs || s->tab_p1 != option->p1 ||
        s->tab_p2 != option->p2_init) {
        if (!upload_tables(s)) return false;
        s->tab_W = width; s->tab_H = height; s->tab_ndirs = s->paths.ndirs;
        s->tab_p1 = option->p1; s->tab_p2 = option->p2_init;
    }

    if (row_tiled(s) && !volume_fed(s) && !upload_census_need(s)) return false;

    sum_reset(s);                                                /* .c:57: memset of cost_aggr, done lazily */
    {
        /* one workgroup per image row segment (the launcher cuts rows into up to 4 segments when a launch has few rows);
         * at KITTI size: a batch of 8 frames 0.093 ms per frame against 0.115 + 0.043 for the two separate kernels, a
         * single frame 0.144 against 0.163 */
        const int want = s->env_fused >= 0 ? s->env_fused != 0 : 1;        /* SGM_FUSED_WTA */
        s->fused_wta = sgmd_sum_wta_lr_supported(&s->g, s->row_cap) && want;
    }
    /* the fused last sweep: batches of whole frames with eight paths and non-negative P1 on the reference's census (sgm_upsum.hip
     * has the shapes: W > H, Dp = 128).  SGM_UPSUM=0 / 1 forces it off / on (also for one frame per launch, where its row-to-row chain
     * costs latency) */
    s->up_rows = 0;
    if (s->fused_wta && !row_tiled(s) && reference_census(s) && !wide_pixels(s) && s->paths.ndirs == 8 && option->p1 >= 0 && s->row_cap <= 8 &&
        (s->env_upsum >= 0 ? s->env_upsum != 0 : UPSUM_DEFAULT && s->batch >= 2))
        s->up_rows = sgmd_upsum_rows(&s->g);
    if (s->up_rows > 0 && s->env_upsum_rows >= 1 && s->env_upsum_rows < s->up_rows) s->up_rows = s->env_upsum_rows;
    s->have_ms = false;
    s->last_both = s->last_both_kept = false;
    s->initialized = true;
    return true;
}

bool sgm_reset(sgm_instance* s, uint16_t width, uint16_t height, const SGMOption* option)
{
    if (!s) return false;
    s->initialized = false;                                      /* .c:130 */
    return sgm_initialize(s, width, height, option);
}

/* mark T_x: stage x begins (and the one before it has ended); M_END: the match is queued to its end */
static void mark_on(sgm_instance* s, void* stream, int idx)
{
    if (s->timing && s->timer) sgmd_timer_mark(s->device, s->timer, stream, s->ring_next * MARKS_PER_MATCH + idx);
}
static void mark(sgm_instance* s, int idx) { mark_on(s, s->stream, idx); }

/* .c:94: the path aggregation, from the census images or (wide windows) from the cost volume */
static int launch_aggregation(sgm_instance* s, const sgmd_paths* paths, const void* d_left)
{
    if (volume_fed(s))
        return sgmd_aggregate_volume(s->device, s->stream, &s->g, paths, d_left, s->d_cost.p, s->d_lut.p, s->d_planes, s->plane_bytes,
                                     s->d_extras.p);
    return sgmd_aggregate(s->device, s->stream, &s->g, paths, d_left, s->d_census_l.p, s->d_census_r, s->d_lut.p, s->d_planes,
                          s->plane_bytes, s->d_extras.p);
}

/* the directions of one vertical sense (forward: downwards) */
static int sweep_mask(const sgm_instance* s, int forward)
{
    int m = 0;
    for (int d = 0; d < s->paths.ndirs; ++d)
        if (s->paths.dy[d] == (forward ? 1 : -1)) m |= 1 << d;
    return m;
}

/* d_S <- [d_S +] sum of the planes of the last frame, if the fused kernel skipped that store */
static int materialize_S(sgm_instance* s)
{
    if (s->S.where != S_IN_PLANES && s->S.where != S_IN_PLANES_ADDS) return 0;
    if (ensure_S(s) != 0) return -1;
    /* d_S may still be in use by a cost sum on its own stream; the scratch map below is the speckle pass's label map: a post
     * pass still running on its own stream comes first */
    if (s->sum_pending && sgmd_stream_wait_event(s->device, s->stream, s->ev_sum) != 0) return -1;
    if (s->post_pending && sgmd_stream_wait_event(s->device, s->stream, s->ev_post) != 0) return -1;
    if (s->S.up_missing) {
        /* the last match ran the fused sweep: the three upward planes do not exist.  Walk those directions now (the census images
         * and the kept copy of the left image are still that frame's; the anomalous lines and their cells were done then) */
        sgmd_paths p = s->paths;
        p.dir_mask = sweep_mask(s, 0);
        p.run_anom = 0;
        p.up_fused = 0;
        if (launch_aggregation(s, &p, s->d_left_keep.p) != 0) return -1;
        s->S.up_missing = false;
    }
    /* the left-view WTA this kernel also produces goes to a dead scratch map (speckle labels) */
    const int rc = sgmd_sum_wta(s->device, s->stream, &s->g, s->paths.ndirs, s->d_planes, s->plane_bytes, s->d_extras.p,
                                s->d_row_extras.p, s->d_row_count.p, s->row_cap, s->S.where == S_IN_PLANES_ADDS ? 1 : 0, s->d_S.p, 0, 0.0f,
                                s->d_labels.p);
    if (rc == 0) s->S.where = S_STORED;                          /* a failed launch leaves the sum in the planes */
    return rc;
}

/* Scratch of the fused last sweep and the kept left image.  The kernel's progress words sit BEHIND the hand-over rows, at an
 * offset that depends on (B, W, Dp); their number on H and the rows per workgroup (sgm_upsum.hip).  A word carries
 * (generation << 13) + iterations published, the generation being the low 19 bits of up_gen, and a waiting row group compares
 * (int)(word - want) < 0.
 *   Unchanged geometry: launch g leaves every word at (g << 13) + n, n < 2^13 (each row group's helper stores its final count before
 *   it draws the next ticket), and launch g + 1 asks for ((g + 1) << 13) + c with 1 <= c < 2^13.  The difference is n - c - 2^13 in
 *   [-2^14, 0) modulo 2^32 whatever g is, the wrap of the 19 bits to 0 included: "behind", as it must be.  Nothing to do.
 *   (A launch that is refused after the counter went up skips a generation: the difference is then within -2^15, behind as well.)
 *   Changed geometry (or a scratch that is new): the words' places hold hand-over bytes of the earlier shape, or the words of a
 *   generation far back.  The scratch is zero-filled on s->stream in front of the launch (behind every earlier fused launch: the
 *   stream has waited for ev_sum, or the launch ran on it) and the counter starts over: a zero word is "behind" want only while
 *   generation << 13 stays below 2^31, which a restart at 1 guarantees and a zero-fill alone would not from launch 2^18 on.
 * The one zero-fill of a first launch is the one the allocation always had; an unchanged geometry adds none. */
static int ensure_upsum(sgm_instance* s)
{
    const size_t px = batch_px(s), bytes = sgmd_upsum_scratch_bytes(&s->g);
    const int key[5] = {s->g.B, s->g.W, s->g.H, s->g.Dp, s->up_rows};
    if (!buf_holds(&s->d_up_scratch, bytes)) s->up_key[0] = 0;
    if (!reserve(s, &s->d_up_scratch, bytes, 0)) return -1;
    if (memcmp(key, s->up_key, sizeof key) != 0) {
        s->up_key[0] = 0;                                        /* (B >= 1: 0 = no key) a fill that fails leaves none behind */
        if (sgmd_memset_async(s->device, s->stream, s->d_up_scratch.p, 0, bytes) != 0) return -1;
        memcpy(s->up_key, key, sizeof key);
        s->up_gen = 0;
    }
    return reserve(s, &s->d_left_keep, px, 0) ? 0 : -1;
}

/* .c:94 (sum over the directions), .c:99 and .c:105 (both ComputeDisparity calls) by one of three routes: fused with the last vertical
 * sweep (sweep: the aggregation in front ran with up_fused, behind ensure_upsum), the fused cost sum, or the separate kernels.
 * conf: where the reference view's matching confidence goes (extension), NULL: nowhere. */
static int cost_sum_stage(sgm_instance* s, void* st, void* d_out, void* conf, bool with_marks, bool both, bool sweep)
{
    const SGMOption* o = &s->opt;
    const int accumulate = s->S.where == S_ZERO ? 0 : 1;         /* Q14 (materialize_S came first: zero or in d_S) */
    const int store = s->keep_stages ? 1 : 0;                    /* the fused cost sum writes S only for a test */
    const int uniq = o->is_check_unique ? 1 : 0;
    const float keep = 1 - o->uniqueness_ratio;
    const bool want_right = both || o->is_check_lr || s->reference_view;    /* both: sgm_match_both finishes the right map as well */
    const bool separate = !s->fused_wta;
    sum_where then = S_STORED;                                   /* where S is once the launch below was accepted */
    int rc;
    if ((separate || accumulate || store) && ensure_S(s) != 0) return -1;    /* (never the sweep: S zero, nothing kept) */
    if (sweep) {
        rc = sgmd_upsum(s->device, st, &s->g, &s->paths, s->d_left_keep.p, s->d_census_l.p, s->d_census_r, s->d_lut.p, s->d_planes, s->plane_bytes,
                        s->d_extras.p, s->d_row_extras.p, s->d_row_count.p, s->row_cap, want_right ? 1 : 0, uniq, keep, s->d_up_scratch.p,
                        ++s->up_gen, s->h_status, s->up_rows, s->env_upsum_wgs > 0 ? s->env_upsum_wgs : 0, d_out, s->d_disp_r.p);
        then = S_IN_PLANES;                                      /* five planes + the three materialize_S re-creates */
    } else if (!separate) {
        if (conf)
            rc = sgmd_sum_wta_lr_conf(s->device, st, &s->g, s->paths.ndirs, s->d_planes, s->plane_bytes, s->d_extras.p, s->d_row_extras.p,
                                      s->d_row_count.p, s->row_cap, accumulate, store, want_right ? 1 : 0, s->d_S.p, uniq, keep, d_out,
                                      s->d_disp_r.p, conf, s->reference_view);
        else
            rc = sgmd_sum_wta_lr(s->device, st, &s->g, s->paths.ndirs, s->d_planes, s->plane_bytes, s->d_extras.p,
                                 s->d_row_extras.p, s->d_row_count.p, s->row_cap, accumulate, store, want_right ? 1 : 0, s->d_S.p,
                                 uniq, keep, d_out, s->d_disp_r.p);
        if (!store) then = accumulate ? S_IN_PLANES_ADDS : S_IN_PLANES;
    } else if (conf && !s->reference_view)
        rc = sgmd_sum_wta_conf(s->device, st, &s->g, s->paths.ndirs, s->d_planes, s->plane_bytes, s->d_extras.p,
                               s->d_row_extras.p, s->d_row_count.p, s->row_cap, accumulate, s->d_S.p, uniq, keep, d_out, conf);
    else
        rc = sgmd_sum_wta(s->device, st, &s->g, s->paths.ndirs, s->d_planes, s->plane_bytes, s->d_extras.p,
                          s->d_row_extras.p, s->d_row_count.p, s->row_cap, accumulate, s->d_S.p, uniq, keep, d_out);
    if (rc != 0) return rc;
    sum_accepted(s, then, sweep);                                /* the state holds whatever happens next: the right view below */
    if (with_marks) mark_on(s, st, T_WTA);
    if (separate && conf && s->reference_view) rc = sgmd_wta_right_conf(s->device, st, &s->g, s->d_S.p, uniq, keep, s->d_disp_r.p, conf);
    else if (separate && want_right) rc = sgmd_wta_right(s->device, st, &s->g, s->d_S.p, uniq, keep, s->d_disp_r.p);
    return rc;
}

/* .c:82-83 (+ .c:89 for the wide centre windows, whose cost is materialised): census of both images */
static int prepare_costs(sgm_instance* s, const void* d_left, const void* d_right)
{
    if (wide_pixels(s)) {
        /* extension: one launch for any census kind and window on the u16 samples, which also writes the narrowed images; every
         * word of the frame is written */
        const int cw = s->census_w ? s->census_w : 5, ch = s->census_h ? s->census_h : 5;
        if (!volume_fed(s))
            return sgmd_census16(s->device, s->stream, &s->g, s->pixel_bits, census_symmetric(s), cw, ch, d_left, d_right, s->d_census_l.p,
                                 s->d_census_r, s->d_g8_l.p, s->d_g8_r.p);
        const size_t need = batch_px(s) * 8;
        const buf_request words[] = {{&s->d_census64_l, need, 0}, {&s->d_census64_r, need, 0}};
        if (!reserve_all(s, words, 2, 0)) return -1;
        int rc = ensure_cost(s);
        if (rc == 0) rc = sgmd_census16(s->device, s->stream, &s->g, s->pixel_bits, 0, cw, ch, d_left, d_right, s->d_census64_l.p,
                                        s->d_census64_r.p, s->d_g8_l.p, s->d_g8_r.p);
        if (rc == 0) rc = sgmd_cost64(s->device, s->stream, &s->g, s->d_census64_l.p, s->d_census64_r.p, s->d_cost.p);
        return rc;
    }
    if (!volume_fed(s)) {
        const bool tiled = row_tiled(s) && !s->keep_stages;          /* stage read-back wants the whole census */
        if (tiled && getenv("SGM_DEBUG_POISON_CENSUS")) {                /* tests: a read of a skipped block must not go unnoticed */
            const size_t bytes = batch_px(s) * 4;
            if (sgmd_memset_async(s->device, s->stream, s->d_census_l.p, 0xA5, bytes) != 0 ||
                sgmd_memset_async(s->device, s->stream, s->d_census_r, 0x5A, bytes) != 0) return -1;
        }
        const void* need = tiled ? s->d_census_need.p : NULL;
        if (census_symmetric(s))                                     /* extension: every word of the blocks is written */
            return sgmd_census_sym(s->device, s->stream, &s->g, s->census_w ? s->census_w : 5, s->census_h ? s->census_h : 5, d_left,
                                   d_right, s->d_census_l.p, s->d_census_r, need);
        /* the reference's own boundary, one whole frame per match: the unwritten census words stay as they are (Q3) */
        const int keep_border = s->reference_statics && s->g.B == 1 && !row_tiled(s);
        return sgmd_census(s->device, s->stream, &s->g, d_left, d_right, s->d_census_l.p, s->d_census_r, need, keep_border);
    }
    const size_t need = batch_px(s) * 8;
    const buf_request words[] = {{&s->d_census64_l, need, 0}, {&s->d_census64_r, need, 0}};
    if (!reserve_all(s, words, 2, 0)) return -1;
    int rc = ensure_cost(s);
    if (rc == 0) rc = sgmd_census_window(s->device, s->stream, &s->g, s->census_w, s->census_h, d_left, d_right, s->d_census64_l.p,
                                         s->d_census64_r.p);
    if (rc == 0) rc = sgmd_cost64(s->device, s->stream, &s->g, s->d_census64_l.p, s->d_census64_r.p, s->d_cost.p);
    return rc;
}

/* .c:109 LRCheck on the left map -- or, with the right view as the reference view (extension), the mirrored check on the
 * right map, whose result replaces the left map in d_out */
static int lr_stage(sgm_instance* s, void* st, void* d_out)
{
    const SGMOption* o = &s->opt;
    if (!s->reference_view) return o->is_check_lr ? sgmd_lrcheck(s->device, st, &s->g, d_out, s->d_disp_r.p, o->lrcheck_thres) : 0;
    /* the rows this instance computes: all rows of all frames of the batch, or its row tile of each of them */
    int rc = sgmd_lrcheck_right(s->device, st, &s->g, s->d_disp_r.p, d_out, o->lrcheck_thres, o->is_check_lr ? 1 : 0, s->d_labels.p);
    const size_t frame = frame_px(s) * sizeof(float), first = (size_t)s->g.row_begin * s->g.W * sizeof(float);
    const size_t rows = (size_t)(s->g.row_end - s->g.row_begin) * s->g.W * sizeof(float);
    if (rows == frame)                                        /* d_labels: scratch until the speckle pass */
        return rc ? rc : sgmd_d2d_async(s->device, st, d_out, s->d_labels.p, frame * s->g.B);
    for (int f = 0; rc == 0 && f < s->g.B; ++f)
        rc = sgmd_d2d_async(s->device, st, (char*)d_out + f * frame + first, (char*)s->d_labels.p + f * frame + first, rows);
    return rc;
}

/* The buffers of sgm_match_both, sized together on its first use (keep: the right view's snapshots too; staging: the page-locked
 * right map of the host-pointer forms).  The median scratch starts zeroed like d_median_scratch; that fill is queued on s->stream,
 * the median may run on another one. */
static int ensure_both(sgm_instance* s, bool keep, bool staging)
{
    const size_t px4 = map_bytes(s);
    sgmd_geom g2 = s->g;
    g2.B *= 2;
    const size_t med = sgmd_median_scratch_bytes(&g2);
    const bool med_new = !buf_holds(&s->d_both_median, med);
    const buf_request maps[] = {{&s->d_both_raw, px4, 0}, {&s->d_both_maps, 2 * px4, 0}, {&s->d_both_labels, 2 * px4, 0},
                                {&s->d_both_sizes, 2 * px4, 0}, {&s->d_both_totals, 2 * px4, 0}, {&s->d_both_median, med, BUF_ZERO},
                                {&s->d_both_snap, keep ? 2 * px4 : 0, 0}, {&s->h_disp_r, staging ? px4 : 0, BUF_PINNED | BUF_LAZY_DRAIN}};
    buf_request want[8];
    int n = 0;
    for (int i = 0; i < 8; ++i)
        if (maps[i].bytes) want[n++] = maps[i];
    if (reserve_all(s, want, n, 0) && (!med_new || !(s->sum_stream || s->post_stream) || sgmd_stream_sync(s->device, s->stream) == 0))
        return 0;
    fprintf(stderr, "sgm_mi355x: device allocation failed for the maps of both views (%zu bytes each)\n", px4);
    return -1;
}

/* .c:115-120 behind the LR check: speckle removal and the median, in place on `maps`.  views == 2 (sgm_match_both, on d_both_maps:
 * the B left maps, then the right ones, with the scratch of that size): one launch sequence for both views instead of two, and the
 * second view's median chain runs beside the first's instead of behind it; the kernels see a batch of 2 B frames: whatever they
 * choose by batch size (speckle tile rows, the median's bands) they choose as a plain match with 2 B frames would.  of_match: the tail
 * of a match -- timed, snapshotted for sgm_keep_stages, hole filling and refinement (conf, guide) hooked in; else the two stages alone. */
typedef struct { void *labels, *sizes, *totals, *median; } post_scratch;      /* the speckle and median scratch of B maps, or of 2 B */

/* The filter behind a match's post pass, on the maps it finished (views == 2: the B left maps, then the right ones): the clear a
 * restart owes, the snapshot for sgm_keep_stages, the launch.  The host's record of the history changes exactly where a launch was
 * accepted: a clear that was queued has restarted the history under the new signature whatever happens next, and a refused
 * filter launch leaves history and record as they were. */
static int temporal_stage(sgm_instance* s, void* st, void* maps, int views, const void* conf)
{
    const size_t streams = temporal_streams(s), px = frame_px(s);
    const int sig[6] = {s->g.W, s->g.H, s->g.B, views == 2 ? 0 : s->reference_view, views, s->tp_eff.sequence};
    sgmd_temporal_params c;
    if (!temporal_spec_valid(&s->tp_eff, true, &c)) return -1;
    if (ensure_temporal(s, views, s->keep_stages != 0) != 0) return -1;
    if (s->tp_restart || memcmp(sig, s->tp_sig, sizeof sig) != 0) {
        if (sgmd_temporal_clear(s->device, st, (size_t)views * streams * px, s->d_tp_value.p, s->d_tp_bits.p) != 0) return -1;
        memcpy(s->tp_sig, sig, sizeof sig);
        s->tp_restart = false;
    }
    if (s->keep_stages && sgmd_d2d_async(s->device, st, s->d_tp_pre.p, maps, (size_t)views * map_bytes(s)) != 0) return -1;
    const int rc = sgmd_temporal(s->device, st, &c, (size_t)views * streams, s->tp_eff.sequence ? (size_t)s->g.B : 1, px, maps,
                                 s->tp_eff.min_conf > 0 ? conf : NULL, s->d_tp_value.p, s->d_tp_bits.p,
                                 s->tp_eff.stats ? s->d_tp_stats.p : NULL, s->tp_eff.stats ? s->d_tp_scratch.p : NULL);
    if (rc == 0) s->tp_stat_maps = s->tp_eff.stats ? views * s->g.B : 0;
    return rc;
}
static int post_pass(sgm_instance* s, void* st, void* maps, int views, bool of_match, const void* conf, const void* guide)
{
    const SGMOption* o = &s->opt;
    const size_t bytes = map_bytes(s);
    const bool keep = of_match && s->keep_stages;
    const post_scratch x = views == 2 ? (post_scratch){s->d_both_labels.p, s->d_both_sizes.p, s->d_both_totals.p, s->d_both_median.p}
                                      : (post_scratch){s->d_labels.p, s->d_sizes.p, s->d_totals.p, s->d_median_scratch.p};
    sgmd_geom g = s->g;
    g.B *= views;
    int rc = 0;
    if (of_match) mark_on(s, st, T_SPECKLE);
    if (o->is_remove_speckles) rc = sgmd_speckle(s->device, st, &g, maps, 1.0f, o->min_speckle_area, x.labels, x.sizes, x.totals);   /* .c:115 */
    if (rc == 0 && keep) rc = sgmd_d2d_async(s->device, st, s->d_snap_speckle.p, maps, bytes);
    if (rc == 0 && keep && views == 2) rc = sgmd_d2d_async(s->device, st, (char*)s->d_both_snap.p + bytes, (char*)maps + bytes, bytes);
    if (rc == 0 && of_match && s->fill_on) rc = fill_passes(s, st, maps, s->d_fill_class.p);         /* extension; timed as "speckle" */
    if (rc != 0) return rc;
    if (of_match) mark_on(s, st, T_MEDIAN);
    rc = sgmd_median(s->device, st, &g, maps, x.median, s->h_status);                                     /* .c:120 */
    if (rc == 0 && of_match && s->refine_on) rc = refine_passes(s, st, maps, conf, guide, &s->rf_eff);   /* extension; timed as "median" */
    if (rc == 0 && of_match && s->temporal_on) rc = temporal_stage(s, st, maps, views, conf);            /* extension; timed as "median" */
    return rc;
}

/* W < H: the diagonal planes are cleared before the aggregation */
static int clear_diagonal_planes(sgm_instance* s)
{
    int rc = 0;
    if (s->need_plane_memset && s->paths.ndirs > 4)
        for (int f = 0; rc == 0 && f < s->g.B; ++f)
            rc = sgmd_memset_async(s->device, s->stream, (char*)s->d_planes_alloc.p + ((size_t)f * 8 + 4) * s->plane_bytes, 0, 4 * s->plane_bytes);
    return rc;
}

/* The body of SGM_Match (SemiGlobalMatching.c:80-122) on device buffers.  The first launch that is refused ends the
 * match: nothing further is queued and false is returned with the instance in a consistent state -- the cost-sum state
 * still describes exactly the matches that completed, so a later Match without Reset (Q14) accumulates onto the right thing. */
#define LAUNCH(expr) do { if ((expr) != 0) goto failed; } while (0)
typedef struct { void *left, *right; } both_out;
/* d_conf: the device map the cost sum stores the reference view's matching confidence to (extension), NULL: none asked for.
 * both != NULL (sgm_match_both): d_out receives the raw left WTA map, the post pass finishes both views in d_both_maps, from where
 * they are copied to both->left / right (device; NULL: they stay there) */
static bool run_pipeline(sgm_instance* s, const void* d_left, const void* d_right, void* d_out, void* d_conf, const both_out* both)
{
    const int dev = s->device;
    void* st = s->stream;
    const sgmd_geom* g = &s->g;
    const SGMOption* o = &s->opt;
    const size_t px_bytes = map_bytes(s);

    /* stage groups on streams of their own (sgm_set_stage_cus / sgm_set_overlap_post; never in row-tile mode) */
    const bool own_sum = s->sum_stream && !row_tiled(s);
    const bool overlap = s->overlap_post && s->post_stream && !row_tiled(s);
    void *sts = st, *st2 = st;
    s->last_both = s->last_both_kept = false;                    /* until this match is queued to its end */
    s->tp_stat_maps = 0;                                         /* until this match's filter launch is accepted */
    if (s->refine_on && !d_conf) d_conf = s->d_rf_conf.p;        /* the refinement needs the confidence: an internal map */
    if (s->temporal_on && s->tp_eff.min_conf > 0 && !d_conf) d_conf = s->d_rf_conf.p;   /* ... and so does a temporal filter with min_conf */
    /* the aggregation rewrites the planes the previous match's cost sum may still be reading on its own stream */
    if (s->sum_pending) LAUNCH(sgmd_stream_wait_event(dev, st, s->ev_sum));
    LAUNCH(materialize_S(s));                                /* Match without Reset: S of the previous frame is needed now */
    /* rectification (extension): from here on the images are the instance's rectified ones; the caller's are only read.  Everything
     * that reads them -- the census, the aggregation's grey values, the copies for the guide and for the fused sweep, a later
     * materialize_S through that copy -- is queued on this stream, so stream order alone keeps the remap of match n + 1 behind the
     * readers of match n, also with the cost sum and the post pass on streams of their own.  Timed as "census" */
    if (s->rect_on) {
        mark(s, T_CENSUS);
        LAUNCH((wide_pixels(s) ? sgmd_remap16 : sgmd_remap)(dev, st, g, s->d_rect_maps.p, d_left, d_right, s->d_rect_l.p, s->d_rect_r.p));
        d_left = s->d_rect_l.p;
        d_right = s->d_rect_r.p;
    }
    /* the refinement's guide: the caller (or the next match's upload) may rewrite the images while the post pass of this match
     * still runs on a stream of its own, so it reads a private copy.  Two copies by turns: the copy of match n + 2 is queued behind
     * what waited for the post pass of match n (the cost sum of match n + 1 waits for it, and this stream waits for that sum) */
    const void* guide = NULL;
    if (s->refine_on) {
        guide = s->d_rf_guide[s->rf_turn].p;
        s->rf_turn ^= 1;
        if (!wide_pixels(s)) LAUNCH(sgmd_d2d_async(dev, st, (void*)guide, s->reference_view ? d_right : d_left, batch_px(s)));
    }
    if (!s->rect_on) mark(s, T_CENSUS);
    LAUNCH(prepare_costs(s, d_left, d_right));                                                      /* .c:82-83 */
    /* more than 8 bits per sample (extension): the census has written the narrowed images; the guide copy (queued behind it),
     * the aggregation's grey values and everything else below read those */
    if (wide_pixels(s)) {
        d_left = s->d_g8_l.p;
        d_right = s->d_g8_r.p;
        if (s->refine_on) LAUNCH(sgmd_d2d_async(dev, st, (void*)guide, s->reference_view ? d_right : d_left, batch_px(s)));
    }
    mark(s, T_COST);
    /* .c:89: the cost volume is recomputed inside the aggregation kernel; it is only materialised when a
     * test wants to read it back (stage 2) */
    if (s->keep_stages && !volume_fed(s)) {
        LAUNCH(ensure_cost(s));
        LAUNCH(sgmd_cost(dev, st, g, s->d_census_l.p, s->d_census_r, s->d_cost.p));
    }
    mark(s, T_AGGREGATE);
    LAUNCH(clear_diagonal_planes(s));
    /* the last vertical sweep fused with the cost sum (sgmd_upsum): whenever this match neither adds to an earlier S (Q14) nor has
     * to leave S behind for a test, nor asks for the matching confidence (written by the cost-sum kernels) */
    const bool use_up = s->up_rows > 0 && !s->keep_stages && s->S.where == S_ZERO && s->fused_wta && !d_conf && !both;
    s->last_up_rows = use_up ? s->up_rows : 0;
    if (use_up) {
        LAUNCH(ensure_upsum(s));
        LAUNCH(sgmd_d2d_async(dev, st, s->d_left_keep.p, d_left, batch_px(s)));
        sgmd_paths p = s->paths;
        p.up_fused = 1;
        LAUNCH(launch_aggregation(s, &p, d_left));
    } else
        LAUNCH(launch_aggregation(s, &s->paths, d_left));                                           /* .c:94 */
    mark(s, T_SUM);
    if (own_sum) {
        LAUNCH(sgmd_event_record(dev, s->ev_agg, st));
        LAUNCH(sgmd_stream_wait_event(dev, s->sum_stream, s->ev_agg));
        sts = st2 = s->sum_stream;
    }
    /* the cost sum writes d_out and the right-view map, which the previous match's post pass may still be reading */
    if (s->post_pending) LAUNCH(sgmd_stream_wait_event(dev, sts, s->ev_post));
    mark_on(s, sts, M_SUM_BEGIN);
    LAUNCH(cost_sum_stage(s, sts, d_out, d_conf, true, both != NULL, use_up));                      /* .c:94 sum, .c:99, .c:105 */
    if (s->keep_stages) LAUNCH(sgmd_d2d_async(dev, sts, s->d_snap_wta.p, d_out, px_bytes));
    mark_on(s, sts, T_LRCHECK);
    /* the post pass (latency-bound kernels that fill a fraction of the GPU) on its own stream, so that the stream(s) before it
     * can start the next match's census, aggregation and cost sum beside it */
    if (overlap || own_sum) LAUNCH(sgmd_event_record(dev, s->ev_sum, sts));
    if (own_sum) s->sum_pending = true;
    if (overlap) {
        LAUNCH(sgmd_stream_wait_event(dev, s->post_stream, s->ev_sum));
        st2 = s->post_stream;
        s->post_pending = true;                                  /* from here on the post stream has work of this match */
    }
    void* maps = both ? s->d_both_maps.p : d_out;                /* what the post pass finishes */
    if (both)                            /* one dual LR check from the raw maps (d_out, d_disp_r) */
        LAUNCH(sgmd_lrcheck_both(dev, st2, g, d_out, s->d_disp_r.p, o->lrcheck_thres, o->is_check_lr ? 1 : 0, maps, (char*)maps + px_bytes));
    else {
        if (s->fill_on)                  /* hole filling (extension): classes from both WTA maps, before the LR check rewrites them */
            LAUNCH(sgmd_fill_classify(dev, st2, g, s->reference_view ? s->d_disp_r.p : d_out, s->reference_view ? d_out : s->d_disp_r.p,
                                      o->lrcheck_thres, s->reference_view, o->is_check_lr ? 1 : 0, s->d_fill_class.p));
        LAUNCH(lr_stage(s, st2, d_out));                                                                /* .c:109 */
    }
    if (s->keep_stages) LAUNCH(sgmd_d2d_async(dev, st2, s->d_snap_lr.p, maps, px_bytes));
    if (s->keep_stages && both) LAUNCH(sgmd_d2d_async(dev, st2, s->d_both_snap.p, (char*)maps + px_bytes, px_bytes));
    LAUNCH(post_pass(s, st2, maps, both ? 2 : 1, true, d_conf, guide));                                 /* .c:115-120 */
    if (both && both->left) LAUNCH(sgmd_d2d_async(dev, st2, both->left, maps, px_bytes));
    if (both && both->right) LAUNCH(sgmd_d2d_async(dev, st2, both->right, (char*)maps + px_bytes, px_bytes));
    mark_on(s, st2, M_END);
    if (overlap) LAUNCH(sgmd_event_record(dev, s->ev_post, st2));
    else if (own_sum) LAUNCH(sgmd_event_record(dev, s->ev_sum, st2));   /* the post pass ran on the sum stream: "sum done" = all of it */
    s->tail_stream = st2;
    if (s->timing && s->timer) {
        s->ring_next = (s->ring_next + 1) % TIMING_RING;
        if (s->ring_pending < TIMING_RING) ++s->ring_pending;      /* older sets are overwritten */
    }
    s->last_both = both != NULL;
    s->last_both_kept = both != NULL && s->keep_stages;
    return true;
failed:
    /* this match's timing set is incomplete: it is recorded over by the next match (ring_next did not advance).  Work may sit
     * on the sum / post stream without the event a later match would wait for: drain everything, so that nothing of the
     * abandoned match is still running when its buffers are reused */
    if (s->sum_stream || s->post_stream) sync_streams(s);
    s->tail_stream = st;
    FAIL("a kernel launch failed; the match was abandoned");
}

/* ------------------------------------------------------------------ row tiles (one frame over several GPUs)
 *
 * The instance computes rows [row_begin,row_end) of aggregation, cost sum, both WTAs and the LR check.  The
 * vertical and diagonal paths cross tile borders, so a tile's sweep in one vertical sense starts from the path
 * costs of the row just outside the tile -- the neighbouring GPU's last row of that sweep -- which the caller
 * moves between GPUs (sgm_tile_export_boundary -> RCCL send/recv or a peer copy -> sgm_tile_import_boundary).
 * Census and the four anomalous diagonal lines are computed on the whole frame by every GPU (the images are
 * replicated: 2 x W*H bytes; that work is ~1 % of a frame).  Speckle removal and the median are whole-frame
 * passes over the gathered W*H disparity map (sgm_tile_post). */

bool sgm_set_rows(sgm_instance* s, int row_begin, int row_end)
{
    if (!s || row_begin < 0 || row_end < 0 || (row_end != 0 && row_begin >= row_end)) return false;
    s->tile_begin = row_begin;
    s->tile_end = row_end;
    s->initialized = false;      /* takes effect at the next sgm_initialize / sgm_reset */
    return true;
}

static bool tile_aggregate(sgm_instance* s, int dir_mask, int run_anom)
{
    sgmd_paths p = s->paths;
    p.dir_mask = dir_mask;
    p.run_anom = run_anom;
    return launch_aggregation(s, &p, s->tile_left) == 0;
}

bool sgm_tile_begin(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right)
{
    if (!s || !s->initialized || !d_left || !d_right) return false;
    int rc = materialize_S(s);
    if (rc == 0) rc = prepare_costs(s, d_left, d_right);
    if (rc == 0) rc = clear_diagonal_planes(s);
    if (rc != 0) FAIL("a kernel launch failed");
    s->tile_left = d_left;
    int hmask = 0;
    for (int d = 0; d < s->paths.ndirs; ++d)
        if (s->paths.dy[d] == 0) hmask |= 1 << d;
    return tile_aggregate(s, hmask, 1);
}

size_t sgm_tile_boundary_bytes(const sgm_instance* s)
{
    if (!s || !s->initialized) return 0;
    return (size_t)s->g.B * (s->paths.ndirs > 4 ? 3 : 1) * s->g.W * s->g.Dp;     /* [frame of the batch][direction of the sweep][W][Dp] */
}

/* rows of the planes a sweep hands over: `inside` = the tile's last row in walking order, else the row just past
 * the tile's first row against the walking order (where the neighbour's hand-over lands) */
static bool boundary_copy(sgm_instance* s, int forward, void* d_buf, bool do_export)
{
    if (!s || !s->initialized || !d_buf) return false;
    const int row = do_export ? (forward ? s->g.row_end - 1 : s->g.row_begin)
                              : (forward ? s->g.row_begin - 1 : s->g.row_end);
    if (row < 0 || row >= s->g.H) return false;               /* the tile touches the frame edge: nothing to import */
    const size_t row_bytes = (size_t)s->g.W * s->g.Dp;
    const int mask = sweep_mask(s, forward);
    int dirs[8], n = 0;
    for (int d = 0; d < s->paths.ndirs; ++d)
        if ((mask >> d) & 1) dirs[n++] = d;
    /* one launch for all frames and directions: [frame][direction of the sweep][W][Dp] in the buffer */
    return sgmd_plane_rows_copy(s->device, s->stream, s->d_planes, s->plane_bytes, (size_t)row * row_bytes, row_bytes, dirs, n, s->g.B,
                                d_buf, do_export ? 1 : 0) == 0;
}

bool sgm_tile_export_boundary(sgm_instance* s, int forward, void* d_buf) { return boundary_copy(s, forward, d_buf, true); }
bool sgm_tile_import_boundary(sgm_instance* s, int forward, const void* d_buf)
{
    return boundary_copy(s, forward, (void*)d_buf, false);
}

bool sgm_tile_sweep(sgm_instance* s, int forward)
{
    if (!s || !s->initialized || !s->tile_left) return false;
    return tile_aggregate(s, sweep_mask(s, forward), 0);
}

bool sgm_tile_finish(sgm_instance* s, float* d_disp_left)
{
    if (!s || !s->initialized || !s->tile_left || !d_disp_left) return false;
    int rc = cost_sum_stage(s, s->stream, d_disp_left, NULL, false, false, false);
    if (rc == 0) rc = lr_stage(s, s->stream, d_disp_left);
    s->tile_left = NULL;
    if (rc != 0) FAIL("a kernel launch failed");
    return true;
}

bool sgm_tile_post(sgm_instance* s, float* d_disp_left)
{
    if (!s || !s->initialized || !d_disp_left) return false;
    if (post_pass(s, s->stream, d_disp_left, 1, false, NULL, NULL) != 0) FAIL("a kernel launch failed");
    return true;
}

/* the stream the instance's last match finishes on (the post-pass or cost-sum stream when those stages have their own) */
static void* result_stream(sgm_instance* s) { return s->tail_stream ? s->tail_stream : s->stream; }

/* the event later matches wait for before they reuse what the tail of the last match works on */
static void* result_event(sgm_instance* s)
{
    void* st = result_stream(s);
    if (st == s->stream) return NULL;                            /* stream order does it */
    return st == s->post_stream ? s->ev_post : s->ev_sum;
}

/* more work on the result of the last match, queued behind it on the stream it finished on: re-record that stream's "done" event
 * so that the next match's waits cover it */
static int rerecord_result_event(sgm_instance* s)
{
    void* ev = result_event(s);
    return ev ? sgmd_event_record(s->device, ev, result_stream(s)) : 0;
}

/* make `stream` wait for the last match's result */
static int wait_for_result(sgm_instance* s, void* stream)
{
    void* ev = result_event(s);
    if (!ev || stream == result_stream(s)) return 0;
    return sgmd_stream_wait_event(s->device, stream, ev);
}

/* D2H of a result behind the match that produced it.  No event is recorded behind the copy: every entry point that could
 * overwrite the copy's source (the instance's own d_disp / d_depth) starts with sgm_match_wait, i.e. after the copy has
 * completed -- and an event record queued behind a D2H costs the pipelined host-pointer path 3 % (measured: 3830 -> 3700 fps) */
static bool queue_result_copy(sgm_instance* s, void* host_dst, const void* d_src, size_t bytes)
{
    return sgmd_d2h_async(s->device, result_stream(s), host_dst, d_src, bytes) == 0;
}

static void collect_timing(sgm_instance* s)
{
    if (!(s->timing && s->timer)) return;
    /* every match recorded since the last collection (the stream is idle here), oldest first */
    while (s->ring_pending > 0) {
        const int set = ((s->ring_next - s->ring_pending) % TIMING_RING + TIMING_RING) % TIMING_RING;
        const int base = set * MARKS_PER_MATCH;
        --s->ring_pending;
        float ms[T_COUNT];
        bool ok = true;
        for (int i = 0; i < T_COUNT && ok; ++i)
            ok = sgmd_timer_elapsed(s->device, s->timer, base + (i == T_SUM ? M_SUM_BEGIN : i), base + i + 1, &ms[i]) == 0;
        if (!ok) continue;
        for (int i = 0; i < T_COUNT; ++i) {
            s->last_ms[i] = ms[i];
            s->sum_ms[i] += ms[i];
            if (ms[i] < s->min_ms[i]) s->min_ms[i] = ms[i];
        }
        ++s->n_timed;
        s->have_ms = true;
    }
}

#define TILED_MATCH "the instance is in row-tile mode (sgm_set_rows): use the sgm_tile_* sequence"
/* what every whole-frame entry point checks first: an initialized instance (.c:70), all of its buffers (.c:73), no row tile */
static bool whole_frames(sgm_instance* s, bool buffers, const char* tiled)
{
    if (!s || !s->initialized || !buffers) return false;
    if (row_tiled(s)) FAIL("%s", tiled);
    return true;
}

bool sgm_match_device(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, float* d_disp_left)
{
    if (!whole_frames(s, d_left && d_right && d_disp_left, TILED_MATCH) || !images_aligned(s, d_left, d_right)) return false;
    return run_pipeline(s, d_left, d_right, d_disp_left, NULL, NULL);
}

bool sgm_synchronize(sgm_instance* s)
{
    if (!s) return false;
    if (sync_streams(s) != 0) return false;
    collect_timing(s);
    return true;
}

/* Hands the result of a queued host-pointer match to its caller: waits for the stream, copies every staged output to the caller's
 * buffer (.c:122).  The list is empty again on every way out: the next match starts clean. */
bool sgm_match_wait(sgm_instance* s)
{
    if (!s) return false;
    if (!s->async_pending) return true;
    s->async_pending = false;
    const int n = s->async_n, chunks = s->async_chunks;
    s->async_n = 0;
    s->async_chunks = 1;
    size_t done = 0;
    if (n > 0 && chunks > 1) {
        /* the pieces as they arrive; a map that turns out invalid (sgm_synchronize below) has been handed over in part, as a
         * failed SGM_Match leaves its output undefined */
        const size_t piece = s->async_out[0].bytes / (size_t)chunks / 4 * 4;
        for (int i = 0; i + 1 < chunks; ++i) {
            if (sgmd_event_sync(s->device, s->ev_chunk[i]) != 0) break;
            memcpy((char*)s->async_out[0].dst + done, (const char*)s->async_out[0].src + done, piece);
            done += piece;
        }
    }
    if (!sgm_synchronize(s)) return false;
    for (int i = 0; i < n; ++i, done = 0)
        memcpy((char*)s->async_out[i].dst + done, (const char*)s->async_out[i].src + done, s->async_out[i].bytes - done);
    return true;
}

/* the confidence staging: a device map for the host-pointer forms, and a page-locked one for callers whose buffer is not */
static int ensure_conf(sgm_instance* s, bool host_staging)
{
    const size_t need = batch_px(s) * sizeof(uint16_t);
    const buf_request maps[] = {{&s->d_conf, need, 0}, {&s->h_conf, need, BUF_PINNED | BUF_LAZY_DRAIN}};
    return reserve_all(s, maps, host_staging ? 2 : 1, 0) ? 0 : -1;
}

#define TILED_CONF "the matching confidence works on whole frames: not available in row-tile mode (sgm_set_rows)"
/* what every confidence entry point checks before it queues anything */
static bool conf_ready(sgm_instance* s, const void* l, const void* r, const void* disp, const void* conf)
{
    if (!whole_frames(s, l && r && disp && conf, TILED_CONF)) return false;
    if (!conf_available()) FAIL("the matching confidence is not part of this build");
    return true;
}

bool sgm_match_confidence_device(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, float* d_disp, uint16_t* d_conf)
{
    if (!conf_ready(s, d_left, d_right, d_disp, d_conf) || !images_aligned(s, d_left, d_right)) return false;
    return run_pipeline(s, d_left, d_right, d_disp, d_conf, NULL);
}

/* The frame of the host-pointer entries (sgm_match_async and its confidence form, sgm_match_both_async, sgm_match_planes_async):
 * validate and wait for the match before (afterwards the staging buffers are free again), see which output buffers of the caller
 * are page-locked (outputs_pinned), size the staging, upload the images, run the pipeline, queue the outputs (queue_outputs). */
static bool host_entry_ready(sgm_instance* s, const void* in_a, const void* in_b, const void* out)
{
    return whole_frames(s, in_a && in_b && out, TILED_MATCH) && sgm_match_wait(s);
}

/* an output of such an entry: the caller's buffer, the page-locked staging buffer for a pageable one, where it is on the device */
typedef struct { void* caller; const sgm_buf* staging; const sgm_buf* device; size_t offset, bytes; bool pinned; } host_out;

static void outputs_pinned(sgm_instance* s, host_out* out, int n)
{
    for (int i = 0; i < n; ++i) out[i].pinned = sgmd_host_is_pinned(s->device, out[i].caller, out[i].bytes) != 0;
}

/* H2D from the caller's buffer, staged unless that buffer is page-locked (sgm_host_alloc) */
static bool upload(sgm_instance* s, void* d_dst, const void* src, void* staging, size_t bytes)
{
    if (!sgmd_host_is_pinned(s->device, src, bytes)) { memcpy(staging, src, bytes); src = staging; }
    return sgmd_h2d_async(s->device, s->stream, d_dst, src, bytes) == 0;
}

/* The end of such an entry (ok: everything before went well).  A failed entry drains the streams: queued copies may still read the
 * caller's / staging buffers.  chunk_first: a staged out[0] of RESULT_CHUNK_MIN bytes or more comes back in pieces -- a single frame:
 * 0.92 -> 0.88 ms per blocking call; batches of 8 through four pipelined instances on pageable buffers: 3500 -> 3640 fps.  Two pieces
 * for a map of a few MB (an event and a wait per piece: 1.86 MB in 2 / 4 / 8 pieces = 0.708 / 0.733 / 0.79 ms per blocking KITTI
 * frame), RESULT_CHUNKS for more (a batch of 8 such maps: 3520 / 3575 / 3590 fps pipelined). */
static bool queue_outputs(sgm_instance* s, bool ok, const host_out* out, int n, bool chunk_first)
{
    int chunks = 1;
    s->async_n = 0;
    for (int k = 0; ok && k < n; ++k) {
        const host_out* o = &out[k];
        const char* src = (const char*)o->device->p + o->offset;
        if (k == 0 && chunk_first && !o->pinned && o->bytes >= RESULT_CHUNK_MIN) {
            chunks = o->bytes < RESULT_CHUNK_SPLIT ? 2 : RESULT_CHUNKS;
            for (int i = 0; ok && i < chunks - 1; ++i)
                if (!s->ev_chunk[i]) ok = sgmd_event_create(s->device, &s->ev_chunk[i]) == 0;
            const size_t piece = o->bytes / (size_t)chunks / 4 * 4;
            size_t off = 0;
            for (int i = 0; ok && i < chunks; ++i) {
                const size_t bytes = i + 1 < chunks ? piece : o->bytes - off;
                ok = queue_result_copy(s, (char*)o->staging->p + off, src + off, bytes) &&
                     (i + 1 == chunks || sgmd_event_record(s->device, s->ev_chunk[i], result_stream(s)) == 0);
                off += bytes;
            }
        } else
            ok = queue_result_copy(s, o->pinned ? o->caller : o->staging->p, src, o->bytes);
        if (!o->pinned) s->async_out[s->async_n++] = (handover){o->caller, o->staging->p, o->bytes};
    }
    if (!ok) { s->async_n = 0; sync_streams(s); return false; }
    s->async_pending = true;
    s->async_chunks = chunks;
    return true;
}

/* The host-pointer match without the final wait: stages the images (not at all when the caller's buffers are pinned,
 * sgm_host_alloc), queues H2D, the pipeline and D2H on the instance's stream and returns.  With a few instances
 * round-robined by the caller, the copies of one overlap the kernels of the others (separate DMA engines). */
/* conf != NULL (sgm_match_confidence_async): the confidence map comes back behind the disparity map, through s->d_conf.p (written by
 * the cost sum, long done by then) */
static bool match_async(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left, uint16_t* conf)
{
    if (!host_entry_ready(s, img_left, img_right, disp_left)) return false;
    const size_t px = batch_px(s);           /* batch > 1: B consecutive frames */
    host_out out[2] = {{disp_left, &s->h_disp, &s->d_disp, 0, px * sizeof(float), false},
                       {conf, &s->h_conf, &s->d_conf, 0, px * sizeof(uint16_t), false}};
    const int n = conf ? 2 : 1;
    outputs_pinned(s, out, n);
    if (conf && ensure_conf(s, !out[1].pinned) != 0) FAIL("device allocation failed for the confidence map");
    /* the left image is on the bus while the right one is staged */
    const size_t img = image_bytes(s);
    const bool ok = upload(s, s->d_left.p, img_left, s->h_left.p, img) && upload(s, s->d_right.p, img_right, s->h_right.p, img) &&
                    run_pipeline(s, s->d_left.p, s->d_right.p, s->d_disp.p, conf ? s->d_conf.p : NULL, NULL);
    return queue_outputs(s, ok, out, n, true);
}

bool sgm_match_async(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left)
{
    return match_async(s, img_left, img_right, disp_left, NULL);
}

bool sgm_match(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left)
{
    return sgm_match_async(s, img_left, img_right, disp_left) && sgm_match_wait(s);
}

bool sgm_match_confidence_async(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left, uint16_t* conf)
{
    if (!conf_ready(s, img_left, img_right, disp_left, conf)) return false;
    return match_async(s, img_left, img_right, disp_left, conf);
}

bool sgm_match_confidence(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left, uint16_t* conf)
{
    return sgm_match_confidence_async(s, img_left, img_right, disp_left, conf) && sgm_match_wait(s);
}

/* ------------------------------------------------------------------ both views' maps from one match (extension) */

#define TILED_BOTH "both views' maps need whole frames: not available in row-tile mode (sgm_set_rows)"
/* what every sgm_match_both entry point checks before it queues (or allocates) anything */
static bool both_ready(sgm_instance* s, const void* l, const void* r, const void* disp_l, const void* disp_r)
{
    if (!whole_frames(s, l && r && disp_l && disp_r, TILED_BOTH)) return false;
    if (s->fill_on || s->refine_on)
        FAIL("sgm_match_both does not combine with hole filling or the refinement: their class map and confidence are defined for one view");
    if (s->temporal_on && s->tp_eff.min_conf > 0)
        FAIL("sgm_match_both does not combine with a temporal filter with min_conf > 0: the confidence is defined for one view");
    if (!both_available()) FAIL("sgm_match_both is not part of this build");
    return true;
}

bool sgm_match_both_device(sgm_instance* s, const uint8_t* d_left, const uint8_t* d_right, float* d_disp_left, float* d_disp_right)
{
    if (!both_ready(s, d_left, d_right, d_disp_left, d_disp_right) || !images_aligned(s, d_left, d_right) ||
        ensure_both(s, s->keep_stages != 0, false) != 0 || (s->temporal_on && ensure_temporal(s, 2, s->keep_stages != 0) != 0))
        return false;
    const both_out out = {d_disp_left, d_disp_right};
    return run_pipeline(s, d_left, d_right, s->d_both_raw.p, NULL, &out);
}

/* as match_async; the two maps come back from the halves of d_both_maps, each in one piece */
bool sgm_match_both_async(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left, float* disp_right)
{
    if (!both_ready(s, img_left, img_right, disp_left, disp_right) || !sgm_match_wait(s)) return false;
    const size_t px = batch_px(s), bytes = px * sizeof(float);
    host_out out[2] = {{disp_left, &s->h_disp, &s->d_both_maps, 0, bytes, false},
                       {disp_right, &s->h_disp_r, &s->d_both_maps, bytes, bytes, false}};
    outputs_pinned(s, out, 2);
    if (ensure_both(s, s->keep_stages != 0, !out[1].pinned) != 0 || (s->temporal_on && ensure_temporal(s, 2, s->keep_stages != 0) != 0))
        return false;
    const both_out maps = {NULL, NULL};
    const size_t img = image_bytes(s);
    const bool ok = upload(s, s->d_left.p, img_left, s->h_left.p, img) && upload(s, s->d_right.p, img_right, s->h_right.p, img) &&
                    run_pipeline(s, s->d_left.p, s->d_right.p, s->d_both_raw.p, NULL, &maps);
    return queue_outputs(s, ok, out, 2, false);
}

bool sgm_match_both(sgm_instance* s, const uint8_t* img_left, const uint8_t* img_right, float* disp_left, float* disp_right)
{
    return sgm_match_both_async(s, img_left, img_right, disp_left, disp_right) && sgm_match_wait(s);
}

void* sgm_host_alloc(sgm_instance* s, size_t bytes)
{
    void* p = NULL;
    if (!s || sgmd_alloc_pinned(s->device, &p, bytes) != 0) return NULL;
    return p;
}
void sgm_host_free(sgm_instance* s, void* p) { if (s && p) sgmd_free_pinned(s->device, p); }

/* ------------------------------------------------------------------ test-platform arithmetic on device buffers (8f-3) */

bool sgm_disparity_to_depth(sgm_instance* s, const float* d_disparity, size_t count, float fx, float baseline, float doffs,
                            float* d_depth)
{
    if (!s || !d_disparity || !d_depth) return false;
    /* the map may be the result of a match whose last stages run on a stream of their own (sgm_set_overlap_post / _stage_cus) */
    if (wait_for_result(s, s->stream) != 0) return false;
    return sgmd_depth(s->device, s->stream, d_disparity, count, fx, baseline, doffs, d_depth) == 0;
}

bool sgm_depth_from_both(sgm_instance* s, const float* d_disp_left, const float* d_disp_right, size_t count, float fx_left,
                         float fx_right, float baseline, float doffs, float* d_depth)
{
    if (!s || !d_disp_left || !d_disp_right || !d_depth) return false;
    if (!sgmd_depth_both) FAIL("the depth from both maps is not part of this build");
    if (wait_for_result(s, s->stream) != 0) return false;
    return sgmd_depth_both(s->device, s->stream, d_disp_left, d_disp_right, count, fx_left, fx_right, baseline, doffs, d_depth) == 0;
}

/* ------------------------------------------------------------------ point clouds (extension) */

/* The cloud launchers (sgm_cloud.hip), weakly referenced like the extensions above: a host built without them has no clouds */
#pragma weak sgmd_cloud_scratch_bytes
#pragma weak sgmd_cloud_organized
#pragma weak sgmd_cloud_points
static bool cloud_available(void) { return sgmd_cloud_scratch_bytes != NULL && sgmd_cloud_organized != NULL && sgmd_cloud_points != NULL; }

static bool finite_positive(float v) { return isfinite(v) && v > 0.0f; }

/* ---- what the entry points that read a map share (clouds, registration, volume; the scale spec and the temporal filter in part) */

/* a frame the kernels take, (y << 16) | x naming its pixels, and at most 2^31 pixels in `frames` of them */
static bool frame_size_valid(int width, int height, long long frames)
{
    return width >= 1 && width <= 65535 && height >= 1 && height <= 65535 && frames * width * height <= (1LL << 31);
}

static bool aligned_to(const void* p, size_t bytes) { return (uintptr_t)p % bytes == 0; }

static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    return a && b && (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

/* The map `entry` reads: the caller's, or (d_disp == NULL) the reference-view final map of the last match, where stage 8 finds it --
 * of an initialised instance that is not row-tiled and whose frames are the spec's.  NULL, with a line on stderr, where there is none. */
static const float* source_map(sgm_instance* s, const sgmd_cloud* c, const float* d_disp, const char* entry)
{
    if (d_disp) return d_disp;
    const float* last = s->initialized ? (const float*)(s->last_both ? s->d_both_maps.p : s->d_disp.p) : NULL;
    if (!last)
        fprintf(stderr, "sgm_mi355x: %s: no map given and no match to take one from\n", entry);
    else if (row_tiled(s))
        fprintf(stderr, "sgm_mi355x: %s: the map of a row tile is the caller's: pass it explicitly\n", entry);
    else if (c->W != s->g.W || c->H != s->g.H || c->B != s->g.B)
        fprintf(stderr, "sgm_mi355x: %s: the source spec is for %d frames of %dx%d, the instance's last match for %d of %dx%d\n", entry,
                c->B, c->W, c->H, s->g.B, s->g.W, s->g.H);
    else
        return last;
    return NULL;
}

/* The scratch `what` of an entry point that works on the last match's result (b == NULL: none), then its place in the queue: behind
 * that result, which may come from a stream of its own (sgm_set_overlap_post / _stage_cus).  The scratch first: growing it drains
 * the streams, since an earlier call may still be using it. */
static bool scratch_then_wait(sgm_instance* s, sgm_buf* b, size_t bytes, const char* what)
{
    if (b && !reserve(s, b, bytes, 0)) FAIL("device allocation failed for %s (%zu bytes)", what, bytes);
    return wait_for_result(s, s->stream) == 0;
}

/* the spec as the kernels take it; false for anything outside the ranges of include/sgm_mi355x.h */
static bool cloud_spec_valid(const sgm_cloud_spec* sp, sgmd_cloud* c)
{
    if (sp->frames < 1 || !frame_size_valid(sp->width, sp->height, sp->frames)) return false;
    const float fb = (float)((double)sp->fx * (double)sp->baseline);
    if (!finite_positive(sp->fx) || !finite_positive(sp->fy) || !finite_positive(sp->baseline) || !finite_positive(fb)) return false;
    if (!isfinite(sp->cx) || !isfinite(sp->cy) || !isfinite(sp->doffs)) return false;
    if (!(sp->z_min >= 0.0f) || !(sp->z_max > sp->z_min) || sp->min_conf > 65535u) return false;       /* !(..) also catches NaN */
    *c = (sgmd_cloud){sp->width, sp->height, sp->frames, sp->fx, sp->fy, sp->cx, sp->cy, fb, sp->doffs, sp->z_min, sp->z_max, sp->min_conf};
    return true;
}

/* What the cloud entry points check before they queue anything; *disp: the map to read (source_map) */
static bool cloud_ready(sgm_instance* s, const sgm_cloud_spec* spec, const void* out, sgmd_cloud* c, const float** disp, const char* entry)
{
    if (!s || !spec || !out) return false;
    if (!cloud_available()) FAIL("the point clouds are not part of this build");
    if (!cloud_spec_valid(spec, c)) return false;
    *disp = source_map(s, c, *disp, entry);
    return *disp != NULL;
}

bool sgm_cloud_organized(sgm_instance* s, const sgm_cloud_spec* spec, const float* d_disp, const uint8_t* d_mask,
                         const uint16_t* d_conf, float* d_xyz)
{
    sgmd_cloud c;
    if (!cloud_ready(s, spec, d_xyz, &c, &d_disp, "sgm_cloud_organized")) return false;
    /* the map may be the result of a match whose last stages run on a stream of their own (sgm_set_overlap_post / _stage_cus) */
    if (wait_for_result(s, s->stream) != 0) return false;
    return sgmd_cloud_organized(s->device, s->stream, &c, d_disp, d_mask, d_conf, d_xyz) == 0;
}

/* the point list into any device buffers, behind the last match; the tile scratch is the instance's */
static bool cloud_points_queue(sgm_instance* s, const sgmd_cloud* c, const float* d_disp, const uint8_t* d_mask, const uint16_t* d_conf,
                               void* d_points, void* d_offsets)
{
    if (!scratch_then_wait(s, &s->d_cloud_scratch, sgmd_cloud_scratch_bytes(c->W, c->H, c->B), "the point list's tiles")) return false;
    return sgmd_cloud_points(s->device, s->stream, c, d_disp, d_mask, d_conf, s->d_cloud_scratch.p, d_points, d_offsets) == 0;
}

bool sgm_cloud_points(sgm_instance* s, const sgm_cloud_spec* spec, const float* d_disp, const uint8_t* d_mask,
                      const uint16_t* d_conf, sgm_point* d_points, uint32_t* d_offsets)
{
    sgmd_cloud c;
    if (!d_offsets || !aligned_to(d_points, sizeof(sgm_point)) || !cloud_ready(s, spec, d_points, &c, &d_disp, "sgm_cloud_points")) return false;
    return cloud_points_queue(s, &c, d_disp, d_mask, d_conf, d_points, d_offsets);
}

bool sgm_read_cloud(sgm_instance* s, const sgm_cloud_spec* spec, sgm_point* points, size_t capacity, uint32_t* offsets)
{
    sgmd_cloud c;
    const float* d_disp = NULL;
    if (!offsets || (!points && capacity) || !cloud_ready(s, spec, offsets, &c, &d_disp, "sgm_read_cloud")) return false;
    if (!sgm_match_wait(s)) return false;
    const size_t px = (size_t)c.B * c.W * c.H, off_bytes = ((size_t)c.B + 1) * sizeof(uint32_t);
    const buf_request bufs[] = {{&s->d_cloud_points, px * sizeof(sgm_point), 0}, {&s->d_cloud_offsets, off_bytes, 0}};
    if (!reserve_all(s, bufs, 2, 0)) FAIL("device allocation failed for the point list of %d frames of %dx%d", c.B, c.W, c.H);
    if (!cloud_points_queue(s, &c, d_disp, NULL, NULL, s->d_cloud_points.p, s->d_cloud_offsets.p)) return false;
    if (sgmd_d2h_async(s->device, s->stream, offsets, s->d_cloud_offsets.p, off_bytes) != 0 || sync_streams(s) != 0) return false;
    const size_t total = offsets[c.B];
    if (total > capacity) return false;                          /* the caller sizes a buffer from offsets[frames] and calls again */
    if (total == 0) return true;
    return sgmd_d2h_async(s->device, s->stream, points, s->d_cloud_points.p, total * sizeof(sgm_point)) == 0 && sync_streams(s) == 0;
}

/* ------------------------------------------------------------------ depth registered to another camera (extension) */

/* The launchers of sgm_register.hip, weakly referenced like the extensions above: a host built without them has no registration */
#pragma weak sgmd_register_scratch_bytes
#pragma weak sgmd_register_depth
#pragma weak sgmd_register_gather
static bool register_available(void) { return sgmd_register_scratch_bytes != NULL && sgmd_register_depth != NULL && sgmd_register_gather != NULL; }

/* the target as the kernels take it; false for anything outside the ranges of include/sgm_mi355x.h */
static bool register_spec_valid(const sgm_register_spec* sp, int frames, sgmd_register* r)
{
    if (!frame_size_valid(sp->width, sp->height, frames)) return false;
    if (!finite_positive(sp->fx) || !finite_positive(sp->fy) || !isfinite(sp->cx) || !isfinite(sp->cy)) return false;
    for (int i = 0; i < 5; ++i) if (!isfinite(sp->dist[i])) return false;
    for (int i = 0; i < 9; ++i) if (!isfinite(sp->R[i])) return false;
    for (int i = 0; i < 3; ++i) if (!isfinite(sp->t[i])) return false;
    if (!(sp->z_min >= 0.0f) || !(sp->z_max > sp->z_min) || (sp->splat != 1 && sp->splat != 2)) return false;     /* !(..) also catches NaN */
    r->W = sp->width; r->H = sp->height;
    r->fx = sp->fx; r->fy = sp->fy; r->cx = sp->cx; r->cy = sp->cy;
    memcpy(r->dist, sp->dist, sizeof r->dist);
    memcpy(r->R, sp->R, sizeof r->R);
    memcpy(r->t, sp->t, sizeof r->t);
    r->z_min = sp->z_min; r->z_max = sp->z_max;
    r->splat = sp->splat;
    return true;
}

/* What both entry points check of their specs before they queue anything */
static bool register_specs(sgm_instance* s, const sgm_cloud_spec* src, const sgm_register_spec* dst, sgmd_cloud* c, sgmd_register* r)
{
    if (!s || !src || !dst) FAIL("sgm_register: NULL instance or spec");
    if (!register_available()) FAIL("the registration is not part of this build");
    if (!cloud_spec_valid(src, c)) FAIL("sgm_register: the source spec is outside its ranges");
    if (!register_spec_valid(dst, c->B, r)) FAIL("sgm_register: the target spec is outside its ranges");
    return true;
}

bool sgm_register_depth(sgm_instance* s, const sgm_cloud_spec* src, const sgm_register_spec* dst, const float* d_disp,
                        const uint8_t* d_mask, const uint16_t* d_conf, float* d_depth, uint32_t* d_source)
{
    sgmd_cloud c;
    sgmd_register r;
    if (!register_specs(s, src, dst, &c, &r)) return false;
    if (!d_depth) FAIL("sgm_register_depth: NULL output");
    if (!aligned_to(d_disp, sizeof(float)) || !aligned_to(d_conf, sizeof(uint16_t)) || !aligned_to(d_depth, sizeof(float)) ||
        !aligned_to(d_source, sizeof(uint32_t)))
        FAIL("sgm_register_depth: a pointer is not aligned to its element");
    d_disp = source_map(s, &c, d_disp, "sgm_register_depth");
    if (!d_disp) return false;
    const size_t in_bytes = (size_t)c.B * c.W * c.H * sizeof(float), out_bytes = (size_t)c.B * r.W * r.H * sizeof(float);
    if (ranges_overlap(d_depth, out_bytes, d_disp, in_bytes) || ranges_overlap(d_source, out_bytes, d_disp, in_bytes) ||
        ranges_overlap(d_depth, out_bytes, d_source, out_bytes))
        FAIL("sgm_register_depth: an output aliases the map or the other output");
    if (!scratch_then_wait(s, &s->d_register_keys, sgmd_register_scratch_bytes(r.W, r.H, c.B), "the z-buffer")) return false;
    return sgmd_register_depth(s->device, s->stream, &c, &r, d_disp, d_mask, d_conf, s->d_register_keys.p, d_depth, d_source) == 0;
}

bool sgm_register_gather(sgm_instance* s, const sgm_cloud_spec* src, const sgm_register_spec* dst, const uint32_t* d_source,
                         int elem_bytes, const void* d_map, const void* fill, void* d_out)
{
    sgmd_cloud c;
    sgmd_register r;
    if (!register_specs(s, src, dst, &c, &r)) return false;
    if (!d_source || !d_map || !fill || !d_out) FAIL("sgm_register_gather: NULL argument");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) FAIL("sgm_register_gather: elements of %d bytes (1, 2 or 4)", elem_bytes);
    if (!aligned_to(d_source, sizeof(uint32_t)) || !aligned_to(d_map, (size_t)elem_bytes) || !aligned_to(d_out, (size_t)elem_bytes))
        FAIL("sgm_register_gather: a pointer is not aligned to its element");
    const size_t in_bytes = (size_t)c.B * c.W * c.H * (size_t)elem_bytes, px = (size_t)c.B * r.W * r.H;
    if (ranges_overlap(d_out, px * (size_t)elem_bytes, d_map, in_bytes) || ranges_overlap(d_out, px * (size_t)elem_bytes, d_source, px * 4))
        FAIL("sgm_register_gather: the output aliases an input");
    uint32_t fill_word = 0;
    memcpy(&fill_word, fill, (size_t)elem_bytes);                /* (little endian: the element in the low bytes) */
    if (wait_for_result(s, s->stream) != 0) return false;
    return sgmd_register_gather(s->device, s->stream, &c, &r, d_source, elem_bytes, d_map, fill_word, d_out) == 0;
}

bool sgm_register_spec_raw(const double K[9], const double dist[5], const double R[9], int width, int height, int splat,
                           sgm_register_spec* out)
{
    /* (frames 0: a target has no pixel count until a call brings the frames) */
    if (!K || !dist || !R || !out || !frame_size_valid(width, height, 0) || (splat != 1 && splat != 2)) return false;
    for (int i = 0; i < 9; ++i) if (!isfinite(K[i]) || !isfinite(R[i])) return false;
    for (int i = 0; i < 5; ++i) if (!isfinite(dist[i])) return false;
    memset(out, 0, sizeof *out);
    out->width = width; out->height = height;
    out->fx = (float)K[0]; out->fy = (float)K[4]; out->cx = (float)K[2]; out->cy = (float)K[5];
    for (int i = 0; i < 5; ++i) out->dist[i] = (float)dist[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out->R[3 * i + j] = (float)R[3 * j + i];      /* back out of the rectified camera: the transpose */
    out->z_min = 0.0f; out->z_max = INFINITY;
    out->splat = splat;
    return true;
}

/* ------------------------------------------------------------------ depth fused into a TSDF volume (extension) */

/* The launchers of sgm_volume.hip, weakly referenced like the extensions above: a host built without them has no volume */
#pragma weak sgmd_volume_scratch_bytes
#pragma weak sgmd_volume_integrate
#pragma weak sgmd_volume_points
static bool volume_available(void) { return sgmd_volume_scratch_bytes != NULL && sgmd_volume_integrate != NULL && sgmd_volume_points != NULL; }

/* the volume as the kernels take it; false for anything outside the ranges of include/sgm_mi355x.h */
static bool volume_spec_valid(const sgm_volume_spec* sp, sgmd_volume* v)
{
    if (sp->nx < 1 || sp->nx > 1024 || sp->ny < 1 || sp->ny > 1024 || sp->nz < 1 || sp->nz > 1024 ||
        (long long)sp->nx * sp->ny * sp->nz > (1LL << 30))
        return false;
    if (!finite_positive(sp->voxel) || !finite_positive(sp->trunc) || sp->max_weight < 1u || sp->max_weight > 65535u) return false;
    for (int i = 0; i < 3; ++i) if (!isfinite(sp->origin[i])) return false;
    *v = (sgmd_volume){sp->nx, sp->ny, sp->nz, sp->voxel, {sp->origin[0], sp->origin[1], sp->origin[2]}, sp->trunc, sp->max_weight};
    return true;
}

static size_t volume_bytes(const sgmd_volume* v) { return (size_t)v->nx * v->ny * v->nz * sizeof(uint32_t); }

size_t sgm_volume_bytes(const sgm_volume_spec* spec)
{
    sgmd_volume v;
    if (!spec || !volume_spec_valid(spec, &v)) return 0;
    return volume_bytes(&v);
}

/* every entry of the poses of `frames` frames is finite */
static bool poses_finite(const char* entry, const float* poses, int frames)
{
    for (int i = 0; i < 12 * frames; ++i)
        if (!isfinite(poses[i])) FAIL("%s: entry %d of the pose of frame %d is not finite", entry, i % 12, i / 12);
    return true;
}

bool sgm_volume_integrate(sgm_instance* s, const sgm_volume_spec* spec, const sgm_cloud_spec* src, const float* poses, const float* d_disp,
                          const uint8_t* d_mask, const uint16_t* d_conf, uint32_t* d_voxels)
{
    sgmd_volume v;
    sgmd_cloud c;
    if (!s || !spec || !src || !poses || !d_voxels) FAIL("sgm_volume_integrate: NULL argument");
    if (!volume_available()) FAIL("the volume is not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_integrate: the volume spec is outside its ranges");
    if (!cloud_spec_valid(src, &c)) FAIL("sgm_volume_integrate: the source spec is outside its ranges");
    if (c.B > SGMD_MAX_POSES) FAIL("sgm_volume_integrate: %d frames in one call (at most %d)", c.B, SGMD_MAX_POSES);
    if (!poses_finite("sgm_volume_integrate", poses, c.B)) return false;
    if (!aligned_to(d_disp, sizeof(float)) || !aligned_to(d_conf, sizeof(uint16_t)) || !aligned_to(d_voxels, sizeof(uint32_t)))
        FAIL("sgm_volume_integrate: a pointer is not aligned to its element");
    d_disp = source_map(s, &c, d_disp, "sgm_volume_integrate");
    if (!d_disp) return false;
    const size_t px = (size_t)c.B * c.W * c.H, vol_bytes = volume_bytes(&v);
    if (ranges_overlap(d_voxels, vol_bytes, d_disp, px * sizeof(float)) || ranges_overlap(d_voxels, vol_bytes, d_mask, px) ||
        ranges_overlap(d_voxels, vol_bytes, d_conf, px * sizeof(uint16_t)))
        FAIL("sgm_volume_integrate: the volume aliases a map");
    /* the map may be the result of a match whose last stages run on a stream of their own (sgm_set_overlap_post / _stage_cus) */
    if (wait_for_result(s, s->stream) != 0) return false;
    return sgmd_volume_integrate(s->device, s->stream, &v, &c, poses, d_disp, d_mask, d_conf, d_voxels) == 0;
}

bool sgm_volume_points(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_voxels, uint32_t min_weight,
                       sgm_surface_point* d_points, size_t capacity, uint32_t* d_count)
{
    sgmd_volume v;
    if (!s || !spec || !d_voxels || !d_count || (!d_points && capacity)) FAIL("sgm_volume_points: NULL argument");
    if (!volume_available()) FAIL("the volume is not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_points: the volume spec is outside its ranges");
    if (min_weight < 1u || min_weight > 65535u) FAIL("sgm_volume_points: a min_weight of %u (1..65535)", min_weight);
    if (!aligned_to(d_voxels, sizeof(uint32_t)) || !aligned_to(d_points, sizeof(sgm_surface_point)) || !aligned_to(d_count, sizeof(uint32_t)))
        FAIL("sgm_volume_points: a pointer is not aligned (the points to 16 bytes, the others to their element)");
    const size_t vol_bytes = volume_bytes(&v), n = vol_bytes / sizeof(uint32_t);
    /* (no more than three crossings per voxel can be written, whatever the capacity says) */
    const size_t pts_bytes = (capacity < 3 * n ? capacity : 3 * n) * sizeof(sgm_surface_point);
    if (ranges_overlap(d_points, pts_bytes, d_voxels, vol_bytes) || ranges_overlap(d_count, sizeof(uint32_t), d_voxels, vol_bytes) ||
        ranges_overlap(d_count, sizeof(uint32_t), d_points, pts_bytes))
        FAIL("sgm_volume_points: an output aliases the volume or the other output");
    if (!scratch_then_wait(s, &s->d_volume_scratch, sgmd_volume_scratch_bytes(v.nx, v.ny, v.nz), "the surface list's tiles")) return false;
    return sgmd_volume_points(s->device, s->stream, &v, d_voxels, min_weight, s->d_volume_scratch.p, d_points, capacity, d_count) == 0;
}

/* The mesh's launchers, weak symbols of their own: a host built with the volume but without them keeps the volume */
#pragma weak sgmd_mesh_scratch_bytes
#pragma weak sgmd_volume_mesh
static bool mesh_available(void) { return sgmd_mesh_scratch_bytes != NULL && sgmd_volume_mesh != NULL; }

#define MESH_MAX_VOXELS ((size_t)1 << 27)       /* n*8 + kind, 7 vertices per voxel and 12 triangles per cell fit 32 bits */

bool sgm_volume_mesh(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_voxels, uint32_t min_weight,
                     sgm_mesh_vertex* d_vertices, size_t vertex_capacity, sgm_mesh_triangle* d_triangles, size_t triangle_capacity,
                     uint32_t* d_counts)
{
    sgmd_volume v;
    if (!s || !spec || !d_voxels || !d_counts || (!d_vertices && vertex_capacity) || (!d_triangles && triangle_capacity))
        FAIL("sgm_volume_mesh: NULL argument");
    if (!mesh_available()) FAIL("sgm_volume_mesh: the mesh is not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_mesh: the volume spec is outside its ranges");
    const size_t vol_bytes = volume_bytes(&v), n = vol_bytes / sizeof(uint32_t);
    if (n > MESH_MAX_VOXELS) FAIL("sgm_volume_mesh: %zu voxels (at most 2^27: ids and counts are 32 bits)", n);
    if (min_weight < 1u || min_weight > 65535u) FAIL("sgm_volume_mesh: a min_weight of %u (1..65535)", min_weight);
    if (!aligned_to(d_voxels, sizeof(uint32_t)) || !aligned_to(d_vertices, sizeof(sgm_mesh_vertex)) ||
        !aligned_to(d_triangles, sizeof(sgm_mesh_triangle)) || !aligned_to(d_counts, sizeof(uint32_t)))
        FAIL("sgm_volume_mesh: a pointer is not aligned (the vertices and triangles to 16 bytes, the others to their element)");
    /* (no more than seven vertices per voxel and twelve triangles per cell can be written, whatever the capacities say) */
    const size_t vtx_bytes = (vertex_capacity < 7 * n ? vertex_capacity : 7 * n) * sizeof(sgm_mesh_vertex);
    const size_t tri_bytes = (triangle_capacity < 12 * n ? triangle_capacity : 12 * n) * sizeof(sgm_mesh_triangle);
    const size_t cnt_bytes = 2 * sizeof(uint32_t);
    if (ranges_overlap(d_vertices, vtx_bytes, d_voxels, vol_bytes) || ranges_overlap(d_triangles, tri_bytes, d_voxels, vol_bytes) ||
        ranges_overlap(d_counts, cnt_bytes, d_voxels, vol_bytes) || ranges_overlap(d_vertices, vtx_bytes, d_triangles, tri_bytes) ||
        ranges_overlap(d_counts, cnt_bytes, d_vertices, vtx_bytes) || ranges_overlap(d_counts, cnt_bytes, d_triangles, tri_bytes))
        FAIL("sgm_volume_mesh: an output overlaps the volume or another output");
    if (!scratch_then_wait(s, &s->d_mesh_scratch, sgmd_mesh_scratch_bytes(v.nx, v.ny, v.nz), "the mesh's tiles")) return false;
    return sgmd_volume_mesh(s->device, s->stream, &v, d_voxels, min_weight, s->d_mesh_scratch.p, d_vertices, vertex_capacity, d_triangles,
                            triangle_capacity, d_counts) == 0;
}

/* The ray-cast's launcher, a weak symbol of its own: a host built with the volume but without it keeps the volume */
#pragma weak sgmd_volume_raycast
static bool raycast_available(void) { return sgmd_volume_raycast != NULL; }

/* the view as the kernel takes it; NULL, or what is outside the ranges of include/sgm_mi355x.h */
static const char* raycast_spec_invalid(const sgm_raycast_spec* sp, sgmd_raycast* r)
{
    if (sp->frames < 1 || sp->frames > SGMD_MAX_POSES) return "1..64 frames in one call (the poses travel as kernel arguments)";
    if (!frame_size_valid(sp->width, sp->height, sp->frames)) return "width and height 1..65535, frames*width*height <= 2^31";
    if (!finite_positive(sp->fx) || !finite_positive(sp->fy)) return "fx, fy finite and > 0";
    if (!isfinite(sp->cx) || !isfinite(sp->cy)) return "cx, cy finite";
    if (!(sp->z_min >= 0.0f)) return "z_min >= 0";                                                  /* !(..) also catches NaN */
    if (!isfinite(sp->z_max) || !(sp->z_max > sp->z_min)) return "z_max finite and > z_min";
    if (!finite_positive(sp->step)) return "step finite and > 0";
    if (!(((double)sp->z_max - (double)sp->z_min) / (double)sp->step < 65536.0)) return "(z_max - z_min) / step < 65536";
    if (sp->min_weight < 1u || sp->min_weight > 65535u) return "min_weight 1..65535";
    *r = (sgmd_raycast){sp->width, sp->height, sp->frames, sp->fx, sp->fy, sp->cx, sp->cy, sp->z_min, sp->z_max, sp->step, sp->min_weight};
    return NULL;
}

bool sgm_volume_raycast(sgm_instance* s, const sgm_volume_spec* vol, const sgm_raycast_spec* view, const float* poses,
                        const uint32_t* d_voxels, float* d_depth, float* d_normal)
{
    sgmd_volume v;
    sgmd_raycast r;
    if (!s || !vol || !view || !poses || !d_voxels || !d_depth) FAIL("sgm_volume_raycast: NULL argument");
    if (!raycast_available()) FAIL("sgm_volume_raycast: the ray-cast is not part of this build");
    if (!volume_spec_valid(vol, &v)) FAIL("sgm_volume_raycast: the volume spec is outside its ranges");
    const char* why = raycast_spec_invalid(view, &r);
    if (why) FAIL("sgm_volume_raycast: the view is outside its ranges (%s)", why);
    if (!poses_finite("sgm_volume_raycast", poses, r.B)) return false;
    if (!aligned_to(d_voxels, sizeof(uint32_t)) || !aligned_to(d_depth, sizeof(float)) || !aligned_to(d_normal, sizeof(float)))
        FAIL("sgm_volume_raycast: a pointer is not aligned to its element");
    const size_t vol_bytes = volume_bytes(&v), depth_bytes = (size_t)r.B * r.W * r.H * sizeof(float);
    if (ranges_overlap(d_depth, depth_bytes, d_voxels, vol_bytes) || ranges_overlap(d_normal, 3 * depth_bytes, d_voxels, vol_bytes) ||
        ranges_overlap(d_normal, 3 * depth_bytes, d_depth, depth_bytes))
        FAIL("sgm_volume_raycast: an output overlaps the volume or the other output");
    /* the volume may be the work of an integration that read a match's result: the same place in the queue as sgm_volume_points */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_volume_raycast(s->device, s->stream, &v, &r, poses, d_voxels, d_depth, d_normal) == 0;
}

/* ------------------------------------------------------------------ colour in the volume (extension) */

/* The coloured launchers of sgm_volume.hip, weak symbols each on its own: a host built without one refuses its entry point and keeps
 * the rest of the volume */
#pragma weak sgmd_volume_integrate_color
#pragma weak sgmd_volume_raycast_color
#pragma weak sgmd_volume_colors

bool sgm_volume_integrate_color(sgm_instance* s, const sgm_volume_spec* spec, const sgm_cloud_spec* src, const float* poses,
                                const float* d_disp, const uint8_t* d_mask, const uint16_t* d_conf, const void* d_image, int channels,
                                uint32_t* d_voxels, uint32_t* d_colors)
{
    sgmd_volume v;
    sgmd_cloud c;
    if (!s || !spec || !src || !poses || !d_voxels || !d_image || !d_colors) FAIL("sgm_volume_integrate_color: NULL argument");
    if (sgmd_volume_integrate_color == NULL) FAIL("sgm_volume_integrate_color: the coloured integration is not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_integrate_color: the volume spec is outside its ranges");
    if (!cloud_spec_valid(src, &c)) FAIL("sgm_volume_integrate_color: the source spec is outside its ranges");
    if (c.B > SGMD_MAX_POSES) FAIL("sgm_volume_integrate_color: %d frames in one call (at most %d)", c.B, SGMD_MAX_POSES);
    if (channels != 1 && channels != 4) FAIL("sgm_volume_integrate_color: %d channels (1: u8 grey, 4: u32 r | g << 8 | b << 16)", channels);
    if (!poses_finite("sgm_volume_integrate_color", poses, c.B)) return false;
    if (!aligned_to(d_disp, sizeof(float)) || !aligned_to(d_conf, sizeof(uint16_t)) || !aligned_to(d_voxels, sizeof(uint32_t)) ||
        !aligned_to(d_colors, sizeof(uint32_t)) || !aligned_to(d_image, (size_t)channels))
        FAIL("sgm_volume_integrate_color: a pointer is not aligned to its element");
    d_disp = source_map(s, &c, d_disp, "sgm_volume_integrate_color");
    if (!d_disp) return false;
    const size_t px = (size_t)c.B * c.W * c.H, vol_bytes = volume_bytes(&v);
    const void* const maps[] = {d_disp, d_mask, d_conf, d_image};
    const size_t map_bytes[] = {px * sizeof(float), px, px * sizeof(uint16_t), px * (size_t)channels};
    for (int i = 0; i < 4; ++i) {
        if (ranges_overlap(d_voxels, vol_bytes, maps[i], map_bytes[i])) FAIL("sgm_volume_integrate_color: the volume aliases a map");
        if (ranges_overlap(d_colors, vol_bytes, maps[i], map_bytes[i])) FAIL("sgm_volume_integrate_color: the colours overlap a map or the image");
    }
    if (ranges_overlap(d_colors, vol_bytes, d_voxels, vol_bytes)) FAIL("sgm_volume_integrate_color: the colours overlap the volume");
    /* the map may be the result of a match whose last stages run on a stream of their own, as in sgm_volume_integrate */
    if (wait_for_result(s, s->stream) != 0) return false;
    return sgmd_volume_integrate_color(s->device, s->stream, &v, &c, poses, d_disp, d_mask, d_conf, d_image, channels, d_voxels, d_colors) == 0;
}

bool sgm_volume_raycast_color(sgm_instance* s, const sgm_volume_spec* vol, const sgm_raycast_spec* view, const float* poses,
                              const uint32_t* d_voxels, const uint32_t* d_colors, float* d_depth, float* d_normal, uint32_t* d_rgba)
{
    sgmd_volume v;
    sgmd_raycast r;
    if (!s || !vol || !view || !poses || !d_voxels || !d_colors || !d_depth || !d_rgba) FAIL("sgm_volume_raycast_color: NULL argument");
    if (sgmd_volume_raycast_color == NULL) FAIL("sgm_volume_raycast_color: the coloured ray-cast is not part of this build");
    if (!volume_spec_valid(vol, &v)) FAIL("sgm_volume_raycast_color: the volume spec is outside its ranges");
    const char* why = raycast_spec_invalid(view, &r);
    if (why) FAIL("sgm_volume_raycast_color: the view is outside its ranges (%s)", why);
    if (!poses_finite("sgm_volume_raycast_color", poses, r.B)) return false;
    if (!aligned_to(d_voxels, sizeof(uint32_t)) || !aligned_to(d_colors, sizeof(uint32_t)) || !aligned_to(d_depth, sizeof(float)) ||
        !aligned_to(d_normal, sizeof(float)) || !aligned_to(d_rgba, sizeof(uint32_t)))
        FAIL("sgm_volume_raycast_color: a pointer is not aligned to its element");
    const size_t vol_bytes = volume_bytes(&v), depth_bytes = (size_t)r.B * r.W * r.H * sizeof(float);
    void* const outs[] = {d_depth, d_normal, d_rgba};
    const size_t out_bytes[] = {depth_bytes, 3 * depth_bytes, depth_bytes};
    for (int i = 0; i < 3; ++i) {
        if (ranges_overlap(outs[i], out_bytes[i], d_voxels, vol_bytes) || ranges_overlap(outs[i], out_bytes[i], d_colors, vol_bytes))
            FAIL("sgm_volume_raycast_color: an output overlaps the volume or the colours");
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) FAIL("sgm_volume_raycast_color: an output overlaps another output");
    }
    /* the same place in the queue as sgm_volume_raycast */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_volume_raycast_color(s->device, s->stream, &v, &r, poses, d_voxels, d_colors, d_depth, d_normal, d_rgba) == 0;
}

bool sgm_volume_colors(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_voxels, const uint32_t* d_colors,
                       const void* d_records, size_t capacity, const uint32_t* d_count, int id_kinds, uint32_t* d_rgba)
{
    sgmd_volume v;
    if (!s || !spec || !d_voxels || !d_colors || (capacity && (!d_records || !d_rgba))) FAIL("sgm_volume_colors: NULL argument");
    if (sgmd_volume_colors == NULL) FAIL("sgm_volume_colors: the colours of a list are not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_colors: the volume spec is outside its ranges");
    if (id_kinds != 4 && id_kinds != 8) FAIL("sgm_volume_colors: id_kinds of %d (8: sgm_mesh_vertex, 4: sgm_surface_point)", id_kinds);
    const size_t vol_bytes = volume_bytes(&v), n = vol_bytes / sizeof(uint32_t);
    if (id_kinds == 8 && n > MESH_MAX_VOXELS) FAIL("sgm_volume_colors: %zu voxels (at most 2^27 for the ids of a mesh)", n);
    if (!aligned_to(d_voxels, sizeof(uint32_t)) || !aligned_to(d_colors, sizeof(uint32_t)) || !aligned_to(d_records, 16) ||
        !aligned_to(d_count, sizeof(uint32_t)) || !aligned_to(d_rgba, sizeof(uint32_t)))
        FAIL("sgm_volume_colors: a pointer is not aligned (the records to 16 bytes, the others to their element)");
    if (capacity > ((size_t)1 << 32)) FAIL("sgm_volume_colors: a capacity of %zu records (ids are 32 bits: at most 2^32)", capacity);
    const void* const ins[] = {d_voxels, d_colors, d_records, d_count};
    const size_t in_bytes[] = {vol_bytes, vol_bytes, capacity * 16, sizeof(uint32_t)};
    for (int i = 0; i < 4; ++i)
        if (ranges_overlap(d_rgba, capacity * sizeof(uint32_t), ins[i], in_bytes[i])) FAIL("sgm_volume_colors: the output overlaps an input");
    if (capacity == 0) return true;
    /* behind the list's own call on this stream, and behind the last match as that call is */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_volume_colors(s->device, s->stream, &v, d_voxels, d_colors, d_records, capacity, d_count, id_kinds, d_rgba) == 0;
}

/* ------------------------------------------------------------------ a window of the volume, and a volume that follows the rig (extension) */

/* The launcher of sgm_window.hip, a weak symbol of its own: a host built without it keeps the volume and refuses the window */
#pragma weak sgmd_volume_window

#define WINDOW_MAX_OFFSET (1 << 20)

/* The spec of a window, dims[] voxels of src's lattice from offset[] on: NULL and *v, *dst filled, or what is wrong with it */
static const char* window_spec_invalid(const sgm_volume_spec* src, const int32_t offset[3], const int32_t dims[3], sgmd_volume* v,
                                       sgm_volume_spec* dst)
{
    if (!volume_spec_valid(src, v)) return "the source spec is outside the volume's ranges";
    *dst = *src;
    dst->nx = dims[0]; dst->ny = dims[1]; dst->nz = dims[2];
    for (int a = 0; a < 3; ++a) {
        if (offset[a] < -WINDOW_MAX_OFFSET || offset[a] > WINDOW_MAX_OFFSET) return "an offset beyond 2^20 voxels";
        const float step = (float)offset[a] * src->voxel;     /* float32: the product, then the sum, each rounded once */
        dst->origin[a] = src->origin[a] + step;
    }
    sgmd_volume w;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || dims[0] > 1024 || dims[1] > 1024 || dims[2] > 1024 ||
        (long long)dims[0] * dims[1] * dims[2] > (1LL << 30))
        return "dims outside the volume's ranges (1..1024 each, at most 2^30 voxels)";
    if (!volume_spec_valid(dst, &w)) return "the window's origin is not finite";
    return NULL;
}

bool sgm_volume_window_spec(const sgm_volume_spec* src, const int32_t offset[3], const int32_t dims[3], sgm_volume_spec* dst)
{
    sgmd_volume v;
    sgm_volume_spec out;
    if (!src || !offset || !dims || !dst) FAIL("sgm_volume_window_spec: NULL argument");
    const char* why = window_spec_invalid(src, offset, dims, &v, &out);
    if (why) FAIL("sgm_volume_window_spec: %s", why);
    *dst = out;
    return true;
}

bool sgm_volume_window(sgm_instance* s, const sgm_volume_spec* src, const int32_t offset[3], const int32_t dims[3],
                       const uint32_t* d_src_voxels, const uint32_t* d_src_colors, uint32_t* d_dst_voxels, uint32_t* d_dst_colors,
                       sgm_volume_spec* dst_out)
{
    sgmd_volume v;
    sgm_volume_spec dst;
    if (!s || !src || !offset || !dims || !d_src_voxels || !d_dst_voxels) FAIL("sgm_volume_window: NULL argument");
    if ((d_src_colors == NULL) != (d_dst_colors == NULL)) FAIL("sgm_volume_window: one colour array without the other");
    if (sgmd_volume_window == NULL) FAIL("sgm_volume_window: the window is not part of this build");
    const char* why = window_spec_invalid(src, offset, dims, &v, &dst);
    if (why) FAIL("sgm_volume_window: %s", why);
    if (!aligned_to(d_src_voxels, sizeof(uint32_t)) || !aligned_to(d_src_colors, sizeof(uint32_t)) ||
        !aligned_to(d_dst_voxels, sizeof(uint32_t)) || !aligned_to(d_dst_colors, sizeof(uint32_t)))
        FAIL("sgm_volume_window: a pointer is not aligned to its element");
    const size_t src_bytes = volume_bytes(&v), dst_bytes = (size_t)dims[0] * dims[1] * dims[2] * sizeof(uint32_t);
    if (ranges_overlap(d_dst_voxels, dst_bytes, d_src_voxels, src_bytes) || ranges_overlap(d_dst_voxels, dst_bytes, d_src_colors, src_bytes) ||
        ranges_overlap(d_dst_colors, dst_bytes, d_src_voxels, src_bytes) || ranges_overlap(d_dst_colors, dst_bytes, d_src_colors, src_bytes) ||
        ranges_overlap(d_dst_voxels, dst_bytes, d_dst_colors, dst_bytes))
        FAIL("sgm_volume_window: a destination array overlaps another array (the window is not made in place)");
    /* the source may be the work of an integration that read a match's result: the same place in the queue as sgm_volume_points */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    if (sgmd_volume_window(s->device, s->stream, &v, offset, dims, d_src_voxels, d_src_colors, d_dst_voxels, d_dst_colors) != 0) return false;
    if (dst_out) *dst_out = dst;
    return true;
}

bool sgm_volume_follow(const sgm_volume_spec* spec, const float pose[12], float focus_z, int32_t granule, int32_t margin, int32_t shift[3])
{
    sgmd_volume v;
    int32_t out[3];
    if (!spec || !pose || !shift) FAIL("sgm_volume_follow: NULL argument");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_follow: the volume spec is outside its ranges");
    if (granule < 1 || margin < 0) FAIL("sgm_volume_follow: a granule of %d (>= 1) or a margin of %d (>= 0)", granule, margin);
    for (int i = 0; i < 12; ++i)
        if (!isfinite(pose[i])) FAIL("sgm_volume_follow: entry %d of the pose is not finite", i);
    if (!isfinite(focus_z)) FAIL("sgm_volume_follow: focus_z is not finite");
    /* in double, every operation on its own (-ffp-contract=off), sums left to right */
    const double c[3] = {0.0 - (double)pose[9], 0.0 - (double)pose[10], (double)focus_z - (double)pose[11]};
    const int n[3] = {v.nx, v.ny, v.nz};
    for (int a = 0; a < 3; ++a) {
        const double P = ((double)pose[a] * c[0] + (double)pose[3 + a] * c[1]) + (double)pose[6 + a] * c[2];
        const double g = (P - (double)spec->origin[a]) / (double)spec->voxel - (double)n[a] / 2.0;
        if (!(fabs(g) < (double)WINDOW_MAX_OFFSET)) FAIL("sgm_volume_follow: the focus is 2^20 voxels or more from the volume's centre");
        const double sh = fabs(g) <= (double)margin ? 0.0 : (double)granule * floor(g / (double)granule + 0.5);
        if (fabs(sh) > (double)WINDOW_MAX_OFFSET) FAIL("sgm_volume_follow: the shift rounds to more than 2^20 voxels");
        out[a] = (int32_t)sh;
    }
    memcpy(shift, out, sizeof out);
    return true;
}

int sgm_volume_leaving(const sgm_volume_spec* spec, const int32_t shift[3], sgm_volume_box boxes[3])
{
    sgmd_volume v;
    if (!spec || !shift || !boxes || !volume_spec_valid(spec, &v)) {
        fprintf(stderr, "sgm_mi355x: sgm_volume_leaving: %s\n", (!spec || !shift || !boxes) ? "NULL argument" : "the volume spec is outside its ranges");
        return -1;
    }
    const int n[3] = {v.nx, v.ny, v.nz};
    int32_t leave[3][2], stay[3][2];                          /* [begin, end) in cells */
    for (int a = 0; a < 3; ++a) {
        const int64_t c = n[a] - 1, sh = shift[a];
        const int64_t cut = sh > 0 ? (sh < c ? sh : c) : (c + sh > 0 ? c + sh : 0);
        if (sh > 0) {
            leave[a][0] = 0; leave[a][1] = (int32_t)cut; stay[a][0] = (int32_t)cut; stay[a][1] = (int32_t)c;
        } else if (sh < 0) {
            leave[a][0] = (int32_t)cut; leave[a][1] = (int32_t)c; stay[a][0] = 0; stay[a][1] = (int32_t)cut;
        } else {
            leave[a][0] = leave[a][1] = 0; stay[a][0] = 0; stay[a][1] = (int32_t)c;
        }
    }
    int count = 0;
    for (int a = 0; a < 3; ++a) {
        sgm_volume_box b;
        bool whole = true;
        for (int i = 0; i < 3; ++i) {
            const int32_t lo = i < a ? stay[i][0] : i == a ? leave[i][0] : 0;
            const int32_t hi = i < a ? stay[i][1] : i == a ? leave[i][1] : n[i] - 1;
            b.lo[i] = lo;
            b.n[i] = hi - lo + 1;                             /* voxels: the cells and one more, so that the last cells are whole */
            whole = whole && hi > lo;
        }
        if (whole) boxes[count++] = b;
    }
    return count;
}

/* ------------------------------------------------------------------ the distance field of the volume (extension) */

/* The launchers of sgm_distance.hip, weak symbols of their own: a host built without them keeps the volume and refuses the two calls */
#pragma weak sgmd_volume_distance
#pragma weak sgmd_volume_distance_field

size_t sgm_volume_distance_bytes(const sgm_volume_spec* spec)
{
    sgmd_volume v;
    if (!spec || !volume_spec_valid(spec, &v)) return 0;
    return volume_bytes(&v) / sizeof(uint32_t) * sizeof(uint16_t);
}

bool sgm_volume_distance(sgm_instance* s, const sgm_volume_spec* spec, const sgm_distance_spec* dist, const uint32_t* d_voxels,
                         uint16_t* d_dist2)
{
    sgmd_volume v;
    if (!s || !spec || !dist || !d_voxels || !d_dist2) FAIL("sgm_volume_distance: NULL argument");
    if (sgmd_volume_distance == NULL) FAIL("sgm_volume_distance: the distance field is not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_distance: the volume spec is outside its ranges");
    if (dist->min_weight < 1u || dist->min_weight > 65535u) FAIL("sgm_volume_distance: a min_weight of %u (1..65535)", dist->min_weight);
    if (dist->radius < 1 || dist->radius > 255) FAIL("sgm_volume_distance: a radius of %d (1..255)", dist->radius);
    if (dist->side < 0 || dist->side > 1 || dist->unknown < 0 || dist->unknown > 1)
        FAIL("sgm_volume_distance: side %d and unknown %d (0 or 1 each)", dist->side, dist->unknown);
    if (!aligned_to(d_voxels, sizeof(uint32_t)) || !aligned_to(d_dist2, sizeof(uint16_t)))
        FAIL("sgm_volume_distance: a pointer is not aligned to its element");
    const size_t vol_bytes = volume_bytes(&v);
    if (ranges_overlap(d_dist2, vol_bytes / 2, d_voxels, vol_bytes)) FAIL("sgm_volume_distance: the output overlaps the volume");
    /* the volume may be the work of an integration that read a match's result: the same place in the queue as sgm_volume_points */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_volume_distance(s->device, s->stream, &v, dist->min_weight, dist->radius, dist->side, dist->unknown, d_voxels, d_dist2) == 0;
}

bool sgm_volume_distance_field(sgm_instance* s, const sgm_volume_spec* spec, const uint16_t* d_out2, const uint16_t* d_in2, float* d_field)
{
    sgmd_volume v;
    if (!s || !spec || !d_out2 || !d_field) FAIL("sgm_volume_distance_field: NULL argument");
    if (sgmd_volume_distance_field == NULL) FAIL("sgm_volume_distance_field: the distance field is not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_distance_field: the volume spec is outside its ranges");
    if (!aligned_to(d_out2, sizeof(uint16_t)) || !aligned_to(d_in2, sizeof(uint16_t)) || !aligned_to(d_field, sizeof(float)))
        FAIL("sgm_volume_distance_field: a pointer is not aligned to its element");
    const size_t vol_bytes = volume_bytes(&v);
    if (ranges_overlap(d_field, vol_bytes, d_out2, vol_bytes / 2) || ranges_overlap(d_field, vol_bytes, d_in2, vol_bytes / 2))
        FAIL("sgm_volume_distance_field: the output overlaps an input");
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_volume_distance_field(s->device, s->stream, &v, d_out2, d_in2, d_field) == 0;
}

/* ------------------------------------------------------------------ connected components of the volume (extension) */

/* The launchers of sgm_components.hip, weak symbols of their own: a host built without them keeps the volume and refuses the calls */
#pragma weak sgmd_components_scratch_bytes
#pragma weak sgmd_volume_components
#pragma weak sgmd_volume_component_of

size_t sgm_volume_components_bytes(const sgm_volume_spec* spec)
{
    sgmd_volume v;
    if (!spec || !volume_spec_valid(spec, &v)) return 0;
    return volume_bytes(&v);
}

bool sgm_volume_components(sgm_instance* s, const sgm_volume_spec* spec, const sgm_component_spec* comp, const uint32_t* d_voxels,
                           uint32_t* d_labels, sgm_component* d_objects, size_t capacity, uint32_t* d_counts)
{
    sgmd_volume v;
    sgmd_components c;
    if (!s || !spec || !comp || !d_voxels || !d_labels || !d_counts || (!d_objects && capacity)) FAIL("sgm_volume_components: NULL argument");
    if (sgmd_volume_components == NULL || sgmd_components_scratch_bytes == NULL)
        FAIL("sgm_volume_components: the components are not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_components: the volume spec is outside its ranges");
    if (comp->min_weight < 1u || comp->min_weight > 65535u) FAIL("sgm_volume_components: a min_weight of %u (1..65535)", comp->min_weight);
    if (comp->set < 0 || comp->set > 1 || comp->unknown < 0 || comp->unknown > 1)
        FAIL("sgm_volume_components: set %d and unknown %d (0 or 1 each)", comp->set, comp->unknown);
    if (comp->connectivity != 6 && comp->connectivity != 26) FAIL("sgm_volume_components: a connectivity of %d (6 or 26)", comp->connectivity);
    if (comp->min_voxels < 1u) FAIL("sgm_volume_components: min_voxels of 0 (at least 1)");
    if (comp->planes < 0 || comp->planes > 4) FAIL("sgm_volume_components: %d planes (0..4)", comp->planes);
    c = (sgmd_components){comp->min_weight, comp->set, comp->unknown, comp->connectivity, comp->min_voxels, comp->planes, {{0}}, {{0}}, {0}};
    for (int q = 0; q < comp->planes; ++q) {
        const sgm_plane* pl = &comp->plane[q];
        bool finite = isfinite(pl->offset) && isfinite(comp->clearance[q]);
        for (int a = 0; a < 3; ++a) finite = finite && isfinite(pl->normal[a]) && isfinite(pl->anchor[a]);
        if (!finite) FAIL("sgm_volume_components: plane %d or its clearance is not finite", q);
        for (int a = 0; a < 3; ++a) { c.normal[q][a] = pl->normal[a]; c.anchor[q][a] = pl->anchor[a]; }
        c.clearance[q] = comp->clearance[q];
    }
    if (!aligned_to(d_voxels, sizeof(uint32_t)) || !aligned_to(d_labels, sizeof(uint32_t)) || !aligned_to(d_counts, sizeof(uint32_t)) ||
        !aligned_to(d_objects, 8))
        FAIL("sgm_volume_components: a pointer is not aligned (the objects to 8 bytes, the others to their element)");
    const size_t vol_bytes = volume_bytes(&v), n = vol_bytes / sizeof(uint32_t);
    /* (no more than one object per voxel can be written, whatever the capacity says) */
    const size_t obj_bytes = (capacity < n ? capacity : n) * sizeof(sgm_component), cnt_bytes = 2 * sizeof(uint32_t);
    if (ranges_overlap(d_labels, vol_bytes, d_voxels, vol_bytes) || ranges_overlap(d_objects, obj_bytes, d_voxels, vol_bytes) ||
        ranges_overlap(d_counts, cnt_bytes, d_voxels, vol_bytes) || ranges_overlap(d_objects, obj_bytes, d_labels, vol_bytes) ||
        ranges_overlap(d_counts, cnt_bytes, d_labels, vol_bytes) || ranges_overlap(d_counts, cnt_bytes, d_objects, obj_bytes))
        FAIL("sgm_volume_components: an output overlaps the volume or another output");
    if (!scratch_then_wait(s, &s->d_components_scratch, sgmd_components_scratch_bytes(v.nx, v.ny, v.nz, capacity), "the components' scratch"))
        return false;
    return sgmd_volume_components(s->device, s->stream, &v, &c, d_voxels, s->d_components_scratch.p, d_labels, d_objects, capacity,
                                  d_counts) == 0;
}

bool sgm_volume_component_of(sgm_instance* s, const sgm_volume_spec* spec, const uint32_t* d_labels, const sgm_component* d_objects,
                             size_t capacity, const uint32_t* d_counts, const void* d_records, size_t records_capacity,
                             const uint32_t* d_records_count, int id_kinds, uint32_t* d_index)
{
    sgmd_volume v;
    if (!s || !spec || !d_labels || !d_counts || (!d_objects && capacity) || (records_capacity && (!d_records || !d_index)))
        FAIL("sgm_volume_component_of: NULL argument");
    if (sgmd_volume_component_of == NULL) FAIL("sgm_volume_component_of: the components are not part of this build");
    if (!volume_spec_valid(spec, &v)) FAIL("sgm_volume_component_of: the volume spec is outside its ranges");
    if (id_kinds != 4 && id_kinds != 8) FAIL("sgm_volume_component_of: id_kinds of %d (8: sgm_mesh_vertex, 4: sgm_surface_point)", id_kinds);
    const size_t vol_bytes = volume_bytes(&v), n = vol_bytes / sizeof(uint32_t);
    if (id_kinds == 8 && n > MESH_MAX_VOXELS) FAIL("sgm_volume_component_of: %zu voxels (at most 2^27 for the ids of a mesh)", n);
    if (!aligned_to(d_labels, sizeof(uint32_t)) || !aligned_to(d_objects, 8) || !aligned_to(d_counts, sizeof(uint32_t)) ||
        !aligned_to(d_records, 16) || !aligned_to(d_records_count, sizeof(uint32_t)) || !aligned_to(d_index, sizeof(uint32_t)))
        FAIL("sgm_volume_component_of: a pointer is not aligned (the records to 16 bytes, the objects to 8, the others to their element)");
    if (records_capacity > ((size_t)1 << 32))
        FAIL("sgm_volume_component_of: a capacity of %zu records (ids are 32 bits: at most 2^32)", records_capacity);
    const void* const ins[] = {d_labels, d_objects, d_counts, d_records, d_records_count};
    const size_t in_bytes[] = {vol_bytes, (capacity < n ? capacity : n) * sizeof(sgm_component), 2 * sizeof(uint32_t), records_capacity * 16,
                               sizeof(uint32_t)};
    for (int i = 0; i < 5; ++i)
        if (ranges_overlap(d_index, records_capacity * sizeof(uint32_t), ins[i], in_bytes[i]))
            FAIL("sgm_volume_component_of: the output overlaps an input");
    if (records_capacity == 0) return true;
    /* behind the list's own call and the components call on this stream, and behind the last match as those calls are */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_volume_component_of(s->device, s->stream, &v, d_labels, d_objects, capacity, d_counts, d_records, records_capacity,
                                    d_records_count, id_kinds, d_index) == 0;
}

void sgm_component_metric(const sgm_volume_spec* spec, const sgm_component* obj, float lo[3], float hi[3], float centroid[3])
{
    if (!spec || !obj) return;
    for (int a = 0; a < 3; ++a) {
        if (lo) lo[a] = spec->origin[a] + (float)obj->lo[a] * spec->voxel;
        if (hi) hi[a] = spec->origin[a] + (float)(obj->hi[a] + 1) * spec->voxel;
        if (centroid) {
            const double mean = obj->voxels ? (double)obj->sum[a] / (double)obj->voxels : 0.0;
            centroid[a] = (float)((double)spec->origin[a] + (mean + 0.5) * (double)spec->voxel);
        }
    }
}

/* ------------------------------------------------------------------ frame-to-model tracking (extension) */

/* The launcher of sgm_track.hip, a weak symbol of its own: a host built without it keeps the volume and the ray-cast */
#pragma weak sgmd_track_sums
static bool track_available(void) { return sgmd_track_sums != NULL; }

#define TRACK_SUMS 29
#define TRACK_MAX_PIXELS (1LL << 24)    /* per frame: a term is at most 2^38, a sum stays at or below 2^62 */

/* the model view as the kernel takes it; NULL, or what is outside the ranges of include/sgm_mi355x.h */
static const char* track_spec_invalid(const sgm_track_spec* sp, sgmd_track* t)
{
    if (sp->width < 1 || sp->width > 65535 || sp->height < 1 || sp->height > 65535) return "width and height 1..65535";
    if (!finite_positive(sp->fx) || !finite_positive(sp->fy)) return "fx, fy finite and > 0";
    if (!isfinite(sp->cx) || !isfinite(sp->cy)) return "cx, cy finite";
    if (!finite_positive(sp->dist_max)) return "dist_max finite and > 0";
    if (!finite_positive(sp->span)) return "span finite and > 0";
    if (sp->iterations < 1 || sp->iterations > 64) return "iterations 1..64";
    if (sp->min_pixels < 6u) return "min_pixels at least 6";
    if (!isfinite(sp->min_pivot) || !(sp->min_pivot >= 0.0f)) return "min_pivot finite and >= 0";
    if (t) *t = (sgmd_track){sp->width, sp->height, sp->fx, sp->fy, sp->cx, sp->cy, sp->dist_max, sp->span};
    return NULL;
}

/* the entry of the pair (i, j), i <= j, of the upper triangle of the 7 x 7 matrix in row-major order */
static double track_sum(const int64_t* sums, int i, int j) { return (double)sums[i * 7 - i * (i - 1) / 2 + (j - i)]; }

bool sgm_track_solve(const sgm_track_spec* model, const int64_t sums[29], const double pose_in[12], double pose_out[12], sgm_track_stats* stats)
{
    if (!model || !sums || !pose_in || !pose_out || !stats) FAIL("sgm_track_solve: NULL argument");
    const char* why = track_spec_invalid(model, NULL);
    if (why) FAIL("sgm_track_solve: the model is outside its ranges (%s)", why);
    for (int i = 0; i < 12; ++i)
        if (!isfinite(pose_in[i])) FAIL("sgm_track_solve: entry %d of the pose is not finite", i);
    if (sums[28] < 0 || sums[28] > TRACK_MAX_PIXELS) FAIL("sgm_track_solve: %lld associated pixels (0..2^24)", (long long)sums[28]);
    const double dist_max = (double)model->dist_max, span = (double)model->span;
    double out[12];
    memcpy(out, pose_in, sizeof out);
    stats->pixels = (uint32_t)sums[28];
    stats->rms = sums[28] > 0 ? dist_max * sqrt((double)sums[27] / (double)sums[28]) / 65536.0 : 0.0;
    stats->status = 0;
    if ((uint64_t)sums[28] < model->min_pixels) stats->status = 1;
    double L[6][6], D[6], y[6], xi[6];
    memset(L, 0, sizeof L);
    for (int j = 0; j < 6 && stats->status == 0; ++j) {
        const double Ajj = track_sum(sums, j, j);
        double acc = 0.0;
        for (int k = 0; k < j; ++k) acc += (L[j][k] * L[j][k]) * D[k];
        D[j] = Ajj - acc;
        if (!isfinite(D[j]) || !(D[j] > (double)model->min_pivot * Ajj)) { stats->status = 2; break; }
        for (int i = j + 1; i < 6; ++i) {
            acc = 0.0;
            for (int k = 0; k < j; ++k) acc += (L[i][k] * L[j][k]) * D[k];
            L[i][j] = (track_sum(sums, j, i) - acc) / D[j];
        }
    }
    if (stats->status == 0) {
        for (int i = 0; i < 6; ++i) {
            double acc = 0.0;
            for (int k = 0; k < i; ++k) acc += L[i][k] * y[k];
            y[i] = track_sum(sums, i, 6) - acc;
        }
        for (int i = 5; i >= 0; --i) {
            double acc = 0.0;
            for (int k = i + 1; k < 6; ++k) acc += L[k][i] * xi[k];
            xi[i] = y[i] / D[i] - acc;
        }
        for (int i = 0; i < 6; ++i)
            if (!isfinite(xi[i])) stats->status = 2;
    }
    if (stats->status == 0) {
        const double k = dist_max / span;
        const double s[3] = {(xi[0] * k) * 0.5, (xi[1] * k) * 0.5, (xi[2] * k) * 0.5};
        const double v[3] = {xi[3] * dist_max, xi[4] * dist_max, xi[5] * dist_max};
        const double ss = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2], a = 1.0 - ss, den = 1.0 + ss;
        const double X[3][3] = {{0.0, -s[2], s[1]}, {s[2], 0.0, -s[0]}, {-s[1], s[0], 0.0}};
        double Ri[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Ri[r][c] = ((a * (r == c ? 1.0 : 0.0) + 2.0 * (s[r] * s[c])) + 2.0 * X[r][c]) / den;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) out[3 * r + c] = (Ri[r][0] * pose_in[c] + Ri[r][1] * pose_in[3 + c]) + Ri[r][2] * pose_in[6 + c];
            out[9 + r] = ((Ri[r][0] * pose_in[9] + Ri[r][1] * pose_in[10]) + Ri[r][2] * pose_in[11]) + v[r];
        }
        for (int i = 0; i < 12; ++i)
            if (!isfinite(out[i])) stats->status = 2;
        if (stats->status != 0) memcpy(out, pose_in, sizeof out);
    }
    memcpy(pose_out, out, sizeof out);
    return true;
}

bool sgm_track_world_pose(const float model_pose[12], const double rel[12], float out[12])
{
    if (!model_pose || !rel || !out) FAIL("sgm_track_world_pose: NULL argument");
    for (int i = 0; i < 12; ++i)
        if (!isfinite(model_pose[i]) || !isfinite(rel[i])) FAIL("sgm_track_world_pose: entry %d of a pose is not finite", i);
    double m[12];
    float res[12];
    for (int i = 0; i < 12; ++i) m[i] = (double)model_pose[i];
    const double dt[3] = {m[9] - rel[9], m[10] - rel[10], m[11] - rel[11]};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) res[3 * r + c] = (float)((rel[r] * m[c] + rel[3 + r] * m[3 + c]) + rel[6 + r] * m[6 + c]);
        res[9 + r] = (float)((rel[r] * dt[0] + rel[3 + r] * dt[1]) + rel[6 + r] * dt[2]);
    }
    memcpy(out, res, sizeof res);
    return true;
}

/* What sgm_track_sums and sgm_track check before they queue anything; *disp: the map to read (source_map).  sums: the caller's
 * device array, or NULL for the instance's own. */
static bool track_ready(sgm_instance* s, const sgm_cloud_spec* src, const sgm_track_spec* model, const float** disp, const uint8_t* d_mask,
                        const uint16_t* d_conf, const float* d_depth, const float* d_normal, const int64_t* sums, sgmd_cloud* c,
                        sgmd_track* t, const char* entry)
{
    if (!track_available()) FAIL("%s: tracking is not part of this build", entry);
    if (!cloud_spec_valid(src, c)) FAIL("%s: the source spec is outside its ranges", entry);
    if (c->B > SGMD_MAX_POSES) FAIL("%s: %d frames in one call (at most %d)", entry, c->B, SGMD_MAX_POSES);
    if ((long long)c->W * c->H > TRACK_MAX_PIXELS) FAIL("%s: a source of %dx%d pixels (at most 2^24: the sums are 64-bit)", entry, c->W, c->H);
    const char* why = track_spec_invalid(model, t);
    if (why) FAIL("%s: the model is outside its ranges (%s)", entry, why);
    if (!aligned_to(*disp, sizeof(float)) || !aligned_to(d_conf, sizeof(uint16_t)) || !aligned_to(d_depth, sizeof(float)) ||
        !aligned_to(d_normal, sizeof(float)) || !aligned_to(sums, sizeof(int64_t)))
        FAIL("%s: a pointer is not aligned (the sums to 8 bytes, the others to their element)", entry);
    *disp = source_map(s, c, *disp, entry);
    if (!*disp) return false;
    const size_t px = (size_t)c->B * c->W * c->H, mpx = (size_t)c->B * t->W * t->H, sum_bytes = (size_t)c->B * TRACK_SUMS * sizeof(int64_t);
    if (ranges_overlap(sums, sum_bytes, *disp, px * sizeof(float)) || ranges_overlap(sums, sum_bytes, d_mask, px) ||
        ranges_overlap(sums, sum_bytes, d_conf, px * sizeof(uint16_t)) || ranges_overlap(sums, sum_bytes, d_depth, mpx * sizeof(float)) ||
        ranges_overlap(sums, sum_bytes, d_normal, 3 * mpx * sizeof(float)))
        FAIL("%s: the sums overlap a map", entry);
    return true;
}

bool sgm_track_sums(sgm_instance* s, const sgm_cloud_spec* src, const sgm_track_spec* model, const float* poses, const float* d_disp,
                    const uint8_t* d_mask, const uint16_t* d_conf, const float* d_model_depth, const float* d_model_normal, int64_t* d_sums)
{
    sgmd_cloud c;
    sgmd_track t;
    if (!s || !src || !model || !poses || !d_model_depth || !d_model_normal || !d_sums) FAIL("sgm_track_sums: NULL argument");
    if (!track_ready(s, src, model, &d_disp, d_mask, d_conf, d_model_depth, d_model_normal, d_sums, &c, &t, "sgm_track_sums")) return false;
    if (!poses_finite("sgm_track_sums", poses, c.B)) return false;
    /* the maps may be the work of a ray-cast on this stream and of a match: the same place in the queue as sgm_volume_raycast */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_track_sums(s->device, s->stream, &c, &t, poses, d_disp, d_mask, d_conf, d_model_depth, d_model_normal, d_sums) == 0;
}

bool sgm_track(sgm_instance* s, const sgm_cloud_spec* src, const sgm_track_spec* model, double* poses, const float* d_disp,
               const uint8_t* d_mask, const uint16_t* d_conf, const float* d_model_depth, const float* d_model_normal,
               sgm_track_stats* stats, int64_t* trace_sums, double* trace_poses)
{
    sgmd_cloud c;
    sgmd_track t;
    if (!s || !src || !model || !poses || !d_model_depth || !d_model_normal || !stats) FAIL("sgm_track: NULL argument");
    if (!track_ready(s, src, model, &d_disp, d_mask, d_conf, d_model_depth, d_model_normal, NULL, &c, &t, "sgm_track")) return false;
    for (int i = 0; i < 12 * c.B; ++i)
        if (!isfinite(poses[i]) || !isfinite((float)poses[i]))
            FAIL("sgm_track: entry %d of the pose of frame %d is not finite as a float", i % 12, i / 12);
    const size_t sum_bytes = (size_t)c.B * TRACK_SUMS * sizeof(int64_t);
    if (!scratch_then_wait(s, &s->d_track_sums, sum_bytes, "the sums of tracking")) return false;
    int64_t sums[SGMD_MAX_POSES * TRACK_SUMS];
    float pose32[SGMD_MAX_POSES * 12];
    bool out[SGMD_MAX_POSES] = {false};                       /* a frame whose solve failed sits out the remaining rounds */
    for (int f = 0; f < c.B; ++f) stats[f] = (sgm_track_stats){0.0, 0u, 0};
    if (trace_poses) memcpy(trace_poses, poses, (size_t)c.B * 12 * sizeof(double));
    for (int it = 0; it < model->iterations; ++it) {
        for (int i = 0; i < 12 * c.B; ++i) pose32[i] = (float)poses[i];
        if (sgmd_track_sums(s->device, s->stream, &c, &t, pose32, d_disp, d_mask, d_conf, d_model_depth, d_model_normal, s->d_track_sums.p) != 0 ||
            sgmd_d2h_async(s->device, s->stream, sums, s->d_track_sums.p, sum_bytes) != 0 || sync_streams(s) != 0)
            return false;
        if (trace_sums) memcpy(trace_sums + (size_t)it * c.B * TRACK_SUMS, sums, sum_bytes);
        for (int f = 0; f < c.B; ++f) {
            if (out[f]) continue;
            double next[12];
            if (!sgm_track_solve(model, sums + f * TRACK_SUMS, poses + 12 * f, next, &stats[f])) return false;
            for (int i = 0; i < 12; ++i)
                if (!isfinite((float)next[i])) stats[f].status = 2;
            if (stats[f].status != 0) out[f] = true;
            else memcpy(poses + 12 * f, next, sizeof next);
        }
        if (trace_poses) memcpy(trace_poses + (size_t)(it + 1) * c.B * 12, poses, (size_t)c.B * 12 * sizeof(double));
    }
    return true;
}

/* ------------------------------------------------------------------ planes in a point list (extension) */

/* The launchers of sgm_plane.hip, weak symbols each on its own: a host built without one refuses its entry point and keeps the rest */
#pragma weak sgmd_plane_votes
#pragma weak sgmd_plane_best
#pragma weak sgmd_plane_sums
#pragma weak sgmd_plane_label

#define PLANE_SUMS 10
#define PLANE_MAX_K 1024
#define PLANE_MAX_RECORDS ((size_t)1 << 32)
#define PLANE_MAX_SUMMED ((size_t)1 << 24)     /* a term is at most 2^38, a sum stays at or below 2^62 */
#define RECORD_BYTES 16

/* the spec as the kernels take it; NULL, or what is outside the ranges of include/sgm_mi355x.h */
static const char* plane_spec_invalid(const sgm_plane_spec* sp, sgmd_plane* p)
{
    if (sp->hypotheses < 1 || sp->hypotheses > PLANE_MAX_K) return "hypotheses 1..1024";
    if (!finite_positive(sp->dist)) return "dist finite and > 0";
    if (!isfinite(sp->axis[0]) || !isfinite(sp->axis[1]) || !isfinite(sp->axis[2])) return "axis finite";
    const int prior = sp->axis[0] != 0.0f || sp->axis[1] != 0.0f || sp->axis[2] != 0.0f;
    const float len = sqrtf((sp->axis[0] * sp->axis[0] + sp->axis[1] * sp->axis[1]) + sp->axis[2] * sp->axis[2]);
    if (prior && !finite_positive(len)) return "an axis with a finite length > 0 as a float";
    if (!isfinite(sp->min_cos) || !(sp->min_cos >= 0.0f) || !(sp->min_cos <= 1.0f)) return "min_cos 0..1";
    if (!finite_positive(sp->span)) return "span finite and > 0";
    if (sp->iterations < 1 || sp->iterations > 64) return "iterations 1..64";
    if (sp->min_inliers < 3u) return "min_inliers at least 3";
    if (!isfinite(sp->min_pivot) || !(sp->min_pivot >= 0.0f)) return "min_pivot finite and >= 0";
    if (p) *p = (sgmd_plane){sp->hypotheses, sp->seed, sp->dist, {sp->axis[0], sp->axis[1], sp->axis[2]}, sp->min_cos * len, sp->span, prior};
    return NULL;
}

/* What the device entry points check of a list before they queue anything */
static bool plane_list_ready(const sgm_plane_spec* spec, const void* d_records, size_t capacity, size_t max_records, const uint32_t* d_count,
                             sgmd_plane* p, const char* entry)
{
    const char* why = plane_spec_invalid(spec, p);
    if (why) FAIL("%s: the spec is outside its ranges (%s)", entry, why);
    if (capacity > max_records) FAIL("%s: a capacity of %zu records (at most 2^%d)", entry, capacity, max_records == PLANE_MAX_RECORDS ? 32 : 24);
    if (!aligned_to(d_records, RECORD_BYTES) || !aligned_to(d_count, sizeof(uint32_t)))
        FAIL("%s: a pointer is not aligned (records and planes to 16 bytes, the sums to 8, the count to 4)", entry);
    return true;
}

/* an output of `bytes` at out against the list (labels: NULL, or the byte per record that is an input here) */
static bool plane_output_clear(const void* out, size_t bytes, const void* d_records, size_t capacity, const uint32_t* d_count,
                               const uint8_t* d_labels, const char* entry)
{
    if (ranges_overlap(out, bytes, d_records, capacity * RECORD_BYTES) || ranges_overlap(out, bytes, d_count, sizeof(uint32_t)) ||
        ranges_overlap(out, bytes, d_labels, capacity))
        FAIL("%s: an output overlaps an input", entry);
    return true;
}

bool sgm_plane_votes(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records, size_t capacity, const uint32_t* d_count,
                     const uint8_t* d_labels, sgm_plane* d_planes)
{
    sgmd_plane p;
    if (!s || !spec || !d_records || !d_planes) FAIL("sgm_plane_votes: NULL argument");
    if (sgmd_plane_votes == NULL) FAIL("sgm_plane_votes: the planes of a list are not part of this build");
    if (!plane_list_ready(spec, d_records, capacity, PLANE_MAX_RECORDS, d_count, &p, "sgm_plane_votes")) return false;
    if (!aligned_to(d_planes, 16)) FAIL("sgm_plane_votes: a pointer is not aligned (records and planes to 16 bytes, the count to 4)");
    if (!plane_output_clear(d_planes, (size_t)p.hypotheses * sizeof(sgm_plane), d_records, capacity, d_count, d_labels, "sgm_plane_votes"))
        return false;
    /* behind the list's own call on this stream, and behind the last match as that call is */
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_plane_votes(s->device, s->stream, &p, d_records, capacity, d_count, d_labels, d_planes) == 0;
}

bool sgm_plane_best(sgm_instance* s, const sgm_plane* d_planes, int K, sgm_plane* d_best)
{
    if (!s || !d_planes || !d_best) FAIL("sgm_plane_best: NULL argument");
    if (sgmd_plane_best == NULL) FAIL("sgm_plane_best: the planes of a list are not part of this build");
    if (K < 1 || K > PLANE_MAX_K) FAIL("sgm_plane_best: %d candidates (1..1024)", K);
    if (!aligned_to(d_planes, 16) || !aligned_to(d_best, 16)) FAIL("sgm_plane_best: a pointer is not aligned (planes to 16 bytes)");
    if (ranges_overlap(d_best, sizeof(sgm_plane), d_planes, (size_t)K * sizeof(sgm_plane))) FAIL("sgm_plane_best: the output overlaps the candidates");
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_plane_best(s->device, s->stream, d_planes, K, d_best) == 0;
}

bool sgm_plane_sums(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records, size_t capacity, const uint32_t* d_count,
                    const uint8_t* d_labels, const sgm_plane* d_plane, int64_t* d_sums)
{
    sgmd_plane p;
    if (!s || !spec || !d_records || !d_plane || !d_sums) FAIL("sgm_plane_sums: NULL argument");
    if (sgmd_plane_sums == NULL) FAIL("sgm_plane_sums: the planes of a list are not part of this build");
    if (!plane_list_ready(spec, d_records, capacity, PLANE_MAX_SUMMED, d_count, &p, "sgm_plane_sums")) return false;
    if (!aligned_to(d_plane, 16) || !aligned_to(d_sums, sizeof(int64_t)))
        FAIL("sgm_plane_sums: a pointer is not aligned (records and planes to 16 bytes, the sums to 8, the count to 4)");
    const size_t sum_bytes = PLANE_SUMS * sizeof(int64_t);
    if (ranges_overlap(d_sums, sum_bytes, d_plane, sizeof(sgm_plane))) FAIL("sgm_plane_sums: an output overlaps an input");
    if (!plane_output_clear(d_sums, sum_bytes, d_records, capacity, d_count, d_labels, "sgm_plane_sums")) return false;
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_plane_sums(s->device, s->stream, &p, d_records, capacity, d_count, d_labels, d_plane, d_sums) == 0;
}

bool sgm_plane_label(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records, size_t capacity, const uint32_t* d_count,
                     const sgm_plane* d_plane, int label, uint8_t* d_labels)
{
    sgmd_plane p;
    if (!s || !spec || !d_records || !d_plane || !d_labels) FAIL("sgm_plane_label: NULL argument");
    if (sgmd_plane_label == NULL) FAIL("sgm_plane_label: the planes of a list are not part of this build");
    if (!plane_list_ready(spec, d_records, capacity, PLANE_MAX_RECORDS, d_count, &p, "sgm_plane_label")) return false;
    if (label < 1 || label > 255) FAIL("sgm_plane_label: a label of %d (1..255)", label);
    if (!aligned_to(d_plane, 16)) FAIL("sgm_plane_label: a pointer is not aligned (records and planes to 16 bytes, the count to 4)");
    if (ranges_overlap(d_labels, capacity, d_plane, sizeof(sgm_plane))) FAIL("sgm_plane_label: an output overlaps an input");
    if (!plane_output_clear(d_labels, capacity, d_records, capacity, d_count, NULL, "sgm_plane_label")) return false;
    if (!scratch_then_wait(s, NULL, 0, NULL)) return false;
    return sgmd_plane_label(s->device, s->stream, &p, d_records, capacity, d_count, d_plane, label, d_labels) == 0;
}

static void plane_cross(const double* p, const double* r, double* out)
{
    out[0] = p[1] * r[2] - p[2] * r[1];
    out[1] = p[2] * r[0] - p[0] * r[2];
    out[2] = p[0] * r[1] - p[1] * r[0];
}

static double plane_dot(const double* p, const double* r) { return (p[0] * r[0] + p[1] * r[1]) + p[2] * r[2]; }

/* M(p, r) of the header for the symmetric matrix M */
static double plane_moment(const double M[3][3], const double* p, const double* r)
{
    const double Mr[3] = {plane_dot(M[0], r), plane_dot(M[1], r), plane_dot(M[2], r)};
    return plane_dot(p, Mr);
}

bool sgm_plane_solve(const sgm_plane_spec* spec, const int64_t sums[10], const sgm_plane* plane_in, sgm_plane* plane_out, sgm_plane_stats* stats)
{
    if (!spec || !sums || !plane_in || !plane_out || !stats) FAIL("sgm_plane_solve: NULL argument");
    sgmd_plane rule;
    const char* why = plane_spec_invalid(spec, &rule);
    if (why) FAIL("sgm_plane_solve: the spec is outside its ranges (%s)", why);
    const double n[3] = {plane_in->normal[0], plane_in->normal[1], plane_in->normal[2]};
    const double A[3] = {plane_in->anchor[0], plane_in->anchor[1], plane_in->anchor[2]};
    for (int i = 0; i < 3; ++i)
        if (!isfinite(n[i]) || !isfinite(A[i])) FAIL("sgm_plane_solve: the plane is not finite");
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) FAIL("sgm_plane_solve: the plane is void");
    if (sums[9] < 0 || sums[9] > (int64_t)PLANE_MAX_SUMMED) FAIL("sgm_plane_solve: %lld inliers (0..2^24)", (long long)sums[9]);
    sgm_plane out = *plane_in;
    stats->inliers = (uint32_t)sums[9];
    stats->rms = 0.0;
    stats->status = 0;
    if ((uint64_t)sums[9] < spec->min_inliers) stats->status = 1;
    if (stats->status == 0) {
        const double N = (double)sums[9];
        const double M[3][3] = {{(double)sums[0], (double)sums[1], (double)sums[2]},
                                {(double)sums[1], (double)sums[4], (double)sums[5]},
                                {(double)sums[2], (double)sums[5], (double)sums[7]}};
        const double m[3] = {(double)sums[3], (double)sums[6], (double)sums[8]};
        const double ln = sqrt(plane_dot(n, n));
        const double w[3] = {n[0] / ln, n[1] / ln, n[2] / ln};
        int axis = 0;
        for (int i = 1; i < 3; ++i)
            if (fabs(w[i]) < fabs(w[axis])) axis = i;
        double e[3] = {0.0, 0.0, 0.0}, c[3], t1[3], t2[3];
        e[axis] = 1.0;
        plane_cross(w, e, c);
        const double lc = sqrt(plane_dot(c, c));
        for (int i = 0; i < 3; ++i) t1[i] = c[i] / lc;
        plane_cross(w, t1, t2);
        const double Su = plane_dot(t1, m), Sv = plane_dot(t2, m), Ss = plane_dot(w, m);
        const double Suu = plane_moment(M, t1, t1), Suv = plane_moment(M, t1, t2), Svv = plane_moment(M, t2, t2);
        const double Sus = plane_moment(M, t1, w), Svs = plane_moment(M, t2, w), Sss = plane_moment(M, w, w);
        const double Am[3][3] = {{N, Su, Sv}, {Su, Suu, Suv}, {Sv, Suv, Svv}};
        const double y[3] = {Ss, Sus, Svs};
        double L[3][3], D[3], z[3], x[3];
        memset(L, 0, sizeof L);
        for (int j = 0; j < 3 && stats->status == 0; ++j) {
            double acc = 0.0;
            for (int k = 0; k < j; ++k) acc += (L[j][k] * L[j][k]) * D[k];
            D[j] = Am[j][j] - acc;
            if (!isfinite(D[j]) || !(D[j] > (double)spec->min_pivot * Am[j][j])) { stats->status = 2; break; }
            for (int i = j + 1; i < 3; ++i) {
                acc = 0.0;
                for (int k = 0; k < j; ++k) acc += (L[i][k] * L[j][k]) * D[k];
                L[i][j] = (Am[i][j] - acc) / D[j];
            }
        }
        if (stats->status == 0) {
            for (int i = 0; i < 3; ++i) {
                double acc = 0.0;
                for (int k = 0; k < i; ++k) acc += L[i][k] * z[k];
                z[i] = y[i] - acc;
            }
            for (int i = 2; i >= 0; --i) {
                double acc = 0.0;
                for (int k = i + 1; k < 3; ++k) acc += L[k][i] * x[k];
                x[i] = z[i] / D[i] - acc;
            }
            for (int i = 0; i < 3; ++i)
                if (!isfinite(x[i])) stats->status = 2;
        }
        if (stats->status == 0) {
            const double g[3] = {(w[0] - x[1] * t1[0]) - x[2] * t2[0], (w[1] - x[1] * t1[1]) - x[2] * t2[1], (w[2] - x[1] * t1[2]) - x[2] * t2[2]};
            const double lg = sqrt(plane_dot(g, g));
            if (!isfinite(lg) || !(lg > 0.0)) stats->status = 2;
            else {
                const double nn[3] = {g[0] / lg, g[1] / lg, g[2] / lg};
                const double gq[3] = {m[0] / N, m[1] / N, m[2] / N};
                const double d = x[0] / lg - plane_dot(nn, gq);
                const double unit = (double)spec->span / 65536.0;
                double Nf[3], af[3];
                for (int i = 0; i < 3; ++i) {
                    out.anchor[i] = (float)(A[i] + (gq[i] + d * nn[i]) * unit);
                    out.normal[i] = (float)nn[i];
                    Nf[i] = (double)out.normal[i];
                    af[i] = (double)out.anchor[i];
                }
                double t = plane_dot(Nf, af);
                const double ax[3] = {spec->axis[0], spec->axis[1], spec->axis[2]};
                if (rule.prior ? plane_dot(Nf, ax) < 0.0 : t > 0.0) {
                    for (int i = 0; i < 3; ++i) out.normal[i] = -out.normal[i];
                    t = -t;
                }
                out.offset = (float)(0.0 - t);
                out.votes = (uint32_t)sums[9];
                double ssr = Sss - ((x[0] * Ss + x[1] * Sus) + x[2] * Svs);
                if (!(ssr >= 0.0)) ssr = 0.0;
                stats->rms = unit * sqrt(ssr / N);
                bool ok = isfinite(out.offset) && isfinite(stats->rms) && (out.normal[0] != 0.0f || out.normal[1] != 0.0f || out.normal[2] != 0.0f);
                for (int i = 0; i < 3; ++i) ok = ok && isfinite(out.normal[i]) && isfinite(out.anchor[i]);
                if (!ok) stats->status = 2;
            }
        }
        if (stats->status != 0) {
            out = *plane_in;
            stats->rms = 0.0;
        }
    }
    *plane_out = out;
    return true;
}

bool sgm_plane_fit(sgm_instance* s, const sgm_plane_spec* spec, const void* d_records, size_t capacity, const uint32_t* d_count,
                   const uint8_t* d_labels, sgm_plane* plane, sgm_plane_stats* stats, int64_t* trace_sums, sgm_plane* trace_planes)
{
    sgmd_plane p;
    if (!s || !spec || !d_records || !plane || !stats) FAIL("sgm_plane_fit: NULL argument");
    if (sgmd_plane_votes == NULL || sgmd_plane_best == NULL || sgmd_plane_sums == NULL) FAIL("sgm_plane_fit: the planes of a list are not part of this build");
    if (!plane_list_ready(spec, d_records, capacity, PLANE_MAX_SUMMED, d_count, &p, "sgm_plane_fit")) return false;
    /* the instance's own: the candidates, the plane that travels, the sums of a round */
    const size_t cand_bytes = (size_t)PLANE_MAX_K * sizeof(sgm_plane), sum_bytes = PLANE_SUMS * sizeof(int64_t);
    if (!scratch_then_wait(s, &s->d_plane_work, cand_bytes + sizeof(sgm_plane) + sum_bytes, "the planes of a fit")) return false;
    char* work = (char*)s->d_plane_work.p;
    void *d_cand = work, *d_plane = work + cand_bytes, *d_sums = work + cand_bytes + sizeof(sgm_plane);
    sgm_plane cur;
    if (sgmd_plane_votes(s->device, s->stream, &p, d_records, capacity, d_count, d_labels, d_cand) != 0 ||
        sgmd_plane_best(s->device, s->stream, d_cand, p.hypotheses, d_plane) != 0 ||
        sgmd_d2h_async(s->device, s->stream, &cur, d_plane, sizeof cur) != 0 || sync_streams(s) != 0)
        return false;
    if (trace_planes) trace_planes[0] = cur;
    *plane = cur;
    *stats = (sgm_plane_stats){0.0, 0u, 0};
    if (cur.normal[0] == 0.0f && cur.normal[1] == 0.0f && cur.normal[2] == 0.0f) {
        stats->status = 1;
        return true;
    }
    for (int it = 0; it < spec->iterations; ++it) {
        int64_t sums[PLANE_SUMS];
        sgm_plane next;
        if ((it > 0 && sgmd_h2d_async(s->device, s->stream, d_plane, &cur, sizeof cur) != 0) ||
            sgmd_plane_sums(s->device, s->stream, &p, d_records, capacity, d_count, d_labels, d_plane, d_sums) != 0 ||
            sgmd_d2h_async(s->device, s->stream, sums, d_sums, sum_bytes) != 0 || sync_streams(s) != 0)
            return false;
        if (trace_sums) memcpy(trace_sums + (size_t)it * PLANE_SUMS, sums, sum_bytes);
        if (!sgm_plane_solve(spec, sums, &cur, &next, stats)) return false;
        cur = next;
        if (trace_planes) trace_planes[it + 1] = cur;
        if (stats->status != 0) break;
    }
    *plane = cur;
    return true;
}

/* ------------------------------------------------------------------ matching at 1/f scale (extension) */

/* The launchers of sgm_scale.hip, weakly referenced like the extensions above: a host built without them has no scaled match */
#pragma weak sgmd_downscale
#pragma weak sgmd_upscale
static bool scale_available(void) { return sgmd_downscale != NULL && sgmd_upscale != NULL; }

/* the spec as the kernels take it; false for anything outside the ranges of include/sgm_mi355x.h */
static bool scale_spec_valid(const sgm_scale_spec* sp, sgmd_scale* c)
{
    if (!sp || sp->frames < 1 || sp->frames > 65535 || !frame_size_valid(sp->width, sp->height, sp->frames)) return false;
    if ((sp->factor != 2 && sp->factor != 4) || sp->width / sp->factor < 1 || sp->height / sp->factor < 1) return false;
    if (sp->bits < 8 || sp->bits > 16 || sp->radius > 4 || sp->penalty < 0 || sp->penalty > 16) return false;
    if (sp->d_lo < 0 || sp->d_lo > sp->d_hi || sp->d_hi > 65535) return false;
    if (c) *c = (sgmd_scale){sp->width, sp->height, sp->frames, sp->factor, sp->bits, sp->radius < 0 ? -1 : sp->radius, sp->penalty,
                             sp->d_lo, sp->d_hi, 0};
    return true;
}

bool sgm_scaled_shape(const sgm_scale_spec* spec, int* w, int* h)
{
    if (!w || !h || !scale_spec_valid(spec, NULL)) return false;
    *w = spec->width / spec->factor;
    *h = spec->height / spec->factor;
    return true;
}

/* what every scaled entry point checks first */
static bool scale_ready(sgm_instance* s, const sgm_scale_spec* spec, bool pointers, sgmd_scale* c)
{
    if (!s || !spec || !pointers) FAIL("a scaled entry point was given a NULL pointer");
    if (!scale_available()) FAIL("matching at 1/f scale is not part of this build");
    if (!scale_spec_valid(spec, c)) FAIL("the scale spec is outside its ranges (include/sgm_mi355x.h, sgm_scale_spec)");
    return true;
}

static bool samples_aligned(const sgmd_scale* c, const void* a, const void* b)
{
    if (c->bits > 8 && (((uintptr_t)a | (uintptr_t)b) & 1u)) FAIL("device images of %d bits per sample must be 2-byte aligned", c->bits);
    return true;
}

bool sgm_downscale(sgm_instance* s, const sgm_scale_spec* spec, const void* d_in, void* d_out)
{
    sgmd_scale c;
    if (!scale_ready(s, spec, d_in && d_out, &c) || !samples_aligned(&c, d_in, d_out)) return false;
    return sgmd_downscale(s->device, s->stream, &c, d_in, d_out) == 0;
}

bool sgm_upscale_disparity(sgm_instance* s, const sgm_scale_spec* spec, const float* d_disp_small, const void* d_guide_small,
                           const void* d_guide_full, const uint32_t* d_census_ref, const uint32_t* d_census_oth, int right_view,
                           float* d_disp_full)
{
    sgmd_scale c;
    const bool planes = (spec && spec->radius < 0) || (d_census_ref && d_census_oth);
    if (!scale_ready(s, spec, d_disp_small && d_guide_small && d_guide_full && d_disp_full && planes, &c) ||
        !samples_aligned(&c, d_guide_small, d_guide_full))
        return false;
    if (((uintptr_t)d_disp_small | (uintptr_t)d_disp_full | (uintptr_t)d_census_ref | (uintptr_t)d_census_oth) & 3u)
        FAIL("the maps and census planes of sgm_upscale_disparity must be 4-byte aligned");
    c.right = right_view ? 1 : 0;
    /* the small map may be the result of a match whose last stages run on a stream of their own */
    if (wait_for_result(s, s->stream) != 0) return false;
    return sgmd_upscale(s->device, s->stream, &c, d_disp_small, d_guide_small, d_guide_full, d_census_ref, d_census_oth, d_disp_full) == 0;
}

/* The composed match on device images (include/sgm_mi355x.h): downscale, the instance's match, the full-resolution census, the
 * upscale with re-search.  Everything is queued on the instance's stream but what the match itself puts elsewhere; later matches
 * write d_disp only behind an event of this stream (run_pipeline), so stream order keeps them behind the upscale's reads. */
static bool scaled_ready(sgm_instance* s, const sgm_scale_spec* spec, const void* l, const void* r, const void* out, sgmd_scale* c)
{
    if (!scale_ready(s, spec, l && r && out, c)) return false;
    if (!s->initialized) FAIL("sgm_match_scaled needs an instance initialised at the low-resolution shape");
    if (row_tiled(s)) FAIL("sgm_match_scaled works on whole frames: not available in row-tile mode (sgm_set_rows)");
    const int w = c->W / c->f, h = c->H / c->f;
    if (s->g.W != w || s->g.H != h || s->g.B != c->B || s->pixel_bits != c->bits)
        FAIL("the scale spec asks for %d frames of %dx%d at %d bits, the instance is initialised for %d of %dx%d at %d", c->B, w, h, c->bits,
             s->g.B, s->g.W, s->g.H, s->pixel_bits);
    if (s->rect_on) FAIL("sgm_match_scaled does not combine with rectification: its maps are for the small shape");
    if (c->radius >= 0 && volume_fed(s)) FAIL("the re-search reads u32 census words: not available with a wide CENTRE census window");
    if (c->radius >= 0 && ((c->bits > 8 && !sgmd_census16) || (c->bits == 8 && census_symmetric(s) && !sgmd_census_sym)))
        FAIL("the census of this instance is not part of this build");
    c->right = s->reference_view;
    c->d_lo = c->f * s->opt.min_disparity;
    c->d_hi = c->f * s->opt.max_disparity - 1;
    return true;
}

static bool scaled_queue(sgm_instance* s, const sgmd_scale* c, const void* d_left, const void* d_right, void* d_out)
{
    const size_t es = c->bits > 8 ? 2 : 1, px = (size_t)c->B * c->W * c->H;
    const bool search = c->radius >= 0;
    const buf_request bufs[] = {{&s->d_sc_small_l, image_bytes(s), 0}, {&s->d_sc_small_r, image_bytes(s), 0},
                                {&s->d_sc_census_l, search ? px * 4 : 0, 0}, {&s->d_sc_census_r, search ? px * 4 : 0, 0},
                                {&s->d_sc_g8_l, search && es == 2 ? px : 0, 0}, {&s->d_sc_g8_r, search && es == 2 ? px : 0, 0}};
    int n = 0;
    buf_request need[6];
    for (int i = 0; i < 6; ++i)
        if (bufs[i].bytes) need[n++] = bufs[i];
    if (!reserve_all(s, need, n, 0)) FAIL("device allocation failed for the scaled match of %d frames of %dx%d", c->B, c->W, c->H);
    const int dev = s->device;
    void* st = s->stream;
    if (sgmd_downscale(dev, st, c, d_left, s->d_sc_small_l.p) != 0 || sgmd_downscale(dev, st, c, d_right, s->d_sc_small_r.p) != 0)
        FAIL("the downscale launch failed; the scaled match was abandoned");
    if (!run_pipeline(s, s->d_sc_small_l.p, s->d_sc_small_r.p, s->d_disp.p, NULL, NULL)) return false;
    if (search) {
        /* the census of the full-resolution views, by the instance's kind: every word written, the border 0 */
        sgmd_geom gf = s->g;
        gf.W = c->W; gf.H = c->H;
        gf.row_begin = 0; gf.row_end = c->H;
        const int cw = s->census_w ? s->census_w : 5, ch = s->census_h ? s->census_h : 5;
        int rc;
        if (es == 2)
            rc = sgmd_census16(dev, st, &gf, c->bits, census_symmetric(s), cw, ch, d_left, d_right, s->d_sc_census_l.p, s->d_sc_census_r.p,
                               s->d_sc_g8_l.p, s->d_sc_g8_r.p);
        else if (census_symmetric(s))
            rc = sgmd_census_sym(dev, st, &gf, cw, ch, d_left, d_right, s->d_sc_census_l.p, s->d_sc_census_r.p, NULL);
        else
            rc = sgmd_census(dev, st, &gf, d_left, d_right, s->d_sc_census_l.p, s->d_sc_census_r.p, NULL, 0);
        if (rc != 0) FAIL("the full-resolution census launch failed; the scaled match was abandoned");
    }
    if (wait_for_result(s, st) != 0) return false;
    const bool right = c->right != 0;
    if (sgmd_upscale(dev, st, c, s->d_disp.p, right ? s->d_sc_small_r.p : s->d_sc_small_l.p, right ? d_right : d_left,
                     search ? (right ? s->d_sc_census_r.p : s->d_sc_census_l.p) : NULL,
                     search ? (right ? s->d_sc_census_l.p : s->d_sc_census_r.p) : NULL, d_out) != 0)
        FAIL("the upscale launch failed; the scaled match was abandoned");
    return true;
}

bool sgm_match_scaled_device(sgm_instance* s, const sgm_scale_spec* spec, const uint8_t* d_left, const uint8_t* d_right, float* d_disp_full)
{
    sgmd_scale c;
    if (!scaled_ready(s, spec, d_left, d_right, d_disp_full, &c) || !samples_aligned(&c, d_left, d_right)) return false;
    if ((uintptr_t)d_disp_full & 3u) FAIL("the map of sgm_match_scaled_device must be 4-byte aligned");
    if (!sgm_match_wait(s)) return false;                        /* an earlier host-pointer match still copies out of d_disp */
    return scaled_queue(s, &c, d_left, d_right, d_disp_full);
}

bool sgm_match_scaled(sgm_instance* s, const sgm_scale_spec* spec, const uint8_t* img_left, const uint8_t* img_right, float* disp_full)
{
    sgmd_scale c;
    if (!scaled_ready(s, spec, img_left, img_right, disp_full, &c) || !sgm_match_wait(s)) return false;
    const size_t px = (size_t)c.B * c.W * c.H, img = px * (c.bits > 8 ? 2 : 1), map = px * sizeof(float);
    const bool pin_l = sgmd_host_is_pinned(s->device, img_left, img) != 0, pin_r = sgmd_host_is_pinned(s->device, img_right, img) != 0;
    const bool pin_out = sgmd_host_is_pinned(s->device, disp_full, map) != 0;
    const buf_request bufs[] = {{&s->d_sc_full_l, img, 0}, {&s->d_sc_full_r, img, 0}, {&s->d_sc_disp, map, 0},
                                {&s->h_sc_l, pin_l ? 0 : img, BUF_PINNED}, {&s->h_sc_r, pin_r ? 0 : img, BUF_PINNED},
                                {&s->h_sc_disp, pin_out ? 0 : map, BUF_PINNED}};
    int n = 0;
    buf_request need[6];
    for (int i = 0; i < 6; ++i)
        if (bufs[i].bytes) need[n++] = bufs[i];
    if (!reserve_all(s, need, n, 0)) FAIL("allocation failed for the scaled match of %d frames of %dx%d", c.B, c.W, c.H);
    void* back = pin_out ? (void*)disp_full : s->h_sc_disp.p;
    const bool ok = upload(s, s->d_sc_full_l.p, img_left, s->h_sc_l.p, img) && upload(s, s->d_sc_full_r.p, img_right, s->h_sc_r.p, img) &&
                    scaled_queue(s, &c, s->d_sc_full_l.p, s->d_sc_full_r.p, s->d_sc_disp.p) &&
                    sgmd_d2h_async(s->device, s->stream, back, s->d_sc_disp.p, map) == 0;
    /* also after a failure: queued copies may still read the caller's / the staging buffers */
    if (!sgm_synchronize(s) || !ok) return false;
    if (!pin_out) memcpy(disp_full, back, map);
    return true;
}

/* ------------------------------------------------------------------ temporal filter of any maps (extension) */

bool sgm_temporal_filter(sgm_instance* s, const sgm_temporal_spec* spec, size_t streams, size_t steps, size_t pixels, float* d_maps,
                         const uint16_t* d_conf, float* d_hist_value, uint8_t* d_hist_bits, uint32_t* d_stats)
{
    sgmd_temporal_params c;
    if (!s || !spec || !d_maps || !d_hist_value || !d_hist_bits) FAIL("sgm_temporal_filter was given a NULL pointer");
    if (!temporal_available()) FAIL("the temporal filter is not part of this build");
    if (!temporal_spec_valid(spec, false, &c)) FAIL("the temporal spec is outside its ranges (include/sgm_mi355x.h, sgm_temporal_spec)");
    if (!temporal_geometry_ok(streams, steps, pixels))
        FAIL("sgm_temporal_filter: streams, steps and pixels must be at least 1 and their product at most 2^31");
    if (!aligned_to(d_maps, 4) || !aligned_to(d_hist_value, 4) || !aligned_to(d_stats, 4) || !aligned_to(d_conf, 2))
        FAIL("the maps, history values and counters of sgm_temporal_filter must be 4-byte aligned, the confidence 2-byte aligned");
    /* (the scratch is shared with the matches' filter, which a later match queues behind everything queued here) */
    if (!scratch_then_wait(s, d_stats ? &s->d_tp_scratch : NULL, d_stats ? sgmd_temporal_scratch_bytes() : 0, "the counters' scratch"))
        return false;
    if (sgmd_temporal(s->device, s->stream, &c, streams, steps, pixels, d_maps, d_conf, d_hist_value, d_hist_bits, d_stats,
                      d_stats ? s->d_tp_scratch.p : NULL) != 0)
        FAIL("a kernel launch failed");
    return true;
}

bool sgm_temporal_clear(sgm_instance* s, size_t streams, size_t pixels, float* d_hist_value, uint8_t* d_hist_bits)
{
    if (!s || !d_hist_value || !d_hist_bits) FAIL("sgm_temporal_clear was given a NULL pointer");
    if (!temporal_available()) FAIL("the temporal filter is not part of this build");
    if (!temporal_geometry_ok(streams, 1, pixels)) FAIL("sgm_temporal_clear: streams and pixels must be at least 1 and their product at most 2^31");
    if ((uintptr_t)d_hist_value & 3u) FAIL("the history values of sgm_temporal_clear must be 4-byte aligned");
    if (sgmd_temporal_clear(s->device, s->stream, streams * pixels, d_hist_value, d_hist_bits) != 0) FAIL("a kernel launch failed");
    return true;
}

int sgm_temporal_stats(sgm_instance* s, uint32_t* out, int capacity)
{
    if (!s || !out || s->tp_stat_maps < 1 || capacity < s->tp_stat_maps || !s->d_tp_stats.p) return 0;
    const size_t bytes = (size_t)s->tp_stat_maps * 5 * sizeof(uint32_t);
    if (!sgm_match_wait(s) || sync_streams(s) != 0) return 0;
    if (sgmd_d2h_async(s->device, s->stream, out, s->d_tp_stats.p, bytes) != 0 || sync_streams(s) != 0) return 0;
    return s->tp_stat_maps;
}

/* ------------------------------------------------------------------ hole filling of any map (extension) */

bool sgm_fill_holes(sgm_instance* s, float* d_disp, const uint8_t* d_class)
{
    if (!s || !s->initialized || !d_disp) return false;
    if (!fill_available()) FAIL("hole filling is not part of this build");
    if (ensure_fill(s) != 0) return false;
    /* the ping-pong map may still be in use by the post pass of the last match on a stream of its own */
    if (wait_for_result(s, s->stream) != 0) return false;
    if (fill_passes(s, s->stream, d_disp, d_class) != 0) FAIL("a kernel launch failed");
    return true;
}

/* ------------------------------------------------------------------ refinement of any map (extension) */

bool sgm_refine_disparity(sgm_instance* s, float* d_disp, const uint16_t* d_conf, const uint8_t* d_guide)
{
    if (!s || !s->initialized || !d_disp || !d_conf || !d_guide) return false;
    if (!refine_available()) FAIL("the refinement is not part of this build");
    if (s->rf_req.iters < 1) FAIL("no refinement parameters: call sgm_set_refine first");
    if (ensure_refine(s) != 0) return false;
    /* U, V and Q may still be in use by the post pass of the last match on a stream of its own */
    if (wait_for_result(s, s->stream) != 0) return false;
    if (refine_passes(s, s->stream, d_disp, d_conf, d_guide, &s->rf_req) != 0) FAIL("a kernel launch failed");
    return true;
}

/* ------------------------------------------------------------------ a test-platform frame end to end (8f-2) */

bool sgm_gray_from_planes(sgm_instance* s, const uint8_t* d_bgr, size_t count, int weight_r, uint8_t* d_gray)
{
    if (!s || !d_bgr || !d_gray) return false;
    if (weight_r != 76 && weight_r != 77) FAIL("grey weight of red must be 76 (stereo_matching.c:18-25) or 77 (stb_image.h:1746-1749)");
    return sgmd_gray_planes(s->device, s->stream, d_bgr, count, weight_r, d_gray) == 0;
}

static int ensure_planes_io(sgm_instance* s)
{
    const size_t px = batch_px(s);
    const buf_request io[] = {{&s->d_bgr, 6 * px, 0}, {&s->d_depth, px * sizeof(float), 0}, {&s->h_bgr, 6 * px, BUF_PINNED}};
    return reserve_all(s, io, 3, 0) ? 0 : -1;
}

bool sgm_match_planes_async(sgm_instance* s, const uint8_t* planes, float fx, float baseline, float doffs, float* depth)
{
    if (!host_entry_ready(s, planes, planes, depth)) return false;
    if (wide_pixels(s)) FAIL("sgm_match_planes takes byte planes: not available with %d bits per sample (sgm_set_pixel_bits)", s->pixel_bits);
    if (ensure_planes_io(s) != 0) FAIL("device allocation failed for the colour planes of %dx%d", s->g.W, s->g.H);
    const int dev = s->device;
    const size_t fpx = frame_px(s), px = (size_t)s->g.B * fpx;
    host_out out = {depth, &s->h_disp, &s->d_depth, 0, px * sizeof(float), false};
    outputs_pinned(s, &out, 1);
    bool ok = upload(s, s->d_bgr.p, planes, s->h_bgr.p, 6 * px);
    for (int f = 0; ok && f < s->g.B; ++f) {                    /* frame f: left B G R, right B G R (server.py:105-131) */
        const char* fr = (const char*)s->d_bgr.p + (size_t)f * 6 * fpx;
        ok = sgmd_gray_planes(dev, s->stream, fr, fpx, 76, (char*)s->d_left.p + f * fpx) == 0 &&
             sgmd_gray_planes(dev, s->stream, fr + 3 * fpx, fpx, 76, (char*)s->d_right.p + f * fpx) == 0;
    }
    ok = ok && run_pipeline(s, s->d_left.p, s->d_right.p, s->d_disp.p, NULL, NULL);
    /* the depth conversion reads the map the next match's cost sum rewrites: "result done" moves behind it (not behind the copy) */
    ok = ok && sgmd_depth(dev, result_stream(s), s->d_disp.p, px, fx, baseline, doffs, s->d_depth.p) == 0 && rerecord_result_event(s) == 0;
    return queue_outputs(s, ok, &out, 1, false);                /* one copy: no chunk events of an earlier match to wait for */
}

bool sgm_match_planes(sgm_instance* s, const uint8_t* planes, float fx, float baseline, float doffs, float* depth)
{
    return sgm_match_planes_async(s, planes, fx, baseline, doffs, depth) && sgm_match_wait(s);
}

bool sgm_compare_depth(sgm_instance* s, const float* d_ground_truth, const float* d_test, size_t count, float abs_thresh,
                       double* rmse, double* bad_pixel_rate, uint64_t* n_valid)
{
    if (!s || !d_ground_truth || !d_test) return false;
    double sumsq = 0.0;
    unsigned long long n = 0, bad = 0;
    if (wait_for_result(s, s->stream) != 0) return false;
    if (sgmd_score(s->device, s->stream, d_ground_truth, d_test, count, abs_thresh, &sumsq, &n, &bad) != 0) return false;
    if (n_valid) *n_valid = n;
    /* depth_image.py:306-308: (nan, nan, 0) when no pixel is finite in both images */
    if (rmse) *rmse = n ? sqrt(sumsq / (double)n) : NAN;
    if (bad_pixel_rate) *bad_pixel_rate = n ? (double)bad / (double)n : NAN;
    return true;
}

/* ------------------------------------------------------------------ stage read-back */

static size_t compact_volume(const sgm_instance* s, const void* padded, size_t elem, void* out)
{
    const size_t px = frame_px(s);
    const char* src = (const char*)padded;
    char* dst = (char*)out;
    for (size_t p = 0; p < px; ++p)
        memcpy(dst + p * s->g.D * elem, src + p * s->g.Dp * elem, (size_t)s->g.D * elem);
    return px * s->g.D * elem;
}

/* The stages sgm_read_stage hands out (include/sgm_mi355x.h has the list): the instance's pointer to each, the size of an element,
 * the half of a buffer of two batches it sits in, whether it is a padded volume ([H][W][Dp], compacted to D on the way out), and what
 * has to hold for it to exist now.  Two rows with one id: whichever holds.  The direction planes (10 .. 17) are not in here. */
enum { HAS_KEPT = 1, HAS_FILL = 2, HAS_RECT = 4, HAS_BOTH = 8, HAS_BOTH_KEPT = 16, HAS_WIDE = 32, HAS_COST = 64, NOT_WIDE = 128, NOT_BOTH = 256,
       HAS_PIX16 = 512, NOT_PIX16 = 1024, HAS_TEMPORAL = 2048 };
#define AT(member) offsetof(struct sgm_instance, member)
static const struct { int id; size_t at; int elem, half; bool volume; int needs; } k_stages[] = {
    {0, AT(d_census64_l.p), 8, 0, false, HAS_WIDE},           {0, AT(d_census_l.p), 4, 0, false, NOT_WIDE},
    {1, AT(d_census64_r.p), 8, 0, false, HAS_WIDE},           {1, AT(d_census_r), 4, 0, false, NOT_WIDE},
    {2, AT(d_cost.p), 1, 0, true, HAS_WIDE | HAS_COST},       {2, AT(d_cost.p), 1, 0, true, HAS_KEPT | HAS_COST},
    {3, AT(d_S.p), 2, 0, true, 0},                            /* (materialised first) */
    {4, AT(d_snap_wta.p), 4, 0, false, HAS_KEPT},             {5, AT(d_disp_r.p), 4, 0, false, 0},
    {6, AT(d_snap_lr.p), 4, 0, false, HAS_KEPT},              {7, AT(d_snap_speckle.p), 4, 0, false, HAS_KEPT},
    {8, AT(d_both_maps.p), 4, 0, false, HAS_BOTH},            {8, AT(d_disp.p), 4, 0, false, NOT_BOTH},
    {9, AT(d_fill_map.p), 4, 0, false, HAS_KEPT | HAS_FILL},  {18, AT(d_fill_class.p), 1, 0, false, HAS_FILL},
    {19, AT(d_rect_l.p), 1, 0, false, HAS_RECT | NOT_PIX16},  {20, AT(d_rect_r.p), 1, 0, false, HAS_RECT | NOT_PIX16},
    /* more than 8 bits per sample: the rectified images are u16; the narrowed images the census wrote */
    {19, AT(d_rect_l.p), 2, 0, false, HAS_RECT | HAS_PIX16},  {20, AT(d_rect_r.p), 2, 0, false, HAS_RECT | HAS_PIX16},
    {21, AT(d_g8_l.p), 1, 0, false, HAS_PIX16},               {22, AT(d_g8_r.p), 1, 0, false, HAS_PIX16},
    /* sgm_match_both: the right view after the LR check, after speckle removal, and finished */
    {26, AT(d_both_snap.p), 4, 0, false, HAS_KEPT | HAS_BOTH_KEPT}, {27, AT(d_both_snap.p), 4, 1, false, HAS_KEPT | HAS_BOTH_KEPT},
    {28, AT(d_both_maps.p), 4, 1, false, HAS_BOTH},
    /* the temporal filter: the maps as they entered it (the right view's after a sgm_match_both); 30 / 31 / 33 / 34 are not in here */
    {29, AT(d_tp_pre.p), 4, 0, false, HAS_KEPT | HAS_TEMPORAL}, {32, AT(d_tp_pre.p), 4, 1, false, HAS_KEPT | HAS_TEMPORAL | HAS_BOTH},
};

size_t sgm_read_stage(sgm_instance* s, int which, void* host_out, size_t capacity)
{
    if (!s || !s->initialized || !host_out) return 0;
    const size_t px = frame_px(s), f = (size_t)s->read_frame;
    const char* src = NULL;
    size_t elem = 0;
    bool volume = false;
    int row_a = 0, row_b = s->g.H;                                /* rows the device holds of a volume stage */
    const int has = (s->keep_stages ? HAS_KEPT : 0) | (s->fill_on ? HAS_FILL : 0) | (s->rect_on ? HAS_RECT : 0) |
                    (s->last_both ? HAS_BOTH : NOT_BOTH) | (s->last_both_kept ? HAS_BOTH_KEPT : 0) |
                    (volume_fed(s) ? HAS_WIDE : NOT_WIDE) | (s->d_cost.p ? HAS_COST : 0) | (wide_pixels(s) ? HAS_PIX16 : NOT_PIX16) |
                    (s->temporal_on && s->tp_sig[0] ? HAS_TEMPORAL : 0);
    if (which == 3 && (ensure_S(s) != 0 || materialize_S(s) != 0)) return 0;
    for (size_t i = 0; !src && i < sizeof k_stages / sizeof k_stages[0]; ++i) {
        const char* base = *(char* const*)((const char*)s + k_stages[i].at);
        if (k_stages[i].id != which || (k_stages[i].needs & ~has) || !base) continue;
        elem = (size_t)k_stages[i].elem;
        volume = k_stages[i].volume;
        src = base + ((size_t)k_stages[i].half * s->g.B + f) * px * elem * (volume ? (size_t)s->g.Dp : 1);
    }
    if (which >= 10 && which < 10 + s->paths.ndirs) {
        /* frame-addressed base of the plane; only rows [plane_row_lo, plane_row_lo + plane_rows) have storage */
        src = (const char*)s->d_planes + (f * 8 + (size_t)(which - 10)) * s->plane_bytes;
        elem = 1; volume = true;
        row_a = s->plane_row_lo; row_b = s->plane_row_lo + s->plane_rows;
    }
    if ((which == 30 || which == 31 || which == 33 || which == 34) && s->temporal_on && s->tp_sig[0] == s->g.W && s->tp_sig[1] == s->g.H &&
        s->tp_sig[2] == s->g.B && s->d_tp_value.p && s->d_tp_bits.p && (which < 33 || s->tp_sig[4] == 2)) {
        /* the history of the selected frame's stream (sequence: the one stream), the right view's behind the left view's */
        const size_t streams = s->tp_sig[5] ? 1 : (size_t)s->g.B, at = ((which >= 33 ? streams : 0) + (s->tp_sig[5] ? 0 : f)) * px;
        const bool bits = which == 31 || which == 34;
        elem = bits ? 1 : 4;
        src = (bits ? (const char*)s->d_tp_bits.p : (const char*)s->d_tp_value.p) + at * elem;
    }
    if (!src) return 0;
    const size_t need = volume ? px * s->g.D * elem : px * elem;
    if (capacity < need) return 0;
    if (sync_streams(s) != 0) return 0;
    if (!volume) {
        if (sgmd_d2h_async(s->device, s->stream, host_out, src, need) != 0) return 0;
        if (sync_streams(s) != 0) return 0;
        return need;
    }
    const size_t row_bytes = (size_t)s->g.W * s->g.Dp * elem;
    void* tmp = calloc(px * s->g.Dp, elem);                       /* rows without storage read 0 */
    if (!tmp) return 0;
    size_t got = 0;
    if (sgmd_d2h_async(s->device, s->stream, (char*)tmp + (size_t)row_a * row_bytes, src + (size_t)row_a * row_bytes,
                       (size_t)(row_b - row_a) * row_bytes) == 0 &&
        sync_streams(s) == 0)
        got = compact_volume(s, tmp, elem, host_out);
    free(tmp);
    return got;
}

/* ------------------------------------------------------------------ the reference boundary */

static sgm_instance* g_default;
static int g_default_device = -1;
static int g_default_honor;

static int default_device(void)
{
    if (g_default_device >= 0) return g_default_device;
    const char* e = getenv("SGM_DEVICE");
    return (e && *e) ? atoi(e) : 0;
}

bool SGM_SetDevice(int device_ordinal)
{
    if (device_ordinal < 0) return false;
    if (g_default && g_default->device != device_ordinal) {
        sgm_destroy(g_default);
        g_default = NULL;
    }
    g_default_device = device_ordinal;
    return true;
}

static int g_default_census_w, g_default_census_h, g_default_census_kind, g_default_view, g_default_fill, g_default_pixel_bits;

bool SGM_SetPixelBits(int bits)
{
    if (!pixel_bits_ok(bits)) return false;
    g_default_pixel_bits = bits;
    return g_default ? sgm_set_pixel_bits(g_default, bits) : true;
}

bool SGM_SetFillHoles(int enable)
{
    if (enable && !fill_available()) FAIL("hole filling is not part of this build");
    g_default_fill = enable ? 1 : 0;
    return g_default ? sgm_set_fill_holes(g_default, enable) : true;
}

static struct { int enable, iters, keep_invalid; float lambda, sigma; } g_default_refine;

bool SGM_SetRefine(int enable, float lambda, float sigma, int iterations, int keep_invalid)
{
    if (enable != 0 && enable != 1) return false;
    if (enable) {
        if (!refine_available()) FAIL("the refinement is not part of this build");
        refine_params p;
        if (!refine_params_set(&p, lambda, sigma, iterations, keep_invalid)) return false;
    }
    if (g_default && !sgm_set_refine(g_default, enable, lambda, sigma, iterations, keep_invalid)) return false;
    g_default_refine.enable = enable;
    if (enable) {
        g_default_refine.lambda = lambda;
        g_default_refine.sigma = sigma;
        g_default_refine.iters = iterations;
        g_default_refine.keep_invalid = keep_invalid;
    }
    return true;
}

static struct { bool on; sgm_temporal_spec spec; } g_default_temporal;

bool SGM_SetTemporal(const sgm_temporal_spec* spec)
{
    if (spec && !temporal_spec_ok(spec)) return false;
    if (g_default && !sgm_set_temporal(g_default, spec)) return false;
    g_default_temporal.on = spec != NULL;
    if (spec) g_default_temporal.spec = *spec;
    return true;
}

bool SGM_TemporalRestart(void) { return g_default ? sgm_temporal_restart(g_default) : false; }
int SGM_TemporalStats(uint32_t* out, int capacity) { return g_default ? sgm_temporal_stats(g_default, out, capacity) : 0; }

/* the default instance's maps, quantised: kept across SGM_Shutdown, each default instance gets a copy */
static struct { int32_t* q; int w, h; } g_default_rect;

static bool default_rectify_install(void)
{
    int32_t* copy = NULL;
    if (g_default_rect.q) {
        const size_t bytes = 4 * SGMD_REMAP_PITCH((size_t)g_default_rect.w * g_default_rect.h) * sizeof(int32_t);
        copy = (int32_t*)malloc(bytes);
        if (!copy) FAIL("out of host memory");
        memcpy(copy, g_default_rect.q, bytes);
    }
    rectify_install(g_default, copy, g_default_rect.w, g_default_rect.h);
    return true;
}

bool SGM_SetRectify(int width, int height, const float* map_lx, const float* map_ly, const float* map_rx, const float* map_ry)
{
    int32_t* q = NULL;
    if (map_lx) {
        if (!rectify_available()) FAIL("the rectification is not part of this build");
        q = rectify_quantise(width, height, map_lx, map_ly, map_rx, map_ry);
        if (!q) return false;
    }
    free(g_default_rect.q);
    g_default_rect.q = q;
    g_default_rect.w = q ? width : 0;
    g_default_rect.h = q ? height : 0;
    return g_default ? default_rectify_install() : true;
}

bool SGM_SetCensusWindow(int width, int height)
{
    if (width < 1 || height < 1 || !(width & 1) || !(height & 1) || width * height > 64) return false;
    g_default_census_w = width; g_default_census_h = height;
    return g_default ? sgm_set_census_window(g_default, width, height) : true;
}

bool SGM_SetCensusKind(int kind)
{
    if (!census_kind_ok(kind)) return false;
    g_default_census_kind = kind;
    return g_default ? sgm_set_census_kind(g_default, kind) : true;
}

void SGM_SetReferenceView(int right)
{
    g_default_view = right ? 1 : 0;
    if (g_default) sgm_set_reference_view(g_default, right);
}

void SGM_SetHonorNumPaths(int honor)
{
    g_default_honor = honor;
    if (g_default) g_default->honor_num_paths = honor;
}

bool SGM_Initialize(uint16_t width, uint16_t height, const SGMOption* option)
{
    if (!option) return false;
    /* argument errors are reported exactly like the reference, before any device is touched */
    if (width == 0 || height == 0) { if (g_default) g_default->initialized = false; return false; }
    if (option->max_disparity <= option->min_disparity) { if (g_default) g_default->initialized = false; return false; }
    if (!g_default) {
        g_default = sgm_create(default_device());
        if (!g_default) return false;
        g_default->honor_num_paths = g_default_honor;
        g_default->reference_statics = 1;
        if (g_default_census_w) sgm_set_census_window(g_default, g_default_census_w, g_default_census_h);
        sgm_set_census_kind(g_default, g_default_census_kind);
        sgm_set_reference_view(g_default, g_default_view);
        if (g_default_pixel_bits) sgm_set_pixel_bits(g_default, g_default_pixel_bits);
        if (g_default_fill) sgm_set_fill_holes(g_default, 1);
        if (g_default_rect.q && !default_rectify_install()) return false;
        if (g_default_temporal.on) sgm_set_temporal(g_default, &g_default_temporal.spec);
        if (g_default_refine.enable)
            sgm_set_refine(g_default, 1, g_default_refine.lambda, g_default_refine.sigma, g_default_refine.iters,
                           g_default_refine.keep_invalid);
    }
    return sgm_initialize(g_default, width, height, option);
}

bool SGM_Reset(uint16_t width, uint16_t height, const SGMOption* option)
{
    if (g_default) g_default->initialized = false;               /* SemiGlobalMatching.c:130 */
    return SGM_Initialize(width, height, option);
}

bool SGM_Match(const uint8_t* img_left, const uint8_t* img_right, float* disp_left)
{
    if (!g_default) return false;
    return sgm_match(g_default, img_left, img_right, disp_left);
}

/* north_star's one-call form: SGM_Reset + SGM_Match (SemiGlobalMatching.c:128-132, 68-125; main.c:72,83) */
bool sgm_compute(const uint8_t* img_left, const uint8_t* img_right, uint16_t width, uint16_t height, const SGMOption* option,
                 float* disp_left)
{
    return SGM_Reset(width, height, option) && SGM_Match(img_left, img_right, disp_left);
}

bool SGM_MatchConfidence(const uint8_t* img_left, const uint8_t* img_right, float* disp_left, uint16_t* conf)
{
    if (!g_default) return false;
    return sgm_match_confidence(g_default, img_left, img_right, disp_left, conf);
}

bool SGM_MatchBoth(const uint8_t* img_left, const uint8_t* img_right, float* disp_left, float* disp_right)
{
    if (!g_default) return false;
    return sgm_match_both(g_default, img_left, img_right, disp_left, disp_right);
}

bool SGM_MatchDevice(const uint8_t* d_left, const uint8_t* d_right, float* d_disp_left)
{
    if (!g_default) return false;
    return sgm_match_device(g_default, d_left, d_right, d_disp_left);
}

bool SGM_Synchronize(void) { return g_default ? sgm_synchronize(g_default) : false; }

void SGM_Shutdown(void)
{
    sgm_destroy(g_default);
    g_default = NULL;
}

size_t SGM_ReadStage(int which, void* host_out, size_t capacity)
{
    return g_default ? sgm_read_stage(g_default, which, host_out, capacity) : 0;
}

bool SGM_ReadCloud(const sgm_cloud_spec* spec, sgm_point* points, size_t capacity, uint32_t* offsets)
{
    return g_default ? sgm_read_cloud(g_default, spec, points, capacity, offsets) : false;
}

bool SGM_MatchScaled(const sgm_scale_spec* spec, const uint8_t* img_left, const uint8_t* img_right, float* disp_full)
{
    return g_default ? sgm_match_scaled(g_default, spec, img_left, img_right, disp_full) : false;
}

void SGM_KeepStages(int enable)
{
    if (g_default) g_default->keep_stages = enable;
}

const char* SGM_Version(void) { return SGM_VERSION_STRING; }

/* ------------------------------------------------------------------ synthetic input */

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s; }

void SGM_SynthPair(int W, int H, int D, uint32_t seed, uint8_t* left, uint8_t* right)
{
    const size_t px = (size_t)W * H;
    uint8_t* noise = (uint8_t*)malloc(px);
    if (!noise) return;
    uint32_t st = seed;
    for (size_t i = 0; i < px; ++i) noise[i] = (uint8_t)(lcg(&st) >> 24);
    for (int y = 0; y < H; ++y) {
        const int yb = (y + 1 < H) ? y + 1 : H - 1;
        for (int x = 0; x < W; ++x) {
            const int xb = (x + 1 < W) ? x + 1 : W - 1;
            const unsigned sum = noise[(size_t)y * W + x] + noise[(size_t)y * W + xb] + noise[(size_t)yb * W + x] +
                                 noise[(size_t)yb * W + xb];
            left[(size_t)y * W + x] = (uint8_t)((sum + 2) >> 2);
        }
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int shift = D / 16 + ((5 * D / 8) * y) / H + 4 * ((x >> 6) & 1);
            int v = (x + shift < W) ? left[(size_t)y * W + x + shift] : (int)(lcg(&st) >> 24);
            v += (int)((lcg(&st) >> 24) & 3u) - 1;
            right[(size_t)y * W + x] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    free(noise);
}
