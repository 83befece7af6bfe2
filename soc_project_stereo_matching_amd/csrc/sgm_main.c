/* sgm_main.c -- command-line driver with the flow of the reference's desktop driver
 * (SemiGlobalMatching/SemiGlobalMatching/main.c:16-126): load a stereo pair as 8-bit grey, fill SGMOption with
 * the same defaults (main.c:48-65), SGM_Initialize + SGM_Match, normalise the valid disparities to 8 bit
 * exactly as main.c:92-117 and write the map.  Unlike the reference (paths hard-coded, argv ignored) the files
 * and options come from the command line.
 *
 *   sgm_main LEFT RIGHT OUT.png|OUT.pgm [--min-disparity N] [--max-disparity N] [--p1 N] [--p2 N]
 *            [--no-lr] [--lr-thres F] [--no-unique] [--unique-ratio F] [--no-speckle] [--speckle-area N]
 *            [--raw OUT.f32] [--repeat N] [--device N]
 *            [--paths 4|8] [--census WxH] [--right-reference]      extensions of the boundary: 4-path
 *            aggregation (the reference stores num_paths and ignores it), census windows other than 5x5, the right image
 *            as reference view; the defaults are the reference's behaviour
 *            [--census-kind centre|symmetric]   extension: the centre-symmetric census (SGM_SetCensusKind), on the fast path for
 *                             any window; symmetric without --census uses SGM_CENSUS_SYMMETRIC_DEFAULT_W x _H (7x7)
 *            [--fill-holes]   extension: occlusion-aware hole filling of the invalid disparities (SGM_SetFillHoles)
 *            [--confidence OUT.pgm]   extension: the matching confidence (SGM_MatchConfidence) as a 16-bit PGM
 *            [--right-out OUT.png] [--right-raw OUT.f32]   extension: the right view's map from the same match (SGM_MatchBoth),
 *                                     normalised / raw exactly like the left one; not with --confidence, --fill-holes, --refine,
 *                                     --right-reference (OUT is the left view's map)
 *            [--refine[=LAMBDA,SIGMA,ITERS]]   extension: confidence-guided edge-aware refinement of the map (SGM_SetRefine;
 *                             defaults SGM_REFINE_DEFAULT_*)
 *            [--rectify CALIB.txt]   extension: LEFT and RIGHT are raw camera images, rectified on the device ahead of the match
 *                             (SGM_SetRectify) through the maps of the 64 numbers in CALIB.txt (sgm_calib.h)
 *            [--rectified-out LEFT.pgm RIGHT.pgm]   with --rectify: the two rectified images the match ran on
 *            [--cloud OUT.ply --pinhole FX,FY,CX,CY,BASELINE,DOFFS [--cloud-z-max Z]]   extension: the valid pixels of OUT's map as
 *                             3-D points (SGM_ReadCloud), a binary little-endian PLY with x y z float and red green blue uchar,
 *                             the colour being the grey at the point's pixel of the image the map belongs to: LEFT (RIGHT with
 *                             --right-reference), the rectified one with --rectify
 *            [--register-raw OUT.f32 [--register-splat 1|2]]   extension: with --rectify and --pinhole (the rectified camera's:
 *                             Knew's focal lengths and principal point), the depth of OUT's map registered back into the raw
 *                             camera LEFT came from (RIGHT with --right-reference) -- sgm_register_depth into the target of
 *                             sgm_register_spec_raw -- as raw float32 [H][W] like --raw, NaN where nothing landed; splat 2 (default)
 *                             votes for the four raw pixels around a projection, 1 for the nearest.  --cloud-z-max cuts it too
 *            [--volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC --volume-ply OUT.ply]   extension: with --pinhole, OUT's map fused into a TSDF
 *                             volume of NX x NY x NZ voxels of edge VOXEL with its corner at (OX, OY, OZ) in the camera's frame
 *                             (units of BASELINE) and truncation distance TRUNC -- sgm_volume_integrate of the one frame with the
 *                             identity pose -- and the volume's surface points (sgm_volume_points, min_weight 1) as a PLY like
 *                             --cloud's, coloured with the grey at the pixel a point projects to.  --cloud-z-max cuts it too
 *            [--volume-mesh OUT.ply]   extension: with --volume, the volume as a triangle mesh (sgm_volume_mesh, marching tetrahedra,
 *                             the min_weight of --volume-ply): a binary little-endian PLY with the elements vertex (x y z float) and
 *                             face (a list of three vertex indices, uchar count and uint indices); prints the two counts
 *            [--volume-view ZMIN,ZMAX,STEP[,MINWEIGHT] [--volume-depth OUT.f32] [--volume-normals OUT.f32]]   extension: with
 *                             --volume, the volume rendered back into the frame's own camera after the frame is integrated
 *                             (sgm_volume_raycast: the --pinhole intrinsics, the identity pose, the image's size), marched at
 *                             Z = ZMIN + k * STEP up to ZMAX over voxels of weight MINWEIGHT (default 1) or more: the depth as raw
 *                             float32 [H][W] like --raw, the unit normals as raw float32 [H][W][3], NaN where no surface is met
 *            [--volume-color [--volume-image OUT.pgm]]   extension: with --volume, the frame fused with its own grey image (the one
 *                             --volume-ply takes its colours from) into a colour volume beside the TSDF words
 *                             (sgm_volume_integrate_color, channels 1); --volume-mesh then gains uchar red green blue per vertex
 *                             (sgm_volume_colors), and --volume-image, with --volume-view, writes the red channel of the coloured
 *                             ray-cast (sgm_volume_raycast_color) as a PGM, 0 where no surface is met.  Without it every output
 *                             file is what it was
 *            [--volume-window OX,OY,OZ,NX,NY,NZ]   extension: with --volume, after the frame is fused (and coloured) the volume is
 *                             replaced by the window of NX x NY x NZ voxels that starts OX,OY,OZ voxels into it (sgm_volume_window:
 *                             zero where the volume has nothing, the origin moved along); every --volume-* output is the window's
 *            [--volume-distance R[,UNKNOWN] --volume-field OUT.f32]   extension: with --volume, the signed distance field of the
 *                             fused volume (of the window, with --volume-window): sgm_volume_distance with radius R voxels on both
 *                             sides (min_weight 1, as --volume-ply; UNKNOWN 1 counts unobserved voxels as obstacles, default 0),
 *                             then sgm_volume_distance_field, written as raw float32, x fastest, behind 16 bytes of header: nx, ny,
 *                             nz as int32 and voxel as float32.  Without it every output file is what it was
 *            [--volume-objects MINVOXELS[,CONN[,CLEARANCE]]]   extension: with --volume, the objects of the fused volume (of the
 *                             window, with --volume-window): sgm_volume_components on the occupied voxels (min_weight 1, as
 *                             --volume-ply) with CONN 6 (default) or 26 neighbours, components below MINVOXELS voxels dropped.  With
 *                             --plane the plane it fits to the surface points is excluded first, with CLEARANCE (default 0, units of
 *                             BASELINE): the floor goes and what stands on it falls apart.  Prints the counts and one line per object
 *                             with its voxels, metric box and centroid (sgm_component_metric); --volume-mesh then gains one more
 *                             vertex property, uint object: 1 + the object's line, 0 for none (sgm_volume_component_of).  Without it
 *                             every output file and line is what it was
 *            [--volume-track ITER,DISTMAX[,TX,TY,TZ]]   extension: with --volume and --volume-view, the frame tracked against that
 *                             render (sgm_track: ITER rounds, gate DISTMAX, span the middle of the march (ZMIN + ZMAX) / 2, at least
 *                             6 pixels, pivots above 1e-6) from the identity displaced by the translation TX,TY,TZ (default 0,0,0);
 *                             prints the status, the associated pixels, the rms and the estimated pose source -> model camera, and
 *                             the world -> camera pose sgm_track_world_pose makes of it
 *            [--plane K,DIST[,SEED[,AX,AY,AZ,MINCOS]] [--plane-labels OUT.pgm]]   extension: with --pinhole, the dominant plane of the
 *                             frame's cloud list (SGM_ReadCloud's records; --cloud-z-max cuts it too) or, with --volume, of the
 *                             volume's surface points: sgm_plane_fit with K candidates, half-thickness DIST, the hash seed SEED
 *                             (default 0), the orientation prior AX,AY,AZ with MINCOS (default none), 4 rounds, at least 3 inliers,
 *                             pivots above 1e-9, span a quarter of the largest finite |coordinate| of the list; prints the status,
 *                             the inliers, the rms, the normal and the offset.  --plane-labels (not with --volume) writes a PGM of
 *                             the image's size, 255 at the cloud pixels sgm_plane_label marks as the plane's.  Without --plane every
 *                             output file and line is what it was
 *            [--bits N]       extension: images of N = 9..16 bits per sample (SGM_SetPixelBits): LEFT and RIGHT are loaded with
 *                             sgm_load_gray16 (binary PGM with maxval up to 65535, PNG grey of depth 16; 8-bit files are widened
 *                             unshifted) and matched on all their bits.  --bits 0: the smallest N >= 8 that holds the files' maxval.
 *                             Default 8, which refuses a 16-bit file.  With --bits above 8, --rectified-out writes 16-bit PGMs and
 *                             the cloud's colour is the narrowed image's
 *            [--scale F [--scale-radius R] [--scale-penalty P]]   extension: match at 1/F scale (F = 2 or 4) and bring the map back
 *                             to the full grid with the re-search on the full-resolution census (SGM_MatchScaled; R and P default to
 *                             SGM_SCALE_DEFAULT_RADIUS / _PENALTY, R < 0: the guided upscale alone).  --min-disparity and
 *                             --max-disparity stay in full-resolution pixels: the match runs at W / F x H / F with min / F (floor)
 *                             and max / F (ceil).  OUT and --raw are the full-resolution map.  Not with --cloud, --confidence,
 *                             --right-out / --right-raw or --rectify
 *   sgm_main --convert IN OUT.png        (image I/O only, no GPU: used by the CPU tests)
 *   sgm_main --convert16 IN OUT.pgm      (the same through sgm_load_gray16 and the 16-bit PGM writer; prints the file's maxval)
 */
#define _POSIX_C_SOURCE 200809L
#include "../../include/sgm_mi355x.h"
#include "sgm_calib.h"
#include "sgm_image_io.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static double now_ms(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

static int ends_with(const char* s, const char* suf)
{
    const size_t n = strlen(s), m = strlen(suf);
    return n >= m && !strcmp(s + n - m, suf);
}

/* main.c:92-117: the map normalised to 8 bits over its valid range (invalid = 0) as PNG / PGM, and, raw != NULL, its float32
 * values as they are; either path may be NULL */
static int write_map(const float* disp, int w, int h, const char* image, const char* raw)
{
    const size_t px = (size_t)w * h;
    float lo = (float)w, hi = -(float)w;
    size_t valid = 0;
    for (size_t i = 0; i < px; ++i)
        if (disp[i] != INFINITY) {
            if (disp[i] < lo) lo = disp[i];
            if (disp[i] > hi) hi = disp[i];
            ++valid;
        }
    const float range = (hi - lo) != 0.0f ? (hi - lo) : 1.0f;
    uint8_t* u8 = (uint8_t*)malloc(px);
    if (!u8) return -1;
    for (size_t i = 0; i < px; ++i) {
        if (disp[i] == INFINITY) { u8[i] = 0; continue; }
        float v = (disp[i] - lo) / range * 255.0f;
        if (v < 0) v = 0;
        if (v > 255) v = 255;
        u8[i] = (unsigned char)v;
    }
    printf("valid %zu of %zu, disparity range [%g, %g]\n", valid, px, lo, hi);
    int rc = 0;
    if (image) rc = ends_with(image, ".pgm") ? sgm_write_pgm(image, u8, w, h) : sgm_write_png_gray(image, u8, w, h);
    if (raw) {
        FILE* f = fopen(raw, "wb");
        if (!f || fwrite(disp, sizeof(float), px, f) != px) rc = -1;
        if (f) fclose(f);
    }
    free(u8);
    return rc;
}

/* the point list as a binary little-endian PLY: x y z float, red green blue uchar = the grey image's value at the point's pixel */
static int write_ply(const char* path, const sgm_point* pts, size_t n, const uint8_t* gray, int w)
{
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n", n);
    int rc = 0;
    for (size_t i = 0; i < n && rc == 0; ++i) {
        unsigned char rec[15];
        const uint8_t g = gray[(size_t)(pts[i].pixel >> 16) * w + (pts[i].pixel & 0xFFFFu)];
        memcpy(rec, &pts[i], 12);                                 /* (the hosts this builds for are little-endian) */
        rec[12] = rec[13] = rec[14] = g;
        if (fwrite(rec, 1, sizeof rec, f) != sizeof rec) rc = -1;
    }
    if (fclose(f) != 0) rc = -1;
    return rc;
}

/* --register-raw: the depth of the map registered into the raw camera of the reference view, as raw float32.  The entry points
 * take device pointers on an explicit instance: the map and the result go through page-locked buffers of an instance of their own,
 * which the device reads and writes in place. */
static int register_raw(const char* path, const char* calib_path, int right_ref, int device, int w, int h, const float* pinhole,
                        float z_max, int splat, const float* disp)
{
    double c[64];
    if (!sgm_calib_read(calib_path, c)) return -1;
    const double* cam = c + (right_ref ? 32 : 0);                 /* K (9), dist (5), R (9), Knew (9) */
    sgm_register_spec dst;
    if (!sgm_register_spec_raw(cam, cam + 9, cam + 14, w, h, splat, &dst)) return -1;
    const sgm_cloud_spec src = {w, h, 1, pinhole[0], pinhole[1], pinhole[2], pinhole[3], pinhole[4], pinhole[5], 0.0f, z_max, 0};
    if (device < 0) {
        const char* e = getenv("SGM_DEVICE");
        device = (e && *e) ? atoi(e) : 0;
    }
    sgm_instance* s = sgm_create(device);
    if (!s) return -1;
    const size_t px = (size_t)w * h;
    float* d_disp = (float*)sgm_host_alloc(s, px * sizeof(float));
    float* d_depth = (float*)sgm_host_alloc(s, px * sizeof(float));
    int rc = -1;
    if (d_disp && d_depth) {
        memcpy(d_disp, disp, px * sizeof(float));
        if (sgm_register_depth(s, &src, &dst, d_disp, NULL, NULL, d_depth, NULL) && sgm_synchronize(s)) {
            size_t landed = 0;
            for (size_t i = 0; i < px; ++i) landed += d_depth[i] == d_depth[i];
            printf("registered: %zu of %zu raw pixels, splat %d\n", landed, px, splat);
            FILE* f = fopen(path, "wb");
            rc = (f && fwrite(d_depth, sizeof(float), px, f) == px) ? 0 : -1;
            if (f && fclose(f) != 0) rc = -1;
        }
    }
    sgm_host_free(s, d_disp);
    sgm_host_free(s, d_depth);
    sgm_destroy(s);
    return rc;
}

/* --volume-view: the march and where the maps go (a path that is NULL is not written) */
typedef struct {
    float z_min, z_max, step;
    uint32_t min_weight;
    const char* depth_path;
    const char* normals_path;
    int track_iterations;          /* --volume-track: 0 without it */
    float track_dist_max, track_t[3];
    const char* image_path;        /* --volume-image (with --volume-color) */
} volume_view;

static int write_floats(const char* path, const float* v, size_t n)
{
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    const size_t put = fwrite(v, sizeof(float), n, f);
    return (fclose(f) == 0 && put == n) ? 0 : -1;
}

/* --volume-track: the frame tracked against its own render, from the identity displaced by the given translation */
static int volume_track(sgm_instance* s, const volume_view* view, const sgm_cloud_spec* src, const float* d_disp, const float* d_depth,
                        const float* d_normal)
{
    static const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const sgm_track_spec model = {src->width, src->height, src->fx, src->fy, src->cx, src->cy, view->track_dist_max,
                                  0.5f * (view->z_min + view->z_max), view->track_iterations, 6, 1e-6f};
    double pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, view->track_t[0], view->track_t[1], view->track_t[2]};
    sgm_track_stats stats;
    float world[12];
    if (!sgm_track(s, src, &model, pose, d_disp, NULL, NULL, d_depth, d_normal, &stats, NULL, NULL) ||
        !sgm_track_world_pose(identity, pose, world))
        return -1;
    printf("volume track: frame 0 status %d, %u pixels, rms %.17g\n", stats.status, stats.pixels, stats.rms);
    printf("volume track: pose");
    for (int i = 0; i < 12; ++i) printf(" %.17g", pose[i]);
    printf("\nvolume track: world pose");
    for (int i = 0; i < 12; ++i) printf(" %.9g", (double)world[i]);
    printf("\n");
    return 0;
}

/* the volume rendered into the frame's own camera with the identity pose, and the maps written; with --volume-track the frame
 * (src, d_disp) tracked against that render, which then has normals whether they are written or not.  d_colors != NULL
 * (--volume-color): the coloured ray-cast, whose red channel --volume-image writes as a PGM, 0 where the pixel is empty */
static int volume_render(sgm_instance* s, const sgm_volume_spec* vol, const volume_view* view, int w, int h, const float* pinhole,
                         const uint32_t* d_voxels, const uint32_t* d_colors, const sgm_cloud_spec* src, const float* d_disp)
{
    static const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const sgm_raycast_spec spec = {w, h, 1, pinhole[0], pinhole[1], pinhole[2], pinhole[3], view->z_min, view->z_max, view->step, view->min_weight};
    const size_t px = (size_t)w * h;
    float* d_depth = (float*)sgm_host_alloc(s, px * sizeof(float));
    const int normals = view->normals_path || view->track_iterations;
    float* d_normal = normals ? (float*)sgm_host_alloc(s, 3 * px * sizeof(float)) : NULL;
    uint32_t* d_rgba = d_colors ? (uint32_t*)sgm_host_alloc(s, px * sizeof(uint32_t)) : NULL;
    int rc = -1;
    if (d_depth && (d_normal || !normals) && (d_rgba || !d_colors) &&
        (d_colors ? sgm_volume_raycast_color(s, vol, &spec, identity, d_voxels, d_colors, d_depth, d_normal, d_rgba)
                  : sgm_volume_raycast(s, vol, &spec, identity, d_voxels, d_depth, d_normal)) &&
        sgm_synchronize(s)) {
        size_t hits = 0;
        for (size_t i = 0; i < px; ++i) hits += d_depth[i] == d_depth[i];
        printf("volume view: %zu of %zu pixels meet the surface\n", hits, px);
        rc = 0;
        if (view->depth_path && write_floats(view->depth_path, d_depth, px) != 0) rc = -1;
        if (view->normals_path && write_floats(view->normals_path, d_normal, 3 * px) != 0) rc = -1;
        if (view->image_path) {
            uint8_t* red = (uint8_t*)malloc(px);
            for (size_t i = 0; red && i < px; ++i) red[i] = (uint8_t)(d_rgba[i] & 0xFFu);
            if (!red || sgm_write_pgm(view->image_path, red, w, h) != 0) rc = -1;
            free(red);
        }
        if (rc == 0 && view->track_iterations) rc = volume_track(s, view, src, d_disp, d_depth, d_normal);
    }
    sgm_host_free(s, d_depth);
    sgm_host_free(s, d_normal);
    sgm_host_free(s, d_rgba);
    return rc;
}

/* --volume-mesh: the volume as a triangle mesh, sized by a counts-only call, written as a binary little-endian PLY.  d_colors !=
 * NULL (--volume-color): sgm_volume_colors of the vertices, queued behind the mesh with its counts, as uchar red green blue */
typedef struct { uint32_t* d_labels; sgm_component* d_objects; size_t capacity; uint32_t* d_counts; } object_list;

static int volume_mesh_ply(sgm_instance* s, const sgm_volume_spec* vol, const uint32_t* d_voxels, const uint32_t* d_colors,
                           uint32_t min_weight, const object_list* objects, const char* path)
{
    uint32_t* d_index = NULL;
    uint32_t* d_counts = (uint32_t*)sgm_host_alloc(s, 2 * sizeof(uint32_t));
    sgm_mesh_vertex* d_vertices = NULL;
    sgm_mesh_triangle* d_triangles = NULL;
    uint32_t* d_rgba = NULL;
    int rc = -1;
    if (d_counts && sgm_volume_mesh(s, vol, d_voxels, min_weight, NULL, 0, NULL, 0, d_counts) && sgm_synchronize(s)) {
        const size_t nv = d_counts[0], nt = d_counts[1];
        d_vertices = nv ? (sgm_mesh_vertex*)sgm_host_alloc(s, nv * sizeof(sgm_mesh_vertex)) : NULL;
        d_triangles = nt ? (sgm_mesh_triangle*)sgm_host_alloc(s, nt * sizeof(sgm_mesh_triangle)) : NULL;
        d_rgba = (d_colors && nv) ? (uint32_t*)sgm_host_alloc(s, nv * sizeof(uint32_t)) : NULL;
        d_index = (objects && nv) ? (uint32_t*)sgm_host_alloc(s, nv * sizeof(uint32_t)) : NULL;
        if ((d_vertices || !nv) && (d_triangles || !nt) && (d_rgba || !d_colors || !nv) && (d_index || !objects || !nv) &&
            sgm_volume_mesh(s, vol, d_voxels, min_weight, d_vertices, nv, d_triangles, nt, d_counts) &&
            (!d_colors || sgm_volume_colors(s, vol, d_voxels, d_colors, d_vertices, nv, d_counts, 8, d_rgba)) &&
            (!objects || sgm_volume_component_of(s, vol, objects->d_labels, objects->d_objects, objects->capacity, objects->d_counts,
                                                 d_vertices, nv, d_counts, 8, d_index)) && sgm_synchronize(s) &&
            d_counts[0] == nv && d_counts[1] == nt) {
            printf("volume mesh: %zu vertices, %zu triangles\n", nv, nt);
            FILE* f = fopen(path, "wb");
            if (f) {
                fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n%s%s"
                           "element face %zu\nproperty list uchar uint vertex_indices\nend_header\n", nv,
                        d_colors ? "property uchar red\nproperty uchar green\nproperty uchar blue\n" : "", objects ? "property uint object\n" : "", nt);
                size_t put = 0;
                for (size_t i = 0; i < nv; ++i) {
                    const uint8_t rgb[3] = {(uint8_t)(d_colors ? d_rgba[i] : 0u), (uint8_t)(d_colors ? d_rgba[i] >> 8 : 0u),
                                            (uint8_t)(d_colors ? d_rgba[i] >> 16 : 0u)};
                    put += fwrite(&d_vertices[i], sizeof(float), 3, f) == 3 && (!d_colors || fwrite(rgb, 1, 3, f) == 3) &&
                           (!objects || fwrite(&d_index[i], sizeof(uint32_t), 1, f) == 1);
                }
                for (size_t i = 0; i < nt; ++i) put += fputc(3, f) == 3 && fwrite(d_triangles[i].v, sizeof(uint32_t), 3, f) == 3;
                rc = (fclose(f) == 0 && put == nv + nt) ? 0 : -1;
            }
        }
    }
    sgm_host_free(s, d_counts);
    sgm_host_free(s, d_vertices);
    sgm_host_free(s, d_triangles);
    sgm_host_free(s, d_rgba);
    sgm_host_free(s, d_index);
    return rc;
}

/* the spec of --plane for a list of n 16-byte records {x, y, z, tag}: K and SEED; opt: -, DIST, -, AX, AY, AZ, MINCOS; 4 rounds, at
 * least 3 inliers, pivots above 1e-9, span a quarter of the largest finite |coordinate| */
static sgm_plane_spec plane_spec_for(const void* records, size_t n, int k, uint32_t seed, const float* opt)
{
    float reach = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float* p = (const float*)records + 4 * i;
        for (int a = 0; a < 3; ++a)
            if (isfinite(p[a]) && fabsf(p[a]) > reach) reach = fabsf(p[a]);
    }
    const sgm_plane_spec spec = {k, seed, opt[1], {opt[3], opt[4], opt[5]}, opt[6], reach > 0.0f ? reach / 4.0f : 1.0f, 4, 3u, 1e-9f};
    return spec;
}

/* --volume-objects: MINVOXELS, CONN, CLEARANCE and, with --plane, what that option was given */
typedef struct { uint32_t min_voxels; int connectivity; float clearance; int have_plane, plane_k; uint32_t plane_seed; const float* plane_opt; } volume_objects;

/* The objects of the volume: the components of its occupied voxels (min_weight 1), with the plane of the n surface points at
 * d_points -- the plane --plane reports: the same records, the same spec -- excluded first where one was asked for and found; sized
 * by a counts-only call, printed one line each.  *list: the arrays the mesh looks its vertices up in, page-locked, the caller's to
 * free.  0 or -1 */
static int volume_objects_report(sgm_instance* s, const sgm_volume_spec* vol, const uint32_t* d_voxels, const volume_objects* o,
                                 const sgm_surface_point* d_points, size_t n, object_list* list)
{
    sgm_component_spec comp;
    memset(&comp, 0, sizeof comp);
    comp.min_weight = 1; comp.connectivity = o->connectivity; comp.min_voxels = o->min_voxels;
    if (o->have_plane) {
        const sgm_plane_spec spec = plane_spec_for(d_points, n, o->plane_k, o->plane_seed, o->plane_opt);
        sgm_plane plane;
        sgm_plane_stats stats;
        if (!sgm_plane_fit(s, &spec, d_points, n, NULL, NULL, &plane, &stats, NULL, NULL)) return -1;
        if (stats.status == 0) {
            comp.planes = 1;
            comp.plane[0] = plane;
            comp.clearance[0] = o->clearance;
        }
    }
    list->d_labels = (uint32_t*)sgm_host_alloc(s, sgm_volume_components_bytes(vol));
    list->d_counts = (uint32_t*)sgm_host_alloc(s, 2 * sizeof(uint32_t));
    list->d_objects = NULL;
    list->capacity = 0;
    if (!list->d_labels || !list->d_counts ||
        !sgm_volume_components(s, vol, &comp, d_voxels, list->d_labels, NULL, 0, list->d_counts) || !sgm_synchronize(s))
        return -1;
    const size_t count = list->d_counts[0];
    if (count) {
        list->d_objects = (sgm_component*)sgm_host_alloc(s, count * sizeof(sgm_component));
        list->capacity = count;
        if (!list->d_objects ||
            !sgm_volume_components(s, vol, &comp, d_voxels, list->d_labels, list->d_objects, count, list->d_counts) || !sgm_synchronize(s) ||
            list->d_counts[0] != count)
            return -1;
    }
    printf("volume objects: %zu of %u components have at least %u voxels (connectivity %d%s)\n", count, list->d_counts[1], o->min_voxels,
           o->connectivity, comp.planes ? ", the plane excluded" : o->have_plane ? ", no plane found" : "");
    for (size_t i = 0; i < count; ++i) {
        float lo[3], hi[3], c[3];
        sgm_component_metric(vol, &list->d_objects[i], lo, hi, c);
        printf("volume object %zu: %u voxels, box (%.9g, %.9g, %.9g) to (%.9g, %.9g, %.9g), centroid (%.9g, %.9g, %.9g)\n", i + 1,
               list->d_objects[i].voxels, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], c[0], c[1], c[2]);
    }
    return 0;
}

/* --volume-distance / --volume-field: both sides of the distance transform (min_weight 1, as the surface points), the signed field,
 * and the file: nx, ny, nz as int32 and voxel as float32, then the floats, x fastest.  distance: the radius, then unknown.  0 or -1 */
static int volume_field_file(sgm_instance* s, const sgm_volume_spec* vol, const uint32_t* d_voxels, const int32_t* distance, const char* path)
{
    const size_t n = sgm_volume_bytes(vol) / sizeof(uint32_t), half = sgm_volume_distance_bytes(vol);
    uint16_t* d_out2 = half ? (uint16_t*)sgm_host_alloc(s, half) : NULL;
    uint16_t* d_in2 = half ? (uint16_t*)sgm_host_alloc(s, half) : NULL;
    float* d_field = half ? (float*)sgm_host_alloc(s, n * sizeof(float)) : NULL;
    const sgm_distance_spec outside = {1, distance[0], 0, distance[1]}, inside = {1, distance[0], 1, distance[1]};
    int rc = -1;
    if (d_out2 && d_in2 && d_field && sgm_volume_distance(s, vol, &outside, d_voxels, d_out2) &&
        sgm_volume_distance(s, vol, &inside, d_voxels, d_in2) && sgm_volume_distance_field(s, vol, d_out2, d_in2, d_field) && sgm_synchronize(s)) {
        size_t obstacles = 0, near = 0;
        for (size_t i = 0; i < n; ++i) {
            obstacles += d_out2[i] == 0;
            near += d_out2[i] != 0 && d_out2[i] != SGM_DISTANCE_FAR;
        }
        printf("volume field: radius %d, unknown %d: %zu obstacle voxels, %zu within the radius\n", distance[0], distance[1], obstacles, near);
        const int32_t dims[3] = {vol->nx, vol->ny, vol->nz};
        FILE* f = fopen(path, "wb");
        if (f && fwrite(dims, sizeof dims, 1, f) == 1 && fwrite(&vol->voxel, sizeof(float), 1, f) == 1 && fwrite(d_field, sizeof(float), n, f) == n)
            rc = 0;
        if (f && fclose(f) != 0) rc = -1;
        if (rc != 0) fprintf(stderr, "cannot write %s\n", path);
    }
    sgm_host_free(s, d_out2);
    sgm_host_free(s, d_in2);
    sgm_host_free(s, d_field);
    return rc;
}

/* --volume: the map fused into a TSDF volume with the identity pose, and the surface points read back, as sgm_point records whose
 * pixel is the one the point projects to (clamped to the image), for write_ply; with view != NULL the volume rendered as well, with
 * mesh_path != NULL its mesh written there.  grey != NULL (--volume-color): the frame fused with that image, its own grey, into a
 * colour volume beside the TSDF words (sgm_volume_integrate_color, channels 1), which the render and the mesh then take.
 * window != NULL (--volume-window: offset, then dims): after the frame is fused the volume is replaced by that window of itself
 * (sgm_volume_window into a second allocation; the first is freed), and everything that is written is the window's.
 * distance != NULL (--volume-distance: the radius, then unknown): the signed distance field of that volume written to field_path.
 * objects != NULL (--volume-objects): the objects of that volume printed, ahead of the mesh, whose vertices then carry theirs.
 * Page-locked buffers of an instance of its own, as above.  *out: malloc'ed, *n records. */
static int volume_surface(const sgm_volume_spec* vol, const int32_t* window, const int32_t* distance, const char* field_path,
                          const volume_objects* objects, const volume_view* view, const char* mesh_path, const uint8_t* grey, int device, int w, int h, const float* pinhole, float z_max, const float* disp, sgm_point** out, size_t* n)
{
    const sgm_cloud_spec src = {w, h, 1, pinhole[0], pinhole[1], pinhole[2], pinhole[3], pinhole[4], pinhole[5], 0.0f, z_max, 0};
    static const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    size_t bytes = sgm_volume_bytes(vol);
    sgm_volume_spec windowed;
    if (!bytes) return -1;
    if (device < 0) {
        const char* e = getenv("SGM_DEVICE");
        device = (e && *e) ? atoi(e) : 0;
    }
    sgm_instance* s = sgm_create(device);
    if (!s) return -1;
    const size_t px = (size_t)w * h;
    float* d_disp = (float*)sgm_host_alloc(s, px * sizeof(float));
    uint32_t* d_voxels = (uint32_t*)sgm_host_alloc(s, bytes);
    uint32_t* d_count = (uint32_t*)sgm_host_alloc(s, sizeof(uint32_t));
    sgm_surface_point* d_points = NULL;
    uint8_t* d_image = grey ? (uint8_t*)sgm_host_alloc(s, px) : NULL;
    uint32_t* d_colors = grey ? (uint32_t*)sgm_host_alloc(s, bytes) : NULL;
    int rc = -1;
    *out = NULL;
    *n = 0;
    if (d_disp && d_voxels && d_count && (!grey || (d_image && d_colors))) {
        memcpy(d_disp, disp, px * sizeof(float));
        memset(d_voxels, 0, bytes);                               /* the empty volume */
        if (grey) {
            memcpy(d_image, grey, px);
            memset(d_colors, 0, bytes);                           /* no colour anywhere */
        }
        bool fused = grey ? sgm_volume_integrate_color(s, vol, &src, identity, d_disp, NULL, NULL, d_image, 1, d_voxels, d_colors)
                          : sgm_volume_integrate(s, vol, &src, identity, d_disp, NULL, NULL, d_voxels);
        if (fused && window) {                                    /* the volume becomes the window: a second allocation, the first freed */
            fused = sgm_volume_window_spec(vol, window, window + 3, &windowed);
            const size_t win_bytes = fused ? sgm_volume_bytes(&windowed) : 0;
            uint32_t* d_win = win_bytes ? (uint32_t*)sgm_host_alloc(s, win_bytes) : NULL;
            uint32_t* d_win_colors = (win_bytes && grey) ? (uint32_t*)sgm_host_alloc(s, win_bytes) : NULL;
            fused = fused && d_win && (d_win_colors || !grey) &&
                    sgm_volume_window(s, vol, window, window + 3, d_voxels, d_colors, d_win, d_win_colors, NULL) && sgm_synchronize(s);
            if (fused) {
                sgm_host_free(s, d_voxels);
                sgm_host_free(s, d_colors);
                d_voxels = d_win;
                d_colors = d_win_colors;
                vol = &windowed;
                bytes = win_bytes;
                printf("volume window: %d x %d x %d voxels from (%d, %d, %d), origin (%.9g, %.9g, %.9g)\n", windowed.nx, windowed.ny, windowed.nz,
                       window[0], window[1], window[2], windowed.origin[0], windowed.origin[1], windowed.origin[2]);
            } else {
                sgm_host_free(s, d_win);
                sgm_host_free(s, d_win_colors);
            }
        }
        if (fused && sgm_volume_points(s, vol, d_voxels, 1, NULL, 0, d_count) && sgm_synchronize(s)) {
            const size_t count = *d_count;
            size_t seen = 0;
            for (size_t i = 0; i < bytes / sizeof(uint32_t); ++i) seen += (d_voxels[i] >> 16) != 0;
            printf("volume: %zu of %zu voxels seen, %zu surface points\n", seen, bytes / sizeof(uint32_t), count);
            d_points = count ? (sgm_surface_point*)sgm_host_alloc(s, count * sizeof(sgm_surface_point)) : NULL;
            *out = (sgm_point*)malloc((count ? count : 1) * sizeof(sgm_point));
            if (*out && (!count || (d_points && sgm_volume_points(s, vol, d_voxels, 1, d_points, count, d_count) && sgm_synchronize(s)))) {
                for (size_t i = 0; i < count; ++i) {
                    const sgm_surface_point q = d_points[i];
                    float u = floorf(pinhole[0] * (q.x / q.z) + pinhole[2] + 0.5f), v = floorf(pinhole[1] * (q.y / q.z) + pinhole[3] + 0.5f);
                    u = u >= 0.0f ? (u < (float)w ? u : (float)(w - 1)) : 0.0f;          /* (a NaN lands on pixel 0) */
                    v = v >= 0.0f ? (v < (float)h ? v : (float)(h - 1)) : 0.0f;
                    (*out)[i] = (sgm_point){q.x, q.y, q.z, ((uint32_t)v << 16) | (uint32_t)u};
                }
                *n = count;
                rc = view ? volume_render(s, vol, view, w, h, pinhole, d_voxels, d_colors, &src, d_disp) : 0;
                object_list list = {NULL, NULL, 0, NULL};
                if (rc == 0 && objects) rc = volume_objects_report(s, vol, d_voxels, objects, d_points, count, &list);
                if (rc == 0 && mesh_path) rc = volume_mesh_ply(s, vol, d_voxels, d_colors, 1, objects ? &list : NULL, mesh_path);
                sgm_host_free(s, list.d_labels);
                sgm_host_free(s, list.d_objects);
                sgm_host_free(s, list.d_counts);
                if (rc == 0 && distance) rc = volume_field_file(s, vol, d_voxels, distance, field_path);
            }
        }
    }
    sgm_host_free(s, d_image);
    sgm_host_free(s, d_colors);
    sgm_host_free(s, d_disp);
    sgm_host_free(s, d_voxels);
    sgm_host_free(s, d_count);
    sgm_host_free(s, d_points);
    sgm_destroy(s);
    return rc;
}

/* --plane: the dominant plane of a list of n records (sgm_plane_fit) printed, and with labels_path (the records are the cloud's: the
 * tag names the pixel) the pixels sgm_plane_label marks written as a w x h PGM.  k, seed: K and SEED; opt: -, DIST, -, AX, AY, AZ, MINCOS.  An instance
 * and page-locked buffers of its own, as above. */
static int plane_report(int device, const sgm_point* pts, size_t n, int k, uint32_t seed, const float* opt, const char* labels_path, int w, int h)
{
    if (device < 0) {
        const char* e = getenv("SGM_DEVICE");
        device = (e && *e) ? atoi(e) : 0;
    }
    const sgm_plane_spec spec = plane_spec_for(pts, n, k, seed, opt);
    sgm_instance* s = sgm_create(device);
    if (!s) return -1;
    sgm_point* d_records = (sgm_point*)sgm_host_alloc(s, (n ? n : 1) * sizeof(sgm_point));
    uint8_t* d_labels = labels_path ? (uint8_t*)sgm_host_alloc(s, n ? n : 1) : NULL;
    sgm_plane* d_plane = labels_path ? (sgm_plane*)sgm_host_alloc(s, sizeof(sgm_plane)) : NULL;
    sgm_plane plane;
    sgm_plane_stats stats;
    int rc = -1;
    if (d_records && (!labels_path || (d_labels && d_plane))) {
        if (n) memcpy(d_records, pts, n * sizeof(sgm_point));
        if (sgm_plane_fit(s, &spec, d_records, n, NULL, NULL, &plane, &stats, NULL, NULL)) {
            printf("plane: status %d, %u inliers, rms %.9g, normal (%.9g, %.9g, %.9g), offset %.9g\n", stats.status, stats.inliers, stats.rms,
                   plane.normal[0], plane.normal[1], plane.normal[2], plane.offset);
            rc = 0;
            if (labels_path) {
                uint8_t* image = (uint8_t*)calloc((size_t)w * h, 1);
                memset(d_labels, 0, n ? n : 1);
                *d_plane = plane;
                rc = -1;
                if (image && sgm_plane_label(s, &spec, d_records, n, NULL, d_plane, 1, d_labels) && sgm_synchronize(s)) {
                    size_t marked = 0;
                    for (size_t i = 0; i < n; ++i) {
                        const uint32_t x = pts[i].pixel & 0xFFFFu, y = pts[i].pixel >> 16;
                        if (d_labels[i] && x < (uint32_t)w && y < (uint32_t)h) { image[(size_t)y * w + x] = 255; ++marked; }
                    }
                    printf("plane labels: %zu pixels\n", marked);
                    rc = sgm_write_pgm(labels_path, image, w, h) == 0 ? 0 : -1;
                }
                free(image);
            }
        }
    }
    sgm_host_free(s, d_records);
    sgm_host_free(s, d_labels);
    sgm_host_free(s, d_plane);
    sgm_destroy(s);
    return rc;
}

/* the 8-bit image the map's pixels are those of: the reference view's, as the match saw it (stage 19 / 20 with --rectify, the
 * narrowed image, stage 21 / 22, with more than 8 bits); *owned: what to free afterwards.  NULL: not available */
static const uint8_t* reference_grey(const uint8_t* left, const uint8_t* right, int right_ref, int rectified, int bits, size_t px,
                                     uint8_t** owned)
{
    *owned = NULL;
    if (!rectified && bits <= 8) return right_ref ? right : left;
    *owned = (uint8_t*)malloc(px);
    return (*owned && SGM_ReadStage((bits > 8 ? 21 : 19) + right_ref, *owned, px) == px) ? *owned : NULL;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "--convert")) {
        int w, h;
        uint8_t* g = sgm_load_gray(argv[2], &w, &h);
        if (!g) return 1;
        const int rc = ends_with(argv[3], ".pgm") ? sgm_write_pgm(argv[3], g, w, h) : sgm_write_png_gray(argv[3], g, w, h);
        free(g);
        return rc ? 1 : 0;
    }
    if (argc == 4 && !strcmp(argv[1], "--convert16")) {
        int w, h, maxval;
        uint16_t* g = sgm_load_gray16(argv[2], &w, &h, &maxval);
        if (!g) return 1;
        printf("w = %d, h = %d, maxval = %d\n", w, h, maxval);
        const int rc = sgm_write_pgm16(argv[3], g, w, h);
        free(g);
        return rc ? 1 : 0;
    }
    if (argc < 4) {
        fprintf(stderr, "usage: %s LEFT RIGHT OUT.png [options]   (see the header of sgm_main.c)\n", argv[0]);
        return 2;
    }
    SGMOption opt;
    memset(&opt, 0, sizeof opt);                       /* main.c:48-65 */
    opt.num_paths = 8;
    opt.min_disparity = 0;
    opt.max_disparity = 64;
    opt.is_check_lr = true;
    opt.lrcheck_thres = 1.0f;
    opt.is_check_unique = true;
    opt.uniqueness_ratio = 0.99;
    opt.is_remove_speckles = true;
    opt.min_speckle_area = 50;
    opt.p1 = 10;
    opt.p2_init = 150;
    const char* raw_path = NULL;
    const char* conf_path = NULL;
    const char* right_out = NULL;
    const char* right_raw = NULL;
    const char* calib_path = NULL;
    const char* rect_out[2] = {NULL, NULL};
    const char* cloud_path = NULL;
    float pinhole[6], cloud_z_max = INFINITY;
    int have_pinhole = 0;
    const char* register_path = NULL;
    const char* volume_path = NULL;
    const char* mesh_path = NULL;
    sgm_volume_spec volume = {0, 0, 0, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f, 65535};
    int have_volume = 0;
    volume_view view = {0.0f, 0.0f, 0.0f, 1, NULL, NULL, 0, 0.0f, {0.0f, 0.0f, 0.0f}, NULL};
    int have_track = 0, volume_color = 0;
    int32_t volume_window[6] = {0, 0, 0, 0, 0, 0};
    int have_window = 0;
    int32_t volume_distance[2] = {0, 0};
    float plane_opt[7] = {0, 0, 0, 0, 0, 0, 0};                   /* --plane: -, DIST, -, AX, AY, AZ, MINCOS */
    int plane_k = 0;
    uint32_t plane_seed = 0;
    int have_plane = 0;
    const char* plane_labels = NULL;
    int have_distance = 0;
    const char* field_path = NULL;
    volume_objects objects = {0, 6, 0.0f, 0, 0, 0, NULL};
    int have_objects = 0;
    int have_view = 0;
    int register_splat = 2, register_splat_set = 0;
    int repeat = 1, device = -1, census_w = 0, census_h = 0, right_ref = 0, fill_holes = 0, refine = 0;
    int census_kind = SGM_CENSUS_CENTRE, bits = 8;
    int scale = 0, scale_radius = SGM_SCALE_DEFAULT_RADIUS, scale_penalty = SGM_SCALE_DEFAULT_PENALTY, scale_tuned = 0;
    float refine_lambda = SGM_REFINE_DEFAULT_LAMBDA, refine_sigma = SGM_REFINE_DEFAULT_SIGMA;
    int refine_iters = SGM_REFINE_DEFAULT_ITERS;
    for (int i = 4; i < argc; ++i) {
        const char* a = argv[i];
        const char* v = (i + 1 < argc) ? argv[i + 1] : NULL;
        if (!strcmp(a, "--no-lr")) opt.is_check_lr = false;
        else if (!strcmp(a, "--no-unique")) opt.is_check_unique = false;
        else if (!strcmp(a, "--no-speckle")) opt.is_remove_speckles = false;
        else if (v && !strcmp(a, "--min-disparity")) { opt.min_disparity = (uint16_t)atoi(v); ++i; }
        else if (v && !strcmp(a, "--max-disparity")) { opt.max_disparity = (uint16_t)atoi(v); ++i; }
        else if (v && !strcmp(a, "--p1")) { opt.p1 = (int16_t)atoi(v); ++i; }
        else if (v && !strcmp(a, "--p2")) { opt.p2_init = (int16_t)atoi(v); ++i; }
        else if (v && !strcmp(a, "--lr-thres")) { opt.lrcheck_thres = (float)atof(v); ++i; }
        else if (v && !strcmp(a, "--unique-ratio")) { opt.uniqueness_ratio = (float)atof(v); ++i; }
        else if (v && !strcmp(a, "--speckle-area")) { opt.min_speckle_area = (uint16_t)atoi(v); ++i; }
        else if (v && !strcmp(a, "--raw")) { raw_path = v; ++i; }
        else if (v && !strcmp(a, "--confidence")) { conf_path = v; ++i; }
        else if (v && !strcmp(a, "--right-out")) { right_out = v; ++i; }
        else if (v && !strcmp(a, "--right-raw")) { right_raw = v; ++i; }
        else if (v && !strcmp(a, "--rectify")) { calib_path = v; ++i; }
        else if (i + 2 < argc && !strcmp(a, "--rectified-out")) { rect_out[0] = argv[i + 1]; rect_out[1] = argv[i + 2]; i += 2; }
        else if (v && !strcmp(a, "--cloud")) { cloud_path = v; ++i; }
        else if (v && !strcmp(a, "--pinhole")) {
            if (sscanf(v, "%f,%f,%f,%f,%f,%f", &pinhole[0], &pinhole[1], &pinhole[2], &pinhole[3], &pinhole[4], &pinhole[5]) != 6) {
                fprintf(stderr, "--pinhole wants FX,FY,CX,CY,BASELINE,DOFFS\n");
                return 2;
            }
            have_pinhole = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--cloud-z-max")) { cloud_z_max = (float)atof(v); ++i; }
        else if (v && !strcmp(a, "--register-raw")) { register_path = v; ++i; }
        else if (v && !strcmp(a, "--volume")) {
            if (sscanf(v, "%d,%d,%d,%f,%f,%f,%f,%f", &volume.nx, &volume.ny, &volume.nz, &volume.voxel, &volume.origin[0], &volume.origin[1],
                       &volume.origin[2], &volume.trunc) != 8) {
                fprintf(stderr, "--volume wants NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC\n");
                return 2;
            }
            have_volume = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--volume-ply")) { volume_path = v; ++i; }
        else if (v && !strcmp(a, "--volume-mesh")) { mesh_path = v; ++i; }
        else if (v && !strcmp(a, "--volume-view")) {
            const int got = sscanf(v, "%f,%f,%f,%u", &view.z_min, &view.z_max, &view.step, &view.min_weight);
            if (got != 3 && got != 4) { fprintf(stderr, "--volume-view wants ZMIN,ZMAX,STEP[,MINWEIGHT]\n"); return 2; }
            have_view = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--volume-depth")) { view.depth_path = v; ++i; }
        else if (v && !strcmp(a, "--volume-normals")) { view.normals_path = v; ++i; }
        else if (v && !strcmp(a, "--volume-image")) { view.image_path = v; ++i; }
        else if (!strcmp(a, "--volume-color")) volume_color = 1;
        else if (v && !strcmp(a, "--volume-window")) {
            if (sscanf(v, "%d,%d,%d,%d,%d,%d", &volume_window[0], &volume_window[1], &volume_window[2], &volume_window[3], &volume_window[4],
                       &volume_window[5]) != 6) {
                fprintf(stderr, "--volume-window wants OX,OY,OZ,NX,NY,NZ\n");
                return 2;
            }
            have_window = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--volume-distance")) {
            if (sscanf(v, "%d,%d", &volume_distance[0], &volume_distance[1]) < 1) {
                fprintf(stderr, "--volume-distance wants R[,UNKNOWN]\n");
                return 2;
            }
            have_distance = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--volume-field")) { field_path = v; ++i; }
        else if (v && !strcmp(a, "--volume-objects")) {
            long long m = 0;
            if (sscanf(v, "%lld,%d,%f", &m, &objects.connectivity, &objects.clearance) < 1 || m < 1 || m > 0xFFFFFFFFLL) {
                fprintf(stderr, "--volume-objects wants MINVOXELS[,CONN[,CLEARANCE]] with MINVOXELS >= 1\n");
                return 2;
            }
            objects.min_voxels = (uint32_t)m;
            have_objects = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--plane")) {
            int k = 0;
            long long seed = 0;                                   /* K and SEED are integers: 64.7 or a seed past 32 bits is refused, not rounded */
            int got = 0, used = -1;                               /* the fields of the form that takes the whole argument */
            if (sscanf(v, "%d,%f,%lld,%f,%f,%f,%f%n", &k, &plane_opt[1], &seed, &plane_opt[3], &plane_opt[4], &plane_opt[5], &plane_opt[6], &used) == 7 &&
                used >= 0 && v[used] == '\0')
                got = 7;
            else if (used = -1, sscanf(v, "%d,%f,%lld%n", &k, &plane_opt[1], &seed, &used) == 3 && used >= 0 && v[used] == '\0')
                got = 3;
            else if (used = -1, seed = 0, sscanf(v, "%d,%f%n", &k, &plane_opt[1], &used) == 2 && used >= 0 && v[used] == '\0')
                got = 2;
            if (got != 7) plane_opt[3] = plane_opt[4] = plane_opt[5] = plane_opt[6] = 0.0f;
            plane_k = k;
            plane_seed = (uint32_t)seed;
            if ((got != 2 && got != 3 && got != 7) || k < 1 || k > 1024 || seed < 0 || seed > 0xFFFFFFFFLL) {
                fprintf(stderr, "--plane wants K,DIST[,SEED[,AX,AY,AZ,MINCOS]] with integers K 1..1024 and SEED 0..2^32-1\n");
                return 2;
            }
            have_plane = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--plane-labels")) { plane_labels = v; ++i; }
        else if (v && !strcmp(a, "--volume-track")) {
            const int got = sscanf(v, "%d,%f,%f,%f,%f", &view.track_iterations, &view.track_dist_max, &view.track_t[0], &view.track_t[1],
                                   &view.track_t[2]);
            if ((got != 2 && got != 5) || view.track_iterations < 1) {
                fprintf(stderr, "--volume-track wants ITER,DISTMAX[,TX,TY,TZ] with ITER >= 1\n");
                return 2;
            }
            have_track = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--register-splat")) {
            if (strcmp(v, "1") && strcmp(v, "2")) { fprintf(stderr, "--register-splat wants 1 or 2\n"); return 2; }
            register_splat = atoi(v);
            register_splat_set = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--repeat")) { repeat = atoi(v); ++i; }
        else if (v && !strcmp(a, "--device")) { device = atoi(v); ++i; }
        else if (v && !strcmp(a, "--bits")) {
            bits = atoi(v);
            if (bits != 0 && (bits < 8 || bits > 16)) { fprintf(stderr, "--bits wants 8..16, or 0 for what the files hold\n"); return 2; }
            ++i;
        }
        else if (v && !strcmp(a, "--scale")) {
            scale = atoi(v);
            if (scale != 2 && scale != 4) { fprintf(stderr, "--scale wants 2 or 4\n"); return 2; }
            ++i;
        }
        else if (v && !strcmp(a, "--scale-radius")) { scale_radius = atoi(v); scale_tuned = 1; ++i; }
        else if (v && !strcmp(a, "--scale-penalty")) { scale_penalty = atoi(v); scale_tuned = 1; ++i; }
        else if (v && !strcmp(a, "--paths")) { opt.num_paths = (uint8_t)atoi(v); SGM_SetHonorNumPaths(1); ++i; }
        else if (v && !strcmp(a, "--census")) {
            if (sscanf(v, "%dx%d", &census_w, &census_h) != 2) { fprintf(stderr, "--census wants WxH, e.g. 7x7\n"); return 2; }
            ++i;
        }
        else if (v && !strcmp(a, "--census-kind")) {
            if (!strcmp(v, "symmetric")) census_kind = SGM_CENSUS_SYMMETRIC;
            else if (strcmp(v, "centre")) { fprintf(stderr, "--census-kind wants centre or symmetric\n"); return 2; }
            ++i;
        }
        else if (!strcmp(a, "--right-reference")) right_ref = 1;
        else if (!strcmp(a, "--fill-holes")) fill_holes = 1;
        else if (!strcmp(a, "--refine")) refine = 1;
        else if (!strncmp(a, "--refine=", 9)) {
            if (sscanf(a + 9, "%f,%f,%d", &refine_lambda, &refine_sigma, &refine_iters) != 3) {
                fprintf(stderr, "--refine= wants LAMBDA,SIGMA,ITERS, e.g. --refine=%g,%g,%d\n", SGM_REFINE_DEFAULT_LAMBDA,
                        SGM_REFINE_DEFAULT_SIGMA, SGM_REFINE_DEFAULT_ITERS);
                return 2;
            }
            refine = 1;
        }
        else { fprintf(stderr, "unknown option %s\n", a); return 2; }
    }
    if ((right_out || right_raw) && (conf_path || fill_holes || refine || right_ref)) {
        fprintf(stderr, "--right-out / --right-raw do not combine with --confidence, --fill-holes, --refine or --right-reference "
                        "(OUT would silently be the left map)\n");
        return 2;
    }
    if (have_volume != (volume_path != NULL)) { fprintf(stderr, "--volume and --volume-ply OUT.ply come together\n"); return 2; }
    if ((have_view || view.depth_path || view.normals_path) && !have_volume) {
        fprintf(stderr, "--volume-view, --volume-depth and --volume-normals need --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC\n");
        return 2;
    }
    if (mesh_path && !have_volume) { fprintf(stderr, "--volume-mesh needs --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC\n"); return 2; }
    if (have_track && (!have_volume || !have_view)) {
        fprintf(stderr, "--volume-track needs --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC and --volume-view ZMIN,ZMAX,STEP[,MINWEIGHT]\n");
        return 2;
    }
    if (volume_color && !have_volume) { fprintf(stderr, "--volume-color needs --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC\n"); return 2; }
    if (have_window && !have_volume) { fprintf(stderr, "--volume-window needs --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC\n"); return 2; }
    if ((have_distance || field_path) && !have_volume) { fprintf(stderr, "--volume-distance needs --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC\n"); return 2; }
    if (have_objects && !have_volume) { fprintf(stderr, "--volume-objects needs --volume NX,NY,NZ,VOXEL,OX,OY,OZ,TRUNC\n"); return 2; }
    if (have_distance != (field_path != NULL)) { fprintf(stderr, "--volume-distance and --volume-field OUT.f32 go together\n"); return 2; }
    if (view.image_path && (!have_view || !volume_color)) {
        fprintf(stderr, "--volume-image OUT.pgm needs --volume-view ZMIN,ZMAX,STEP[,MINWEIGHT] and --volume-color\n");
        return 2;
    }
    if (have_view != (view.depth_path || view.normals_path || have_track || view.image_path)) {
        fprintf(stderr, "--volume-view ZMIN,ZMAX,STEP[,MINWEIGHT] and --volume-depth / --volume-normals OUT.f32 come together\n");
        return 2;
    }
    if (have_plane && !have_pinhole) { fprintf(stderr, "--plane needs --pinhole FX,FY,CX,CY,BASELINE,DOFFS\n"); return 2; }
    if (plane_labels && (!have_plane || volume_path)) { fprintf(stderr, "--plane-labels OUT.pgm needs --plane and is the cloud's: not with --volume\n"); return 2; }
    if (have_plane && scale) { fprintf(stderr, "--scale does not combine with --plane\n"); return 2; }
    if (volume_path && !have_pinhole) { fprintf(stderr, "--volume needs --pinhole FX,FY,CX,CY,BASELINE,DOFFS\n"); return 2; }
    if (scale && volume_path) { fprintf(stderr, "--scale does not combine with --volume\n"); return 2; }
    if (scale && register_path) { fprintf(stderr, "--scale does not combine with --register-raw (it needs --rectify)\n"); return 2; }
    if (scale && (cloud_path || conf_path || right_out || right_raw || calib_path)) {
        fprintf(stderr, "--scale does not combine with --cloud, --confidence, --right-out / --right-raw or --rectify "
                        "(they work on the low-resolution match)\n");
        return 2;
    }
    if (scale_tuned && !scale) { fprintf(stderr, "--scale-radius / --scale-penalty need --scale\n"); return 2; }
    if (scale && (scale_radius > 4 || scale_penalty < 0 || scale_penalty > 16)) {
        fprintf(stderr, "--scale-radius wants at most 4 (negative: no re-search), --scale-penalty 0..16\n");
        return 2;
    }
    if (rect_out[0] && !calib_path) { fprintf(stderr, "--rectified-out needs --rectify\n"); return 2; }
    if (cloud_path && !have_pinhole) { fprintf(stderr, "--cloud needs --pinhole FX,FY,CX,CY,BASELINE,DOFFS\n"); return 2; }
    if (register_path && !have_pinhole) { fprintf(stderr, "--register-raw needs --pinhole FX,FY,CX,CY,BASELINE,DOFFS\n"); return 2; }
    if (register_path && !calib_path) { fprintf(stderr, "--register-raw needs --rectify CALIB.txt\n"); return 2; }
    if (register_splat_set && !register_path) { fprintf(stderr, "--register-splat needs --register-raw\n"); return 2; }

    int w1, h1, w2, h2;
    uint8_t *left = NULL, *right = NULL;                          /* the images as the library takes them: bytes, or uint16_t samples */
    if (bits == 8) {
        left = sgm_load_gray(argv[1], &w1, &h1);
        right = sgm_load_gray(argv[2], &w2, &h2);
    } else {
        int max1 = 0, max2 = 0;
        uint16_t* l16 = sgm_load_gray16(argv[1], &w1, &h1, &max1);
        uint16_t* r16 = sgm_load_gray16(argv[2], &w2, &h2, &max2);
        const int maxval = max1 > max2 ? max1 : max2;
        if (bits == 0)
            for (bits = 8; (1 << bits) <= maxval; ++bits) {}
        if (l16 && r16) printf("maxval %d, %d bits per sample\n", maxval, bits);
        if (l16 && r16 && bits > 8 && maxval >= (1 << bits)) printf("warning: samples of %d bits and more saturate the narrowed image\n", bits);
        if (l16 && r16 && bits == 8 && w1 == w2 && h1 == h2) {     /* --bits 0 on 8-bit files: the plain path */
            const size_t px = (size_t)w1 * h1;
            left = (uint8_t*)malloc(px);
            right = (uint8_t*)malloc(px);
            for (size_t i = 0; left && right && i < px; ++i) { left[i] = (uint8_t)l16[i]; right[i] = (uint8_t)r16[i]; }
            free(l16); free(r16);
        } else { left = (uint8_t*)l16; right = (uint8_t*)r16; }
    }
    if (!left || !right) { printf("Failed to load images\n"); return -1; }
    if (w1 != w2 || h1 != h2) { printf("Images must have same dimensions\n"); return -1; }
    if (w1 > 65535 || h1 > 65535) { printf("Image too large\n"); return -1; }
    printf("w = %d, h = %d, d = [%d,%d]\n", w1, h1, opt.min_disparity, opt.max_disparity);

    if (device >= 0) SGM_SetDevice(device);
    if (census_kind == SGM_CENSUS_SYMMETRIC && !census_w) {
        census_w = SGM_CENSUS_SYMMETRIC_DEFAULT_W;
        census_h = SGM_CENSUS_SYMMETRIC_DEFAULT_H;
    }
    if (!SGM_SetCensusKind(census_kind)) { printf("unsupported census kind\n"); return -2; }
    if (census_w && !SGM_SetCensusWindow(census_w, census_h)) { printf("unsupported census window %dx%d\n", census_w, census_h); return -2; }
    if (right_ref) SGM_SetReferenceView(1);
    if (!SGM_SetPixelBits(bits)) { printf("%d bits per sample are not available\n", bits); return -2; }
    if (fill_holes && !SGM_SetFillHoles(1)) { printf("hole filling unavailable\n"); return -2; }
    if (refine && !SGM_SetRefine(1, refine_lambda, refine_sigma, refine_iters, 0)) {
        printf("refinement unavailable or parameters out of range (%g, %g, %d)\n", refine_lambda, refine_sigma, refine_iters);
        return -2;
    }
    if (calib_path) {
        const size_t px = (size_t)w1 * h1;
        float* maps = sgm_calib_maps(calib_path, w1, h1);
        const bool ok = maps && SGM_SetRectify(w1, h1, maps, maps + px, maps + 2 * px, maps + 3 * px);
        free(maps);
        if (!ok) { printf("rectification unavailable or a bad calibration file\n"); return -2; }
    }
    /* --scale: the instance works at the low resolution, on the disparities of that resolution */
    int wm = w1, hm = h1;
    sgm_scale_spec scale_spec = {w1, h1, 1, scale, bits, scale_radius, scale_penalty, 0, 65535};
    if (scale) {
        if (!sgm_scaled_shape(&scale_spec, &wm, &hm)) { printf("the images are too small for --scale %d\n", scale); return -2; }
        opt.min_disparity = (uint16_t)(opt.min_disparity / scale);
        opt.max_disparity = (uint16_t)((opt.max_disparity + scale - 1) / scale);
        printf("scale %d: matching %d x %d, d = [%d,%d], radius %d, penalty %d\n", scale, wm, hm, opt.min_disparity, opt.max_disparity,
               scale_radius, scale_penalty);
    }
    if (!SGM_Initialize((uint16_t)wm, (uint16_t)hm, &opt)) { printf("SGM initialization failed\n"); return -2; }
    float* disp = (float*)malloc(sizeof(float) * (size_t)w1 * h1);
    float* disp_r = (right_out || right_raw) ? (float*)malloc(sizeof(float) * (size_t)w1 * h1) : NULL;
    uint16_t* conf = conf_path ? (uint16_t*)malloc(sizeof(uint16_t) * (size_t)w1 * h1) : NULL;
    double best = 1e30;
    for (int r = 0; r < repeat; ++r) {
        const double t0 = now_ms();
        if (r > 0 && !SGM_Reset((uint16_t)wm, (uint16_t)hm, &opt)) { printf("SGM reset failed\n"); return -2; }
        const bool ok = scale ? SGM_MatchScaled(&scale_spec, left, right, disp)
                              : disp_r ? SGM_MatchBoth(left, right, disp, disp_r)
                                       : (conf ? SGM_MatchConfidence(left, right, disp, conf) : SGM_Match(left, right, disp));
        if (!ok) { printf("SGM matching failed\n"); return -2; }
        const double t = now_ms() - t0;
        if (t < best) best = t;
    }
    printf("SGM_Match (host images in, host disparity out): %.3f ms\n", best);

    int rc = write_map(disp, w1, h1, argv[3], raw_path);
    if (disp_r && write_map(disp_r, w1, h1, right_out, right_raw) != 0) rc = -1;
    if (conf_path && sgm_write_pgm16(conf_path, conf, w1, h1) != 0) rc = -1;
    for (int v = 0; v < 2 && rect_out[0]; ++v) {                  /* the images the match ran on: stages 19 / 20 */
        const size_t px = (size_t)w1 * h1, bytes = px * (bits > 8 ? 2 : 1);
        uint8_t* img = (uint8_t*)malloc(bytes);
        if (!img || SGM_ReadStage(19 + v, img, bytes) != bytes ||
            (bits > 8 ? sgm_write_pgm16(rect_out[v], (const uint16_t*)img, w1, h1) : sgm_write_pgm(rect_out[v], img, w1, h1)) != 0)
            rc = -1;
        free(img);
    }
    if (cloud_path) {                                             /* sized from a first call, which copies the offsets alone */
        const sgm_cloud_spec spec = {w1, h1, 1, pinhole[0], pinhole[1], pinhole[2], pinhole[3], pinhole[4], pinhole[5], 0.0f, cloud_z_max, 0};
        uint32_t offsets[2] = {0, 0};
        sgm_point* pts = NULL;
        bool ok = SGM_ReadCloud(&spec, NULL, 0, offsets);
        if (!ok && offsets[1] > 0) {
            pts = (sgm_point*)malloc(sizeof(sgm_point) * offsets[1]);
            ok = pts && SGM_ReadCloud(&spec, pts, offsets[1], offsets);
        }
        if (!ok) { printf("point cloud unavailable or --pinhole / --cloud-z-max out of range\n"); rc = -1; }
        else {
            printf("cloud: %u points\n", offsets[1]);
            uint8_t* rect = NULL;
            const uint8_t* grey = reference_grey(left, right, right_ref, calib_path != NULL, bits, (size_t)w1 * h1, &rect);
            if (!grey || write_ply(cloud_path, pts, offsets[1], grey, w1) != 0) rc = -1;
            free(rect);
        }
        free(pts);
    }
    if (have_plane && !volume_path) {                             /* the plane of the frame's cloud list */
        const sgm_cloud_spec spec = {w1, h1, 1, pinhole[0], pinhole[1], pinhole[2], pinhole[3], pinhole[4], pinhole[5], 0.0f, cloud_z_max, 0};
        uint32_t offsets[2] = {0, 0};
        sgm_point* pts = NULL;
        bool ok = SGM_ReadCloud(&spec, NULL, 0, offsets);
        if (!ok && offsets[1] > 0) {
            pts = (sgm_point*)malloc(sizeof(sgm_point) * offsets[1]);
            ok = pts && SGM_ReadCloud(&spec, pts, offsets[1], offsets);
        }
        if (!ok || plane_report(device, pts, offsets[1], plane_k, plane_seed, plane_opt, plane_labels, w1, h1) != 0) {
            printf("plane unavailable or --plane / --pinhole / --cloud-z-max out of range\n");
            rc = -1;
        }
        free(pts);
    }
    if (register_path && register_raw(register_path, calib_path, right_ref, device, w1, h1, pinhole, cloud_z_max, register_splat, disp) != 0) {
        printf("registration unavailable, a bad calibration file or --pinhole / --cloud-z-max out of range\n");
        rc = -1;
    }
    if (volume_path) {
        sgm_point* pts = NULL;
        size_t n = 0;
        uint8_t* rect = NULL;
        const uint8_t* grey = NULL;
        objects.have_plane = have_plane; objects.plane_k = plane_k; objects.plane_seed = plane_seed; objects.plane_opt = plane_opt;
        if (volume_color) grey = reference_grey(left, right, right_ref, calib_path != NULL, bits, (size_t)w1 * h1, &rect);
        if ((volume_color && !grey) ||
            volume_surface(&volume, have_window ? volume_window : NULL, have_distance ? volume_distance : NULL, field_path,
                           have_objects ? &objects : NULL, have_view ? &view : NULL, mesh_path, grey, device, w1, h1, pinhole, cloud_z_max, disp, &pts, &n) != 0) {
            printf("volume unavailable or --volume / --volume-window / --volume-distance / --volume-objects / --volume-view / --volume-mesh / --pinhole / --cloud-z-max out of range\n");
            rc = -1;
        } else {
            if (!grey) grey = reference_grey(left, right, right_ref, calib_path != NULL, bits, (size_t)w1 * h1, &rect);
            if (!grey || write_ply(volume_path, pts, n, grey, w1) != 0) rc = -1;
            if (have_plane && plane_report(device, pts, n, plane_k, plane_seed, plane_opt, NULL, w1, h1) != 0) {       /* the plane of the surface points */
                printf("plane unavailable or --plane out of range\n");
                rc = -1;
            }
        }
        free(rect);
        free(pts);
    }
    SGM_Shutdown();
    free(disp); free(disp_r); free(conf); free(left); free(right);
    return rc ? 1 : 0;
}
