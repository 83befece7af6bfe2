/* sgm_calib.h -- the --rectify CALIB.txt of the drivers (sgm_main.c, sgm_stream.c).
 *
 * CALIB.txt is plain text, 64 numbers separated by white space: K (9, row-major), dist (5: k1 k2 p1 p2 k3), R (9), Knew (9) of
 * the left camera, then the same 32 of the right camera -- what OpenCV's stereoRectify returns, as sgm_rectify_maps takes it
 * (include/sgm_mi355x.h, SGM_SetRectify). */
#ifndef SGM_CALIB_H
#define SGM_CALIB_H

#include "../../include/sgm_mi355x.h"

#include <stdio.h>
#include <stdlib.h>

/* the 64 numbers of CALIB.txt; 0 with the reason on stderr */
static int sgm_calib_read(const char* path, double c[64])
{
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "%s: cannot open\n", path); return 0; }
    int n = 0;
    while (n < 64 && fscanf(f, "%lf", &c[n]) == 1) ++n;
    fclose(f);
    if (n != 64) { fprintf(stderr, "%s: 64 numbers wanted (K dist R Knew of the left camera, then of the right one), %d found\n", path, n); return 0; }
    return 1;
}

/* the four maps of a width x height frame as one malloc'ed block -- map_lx, map_ly, map_rx, map_ry, width * height floats each --
 * or NULL with the reason on stderr */
static float* sgm_calib_maps(const char* path, int width, int height)
{
    double c[64];
    if (!sgm_calib_read(path, c)) return NULL;
    const size_t px = (size_t)width * height;
    float* maps = (float*)malloc(4 * px * sizeof(float));
    if (!maps) return NULL;
    for (int cam = 0; cam < 2; ++cam) {
        const double* p = c + 32 * cam;
        if (!sgm_rectify_maps(p, p + 9, p + 14, p + 23, width, height, maps + 2 * cam * px, maps + (2 * cam + 1) * px)) {
            fprintf(stderr, "%s: the %s camera's Knew R is singular\n", path, cam ? "right" : "left");
            free(maps);
            return NULL;
        }
    }
    return maps;
}

#endif
