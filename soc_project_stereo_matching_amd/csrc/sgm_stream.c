/* sgm_stream.c -- a C caller with a stream of frames: what the library's host-pointer boundary delivers without any Python in
 * the process.  The call site this stands for is the reference's intended one, a C loop around the matcher
 * (ZedBoard/Vitis/lwip_tcp_perf_client/src/stereo_matching.c:34-40; the contract of SemiGlobalMatching.c:77-78,122: borrowed host
 * images in, host floats out).
 *
 *   sgm_stream [--width W] [--height H] [--disparities D] [--batch B] [--instances N] [--seconds S] [--frames F] [--seed X]
 *              [--pageable] [--blocking] [--numa-node K] [--both] [--census WxH] [--census-kind centre|symmetric]
 *              [--temporal A,D,N,K]
 *
 *   default      N instances, one host thread each, batches of B frames through sgm_reset + sgm_match_async + sgm_match_wait on
 *                page-locked buffers (sgm_host_alloc) for S seconds: the pipelined throughput path (bench.py's headline, in C)
 *   --blocking   one thread, one frame per call through sgm_compute (SGM_Reset + SGM_Match) on malloc'd buffers: the reference
 *                contract as it stands
 *   --pageable   malloc'd caller buffers instead of page-locked ones (staged by the library)
 *   --both       every match returns both views' maps (sgm_match_both_async; not with --blocking); fps counts frames, each with
 *                two maps, and "hash_frame0_right" is the right view's hash beside the left one's
 *   --census WxH, --census-kind centre|symmetric   extensions: the census window (SGM_SetCensusWindow) and kind (SGM_SetCensusKind);
 *                symmetric without --census uses SGM_CENSUS_SYMMETRIC_DEFAULT_W x _H
 *   --rectify CALIB.txt   extension: the frames are raw camera images, rectified on the device ahead of every match (SGM_SetRectify)
 *                through the maps of the 64 numbers in CALIB.txt (sgm_calib.h)
 *   --temporal A,D,N,K   extension: the temporal filter (sgm_set_temporal) with alpha A, gate D and hold K of N; every instance is ONE
 *                stream whose consecutive frames are the frames of its batches (sequence = 1; not with --blocking).  After the
 *                untimed warm-up batch the worker calls sgm_temporal_restart, and the line gains "hash_temporal": the hash of the
 *                LAST frame of batch 0 the first time the timed loop computes it (with --instances 1: frame B - 1 filtered through
 *                frames 0 .. B - 2); "hash_frame0" is then taken at that moment too (frame 0 meets an empty history)
 *   --numa-node K  run (and allocate) on the CPUs of NUMA node K -- the node the GPU hangs off (/sys/bus/pci/devices/<bdf>/numa_node):
 *                the host threads spin in stream synchronisation and feed 11 GB/s over PCIe; bench.py pins itself the same way
 *
 * Frames are the synthetic pairs of SURVEY.md 8(d) (SGM_SynthPair, seed + frame index), F distinct ones cycled.  Prints one JSON
 * line: frames, seconds, fps, Mdisp/s and an FNV-1a hash of the disparity map of frame 0 (tests/test_gpu_stream_c.py compares
 * it with the oracle's map hashed the same way).
 */
#define _GNU_SOURCE
#include "../../include/sgm_mi355x.h"
#include "sgm_calib.h"

#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static double now_s(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + t.tv_nsec * 1e-9;
}

/* restrict the process to the CPUs of a NUMA node (best effort: false if sysfs does not list them) */
static int pin_to_node(int node)
{
    char path[96], buf[4096];
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f || !fgets(buf, sizeof buf, f)) { if (f) fclose(f); return 0; }
    fclose(f);
    cpu_set_t set;
    CPU_ZERO(&set);
    for (char* tok = strtok(buf, ",\n"); tok; tok = strtok(NULL, ",\n")) {
        int a = 0, b = 0;
        const int n = sscanf(tok, "%d-%d", &a, &b);
        if (n < 1) continue;
        if (n == 1) b = a;
        for (int c = a; c <= b && c < CPU_SETSIZE; ++c) CPU_SET(c, &set);
    }
    return sched_setaffinity(0, sizeof set, &set) == 0;
}

static unsigned long long fnv1a(const void* p, size_t n)
{
    const unsigned char* b = (const unsigned char*)p;
    unsigned long long h = 1469598103934665603ULL;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ULL; }
    return h;
}

typedef struct {
    int k, n_inst, W, H, B, n_batches, pageable, both, census_kind, census_w, census_h;
    const SGMOption* opt;
    const sgm_temporal_spec* temporal;   /* --temporal (NULL: none) */
    unsigned long long hash_t;   /* --temporal: hash of the last frame of batch 0, the first time this instance computed it (0: never) */
    const float* maps;           /* --rectify: map_lx, map_ly, map_rx, map_ry of W * H floats each (NULL: none) */
    uint8_t **L, **R;            /* [n_batches] batches of B frames, shared, read-only */
    volatile double stop_at;     /* set by main right after the start barrier */
    long batches_done;
    unsigned long long hash0;    /* hash of frame 0 of batch 0 as this instance computed it (0: never) */
    unsigned long long hash0_r;  /* --both: the same of the right view's map */
    int failed;
    pthread_barrier_t* start;
} worker;

static void* worker_main(void* p)
{
    worker* w = (worker*)p;
    const size_t px = (size_t)w->W * w->H;
    sgm_instance* s = sgm_create(0);
    float *out = NULL, *out_r = NULL;
    w->failed = 1;
    if (s && sgm_set_batch(s, w->B) && sgm_set_overlap_post(s, 1) && sgm_set_census_kind(s, w->census_kind) &&
        (!w->census_w || sgm_set_census_window(s, w->census_w, w->census_h)) && (!w->temporal || sgm_set_temporal(s, w->temporal)) &&
        (!w->maps || sgm_set_rectify(s, w->W, w->H, w->maps, w->maps + px, w->maps + 2 * px, w->maps + 3 * px)) && sgm_initialize(s, (uint16_t)w->W, (uint16_t)w->H, w->opt)) {
        out = w->pageable ? (float*)malloc(w->B * px * sizeof(float)) : (float*)sgm_host_alloc(s, w->B * px * sizeof(float));
        if (w->both) out_r = w->pageable ? (float*)malloc(w->B * px * sizeof(float)) : (float*)sgm_host_alloc(s, w->B * px * sizeof(float));
        w->failed = out == NULL || (w->both && out_r == NULL);
    }
    /* one untimed batch: first-use allocations */
#define QUEUE(i) (w->both ? sgm_match_both_async(s, w->L[i], w->R[i], out, out_r) : sgm_match_async(s, w->L[i], w->R[i], out))
    if (!w->failed) w->failed = !(QUEUE(0) && sgm_match_wait(s));
    if (!w->failed && w->temporal) w->failed = !sgm_temporal_restart(s);      /* the timed stream starts from an empty history */
    pthread_barrier_wait(w->start);
    for (long b = w->k; !w->failed && now_s() < w->stop_at; b += w->n_inst) {
        const int i = (int)(b % w->n_batches);
        if (!(sgm_reset(s, (uint16_t)w->W, (uint16_t)w->H, w->opt) && QUEUE(i) && sgm_match_wait(s))) {
            w->failed = 1;
            break;
        }
        if (w->temporal) {
            /* the maps depend on what the instance saw before: the first pass over batch 0 is the one that is defined */
            if (i == 0 && !w->hash_t) {
                w->hash0 = fnv1a(out, px * sizeof(float));
                w->hash_t = fnv1a(out + (size_t)(w->B - 1) * px, px * sizeof(float));
            }
            ++w->batches_done;
            continue;
        }
        if (i == 0) w->hash0 = fnv1a(out, px * sizeof(float));
        if (i == 0 && w->both) w->hash0_r = fnv1a(out_r, px * sizeof(float));
        ++w->batches_done;
    }
    if (s) {
        if (out && !w->pageable) sgm_host_free(s, out);
        else free(out);
        if (out_r && !w->pageable) sgm_host_free(s, out_r);
        else free(out_r);
        sgm_destroy(s);
    }
    return NULL;
}

int main(int argc, char** argv)
{
    int W = 1242, H = 375, D = 128, B = 8, N = 4, F = 32, pageable = 0, blocking = 0, node = -1, both = 0;
    int census_kind = SGM_CENSUS_CENTRE, census_w = 0, census_h = 0;
    double seconds = 2.0;
    unsigned seed = 0x5EED0002u;
    const char* calib_path = NULL;
    sgm_temporal_spec temporal;
    int use_temporal = 0;
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        const char* v = i + 1 < argc ? argv[i + 1] : NULL;
        if (!strcmp(a, "--pageable")) pageable = 1;
        else if (!strcmp(a, "--blocking")) blocking = 1;
        else if (!strcmp(a, "--both")) both = 1;
        else if (v && !strcmp(a, "--width")) W = atoi(argv[++i]);
        else if (v && !strcmp(a, "--height")) H = atoi(argv[++i]);
        else if (v && !strcmp(a, "--disparities")) D = atoi(argv[++i]);
        else if (v && !strcmp(a, "--batch")) B = atoi(argv[++i]);
        else if (v && !strcmp(a, "--instances")) N = atoi(argv[++i]);
        else if (v && !strcmp(a, "--frames")) F = atoi(argv[++i]);
        else if (v && !strcmp(a, "--seconds")) seconds = atof(argv[++i]);
        else if (v && !strcmp(a, "--numa-node")) node = atoi(argv[++i]);
        else if (v && !strcmp(a, "--seed")) seed = (unsigned)strtoul(argv[++i], NULL, 0);
        else if (v && !strcmp(a, "--rectify")) calib_path = argv[++i];
        else if (v && !strcmp(a, "--temporal")) {
            memset(&temporal, 0, sizeof temporal);
            if (sscanf(v, "%f,%f,%d,%d", &temporal.alpha, &temporal.delta, &temporal.hold_window, &temporal.hold_count) != 4) {
                fprintf(stderr, "sgm_stream: --temporal wants ALPHA,DELTA,WINDOW,COUNT, e.g. 0.4,1.0,3,2\n");
                return 2;
            }
            temporal.sequence = 1;
            use_temporal = 1;
            ++i;
        }
        else if (v && !strcmp(a, "--census")) {
            if (sscanf(v, "%dx%d", &census_w, &census_h) != 2) { fprintf(stderr, "sgm_stream: --census wants WxH, e.g. 7x7\n"); return 2; }
            ++i;
        }
        else if (v && !strcmp(a, "--census-kind")) {
            if (!strcmp(v, "symmetric")) census_kind = SGM_CENSUS_SYMMETRIC;
            else if (strcmp(v, "centre")) { fprintf(stderr, "sgm_stream: --census-kind wants centre or symmetric\n"); return 2; }
            ++i;
        }
        else { fprintf(stderr, "sgm_stream: unknown argument %s (see the header of sgm_stream.c)\n", a); return 2; }
    }
    if (W < 1 || H < 1 || D < 1 || B < 1 || N < 1 || N > 16 || F < 1 || (both && blocking) || (use_temporal && blocking)) return 2;
    if (census_kind == SGM_CENSUS_SYMMETRIC && !census_w) {
        census_w = SGM_CENSUS_SYMMETRIC_DEFAULT_W;
        census_h = SGM_CENSUS_SYMMETRIC_DEFAULT_H;
    }
    if (node >= 0 && !pin_to_node(node)) fprintf(stderr, "sgm_stream: could not pin to NUMA node %d (continuing unpinned)\n", node);
    SGMOption opt;
    memset(&opt, 0, sizeof opt);                       /* main.c:48-65 with max_disparity = D */
    opt.num_paths = 8; opt.min_disparity = 0; opt.max_disparity = (uint16_t)D;
    opt.is_check_lr = true; opt.lrcheck_thres = 1.0f; opt.is_check_unique = true; opt.uniqueness_ratio = 0.99;
    opt.is_remove_speckles = true; opt.min_speckle_area = 50; opt.p1 = 10; opt.p2_init = 150;
    const size_t px = (size_t)W * H;
    float* maps = calib_path ? sgm_calib_maps(calib_path, W, H) : NULL;
    if (calib_path && !maps) return 2;

    if (blocking) {
        if (maps && !SGM_SetRectify(W, H, maps, maps + px, maps + 2 * px, maps + 3 * px)) {
            fprintf(stderr, "sgm_stream: rectification unavailable\n");
            return 2;
        }
        if (!SGM_SetCensusKind(census_kind) || (census_w && !SGM_SetCensusWindow(census_w, census_h))) {
            fprintf(stderr, "sgm_stream: unsupported census %dx%d\n", census_w, census_h);
            return 2;
        }
        uint8_t* l = (uint8_t*)malloc(px * F);
        uint8_t* r = (uint8_t*)malloc(px * F);
        float* out = (float*)malloc(px * sizeof(float));
        if (!l || !r || !out) return 1;
        for (int f = 0; f < F; ++f) SGM_SynthPair(W, H, D, seed + (unsigned)f, l + px * f, r + px * f);
        unsigned long long hash0 = 0;
        for (int f = 0; f < 2; ++f)                    /* untimed: first-use allocations */
            if (!sgm_compute(l, r, (uint16_t)W, (uint16_t)H, &opt, out)) { fprintf(stderr, "sgm_stream: sgm_compute failed\n"); return 1; }
        hash0 = fnv1a(out, px * sizeof(float));
        long n = 0;
        const double t0 = now_s();
        while (now_s() - t0 < seconds) {
            const int f = (int)(n % F);
            if (!sgm_compute(l + px * f, r + px * f, (uint16_t)W, (uint16_t)H, &opt, out)) return 1;
            ++n;
        }
        const double el = now_s() - t0;
        printf("{\"mode\": \"blocking sgm_compute per frame, malloc'd buffers, one thread\", \"width\": %d, \"height\": %d, \"disparity_range\": %d, "
               "\"frames\": %ld, \"seconds\": %.4f, \"fps\": %.2f, \"ms_per_frame\": %.4f, \"mdisp_per_s\": %.1f, \"hash_frame0\": \"%016llx\"}\n",
               W, H, D, n, el, n / el, el / n * 1e3, (double)px * D * 8 * n / el / 1e6, hash0);
        SGM_Shutdown();
        free(l); free(r); free(out); free(maps);
        return 0;
    }

    /* the shared input batches: page-locked (one throw-away instance owns the allocation) or malloc'd */
    const int n_batches = (F + B - 1) / B;
    sgm_instance* owner = sgm_create(0);
    if (!owner) { fprintf(stderr, "sgm_stream: no usable GPU\n"); return 1; }
    uint8_t** L = (uint8_t**)calloc((size_t)n_batches, sizeof *L);
    uint8_t** R = (uint8_t**)calloc((size_t)n_batches, sizeof *R);
    for (int i = 0; i < n_batches; ++i) {
        L[i] = pageable ? (uint8_t*)malloc(px * B) : (uint8_t*)sgm_host_alloc(owner, px * B);
        R[i] = pageable ? (uint8_t*)malloc(px * B) : (uint8_t*)sgm_host_alloc(owner, px * B);
        if (!L[i] || !R[i]) { fprintf(stderr, "sgm_stream: out of host memory\n"); return 1; }
        for (int j = 0; j < B; ++j) SGM_SynthPair(W, H, D, seed + (unsigned)((i * B + j) % F), L[i] + px * j, R[i] + px * j);
    }
    pthread_barrier_t start;
    pthread_barrier_init(&start, NULL, (unsigned)N + 1);
    worker w[16];
    pthread_t th[16];
    memset(w, 0, sizeof w);
    for (int k = 0; k < N; ++k) {
        w[k] = (worker){k, N, W, H, B, n_batches, pageable, both, census_kind, census_w, census_h, &opt, use_temporal ? &temporal : NULL, 0,
                        maps, L, R, 1e300, 0, 0, 0, 0, &start};
        if (pthread_create(&th[k], NULL, worker_main, &w[k]) != 0) return 1;
    }
    /* every worker is set up (its warm-up batch included) when the barrier opens */
    pthread_barrier_wait(&start);
    const double t1 = now_s();
    for (int k = 0; k < N; ++k) w[k].stop_at = t1 + seconds;
    long batches = 0;
    int failed = 0;
    unsigned long long hash0 = 0, hash0_r = 0, hash_t = 0;
    for (int k = 0; k < N; ++k) {
        pthread_join(th[k], NULL);
        batches += w[k].batches_done;
        failed |= w[k].failed;
        if (use_temporal) {
            /* every instance is a stream of its own with a history of its own: the one that ran batch 0 first speaks */
            if (k == 0) { hash0 = w[k].hash0; hash_t = w[k].hash_t; }
            continue;
        }
        if (w[k].hash0) {
            if (hash0 && hash0 != w[k].hash0) failed = 1;      /* every instance must compute the same map for the same frame */
            hash0 = w[k].hash0;
        }
        if (w[k].hash0_r) {
            if (hash0_r && hash0_r != w[k].hash0_r) failed = 1;
            hash0_r = w[k].hash0_r;
        }
    }
    const double el = now_s() - t1;
    for (int i = 0; i < n_batches; ++i) {
        if (pageable) { free(L[i]); free(R[i]); }
        else { sgm_host_free(owner, L[i]); sgm_host_free(owner, R[i]); }
    }
    sgm_destroy(owner);
    free(L); free(R); free(maps);
    const long frames = batches * B;
    char right[128] = "";                                /* --both: the right view's hash beside the left one's */
    if (both) snprintf(right, sizeof right, "\"hash_frame0_right\": \"%016llx\", ", hash0_r);
    if (use_temporal) snprintf(right + strlen(right), sizeof right - strlen(right), "\"hash_temporal\": \"%016llx\", ", hash_t);
    printf("{\"mode\": \"%d instances x batches of %d, sgm_reset + %s + sgm_match_wait, %s buffers, one thread each\", "
           "\"width\": %d, \"height\": %d, \"disparity_range\": %d, \"frames\": %ld, \"seconds\": %.4f, \"fps\": %.2f, \"ms_per_frame\": %.4f, "
           "\"mdisp_per_s\": %.1f, \"hash_frame0\": \"%016llx\", %s\"failed\": %s}\n",
           N, B, both ? "sgm_match_both_async" : "sgm_match_async", pageable ? "malloc'd" : "page-locked", W, H, D, frames, el, frames / el,
           frames ? el / frames * 1e3 : 0.0, (double)px * D * 8 * frames / el / 1e6, hash0, right, failed ? "true" : "false");
    return failed ? 1 : 0;
}
