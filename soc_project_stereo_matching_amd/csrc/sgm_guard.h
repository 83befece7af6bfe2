/* Guard bands and poison for device allocations: the bookkeeping of the debug allocation mode ("Guard bands").
 *
 * Plain C, static functions only, no HIP: csrc/sgm_runtime.hip includes it with the HIP calls behind sgm_guard_dev, and
 * tests/guard_driver.c includes it with malloc as the device.
 *
 * A guarded allocation of `bytes` is one device allocation of G + bytes + G, the whole of it filled with the poison byte:
 *
 *     base                 payload = base + G          payload + bytes              payload + bytes + G
 *     |<---- front band ---->|<-------- payload -------->|<-------- back band -------->|
 *
 * G is the band size asked for rounded up to SGM_GUARD_ALIGN, so the payload keeps the alignment the allocator gives; the back
 * band starts at payload + bytes exactly (no rounding gap: a one-byte overrun shows).  A band is intact while every byte of it
 * still holds the poison.  A stray write of the very poison byte cannot show -- which is why the tests run under two. */
#ifndef SGM_GUARD_H
#define SGM_GUARD_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define SGM_GUARD_ALIGN 4096u
#define SGM_GUARD_DEFAULT_POISON 0xA5

/* the device behind the registry; every call returns 0 on success.  sync: everything queued on that device has finished. */
typedef struct sgm_guard_dev {
    int (*alloc)(int ord, void** p, size_t bytes);
    int (*release)(int ord, void* p);
    int (*fill)(int ord, void* p, int byte, size_t bytes);
    int (*read)(int ord, void* host, const void* p, size_t bytes);
    int (*sync)(int ord);
} sgm_guard_dev;

typedef struct sgm_guard_entry {
    char*   base;
    char*   payload;
    size_t  bytes, guard;
    int     ord, poison;
} sgm_guard_entry;

static pthread_mutex_t  sgm_guard_lock = PTHREAD_MUTEX_INITIALIZER;
static sgm_guard_entry* sgm_guard_tab;
static size_t           sgm_guard_n, sgm_guard_cap;
static int              sgm_guard_sticky;        /* bands found violated when their buffer was freed, not yet returned by a check */

/* the band size for a guard of `guard` bytes: rounded up to SGM_GUARD_ALIGN (0 stays 0) */
static size_t sgm_guard_pad(size_t guard)
{
    return (guard + (SGM_GUARD_ALIGN - 1)) / SGM_GUARD_ALIGN * SGM_GUARD_ALIGN;
}

/* what one device allocation holds: both bands and the payload; never 0 bytes */
static size_t sgm_guard_total(size_t bytes, size_t G)
{
    const size_t t = 2 * G + bytes;
    return t ? t : 16;
}

/* SGM_DEBUG_GUARD=<bytes> and SGM_DEBUG_POISON=<0..255>, read at every call (a test sets them in a process that has the library
 * loaded).  Returns 1 with *G (padded) and *poison where either is set to something usable: a poison alone fills payloads and
 * keeps no bands.  Returns 0 with both unset: the caller then allocates exactly as it always did. */
static int sgm_guard_env(size_t* G, int* poison)
{
    const char* g = getenv("SGM_DEBUG_GUARD");
    const char* p = getenv("SGM_DEBUG_POISON");
    unsigned long long gv = 0;
    long pv = SGM_GUARD_DEFAULT_POISON;
    int on = 0;
    if (g && *g) {
        char* end = NULL;
        gv = strtoull(g, &end, 0);
        if (end == g || *end || gv > ((unsigned long long)1 << 30)) {
            fprintf(stderr, "sgm_mi355x: SGM_DEBUG_GUARD=%s is not a byte count up to 2^30; ignored\n", g);
            gv = 0;
        }
        on = gv > 0;
    }
    if (p && *p) {
        char* end = NULL;
        pv = strtol(p, &end, 0);
        if (end == p || *end || pv < 0 || pv > 255) {
            fprintf(stderr, "sgm_mi355x: SGM_DEBUG_POISON=%s is not a byte 0..255; ignored\n", p);
            pv = SGM_GUARD_DEFAULT_POISON;
        } else {
            on = 1;
        }
    }
    *G = sgm_guard_pad((size_t)gv);
    *poison = (int)pv;
    return on;
}

/* first and last offset in b[0..n) that does not hold the poison; 0 where every byte does */
static int sgm_guard_scan(const unsigned char* b, size_t n, int poison, size_t* first, size_t* last)
{
    if (n == 0 || (b[0] == (unsigned char)poison && memcmp(b, b + 1, n - 1) == 0)) return 0;
    size_t i = 0, j = n - 1;
    while (b[i] == (unsigned char)poison) ++i;
    while (b[j] == (unsigned char)poison) --j;
    *first = i;
    *last = j;
    return 1;
}

/* Both bands of one entry copied into scratch (guard bytes) and compared.  One line per violated band on `out`: the payload's
 * size, the band, the first and last differing offset -- relative to the payload's start for the front band (-1 is the byte just
 * in front of it), to the payload's end for the back band (0 is the first byte behind it).  Returns the number of violated bands
 * (a band that could not be read counts as one). */
static int sgm_guard_verify(const sgm_guard_dev* dev, const sgm_guard_entry* e, unsigned char* scratch, FILE* out)
{
    int bad = 0;
    if (e->guard == 0) return 0;
    for (int back = 0; back < 2; ++back) {
        const char* band = back ? e->payload + e->bytes : e->base;
        size_t first = 0, last = 0;
        if (dev->read(e->ord, scratch, band, e->guard) != 0) {
            if (out) fprintf(out, "sgm_mi355x: guard: payload of %zu bytes: the %s band could not be read\n", e->bytes, back ? "back" : "front");
            ++bad;
            continue;
        }
        if (!sgm_guard_scan(scratch, e->guard, e->poison, &first, &last)) continue;
        ++bad;
        if (!out) continue;
        if (back)
            fprintf(out, "sgm_mi355x: guard: payload of %zu bytes: back band written at +%zu .. +%zu behind its end (poison 0x%02X)\n",
                    e->bytes, first, last, e->poison);
        else
            fprintf(out, "sgm_mi355x: guard: payload of %zu bytes: front band written at -%zu .. -%zu in front of its start (poison 0x%02X)\n",
                    e->bytes, e->guard - first, e->guard - last, e->poison);
    }
    return bad;
}

/* G + bytes + G from the device, all of it poisoned, registered; *p = the payload */
static int sgm_guard_alloc(const sgm_guard_dev* dev, int ord, void** p, size_t bytes, size_t G, int poison)
{
    const size_t total = sgm_guard_total(bytes, G);
    void* base = NULL;
    if (dev->alloc(ord, &base, total) != 0 || !base) return -1;
    if (dev->fill(ord, base, poison, total) != 0) {
        (void)dev->release(ord, base);
        return -1;
    }
    sgm_guard_entry e;
    e.base = (char*)base;
    e.payload = (char*)base + G;
    e.bytes = bytes;
    e.guard = G;
    e.ord = ord;
    e.poison = poison;
    pthread_mutex_lock(&sgm_guard_lock);
    if (sgm_guard_n == sgm_guard_cap) {
        const size_t cap = sgm_guard_cap ? 2 * sgm_guard_cap : 128;
        sgm_guard_entry* tab = (sgm_guard_entry*)realloc(sgm_guard_tab, cap * sizeof *tab);
        if (!tab) {
            pthread_mutex_unlock(&sgm_guard_lock);
            (void)dev->release(ord, base);
            return -1;
        }
        sgm_guard_tab = tab;
        sgm_guard_cap = cap;
    }
    sgm_guard_tab[sgm_guard_n++] = e;
    pthread_mutex_unlock(&sgm_guard_lock);
    *p = e.payload;
    return 0;
}

/* 1: p was a guarded payload -- its bands verified (violations go to the sticky count, so a buffer released by a re-allocation
 * does not take its evidence with it), its allocation released, its entry dropped.  0: p is not registered, the caller frees it
 * as it always did.  -1: the device refused the release. */
static int sgm_guard_free(const sgm_guard_dev* dev, int ord, void* p, FILE* out)
{
    sgm_guard_entry e;
    size_t i;
    pthread_mutex_lock(&sgm_guard_lock);
    for (i = 0; i < sgm_guard_n; ++i)
        if (sgm_guard_tab[i].payload == (char*)p && sgm_guard_tab[i].ord == ord) break;
    if (i == sgm_guard_n) {
        pthread_mutex_unlock(&sgm_guard_lock);
        return 0;
    }
    e = sgm_guard_tab[i];
    sgm_guard_tab[i] = sgm_guard_tab[--sgm_guard_n];
    if (sgm_guard_n == 0) {
        free(sgm_guard_tab);
        sgm_guard_tab = NULL;
        sgm_guard_cap = 0;
    }
    pthread_mutex_unlock(&sgm_guard_lock);       /* the entry is ours alone now: nobody else can find it */
    if (e.guard) {
        unsigned char* scratch = (unsigned char*)malloc(e.guard);
        int bad = 2;                             /* bands nobody could look at are not clean */
        if (scratch && dev->sync(e.ord) == 0) bad = sgm_guard_verify(dev, &e, scratch, out);
        free(scratch);
        if (bad) {
            pthread_mutex_lock(&sgm_guard_lock);
            sgm_guard_sticky += bad;
            pthread_mutex_unlock(&sgm_guard_lock);
        }
    }
    return dev->release(e.ord, e.base) == 0 ? 1 : -1;
}

/* Every live band verified; returns the number of violated bands, those found at free time since the last check included (and
 * cleared).  *live / *live_bytes (either may be NULL): the registered allocations and the sum of their payloads. */
static int sgm_guard_check(const sgm_guard_dev* dev, int* live, size_t* live_bytes, FILE* out)
{
    int bad = 0, synced = -1;
    size_t n_bytes = 0, gmax = 0;
    unsigned char* scratch = NULL;
    pthread_mutex_lock(&sgm_guard_lock);         /* held over the copies: no buffer is freed under the check */
    for (size_t i = 0; i < sgm_guard_n; ++i)
        if (sgm_guard_tab[i].guard > gmax) gmax = sgm_guard_tab[i].guard;
    if (gmax) scratch = (unsigned char*)malloc(gmax);
    for (size_t i = 0; i < sgm_guard_n; ++i) {
        const sgm_guard_entry* e = &sgm_guard_tab[i];
        n_bytes += e->bytes;
        if (e->guard == 0) continue;
        if (!scratch) { bad += 2; continue; }
        if (e->ord != synced) {
            if (dev->sync(e->ord) != 0) { bad += 2; continue; }
            synced = e->ord;
        }
        bad += sgm_guard_verify(dev, e, scratch, out);
    }
    if (live) *live = (int)sgm_guard_n;
    if (live_bytes) *live_bytes = n_bytes;
    bad += sgm_guard_sticky;
    sgm_guard_sticky = 0;
    pthread_mutex_unlock(&sgm_guard_lock);
    free(scratch);
    return bad;
}

#endif /* SGM_GUARD_H */
