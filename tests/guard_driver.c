/* The bookkeeping of the debug allocation mode (csrc/sgm_guard.h) on its own, with malloc as the device: a stand-alone program
 * for -fsanitize=address,undefined (tests/test_guard_cpu.py builds and runs it).  The sanitizer sees every byte the registry
 * itself touches: a band it mis-sizes or a payload it misplaces is a heap overflow here. */
#define _GNU_SOURCE
#include "sgm_guard.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "guard_driver: %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static int n_sync;
static int dev_alloc(int o, void** p, size_t n) { (void)o; *p = malloc(n); return *p ? 0 : 1; }
static int dev_release(int o, void* p) { (void)o; free(p); return 0; }
static int dev_fill(int o, void* p, int byte, size_t n) { (void)o; memset(p, byte, n); return 0; }
static int dev_read(int o, void* host, const void* p, size_t n) { (void)o; memcpy(host, p, n); return 0; }
static int dev_sync(int o) { (void)o; __atomic_add_fetch(&n_sync, 1, __ATOMIC_RELAXED); return 0; }
static const sgm_guard_dev DEV = {dev_alloc, dev_release, dev_fill, dev_read, dev_sync};

/* one check with its report in `text` (at most cap - 1 bytes) */
static int check_into(char* text, size_t cap, int* live, size_t* bytes)
{
    char* buf = NULL;
    size_t len = 0;
    FILE* f = open_memstream(&buf, &len);
    CHECK(f);
    const int bad = sgm_guard_check(&DEV, live, bytes, f);
    fclose(f);
    CHECK(len < cap);
    memcpy(text, buf, len);
    text[len] = 0;
    free(buf);
    return bad;
}

static const sgm_guard_entry* entry_of(const void* payload)
{
    for (size_t i = 0; i < sgm_guard_n; ++i)
        if (sgm_guard_tab[i].payload == (const char*)payload) return &sgm_guard_tab[i];
    return NULL;
}

static void test_env(void)
{
    size_t G = 99;
    int poison = -1;
    unsetenv("SGM_DEBUG_GUARD");
    unsetenv("SGM_DEBUG_POISON");
    CHECK(sgm_guard_env(&G, &poison) == 0);
    setenv("SGM_DEBUG_GUARD", "1048576", 1);
    CHECK(sgm_guard_env(&G, &poison) == 1 && G == 1048576 && poison == SGM_GUARD_DEFAULT_POISON);
    setenv("SGM_DEBUG_GUARD", "1000", 1);
    setenv("SGM_DEBUG_POISON", "255", 1);
    CHECK(sgm_guard_env(&G, &poison) == 1 && G == 4096 && poison == 255);
    setenv("SGM_DEBUG_POISON", "0x5A", 1);
    CHECK(sgm_guard_env(&G, &poison) == 1 && poison == 0x5A);
    unsetenv("SGM_DEBUG_GUARD");
    setenv("SGM_DEBUG_POISON", "0", 1);                       /* a poison alone: payloads filled, no bands */
    CHECK(sgm_guard_env(&G, &poison) == 1 && G == 0 && poison == 0);
    setenv("SGM_DEBUG_POISON", "256", 1);                     /* not a byte: ignored, and with it the mode */
    CHECK(sgm_guard_env(&G, &poison) == 0);
    setenv("SGM_DEBUG_POISON", "junk", 1);
    setenv("SGM_DEBUG_GUARD", "12q", 1);
    CHECK(sgm_guard_env(&G, &poison) == 0 && G == 0);
    setenv("SGM_DEBUG_GUARD", "0", 1);
    unsetenv("SGM_DEBUG_POISON");
    CHECK(sgm_guard_env(&G, &poison) == 0);
    unsetenv("SGM_DEBUG_GUARD");
}

static void test_pad_arithmetic(void)
{
    static const size_t sizes[] = {0, 1, 4095, 4096, 4097};
    static const size_t guards[] = {0, 1, 100, 4095, 4096, 4097, 5000, 1 << 20, (1 << 20) + 1};
    static const size_t padded[] = {0, 4096, 4096, 4096, 4096, 8192, 8192, 1 << 20, (1 << 20) + 4096};
    char text[512];
    for (size_t g = 0; g < sizeof guards / sizeof *guards; ++g) {
        const size_t G = sgm_guard_pad(guards[g]);
        CHECK(G == padded[g] && G % SGM_GUARD_ALIGN == 0 && G >= guards[g]);
        for (size_t k = 0; k < sizeof sizes / sizeof *sizes; ++k) {
            const size_t n = sizes[k];
            const int poison = (k & 1) ? 0xFF : 0x5A;
            CHECK(sgm_guard_total(n, G) == (2 * G + n ? 2 * G + n : 16));
            void* p = NULL;
            CHECK(sgm_guard_alloc(&DEV, 0, &p, n, G, poison) == 0 && p);
            const sgm_guard_entry* e = entry_of(p);
            CHECK(e && e->payload == (char*)p && e->payload == e->base + G && e->bytes == n && e->guard == G && e->poison == poison);
            for (size_t i = 0; i < 2 * G + n; ++i) CHECK((unsigned char)e->base[i] == poison);   /* bands AND payload */
            /* the payload is the caller's: every byte of it written, first to last (the sanitizer has the allocation's true
             * end: a payload placed too far back would overflow here), and no band notices */
            memset(p, poison ^ 0xFF, n);
            int live = -1;
            size_t bytes = 99;
            CHECK(check_into(text, sizeof text, &live, &bytes) == 0 && live == 1 && bytes == n && text[0] == 0);
            CHECK(sgm_guard_free(&DEV, 0, p, stderr) == 1);
            CHECK(check_into(text, sizeof text, &live, &bytes) == 0 && live == 0 && bytes == 0);
        }
    }
}

static void test_two_of_one_size(void)
{
    void *a = NULL, *b = NULL;
    char text[512];
    int live = 0;
    size_t bytes = 0;
    CHECK(sgm_guard_alloc(&DEV, 0, &a, 640, 4096, 0xFF) == 0 && sgm_guard_alloc(&DEV, 0, &b, 640, 4096, 0xFF) == 0);
    CHECK(a != b && entry_of(a) && entry_of(b) && entry_of(a) != entry_of(b));
    CHECK(check_into(text, sizeof text, &live, &bytes) == 0 && live == 2 && bytes == 1280);
    CHECK(sgm_guard_free(&DEV, 0, a, stderr) == 1);
    CHECK(!entry_of(a) && entry_of(b));
    CHECK(sgm_guard_free(&DEV, 1, b, stderr) == 0);           /* another device's pointer of the same value is not this one */
    CHECK(check_into(text, sizeof text, &live, &bytes) == 0 && live == 1 && bytes == 640);
    CHECK(sgm_guard_free(&DEV, 0, b, stderr) == 1);
    CHECK(sgm_guard_free(&DEV, 0, b, stderr) == 0);           /* gone: a second free would be the caller's to do */
}

/* one byte planted at payload + where: reported once, with this side and this offset */
static void plant(char* payload, ptrdiff_t where, int value, const char* want)
{
    char text[512];
    int live = 0;
    const char old = payload[where];
    payload[where] = (char)value;
    const int bad = check_into(text, sizeof text, &live, NULL);
    payload[where] = old;
    if (!want) {
        CHECK(bad == 0 && text[0] == 0);
        return;
    }
    if (bad != 1 || !strstr(text, want) || strchr(text, '\n') != text + strlen(text) - 1) {
        fprintf(stderr, "guard_driver: wanted one line with \"%s\", got %d violation(s):\n%s", want, bad, text);
        exit(1);
    }
    CHECK(check_into(text, sizeof text, &live, NULL) == 0);   /* the byte put back: clean again, nothing sticks from a check */
}

static void test_planted_bytes(void)
{
    static const size_t sizes[] = {1, 4097, 100000};
    for (size_t k = 0; k < sizeof sizes / sizeof *sizes; ++k) {
        const size_t n = sizes[k], G = sgm_guard_pad(5000);   /* 8192 */
        const int poison = 0x5A;
        char* p = NULL;
        char want[128], head[64];
        CHECK(sgm_guard_alloc(&DEV, 0, (void**)&p, n, G, poison) == 0);
        snprintf(head, sizeof head, "payload of %zu bytes: ", n);
        snprintf(want, sizeof want, "%sfront band written at -1 .. -1 ", head);
        plant(p, -1, 0, want);
        snprintf(want, sizeof want, "%sback band written at +0 .. +0 ", head);
        plant(p, (ptrdiff_t)n, 0, want);
        snprintf(want, sizeof want, "%sfront band written at -%zu .. -%zu ", head, G, G);
        plant(p, -(ptrdiff_t)G, 0xFF, want);
        snprintf(want, sizeof want, "%sback band written at +%zu .. +%zu ", head, G - 1, G - 1);
        plant(p, (ptrdiff_t)(n + G - 1), 0xFF, want);
        /* THE blind spot, and the reason the GPU tests run under two poisons: a stray byte equal to the poison is not seen */
        plant(p, -1, poison, NULL);
        plant(p, (ptrdiff_t)n, poison, NULL);
        /* a run of bytes: first and last of it */
        char text[512];
        memset(p + n + 3, 0, 10);
        p[-7] = 1; p[-2] = 1;
        CHECK(check_into(text, sizeof text, NULL, NULL) == 2);
        CHECK(strstr(text, "front band written at -7 .. -2 ") && strstr(text, "back band written at +3 .. +12 "));
        memset(p + n + 3, poison, 10);
        p[-7] = p[-2] = (char)poison;
        CHECK(check_into(text, sizeof text, NULL, NULL) == 0);
        CHECK(sgm_guard_free(&DEV, 0, p, stderr) == 1);
    }
}

static void test_sticky(void)
{
    char text[512];
    char *p = NULL, *q = NULL;
    int live = -1;
    CHECK(sgm_guard_alloc(&DEV, 0, (void**)&p, 300, 4096, 0xFF) == 0 && sgm_guard_alloc(&DEV, 0, (void**)&q, 300, 4096, 0xFF) == 0);
    p[300] = 7;                                               /* one byte behind the payload ... */
    p[-4096] = 7;                                             /* ... and the first of the front band */
    char* buf = NULL;
    size_t len = 0;
    FILE* f = open_memstream(&buf, &len);
    CHECK(f && sgm_guard_free(&DEV, 0, p, f) == 1);           /* (a re-allocation frees the old buffer like this) */
    fclose(f);
    CHECK(strstr(buf, "payload of 300 bytes: front band written at -4096 .. -4096 ") &&
          strstr(buf, "payload of 300 bytes: back band written at +0 .. +0 "));
    free(buf);
    CHECK(check_into(text, sizeof text, &live, NULL) == 2 && live == 1 && text[0] == 0);   /* reported at the free, counted now */
    CHECK(check_into(text, sizeof text, &live, NULL) == 0 && live == 1);                   /* ... once */
    CHECK(sgm_guard_free(&DEV, 0, q, stderr) == 1);
    CHECK(check_into(text, sizeof text, &live, NULL) == 0 && live == 0);
}

static void test_unregistered(void)
{
    char text[64];
    int live = -1;
    size_t bytes = 99;
    void* p = malloc(32);
    CHECK(sgm_guard_free(&DEV, 0, p, stderr) == 0);           /* not ours: the caller frees it as it always did */
    free(p);
    CHECK(sgm_guard_free(&DEV, 0, NULL, stderr) == 0);
    CHECK(check_into(text, sizeof text, &live, &bytes) == 0 && live == 0 && bytes == 0 && sgm_guard_tab == NULL);
    /* a poison without bands: registered, filled, nothing to verify */
    char* q = NULL;
    CHECK(sgm_guard_alloc(&DEV, 0, (void**)&q, 0, 0, 0x5A) == 0 && q);
    CHECK(sgm_guard_alloc(&DEV, 0, (void**)&p, 48, 0, 0x5A) == 0 && ((unsigned char*)p)[47] == 0x5A);
    CHECK(check_into(text, sizeof text, &live, &bytes) == 0 && live == 2 && bytes == 48);
    CHECK(sgm_guard_free(&DEV, 0, p, stderr) == 1 && sgm_guard_free(&DEV, 0, q, stderr) == 1);
}

#define ROUNDS 1000
static void* worker(void* arg)
{
    const unsigned id = (unsigned)(size_t)arg;
    unsigned state = 12345u + id;
    char* held[4] = {0};
    for (int r = 0; r < ROUNDS; ++r) {
        state = state * 1664525u + 1013904223u;
        const int slot = r & 3;
        if (held[slot]) CHECK(sgm_guard_free(&DEV, (int)id & 1, held[slot], stderr) == 1);
        const size_t n = (state >> 8) % 9000;
        CHECK(sgm_guard_alloc(&DEV, (int)id & 1, (void**)&held[slot], n, 4096, 0xFF) == 0);
        memset(held[slot], (int)id, n);
        if ((r & 63) == 0) CHECK(sgm_guard_check(&DEV, NULL, NULL, stderr) == 0);          /* a check while others allocate */
    }
    for (int k = 0; k < 4; ++k) CHECK(sgm_guard_free(&DEV, (int)id & 1, held[k], stderr) == 1);
    return NULL;
}

static void test_threads(void)
{
    pthread_t t[4];
    char text[64];
    int live = -1;
    for (size_t i = 0; i < 4; ++i) CHECK(pthread_create(&t[i], NULL, worker, (void*)i) == 0);
    for (size_t i = 0; i < 4; ++i) CHECK(pthread_join(t[i], NULL) == 0);
    CHECK(check_into(text, sizeof text, &live, NULL) == 0 && live == 0 && sgm_guard_n == 0);
}

int main(void)
{
    test_env();
    test_pad_arithmetic();
    test_two_of_one_size();
    test_planted_bytes();
    test_sticky();
    test_unregistered();
    test_threads();
    CHECK(n_sync > 0);
    printf("guard_driver ok\n");
    return 0;
}
