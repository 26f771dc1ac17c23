/* Stand-alone check of libhuffman_amd/csrc/host/workspace.hpp (tests/test_workspace.py builds this file with
 * AddressSanitizer + UndefinedBehaviorSanitizer and runs it): a toy owner with one group of each growth rule, a group of
 * two capacities, a soft group and a scan table that two groups include, over hooks that count what lives, zero only
 * when waited for, and fail the k-th allocation on request.
 * Exit status 0 and a last line "ok" when every check held; the first one that does not is printed and ends the run. */
#include <stdio.h>
#include <stdlib.h>

#include "../libhuffman_amd/csrc/host/workspace.hpp"

#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);          \
            printf(__VA_ARGS__);                                              \
            printf("\n");                                                     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

/* ---- the hooks: malloc behind a register of what lives ---- */
#define MAX_LIVE 64
static struct { void *p; uint64_t bytes; int pinned; } g_live[MAX_LIVE];
static struct { void *p; uint64_t bytes; } g_zero[MAX_LIVE];     /* zero fills enqueued, done by the next wait */
static int g_nzero, g_allocs, g_waits, g_fail_at, g_bad;
static int g_wait_mark = -1;                                      /* >= 0: a free while g_waits is still this is out of order */
#define TOY_ERROR 7

static int live_count(void)
{
    int n = 0;
    for (int i = 0; i < MAX_LIVE; i++) n += g_live[i].p != NULL;
    return n;
}
static int live_find(const void *p)
{
    for (int i = 0; i < MAX_LIVE; i++)
        if (p && g_live[i].p == p) return i;
    return -1;
}
static int toy_alloc(void **p, uint64_t bytes, int pinned)
{
    g_allocs++;
    if (g_fail_at && --g_fail_at == 0) return TOY_ERROR;
    for (int i = 0; i < MAX_LIVE; i++) {
        if (g_live[i].p) continue;
        g_live[i].p = malloc(bytes ? bytes : 1);
        if (!g_live[i].p) return TOY_ERROR;
        memset(g_live[i].p, 0xA5, bytes);
        g_live[i].bytes = bytes;
        g_live[i].pinned = pinned;
        *p = g_live[i].p;
        return 0;
    }
    g_bad = 1;                                      /* more buffers alive than the toy has */
    return TOY_ERROR;
}
static void toy_free(void *p, int pinned)
{
    const int i = live_find(p);
    if (i < 0 || g_live[i].pinned != pinned || g_waits == g_wait_mark) g_bad = 1;
    if (i < 0) return;
    free(p);
    g_live[i].p = NULL;
}
static int alloc_device(void **p, uint64_t bytes) { return toy_alloc(p, bytes, 0); }
static int alloc_pinned(void **p, uint64_t bytes) { return toy_alloc(p, bytes, 1); }
static void free_device(void *p) { toy_free(p, 0); }
static void free_pinned(void *p) { toy_free(p, 1); }
static int zero_device(void *p, uint64_t bytes)
{
    const int i = live_find(p);
    if (i < 0 || g_live[i].pinned || g_live[i].bytes != bytes || g_nzero == MAX_LIVE) { g_bad = 1; return TOY_ERROR; }
    g_zero[g_nzero].p = p;
    g_zero[g_nzero++].bytes = bytes;
    return 0;
}
static int toy_wait(void)
{
    g_waits++;
    for (int i = 0; i < g_nzero; i++)
        if (live_find(g_zero[i].p) >= 0) memset(g_zero[i].p, 0, g_zero[i].bytes);
    g_nzero = 0;
    return 0;
}
static const ws_hooks HOOKS = {alloc_device, alloc_pinned, free_device, free_pinned, zero_device, toy_wait};

/* ---- the toy owner ---- */
struct Scan { uint64_t *vals; uint32_t *tickets; uint32_t *done; void *not_a_buffer; };
struct Toy {
    int tag;
    uint64_t cap_e; uint32_t *e0; uint64_t *e1; Scan e_scan;     /* eighth, the scan table, e1 zero-filled */
    uint64_t cap_q; uint64_t *q_host, *q_dev;                    /* quarter, a pinned and a device buffer */
    uint64_t cap_d; void *d0; Scan d_scan;                       /* doubling, the scan table again */
    uint64_t cap_x; uint8_t *x0;                                 /* exact, soft */
    uint64_t cap_b0, cap_b1; uint64_t *b0; uint32_t *b1, *b_host; /* two capacities */
};

#define ROW(type, member, flags, expr) {offsetof(type, member), [](uint64_t n, uint64_t m) -> uint64_t { (void)n; (void)m; return (expr); }, flags}
static const ws_buf SCAN_ROWS[] = {
    ROW(Scan, vals, 0, n * sizeof(uint64_t)),
    ROW(Scan, tickets, WS_ZERO, (n / 4 + 2) * sizeof(uint32_t)),
    ROW(Scan, done, WS_ZERO, sizeof(uint32_t)),
};
static const ws_buf E_ROWS[] = {ROW(Toy, e0, 0, n * sizeof(uint32_t)), ROW(Toy, e1, WS_ZERO, (n + 1) * sizeof(uint64_t))};
static const ws_buf Q_ROWS[] = {ROW(Toy, q_host, WS_PINNED, n * sizeof(uint64_t)), ROW(Toy, q_dev, 0, n * sizeof(uint64_t))};
static const ws_buf D_ROWS[] = {ROW(Toy, d0, 0, 2 * n)};
static const ws_buf X_ROWS[] = {ROW(Toy, x0, 0, n)};
static const ws_buf B_ROWS[] = {ROW(Toy, b0, WS_ZERO, (n / 4 + 2) * sizeof(uint64_t)), ROW(Toy, b1, 0, 3 * m * sizeof(uint32_t)),
                                ROW(Toy, b_host, WS_PINNED, 3 * m * sizeof(uint32_t))};
enum { G_E, G_Q, G_D, G_X, G_B, G_COUNT };
static const ws_group GROUPS[G_COUNT] = {
    {"eighth", E_ROWS, 2, {offsetof(Toy, cap_e), WS_NO_CAP}, WS_EIGHTH, false, SCAN_ROWS, 3, offsetof(Toy, e_scan)},
    {"quarter", Q_ROWS, 2, {offsetof(Toy, cap_q), WS_NO_CAP}, WS_QUARTER, false, NULL, 0, 0},
    {"double", D_ROWS, 1, {offsetof(Toy, cap_d), WS_NO_CAP}, WS_DOUBLE, false, SCAN_ROWS, 3, offsetof(Toy, d_scan)},
    {"exact", X_ROWS, 1, {offsetof(Toy, cap_x), WS_NO_CAP}, WS_EXACT, true, NULL, 0, 0},
    {"two", B_ROWS, 3, {offsetof(Toy, cap_b0), offsetof(Toy, cap_b1)}, WS_EIGHTH, false, NULL, 0, 0},
};
static const int NALLOC[G_COUNT] = {5, 2, 4, 1, 3};

/* what a group holds: its live buffers, and whether none of its pointers is set */
static void group_state(Toy *t, int g, int *live, bool *all_null)
{
    *live = 0;
    *all_null = true;
    for (int i = 0; i < GROUPS[g].nbufs + GROUPS[g].nsub; i++) {
        const ws_buf *b;
        void *p;
        memcpy(&p, ws_slot(t, &GROUPS[g], i, &b), sizeof(p));
        if (p) *all_null = false;
        if (live_find(p) >= 0) (*live)++;
    }
}
static uint64_t cap_of(Toy *t, int g, int k) { return *ws_cap(t, GROUPS[g].cap_off[k]); }
static bool all_zero(const void *p, uint64_t bytes)
{
    for (uint64_t i = 0; i < bytes; i++)
        if (((const unsigned char *)p)[i]) return false;
    return true;
}
static uint64_t bytes_of(const void *p) { const int i = live_find(p); return i < 0 ? ~0ull : g_live[i].bytes; }

/* one grow() with the order of wait and free watched */
static int grow(Toy *t, int g, uint64_t need0, uint64_t need1)
{
    g_wait_mark = g_waits;
    const int rc = ws_grow(&HOOKS, t, &GROUPS[g], need0, need1);
    g_wait_mark = -1;
    return rc;
}

static int check_sequences(Toy *t)
{
    static const uint64_t needs[5] = {1, 17, 18, 400, 3};
    /* the closed forms: n + n/8 + 16; n + n/4 + 64; max(n, 2 cap) + 16; n - a request that fits changes nothing */
    static const uint64_t want[4][5] = {{17, 17, 36, 466, 466}, {65, 65, 65, 564, 564}, {17, 17, 50, 416, 416}, {1, 17, 18, 400, 400}};
    for (int g = G_E; g <= G_X; g++)
        for (int i = 0; i < 5; i++) {
            const uint64_t before = cap_of(t, g, 0);
            const int allocs = g_allocs, waits = g_waits;
            CHECK(grow(t, g, needs[i], 0) == 0, "%s need %llu", GROUPS[g].name, (unsigned long long)needs[i]);
            CHECK(cap_of(t, g, 0) == want[g][i], "%s need %llu: capacity %llu, not %llu", GROUPS[g].name, (unsigned long long)needs[i],
                  (unsigned long long)cap_of(t, g, 0), (unsigned long long)want[g][i]);
            if (want[g][i] == before)
                CHECK(g_allocs == allocs && g_waits == waits, "%s need %llu fits, yet %d allocations, %d waits", GROUPS[g].name,
                      (unsigned long long)needs[i], g_allocs - allocs, g_waits - waits);
            else
                CHECK(g_allocs == allocs + NALLOC[g] && g_waits > waits, "%s need %llu: %d allocations, %d waits", GROUPS[g].name,
                      (unsigned long long)needs[i], g_allocs - allocs, g_waits - waits);
            int live;
            bool none;
            group_state(t, g, &live, &none);
            CHECK(live == NALLOC[g], "%s holds %d live buffers", GROUPS[g].name, live);
        }
    /* sizes, kinds and zero fills of what stands now */
    CHECK(bytes_of(t->e0) == 466 * 4 && bytes_of(t->e1) == 467 * 8, "eighth: buffer sizes");
    CHECK(bytes_of(t->e_scan.vals) == 466 * 8 && bytes_of(t->e_scan.tickets) == (466 / 4 + 2) * 4 && bytes_of(t->e_scan.done) == 4, "eighth: scan sizes");
    CHECK(bytes_of(t->d0) == 832 && bytes_of(t->d_scan.vals) == 416 * 8 && bytes_of(t->d_scan.tickets) == (416 / 4 + 2) * 4, "double: sizes");
    CHECK(t->e_scan.not_a_buffer == NULL && t->d_scan.not_a_buffer == NULL, "a member no row names was written");
    CHECK(bytes_of(t->x0) == 400 && bytes_of(t->q_dev) == 564 * 8, "exact / quarter: sizes");
    CHECK(g_live[live_find(t->q_host)].pinned == 1 && g_live[live_find(t->q_dev)].pinned == 0, "quarter: kinds");
    CHECK(all_zero(t->e1, 467 * 8) && all_zero(t->e_scan.tickets, (466 / 4 + 2) * 4) && all_zero(t->e_scan.done, 4), "eighth: zero fills");
    CHECK(all_zero(t->d_scan.tickets, (416 / 4 + 2) * 4) && all_zero(t->d_scan.done, 4), "double: zero fills");
    CHECK(!all_zero(t->e0, 466 * 4) && !all_zero(t->e_scan.vals, 466 * 8), "a buffer that did not ask for zeros got them");

    static const uint64_t needs2[4][2] = {{2, 1}, {2, 40}, {100, 1}, {1, 1}};
    static const uint64_t want2[4][2] = {{18, 17}, {34, 61}, {128, 77}, {128, 77}};    /* the word that did not grow: + 16 */
    for (int i = 0; i < 4; i++) {
        const int allocs = g_allocs, waits = g_waits;
        CHECK(grow(t, G_B, needs2[i][0], needs2[i][1]) == 0, "two: step %d", i);
        CHECK(cap_of(t, G_B, 0) == want2[i][0] && cap_of(t, G_B, 1) == want2[i][1], "two: step %d: capacities %llu, %llu", i,
              (unsigned long long)cap_of(t, G_B, 0), (unsigned long long)cap_of(t, G_B, 1));
        CHECK(g_allocs - allocs == (i < 3 ? 3 : 0) && (i < 3 ? g_waits > waits : g_waits == waits), "two: step %d: %d allocations, %d waits", i,
              g_allocs - allocs, g_waits - waits);
    }
    CHECK(bytes_of(t->b0) == (128 / 4 + 2) * 8 && bytes_of(t->b1) == 3 * 77 * 4 && bytes_of(t->b_host) == 3 * 77 * 4, "two: sizes");
    CHECK(all_zero(t->b0, (128 / 4 + 2) * 8), "two: zero fill");
    CHECK(!g_bad, "a hook saw a pointer it does not know, the wrong kind of free, or a free before the wait");
    return 0;
}

static int check_failures(Toy *t)
{
    for (int g = 0; g < G_COUNT; g++)
        for (int k = 1; k <= NALLOC[g]; k++) {
            int others = 0;
            for (int o = 0; o < G_COUNT; o++) others += o == g ? 0 : NALLOC[o];
            const uint64_t need = cap_of(t, g, 0) + 1;
            g_fail_at = k;
            const int rc = grow(t, g, need, 1);
            g_fail_at = 0;
            CHECK(rc == TOY_ERROR, "%s, allocation %d failing: returned %d", GROUPS[g].name, k, rc);
            int live;
            bool none;
            group_state(t, g, &live, &none);
            CHECK(none && live == 0, "%s, allocation %d failing: pointers left", GROUPS[g].name, k);
            CHECK(cap_of(t, g, 0) == 0 && (GROUPS[g].cap_off[1] == WS_NO_CAP || cap_of(t, g, 1) == 0), "%s, allocation %d failing: capacity left", GROUPS[g].name, k);
            CHECK(live_count() == others, "%s, allocation %d failing: %d buffers live, the other groups have %d", GROUPS[g].name, k, live_count(), others);
            CHECK(grow(t, g, need, 1) == 0 && cap_of(t, g, 0) >= need, "%s: the growth after a failed one", GROUPS[g].name);
            CHECK(live_count() == others + NALLOC[g], "%s: %d buffers live after the growth that followed", GROUPS[g].name, live_count());
        }
    CHECK(all_zero(t->e1, (cap_of(t, G_E, 0) + 1) * 8) && all_zero(t->d_scan.done, 4) && all_zero(t->b0, (cap_of(t, G_B, 0) / 4 + 2) * 8), "zero fills after the failures");
    CHECK(!g_bad, "a hook saw a pointer it does not know, the wrong kind of free, or a free before the wait");
    return 0;
}

static int check_release(Toy *t)
{
    for (int round = 0; round < 2; round++) {       /* the second time on an owner that holds nothing */
        ws_release_all(&HOOKS, t, GROUPS, G_COUNT);
        CHECK(live_count() == 0, "%d buffers live after release_all", live_count());
        Toy zero;
        memset(&zero, 0, sizeof(zero));
        zero.tag = 41;
        CHECK(memcmp(t, &zero, sizeof(zero)) == 0, "release_all left a pointer or a capacity (or touched another member)");
    }
    CHECK(grow(t, G_D, 5, 0) == 0 && t->cap_d == 21 && live_count() == NALLOC[G_D], "a growth after release_all");
    ws_release(&HOOKS, t, &GROUPS[G_D]);
    CHECK(live_count() == 0 && !g_bad, "release of one group");
    return 0;
}

int main(void)
{
    Toy *t = (Toy *)calloc(1, sizeof(Toy));
    if (!t) return 1;
    t->tag = 41;
    const int rc = check_sequences(t) || check_failures(t) || check_release(t);
    ws_release_all(&HOOKS, t, GROUPS, G_COUNT);
    free(t);
    if (rc) return 1;
    printf("ok\n");
    return 0;
}
