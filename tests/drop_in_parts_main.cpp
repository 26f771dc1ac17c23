/* Stand-alone check of libhuffman_amd/csrc/drop_in/parts.hpp (tests/test_drop_in_parts.py builds this file with
 * AddressSanitizer + UndefinedBehaviorSanitizer and with ThreadSanitizer and runs both): split_parts, run_parts, env_int.
 * Exit status 0 and a last line "ok" when every check held; the first one that does not is printed and ends the run. */
#include <stdio.h>
#include <string.h>

#include "../libhuffman_amd/csrc/drop_in/parts.hpp"

#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);          \
            printf(__VA_ARGS__);                                              \
            printf("\n");                                                     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static const size_t MIB = (size_t)1 << 20;
static const int THREADS[] = {1, 3, 4, 16};

static int check_split(void)
{
    const size_t sizes[] = {0, 1, 2 * MIB - 1, 2 * MIB, 2 * MIB + 1, 16 * MIB, 16 * MIB + 5, 100 * MIB + 3};
    for (size_t n : sizes)
        for (int t : THREADS) {
            part_t parts[PARTS_MAX];
            const int count = split_parts(n, t, parts);
            CHECK(count >= 0 && count <= t && count <= PARTS_MAX, "n=%zu threads=%d count=%d", n, t, count);
            CHECK((count == 0) == (n == 0), "n=%zu threads=%d count=%d", n, t, count);
            size_t at = 0;
            for (int i = 0; i < count; i++) {
                CHECK(parts[i].off == at, "n=%zu threads=%d part %d starts at %zu, not %zu", n, t, i, parts[i].off, at);
                CHECK(parts[i].n > 0, "n=%zu threads=%d part %d is empty", n, t, i);
                if (i + 1 < count) CHECK(parts[i].n % (2 * MIB) == 0, "n=%zu threads=%d part %d has %zu bytes", n, t, i, parts[i].n);
                at += parts[i].n;
            }
            CHECK(at == n, "n=%zu threads=%d: the parts end at %zu", n, t, at);
        }
    return 0;
}

typedef struct { unsigned char *p; size_t n; unsigned char byte; int runs; } fill_t;
static void *fill_main(void *arg)
{
    fill_t *f = (fill_t *)arg;
    memset(f->p, f->byte, f->n);
    f->runs++;
    return NULL;
}

static int check_run(void)
{
    const size_t n = 16 * MIB + 5;
    unsigned char *buf = (unsigned char *)malloc(n);
    CHECK(buf != NULL, "malloc");
    for (int t : THREADS) {
        part_t cut[PARTS_MAX];
        fill_t fill[PARTS_MAX];
        const int count = split_parts(n, t, cut);
        memset(buf, 0, n);
        for (int i = 0; i < count; i++) { fill[i].p = buf + cut[i].off; fill[i].n = cut[i].n; fill[i].byte = (unsigned char)(i + 1); fill[i].runs = 0; }
        run_parts(fill_main, fill, count);
        for (int i = 0; i < count; i++) {
            CHECK(fill[i].runs == 1, "threads=%d: part %d ran %d times", t, i, fill[i].runs);
            for (size_t at = 0; at < cut[i].n; at++)
                CHECK(buf[cut[i].off + at] == i + 1, "threads=%d: byte %zu of part %d is %d", t, at, i, buf[cut[i].off + at]);
        }
    }
    fill_t none = {buf, n, 9, 0};
    memset(buf, 0, n);
    run_parts(fill_main, &none, 0);              /* no part: nothing runs */
    CHECK(none.runs == 0 && buf[0] == 0 && buf[n - 1] == 0, "run_parts ran a part of an empty list");
    free(buf);
    return 0;
}

/* what the hand-written readers that env_int replaced answered (value = set ? atoi(text) : default, then 0 <= value <= max) */
static int check_env(void)
{
    const char *name = "HUF_TEST_ENV_INT";
    const struct { const char *text; int want_0_8, want_1_16; } cases[] = {
        {NULL, 6, 6},  /* unset: the fallback */
        {"", 0, 1},    /* empty and non-numeric: atoi gives 0, then the lower bound */
        {"abc", 0, 1},
        {"-3", 0, 1},
        {"99", 8, 16},
        {"5", 5, 5},
        {"7x", 7, 7},
        {"0", 0, 1},
    };
    for (const auto &c : cases) {
        if (c.text) setenv(name, c.text, 1); else unsetenv(name);
        const int a = env_int(name, 6, 0, 8), b = env_int(name, 6, 1, 16);
        CHECK(a == c.want_0_8 && b == c.want_1_16, "\"%s\": %d and %d, not %d and %d", c.text ? c.text : "(unset)", a, b, c.want_0_8, c.want_1_16);
    }
    unsetenv(name);
    CHECK(env_int(name, 20, 0, 8) == 8 && env_int(name, -2, 0, 8) == 0, "a fallback outside the bounds is brought inside");
    CHECK(env_flag(name, 1) == 1 && env_flag(name, 0) == 0, "env_flag, unset");
    setenv(name, "0", 1);
    CHECK(env_flag(name, 1) == 0, "env_flag 0");
    setenv(name, "", 1);
    CHECK(env_flag(name, 1) == 0, "env_flag, empty");
    setenv(name, "-1", 1);
    CHECK(env_flag(name, 0) == 1, "env_flag -1");
    unsetenv(name);
    return 0;
}

int main(void)
{
    if (check_split() || check_run() || check_env()) return 1;
    printf("ok\n");
    return 0;
}
