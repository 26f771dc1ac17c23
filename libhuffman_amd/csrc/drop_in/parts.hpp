/*
 * drop_in/parts.hpp - what the other parts share and what needs nothing but libc and pthreads (no HIP header: a
 * stand-alone program can include this file alone, tests/test_drop_in_parts.py does): the environment reader, page
 * arithmetic, and "cut n bytes into parts, run them on helper threads".
 */
#pragma once

#include <limits.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <unistd.h>

/* An integer switch of the environment: `fallback` when the variable is not set, else what atoi() makes of it (an empty
 * or non-numeric value is 0), either of them brought into [lo, hi].  Never cached here: a caller that reads its switch
 * once keeps the result in a static of its own. */
static int env_int(const char *name, int fallback, int lo, int hi)
{
    const char *e = getenv(name);
    const int v = e ? atoi(e) : fallback;
    return v < lo ? lo : (v > hi ? hi : v);
}
/* a switch that is on or off: any value but 0 is on */
static int env_flag(const char *name, int fallback) { return env_int(name, fallback, INT_MIN, INT_MAX) != 0; }

/* The whole pages around [p, p + n) (outward: every page that holds one of its bytes) or inside it (inward: only pages
 * that hold nothing else; hi <= lo when there is none). */
typedef struct { uintptr_t lo, hi; } page_span_t;
static page_span_t page_span(const void *p, size_t n, int outward)
{
    const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE), up = outward ? 0 : page - 1, a = (uintptr_t)p;
    page_span_t s;
    s.lo = (a + up) & ~(page - 1);
    s.hi = (a + n + (page - 1 - up)) & ~(page - 1);
    return s;
}

/* ask for huge pages behind a buffer that is about to be written for the first time (advice only: failure is fine) */
static void advise_huge(void *dst, size_t n)
{
    const page_span_t s = page_span(dst, n, 0);
    if (s.hi > s.lo) (void)madvise((void *)s.lo, (size_t)(s.hi - s.lo), MADV_HUGEPAGE);
}

/* n bytes in at most `nthreads` contiguous parts of whole huge pages (2 MiB); the last part takes the rest.  Returns
 * the number of parts (0 for n == 0). */
#define PARTS_MAX 16
typedef struct { size_t off, n; } part_t;
static int split_parts(size_t n, int nthreads, part_t parts[PARTS_MAX])
{
    const size_t huge = (size_t)2 << 20;
    if (nthreads > PARTS_MAX) nthreads = PARTS_MAX;
    if (nthreads < 1) nthreads = 1;
    size_t piece = ((n / (size_t)nthreads) + huge - 1) & ~(huge - 1);
    if (!piece) piece = huge;                        /* (fewer bytes than threads) */
    int count = 0;
    for (; count < nthreads; count++) {
        const size_t off = (size_t)count * piece;
        if (off >= n) break;
        parts[count].off = off;
        parts[count].n = (n - off < piece || count == nthreads - 1) ? n - off : piece;
    }
    return count;
}

/* fn(&parts[i]) for every i < count (at most PARTS_MAX): part 0 on the calling thread, every other part on a thread of
 * its own - or here as well, when that thread cannot be made.  Returns when all have run. */
static void run_parts_sized(void *(*fn)(void *), char *parts, size_t size, int count)
{
    pthread_t th[PARTS_MAX];
    unsigned started = 0;            /* bit i: th[i] runs */
    for (int i = 1; i < count; i++) {
        if (pthread_create(&th[i], NULL, fn, parts + (size_t)i * size) == 0) started |= 1u << i;
        else (void)fn(parts + (size_t)i * size);
    }
    if (count > 0) (void)fn(parts);
    for (int i = 1; i < count; i++)
        if (started & (1u << i)) pthread_join(th[i], NULL);
}
template <typename T> static void run_parts(void *(*fn)(void *), T *parts, int count)
{
    run_parts_sized(fn, (char *)parts, sizeof(T), count);
}
