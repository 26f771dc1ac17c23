/*
 * host/workspace.hpp - growable groups of buffers described by tables (no HIP header, no hufgpu_ctx: a stand-alone
 * program can include this file alone, tests/test_workspace.py does).  A group is a list of buffers whose pointers are
 * members of one owner struct, sized from the group's one or two capacity words, which are members of it too.  The
 * memory itself comes through the includer's hooks.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* Every int is 0 or an error, which ws_grow() hands back as it is. */
struct ws_hooks {
    int (*alloc_device)(void **p, uint64_t bytes);
    int (*alloc_pinned)(void **p, uint64_t bytes);
    void (*free_device)(void *p);
    void (*free_pinned)(void *p);
    int (*zero_device)(void *p, uint64_t bytes);   /* may only enqueue: ws_grow() waits behind it */
    int (*wait)(void);                             /* until nothing enqueued uses the group's buffers, nor will before it returns */
};

/* The capacity a word gets when its group grows: `need` is what the call asks for, `cap` what the word holds. */
enum ws_rule {
    WS_EIGHTH,    /* need + need/8 + 16.  In a group of two words the one that did not grow keeps its value, + 16 */
    WS_QUARTER,   /* need + need/4 + 64 */
    WS_DOUBLE,    /* max(need, 2 cap) + 16: for bounds that jump */
    WS_EXACT      /* need */
};

static uint64_t ws_new_cap(ws_rule rule, uint64_t need, uint64_t cap)
{
    switch (rule) {
    case WS_EIGHTH: return (need > cap ? need + need / 8 : cap) + 16;
    case WS_QUARTER: return need + need / 4 + 64;
    case WS_DOUBLE: return (need > 2 * cap ? need : 2 * cap) + 16;
    default: return need;
    }
}

#define WS_PINNED 1u   /* pinned host memory, not device memory */
#define WS_ZERO 2u     /* zero-filled after allocation (device memory only) */
struct ws_buf {
    size_t off;                                      /* of the pointer, in the owner (the members differ in pointer type) */
    uint64_t (*bytes)(uint64_t cap0, uint64_t cap1);
    unsigned flags;
};

#define WS_NO_CAP ((size_t)-1)
struct ws_group {
    const char *name;
    const ws_buf *bufs;
    int nbufs;
    size_t cap_off[2];      /* of the capacity words (uint64_t) in the owner; [1] = WS_NO_CAP: one word */
    ws_rule rule;
    bool soft;              /* for the includer, ws_grow() does the same either way: a failure is the caller's cue to fall back, not an error to report */
    const ws_buf *sub;      /* a second table whose offsets count from sub_off: a struct of buffers that several groups hold */
    int nsub;
    size_t sub_off;
};

static uint64_t *ws_cap(void *owner, size_t off) { return (uint64_t *)((char *)owner + off); }

/* buffer i of a group: the slot of its pointer; *buf its row */
static char *ws_slot(void *owner, const ws_group *g, int i, const ws_buf **buf)
{
    *buf = i < g->nbufs ? &g->bufs[i] : &g->sub[i - g->nbufs];
    return (char *)owner + (i < g->nbufs ? 0 : g->sub_off) + (*buf)->off;
}

/* Frees a group (no wait: the caller knows that nothing uses it): every pointer null, the capacities 0. */
static void ws_release(const ws_hooks *h, void *owner, const ws_group *g)
{
    for (int i = 0; i < g->nbufs + g->nsub; i++) {
        const ws_buf *b;
        char *slot = ws_slot(owner, g, i, &b);
        void *p;
        memcpy(&p, slot, sizeof(p));
        if (!p) continue;
        if (b->flags & WS_PINNED) h->free_pinned(p);
        else h->free_device(p);
        memset(slot, 0, sizeof(p));
    }
    *ws_cap(owner, g->cap_off[0]) = 0;
    if (g->cap_off[1] != WS_NO_CAP) *ws_cap(owner, g->cap_off[1]) = 0;
}

static void ws_release_all(const ws_hooks *h, void *owner, const ws_group *groups, int n)
{
    for (int i = 0; i < n; i++) ws_release(h, owner, &groups[i]);
}

/* Room for need0 (and need1) in a group.  When it is there already - every call but a few - this is the compares.
 * Otherwise: wait, free the group, allocate every buffer at the new capacities, zero those that ask for it and wait for
 * the zeros, store the capacities.  Any failure leaves the group released - a later call starts clean - and is returned. */
static int ws_grow(const ws_hooks *h, void *owner, const ws_group *g, uint64_t need0, uint64_t need1)
{
    uint64_t *const c0 = ws_cap(owner, g->cap_off[0]);
    uint64_t *const c1 = g->cap_off[1] == WS_NO_CAP ? NULL : ws_cap(owner, g->cap_off[1]);
    if (need0 <= *c0 && (!c1 || need1 <= *c1)) return 0;
    int rc = h->wait();
    if (rc) return rc;
    const uint64_t n0 = ws_new_cap(g->rule, need0, *c0), n1 = c1 ? ws_new_cap(g->rule, need1, *c1) : 0;
    ws_release(h, owner, g);
    bool zeroed = false;
    for (int i = 0; i < g->nbufs + g->nsub && !rc; i++) {
        const ws_buf *b;
        char *slot = ws_slot(owner, g, i, &b);
        const uint64_t bytes = b->bytes(n0, n1);
        void *p = NULL;
        rc = b->flags & WS_PINNED ? h->alloc_pinned(&p, bytes) : h->alloc_device(&p, bytes);
        if (rc) break;
        memcpy(slot, &p, sizeof(p));
        if (b->flags & WS_ZERO) {
            rc = h->zero_device(p, bytes);
            zeroed = true;
        }
    }
    if (!rc && zeroed) rc = h->wait();
    if (rc) {
        ws_release(h, owner, g);
        return rc;
    }
    *c0 = n0;
    if (c1) *c1 = n1;
    return 0;
}
