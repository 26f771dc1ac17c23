/*
 * drop_in/transfer.hpp - bytes between pageable host memory and the device: populating pages before they are copied
 * into, the double-buffered piece mover, lane_copy() (one transfer over a few threads), the duplex pool (persistent
 * lanes per direction, transfers that overlap the kernels), and huf_gpu_copy_out (host -> fresh host memory).
 */

/* Device -> a memory stream's buffer.  The bytes behind a stream's contents are usually pages that
 * were never touched (a fresh buffer, the caller's huf_memopen capacity): copied into as they are,
 * the copy spends its time in page faults (240 MiB: 28-35 ms for a 4.5 ms copy).  So the pages are
 * populated first - madvise(MADV_POPULATE_WRITE), contents untouched, a few threads on disjoint
 * parts; with the huge pages stream_alloc asked for that is 2-3 ms - and copied into afterwards
 * (not at the same time as ANY copy of this process, in either direction: the copies' page pinning
 * and the populating threads then fight for the address-space lock - populating under the copy
 * itself 56 ms, under the input's copy to the device still slower than one after the other). */
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
#define PREFAULT_MIN ((size_t)16 << 20)
typedef struct { char *p; size_t n; } prefault_t;

static void *prefault_main(void *arg)
{
    prefault_t *w = (prefault_t *)arg;
    const page_span_t s = page_span(w->p, w->n, 1);
    if (madvise((void *)s.lo, (size_t)(s.hi - s.lo), MADV_POPULATE_WRITE) != 0) {
        /* older kernels: a write fault per page, contents kept (one atomic read-modify-write) */
        const size_t page = (size_t)sysconf(_SC_PAGESIZE);
        for (char *q = w->p; q < w->p + w->n; q += page) (void)__atomic_fetch_or(q, 0, __ATOMIC_RELAXED);
    }
    return NULL;
}

/* a default that grows with the machine: for 16 CPUs and more, for 8, for 4, for fewer */
static int by_cpus(int from16, int from8, int from4, int fewer)
{
    const long cpus = sysconf(_SC_NPROCESSORS_ONLN);
    return cpus >= 16 ? from16 : (cpus >= 8 ? from8 : (cpus >= 4 ? from4 : fewer));
}

static int prefault_threads(void)
{
    static const int n = env_int("HUF_GPU_PREFAULT_THREADS", by_cpus(4, 4, 4, (int)sysconf(_SC_NPROCESSORS_ONLN)), 0, PARTS_MAX);
    return n;
}

/* populate [p, p + n): the calling thread and a few helpers on disjoint parts; returns when the pages are there (never
 * beside a copy, see above) */
static void prefault(char *p, size_t n)
{
    const int nthreads = prefault_threads();
    if (n < PREFAULT_MIN || nthreads <= 0) return;
    part_t cut[PARTS_MAX];
    prefault_t part[PARTS_MAX];
    const int count = split_parts(n, nthreads, cut);
    for (int i = 0; i < count; i++) { part[i].p = p + cut[i].off; part[i].n = cut[i].n; }
    run_parts(prefault_main, part, count);
}

/* Large transfers between PAGEABLE host memory (a caller's buffer, a memory stream) and the device.
 * hipMemcpy from or to pageable memory runs at 10-18 GB/s here (the runtime pins or stages piece by piece on one
 * thread), a fifth of what the link carries.  lane_copy() cuts the transfer into pieces of LANE_SLOT bytes and gives
 * them to a few threads (lanes); every lane owns two pinned slots and a stream: memcpy into a slot, asynchronous copy
 * from it - while that runs, memcpy into the other slot (and the other way round for device -> host, where the
 * destination's pages are populated piece by piece by the lane that is about to fill them: no populate of the whole
 * buffer in front of the copy).  Returns when everything has arrived. */
#define LANE_SLOT ((size_t)8 << 20)
#define LANE_MIN ((size_t)32 << 20)        /* below this one hipMemcpy is as good */
typedef struct {
    staging_t *st;
    int device, lane, nlanes, to_device;
    char *host;
    char *dev;
    size_t n;
    int err;
} lane_job_t;

static int lane_count(void)
{
    /* (1 GiB of log text through huffmanfile: 0 lanes 5.2, 2: 5.3, 4: 5.7, 6: 6.0, 8: 4.7 GiB/s) */
    static const int n = env_int("HUF_GPU_COPY_LANES", by_cpus(6, 4, 2, 1), 0, LANE_MAX);
    return n;
}

/* The double-buffered piece loops of every lane, lane_copy's and the duplex pool's.  A transfer of n bytes is cut into
 * pieces of `piece` bytes; the caller moves pieces first, first + step, ... through its two pinned slots of `piece`
 * bytes on its stream.  ev[i] stands behind the last copy that used slot[i]; k counts the pieces the caller has moved
 * through the slots since they were made (k & 1: the slot of the next piece) - a lane that lives across transfers
 * carries it along.  Both return nonzero at the first failing HIP call.
 *
 * host -> device: memcpy into a slot, asynchronous copy from it, the next piece into the other slot meanwhile.  Returns
 * with the copies on the stream, not waited for. */
static int move_pieces_h2d(const char *host, char *dev, size_t n, size_t first, size_t step, size_t piece,
                           hipStream_t stream, char *const slot[2], hipEvent_t ev[2], unsigned &k)
{
    const size_t pieces = (n + piece - 1) / piece;
    for (size_t q = first; q < pieces; q += step) {
        const size_t off = q * piece, len = (n - off < piece) ? n - off : piece;
        const unsigned i = k & 1;
        if (k >= 2 && hipEventSynchronize(ev[i]) != hipSuccess) return 1;        /* the copy that read this slot two pieces ago */
        memcpy(slot[i], host + off, len);
        k++;                                                                     /* (the slot is used, whatever becomes of its copy) */
        if (hipMemcpyAsync(dev + off, slot[i], len, hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipEventRecord(ev[i], stream) != hipSuccess) return 1;
    }
    return 0;
}

/* device -> host: the copy of piece q + step is in flight while piece q goes from its slot to the destination, whose
 * pages are populated just before (contents untouched; pages that are there already cost nothing).  Returns when the
 * caller's pieces are in place. */
static int move_pieces_d2h(char *host, const char *dev, size_t n, size_t first, size_t step, size_t piece,
                           hipStream_t stream, char *const slot[2], hipEvent_t ev[2], unsigned &k)
{
    const size_t pieces = (n + piece - 1) / piece;
    size_t q = first, off = q * piece, len = 0;
    if (q < pieces) {
        len = (n - off < piece) ? n - off : piece;
        if (hipMemcpyAsync(slot[k & 1], dev + off, len, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipEventRecord(ev[k & 1], stream) != hipSuccess) return 1;
    }
    for (; q < pieces; q += step, k++) {
        const size_t qn = q + step;
        size_t offn = 0, lenn = 0;
        if (qn < pieces) {
            offn = qn * piece;
            lenn = (n - offn < piece) ? n - offn : piece;
            if (hipMemcpyAsync(slot[(k + 1) & 1], dev + offn, lenn, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                hipEventRecord(ev[(k + 1) & 1], stream) != hipSuccess) return 1;
        }
        prefault_t w = {host + off, len};
        prefault_main(&w);
        if (hipEventSynchronize(ev[k & 1]) != hipSuccess) return 1;
        memcpy(host + off, slot[k & 1], len);
        off = offn;
        len = lenn;
    }
    return 0;
}

static void *lane_main(void *arg)
{
    lane_job_t *j = (lane_job_t *)arg;
    staging_t *st = j->st;
    if (hipSetDevice(j->device) != hipSuccess) { j->err = 1; return NULL; }
    hipStream_t s = st->lane_stream[j->lane];
    char *const slot[2] = {(char *)st->lane_pin + (size_t)(2 * j->lane) * LANE_SLOT, (char *)st->lane_pin + (size_t)(2 * j->lane + 1) * LANE_SLOT};
    unsigned k = 0;                              /* (every transfer ends with the stream drained: the slots start afresh) */
    /* this lane's pieces, in order: lane, lane + nlanes, ... */
    if (j->to_device ? move_pieces_h2d(j->host, j->dev, j->n, (size_t)j->lane, (size_t)j->nlanes, LANE_SLOT, s, slot, st->lane_ev[j->lane], k)
                     : move_pieces_d2h(j->host, j->dev, j->n, (size_t)j->lane, (size_t)j->nlanes, LANE_SLOT, s, slot, st->lane_ev[j->lane], k))
        j->err = 1;
    if (hipStreamSynchronize(s) != hipSuccess) j->err = 1;
    return NULL;
}

/* host <-> device, n bytes; falls back to one plain copy for small transfers or when the lanes cannot be set up */
static huf_error_t lane_copy(int to_device, void *dev, void *host, size_t n)
{
    staging_t *st = &g_stage;
    const int nl = lane_count();
    if (n < LANE_MIN || nl <= 0) goto plain;
    (void)hipSetDevice(t_session->device);
    if (st->lanes_ready < 0) goto plain;             /* a set-up that failed once: plain copies from then on */
    if (st->lanes_ready == 0) {
        st->lanes_ready = -1;
        int made_streams = 0, made_events = 0, failed = 0;
        if (hipHostMalloc(&st->lane_pin, (size_t)2 * (size_t)nl * LANE_SLOT, hipHostMallocPortable) != hipSuccess) { st->lane_pin = NULL; failed = 1; }
        for (int i = 0; i < nl && !failed; i++) {
            if (hipStreamCreateWithFlags(&st->lane_stream[i], hipStreamNonBlocking) != hipSuccess) { failed = 1; break; }
            made_streams++;
            for (int e = 0; e < 2; e++) {
                if (hipEventCreateWithFlags(&st->lane_ev[i][e], hipEventDisableTiming) != hipSuccess) { failed = 1; break; }
                made_events++;
            }
        }
        if (failed) {                                /* give back what was made: nothing of it is looked at again */
            (void)hipGetLastError();
            for (int k = 0; k < made_events; k++) (void)hipEventDestroy(st->lane_ev[k / 2][k % 2]);
            for (int i = 0; i < made_streams; i++) (void)hipStreamDestroy(st->lane_stream[i]);
            if (st->lane_pin) (void)hipHostFree(st->lane_pin);
            st->lane_pin = NULL;
            goto plain;
        }
        st->lanes_ready = 1;
    }
    {
        (void)hipDeviceSynchronize();                /* what the device buffer is read from or written by has finished (the lanes' streams do not wait for others) */
        lane_job_t job[LANE_MAX];
        int bad = 0;
        if (!to_device) advise_huge(host, n);
        for (int i = 0; i < nl; i++) {
            job[i].st = st; job[i].device = t_session->device; job[i].lane = i; job[i].nlanes = nl; job[i].to_device = to_device;
            job[i].host = (char *)host; job[i].dev = (char *)dev; job[i].n = n; job[i].err = 0;
        }
        run_parts(lane_main, job, nl);               /* lane 0 is the calling thread's */
        for (int i = 0; i < nl; i++) bad |= job[i].err;
        if (bad) { (void)hipGetLastError(); return HUF_ERROR_FATAL; }
        return HUF_ERROR_SUCCESS;
    }
plain:
    return (huf_error_t)(to_device ? hufgpu_memcpy_h2d(g_ctx, dev, host, n) : hufgpu_memcpy_d2h(g_ctx, host, dev, n));
}

/* ------------------------------------------------------------------ transfers in both directions at once
 * huf_encode / huf_decode between two memory streams (src/encoder.c:261-388, src/decoder.c:201-287 with the
 * reference's memory streams on both ends) move N bytes to the device and about as many back; done one after the
 * other - copy in, kernels, copy out, per round of 256 MiB - that reaches 11 GiB/s over a link that carries 53 each
 * way AT THE SAME TIME.  Here a session owns two sets of persistent copy threads ("lanes"), one per direction;
 * a lane has two pinned slots, a stream and its events.  The caller publishes SEGMENTS - (host address, device
 * address, bytes) - per direction; the lanes of that direction take the segments in order and share the pieces of
 * each (DX_SLOT bytes, dealt out round robin).
 *   host -> device: memcpy into a slot, asynchronous copy from it, the next piece into the other slot meanwhile.
 *     A lane reports a segment as ISSUED - its copies are on the lane's stream, an event behind them - and the
 *     caller makes the compute stream wait for those events: no host thread waits for a copy to arrive.
 *   device -> host: asynchronous copy into a slot, and while it runs the piece before it goes from the other slot
 *     to its destination, whose pages the lane populates first (d2h_to_memstream's comment says why not earlier).
 *     A lane reports a segment as DONE when its pieces are in place.
 * Rounds of HUF_GPU_ROUND_MB (32) then overlap as: copy-in of round i + 1 | kernels of round i | copy-out of round
 * i - 1, inside ONE session (two sessions on one GPU lose: profiles/r04/python_layer_sessions.txt). */
#define DX_LANES_MAX 8
#define DX_SLOT ((size_t)4 << 20)
#define DX_RING 16                       /* segments a direction may have in flight */
typedef struct {
    char *host, *dev;
    size_t n;
    int direct;                          /* host -> device: the host bytes lie in registered (pinned) pages - copied from where they are */
    int issued_left;                     /* lanes that have not yet put their pieces on their streams (host -> device) */
    int done_left;                       /* lanes that have not yet finished their pieces */
} dx_seg_t;
typedef struct {
    struct dx_pool *pool;
    int dir, idx;
    pthread_t th;
    hipStream_t stream;
    hipEvent_t slot_ev[2];
    hipEvent_t seg_ev[DX_RING];          /* host -> device: behind the lane's last copy of a segment */
    char *slot[2];
} dx_lane_t;
typedef struct dx_pool {
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int device;
    int ready;                           /* 0 not made, 1 usable, -1 could not be made */
    int err;                             /* a lane met a failing HIP call (sticky for the pool's life) */
    int nl[2];                           /* lanes per direction: [0] host -> device, [1] device -> host */
    int can_register;                    /* hipHostRegister works on this process's pageable memory (dx_register_input) */
    dx_lane_t lane[2][DX_LANES_MAX];
    dx_seg_t seg[2][DX_RING];
    uint64_t published[2];               /* segments ever published per direction (a segment's id is its number) */
    void *pin;
} dx_pool_t;

static int dx_lanes_per_dir(void)
{
    static const int n = env_int("HUF_GPU_DUPLEX_LANES", by_cpus(5, 3, 2, 1), 0, DX_LANES_MAX);
    return n;
}

static void dx_fail(dx_pool_t *P) { pthread_mutex_lock(&P->mu); P->err = 1; pthread_cond_broadcast(&P->cv); pthread_mutex_unlock(&P->mu); (void)hipGetLastError(); }

static void *dx_lane_main(void *arg)
{
    dx_lane_t *L = (dx_lane_t *)arg;
    dx_pool_t *P = L->pool;
    const int dir = L->dir, nl = P->nl[dir];
    if (hipSetDevice(P->device) != hipSuccess) dx_fail(P);
    uint64_t cur = 0;                    /* the next segment of this direction this lane looks at */
    unsigned k = 0;                      /* pieces this lane has moved: k & 1 is the slot of the next */
    for (;;) {
        pthread_mutex_lock(&P->mu);
        while (cur >= P->published[dir]) pthread_cond_wait(&P->cv, &P->mu);
        const dx_seg_t sg = P->seg[dir][cur % DX_RING];
        pthread_mutex_unlock(&P->mu);
        /* piece q of segment `cur` is lane (q + cur) % nl's: short segments do not all start at lane 0 */
        size_t q = (size_t)(((uint64_t)L->idx + (uint64_t)nl - cur % (uint64_t)nl) % (uint64_t)nl);
        int bad = 0;
        if (dir == 0 && sg.direct) {
            /* registered pages: one asynchronous copy of the whole segment, by the lane whose turn it is */
            if (q == 0 && hipMemcpyAsync(sg.dev, sg.host, sg.n, hipMemcpyHostToDevice, L->stream) != hipSuccess) bad = 1;
            if (hipEventRecord(L->seg_ev[cur % DX_RING], L->stream) != hipSuccess) bad = 1;
        } else if (dir == 0) {
            bad = move_pieces_h2d(sg.host, sg.dev, sg.n, q, (size_t)nl, DX_SLOT, L->stream, L->slot, L->slot_ev, k);
            if (hipEventRecord(L->seg_ev[cur % DX_RING], L->stream) != hipSuccess) bad = 1;
        } else {
            bad = move_pieces_d2h(sg.host, sg.dev, sg.n, q, (size_t)nl, DX_SLOT, L->stream, L->slot, L->slot_ev, k);
        }
        pthread_mutex_lock(&P->mu);
        if (bad) { P->err = 1; (void)hipGetLastError(); }
        dx_seg_t *g = &P->seg[dir][cur % DX_RING];
        g->issued_left--;
        g->done_left--;
        pthread_cond_broadcast(&P->cv);
        pthread_mutex_unlock(&P->mu);
        cur++;
    }
    return NULL;
}

/* the session's pool, made on first use; NULL when it cannot be made (the callers then move bytes the old way) */
static dx_pool_t *dx_get(void)
{
    static dx_pool_t pools[HUF_MAX_SESSIONS];
    dx_pool_t *P = &pools[t_session - g_sessions];
    if (P->ready > 0) return P->err ? NULL : P;
    if (P->ready < 0) return NULL;
    const int nl = dx_lanes_per_dir();
    P->ready = -1;
    if (nl <= 0) return NULL;
    (void)hipSetDevice(t_session->device);
    P->device = t_session->device;
    P->nl[0] = P->nl[1] = nl;
    {   /* can this process register pageable memory at all?  (HUF_GPU_REGISTER=0: never tried) */
        void *probe = NULL;
        if (env_flag("HUF_GPU_REGISTER", 1) && posix_memalign(&probe, 4096, 1 << 16) == 0) {
            memset(probe, 1, 1 << 16);
            if (hipHostRegister(probe, 1 << 16, hipHostRegisterDefault) == hipSuccess) {
                (void)hipHostUnregister(probe);
                P->can_register = 1;
                P->nl[1] = nl + 3 < DX_LANES_MAX ? nl + 3 : DX_LANES_MAX;     /* (threads the other direction will rarely need) */
            } else (void)hipGetLastError();
            free(probe);
        }
    }
    pthread_mutex_init(&P->mu, NULL);
    pthread_cond_init(&P->cv, NULL);
    if (hipHostMalloc(&P->pin, (size_t)2 * (size_t)(P->nl[0] + P->nl[1]) * DX_SLOT, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); P->pin = NULL; return NULL; }
    int ok = 1, slots = 0;
    for (int d = 0; d < 2 && ok; d++)
        for (int i = 0; i < P->nl[d] && ok; i++, slots += 2) {
            dx_lane_t *L = &P->lane[d][i];
            L->pool = P; L->dir = d; L->idx = i;
            L->slot[0] = (char *)P->pin + (size_t)slots * DX_SLOT;
            L->slot[1] = L->slot[0] + DX_SLOT;
            if (hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking) != hipSuccess) ok = 0;
            for (int e = 0; e < 2 && ok; e++) if (hipEventCreateWithFlags(&L->slot_ev[e], hipEventDisableTiming) != hipSuccess) ok = 0;
            for (int e = 0; e < DX_RING && ok; e++) if (hipEventCreateWithFlags(&L->seg_ev[e], hipEventDisableTiming) != hipSuccess) ok = 0;
        }
    if (!ok) { (void)hipGetLastError(); return NULL; }        /* (what was made stays: a process makes at most one pool a session) */
    for (int d = 0; d < 2; d++)
        for (int i = 0; i < P->nl[d]; i++) {
            dx_lane_t *L = &P->lane[d][i];
            if (pthread_create(&L->th, NULL, dx_lane_main, L) != 0) return NULL;     /* (lanes that run wait for ever for work: harmless) */
            pthread_detach(L->th);
        }
    P->ready = 1;
    return P;
}

/* a segment for the lanes of direction `dir`; returns its id.  Waits while the direction's ring is full. */
static uint64_t dx_publish(dx_pool_t *P, int dir, void *host, void *dev, size_t n, int direct = 0)
{
    pthread_mutex_lock(&P->mu);
    const uint64_t id = P->published[dir];
    if (id >= DX_RING)
        while (P->seg[dir][id % DX_RING].done_left > 0 && !P->err) pthread_cond_wait(&P->cv, &P->mu);      /* the segment a ring ago */
    dx_seg_t *g = &P->seg[dir][id % DX_RING];
    g->host = (char *)host; g->dev = (char *)dev; g->n = n; g->direct = direct;
    g->issued_left = g->done_left = P->nl[dir];
    P->published[dir] = id + 1;
    pthread_cond_broadcast(&P->cv);
    pthread_mutex_unlock(&P->mu);
    return id;
}
/* host -> device segment `id`: every lane has its copies on its stream; the default stream (the kernels') waits for them */
static huf_error_t dx_wait_issued(dx_pool_t *P, uint64_t id)
{
    pthread_mutex_lock(&P->mu);
    while (P->seg[0][id % DX_RING].issued_left > 0 && !P->err) pthread_cond_wait(&P->cv, &P->mu);
    const int err = P->err;
    pthread_mutex_unlock(&P->mu);
    if (err) return HUF_ERROR_FATAL;
    for (int i = 0; i < P->nl[0]; i++)
        if (hipStreamWaitEvent((hipStream_t)0, P->lane[0][i].seg_ev[id % DX_RING], 0) != hipSuccess) { (void)hipGetLastError(); return HUF_ERROR_FATAL; }
    return HUF_ERROR_SUCCESS;
}
static huf_error_t dx_wait_done(dx_pool_t *P, int dir, uint64_t id)
{
    pthread_mutex_lock(&P->mu);
    while (P->seg[dir][id % DX_RING].done_left > 0 && !P->err) pthread_cond_wait(&P->cv, &P->mu);
    const int err = P->err;
    pthread_mutex_unlock(&P->mu);
    return err ? HUF_ERROR_FATAL : HUF_ERROR_SUCCESS;
}
/* everything published so far has been moved (a failed pool: the lanes still count their segments down) */
static void dx_drain(dx_pool_t *P)
{
    pthread_mutex_lock(&P->mu);
    for (int d = 0; d < 2; d++) {
        const uint64_t n = P->published[d];
        for (uint64_t id = n > DX_RING ? n - DX_RING : 0; id < n; id++)
            while (P->seg[d][id % DX_RING].done_left > 0) pthread_cond_wait(&P->cv, &P->mu);
    }
    pthread_mutex_unlock(&P->mu);
}

/* What a call reads from host memory has been written by somebody: its pages are there, and registering pages that are
 * there costs 2 ms per GiB on these boxes (tools/calib/host_link_probe.hip; pages never touched: 45 ms, the faults).  The
 * whole input is registered ONCE, before the first lane moves - a hipHostRegister beside the output lanes' page
 * populating brings both to a crawl (the address-space lock: 29 GiB/s where 50 were measured alone, and two threads
 * that register at once get a fifth of one thread's rate) - and the copies then run straight from the caller's pages:
 * no memcpy into a slot, 2 GiB of memory traffic per GiB and five busy threads less.  Returns the registered base (to
 * hand to dx_unregister_input) or NULL: a read-only mapping, pages somebody else has registered - the staged lanes
 * take the call then. */
static void *dx_register_input(dx_pool_t *P, const void *host, size_t n)
{
    if (!P->can_register || !n) return NULL;
    const page_span_t s = page_span(host, n, 1);     /* (the pages that hold its first and last byte are mapped) */
    if (hipHostRegister((void *)s.lo, (size_t)(s.hi - s.lo), hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return NULL; }
    return (void *)s.lo;
}
static void dx_unregister_input(void *base)
{
    if (base && hipHostUnregister(base) != hipSuccess) (void)hipGetLastError();
}

/* bytes a round: HUF_GPU_ROUND_MB, else a quarter of the call between 16 and 32 MiB (a round much below 8 MiB is a piece
 * or two for ten lanes), more for blocks of 128 KiB to 4 MiB */
static uint64_t dx_round_bytes(uint64_t total, uint64_t blocksize)
{
    static const int env = env_int("HUF_GPU_ROUND_MB", 0, 0, INT_MAX);
    if (env > 0) return (uint64_t)env << 20;
    /* (a round costs about 0.1 ms beside its transfers - its launches and the wait for its length; 64 MiB in rounds of 8 MiB:
     *  3.5 + 3.7 ms, of 16-24 MiB: 2.8-2.9 + 3.2) */
    uint64_t r = (total / 4) & ~(((uint64_t)1 << 20) - 1);
    if (r < ((uint64_t)16 << 20)) r = (uint64_t)16 << 20;
    if (r > ((uint64_t)32 << 20)) r = (uint64_t)32 << 20;
    /* A block is one workgroup's work up to 2 MiB (encode) / 4 MiB (decode): a round of 32 MiB in blocks of 1 MiB - the Python
     * layer's default - is 32 workgroups on 256 CUs, and a round then takes as long as ONE block does (1 GiB of log text: 16-20 ms
     * of an encode's 30 and 25 ms of a decode's 42 were that).  Rounds of at least 128 blocks, 256 MiB at most. */
    if (blocksize > ((uint64_t)128 << 10) && blocksize < ((uint64_t)4 << 20)) {
        uint64_t want = 128 * blocksize;
        if (want > ((uint64_t)256 << 20)) want = (uint64_t)256 << 20;
        if (want > r) r = want;
    }
    return r;
}
#define DX_MIN_BYTES ((uint64_t)32 << 20)      /* below this the rounds are too few to overlap anything */

static huf_error_t d2h_to_memstream(membuf_t *wmem, const void *d_src, size_t n)
{
    TRY(mem_reserve(wmem, n));
    char *dst = (char *)*wmem->buf + wmem->len;
    if (n >= LANE_MIN && lane_count() > 0) {
        TRY(lane_copy(0, (void *)d_src, dst, n));       /* (populates the pages piece by piece, beside the copies) */
    } else {
        prefault(dst, n);
        TRY(hufgpu_memcpy_d2h(g_ctx, dst, d_src, n));
    }
    wmem->len += n;
    return HUF_ERROR_SUCCESS;
}

/* HUF_GPU_DX_TRACE=1: where the calling thread of a duplex call spends its time, one line per call on stderr */
static int dx_trace(void)
{
    static const int on = env_flag("HUF_GPU_DX_TRACE", 0);
    return on;
}
static double dx_now(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
#define DX_T(acc, stmt) do { const double t_ = dx_trace() ? dx_now() : 0.0; stmt; if (dx_trace()) (acc) += dx_now() - t_; } while (0)

static int duplex_enabled(void)
{
    static const int on = env_flag("HUF_GPU_DUPLEX", 1);
    return on;
}

/* room for `count` bytes behind the `pending` bytes that lie behind the stream's contents already (results of earlier
 * rounds, not yet counted in len).  A buffer that has to grow moves: the lanes that write into it finish first. */
static huf_error_t mem_reserve_behind(membuf_t *m, dx_pool_t *P, size_t pending, size_t count)
{
    if (m->cap - m->len >= pending + count) return HUF_ERROR_SUCCESS;
    dx_drain(P);
    m->len += pending;                               /* (what a grown buffer takes along) */
    const huf_error_t rc = mem_reserve(m, count);
    m->len -= pending;
    return rc;
}

/* host -> host, for a binding that has to hand the result over as an object of its own (the
 * Python layer's `bytes`): the destination is fresh memory, so a plain memcpy runs at page-fault
 * speed (256 MiB: 35-40 ms).  Huge-page advice, then every thread makes its part present and copies it. */
typedef struct { char *dst; const char *src; size_t n; } copy_part_t;
static void *copy_part_main(void *arg)
{
    copy_part_t *c = (copy_part_t *)arg;
    prefault_t w = {c->dst, c->n};
    prefault_main(&w);
    memcpy(c->dst, c->src, c->n);
    return NULL;
}

int huf_gpu_copy_out(void *dst, const void *src, size_t n)
{
    if ((!dst || !src) && n) return HUF_ERROR_INVALID_ARGUMENT;
    const int nthreads = prefault_threads();
    if (n < PREFAULT_MIN || nthreads <= 1) {
        if (n) memcpy(dst, src, n);
        return HUF_ERROR_SUCCESS;
    }
    advise_huge(dst, n);
    part_t cut[PARTS_MAX];
    copy_part_t part[PARTS_MAX];
    const int count = split_parts(n, nthreads, cut);
    for (int i = 0; i < count; i++) { part[i].dst = (char *)dst + cut[i].off; part[i].src = (const char *)src + cut[i].off; part[i].n = cut[i].n; }
    run_parts(copy_part_main, part, count);
    return HUF_ERROR_SUCCESS;
}
