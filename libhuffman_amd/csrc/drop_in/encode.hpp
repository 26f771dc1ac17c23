/*
 * drop_in/encode.hpp - huf_encode (src/encoder.c:261-388): round by round through one session, dealt out over several
 * sessions (fanout), or in rounds whose transfers overlap the kernels (duplex).
 */
#define SMALL_CALL_BYTES ((uint64_t)32 << 10)     /* (1 B: 56 -> 31 us, 4 KiB: 78 -> 54; from 64 KiB on the bound-sized copy back costs more than the waits) */

/* HUF_GPU_BATCH_MB, read at every call: MiB per round, `fallback` when it is not set or not positive */
static uint64_t batch_bytes(int fallback)
{
    const int mb = env_int("HUF_GPU_BATCH_MB", 0, 0, INT_MAX);
    return (uint64_t)(mb ? mb : fallback) << 20;
}

static huf_error_t encode_rounds(huf_encoder_t *enc, uint64_t batch, membuf_t *rmem, membuf_t *wmem,
                                 fd_worker_t *rd, fd_worker_t *wr)
{
    const uint64_t length = enc->config->length;
    const uint64_t blocksize = enc->config->blocksize;
    const uint64_t bound = hufgpu_encode_bound(batch, blocksize);
    int round = 0;
    /* a small call between two memory streams: one synchronisation instead of three (hufgpu_encode_small) */
    if (rmem && wmem && length <= SMALL_CALL_BYTES && rmem->len - rmem->off >= length) {
        const uint64_t b8 = ((bound + 7u) & ~7ull) + 8u;
        TRY(grow_host(&g_stage.h_a, &g_stage.h_a_cap, length));
        TRY(grow_host(&g_stage.h_b, &g_stage.h_b_cap, b8));
        memcpy(g_stage.h_a, (const char *)*rmem->buf + rmem->off, length);
        uint64_t out_len = 0;
        const int rc = hufgpu_encode_small(g_ctx, g_stage.h_a, length, blocksize, g_stage.d_a, g_stage.d_b, g_stage.d_b_cap,
                                           g_stage.h_b, g_stage.h_b_cap, &out_len);
        if (rc != HUF_ERROR_SUCCESS) return (huf_error_t)rc;
        rmem->off += length;
        return memwrite(wmem, g_stage.h_b, out_len);
    }
    for (uint64_t done = 0; done < length; round ^= 1) {
        const uint64_t take = (length - done < batch) ? length - done : batch;
        /* one large read per round; a short read is an error exactly like the reference's
         * block read (src/encoder.c:296, src/bufio.c:251-253) */
        int rc = HUF_ERROR_SUCCESS;
        if (rmem) {
            if (rmem->len - rmem->off < take) {
                rmem->off = rmem->len;                          /* what a failed read would have consumed */
                rc = HUF_ERROR_READ_WRITE;
            } else {
                rc = lane_copy(1, g_stage.d_a, (char *)*rmem->buf + rmem->off, take);
                if (rc == HUF_ERROR_SUCCESS) rmem->off += take;
            }
        } else if (rd->started) {
            rc = fd_reader_wait(rd, round, take);
            if (rc == HUF_ERROR_SUCCESS) rc = hufgpu_memcpy_h2d(g_ctx, g_stage.d_a, rd->buf[round], take);
            if (rc == HUF_ERROR_SUCCESS) fd_reader_release(rd, round);   /* the next read starts under the encode */
        } else {
            rc = huf_bufio_read(enc->bufio_reader, g_stage.h_a, take);
            if (rc == HUF_ERROR_SUCCESS) rc = hufgpu_memcpy_h2d(g_ctx, g_stage.d_a, g_stage.h_a, take);
        }
        uint64_t out_len = 0;
        if (rc == HUF_ERROR_SUCCESS)
            rc = hufgpu_encode(g_ctx, g_stage.d_a, take, blocksize, g_stage.d_b, g_stage.d_b_cap, NULL, &out_len, NULL);
        if (rc != HUF_ERROR_SUCCESS) return (huf_error_t)rc;
        if (wmem) {
            TRY(d2h_to_memstream(wmem, g_stage.d_b, out_len));
        } else if (wr->started) {
            TRY(fd_writer_push(wr, g_stage.d_b, out_len));      /* waits for the write of two rounds ago */
        } else {
            TRY(hufgpu_memcpy_d2h(g_ctx, g_stage.h_b, g_stage.d_b, out_len));
            TRY(huf_bufio_write(enc->bufio_writer, g_stage.h_b, out_len));
        }
        done += take;
    }
    (void)bound;
    return HUF_ERROR_SUCCESS;
}

/* how many huf_encode() / huf_decode() calls of this process were spread over several sessions */
static std::atomic<int> g_fanout_decodes(0), g_fanout_encodes(0);
int huf_gpu_fanouts(int *encodes, int *decodes)
{
    if (encodes) *encodes = g_fanout_encodes.load();
    if (decodes) *decodes = g_fanout_decodes.load();
    return g_fanout_encodes.load() + g_fanout_decodes.load();
}

/* One huf_encode() over several sessions (HUF_GPU_DEVICES lists more than one and some are free):
 * memory stream -> memory stream only.  The input is cut into rounds of whole blocks - blocks are
 * independent (src/encoder.c:288-374, reset :360-373), so the stream is the rounds' streams one after
 * the other, byte for byte what one session writes.  Every session runs on a thread of its own:
 * input round to its device, encode, and - once the sizes of all earlier rounds are known - the
 * result to its place in the output.  With sessions on different GPUs the rounds travel over
 * different host links; with two sessions on ONE GPU a round's copy back runs beside the next
 * round's copy in (full duplex).  The output's pages are made present before the first copy (a
 * populate beside running copies fights them for the address-space lock, see d2h_to_memstream). */
typedef struct {
    const char *src;
    char *dst;
    uint64_t length, blocksize, round_bytes, nrounds;
    std::atomic<uint64_t> next;
    uint64_t *out_len;              /* per round, valid once known[k] */
    unsigned char *known;
    unsigned char *done;            /* per round: its stream is in place in dst (written under mu, read after the joins) */
    pthread_mutex_t mu;
    pthread_cond_t cv;
    std::atomic<int> err;
} fanout_t;


typedef struct { fanout_t *f; session_t *session; int extra; } fanout_worker_t;   /* extra: not the call's own session */

#define HUF_MAX_LINKS 64
static pthread_mutex_t g_link_lock[HUF_MAX_LINKS][2];               /* per device: [0] host -> device, [1] device -> host */
static pthread_once_t g_link_once = PTHREAD_ONCE_INIT;
static void link_locks_init(void)
{
    for (int i = 0; i < HUF_MAX_LINKS; i++) {
        pthread_mutex_init(&g_link_lock[i][0], NULL);
        pthread_mutex_init(&g_link_lock[i][1], NULL);
    }
}

static void fanout_fail(fanout_t *f, int err)
{
    pthread_mutex_lock(&f->mu);
    int none = HUF_ERROR_SUCCESS;
    f->err.compare_exchange_strong(none, err);
    pthread_cond_broadcast(&f->cv);
    pthread_mutex_unlock(&f->mu);
}

static void *fanout_main(void *arg)
{
    fanout_worker_t *w = (fanout_worker_t *)arg;
    fanout_t *f = w->f;
    t_session = w->session;                                          /* this thread's g_ctx / g_stage */
    int rc = session_acquire();
    const uint64_t bound = hufgpu_encode_bound(f->round_bytes, f->blocksize);
    if (rc == HUF_ERROR_SUCCESS) rc = grow_dev(&g_stage.d_a, &g_stage.d_a_cap, f->round_bytes);
    if (rc == HUF_ERROR_SUCCESS) rc = grow_dev(&g_stage.d_b, &g_stage.d_b_cap, bound);
    if (rc != HUF_ERROR_SUCCESS && w->extra) {
        /* an EXTRA session that cannot be set up (a device of HUF_GPU_DEVICES without memory left, a context
         * that cannot be created) has taken no round yet: the call goes on with the sessions that work */
        t_session = NULL;
        return NULL;
    }
    while (rc == HUF_ERROR_SUCCESS) {
        if (f->err.load() != HUF_ERROR_SUCCESS) break;                   /* another session failed */
        const uint64_t k = f->next.fetch_add(1);
        if (k >= f->nrounds) break;
        const uint64_t off = k * f->round_bytes;
        const uint64_t take = (f->length - off < f->round_bytes) ? f->length - off : f->round_bytes;
        uint64_t out_len = 0;
        /* sessions on one device take turns per direction: while one copies a result back the next
         * copies its input in (both at once in the SAME direction only share the link, and all
         * sessions would move through their phases in step) */
        pthread_mutex_t *dir = g_link_lock[(unsigned)w->session->device % HUF_MAX_LINKS];
        pthread_mutex_lock(&dir[0]);
        rc = hufgpu_memcpy_h2d(g_ctx, g_stage.d_a, f->src + off, take);
        pthread_mutex_unlock(&dir[0]);
        if (rc == HUF_ERROR_SUCCESS)
            rc = hufgpu_encode(g_ctx, g_stage.d_a, take, f->blocksize, g_stage.d_b, g_stage.d_b_cap, NULL, &out_len, NULL);
        if (rc != HUF_ERROR_SUCCESS) break;
        /* publish this round's size, then wait for the sizes of all rounds in front of it */
        uint64_t before = 0;
        pthread_mutex_lock(&f->mu);
        f->out_len[k] = out_len;
        f->known[k] = 1;
        pthread_cond_broadcast(&f->cv);
        for (;;) {
            uint64_t j = 0;
            before = 0;
            while (j < k && f->known[j]) before += f->out_len[j++];
            if (j == k) break;                                       /* every earlier size is known: this round still lands, */
            if (f->err.load() != HUF_ERROR_SUCCESS) break;           /* even after another session failed behind it */
            pthread_cond_wait(&f->cv, &f->mu);
        }
        uint64_t j2 = 0;
        while (j2 < k && f->known[j2]) j2++;
        const int stop = j2 < k;                                         /* (only possible after a failure) */
        pthread_mutex_unlock(&f->mu);
        if (stop) break;
        pthread_mutex_lock(&dir[1]);
        rc = hufgpu_memcpy_d2h(g_ctx, f->dst + before, g_stage.d_b, out_len);
        pthread_mutex_unlock(&dir[1]);
        if (rc == HUF_ERROR_SUCCESS) {
            pthread_mutex_lock(&f->mu);
            f->done[k] = 1;
            pthread_mutex_unlock(&f->mu);
        }
    }
    if (rc != HUF_ERROR_SUCCESS) fanout_fail(f, rc);
    t_session = NULL;
    return NULL;
}

/* returns 1 when the call was done here (*result = its outcome), 0 when the ordinary path should run */
static int encode_fanout(huf_encoder_t *enc, membuf_t *rmem, membuf_t *wmem, huf_error_t *result)
{
    const uint64_t length = enc->config->length, blocksize = enc->config->blocksize;
    if (!rmem || !wmem || wmem->readonly || g_nsessions < 2) return 0;
    if (rmem->len - rmem->off < length) return 0;                     /* a short input: the ordinary path reports it */
    uint64_t round_bytes = batch_bytes(32);
    if (round_bytes < blocksize) round_bytes = blocksize;
    round_bytes -= round_bytes % blocksize;
    const uint64_t nrounds = (length + round_bytes - 1) / round_bytes;
    if (nrounds < 2) return 0;

    session_t *mine = t_session;
    session_t *extra[HUF_MAX_SESSIONS];
    int nextra = 0;
    while ((uint64_t)nextra + 1 < nrounds && nextra < HUF_MAX_SESSIONS - 1) {
        session_t *s = session_try_extra();
        if (!s) break;
        extra[nextra++] = s;
    }
    if (nextra == 0) return 0;                                        /* every other session is busy: one after the other */
    pthread_once(&g_link_once, link_locks_init);

    uint64_t bound = 0;
    for (uint64_t k = 0; k < nrounds; k++) {
        const uint64_t off = k * round_bytes;
        bound += hufgpu_encode_bound(length - off < round_bytes ? length - off : round_bytes, blocksize);
    }
    fanout_t f;
    f.src = (const char *)*rmem->buf + rmem->off;
    f.length = length;
    f.blocksize = blocksize;
    f.round_bytes = round_bytes;
    f.nrounds = nrounds;
    f.next.store(0);
    f.err.store(HUF_ERROR_SUCCESS);
    f.out_len = (uint64_t *)calloc(nrounds, sizeof(uint64_t));
    f.known = (unsigned char *)calloc(nrounds, 1);
    f.done = (unsigned char *)calloc(nrounds, 1);
    huf_error_t err = (f.out_len && f.known && f.done) ? mem_reserve(wmem, bound) : HUF_ERROR_MEMORY_ALLOCATION;
    if (err == HUF_ERROR_SUCCESS) {
        f.dst = (char *)*wmem->buf + wmem->len;
        prefault(f.dst, (size_t)(length < bound ? length : bound));   /* about as many bytes as the stream will have */
        pthread_mutex_init(&f.mu, NULL);
        pthread_cond_init(&f.cv, NULL);
        fanout_worker_t workers[HUF_MAX_SESSIONS];
        pthread_t th[HUF_MAX_SESSIONS];
        int started = 0;
        for (int i = 0; i < nextra; i++) {
            workers[i + 1].f = &f;
            workers[i + 1].session = extra[i];
            workers[i + 1].extra = 1;
            if (pthread_create(&th[i], NULL, fanout_main, &workers[i + 1]) != 0) break;
            started++;
        }
        workers[0].f = &f;
        workers[0].session = mine;
        workers[0].extra = 0;
        fanout_main(&workers[0]);                                     /* this thread works with the call's own session */
        t_session = mine;
        for (int i = 0; i < started; i++) pthread_join(th[i], NULL);
        pthread_mutex_destroy(&f.mu);
        pthread_cond_destroy(&f.cv);
        err = (huf_error_t)f.err.load();
        /* what the reference's unbuffered writer has delivered when it fails stays delivered: the rounds in
         * front of the first one that is not in place (all of them on success) */
        uint64_t total = 0, p = 0;
        while (p < nrounds && f.done[p]) total += f.out_len[p++];
        if (err == HUF_ERROR_SUCCESS && p < nrounds) err = HUF_ERROR_FATAL;   /* (cannot happen: every round was taken) */
        wmem->len += total;
        rmem->off += (p == nrounds) ? length : p * round_bytes;
        if (err == HUF_ERROR_SUCCESS) g_fanout_encodes.fetch_add(1);
    }
    for (int i = 0; i < nextra; i++) session_release_extra(extra[i]);
    free(f.out_len);
    free(f.known);
    free(f.done);
    *result = err;
    return 1;
}

/* huf_encode() between two memory streams in rounds whose transfers overlap (the comment above dx_lane_main): returns
 * 1 when it took the call (*result = what huf_encode returns), 0 when the call is not of that kind - the caller goes
 * on as before.  Rounds are whole blocks (src/encoder.c:288-374: blocks are independent), the stream is the rounds'
 * streams one after the other; a round that fails ends the call with the rounds in front of it delivered, as
 * encode_rounds does. */
static int encode_duplex(huf_encoder_t *enc, membuf_t *rmem, membuf_t *wmem, huf_error_t *result)
{
    const uint64_t length = enc->config->length, blocksize = enc->config->blocksize;
    if (!rmem || !wmem || !duplex_enabled() || length < DX_MIN_BYTES || rmem->len - rmem->off < length || blocksize == 0) return 0;
    uint64_t R = dx_round_bytes(length, blocksize < ((uint64_t)2 << 20) ? blocksize : 0)   /* (from 2 MiB on the encoder cuts blocks into chunks itself) */;
    if (R < blocksize) R = blocksize;
    R -= R % blocksize;
    if (length <= R + R / 2) return 0;
    dx_pool_t *P = dx_get();
    if (!P) return 0;
    const uint64_t bound = (hufgpu_encode_bound(R, blocksize) + 255u) & ~(uint64_t)255;
    if (grow_dev(&g_stage.d_a, &g_stage.d_a_cap, 2 * R) != HUF_ERROR_SUCCESS ||
        grow_dev(&g_stage.d_b, &g_stage.d_b_cap, 2 * bound) != HUF_ERROR_SUCCESS) return 0;
    if (!wmem->fixed && mem_reserve(wmem, hufgpu_encode_bound(length, blocksize)) != HUF_ERROR_SUCCESS) return 0;
    const uint64_t nr = (length + R - 1) / R;
    char *src = (char *)*rmem->buf + rmem->off;
    char *d_in[2] = {(char *)g_stage.d_a, (char *)g_stage.d_a + R};
    char *d_out[2] = {(char *)g_stage.d_b, (char *)g_stage.d_b + bound};
#define ROUND_BYTES(i) (((i) + 1) * R <= length ? R : length - (i) * R)
    void *const reg = dx_register_input(P, src, length);
    const int direct = reg != NULL;
    const uint64_t in0 = dx_publish(P, 0, src, d_in[0], ROUND_BYTES((uint64_t)0), direct);
    if (nr > 1) (void)dx_publish(P, 0, src + R, d_in[1], ROUND_BYTES((uint64_t)1), direct);
    uint64_t out0 = 0, out_total = 0, done_in = 0;
    huf_error_t err = HUF_ERROR_SUCCESS;
    double t_in = 0, t_out = 0, t_k = 0, t_end = 0;
    const double t_start = dx_trace() ? dx_now() : 0.0;
    for (uint64_t i = 0; i < nr; i++) {
        DX_T(t_in, err = dx_wait_issued(P, in0 + i));
        if (err == HUF_ERROR_SUCCESS && i >= 2) DX_T(t_out, err = dx_wait_done(P, 1, out0 + i - 2));      /* the round that used this output buffer */
        if (err != HUF_ERROR_SUCCESS) break;
        uint64_t out_len = 0;
        DX_T(t_k, err = (huf_error_t)hufgpu_encode(g_ctx, d_in[i & 1], ROUND_BYTES(i), blocksize, d_out[i & 1], bound, NULL, &out_len, NULL));
        done_in = (i + 1 < nr) ? (i + 1) * R : length;                                       /* (what a failed round has consumed, too) */
        if (err != HUF_ERROR_SUCCESS) break;
        err = mem_reserve_behind(wmem, P, out_total, out_len);
        if (err != HUF_ERROR_SUCCESS) break;
        const uint64_t id = dx_publish(P, 1, (char *)*wmem->buf + wmem->len + out_total, d_out[i & 1], out_len);
        if (i == 0) out0 = id;
        out_total += out_len;
        if (i + 2 < nr) (void)dx_publish(P, 0, src + (i + 2) * R, d_in[i & 1], ROUND_BYTES(i + 2), direct);   /* its kernels are done: the buffer is free */
    }
#undef ROUND_BYTES
    DX_T(t_end, dx_drain(P));
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); if (err == HUF_ERROR_SUCCESS) err = HUF_ERROR_FATAL; }   /* (copies of rounds a failure left behind) */
    dx_unregister_input(reg);
    if (dx_trace())
        fprintf(stderr, "encode_duplex: %llu rounds of %llu MiB, %.2f ms: waiting for input %.2f, for an output buffer %.2f, kernels (+ their wait) %.2f, the last copies %.2f; input registered=%d lanes %d/%d\n",
                (unsigned long long)nr, (unsigned long long)(R >> 20), (dx_now() - t_start) * 1e3, t_in * 1e3, t_out * 1e3, t_k * 1e3, t_end * 1e3, direct, P->nl[0], P->nl[1]);
    if (err == HUF_ERROR_SUCCESS && P->err) err = HUF_ERROR_FATAL;
    rmem->off += done_in;
    wmem->len += out_total;
    *result = err;
    return 1;
}

static huf_error_t encode_locked(huf_encoder_t *enc)
{
    const uint64_t length = enc->config->length;
    const uint64_t blocksize = enc->config->blocksize;
    if (blocksize > HUFGPU_MAX_BLOCK) {
        fprintf(stderr, "libhuffman: blocksize %llu exceeds the GPU kernel limit (%llu)\n",
                (unsigned long long)blocksize, (unsigned long long)HUFGPU_MAX_BLOCK);
        return HUF_ERROR_INVALID_ARGUMENT;
    }
    TRY(session_acquire());

    membuf_t *rmem = zero_copy_enabled() ? own_memstream_reader(enc->config->reader) : NULL;
    membuf_t *wmem = zero_copy_enabled() ? own_memstream_writer(enc->config->writer) : NULL;
    const int rfd = (rmem || !zero_copy_enabled()) ? -1 : own_fd_of(enc->config->reader, 0);
    const int wfd = (wmem || !zero_copy_enabled()) ? -1 : own_fd_of(enc->config->writer, 1);
    {
        huf_error_t fan = HUF_ERROR_SUCCESS;
        if (encode_fanout(enc, rmem, wmem, &fan) || encode_duplex(enc, rmem, wmem, &fan))
            return fan != HUF_ERROR_SUCCESS ? fan : huf_bufio_read_writer_flush(enc->bufio_writer);
    }

    /* bytes per round: whole blocks; smaller rounds when descriptor I/O runs next to the GPU
     * (the first read and the last write are not hidden) */
    uint64_t batch = batch_bytes((rfd >= 0 || wfd >= 0) ? 32 : 256);
    if (batch < blocksize) batch = blocksize;
    batch -= batch % blocksize;
    if (batch > length) batch = length;

    const uint64_t bound = hufgpu_encode_bound(batch, blocksize);
    if (!rmem) TRY(grow_host(&g_stage.h_a, &g_stage.h_a_cap, rfd >= 0 ? 2 * batch : batch));
    if (!wmem) TRY(grow_host(&g_stage.h_b, &g_stage.h_b_cap, wfd >= 0 ? 2 * bound : bound));
    TRY(grow_dev(&g_stage.d_a, &g_stage.d_a_cap, batch));
    TRY(grow_dev(&g_stage.d_b, &g_stage.d_b_cap, bound));

    fd_worker_t rd, wr;
    memset(&rd, 0, sizeof(rd));
    memset(&wr, 0, sizeof(wr));
    huf_error_t err = HUF_ERROR_SUCCESS;
    if (rfd >= 0) {
        rd.fd = rfd;
        rd.buf[0] = (char *)g_stage.h_a;
        rd.buf[1] = (char *)g_stage.h_a + batch;
        rd.remaining = length;
        rd.batch = (size_t)batch;
        err = fd_worker_start(&rd);
    }
    if (wfd >= 0 && err == HUF_ERROR_SUCCESS) {
        wr.fd = wfd;
        wr.writer = 1;
        wr.buf[0] = (char *)g_stage.h_b;
        wr.buf[1] = (char *)g_stage.h_b + bound;
        wr.batch = (size_t)bound;
        err = fd_worker_start(&wr);
    }
    if (err == HUF_ERROR_SUCCESS) err = encode_rounds(enc, batch, rmem, wmem, &rd, &wr);
    (void)fd_worker_finish(&rd);                                  /* its failures surfaced with their round */
    const huf_error_t werr = fd_worker_finish(&wr);               /* results of complete rounds still go out */
    if (err == HUF_ERROR_SUCCESS) err = werr;
    if (err != HUF_ERROR_SUCCESS) return err;
    return huf_bufio_read_writer_flush(enc->bufio_writer);        /* encoder.c:377 */
}

huf_error_t huf_encode(const huf_config_t *config)
{
    GUARD(config);
    huf_encoder_t *enc = NULL;
    TRY(huf_encoder_init(&enc, config));
    huf_error_t err = HUF_ERROR_SUCCESS;
    if (enc->config->length) {                    /* length 0: nothing is read or written */
        session_enter();
        err = encode_locked(enc);
        session_leave();
    }
    huf_encoder_free(&enc);
    return err;
}
