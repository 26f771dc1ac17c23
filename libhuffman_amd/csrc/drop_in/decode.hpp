/*
 * drop_in/decode.hpp - huf_decode (src/decoder.c:201-287) and huf_gpu_decode_blocks: from a descriptor in rounds, dealt
 * out over several sessions (fanout), in rounds whose transfers overlap the kernels (duplex), or in one piece.
 */
#define SMALL_DECODE_BYTES ((uint64_t)128 << 10)  /* (streams of up to 128 KiB decode in one workgroup's chain with one wait - 64 KiB: 141 -> ~70 us) */

/* ------------------------------------------------------------------ huf_decode (src/decoder.c:201-287) */
static huf_error_t read_upto(huf_read_writer_t *rw, uint8_t *dst, size_t want, size_t *got)
{
    size_t total = 0;
    while (total < want) {
        size_t n = want - total;
        TRY(rw->read(rw->stream, dst + total, &n));
        if (!n) break;
        total += n;
    }
    *got = total;
    return HUF_ERROR_SUCCESS;
}

/* the helper thread's next piece (it asked for `want` bytes) -> behind the `*loaded` stream bytes on the device */
static huf_error_t fd_reader_to_device(fd_worker_t *rd, int *rslot, uint64_t want, uint64_t *loaded, int *eof)
{
    const int k = *rslot;
    pthread_mutex_lock(&rd->mu);
    while (!rd->full[k]) pthread_cond_wait(&rd->cv, &rd->mu);
    const size_t got = rd->len[k];
    const huf_error_t rerr = rd->err;
    pthread_mutex_unlock(&rd->mu);
    if (rerr != HUF_ERROR_SUCCESS) return rerr;
    TRY(hufgpu_memcpy_h2d(g_ctx, (char *)g_stage.d_a + *loaded, rd->buf[k], got));
    fd_reader_release(rd, k);
    *rslot = k ^ 1;
    *loaded += got;
    if (got < want) *eof = 1;
    return HUF_ERROR_SUCCESS;
}

/* Decode with the input on a huf_fdopen() descriptor: the file is read by a helper thread in
 * pieces that go to the device as they arrive, and the stream is decoded in rounds of `piece`
 * compressed bytes - the block loop of src/decoder.c:218 cut at block boundaries: a round starts
 * where the previous one stopped and runs while fewer than its share of bytes is consumed, which
 * is the reference's loop condition with more check points.  Each round's output leaves through
 * the writer (a helper thread as well when that is a descriptor) while the next pieces are read
 * and decoded.  A round whose last block needs bytes that are not there yet is repeated once
 * they are; past `length` the descriptor is asked for more like the reference's on-demand reads. */
static huf_error_t decode_rounds_fd(huf_decoder_t *dec, fd_worker_t *rd, membuf_t *wmem, fd_worker_t *wr,
                                    uint64_t piece, uint32_t flags)
{
    const uint64_t length = dec->config->length;
    const uint64_t margin = 4u << 20;            /* what a round may look ahead before it is worth starting */
    uint64_t loaded = 0;                         /* bytes of the stream on the device (g_stage.d_a) */
    uint64_t requested = 0;                      /* of `length`, by the helper thread */
    int rslot = 0, eof = 0;
    uint64_t pos = 0;
    uint64_t out_cap = (piece + margin) * 8 + (1u << 20);
    TRY(grow_dev(&g_stage.d_a, &g_stage.d_a_cap, (size_t)length + 16));

    while (pos < length) {
        const uint64_t round_len = (length - pos < piece) ? length - pos : piece;
        /* input up to the round's end plus the margin, or all there is */
        while (!eof && requested < length && loaded < pos + round_len + margin) {
            TRY(fd_reader_to_device(rd, &rslot, (length - requested < piece) ? length - requested : piece, &loaded, &eof));
            requested = (length - requested < piece) ? length : requested + piece;
        }
        const uint64_t avail = loaded - pos;
        /* the round's bytes at an aligned address (the parallel block discovery wants that) */
        TRY(grow_dev(&g_stage.d_c, &g_stage.d_c_cap, (size_t)avail + 16));
        TRY(hufgpu_memcpy_d2d(g_ctx, g_stage.d_c, (const char *)g_stage.d_a + pos, avail));
        TRY(grow_dev(&g_stage.d_b, &g_stage.d_b_cap, out_cap));
        uint64_t raw = 0, used = 0;
        int rc = hufgpu_decode_stream(g_ctx, g_stage.d_c, avail, round_len, g_stage.d_b, g_stage.d_b_cap, flags, &raw, &used, NULL);
        if (rc == HUF_ERROR_MEMORY_ALLOCATION && out_cap < ((uint64_t)1 << 40)) {   /* output did not fit: enlarge */
            out_cap *= 4;
            continue;
        }
        if (rc == HUF_ERROR_READ_WRITE) {
            if (!eof && requested < length) {            /* more of the stream is on its way: take a piece, again */
                TRY(fd_reader_to_device(rd, &rslot, (length - requested < piece) ? length - requested : piece, &loaded, &eof));
                requested = (length - requested < piece) ? length : requested + piece;
                continue;
            }
            if (!eof) {                                   /* maybe the descriptor holds more than `length` */
                const size_t more_want = loaded < 65536 ? 65536 : (size_t)loaded;
                TRY(grow_dev_keep(&g_stage.d_a, &g_stage.d_a_cap, (size_t)loaded + more_want + 16, (size_t)loaded));
                size_t more = 0;
                while (more < more_want) {                /* the helper thread has finished: read here */
                    size_t n = more_want - more < rd->batch ? more_want - more : rd->batch;
                    const size_t asked = n;
                    TRY(fdread(&rd->fd, rd->buf[0], &n));
                    TRY(hufgpu_memcpy_h2d(g_ctx, (char *)g_stage.d_a + loaded + more, rd->buf[0], n));
                    more += n;
                    if (n < asked) { eof = 1; break; }
                }
                loaded += more;
                if (more) continue;
            }
        }
        /* bytes of the blocks that decoded completely are delivered even when a later block
         * fails, as the reference's unbuffered writer would have done */
        if (raw && wmem) {
            TRY(d2h_to_memstream(wmem, g_stage.d_b, raw));
        } else if (raw && wr->started) {
            TRY(fd_writer_push(wr, g_stage.d_b, raw));
        } else if (raw) {
            TRY(grow_host(&g_stage.h_b, &g_stage.h_b_cap, raw));
            TRY(hufgpu_memcpy_d2h(g_ctx, g_stage.h_b, g_stage.d_b, raw));
            TRY(huf_bufio_write(dec->bufio_writer, g_stage.h_b, raw));
        }
        if (rc != HUF_ERROR_SUCCESS) return (huf_error_t)rc;
        pos += used;
    }
    return HUF_ERROR_SUCCESS;
}

static huf_error_t decode_from_fd(huf_decoder_t *dec, int rfd, membuf_t *wmem, int wfd, uint32_t flags)
{
    const uint64_t length = dec->config->length;
    uint64_t piece = batch_bytes(32);
    if (piece > length) piece = length;
    if (piece < 65536) piece = 65536;                             /* also the size of the reads past `length` */
    TRY(grow_host(&g_stage.h_a, &g_stage.h_a_cap, 2 * piece));
    if (wfd >= 0) TRY(grow_host(&g_stage.h_b, &g_stage.h_b_cap, 2 * piece));

    fd_worker_t rd, wr;
    memset(&rd, 0, sizeof(rd));
    memset(&wr, 0, sizeof(wr));
    rd.fd = rfd;
    rd.buf[0] = (char *)g_stage.h_a;
    rd.buf[1] = (char *)g_stage.h_a + piece;
    rd.remaining = length;
    rd.batch = (size_t)piece;
    rd.eof_ok = 1;
    huf_error_t err = fd_worker_start(&rd);
    if (wfd >= 0 && err == HUF_ERROR_SUCCESS) {
        wr.fd = wfd;
        wr.writer = 1;
        wr.buf[0] = (char *)g_stage.h_b;
        wr.buf[1] = (char *)g_stage.h_b + piece;
        wr.batch = (size_t)piece;
        err = fd_worker_start(&wr);
    }
    if (err == HUF_ERROR_SUCCESS) err = decode_rounds_fd(dec, &rd, wmem, &wr, piece, flags);
    (void)fd_worker_finish(&rd);
    const huf_error_t werr = fd_worker_finish(&wr);               /* what was delivered before a failure still goes out */
    if (err == HUF_ERROR_SUCCESS) err = werr;
    if (err != HUF_ERROR_SUCCESS) return err;                     /* no flush on the error path (decoder.c:278-286) */
    return huf_bufio_read_writer_flush(dec->bufio_writer);
}

/* One huf_decode() over several sessions (the twin of encode_fanout): memory stream -> memory stream, sessions
 * free.  Blocks are independent once they are found (src/decoder.c:218-276), and finding them is a device job
 * of a few milliseconds per GiB (hufgpu_block_index: every candidate header probed count-only, the chain
 * walked).  So: the stream goes to the call's own device, its block index comes back, the blocks are dealt out
 * in contiguous ranges balanced by COMPRESSED bytes, and every session - a thread of its own -
 * takes its range of the stream from host memory, decodes it with the indexed kernels and writes its output
 * where it belongs (the sum of the block_len fields in front of it).  Anything unusual - a stream the walk
 * cannot validate to its end, an error in any range - leaves the whole call to the ordinary path, which
 * reports what the reference reports; nothing has been committed by then. */

typedef struct {
    const char *src;                /* the stream in host memory */
    char *dst;                      /* the output's place in the writer's buffer */
    const uint64_t *offs;           /* nblocks + 1 header offsets (host) */
    const uint64_t *outoff;         /* nblocks + 1 output offsets (host) */
    uint64_t b0, b1;                /* this worker's blocks */
    uint32_t flags;
    session_t *session;
    int own;                        /* the call's own session: the stream is already on its device (at d_a) */
    const uint64_t *d_index;        /* own: the device index */
    int rc;
} dfan_worker_t;

static void *dfan_main(void *arg)
{
    dfan_worker_t *w = (dfan_worker_t *)arg;
    w->rc = HUF_ERROR_SUCCESS;
    if (w->b1 <= w->b0) return NULL;
    session_t *const before = t_session;
    t_session = w->session;
    int rc = session_acquire();
    const uint64_t nb = w->b1 - w->b0;
    const uint64_t s0 = w->offs[w->b0], s1 = w->offs[w->b1];
    const uint64_t raw = w->outoff[w->b1] - w->outoff[w->b0];
    pthread_mutex_t *dir = g_link_lock[(unsigned)w->session->device % HUF_MAX_LINKS];
    uint64_t got = 0;
    if (rc == HUF_ERROR_SUCCESS) rc = grow_dev(&g_stage.d_b, &g_stage.d_b_cap, raw + 16);
    if (rc == HUF_ERROR_SUCCESS && w->own) {
        rc = hufgpu_decode(g_ctx, g_stage.d_a, s1, w->d_index + w->b0, nb, g_stage.d_b, g_stage.d_b_cap, w->flags, &got, NULL);
    } else if (rc == HUF_ERROR_SUCCESS) {
        uint64_t *rel = (uint64_t *)malloc((nb + 1) * sizeof(uint64_t));
        if (!rel) rc = HUF_ERROR_MEMORY_ALLOCATION;
        if (rc == HUF_ERROR_SUCCESS) rc = grow_dev(&g_stage.d_a, &g_stage.d_a_cap, s1 - s0 + 16);
        if (rc == HUF_ERROR_SUCCESS) rc = grow_dev(&g_stage.d_c, &g_stage.d_c_cap, (nb + 1) * sizeof(uint64_t));
        if (rc == HUF_ERROR_SUCCESS) {
            for (uint64_t i = 0; i <= nb; i++) rel[i] = w->offs[w->b0 + i] - s0;
            pthread_mutex_lock(&dir[0]);
            rc = hufgpu_memcpy_h2d(g_ctx, g_stage.d_a, w->src + s0, s1 - s0);
            if (rc == HUF_ERROR_SUCCESS) rc = hufgpu_memcpy_h2d(g_ctx, g_stage.d_c, rel, (nb + 1) * sizeof(uint64_t));
            pthread_mutex_unlock(&dir[0]);
        }
        if (rc == HUF_ERROR_SUCCESS)
            rc = hufgpu_decode(g_ctx, g_stage.d_a, s1 - s0, (const uint64_t *)g_stage.d_c, nb, g_stage.d_b, g_stage.d_b_cap, w->flags,
                               &got, NULL);
        free(rel);
    }
    if (rc == HUF_ERROR_SUCCESS && got != raw) rc = HUF_ERROR_FATAL;       /* (the block_len fields said otherwise) */
    if (rc == HUF_ERROR_SUCCESS) {
        pthread_mutex_lock(&dir[1]);
        rc = hufgpu_memcpy_d2h(g_ctx, w->dst + w->outoff[w->b0], g_stage.d_b, raw);
        pthread_mutex_unlock(&dir[1]);
    }
    w->rc = rc;
    t_session = before;
    return NULL;
}

/* returns 1 when the call was done here (*result = its outcome), 0 when the ordinary path should run */
static int decode_fanout(huf_decoder_t *dec, membuf_t *rmem, membuf_t *wmem, uint32_t flags, huf_error_t *result)
{
    const uint64_t length = dec->config->length;
    if (!rmem || !wmem || wmem->readonly || g_nsessions < 2) return 0;
    if (rmem->len - rmem->off < length) return 0;
    const int min_mb = env_int("HUF_GPU_FANOUT_MIN_MB", 0, 0, INT_MAX);     /* (read at every call) */
    const uint64_t min_bytes = (uint64_t)(min_mb ? min_mb : 64) << 20;
    if (length < min_bytes) return 0;
    session_t *mine = t_session;
    session_t *extra[HUF_MAX_SESSIONS];
    int nextra = 0;
    while (nextra < HUF_MAX_SESSIONS - 1) {
        session_t *s = session_try_extra();
        if (!s) break;
        extra[nextra++] = s;
    }
    if (nextra == 0) return 0;
    pthread_once(&g_link_once, link_locks_init);
    const char *src = (const char *)*rmem->buf + rmem->off;
    uint64_t *offs = NULL, *outoff = NULL;
    int done = 0;
    do {
        /* the stream on the call's own device, and its block index */
        if (grow_dev(&g_stage.d_a, &g_stage.d_a_cap, length + 16) != HUF_ERROR_SUCCESS) break;
        if (hufgpu_memcpy_h2d(g_ctx, g_stage.d_a, src, length) != HUF_ERROR_SUCCESS) break;
        const uint64_t *d_index = NULL;
        uint64_t nb = 0, used = 0;
        if (hufgpu_block_index(g_ctx, g_stage.d_a, length, length, flags, &d_index, &nb, &used, NULL) != HUF_ERROR_SUCCESS) break;
        if (nb < 2 || used != length) break;                          /* not validated to its end: the ordinary path */
        offs = (uint64_t *)malloc((nb + 1) * sizeof(uint64_t));
        outoff = (uint64_t *)malloc((nb + 1) * sizeof(uint64_t));
        if (!offs || !outoff) break;
        if (hufgpu_memcpy_d2h(g_ctx, offs, d_index, (nb + 1) * sizeof(uint64_t)) != HUF_ERROR_SUCCESS) break;
        outoff[0] = 0;
        int sane = offs[0] == 0 && offs[nb] == length;
        for (uint64_t b = 0; b < nb && sane; b++) {
            if (offs[b + 1] < offs[b] + 10 || offs[b + 1] > length) { sane = 0; break; }
            uint64_t bl;
            memcpy(&bl, src + offs[b], sizeof(bl));                   /* block_len, little-endian (src/encoder.c:325) */
            if (bl > ((uint64_t)1 << 40)) { sane = 0; break; }
            outoff[b + 1] = outoff[b] + bl;
        }
        if (!sane) break;
        const uint64_t total = outoff[nb];
        if (mem_reserve(wmem, total) != HUF_ERROR_SUCCESS) break;
        char *dst = (char *)*wmem->buf + wmem->len;
        prefault(dst, (size_t)total);
        /* contiguous block ranges, balanced by compressed bytes: worker w takes the blocks whose header lies in
         * its share of the stream */
        const int nw = nextra + 1;
        dfan_worker_t workers[HUF_MAX_SESSIONS];
        int created[HUF_MAX_SESSIONS];
        pthread_t th[HUF_MAX_SESSIONS];
        uint64_t b = 0;
        for (int w = 0; w < nw; w++) {
            const uint64_t want = (uint64_t)(((unsigned __int128)length * (unsigned)(w + 1)) / (unsigned)nw);
            uint64_t e = b;
            while (e < nb && (w == nw - 1 || offs[e] < want)) e++;
            workers[w].src = src; workers[w].dst = dst; workers[w].offs = offs; workers[w].outoff = outoff;
            workers[w].b0 = b; workers[w].b1 = e; workers[w].flags = flags;
            workers[w].session = (w == 0) ? mine : extra[w - 1];
            workers[w].own = (w == 0);
            workers[w].d_index = d_index;
            workers[w].rc = HUF_ERROR_SUCCESS;
            created[w] = 0;
            b = e;
        }
        for (int w = 1; w < nw; w++) {
            if (pthread_create(&th[w], NULL, dfan_main, &workers[w]) == 0) created[w] = 1;
            else workers[w].rc = HUF_ERROR_FATAL;
        }
        dfan_main(&workers[0]);
        t_session = mine;
        int ok = workers[0].rc == HUF_ERROR_SUCCESS;
        for (int w = 1; w < nw; w++) {
            if (created[w]) pthread_join(th[w], NULL);
            ok = ok && workers[w].rc == HUF_ERROR_SUCCESS;
        }
        if (!ok) break;                                               /* nothing committed: the ordinary path decides */
        wmem->len += total;
        rmem->off += length;
        g_fanout_decodes.fetch_add(1);
        *result = huf_bufio_read_writer_flush(dec->bufio_writer);
        done = 1;
    } while (0);
    free(offs);
    free(outoff);
    for (int i = 0; i < nextra; i++) session_release_extra(extra[i]);
    return done;
}

/* huf_decode() between two memory streams, the same way: the stream goes to the device segment by segment, is decoded in
 * rounds of HUF_GPU_ROUND_MB compressed bytes cut at block boundaries (decode_rounds_fd's loop: the block loop of
 * src/decoder.c:218 with more check points) and every round's output leaves while the next is decoded.  Returns 1 when
 * it took the call.  ANYTHING unusual - an error in any round, a last block that wants bytes beyond `length`, an output
 * that does not fit - leaves the call to the ordinary path (returns 0 with nothing committed), which reports what the
 * reference reports. */
static int decode_duplex(huf_decoder_t *dec, membuf_t *rmem, membuf_t *wmem, uint32_t flags, huf_error_t *result)
{
    if (!rmem || !wmem || !duplex_enabled()) return 0;
    const uint64_t length = dec->config->length;
    const uint64_t left = rmem->len - rmem->off;
    const uint64_t total = length < left ? length : left;
    /* (the first block's length field stands for the stream's block size: a hint for the rounds' size, nothing else) */
    uint64_t first_len = 0;
    if (total >= 8) memcpy(&first_len, (const char *)*rmem->buf + rmem->off, 8);
    const uint64_t R = dx_round_bytes(total, first_len);
    if (total < DX_MIN_BYTES || total <= R + R / 2) return 0;
    dx_pool_t *P = dx_get();
    if (!P) return 0;
    const uint64_t margin = 4u << 20;                /* what a round may look ahead (its last block's end) */
    const uint64_t out_cap = ((R + margin) * 8 + (1u << 20) + 255u) & ~(uint64_t)255;
    if (grow_dev(&g_stage.d_a, &g_stage.d_a_cap, total + 16) != HUF_ERROR_SUCCESS ||
        grow_dev(&g_stage.d_b, &g_stage.d_b_cap, 2 * out_cap) != HUF_ERROR_SUCCESS ||
        grow_dev(&g_stage.d_c, &g_stage.d_c_cap, R + margin + 16) != HUF_ERROR_SUCCESS) return 0;
    if (!wmem->fixed && mem_reserve(wmem, total + total / 4 + (1u << 20)) != HUF_ERROR_SUCCESS) return 0;
    char *src = (char *)*rmem->buf + rmem->off;
    char *d_out[2] = {(char *)g_stage.d_b, (char *)g_stage.d_b + out_cap};
    void *const reg = dx_register_input(P, src, total);
    const int direct = reg != NULL;
    const uint64_t nseg = (total + R - 1) / R;
    uint64_t pub = 0, waited = 0, loaded = 0, in0 = 0;   /* input segments published / the kernels' stream waits for / their bytes */
    uint64_t pos = 0, out_total = 0, out0 = 0, rounds = 0;
    int ok = 1;
    double t_in = 0, t_out = 0, t_k = 0, t_cp = 0, t_end = 0;
    const double t_start = dx_trace() ? dx_now() : 0.0;
    while (ok && pos < total) {
        const uint64_t round_len = (total - pos < R) ? total - pos : R;
        uint64_t need = pos + round_len + margin;
        if (need > total) need = total;
        uint64_t raw = 0, used = 0;
        for (;;) {
            while (ok && loaded < need) {            /* (at most three segments ahead of what has been asked for) */
                while (pub < nseg && pub < waited + 3) {
                    const uint64_t n = (pub + 1) * R <= total ? R : total - pub * R;
                    const uint64_t id = dx_publish(P, 0, src + pub * R, (char *)g_stage.d_a + pub * R, n, direct);
                    if (pub == 0) in0 = id;
                    pub++;
                }
                huf_error_t we = HUF_ERROR_SUCCESS;
                DX_T(t_in, we = dx_wait_issued(P, in0 + waited));
                if (we != HUF_ERROR_SUCCESS) { ok = 0; break; }
                waited++;
                loaded = waited * R < total ? waited * R : total;
            }
            if (!ok) break;
            const uint64_t avail = (loaded - pos < R + margin) ? loaded - pos : R + margin;   /* (whole segments arrive: more than was asked for) */
            /* the round's bytes at an aligned address (the parallel block discovery wants that); the buffer two rounds back is free */
            int rc = HUF_ERROR_SUCCESS;
            DX_T(t_cp, rc = hufgpu_memcpy_d2d(g_ctx, g_stage.d_c, (const char *)g_stage.d_a + pos, avail));
            if (rc != HUF_ERROR_SUCCESS) { ok = 0; break; }
            if (rounds >= 2) DX_T(t_out, rc = dx_wait_done(P, 1, out0 + rounds - 2));
            if (rc != HUF_ERROR_SUCCESS) { ok = 0; break; }
            DX_T(t_k, rc = hufgpu_decode_stream(g_ctx, g_stage.d_c, avail, round_len, d_out[rounds & 1], out_cap, flags, &raw, &used, NULL));
            /* (a round that already looks at all it may - R + margin bytes - and still wants more holds a block longer than
             *  that: more segments cannot help it, the ordinary path takes the call at once instead of loading every
             *  remaining segment and decoding in vain each time) */
            if (rc == HUF_ERROR_READ_WRITE && loaded < total && avail < R + margin) {          /* the last block wants more of the stream: it is on its way */
                need = loaded + R < total ? loaded + R : total;
                continue;
            }
            if (rc != HUF_ERROR_SUCCESS || used == 0) ok = 0;
            break;
        }
        if (!ok) break;
        if (raw) {
            if (mem_reserve_behind(wmem, P, out_total, raw) != HUF_ERROR_SUCCESS) { ok = 0; break; }
            const uint64_t id = dx_publish(P, 1, (char *)*wmem->buf + wmem->len + out_total, d_out[rounds & 1], raw);
            if (rounds == 0) out0 = id;
            out_total += raw;
            rounds++;
        }
        pos += used;
    }
    DX_T(t_end, dx_drain(P));
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); ok = 0; }           /* (input segments still on their way) */
    dx_unregister_input(reg);
    if (dx_trace())
        fprintf(stderr, "decode_duplex: %llu rounds of %llu MiB, %.2f ms: waiting for input %.2f, for an output buffer %.2f, the round's copy %.2f, kernels (+ their waits) %.2f, the last copies %.2f; ok=%d\n",
                (unsigned long long)rounds, (unsigned long long)(R >> 20), (dx_now() - t_start) * 1e3, t_in * 1e3, t_out * 1e3, t_cp * 1e3, t_k * 1e3, t_end * 1e3, ok);
    if (!ok || P->err) return 0;                                                               /* nothing committed: the ordinary path takes the call */
    rmem->off += pos;
    wmem->len += out_total;
    *result = huf_bufio_read_writer_flush(dec->bufio_writer);
    return 1;
}

/* pieces = NULL: huf_decode().  pieces != NULL: huf_gpu_decode_blocks() - only the blocks that lie
 * completely inside `length` bytes, *pieces = their stream bytes, a cut-off last block is no error. */
static huf_error_t decode_locked(huf_decoder_t *dec, uint64_t *pieces)
{
    const uint64_t length = dec->config->length;
    TRY(session_acquire());
    const uint32_t flags = relaxed_tree() ? HUFGPU_RELAXED_TREE : HUFGPU_STRICT_TREE;
    if (!pieces && zero_copy_enabled() && own_fd_of(dec->config->reader, 0) >= 0) {
        membuf_t *wm = own_memstream_writer(dec->config->writer);
        return decode_from_fd(dec, own_fd_of(dec->config->reader, 0), wm, wm ? -1 : own_fd_of(dec->config->writer, 1), flags);
    }

    /* The reference pulls bytes on demand and may run past `length` to finish the last block
     * (src/decoder.c:218); here: take `length` bytes, and if the device reports that a block
     * needs more input, ask the reader for more and decode again. */
    membuf_t *rmem = zero_copy_enabled() ? own_memstream_reader(dec->config->reader) : NULL;
    membuf_t *wmem = zero_copy_enabled() ? own_memstream_writer(dec->config->writer) : NULL;
    if (!pieces) {
        huf_error_t fan = HUF_ERROR_SUCCESS;
        if (decode_fanout(dec, rmem, wmem, flags, &fan) || decode_duplex(dec, rmem, wmem, flags, &fan)) return fan;
    }
    /* a small call between two memory streams: one synchronisation instead of three (hufgpu_decode_small).  Anything but
     * a clean decode - an error, a last block that wants bytes behind `length` - goes on below as if nothing had happened */
    if (!pieces && rmem && wmem && length <= SMALL_DECODE_BYTES && rmem->len - rmem->off >= length) {
        const uint64_t out_cap = (uint64_t)length * 8 + 64;
        const uint64_t h_need = ((out_cap + 7u) & ~7ull) + 64u;
        if (grow_host(&g_stage.h_a, &g_stage.h_a_cap, (size_t)length) == HUF_ERROR_SUCCESS &&
            grow_host(&g_stage.h_b, &g_stage.h_b_cap, (size_t)h_need) == HUF_ERROR_SUCCESS &&
            grow_dev(&g_stage.d_a, &g_stage.d_a_cap, (size_t)length + 16) == HUF_ERROR_SUCCESS &&
            grow_dev(&g_stage.d_b, &g_stage.d_b_cap, (size_t)out_cap) == HUF_ERROR_SUCCESS) {
            memcpy(g_stage.h_a, (const char *)*rmem->buf + rmem->off, (size_t)length);
            uint64_t raw = 0, used = 0;
            const int rc = hufgpu_decode_small(g_ctx, g_stage.h_a, length, length, flags, g_stage.d_a, g_stage.d_b, out_cap,
                                               g_stage.h_b, g_stage.h_b_cap, &raw, &used);
            if (rc == HUF_ERROR_FATAL) return HUF_ERROR_FATAL;
            if (rc == HUF_ERROR_SUCCESS) {
                rmem->off += (size_t)(used < length ? used : length);
                if (raw) TRY(memwrite(wmem, g_stage.h_b, (size_t)raw));
                return huf_bufio_read_writer_flush(dec->bufio_writer);
            }
        }
    }
    size_t avail = 0;
    const char *in_ptr = NULL;              /* host bytes [0, avail) of the input */
    const size_t start_off = rmem ? rmem->off : 0;
    if (rmem) {
        const size_t left = rmem->len - rmem->off;
        in_ptr = (const char *)*rmem->buf + rmem->off;
        avail = (size_t)length < left ? (size_t)length : left;
        rmem->off += avail;
    } else {
        size_t cap_in = (size_t)length + 4096;
        TRY(grow_host(&g_stage.h_a, &g_stage.h_a_cap, cap_in));
        TRY(read_upto(dec->config->reader, (uint8_t *)g_stage.h_a, (size_t)length, &avail));
    }

    uint64_t out_cap = (uint64_t)avail * 8 + (1u << 20);
    for (;;) {
        TRY(grow_dev(&g_stage.d_a, &g_stage.d_a_cap, avail + 16));
        TRY(grow_dev(&g_stage.d_b, &g_stage.d_b_cap, out_cap));
        uint64_t raw = 0, used = 0;
        int rc = rmem ? (int)lane_copy(1, g_stage.d_a, (void *)in_ptr, avail) : hufgpu_memcpy_h2d(g_ctx, g_stage.d_a, g_stage.h_a, avail);
        if (rc == HUF_ERROR_SUCCESS)
            rc = hufgpu_decode_stream(g_ctx, g_stage.d_a, avail, length, g_stage.d_b, g_stage.d_b_cap, flags, &raw, &used, NULL);
        if (rc == HUF_ERROR_FATAL) return (huf_error_t)rc;
        if (rc == HUF_ERROR_MEMORY_ALLOCATION && out_cap < ((uint64_t)1 << 40)) {   /* output did not fit: enlarge */
            out_cap *= 4;
            continue;
        }
        if (pieces) {
            /* a piece of a stream: what counts is the last block boundary inside it */
            uint64_t good_raw = 0, good_used = 0;
            TRY(hufgpu_decode_stream_complete(g_ctx, &good_raw, &good_used));
            if (rc == HUF_ERROR_READ_WRITE) { rc = HUF_ERROR_SUCCESS; raw = good_raw; used = good_used; }
            *pieces = (rc == HUF_ERROR_SUCCESS) ? used : good_used;
            if (rc != HUF_ERROR_SUCCESS) raw = good_raw;          /* the blocks in front of a damaged one */
        } else
        if (rc == HUF_ERROR_READ_WRITE && rmem) {  /* maybe the stream holds more than `length` */
            const size_t more_want = avail < 65536 ? 65536 : avail;
            const size_t left = rmem->len - rmem->off;
            const size_t more = more_want < left ? more_want : left;
            if (more) { rmem->off += more; avail += more; continue; }
        } else if (rc == HUF_ERROR_READ_WRITE) {   /* maybe the reader has more than `length` */
            size_t more_want = avail < 65536 ? 65536 : avail;
            if (g_stage.h_a_cap < avail + more_want) {
                void *bigger = NULL; size_t bigger_cap = 0;
                TRY(grow_host(&bigger, &bigger_cap, avail + more_want));
                memcpy(bigger, g_stage.h_a, avail);
                (void)hipHostFree(g_stage.h_a);
                g_stage.h_a = bigger; g_stage.h_a_cap = bigger_cap;
            }
            size_t more = 0;
            TRY(read_upto(dec->config->reader, (uint8_t *)g_stage.h_a + avail, more_want, &more));
            if (more) { avail += more; continue; }
        }
        /* the reference's unbuffered reader stops right behind the last block it took (src/decoder.c:
         * 218-276 pulls bytes on demand): the bytes looked at speculatively beyond that stay unread, so
         * that a caller can decode consecutive streams from one memstream */
        if (rmem) rmem->off = start_off + (size_t)(used < avail ? used : avail);
        /* bytes of the blocks that decoded completely are delivered even when a later block
         * fails, as the reference's unbuffered writer would have done */
        if (raw && wmem) {
            TRY(d2h_to_memstream(wmem, g_stage.d_b, raw));
        } else if (raw) {
            TRY(grow_host(&g_stage.h_b, &g_stage.h_b_cap, raw));
            TRY(hufgpu_memcpy_d2h(g_ctx, g_stage.h_b, g_stage.d_b, raw));
            TRY(huf_bufio_write(dec->bufio_writer, g_stage.h_b, raw));
        }
        if (rc != HUF_ERROR_SUCCESS) return (huf_error_t)rc;   /* no flush on the error path (decoder.c:278-286) */
        return huf_bufio_read_writer_flush(dec->bufio_writer);
    }
}

huf_error_t huf_decode(const huf_config_t *config)
{
    GUARD(config);
    huf_decoder_t *dec = NULL;
    TRY(huf_decoder_init(&dec, config));
    huf_error_t err = HUF_ERROR_SUCCESS;
    if (dec->config->length) {                    /* test/decode_test.c:32-36: empty input is fine */
        session_enter();
        err = decode_locked(dec, NULL);
        session_leave();
    }
    huf_decoder_free(&dec);
    return err;
}

int huf_gpu_decode_blocks(const huf_config_t *config, uint64_t *consumed)
{
    GUARD(config);
    GUARD(consumed);
    *consumed = 0;
    huf_decoder_t *dec = NULL;
    TRY(huf_decoder_init(&dec, config));
    huf_error_t err = HUF_ERROR_SUCCESS;
    if (dec->config->length) {
        session_enter();
        err = decode_locked(dec, consumed);
        session_leave();
    }
    huf_decoder_free(&dec);
    return err;
}
