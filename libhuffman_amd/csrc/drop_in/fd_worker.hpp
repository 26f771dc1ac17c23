/*
 * drop_in/fd_worker.hpp - fd streams: I/O next to the GPU work.
 *
 * A stream made by huf_fdopen() is this library's own object too: its read(2)/write(2) calls can
 * run on a helper thread while the calling thread drives the GPU, in order and one at a time per
 * descriptor.  Two pinned buffers per direction: the reader fills one while the other is encoded,
 * the writer drains one while the next result arrives.  Streams with foreign
 * callbacks are never touched from a helper thread (§8b: callbacks run serially on the caller's
 * thread).
 */
typedef struct {
    pthread_t thread;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int started;
    int fd;
    int writer;              /* 0: fills the slots from fd, 1: drains them to fd */
    char *buf[2];
    size_t len[2];           /* bytes in the slot (reader: what the read returned) */
    int full[2];             /* reader: filled, waiting for the consumer; writer: handed over, waiting for write(2) */
    uint64_t remaining;      /* reader: bytes still to be requested */
    size_t batch;            /* reader: bytes per request; writer: bytes a slot holds */
    int eof_ok;              /* reader: the end of the input is the consumer's business (decode), not a failure */
    int next;                /* writer: slot of the next fd_writer_push() piece */
    int quit;                /* consumer/producer side is done (or gave up) */
    huf_error_t err;
} fd_worker_t;

static void *fd_worker_main(void *arg)
{
    fd_worker_t *w = (fd_worker_t *)arg;
    for (int k = 0;; k ^= 1) {
        pthread_mutex_lock(&w->mu);
        if (w->writer) {
            while (!w->full[k] && !w->quit) pthread_cond_wait(&w->cv, &w->mu);
            if (!w->full[k]) { pthread_mutex_unlock(&w->mu); break; }     /* quit and nothing handed over */
        } else {
            while (w->full[k] && !w->quit) pthread_cond_wait(&w->cv, &w->mu);
            if (w->quit || !w->remaining) { pthread_mutex_unlock(&w->mu); break; }
        }
        pthread_mutex_unlock(&w->mu);
        huf_error_t err = HUF_ERROR_SUCCESS;
        size_t got = 0;
        if (w->writer) {
            if (w->err == HUF_ERROR_SUCCESS) err = fdwrite(&w->fd, w->buf[k], w->len[k]);   /* after a failure: drop */
        } else {
            got = w->remaining < w->batch ? (size_t)w->remaining : w->batch;
            const size_t want = got;
            err = fdread(&w->fd, w->buf[k], &got);
            if (err == HUF_ERROR_SUCCESS && got < want && !w->eof_ok) err = HUF_ERROR_READ_WRITE;   /* bufio.c:251-253 */
            w->remaining = (got < want) ? 0 : w->remaining - want;
        }
        pthread_mutex_lock(&w->mu);
        if (err != HUF_ERROR_SUCCESS && w->err == HUF_ERROR_SUCCESS) w->err = err;
        if (w->writer) w->full[k] = 0;
        else { w->len[k] = got; w->full[k] = 1; }
        pthread_cond_broadcast(&w->cv);
        const int stop = !w->writer && (err != HUF_ERROR_SUCCESS || !w->remaining);
        pthread_mutex_unlock(&w->mu);
        if (stop) break;
    }
    return NULL;
}

static huf_error_t fd_worker_start(fd_worker_t *w)
{
    pthread_mutex_init(&w->mu, NULL);
    pthread_cond_init(&w->cv, NULL);
    if (pthread_create(&w->thread, NULL, fd_worker_main, w) != 0) return HUF_ERROR_MEMORY_ALLOCATION;
    w->started = 1;
    return HUF_ERROR_SUCCESS;
}

/* the caller is done with the worker: a writer first drains what was handed over */
static huf_error_t fd_worker_finish(fd_worker_t *w)
{
    if (!w->started) return HUF_ERROR_SUCCESS;
    pthread_mutex_lock(&w->mu);
    w->quit = 1;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
    pthread_join(w->thread, NULL);
    pthread_mutex_destroy(&w->mu);
    pthread_cond_destroy(&w->cv);
    w->started = 0;
    return w->err;
}

/* reader slot k: wait for its bytes (a short or failed read is reported with the slot it hit) */
static huf_error_t fd_reader_wait(fd_worker_t *w, int k, size_t want)
{
    pthread_mutex_lock(&w->mu);
    while (!w->full[k]) pthread_cond_wait(&w->cv, &w->mu);
    const huf_error_t err = (w->len[k] < want) ? (w->err != HUF_ERROR_SUCCESS ? w->err : HUF_ERROR_READ_WRITE)
                                                : HUF_ERROR_SUCCESS;
    pthread_mutex_unlock(&w->mu);
    return err;
}

static void fd_reader_release(fd_worker_t *w, int k)
{
    pthread_mutex_lock(&w->mu);
    w->full[k] = 0;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
}

/* writer slot k: wait until its previous content is on the descriptor */
static huf_error_t fd_writer_wait(fd_worker_t *w, int k)
{
    pthread_mutex_lock(&w->mu);
    while (w->full[k]) pthread_cond_wait(&w->cv, &w->mu);
    const huf_error_t err = w->err;
    pthread_mutex_unlock(&w->mu);
    return err;
}

static void fd_writer_submit(fd_worker_t *w, int k, size_t len)
{
    pthread_mutex_lock(&w->mu);
    w->len[k] = len;
    w->full[k] = 1;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
}

/* len bytes at d_src -> the descriptor, through the slots (a piece per slot) */
static huf_error_t fd_writer_push(fd_worker_t *w, const void *d_src, uint64_t len)
{
    const char *p = (const char *)d_src;
    while (len) {
        const size_t n = len < w->batch ? (size_t)len : w->batch;
        const int k = w->next;
        TRY(fd_writer_wait(w, k));
        TRY(hufgpu_memcpy_d2h(g_ctx, w->buf[k], p, n));
        fd_writer_submit(w, k, n);
        w->next ^= 1;
        p += n;
        len -= n;
    }
    return HUF_ERROR_SUCCESS;
}

static int own_fd_of(const huf_read_writer_t *rw, int writer)
{
    if (!rw || !rw->stream) return -1;
    if (writer ? rw->write != fdwrite : rw->read != fdread) return -1;
    return *(const int *)rw->stream;
}
