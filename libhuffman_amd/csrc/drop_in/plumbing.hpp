/*
 * drop_in/plumbing.hpp - host plumbing with the reference's observable behaviour: error strings, huf_malloc, the config
 * object, memory streams, descriptor streams, the bit writer and buffered byte I/O.
 */
/* ------------------------------------------------------------------ errors / alloc / config */
const char *huf_error_string(huf_error_t error)   /* src/errors.c:5-33 */
{
    /* callers pass anything (the reference answers "Unknown error" for -1, 7, 8 ...): the bytes are read as
     * an int, a C++ load of an out-of-range enum value would be undefined (UBSan: -fsanitize=enum) */
    int code;
    memcpy(&code, &error, sizeof(code));
    static_assert(sizeof(code) == sizeof(error), "huf_error_t is a 4-byte enum");
    switch (code) {
    case HUF_ERROR_SUCCESS: return "Success";
    case HUF_ERROR_MEMORY_ALLOCATION: return "Failed to allocate the requested memory block";
    case HUF_ERROR_INVALID_ARGUMENT: return "An invalid argument was specified to the function";
    case HUF_ERROR_READ_WRITE: return "Failed on read/write operation";
    case HUF_ERROR_FATAL: return "Fatal error";
    case HUF_ERROR_BTREE_OVERFLOW: return "Block is corrupted, Huffman tree has impossible size";
    case HUF_ERROR_BTREE_CORRUPTED: return "Huffman tree is corrupted and cannot be used to decode the block";
    default: return "Unknown error";
    }
}

huf_error_t huf_malloc(void **ptr, size_t size, size_t num)   /* src/malloc.c:7-19 */
{
    GUARD(ptr);
    *ptr = calloc(num, size);
    return *ptr ? HUF_ERROR_SUCCESS : HUF_ERROR_MEMORY_ALLOCATION;
}

huf_error_t huf_config_init(huf_config_t **self)   /* src/config.c:7-19 */
{
    GUARD(self);
    return huf_malloc((void **)self, sizeof(huf_config_t), 1);
}

huf_error_t huf_config_free(huf_config_t **self)   /* src/config.c:22-33 */
{
    GUARD(self);
    free(*self);
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

/* ------------------------------------------------------------------ memory stream (src/io.c:66-226) */
typedef struct {
    void **buf;     /* caller-owned pointer, replaced on growth */
    size_t off;     /* read cursor */
    size_t len;
    size_t cap;
    void *wrapped;  /* huf_gpu_memwrap[_out](): the caller's bytes (buf points here); never freed */
    int readonly;   /* huf_gpu_memwrap(): never written either */
    int fixed;      /* huf_gpu_memwrap_out(): written up to cap, never grown */
} membuf_t;

/* A stream buffer: zeroed like the reference's calloc (src/io.c:79-104, :181), free()d by the caller
 * like the reference's.  From a few MiB on the kernel is asked to back it with huge pages: the
 * first write into such a buffer is bound by page faults, and a 2 MiB page is one fault instead of
 * 512 (transparent huge pages are in "madvise" mode on the GPU boxes). */
#define HUF_BIG_BUFFER ((size_t)4 << 20)
static void advise_huge_pages(void *p, size_t bytes)
{
    if (p && bytes >= HUF_BIG_BUFFER) advise_huge(p, bytes);
}
static void *stream_alloc(size_t bytes)
{
    void *p = calloc(bytes ? bytes : 1, 1);
    advise_huge_pages(p, bytes);
    return p;
}

/* room for `count` more bytes behind the stream's contents */
static huf_error_t mem_reserve(membuf_t *m, size_t count)
{
    if (m->readonly) return HUF_ERROR_INVALID_ARGUMENT;
    if (m->fixed && m->cap - m->len < count) return HUF_ERROR_MEMORY_ALLOCATION;      /* the caller's memory ends here */
    if (m->cap - m->len < count) {
        /* growth policy of src/io.c:79-84 (double, or twice the request), but never smaller
         * than what is needed - the reference under-allocates here */
        size_t want = m->cap * 2;
        if (count > want) want = count * 2;
        if (want < m->len + count) want = m->len + count;
        void *grown = stream_alloc(want);
        if (!grown) return HUF_ERROR_MEMORY_ALLOCATION;
        if (m->len) memcpy(grown, *m->buf, m->len);
        free(*m->buf);
        *m->buf = grown;
        m->cap = want;
    }
    return HUF_ERROR_SUCCESS;
}

huf_error_t memwrite(void *stream, const void *buf, size_t count)
{
    membuf_t *m = (membuf_t *)stream;
    if (!m || (!buf && count)) return HUF_ERROR_INVALID_ARGUMENT;
    TRY(mem_reserve(m, count));
    if (count) memcpy((char *)*m->buf + m->len, buf, count);
    m->len += count;
    return HUF_ERROR_SUCCESS;
}

huf_error_t memread(void *stream, void *buf, size_t *count)
{
    membuf_t *m = (membuf_t *)stream;
    if (!m || !count) return HUF_ERROR_INVALID_ARGUMENT;
    size_t left = m->len - m->off;
    size_t take = *count < left ? *count : left;     /* short reads are not an error here */
    if (take) memcpy(buf, (char *)*m->buf + m->off, take);
    m->off += take;
    *count = take;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_memopen(huf_read_writer_t **self, void **buf, size_t capacity)
{
    GUARD(self);
    GUARD(buf);
    huf_read_writer_t *rw = (huf_read_writer_t *)calloc(1, sizeof(*rw));
    membuf_t *m = (membuf_t *)calloc(1, sizeof(*m));
    void *mem = stream_alloc(capacity);
    if (!rw || !m || !mem) {
        free(rw); free(m); free(mem);
        return HUF_ERROR_MEMORY_ALLOCATION;
    }
    *buf = mem;
    m->buf = buf;
    m->cap = capacity;
    rw->stream = m;
    rw->write = memwrite;
    rw->read = memread;
    *self = rw;
    return HUF_ERROR_SUCCESS;
}

/* Extension (not in the reference): a read-only memory stream over bytes the caller already has,
 * e.g. a Python bytes object - no copy into a huf_memopen() buffer.  Closed with huf_memclose(),
 * which never touches the bytes. */
int huf_gpu_memwrap(huf_read_writer_t **self, const void *data, size_t length)
{
    GUARD(self);
    if (!data && length) return HUF_ERROR_INVALID_ARGUMENT;
    huf_read_writer_t *rw = (huf_read_writer_t *)calloc(1, sizeof(*rw));
    membuf_t *m = (membuf_t *)calloc(1, sizeof(*m));
    if (!rw || !m) {
        free(rw); free(m);
        return HUF_ERROR_MEMORY_ALLOCATION;
    }
    m->wrapped = (void *)data;
    m->buf = &m->wrapped;
    m->len = m->cap = length;
    m->readonly = 1;
    rw->stream = m;
    rw->write = memwrite;
    rw->read = memread;
    *self = rw;
    return HUF_ERROR_SUCCESS;
}

/* Extension: a WRITER over memory the caller provides (`capacity` bytes, e.g. a Python bytes object that is
 * to become the result): what huf_encode()/huf_decode() write goes there directly, a write that does not fit
 * fails with HUF_ERROR_MEMORY_ALLOCATION (the memory is never grown, moved or freed).  huf_memlen() says how
 * much was written; closed with huf_memclose(). */
int huf_gpu_memwrap_out(huf_read_writer_t **self, void *buffer, size_t capacity)
{
    GUARD(self);
    if (!buffer && capacity) return HUF_ERROR_INVALID_ARGUMENT;
    huf_read_writer_t *rw = (huf_read_writer_t *)calloc(1, sizeof(*rw));
    membuf_t *m = (membuf_t *)calloc(1, sizeof(*m));
    if (!rw || !m) {
        free(rw); free(m);
        return HUF_ERROR_MEMORY_ALLOCATION;
    }
    m->wrapped = buffer;
    m->buf = &m->wrapped;
    m->cap = capacity;
    m->fixed = 1;
    advise_huge_pages(buffer, capacity);            /* (a fresh result buffer: its first write is bound by page faults) */
    rw->stream = m;
    rw->write = memwrite;
    rw->read = memread;
    *self = rw;
    return HUF_ERROR_SUCCESS;
}

static membuf_t *as_mem(const huf_read_writer_t *rw) { return rw ? (membuf_t *)rw->stream : NULL; }

huf_error_t huf_memlen(const huf_read_writer_t *self, size_t *len)
{
    GUARD(self); GUARD(len);
    *len = as_mem(self)->len;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_memcap(const huf_read_writer_t *self, size_t *cap)
{
    GUARD(self); GUARD(cap);
    *cap = as_mem(self)->cap;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_memrewind(huf_read_writer_t *self)   /* truncate, src/io.c:160-170 */
{
    GUARD(self);
    if (as_mem(self)->readonly) { as_mem(self)->off = 0; return HUF_ERROR_SUCCESS; }   /* wrapped bytes: start over */
    as_mem(self)->len = 0;
    as_mem(self)->off = 0;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_memclose(huf_read_writer_t **self)   /* leaves *buf to the caller, src/io.c:213-226 */
{
    GUARD(self);
    if (*self) {
        free((*self)->stream);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

/* ------------------------------------------------------------------ fd stream (src/io.c:9-63) */
huf_error_t fdwrite(void *stream, const void *buf, size_t count)
{
    if (!stream) return HUF_ERROR_INVALID_ARGUMENT;
    const int fd = *(int *)stream;
    const char *p = (const char *)buf;
    while (count) {                      /* partial writes and EINTR are retried */
        ssize_t w = write(fd, p, count);
        if (w < 0) {
            if (errno == EINTR) continue;
            return HUF_ERROR_READ_WRITE;
        }
        p += w;
        count -= (size_t)w;
    }
    return HUF_ERROR_SUCCESS;
}

huf_error_t fdread(void *stream, void *buf, size_t *count)
{
    if (!stream || !count) return HUF_ERROR_INVALID_ARGUMENT;
    const int fd = *(int *)stream;
    size_t got = 0;
    while (got < *count) {               /* fill the request unless EOF comes first */
        ssize_t r = read(fd, (char *)buf + got, *count - got);
        if (r < 0) {
            if (errno == EINTR) continue;
            *count = got;
            return HUF_ERROR_READ_WRITE;
        }
        if (r == 0) break;
        got += (size_t)r;
    }
    *count = got;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_fdopen(huf_read_writer_t **self, int fd)
{
    GUARD(self);
    huf_read_writer_t *rw = (huf_read_writer_t *)calloc(1, sizeof(*rw));
    int *slot = (int *)malloc(sizeof(int));   /* the reference keeps the address of its own
                                                  parameter (src/io.c:45); a heap copy here */
    if (!rw || !slot) { free(rw); free(slot); return HUF_ERROR_MEMORY_ALLOCATION; }
    *slot = fd;
    rw->stream = slot;
    rw->read = fdread;
    rw->write = fdwrite;
    *self = rw;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_fdclose(huf_read_writer_t **self)
{
    GUARD(self);
    if (*self) {
        free((*self)->stream);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

/* ------------------------------------------------------------------ bit writer (src/bufio.c:18-32) */
void huf_bit_write(huf_bit_read_writer_t *self, uint8_t bit)
{
    if (self->offset) self->offset--;
    self->bits |= (uint8_t)((bit & 1u) << self->offset);
}

void huf_bit_read_writer_reset(huf_bit_read_writer_t *self)
{
    self->bits = 0;
    self->offset = 8;
}

/* ------------------------------------------------------------------ buffered byte I/O (src/bufio.c:37-320) */
huf_error_t huf_bufio_read_writer_init(huf_bufio_read_writer_t **self, huf_read_writer_t *read_writer, size_t size)
{
    GUARD(self); GUARD(read_writer);
    huf_bufio_read_writer_t *b = (huf_bufio_read_writer_t *)calloc(1, sizeof(*b));
    if (!b) return HUF_ERROR_MEMORY_ALLOCATION;
    if (size) {                          /* 0 => pass-through (src/bufio.c:58-68) */
        b->bytes = (uint8_t *)calloc(size, 1);
        if (!b->bytes) { free(b); return HUF_ERROR_MEMORY_ALLOCATION; }
    }
    b->capacity = size;
    b->read_writer = read_writer;
    *self = b;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_bufio_read_writer_free(huf_bufio_read_writer_t **self)
{
    GUARD(self);
    if (*self) {
        free((*self)->bytes);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_bufio_read_writer_flush(huf_bufio_read_writer_t *self)
{
    GUARD(self);
    if (!self->length) return HUF_ERROR_SUCCESS;
    TRY(self->read_writer->write(self->read_writer->stream, self->bytes, self->length));
    self->length = 0;                    /* bytes were counted when they were accepted */
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_bufio_write(huf_bufio_read_writer_t *self, const void *buf, size_t size)
{
    GUARD(self); GUARD(buf);
    if (self->capacity && self->length >= self->capacity) TRY(huf_bufio_read_writer_flush(self));
    if (self->capacity && size <= self->capacity - self->length) {
        memcpy(self->bytes + self->length, buf, size);
        self->length += size;
        self->have_been_processed += size;
        return HUF_ERROR_SUCCESS;
    }
    if (size) {                          /* too big for the buffer: drain, then write through */
        TRY(huf_bufio_read_writer_flush(self));
        TRY(self->read_writer->write(self->read_writer->stream, buf, size));
        self->have_been_processed += size;
    }
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_bufio_read(huf_bufio_read_writer_t *self, void *buf, size_t size)
{
    GUARD(self); GUARD(buf);
    uint8_t *dst = (uint8_t *)buf;
    size_t want = size;
    size_t have = self->length - self->offset;
    if (have && want) {
        size_t take = have < want ? have : want;
        memcpy(dst, self->bytes + self->offset, take);
        self->offset += take;
        dst += take;
        want -= take;
    }
    if (want) {
        if (want >= self->capacity) {    /* straight into the destination (src/bufio.c:239-257) */
            size_t got = want;
            TRY(self->read_writer->read(self->read_writer->stream, dst, &got));
            self->length = self->offset = 0;
            if (got < want) return HUF_ERROR_READ_WRITE;
        } else {                         /* refill, then copy (src/bufio.c:259-277) */
            size_t got = self->capacity;
            TRY(self->read_writer->read(self->read_writer->stream, self->bytes, &got));
            self->length = got;
            self->offset = 0;
            if (got < want) return HUF_ERROR_READ_WRITE;
            memcpy(dst, self->bytes, want);
            self->offset = want;
        }
    }
    self->have_been_processed += size;   /* only successful requests are counted */
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_bufio_read_uint8(huf_bufio_read_writer_t *self, uint8_t *byte)
{
    GUARD(self); GUARD(byte);
    return huf_bufio_read(self, byte, 1);
}

huf_error_t huf_bufio_write_uint8(huf_bufio_read_writer_t *self, uint8_t byte)
{
    GUARD(self);
    return huf_bufio_write(self, &byte, 1);
}
