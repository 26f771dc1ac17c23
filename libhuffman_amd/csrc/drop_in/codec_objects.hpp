/*
 * drop_in/codec_objects.hpp - the encoder / decoder objects of the reference's API, and what a call finds out about
 * its streams before it picks a route: whether they are this library's own, whether trees may be relaxed.
 */
static int g_relaxed = -1;                         /* HUF_GPU_RELAXED_TREE, read at the first decode unless set before */
static int relaxed_tree(void)
{
    if (g_relaxed < 0) g_relaxed = env_flag("HUF_GPU_RELAXED_TREE", 0);
    return g_relaxed;
}

/* Exported switch (not part of the reference API): 1 = accept tree_len 1025 on decode. */
void huf_gpu_set_relaxed_tree(int enabled) { g_relaxed = enabled ? 1 : 0; }

/* ------------------------------------------------------------------ encoder / decoder objects */
struct __huf_encoder {
    huf_config_t *config;
    huf_bufio_read_writer_t *bufio_writer;
    huf_bufio_read_writer_t *bufio_reader;
};
struct __huf_decoder {
    huf_config_t *config;
    huf_bufio_read_writer_t *bufio_writer;
    huf_bufio_read_writer_t *bufio_reader;
};

static huf_error_t codec_init(huf_config_t **cfg, huf_bufio_read_writer_t **w, huf_bufio_read_writer_t **r,
                              const huf_config_t *config)
{
    GUARD(config);
    if (!config->reader || !config->writer) return HUF_ERROR_INVALID_ARGUMENT;   /* the reference crashes */
    TRY(huf_config_init(cfg));
    memcpy(*cfg, config, sizeof(*config));       /* private copy: the caller's struct is never written */
    TRY(huf_bufio_read_writer_init(w, (*cfg)->writer, (*cfg)->writer_buffer_size));
    TRY(huf_bufio_read_writer_init(r, (*cfg)->reader, (*cfg)->reader_buffer_size));
    return HUF_ERROR_SUCCESS;
}

static void codec_free(huf_config_t **cfg, huf_bufio_read_writer_t **w, huf_bufio_read_writer_t **r)
{
    huf_bufio_read_writer_free(w);
    huf_bufio_read_writer_free(r);
    huf_config_free(cfg);
}

huf_error_t huf_encoder_init(huf_encoder_t **self, const huf_config_t *config)
{
    GUARD(self); GUARD(config);
    huf_encoder_t *e = (huf_encoder_t *)calloc(1, sizeof(*e));
    if (!e) return HUF_ERROR_MEMORY_ALLOCATION;
    *self = e;
    huf_error_t err = codec_init(&e->config, &e->bufio_writer, &e->bufio_reader, config);
    if (err == HUF_ERROR_SUCCESS && !e->config->blocksize) e->config->blocksize = e->config->length;   /* encoder.c:163-165 */
    if (err != HUF_ERROR_SUCCESS) huf_encoder_free(self);
    return err;
}

huf_error_t huf_encoder_free(huf_encoder_t **self)
{
    GUARD(self);
    if (*self) {
        codec_free(&(*self)->config, &(*self)->bufio_writer, &(*self)->bufio_reader);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_decoder_init(huf_decoder_t **self, const huf_config_t *config)
{
    GUARD(self); GUARD(config);
    huf_decoder_t *d = (huf_decoder_t *)calloc(1, sizeof(*d));
    if (!d) return HUF_ERROR_MEMORY_ALLOCATION;
    *self = d;
    huf_error_t err = codec_init(&d->config, &d->bufio_writer, &d->bufio_reader, config);
    if (err != HUF_ERROR_SUCCESS) huf_decoder_free(self);
    return err;
}

huf_error_t huf_decoder_free(huf_decoder_t **self)
{
    GUARD(self);
    if (*self) {
        codec_free(&(*self)->config, &(*self)->bufio_writer, &(*self)->bufio_reader);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

/* A stream made by huf_memopen() is this library's own object: the codec then copies between
 * its buffer and the device directly instead of through read()/write() and a staging buffer
 * (one host memcpy less per direction; the stream's cursor and length move exactly as the
 * callbacks would have moved them).  Any other stream goes through its callbacks. */
static membuf_t *own_memstream_reader(const huf_read_writer_t *rw) { return (rw && rw->read == memread) ? (membuf_t *)rw->stream : NULL; }
static membuf_t *own_memstream_writer(const huf_read_writer_t *rw) { return (rw && rw->write == memwrite) ? (membuf_t *)rw->stream : NULL; }
/* HUF_GPU_ZERO_COPY, read at every call (a process may switch it between calls) */
static int zero_copy_enabled(void) { return env_flag("HUF_GPU_ZERO_COPY", 1); }
