/*
 * drop_in/session.hpp - the GPU sessions of huf_encode / huf_decode, and the staging buffers a session owns.
 *
 * A session = one device context plus its staging buffers; a call holds one session from start to
 * end.  By default there is ONE session on device HUF_GPU_DEVICE (0): concurrent calls take turns.
 * HUF_GPU_DEVICES = "0,1,2" / "all" makes one session per listed device ("0,0": two on device 0), and
 * concurrent calls - disjoint configs on different threads are legal and parallel in the
 * reference, which has no global state (src/encoder.c:379-392) - run side by side, each on the
 * first session that is free: a multi-threaded C caller uses every listed GPU.
 */
#define LANE_MAX 8             /* copy lanes (threads) of a large host <-> device transfer */
typedef struct {
    void *h_a, *h_b;           /* pinned staging */
    size_t h_a_cap, h_b_cap;
    void *d_a, *d_b, *d_c;     /* device staging (d_c: one round of a descriptor-fed decode) */
    size_t d_a_cap, d_b_cap, d_c_cap;
    void *lane_pin;            /* LANE_MAX x 2 pinned slots of LANE_SLOT bytes (lane_copy) */
    hipStream_t lane_stream[LANE_MAX];
    hipEvent_t lane_ev[LANE_MAX][2];
    int lanes_ready;
} staging_t;

#define HUF_MAX_SESSIONS 32
typedef struct {
    int device;
    int busy;
    hufgpu_ctx_t *ctx;
    staging_t stage;
} session_t;

static pthread_mutex_t g_pool_lock = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_pool_cv = PTHREAD_COND_INITIALIZER;
static session_t g_sessions[HUF_MAX_SESSIONS];
static int g_nsessions = 0;
static __thread session_t *t_session = NULL;       /* the session the calling thread holds */
#define g_ctx (t_session->ctx)
#define g_stage (t_session->stage)

/* the device list, read once (no GPU call: a process without a GPU still gets its loud error from
 * session_acquire) */
static void session_pool_init(void)
{
    if (g_nsessions) return;
    const char *list = getenv("HUF_GPU_DEVICES");
    if (list && *list) {
        if (strcmp(list, "all") == 0) {
            int n = hufgpu_device_count();
            if (n > HUF_MAX_SESSIONS) n = HUF_MAX_SESSIONS;
            for (int i = 0; i < n; i++) g_sessions[g_nsessions++].device = i;
        } else {
            const char *p = list;
            while (*p && g_nsessions < HUF_MAX_SESSIONS) {
                char *end = NULL;
                const long v = strtol(p, &end, 10);
                if (end == p) break;
                if (v >= 0) g_sessions[g_nsessions++].device = (int)v;
                p = end;
                while (*p == ',' || *p == ' ') p++;
            }
        }
    }
    if (!g_nsessions) {
        g_sessions[g_nsessions++].device = env_int("HUF_GPU_DEVICE", 0, INT_MIN, INT_MAX);
    }
}

static void session_enter(void)
{
    pthread_mutex_lock(&g_pool_lock);
    session_pool_init();
    for (;;) {
        for (int i = 0; i < g_nsessions; i++)
            if (!g_sessions[i].busy) {
                g_sessions[i].busy = 1;
                t_session = &g_sessions[i];
                pthread_mutex_unlock(&g_pool_lock);
                return;
            }
        pthread_cond_wait(&g_pool_cv, &g_pool_lock);
    }
}

static void session_leave(void)
{
    pthread_mutex_lock(&g_pool_lock);
    t_session->busy = 0;
    t_session = NULL;
    pthread_cond_signal(&g_pool_cv);
    pthread_mutex_unlock(&g_pool_lock);
}

/* a second, third ... session for the calling call, if one is free right now (never waits) */
static session_t *session_try_extra(void)
{
    session_t *got = NULL;
    pthread_mutex_lock(&g_pool_lock);
    for (int i = 0; i < g_nsessions && !got; i++)
        if (!g_sessions[i].busy) {
            g_sessions[i].busy = 1;
            got = &g_sessions[i];
        }
    pthread_mutex_unlock(&g_pool_lock);
    return got;
}

static void session_release_extra(session_t *s)
{
    pthread_mutex_lock(&g_pool_lock);
    s->busy = 0;
    pthread_cond_signal(&g_pool_cv);
    pthread_mutex_unlock(&g_pool_lock);
}

static huf_error_t session_acquire(void)
{
    if (g_ctx) return HUF_ERROR_SUCCESS;
    int rc = hufgpu_ctx_create(&g_ctx, t_session->device);
    if (rc != HUF_ERROR_SUCCESS) {
        fprintf(stderr, "libhuffman: the codec needs an MI355X (gfx950) GPU and has no CPU fallback: %s\n",
                hufgpu_last_error(NULL));
        g_ctx = NULL;
        return HUF_ERROR_FATAL;
    }
    return HUF_ERROR_SUCCESS;
}

static huf_error_t grow_host(void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return HUF_ERROR_SUCCESS;
    if (*p) (void)hipHostFree(*p);
    *p = NULL; *cap = 0;
    (void)hipSetDevice(t_session->device);
    if (hipHostMalloc(p, want, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return HUF_ERROR_MEMORY_ALLOCATION;
    }
    *cap = want;
    return HUF_ERROR_SUCCESS;
}

static huf_error_t grow_dev(void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return HUF_ERROR_SUCCESS;
    if (*p) hufgpu_free(g_ctx, *p);
    *p = NULL; *cap = 0;
    TRY(hufgpu_malloc(g_ctx, p, want));
    *cap = want;
    return HUF_ERROR_SUCCESS;
}

/* like grow_dev(), but the first `keep` bytes survive */
static huf_error_t grow_dev_keep(void **p, size_t *cap, size_t want, size_t keep)
{
    if (*cap >= want) return HUF_ERROR_SUCCESS;
    void *bigger = NULL;
    TRY(hufgpu_malloc(g_ctx, &bigger, want));
    if (keep) {
        const int rc = hufgpu_memcpy_d2d(g_ctx, bigger, *p, keep);
        if (rc != HUF_ERROR_SUCCESS) { hufgpu_free(g_ctx, bigger); return (huf_error_t)rc; }
    }
    if (*p) hufgpu_free(g_ctx, *p);
    *p = bigger;
    *cap = want;
    return HUF_ERROR_SUCCESS;
}

/* sessions that hold a device context right now, and how many the device list allows */
int huf_gpu_sessions(int *configured)
{
    pthread_mutex_lock(&g_pool_lock);
    session_pool_init();
    int live = 0;
    for (int i = 0; i < g_nsessions; i++) live += g_sessions[i].ctx != NULL;
    if (configured) *configured = g_nsessions;
    pthread_mutex_unlock(&g_pool_lock);
    return live;
}
