/*
 * drop_in/blocks.hpp - host-callable building blocks the reference also exports (histogram, symbol mapping, pointer
 * tree): small re-implementations so that programs linking those symbols keep working.  The codec does not use them.
 */
/* ------------------------------------------------------------------ histogram (src/histogram.c) */
huf_error_t huf_histogram_init(huf_histogram_t **self, size_t iota, size_t length)
{
    GUARD(self);
    if (!iota || !length) return HUF_ERROR_INVALID_ARGUMENT;
    huf_histogram_t *h = (huf_histogram_t *)calloc(1, sizeof(*h));
    if (!h) return HUF_ERROR_MEMORY_ALLOCATION;
    h->frequencies = (uint64_t *)calloc(length, sizeof(uint64_t));
    if (!h->frequencies) { free(h); return HUF_ERROR_MEMORY_ALLOCATION; }
    h->iota = iota;
    h->length = length;
    h->start = (size_t)-1;
    *self = h;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_histogram_free(huf_histogram_t **self)
{
    GUARD(self);
    if (*self) {
        free((*self)->frequencies);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_histogram_reset(huf_histogram_t *self)
{
    GUARD(self);
    memset(self->frequencies, 0, self->length * sizeof(uint64_t));
    self->start = (size_t)-1;
    return HUF_ERROR_SUCCESS;
}

/* Generic element width (1..8 bytes, little-endian), whole elements only. The GPU kernel
 * hist256_kernel is the iota == 1 case the codec uses; this host version exists because the
 * reference exports it with a host-pointer signature. */
huf_error_t huf_histogram_populate(huf_histogram_t *self, void *buf, size_t len)
{
    GUARD(self); GUARD(buf);
    if (self->iota > 8) return HUF_ERROR_INVALID_ARGUMENT;
    const uint8_t *p = (const uint8_t *)buf;
    for (size_t at = 0; at + self->iota <= len; at += self->iota) {
        uint64_t el = 0;
        memcpy(&el, p + at, self->iota);
        if (el >= self->length) return HUF_ERROR_INVALID_ARGUMENT;   /* the reference writes out of bounds */
        self->frequencies[el]++;
        if (self->start == (size_t)-1 || el < self->start) self->start = (size_t)el;
    }
    return HUF_ERROR_SUCCESS;
}

/* ------------------------------------------------------------------ symbol map (src/symbol.c) */
huf_error_t huf_symbol_mapping_element_init(huf_symbol_mapping_element_t **self, const uint8_t *coding, size_t length)
{
    GUARD(self); GUARD(coding);
    huf_symbol_mapping_element_t *e = (huf_symbol_mapping_element_t *)calloc(1, sizeof(*e));
    if (!e) return HUF_ERROR_MEMORY_ALLOCATION;
    e->coding = (uint8_t *)calloc(length + 1, 1);
    if (!e->coding) { free(e); return HUF_ERROR_MEMORY_ALLOCATION; }
    memcpy(e->coding, coding, length);
    e->length = length;
    *self = e;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_symbol_mapping_element_free(huf_symbol_mapping_element_t **self)
{
    GUARD(self);
    if (*self) {
        free((*self)->coding);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_symbol_mapping_init(huf_symbol_mapping_t **self, size_t length)
{
    GUARD(self);
    huf_symbol_mapping_t *m = (huf_symbol_mapping_t *)calloc(1, sizeof(*m));
    if (!m) return HUF_ERROR_MEMORY_ALLOCATION;
    m->symbols = (huf_symbol_mapping_element_t **)calloc(length ? length : 1, sizeof(*m->symbols));
    if (!m->symbols) { free(m); return HUF_ERROR_MEMORY_ALLOCATION; }
    m->length = length;
    *self = m;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_symbol_mapping_reset(huf_symbol_mapping_t *self)
{
    GUARD(self);
    for (size_t i = 0; i < self->length; i++)
        if (self->symbols[i]) huf_symbol_mapping_element_free(&self->symbols[i]);
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_symbol_mapping_free(huf_symbol_mapping_t **self)
{
    GUARD(self);
    if (*self) {
        huf_symbol_mapping_reset(*self);
        free((*self)->symbols);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_symbol_mapping_insert(huf_symbol_mapping_t *self, size_t position, huf_symbol_mapping_element_t *element)
{
    GUARD(self); GUARD(element);
    if (position >= self->length) return HUF_ERROR_INVALID_ARGUMENT;
    if (self->symbols[position]) huf_symbol_mapping_element_free(&self->symbols[position]);
    self->symbols[position] = element;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_symbol_mapping_get(huf_symbol_mapping_t *self, size_t position, huf_symbol_mapping_element_t **element)
{
    GUARD(self); GUARD(element);
    if (position >= self->length) return HUF_ERROR_INVALID_ARGUMENT;
    *element = self->symbols[position];
    return HUF_ERROR_SUCCESS;
}

/* ------------------------------------------------------------------ pointer tree (src/tree.c) */
huf_error_t huf_node_to_string(const huf_node_t *self, uint8_t *buf, size_t *len)
{
    GUARD(buf); GUARD(len);
    size_t n = 0;
    for (const huf_node_t *cur = self; cur && cur->parent && n < *len; cur = cur->parent)
        buf[n++] = (cur->parent->left == cur) ? '0' : '1';    /* leaf -> root, src/tree.c:23-41 */
    *len = n;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_tree_init(huf_tree_t **self)
{
    GUARD(self);
    huf_tree_t *t = (huf_tree_t *)calloc(1, sizeof(*t));
    if (!t) return HUF_ERROR_MEMORY_ALLOCATION;
    t->leaves = (huf_node_t **)calloc(HUF_HISTOGRAM_LEN, sizeof(huf_node_t *));
    if (!t->leaves) { free(t); return HUF_ERROR_MEMORY_ALLOCATION; }
    *self = t;
    return HUF_ERROR_SUCCESS;
}

static void free_nodes(huf_node_t *root)   /* iterative: foreign trees may be 1025 deep */
{
    huf_node_t *cur = root;
    while (cur) {
        if (cur->left) { huf_node_t *c = cur->left; cur->left = NULL; c->parent = cur; cur = c; }
        else if (cur->right) { huf_node_t *c = cur->right; cur->right = NULL; c->parent = cur; cur = c; }
        else {
            huf_node_t *up = (cur == root) ? NULL : cur->parent;
            free(cur);
            cur = up;
        }
    }
}

huf_error_t huf_tree_reset(huf_tree_t *self)
{
    GUARD(self);
    free_nodes(self->root);
    self->root = NULL;
    memset(self->leaves, 0, HUF_HISTOGRAM_LEN * sizeof(huf_node_t *));
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_tree_free(huf_tree_t **self)
{
    GUARD(self);
    if (*self) {
        free_nodes((*self)->root);
        free((*self)->leaves);
        free(*self);
    }
    *self = NULL;
    return HUF_ERROR_SUCCESS;
}

/* Same selection rule as the device tree_kernel: smallest (rate, 511 - index) first; the
 * smaller becomes the left child; a lone survivor gets a left-only root (src/tree.c:292-427).
 * Consumes the histogram like the reference does. */
huf_error_t huf_tree_from_histogram(huf_tree_t *self, huf_histogram_t *histogram)
{
    GUARD(self); GUARD(histogram);
    if (histogram->length < HUF_HISTOGRAM_LEN) return HUF_ERROR_INVALID_ARGUMENT;
    uint64_t *rate = histogram->frequencies;
    huf_node_t *slot[HUF_HISTOGRAM_LEN] = {0};
    int next = HUF_ASCII_COUNT;
    for (;;) {
        int best = -1, second = -1;
        for (int i = next - 1; i >= 0; i--) {          /* descending index: ties keep the earlier hit */
            if (!rate[i]) continue;
            if (best < 0 || rate[i] < rate[best]) { second = best; best = i; }
            else if (second < 0 || rate[i] < rate[second]) second = i;
        }
        if (best < 0) break;
        if (next >= HUF_HISTOGRAM_LEN) return HUF_ERROR_FATAL;
        huf_node_t *parent = (huf_node_t *)calloc(1, sizeof(huf_node_t));
        if (!parent) return HUF_ERROR_MEMORY_ALLOCATION;
        parent->index = (int16_t)next;
        const int pick[2] = {best, second};
        for (int side = 0; side < 2; side++) {
            const int i = pick[side];
            if (i < 0) continue;
            if (!slot[i]) {
                slot[i] = (huf_node_t *)calloc(1, sizeof(huf_node_t));
                if (!slot[i]) { free(parent); return HUF_ERROR_MEMORY_ALLOCATION; }
                slot[i]->index = (int16_t)i;
            }
            slot[i]->parent = parent;
            if (side == 0) parent->left = slot[i]; else parent->right = slot[i];
            if (i < HUF_ASCII_COUNT) self->leaves[i] = slot[i];
        }
        rate[next] = rate[best] + (second >= 0 ? rate[second] : 0);
        rate[best] = 0;
        if (second >= 0) rate[second] = 0;
        slot[next] = parent;
        self->root = parent;
        next++;
        if (second < 0) break;
    }
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_tree_serialize(huf_tree_t *self, int16_t *buf, size_t *len)   /* preorder, -1 = absent */
{
    GUARD(self); GUARD(buf); GUARD(len);
    size_t n = 0;
    /* explicit stack of "right children still to emit" */
    const huf_node_t *stack[2 * HUF_HISTOGRAM_LEN + 4];
    int top = 0;
    const huf_node_t *cur = self->root;
    for (;;) {
        if (cur) {
            buf[n++] = cur->index;
            if (top >= (int)(sizeof(stack) / sizeof(stack[0]))) return HUF_ERROR_FATAL;
            stack[top++] = cur->right;
            cur = cur->left;
        } else {
            buf[n++] = HUF_LEAF_NODE;
            if (!top) break;
            cur = stack[--top];
        }
    }
    *len = n;
    return HUF_ERROR_SUCCESS;
}

huf_error_t huf_tree_deserialize(huf_tree_t *self, const int16_t *buf, size_t len)
{
    GUARD(self); GUARD(buf);
    /* every entry other than -1 is a node, entries past `len` are absent children */
    huf_node_t **pending = (huf_node_t **)calloc(len + 1, sizeof(huf_node_t *));
    if (!pending) return HUF_ERROR_MEMORY_ALLOCATION;
    size_t top = 0, at = 0;
    huf_node_t **link = &self->root;
    huf_node_t *owner = NULL;
    for (;;) {
        huf_node_t *made = NULL;
        if (at < len) {
            const int16_t v = buf[at++];
            if (v != HUF_LEAF_NODE) {
                made = (huf_node_t *)calloc(1, sizeof(huf_node_t));
                if (!made) { free(pending); return HUF_ERROR_MEMORY_ALLOCATION; }
                made->index = v;
                made->parent = owner;
            }
        }
        if (made) {
            *link = made;
            pending[top++] = made;
            owner = made;
            link = &made->left;
            continue;
        }
        if (!top) break;
        owner = pending[--top];
        link = &owner->right;
    }
    free(pending);
    return HUF_ERROR_SUCCESS;
}
