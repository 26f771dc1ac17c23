/*
 * huf_host.cpp - host half of the drop-in libhuffman API (include/huffman.h).
 *
 *  - stream backends, buffered byte I/O, error strings, config/alloc helpers: host plumbing
 *    with the reference's observable behaviour (src/io.c, src/bufio.c, src/errors.c,
 *    src/config.c, src/malloc.c) minus the defects listed in SURVEY Appendix D;
 *  - host-callable building blocks the reference also exports (histogram, symbol map, pointer
 *    tree): small re-implementations so that programs linking those symbols keep working;
 *  - huf_encode()/huf_decode(): read a batch through the caller's reader, run the block
 *    codec ON THE GPU (hufgpu_encode / hufgpu_decode_stream), hand the result to the writer.
 *    There is no CPU codec behind them: no GPU => HUF_ERROR_FATAL.
 *
 * Environment (huf_config_t's 48-byte layout is ABI, so switches live outside it):
 *   HUF_GPU_DEVICE        device ordinal (default 0)
 *   HUF_GPU_BATCH_MB      MiB per GPU round: input of huf_encode (default 256; 32 when a
 *                         huf_fdopen() descriptor is read or written under the GPU work), stream
 *                         bytes of a huf_decode that reads a huf_fdopen() descriptor (default 32)
 *   HUF_GPU_ZERO_COPY     0 = always go through the streams' read/write callbacks (default 1:
 *                         huf_memopen() streams are copied to/from the device directly and
 *                         huf_fdopen() descriptors are read/written by helper threads)
 *   HUF_GPU_RELAXED_TREE  1 = accept 1025-entry trees on decode
 *
 * The text is in csrc/drop_in/, included below in the order the compiler reads it.
 */
#include <errno.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <sched.h>

#include <atomic>
#include <sys/mman.h>

#include <hip/hip_runtime_api.h>

#include "../../include/huffman.h"
#include "../../include/huffman_gpu.h"

#define GUARD(ptr)                                   \
    do {                                             \
        if (!(ptr)) return HUF_ERROR_INVALID_ARGUMENT; \
    } while (0)
#define TRY(expr)                                    \
    do {                                             \
        huf_error_t e__ = (huf_error_t)(expr);       \
        if (e__ != HUF_ERROR_SUCCESS) return e__;    \
    } while (0)

/* The parts, in the order the compiler reads them: each uses only what stands above it (no forward declarations). */
#include "drop_in/parts.hpp"          /* env_int, page_span, advise_huge, split_parts / run_parts: libc and pthreads only */

extern "C" {

#include "drop_in/plumbing.hpp"       /* errors, huf_malloc, config, memory streams, fd streams, bit writer, bufio */
#include "drop_in/blocks.hpp"         /* histogram, symbol mapping, pointer tree */
#include "drop_in/session.hpp"        /* the session pool, grow_host / grow_dev / grow_dev_keep, huf_gpu_sessions */
#include "drop_in/transfer.hpp"       /* prefault, the piece mover, lane_copy, the dx_* pool, d2h_to_memstream, huf_gpu_copy_out */
#include "drop_in/fd_worker.hpp"      /* the descriptor helper threads */
#include "drop_in/codec_objects.hpp"  /* encoder / decoder objects, relaxed_tree, own_* and zero_copy_enabled */
#include "drop_in/encode.hpp"         /* encode_rounds, encode_fanout, encode_duplex, encode_locked, huf_encode, huf_gpu_fanouts */
#include "drop_in/decode.hpp"         /* the fd route, decode_fanout, decode_duplex, decode_locked, huf_decode, huf_gpu_decode_blocks */

}  /* extern "C" */
