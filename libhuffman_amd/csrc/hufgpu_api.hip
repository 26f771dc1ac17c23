/*
 * hufgpu_api.hip - host side of the device-resident C ABI (include/huffman_gpu.h).
 *
 * Owns the per-device context (stream, workspaces in HBM, pinned result words) and launches the
 * kernels of hufgpu_kernels.hip.  No CPU implementation of the codec lives here: if HIP or a
 * gfx950 device is unavailable every entry point fails with HUF_ERROR_FATAL and says why.
 */
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/huffman_gpu.h"
#include "hufgpu_common.h"
#include "hufgpu_kernels.hip"

using namespace hufgpu;

#ifndef HIST_THREADS
#define HIST_THREADS 256
#endif
#define PACK_THREADS 256
#ifndef DSUB_THREADS
#define DSUB_THREADS 256      /* decode_sub_kernel: four waves a workgroup, eight wave tiles a wave - a workgroup's table build is paid once per 64 KiB */
#endif
#ifndef DEC_THREADS
#define DEC_THREADS 512
#endif
#define SCAN_THREADS 1024
#define MAX_STAGES 8
#define PROF_SLOTS 256
#define PROF_ENCODE 0
#define PROF_DECODE 1


/* The parts, in the order the compiler reads them: each uses only what stands above it (no forward declarations). */
#include "host/ctx.hpp"         /* the context: struct, errors, the table of its workspaces (host/workspace.hpp), create / destroy */
#include "host/profile.hpp"     /* STAGE_BEGIN / STAGE_MARK, hufgpu_set_profiling, hufgpu_get_profile */
#include "host/encode.hpp"      /* block and sub-index geometry, hufgpu_histogram, hufgpu_encode*, hufgpu_encode_small */
#include "host/decode.hpp"      /* the one launcher of the indexed decoders, hufgpu_decode*, hufgpu_decode_result */
#include "host/stream.hpp"      /* raw streams: discovery, blocks of many MiB, hufgpu_block_index, hufgpu_decode_stream* */
#include "host/device.hpp"      /* memory, copies, fill, calibration, debug counters */
#include "host/batch.hpp"       /* hufgpu_encode_batch, hufgpu_decode_batch, the pinned staging area */
#include "host/ranges.hpp"      /* hufgpu_decode_ranges */
#include "host/gather.hpp"      /* hufgpu_gather */
#include "host/find.hpp"        /* hufgpu_find_bytes */
#include "host/select.hpp"      /* hufgpu_select_spans */
#include "host/update.hpp"      /* hufgpu_update_ranges, the row encoders */
#include "host/scatter.hpp"     /* hufgpu_scatter */
#include "host/append.hpp"      /* hufgpu_append, hufgpu_truncate */
#include "host/sub_build.hpp"   /* hufgpu_sub_index_from_raw, hufgpu_decode_build_sub, hufgpu_build_sub_index */
