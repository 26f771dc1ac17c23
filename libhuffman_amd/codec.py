"""Device-resident codec object over the hufgpu_* C ABI (include/huffman_gpu.h).

``GpuCodec`` works on torch uint8 tensors that already live in HBM: torch is used for device
memory and streams only, every byte of codec work happens in the HIP kernels of
``csrc/kernels/*.hpp`` (one translation unit, ``csrc/hufgpu_kernels.hip``) through the C ABI.
There is no eager/CPU path: constructing a codec without a usable MI355X raises
``HuffmanGpuError``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import torch

from . import _native

FILL_KINDS = {"const41": 0, "uniform256": 1, "uniform255": 2, "zipf255": 3}
FILL_SEEDS = {"const41": 0, "uniform256": 1, "uniform255": 2, "zipf255": 3}


class HuffmanGpuError(RuntimeError):
    def __init__(self, err: int, context: str, detail: str = ""):
        self.err = err
        self.raw = None
        msg = f"{_native.error_string(err)}. {context}"
        if detail:
            msg += f" ({detail})"
        super().__init__(msg)


class EncodedBatch:
    """What GpuCodec.encode_batch returns: the stream of many items back to back and where everything lies in it.

    stream        : uint8 device view of the whole stream (the items' streams back to back - one valid stream)
    offsets       : int64 device tensor, nblocks + 1 block header offsets in `stream` (the last = its length)
    item_blocks   : host list, nitems + 1: item i = blocks [item_blocks[i], item_blocks[i + 1])
    item_offsets  : host list, nitems + 1: item i = stream[item_offsets[i]:item_offsets[i + 1]]
    item_lens     : host list of the items' raw lengths, or None when not known (batch_from_streams without them)
    blocksize, row_blocksize, sub_index (int64 device tensor or None: the batch sub-index)
    """

    def __init__(self, stream, offsets, item_blocks, item_offsets, item_lens, blocksize, row_blocksize, sub_index=None):
        self.stream = stream
        self.offsets = offsets
        self.item_blocks = list(item_blocks)
        self.item_offsets = list(item_offsets)
        self.item_lens = None if item_lens is None else list(item_lens)
        self.blocksize = blocksize
        self.row_blocksize = row_blocksize
        self.sub_index = sub_index

    @property
    def nitems(self) -> int:
        return len(self.item_blocks) - 1

    @property
    def nblocks(self) -> int:
        return self.item_blocks[-1]

    @property
    def stream_len(self) -> int:
        return self.item_offsets[-1]

    def item_stream(self, i: int) -> torch.Tensor:
        """View of item i's stream: what GpuCodec.encode writes for the item alone."""
        return self.stream[self.item_offsets[i]: self.item_offsets[i + 1]]


def _u64_array(values):
    values = [int(v) for v in values]
    return (C.c_uint64 * max(1, len(values)))(*values)


class GpuCodec:
    """One codec context per device. Not thread-safe (like the reference's objects)."""

    def __init__(self, device: int = 0):
        self.lib = _native.load()
        self.device = device
        self._ctx = C.c_void_p()
        err = self.lib.hufgpu_ctx_create(C.byref(self._ctx), device)
        if err:
            raise HuffmanGpuError(err, "Failed to create the GPU codec context",
                                  self.lib.hufgpu_last_error(None).decode())
        self.tdev = torch.device("cuda", device)
        self._pending_decode = None

    def close(self):
        if self._ctx:
            self.lib.hufgpu_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ----------------------------------------------------------------------------
    def _check(self, err: int, what: str, raw: int | None = None):
        if err:
            e = HuffmanGpuError(err, what, self.lib.hufgpu_last_error(self._ctx).decode())
            e.raw = raw                 # decode: bytes delivered before the failure (src/decoder.c:69-91)
            raise e

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.tdev).cuda_stream)

    def block_count(self, n: int, blocksize: int) -> int:
        return int(self.lib.hufgpu_block_count(n, blocksize))

    def encode_bound(self, n: int, blocksize: int) -> int:
        return int(self.lib.hufgpu_encode_bound(n, blocksize))

    def sub_index_bytes(self, n: int, blocksize: int) -> int:
        """Size of the optional sub-index of an encode of n bytes (see include/huffman_gpu.h)."""
        return int(self.lib.hufgpu_sub_index_bytes(n, blocksize))

    def new_sub_index(self, n: int, blocksize: int) -> torch.Tensor:
        return torch.empty(max(1, (self.sub_index_bytes(n, blocksize) + 7) // 8), dtype=torch.int64, device=self.tdev)

    # -- hot path ---------------------------------------------------------------------------
    def histogram(self, data: torch.Tensor, blocksize: int) -> torch.Tensor:
        n = data.numel()
        nb = self.block_count(n, blocksize)
        hist = torch.empty((nb, 256), dtype=torch.int32, device=self.tdev)
        self._check(self.lib.hufgpu_histogram(self._ctx, data.data_ptr(), n, blocksize,
                                              hist.data_ptr(), self._stream()), "histogram failed")
        return hist

    def encode(self, data: torch.Tensor, blocksize: int, out: torch.Tensor | None = None,
               offsets: torch.Tensor | None = None, sync: bool = True, sub_index: torch.Tensor | None = None):
        """Returns (stream tensor view, offsets tensor[nblocks+1], length or None).  `sub_index`
        (from new_sub_index) also receives the encoder's sub-index for decode(..., sub_index=)."""
        assert data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()
        n = data.numel()
        nb = self.block_count(n, blocksize)
        if out is None:
            out = torch.empty(self.encode_bound(n, blocksize), dtype=torch.uint8, device=self.tdev)
        if offsets is None:
            offsets = torch.empty(nb + 1, dtype=torch.int64, device=self.tdev)
        out_len = C.c_uint64(0)
        if sub_index is not None:
            assert sub_index.numel() * sub_index.element_size() >= self.sub_index_bytes(n, blocksize)
            err = self.lib.hufgpu_encode_sub(self._ctx, data.data_ptr(), n, blocksize, out.data_ptr(),
                                             out.numel(), offsets.data_ptr(), sub_index.data_ptr(),
                                             C.byref(out_len) if sync else None, self._stream())
        else:
            err = self.lib.hufgpu_encode(self._ctx, data.data_ptr(), n, blocksize, out.data_ptr(),
                                         out.numel(), offsets.data_ptr(),
                                         C.byref(out_len) if sync else None, self._stream())
        self._check(err, "Failed to encode the data")
        if sync:
            return out[: out_len.value], offsets, int(out_len.value)
        return out, offsets, None

    def decode(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
               out: torch.Tensor, relaxed: bool = False, sync: bool = True,
               sub_index: torch.Tensor | None = None, raw_size: int = 0, blocksize: int = 0):
        """Indexed decode. Returns bytes written (sync) or None (enqueued only).  With `sub_index`
        (as written by encode of `raw_size` bytes in blocks of `blocksize`) every symbol is decoded
        once; the sub-index is verified on the device, never trusted."""
        raw = C.c_uint64(0)
        flags = _native.RELAXED_TREE if relaxed else _native.STRICT_TREE
        if sub_index is not None:
            assert self.block_count(raw_size, blocksize) == nblocks
            err = self.lib.hufgpu_decode_sub(self._ctx, stream.data_ptr(), stream_len, offsets.data_ptr(),
                                             raw_size, blocksize, sub_index.data_ptr(), out.data_ptr(),
                                             out.numel(), flags, C.byref(raw) if sync else None, self._stream())
        else:
            err = self.lib.hufgpu_decode(self._ctx, stream.data_ptr(), stream_len, offsets.data_ptr(),
                                         nblocks, out.data_ptr(), out.numel(), flags,
                                         C.byref(raw) if sync else None, self._stream())
        # an enqueued decode's buffers are read - and, after a failed block, written - by hufgpu_decode_result():
        # they stay referenced until then (include/huffman_gpu.h)
        self._pending_decode = None if sync else (stream, offsets, out, sub_index)
        self._check(err, "Failed to decode the data", raw=int(raw.value) if sync else None)
        return int(raw.value) if sync else None

    def decode_result(self) -> int:
        raw = C.c_uint64(0)
        try:
            self._check(self.lib.hufgpu_decode_result(self._ctx, C.byref(raw)), "Failed to decode the data", raw=int(raw.value))
        finally:
            self._pending_decode = None
        return int(raw.value)

    # -- batches: many independent inputs in one launch sequence -----------------------------
    def batch_geometry(self, item_lens, blocksize: int):
        """(nblocks, row_blocksize, out_bound, sub_index_bytes) of a batch (hufgpu_batch_geometry)."""
        lens = _u64_array(item_lens)
        nb, rbs, bound, subb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.hufgpu_batch_geometry(len(item_lens), lens, blocksize, C.byref(nb), C.byref(rbs),
                                                   C.byref(bound), C.byref(subb)), "batch geometry failed")
        return int(nb.value), int(rbs.value), int(bound.value), int(subb.value)

    def encode_batch(self, data: torch.Tensor, item_lens, blocksize: int, sub_index: bool = False) -> EncodedBatch:
        """Encode the items that lie back to back in `data` (item i = the item_lens[i] bytes behind the ones before it),
        each as hufgpu_encode would encode it alone, in one launch sequence.  Synchronises."""
        assert data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()
        item_lens = [int(x) for x in item_lens]
        if sum(item_lens) != data.numel():
            raise ValueError(f"the item lengths add up to {sum(item_lens)} bytes, the data holds {data.numel()}")
        nb, rbs, bound, subb = self.batch_geometry(item_lens, blocksize)
        out = torch.empty(max(1, bound), dtype=torch.uint8, device=self.tdev)
        offsets = torch.empty(nb + 1, dtype=torch.int64, device=self.tdev)
        sub = torch.empty(max(1, (subb + 7) // 8), dtype=torch.int64, device=self.tdev) if sub_index else None
        item_offs = (C.c_uint64 * (len(item_lens) + 1))()
        err = self.lib.hufgpu_encode_batch(self._ctx, data.data_ptr() if data.numel() else None, len(item_lens),
                                           _u64_array(item_lens), blocksize, out.data_ptr(), out.numel(),
                                           offsets.data_ptr(), None, sub.data_ptr() if sub is not None else None,
                                           item_offs, self._stream())
        self._check(err, "Failed to encode the batch")
        item_blocks = [0]
        for n in item_lens:
            item_blocks.append(item_blocks[-1] + self.block_count(n, blocksize))
        item_offsets = list(item_offs)
        return EncodedBatch(out[: item_offsets[-1]], offsets, item_blocks, item_offsets, item_lens, blocksize, rbs, sub)

    def decode_batch(self, batch: EncodedBatch, out: torch.Tensor | None = None, out_offsets=None, relaxed: bool = False):
        """Decode every item of `batch` into its slot out[out_offsets[i]:out_offsets[i + 1]] (default: the item lengths
        back to back).  Returns (out, errs, raw_lens): per item the error and the bytes delivered that hufgpu_decode of
        the item alone into its slot returns - per-item errors are returned, not raised."""
        n = batch.nitems
        if out_offsets is None:
            if batch.item_lens is None:
                raise ValueError("the batch does not know its item lengths: pass out_offsets")
            out_offsets = [0]
            for x in batch.item_lens:
                out_offsets.append(out_offsets[-1] + x)
        out_offsets = [int(x) for x in out_offsets]
        assert len(out_offsets) == n + 1
        if out is None:
            out = torch.empty(max(1, out_offsets[-1]), dtype=torch.uint8, device=self.tdev)
        assert out.dtype == torch.uint8 and out.is_cuda and out.numel() >= out_offsets[-1]
        errs = (C.c_int32 * max(1, n))()
        raws = (C.c_uint64 * max(1, n))()
        flags = _native.RELAXED_TREE if relaxed else _native.STRICT_TREE
        sub = batch.sub_index
        err = self.lib.hufgpu_decode_batch(self._ctx, batch.stream.data_ptr() if batch.stream.numel() else None,
                                           batch.stream_len, batch.offsets.data_ptr(), n, _u64_array(batch.item_blocks),
                                           _u64_array(out_offsets), sub.data_ptr() if sub is not None else None,
                                           batch.row_blocksize if sub is not None else 0, out.data_ptr(), flags,
                                           errs, raws, self._stream())
        if err == _native.HUF_ERROR_INVALID_ARGUMENT or err == _native.HUF_ERROR_FATAL:
            self._check(err, "Failed to decode the batch")
        return out, [int(errs[i]) for i in range(n)], [int(raws[i]) for i in range(n)]

    def batch_from_streams(self, items) -> EncodedBatch:
        """A batch for decode_batch from streams encoded one by one: items = [(stream, offsets) or
        (stream, offsets, raw_len), ...], stream = a uint8 device tensor of exactly the stream's bytes, offsets = its
        block index (nblocks + 1 int64, as encode returns it).  The streams are copied back to back and the indexes
        shifted to match.  Without raw lengths decode_batch needs out_offsets."""
        streams, offs, item_blocks, item_offsets, lens = [], [], [0], [0], []
        for it in items:
            stream, offsets = it[0], it[1]
            lens.append(int(it[2]) if len(it) > 2 else None)
            assert stream.dtype == torch.uint8
            o = offsets.to(device=self.tdev, dtype=torch.int64)
            if o.numel() == 0:
                o = torch.zeros(1, dtype=torch.int64, device=self.tdev)
            offs.append(o[:-1] + item_offsets[-1])
            streams.append(stream.to(self.tdev).reshape(-1))
            item_blocks.append(item_blocks[-1] + o.numel() - 1)
            item_offsets.append(item_offsets[-1] + stream.numel())
        offs.append(torch.tensor([item_offsets[-1]], dtype=torch.int64, device=self.tdev))
        stream = torch.cat(streams) if streams else torch.empty(0, dtype=torch.uint8, device=self.tdev)
        known = all(x is not None for x in lens)
        return EncodedBatch(stream, torch.cat(offs), item_blocks, item_offsets, lens if known else None, None, 0)

    # -- ranges: bytes [lo, hi) of the original data out of one indexed stream --------------------
    def decode_ranges(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, ranges,
                      out: torch.Tensor | None = None, out_offsets=None, relaxed: bool = False,
                      sub_index: torch.Tensor | None = None, raw_size: int = 0, blocksize: int = 0, tiles: bool = False):
        """Decode the byte ranges `ranges` = [(lo, hi), ...] of the original data, range i into its slot
        out[out_offsets[i]:out_offsets[i + 1]] (default: the range lengths back to back), in one launch sequence
        (hufgpu_decode_ranges).  Only the blocks a range touches are decoded.  Returns (out, errs, raw_lens): per range
        the error and the bytes delivered - per-range errors are returned, not raised.
        tiles=True (HUFGPU_RANGES_TILES): `sub_index` is vouched to be this stream's own, and of a cut block only the
        sub-index tiles that hold bytes of a range are decoded (the contract: include/huffman_gpu.h, TILES).  Without
        `sub_index` it does nothing."""
        ranges = [(int(lo), int(hi)) for lo, hi in ranges]
        n = len(ranges)
        if out_offsets is None:
            out_offsets = [0]
            for lo, hi in ranges:
                out_offsets.append(out_offsets[-1] + max(0, hi - lo))
        out_offsets = [int(x) for x in out_offsets]
        assert len(out_offsets) == n + 1
        if out is None:
            out = torch.empty(max(1, out_offsets[-1]), dtype=torch.uint8, device=self.tdev)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.numel() >= out_offsets[-1]
        errs = (C.c_int32 * max(1, n))()
        raws = (C.c_uint64 * max(1, n))()
        flags = (_native.RELAXED_TREE if relaxed else _native.STRICT_TREE) | (_native.RANGES_TILES if tiles else 0)
        err = self.lib.hufgpu_decode_ranges(self._ctx, stream.data_ptr() if stream.numel() else None, stream_len,
                                            offsets.data_ptr(), nblocks, n, _u64_array(lo for lo, _ in ranges),
                                            _u64_array(hi for _, hi in ranges), _u64_array(out_offsets),
                                            sub_index.data_ptr() if sub_index is not None else None,
                                            raw_size if sub_index is not None else 0,
                                            blocksize if sub_index is not None else 0, out.data_ptr(), flags,
                                            errs, raws, self._stream())
        if err == _native.HUF_ERROR_INVALID_ARGUMENT or err == _native.HUF_ERROR_FATAL:
            self._check(err, "Failed to decode the ranges")
        return out, [int(errs[i]) for i in range(n)], [int(raws[i]) for i in range(n)]

    def decode_range(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, lo: int, hi: int,
                     relaxed: bool = False, sub_index: torch.Tensor | None = None, raw_size: int = 0,
                     blocksize: int = 0, tiles: bool = False) -> torch.Tensor:
        """The bytes [lo, hi) of the original data (cut at its end) as a new tensor.  Raises HuffmanGpuError, with the
        bytes delivered in front of the failure in `.raw`, when a block of the range does not decode."""
        out, errs, raws = self.decode_ranges(stream, stream_len, offsets, nblocks, [(lo, hi)], relaxed=relaxed,
                                             sub_index=sub_index, raw_size=raw_size, blocksize=blocksize, tiles=tiles)
        self._check(errs[0], "Failed to decode the range", raw=raws[0])
        return out[: raws[0]]

    def ranges_counters(self):
        """How the last decode_ranges routed its blocks (hufgpu_ranges_counters): (direct, staged whole, served by
        tiles, (range, tile) items decoded, failed a tile check and decoded again, 0, 0, 0)."""
        c = (C.c_uint64 * 8)()
        self._check(self.lib.hufgpu_ranges_counters(self._ctx, c), "counter readout failed")
        return tuple(int(x) for x in c)

    # -- gather: records whose positions are on the GPU, enqueue-only ------------------------------
    def gather(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, positions: torch.Tensor,
               lengths, *, sub_index: torch.Tensor, raw_size: int, blocksize: int, max_len: int | None = None,
               out: torch.Tensor | None = None, relaxed: bool = False):
        """Record i = bytes [positions[i], positions[i] + length_i) of the original data into out[i, :length_i], on
        torch's current stream and without a synchronisation (hufgpu_gather): `positions` is a CUDA int64 / uint64
        tensor, `lengths` an int (every record that long) or a CUDA int32 tensor, with `max_len` their host-known
        bound.  `sub_index` is vouched to be this stream's own (the TILES contract of include/huffman_gpu.h).
        `out`: uint8 [nrecords, >= max_len], rows at any stride and alignment; made when not given.  Returns
        (out, errs, raw_lens), CUDA tensors: per record 0, or the status that says "not served here: ask
        decode_ranges" (HUF_ERROR_READ_WRITE; HUF_ERROR_INVALID_ARGUMENT for a length above max_len), and the
        record's length cut at raw_size.  Nothing is raised for a record."""
        assert positions.is_cuda and positions.dtype in (torch.int64, torch.uint64) and positions.dim() == 1
        positions = positions.contiguous()
        n = positions.numel()
        if isinstance(lengths, torch.Tensor):
            assert max_len is not None, "lengths on the device need max_len, their bound"
            assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.numel() == n
            lengths = lengths.contiguous()
            len_ptr = lengths.data_ptr() if n else None
        else:
            max_len = int(lengths) if max_len is None else int(max_len)
            assert int(lengths) == max_len, "a fixed record size is max_len"
            len_ptr = None
        max_len = int(max_len)
        if out is None:
            out = torch.empty((n, max_len), dtype=torch.uint8, device=self.tdev)
        assert out.dtype == torch.uint8 and out.is_cuda and out.dim() == 2 and out.size(0) == n and out.size(1) >= max_len
        assert out.size(1) <= 1 or out.stride(1) == 1
        stride = out.stride(0) if n > 1 else max(out.stride(0), out.size(1))
        errs = torch.zeros(n, dtype=torch.int32, device=self.tdev)
        raw_lens = torch.zeros(n, dtype=torch.int32, device=self.tdev)
        err = self.lib.hufgpu_gather(self._ctx, stream.data_ptr() if stream.numel() else None, stream_len,
                                     offsets.data_ptr(), nblocks, sub_index.data_ptr(), raw_size, blocksize, n,
                                     positions.data_ptr() if n else None, len_ptr, max_len,
                                     out.data_ptr() if out.numel() else None, stride, errs.data_ptr() if n else None,
                                     raw_lens.data_ptr() if n else None,
                                     _native.RELAXED_TREE if relaxed else _native.STRICT_TREE, self._stream())
        self._check(err, "Failed to enqueue the gather")
        return out, errs, raw_lens

    # -- find: where byte values lie in the original data, enqueue-only -------------------------------
    @staticmethod
    def byte_set(values) -> bytes:
        """the 32-byte set of hufgpu_find_bytes: bit v & 7 of byte v >> 3 is 1 for every v in `values`"""
        s = bytearray(32)
        for v in bytes(values) if isinstance(values, (bytes, bytearray)) else values:
            v = int(v)
            if not 0 <= v <= 255:
                raise ValueError(f"byte value {v} out of range")
            s[v >> 3] |= 1 << (v & 7)
        return bytes(s)

    def _find_buffer(self, given, n: int, dtype):
        """An output buffer of `n` items: `given` - contiguous, [n], of that dtype, on the device - or a new one"""
        buf = torch.empty(n, dtype=dtype, device=self.tdev) if given is None else given
        assert buf.is_cuda and buf.dtype == dtype and buf.dim() == 1 and buf.numel() == n and buf.is_contiguous()
        return buf

    def _find_args(self, stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, block_counts, relaxed):
        """What every find call's C argument list starts and ends with, around the call's own part, and the tensors the
        end points to: (head, tail, totals, errs, counts)"""
        totals = torch.empty(4, dtype=torch.int64, device=self.tdev)
        errs = torch.empty(nblocks, dtype=torch.int32, device=self.tdev)
        counts = torch.empty(nblocks, dtype=torch.int64, device=self.tdev) if block_counts else None
        head = (self._ctx, stream.data_ptr() if stream.numel() else None, stream_len, offsets.data_ptr() if nblocks else None,
                nblocks, sub_index.data_ptr() if nblocks else None, raw_size, blocksize)
        tail = (counts.data_ptr() if block_counts and nblocks else None, totals.data_ptr(), errs.data_ptr() if nblocks else None,
                _native.RELAXED_TREE if relaxed else _native.STRICT_TREE, self._stream())
        return head, tail, totals, errs, counts

    def find_bytes(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                   sub_index: torch.Tensor, raw_size: int, blocksize: int, values, max_positions: int = 0,
                   block_counts: bool = False, relaxed: bool = False, out: torch.Tensor | None = None):
        """The positions in the original data of the bytes whose value is in `values` (an iterable of ints or a
        `bytes`), on torch's current stream and without a synchronisation (hufgpu_find_bytes): no decoded byte is
        written to memory, and for any content of `sub_index` a block is served exactly or its status is non-zero.
        Returns CUDA tensors (positions[max_positions] int64 - the first totals[1] are written, ascending -,
        totals[4] = matches in served blocks, positions written, blocks not served, 0; block_errs[nblocks] int32,
        0 or HUF_ERROR_READ_WRITE = "ask decode"; block_counts[nblocks] int64 or None).  `out`: the positions' buffer,
        contiguous int64 [max_positions]; made when not given."""
        st = self.byte_set(values)
        max_positions = int(max_positions)
        pos = self._find_buffer(out, max_positions, torch.int64)
        head, tail, totals, errs, counts = self._find_args(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize,
                                                           block_counts, relaxed)
        err = self.lib.hufgpu_find_bytes(*head, st, pos.data_ptr() if max_positions else None, max_positions, *tail)
        self._check(err, "Failed to enqueue the search")
        return pos, totals, errs, counts

    def count_bytes(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                    sub_index: torch.Tensor, raw_size: int, blocksize: int, values, relaxed: bool = False):
        """How many bytes of the original data have a value in `values`: find_bytes without positions, enqueue-only.
        Returns CUDA tensors (totals[4], block_errs[nblocks]) as find_bytes does."""
        _, totals, errs, _ = self.find_bytes(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, values,
                                             relaxed=relaxed)
        return totals, errs

    ANY = bytes(range(256))         # the full class of byte_classes: a position that may hold any byte

    @staticmethod
    def byte_classes(pattern, ignore_case: bool = False) -> np.ndarray:
        """The classes of hufgpu_find_classes, uint8 [len(pattern)][32]: row k is the byte_set of the values that
        position k may hold.  A `bytes` / `bytearray` gives one value a position - with `ignore_case` both cases of an
        ASCII letter and nothing else; a `list` / `tuple` gives one class an item: an int, a `bytes` of the allowed values
        or an iterable of ints (GpuCodec.ANY: every value; `ignore_case` adds the other case of every letter of a class).
        Raises ValueError for a length outside 1 to FIND_PATTERN_MAX and for an empty class."""
        if isinstance(pattern, (list, tuple)):
            items = [[int(c)] if isinstance(c, (int, np.integer)) else list(bytes(c)) if isinstance(c, (bytes, bytearray, memoryview))
                     else [int(v) for v in c] for c in pattern]
        elif isinstance(pattern, str):
            raise TypeError("a pattern is a bytes-like object or a list / tuple of classes, not a str")
        else:
            items = [[v] for v in bytes(pattern)]            # any bytes-like object, as the literal route takes it
        if not 1 <= len(items) <= _native.FIND_PATTERN_MAX:
            raise ValueError(f"a pattern has 1 to {_native.FIND_PATTERN_MAX} positions, not {len(items)}")
        out = np.zeros((len(items), 32), np.uint8)
        for k, values in enumerate(items):
            if ignore_case:
                values = values + [v ^ 0x20 for v in values if 0x41 <= (v & ~0x20) <= 0x5a and v < 128]
            if not values:
                raise ValueError(f"class {k} of the pattern is empty: it matches nothing")
            out[k] = np.frombuffer(GpuCodec.byte_set(values), np.uint8)
        return out

    class AnyOf:
        """Several ALTERNATIVES for the `pattern` of find_pattern / count_pattern / find_records / count_records / grep
        (grep -e A -e B, grep -F -f words, grep -E 'A|B'): a match is a start at which at least one of them lies, and
        one call - one walk of the stream - looks for all of them (hufgpu_find_any / hufgpu_find_records_any).  Each
        alternative is what byte_classes takes: a bytes-like literal or a list / tuple of classes.  1 to FIND_PATTERN_MAX
        alternatives whose lengths sum to at most FIND_PATTERN_MAX (alt_classes checks that)."""
        __slots__ = ("alternatives",)

        def __init__(self, *alternatives):
            self.alternatives = tuple(alternatives)

        def __len__(self):
            return len(self.alternatives)

        def __iter__(self):
            return iter(self.alternatives)

        def __repr__(self):
            return "AnyOf(" + ", ".join(repr(a) for a in self.alternatives) + ")"

    class Opt:
        """An item of a `list` / `tuple` pattern or of an AnyOf alternative: a position that may be left out (grep -E 'x?').
        `cls` is what a position of byte_classes is: an int, a `bytes` of the allowed values or an iterable of ints.
        list(b"colo") + [GpuCodec.Opt(b"u"), ord("r")] is 'colou?r' (hufgpu_find_any_quant)."""
        __slots__ = ("cls",)

        def __init__(self, cls):
            self.cls = cls

        def __repr__(self):
            return f"Opt({self.cls!r})"

    class Rep:
        """An item as Opt: `lo` to `hi` copies of one position (grep -E 'x{lo,hi}'), that is `lo` required positions and
        `hi - lo` optional ones of the class `cls`.  Every copy takes one of the FIND_PATTERN_MAX positions."""
        __slots__ = ("cls", "lo", "hi")

        def __init__(self, cls, lo, hi):
            self.cls, self.lo, self.hi = cls, int(lo), int(hi)

        def __repr__(self):
            return f"Rep({self.cls!r}, {self.lo}, {self.hi})"

    class _Terms:
        """What AllOf and Seq share: 1 to FIND_TERMS_MAX items, each a bytes-like literal, a list / tuple of classes or an
        AnyOf - one TERM of hufgpu_find_records_terms."""
        __slots__ = ("items",)

        def __init__(self, *items):
            self.items = tuple(items)

        def __len__(self):
            return len(self.items)

        def __iter__(self):
            return iter(self.items)

        def __repr__(self):
            return type(self).__name__ + "(" + ", ".join(repr(a) for a in self.items) + ")"

    class AllOf(_Terms):
        """A `pattern` of find_records / count_records / grep: the records that hold EVERY item, anywhere and in any order,
        overlapping or not (grep A | grep B), in one walk of the stream (hufgpu_find_records_terms, HUFGPU_TERMS_ALL)."""
        __slots__ = ()

    class Seq(_Terms):
        """A `pattern` of find_records / count_records / grep: the records that hold the items one BEHIND the other without
        overlap, anything that is no delimiter between them (grep 'A.*B'; HUFGPU_TERMS_ORDERED).  The alternatives of an
        AnyOf item must have one length."""
        __slots__ = ()

    class Expr:
        """A whole grep -E line of this matcher's subset as the `pattern` of find_records / count_records / grep, and with one
        term of find_pattern / count_pattern (hufgpu_find_any_expr / hufgpu_find_records_expr): anchors, terms and optional
        positions TOGETHER.  Each term is a bytes-like literal, a list / tuple of classes with Opt / Rep items, or an AnyOf
        of those.  `ordered`: the terms one behind the other without overlap (grep 'A.*B'), else all of them anywhere
        (grep A | grep B).  `bol`, `eol`, `whole_line`, `word`, `word_bytes` are the keywords of find_records, carried by the
        Expr: with ordered terms they bind the OUTER edges ('^A.*B$'), and they do not go with `ordered=False` and several
        terms.  Of ordered terms only the LAST may hold Opt / Rep items or alternatives of several lengths.  GpuCodec.egrep()
        writes an Expr from a grep -E expression.  `ignore_case` and `delimiters` stay keywords of the methods."""
        __slots__ = ("terms", "ordered", "bol", "eol", "word", "word_bytes")

        def __init__(self, *terms, ordered=True, bol=False, eol=False, whole_line=False, word=False, word_bytes=None):
            self.terms, self.ordered = tuple(terms), bool(ordered)
            self.bol, self.eol = bool(bol or whole_line), bool(eol or whole_line)
            self.word, self.word_bytes = bool(word), word_bytes

        def __len__(self):
            return len(self.terms)

        def __iter__(self):
            return iter(self.terms)

        def __repr__(self):
            flags = [f"{k}={getattr(self, k)!r}" for k in ("bol", "eol", "word") if getattr(self, k)]
            flags += [] if self.ordered else ["ordered=False"]
            flags += [] if self.word_bytes is None else [f"word_bytes={self.word_bytes!r}"]
            return "Expr(" + ", ".join([repr(t) for t in self.terms] + flags) + ")"

    @staticmethod
    def expr_arrays(expr, ignore_case: bool = False, delimiters=b"\n"):
        """The host arrays of hufgpu_find_records_expr for an Expr, checked as the C call checks them: a dict of `classes`
        uint8 [total][32], `alt_lens` uint32 [n_alts], `optional` uint8 [total], `term_alts` uint32 [n_terms], `ordered`,
        `anchors` (the HUFGPU_ANCHOR bits), `delim_set` and `word_set` (byte_sets; the latter None without `word`).
        `delimiters` None: a search for positions, no class is looked at for delimiters.  Raises ValueError for no term or
        more than FIND_TERMS_MAX, `word_bytes` without `word`, anchors next to several terms with `ordered=False`, what
        quant_classes raises for a term (the message names the term), and for ordered terms an Opt / Rep item or alternatives
        of several lengths in a term other than the last (the message names the term, the alternative and the item), a class
        that holds a delimiter, and positions - plus one for every alternative whose byte behind is tested: with `eol` or
        `word` all of one term, the last term's otherwise - above FIND_PATTERN_MAX; TypeError for a term that is a str, an
        AllOf, a Seq or an Expr."""
        if not isinstance(expr, GpuCodec.Expr):
            raise TypeError("expr_arrays takes a GpuCodec.Expr")
        n_terms = len(expr)
        if not 1 <= n_terms <= _native.FIND_TERMS_MAX:
            raise ValueError(f"Expr has 1 to {_native.FIND_TERMS_MAX} terms, not {n_terms}")
        if expr.word_bytes is not None and not expr.word:
            raise ValueError("`word_bytes` says what `word` looks at: give `word=True` with it")
        bits = ((_native.ANCHOR_BOL if expr.bol else 0) | (_native.ANCHOR_EOL if expr.eol else 0) |
                (_native.ANCHOR_WORD if expr.word else 0))
        if bits and n_terms > 1 and not expr.ordered:
            raise ValueError(f"anchors do not go with `ordered=False` and {n_terms} terms: which term would they bind?")
        rows, lens, opts, counts = [], [], [], []
        for t, term in enumerate(expr):
            if isinstance(term, (str, GpuCodec._Terms, GpuCodec.Expr)):
                raise TypeError(f"term {t} is a {type(term).__name__}: a term is a bytes-like literal, a list / tuple of classes "
                                "or an AnyOf")
            alts = term if isinstance(term, GpuCodec.AnyOf) else GpuCodec.AnyOf(term)
            if len(alts) == 0:
                raise ValueError(f"term {t} has no alternative: no record would hold it")
            inner = expr.ordered and t + 1 < n_terms                   # a term in front of another: one length, no optional position
            for j, alt in enumerate(alts if inner else ()):
                for k, c in enumerate(alt if isinstance(alt, (list, tuple)) else ()):
                    if isinstance(c, (GpuCodec.Opt, GpuCodec.Rep)):
                        raise ValueError(f"term {t}, alternative {j}, item {k} is {c!r}: of ordered terms only the last may hold "
                                         "optional positions")
            try:
                c, l, o = GpuCodec.quant_classes(alts, ignore_case)
            except ValueError as e:
                raise ValueError(f"term {t}: {e}") from None
            if inner and len(set(l.tolist())) > 1:
                raise ValueError(f"term {t} has alternatives of the lengths {sorted(set(l.tolist()))}: of ordered terms only the "
                                 "last may have several")
            rows.append(c), lens.append(l), opts.append(o), counts.append(len(l))
        classes, alt_lens, optional = np.concatenate(rows), np.concatenate(lens), np.concatenate(opts)
        behind = bits & (_native.ANCHOR_EOL | _native.ANCHOR_WORD)
        total = int(alt_lens.sum()) + (counts[-1] if behind else 0)
        if len(alt_lens) > _native.FIND_PATTERN_MAX or total > _native.FIND_PATTERN_MAX:
            raise ValueError(f"the {len(alt_lens)} alternatives' positions" + (f" and one position behind each of the {counts[-1]} "
                             "whose byte behind is tested" if behind else "") + f" sum to {total}, above {_native.FIND_PATTERN_MAX}")
        st = None if delimiters is None else GpuCodec.byte_set(delimiters)
        both = classes & np.frombuffer(st, np.uint8) if st is not None else None
        if both is not None and both.any():
            row = int(np.flatnonzero(both.any(axis=1))[0])
            v = int(np.flatnonzero(np.unpackbits(both[row], bitorder="little"))[0])
            j = int(np.searchsorted(np.cumsum(alt_lens), row, side="right"))
            t = int(np.searchsorted(np.cumsum(counts), j, side="right"))
            raise ValueError(f"term {t}: class {row - int(alt_lens[:j].sum())} of alternative {j - int(sum(counts[:t]))} holds a "
                             f"delimiter (value {v}): a match lies inside one record")
        ws = GpuCodec.byte_set(GpuCodec.WORD_BYTES if expr.word_bytes is None else expr.word_bytes) if expr.word else None
        return {"classes": classes, "alt_lens": alt_lens, "optional": optional, "term_alts": np.array(counts, np.uint32),
                "ordered": expr.ordered, "anchors": bits, "delim_set": st, "word_set": ws}

    @staticmethod
    def _expr_alone(pattern, bol, eol, whole_line, word, word_bytes):
        """an Expr carries its anchors: the methods' anchor keywords next to one are a ValueError"""
        if bol or eol or whole_line or word or word_bytes is not None:
            raise ValueError("`bol`, `eol`, `whole_line`, `word` and `word_bytes` next to an Expr: the Expr carries its anchors")

    @staticmethod
    def egrep(expr: bytes, delimiters=b"\n", ignore_case: bool = False):
        """A grep -E line of this matcher's subset, compiled on the host to a GpuCodec.Expr.  regex()'s grammar - its parser -
        and besides: '^' at the start and '$' at the end of an alternative; '\\<' at its start with '\\>' at its end, or '\\b'
        at both, for `word`; and, in an expression without a top-level '|', a top-level '.*' that splits it into ordered terms,
        FIND_TERMS_MAX at most.  A leading '.*' is dropped together with a '^' in front of it, a trailing one together with a
        '$' behind it.  Raises ValueError ("egrep: offset N: ...") for what regex() raises it for - 'x*', 'x+', '.+', '{m,}' and
        groups among it - and for an anchor anywhere else, '\\b' inside a term or at one end only, alternatives that do not all
        carry the same anchors (anchors per alternative are out of scope), a quantified term in front of a '.*', '.*' next to
        '|', and more than FIND_TERMS_MAX terms."""
        alts = GpuCodec._regex_parse(expr, delimiters, ignore_case, "egrep", True)
        for alt in alts:
            if alt["wl"] != alt["wr"]:
                raise ValueError(f"egrep: offset {alt['at']}: a word's edge at one end of the alternative only: '\\<' and '\\>' "
                                 "(or '\\b' and '\\b') stand at both")
            if any(alt[k] != alts[0][k] for k in ("bol", "eol", "wl")):
                raise ValueError(f"egrep: offset {alt['at']}: the alternatives do not carry the same anchors: anchors per "
                                 "alternative are not in this matcher")
        first = alts[0]
        terms = first["terms"] if len(alts) == 1 else [GpuCodec.AnyOf(*(alt["terms"][0] for alt in alts))]
        return GpuCodec.Expr(*terms, ordered=True, bol=first["bol"], eol=first["eol"], word=first["wl"])

    @staticmethod
    def _find_terms(pattern, ignore_case, delimiters, anchors):
        """(key, st, term_alts, n_terms, mode) of hufgpu_find_records_terms for an AllOf / Seq of two items or more: the
        any-of table of all items' alternatives, one behind the other, as _find_route makes it, the delimiters' byte_set,
        and the host array of the alternatives a term.  Raises ValueError for no item or more than FIND_TERMS_MAX, for any
        of `bol` / `eol` / `whole_line` / `word` and for a Seq item whose alternatives differ in length; TypeError for an
        AllOf / Seq inside another one."""
        bol, eol, whole_line, word, word_bytes = anchors
        name = type(pattern).__name__
        if bol or eol or whole_line or word or word_bytes is not None:
            raise ValueError(f"`bol`, `eol`, `whole_line` and `word` do not go with {name}: an anchored search has one term")
        if not 1 <= len(pattern) <= _native.FIND_TERMS_MAX:
            raise ValueError(f"{name} has 1 to {_native.FIND_TERMS_MAX} items, not {len(pattern)}")
        flat, counts = [], []
        for t, item in enumerate(pattern):
            if isinstance(item, GpuCodec._Terms):
                raise TypeError(f"item {t} of {name} is {type(item).__name__}: AllOf and Seq do not nest")
            alts = list(item) if isinstance(item, GpuCodec.AnyOf) else [item]
            if GpuCodec._is_quant(GpuCodec.AnyOf(*alts)):
                raise ValueError(f"item {t} of {name} holds an Opt or a Rep: a pattern with optional positions has one term")
            if not alts:
                raise ValueError(f"item {t} of {name} has no alternative: no record would hold it")
            if isinstance(pattern, GpuCodec.Seq) and len({len(a) for a in alts if not isinstance(a, str)}) > 1:
                raise ValueError(f"item {t} of Seq has alternatives of the lengths {sorted({len(a) for a in alts})}: "
                                 "'A.*B' needs one length an item")
            flat += alts
            counts.append(len(alts))
        _, key, st = GpuCodec._find_route(GpuCodec.AnyOf(*flat), ignore_case, delimiters, True)
        mode = _native.TERMS_ORDERED if isinstance(pattern, GpuCodec.Seq) else _native.TERMS_ALL
        return key, st, np.array(counts, np.uint32).tobytes(), len(counts), mode

    @staticmethod
    def alt_classes(anyof, ignore_case: bool = False):
        """The two host arrays of hufgpu_find_any for an AnyOf: (classes uint8 [total][32] - the alternatives' byte_classes
        one behind the other -, alt_lens uint32 [n]).  `ignore_case` applies to every alternative.  Raises ValueError for
        no alternative or more than FIND_PATTERN_MAX, for an alternative of length 0, for lengths that sum to more than
        FIND_PATTERN_MAX and for an empty class (the message names the alternative)."""
        if not isinstance(anyof, GpuCodec.AnyOf):
            raise TypeError("alt_classes takes a GpuCodec.AnyOf")
        n = len(anyof)
        if not 1 <= n <= _native.FIND_PATTERN_MAX:
            raise ValueError(f"an AnyOf has 1 to {_native.FIND_PATTERN_MAX} alternatives, not {n}")
        rows = []
        for j, alt in enumerate(anyof):
            if isinstance(alt, (str, GpuCodec._Terms)):
                raise TypeError(f"an alternative is a bytes-like object or a list / tuple of classes, not a {type(alt).__name__}")
            if len(alt) == 0:
                raise ValueError(f"alternative {j} has length 0: it would match everywhere")
            try:
                rows.append(GpuCodec.byte_classes(alt, ignore_case))
            except ValueError as e:
                raise ValueError(f"alternative {j}: {e}") from None
        total = sum(len(r) for r in rows)
        if total > _native.FIND_PATTERN_MAX:
            raise ValueError(f"the alternatives' lengths sum to {total}, above {_native.FIND_PATTERN_MAX}")
        return np.concatenate(rows), np.array([len(r) for r in rows], np.uint32)

    @staticmethod
    def _is_quant(pattern) -> bool:
        """does a pattern - a list / tuple, or an AnyOf of such - hold an Opt or a Rep"""
        alts = pattern if isinstance(pattern, GpuCodec.AnyOf) else (pattern,)
        return any(isinstance(a, (list, tuple)) and any(isinstance(c, (GpuCodec.Opt, GpuCodec.Rep)) for c in a) for a in alts)

    @staticmethod
    def quant_classes(pattern, ignore_case: bool = False):
        """The three host arrays of hufgpu_find_any_quant for a pattern with Opt / Rep items - a list / tuple, or an AnyOf
        of alternatives -: (classes uint8 [total][32], alt_lens uint32 [n], optional uint8 [total]), a Rep written out as
        its `lo` required and `hi - lo` optional positions.  `ignore_case` applies to every class.  Raises ValueError for what
        alt_classes raises it for - the lengths count every copy of a Rep -, for a Rep with lo < 0, lo > hi or hi = 0 and
        for an alternative whose positions are all optional; the message names the alternative and the item."""
        if not isinstance(pattern, GpuCodec.AnyOf):
            if isinstance(pattern, (str, GpuCodec._Terms)):
                raise TypeError(f"a pattern is a bytes-like object, a list / tuple of classes or an AnyOf, not a {type(pattern).__name__}")
            pattern = GpuCodec.AnyOf(pattern)
        flat, flags = [], []
        for j, alt in enumerate(pattern):
            items, opt = [], []
            for k, c in enumerate(alt if isinstance(alt, (list, tuple)) else ()):
                if isinstance(c, GpuCodec.Rep):
                    if c.lo < 0 or c.lo > c.hi:
                        raise ValueError(f"alternative {j}, item {k}: Rep from {c.lo} to {c.hi} copies: 0 <= lo <= hi")
                    if c.hi == 0:
                        raise ValueError(f"alternative {j}, item {k}: Rep of at most 0 copies: leave the item out")
                    items += [c.cls] * c.hi
                    opt += [0] * c.lo + [1] * (c.hi - c.lo)
                else:
                    items.append(c.cls if isinstance(c, GpuCodec.Opt) else c)
                    opt.append(int(isinstance(c, GpuCodec.Opt)))
                if len(items) > _native.FIND_PATTERN_MAX:
                    raise ValueError(f"alternative {j}, item {k}: the positions come to {len(items)}, above {_native.FIND_PATTERN_MAX}")
            if not isinstance(alt, (list, tuple)):
                items, opt = alt, [0] * len(alt)                    # (a literal; alt_classes words a str)
            elif items and all(opt):
                raise ValueError(f"alternative {j}: every position is optional: it would match everywhere")
            flat.append(items)
            flags += opt
        classes, lens = GpuCodec.alt_classes(GpuCodec.AnyOf(*flat), ignore_case)
        return classes, lens, np.array(flags, np.uint8)

    _REGEX_SETS = {ord("d"): b"0123456789", ord("w"): b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_",
                   ord("s"): b" \t\n\r\f\v"}
    _REGEX_CHARS = {ord("n"): 10, ord("t"): 9, ord("r"): 13, ord("f"): 12, ord("v"): 11}
    _REGEX_META = b"\\.[]{}()*+?|^$-/"

    @staticmethod
    def regex(expr: bytes, delimiters=b"\n", ignore_case: bool = False):
        """A subset of grep -E, compiled on the host to the pattern that find_pattern / find_records / grep take: an AnyOf of
        lists with Opt / Rep items, one alternative a top-level '|'.  Taken: literal bytes; '\\' in front of a metacharacter;
        \\n \\t \\r \\f \\v \\xHH; \\d \\w \\s and \\D \\W \\S; '.'; '[...]' with ranges, a leading '^' and the escapes above (a ']'
        right behind the '[' or '[^' is a member); and behind a single position '?', '{m}', '{m,n}' and '{,n}'.  '.', a negated
        set and \\D \\W \\S never hold one of `delimiters`, as a line of grep never holds a newline.  `ignore_case` adds the
        other case of every ASCII letter of every class, in front of a set's negation.  Every position, a repeat's every copy, takes one of the
        FIND_PATTERN_MAX positions that the alternatives share.
        Raises ValueError, naming the offset in `expr`, for '*', '+' and '{m,}' (unbounded: not in this matcher), for '(' and
        ')' (no groups), '^' and '$' (the `bol` / `eol` keywords anchor a pattern without repeats), a quantifier with nothing
        to repeat, a bad '{...}', a bad range or escape, a set without its ']', an empty alternative or class, a repeat of at
        most 0 copies, and a total above FIND_PATTERN_MAX positions."""
        return GpuCodec.AnyOf(*(alt["terms"][0] for alt in GpuCodec._regex_parse(expr, delimiters, ignore_case, "regex", False)))

    @staticmethod
    def _regex_parse(expr, delimiters, ignore_case, who, extended):
        """The parser that regex() and egrep() share: a list of one dict an alternative, {"terms": the lists of items that a
        top-level '.*' separates - regex(): always one -, "bol", "eol", "wl", "wr": the anchors at its two ends, "at": its
        offset}.  `extended` (egrep): '^', '\\<' and '\\b' at the start of an alternative, '$', '\\>' and '\\b' at its end, and
        a top-level '.*' are taken; without it they are the errors that regex() documents."""
        expr = bytes(expr)
        delims = set(bytes(delimiters) if isinstance(delimiters, (bytes, bytearray)) else [int(v) for v in delimiters])
        n = len(expr)

        def bad(at, why):
            return ValueError(f"{who}: offset {at}: {why}")

        def fold(values):
            return set(values) | ({v ^ 0x20 for v in values if 0x41 <= (v & ~0x20) <= 0x5a and v < 128} if ignore_case else set())

        def negated(values):
            return set(range(256)) - fold(values) - delims

        def escape(at, in_set):
            """the class of the escape whose '\\' stands at `at`, and the offset behind it"""
            if at + 1 >= n:
                raise bad(at, "a '\\' at the end")
            c = expr[at + 1]
            if c in GpuCodec._REGEX_SETS:
                return set(GpuCodec._REGEX_SETS[c]), at + 2
            if c in b"DWS":
                if in_set:
                    raise bad(at, f"'\\{chr(c)}' inside a set")
                return negated(GpuCodec._REGEX_SETS[c | 0x20]), at + 2
            if c in GpuCodec._REGEX_CHARS:
                return {GpuCodec._REGEX_CHARS[c]}, at + 2
            if c == ord("x"):
                digits = expr[at + 2:at + 4]
                if len(digits) != 2 or any(d not in b"0123456789abcdefABCDEF" for d in digits):
                    raise bad(at, "'\\x' needs two hex digits")
                return {int(digits, 16)}, at + 4
            if c in GpuCodec._REGEX_META:
                return {c}, at + 2
            raise bad(at, f"the escape '\\{chr(c)}' is not in this subset")

        def bracket(at):
            """the class of the set whose '[' stands at `at`, and the offset behind its ']'"""
            i = at + 1
            neg = i < n and expr[i] == ord("^")
            i += neg
            values, first = set(), True
            while True:
                if i >= n:
                    raise bad(at, "a '[' without its ']'")
                if expr[i] == ord("]") and not first:
                    break
                first = False
                single = True
                if expr[i] == ord("\\"):
                    lo, j = escape(i, True)
                    single = len(lo) == 1 and expr[i + 1] not in GpuCodec._REGEX_SETS
                else:
                    lo, j = {expr[i]}, i + 1
                if j + 1 < n and expr[j] == ord("-") and expr[j + 1] != ord("]"):
                    if expr[j + 1] == ord("\\"):
                        hi, k = escape(j + 1, True)
                        hi_single = len(hi) == 1 and expr[j + 2] not in GpuCodec._REGEX_SETS
                    else:
                        hi, k, hi_single = {expr[j + 1]}, j + 2, True
                    a, b = min(lo), min(hi)
                    if not single or not hi_single or a > b:
                        raise bad(i, "a bad range")
                    lo, j = set(range(a, b + 1)), k
                values |= lo
                i = j
            return (negated(values) if neg else values), i + 1

        def repeat(at):
            """(lo, hi, the offset behind) of the quantifier at `at`, None when there is none"""
            if at >= n or expr[at] not in b"?*+{":
                return None
            if expr[at] == ord("?"):
                return 0, 1, at + 1
            if expr[at] != ord("{"):
                raise bad(at, f"'{chr(expr[at])}' is unbounded: not in this matcher")
            end = expr.find(b"}", at)
            body = expr[at + 1:end] if end >= 0 else b""
            parts = body.split(b",")
            if end < 0 or len(parts) > 2 or any(p and not p.isdigit() for p in parts) or not any(parts):
                raise bad(at, "a bad '{...}': {m}, {m,n} or {,n}")
            if len(parts) == 2 and not parts[1]:
                raise bad(at, "'{m,}' is unbounded: not in this matcher")
            lo = int(parts[0] or 0)
            hi = int(parts[1]) if len(parts) == 2 else lo
            if lo > hi:
                raise bad(at, f"a repeat from {lo} to {hi}")
            if hi == 0:
                raise bad(at, "a repeat of at most 0 copies")
            return lo, hi, end + 1

        def quantified(term):
            return any(isinstance(c, (GpuCodec.Opt, GpuCodec.Rep)) for c in term)

        def alt_ends(at):
            """does the alternative end at `at`, but for a '$'"""
            at += at < n and expr[at] == ord("$")
            return at >= n or expr[at] == ord("|")

        def new_alt(at):
            return {"terms": [], "bol": False, "eol": False, "wl": False, "wr": False, "at": at, "star": None}

        # (egrep) split_at: the offset of a '.*' behind which no item has come yet; lead: it stood in front of the first item
        alts, alt, items, total, i, alt_at, split_at, lead = [], new_alt(0), [], 0, 0, 0, None, False
        while True:
            if i >= n or expr[i] == ord("|"):
                if alt["star"] is not None and (alts or i < n):
                    raise bad(alt["star"], "'.*' next to '|': an expression has alternatives or terms, not both")
                if split_at is not None and not lead:                 # a trailing '.*', and a '$' behind it: nothing to test
                    if alt["wr"]:
                        raise bad(split_at, "'.*' in front of a word's end: '\\b' would stand inside a term")
                    alt["eol"] = False
                elif not items:
                    raise bad(alt_at, "an empty alternative: it would match everywhere")
                else:
                    alt["terms"].append(items)
                for term in alt["terms"]:
                    if all(isinstance(c, GpuCodec.Opt) or (isinstance(c, GpuCodec.Rep) and c.lo == 0) for c in term):
                        raise bad(alt_at, "every position of the alternative is optional: it would match everywhere"
                                  if len(alt["terms"]) == 1 else "every position of a term is optional: it would match everywhere")
                if not alt["terms"]:
                    raise bad(alt_at, "an empty alternative: it would match everywhere")
                alts.append(alt)
                if i >= n:
                    break
                items, i, split_at, lead = [], i + 1, None, False
                alt_at, alt = i, new_alt(i)
                continue
            at, c = i, expr[i]
            if c in b"?*+{":
                raise bad(at, f"'{chr(c)}' has nothing to repeat")
            if c in b"()":
                raise bad(at, f"'{chr(c)}': groups are not in this matcher")
            if c in b"^$" and not extended:
                raise bad(at, f"'{chr(c)}': anchors are keywords of the calls (bol, eol), not part of the expression")
            fresh = not items and not alt["terms"] and split_at is None   # nothing of the alternative but anchors has come
            if c == ord("^"):
                if not fresh or alt["bol"] or alt["wl"]:
                    raise bad(at, "'^' stands at the start of an alternative")
                alt["bol"], i = True, at + 1
                continue
            if c == ord("$"):
                if not (at + 1 >= n or expr[at + 1] == ord("|")) or fresh:
                    raise bad(at, "'$' stands at the end of an alternative")
                alt["eol"], i = True, at + 1
                continue
            if extended and c == ord("\\") and at + 1 < n and expr[at + 1] in b"<>b":
                k = expr[at + 1]
                if k != ord(">") and fresh and not alt["wl"]:
                    alt["wl"] = True
                elif k != ord("<") and not fresh and not alt["wr"] and alt_ends(at + 2):
                    alt["wr"] = True
                else:
                    raise bad(at, f"'\\{chr(k)}' inside a term: a word's edges stand at the two ends of an alternative")
                i = at + 2
                continue
            if extended and c == ord(".") and at + 1 < n and expr[at + 1] == ord("*"):
                if at + 2 < n and expr[at + 2] in b"?*+{":
                    raise bad(at + 2, f"'{chr(expr[at + 2])}' behind a quantifier has nothing to repeat")
                if fresh:                                               # a leading '.*', and a '^' in front of it: nothing to test
                    if alt["wl"]:
                        raise bad(at, "'.*' behind a word's start: '\\b' would stand inside a term")
                    alt["bol"], lead = False, True
                elif items:
                    alt["terms"].append(items)
                    items, lead = [], False
                if split_at is None:
                    split_at = at
                if alt["star"] is None:
                    alt["star"] = at
                i = at + 2
                continue
            if split_at is not None and not lead:                       # an item behind a '.*': the term in front must have one length
                if quantified(alt["terms"][-1]):
                    raise bad(split_at, "a quantified term in front of a '.*': only the last term may hold '?' or '{m,n}'")
                if len(alt["terms"]) >= _native.FIND_TERMS_MAX:
                    raise bad(split_at, f"more than {_native.FIND_TERMS_MAX} terms")
            split_at, lead = None, False
            if c == ord("\\"):
                values, i = escape(at, False)
            elif c == ord("["):
                values, i = bracket(at)
            elif c == ord("."):
                values, i = negated(()), at + 1
            else:
                values, i = {c}, at + 1
            values = fold(values)
            if not values:
                raise bad(at, "an empty class: it matches nothing")
            cls = bytes(sorted(values))
            rep = repeat(i)
            copies = 1
            if rep is None:
                items.append(cls)
            else:
                lo, copies, i = rep
                if i < n and expr[i] in b"?*+{":
                    raise bad(i, f"'{chr(expr[i])}' behind a quantifier has nothing to repeat")
                items.append(GpuCodec.Opt(cls) if (lo, copies) == (0, 1) else GpuCodec.Rep(cls, lo, copies))
            total += copies
            if total > _native.FIND_PATTERN_MAX:
                raise bad(at, f"the positions come to {total}, above {_native.FIND_PATTERN_MAX}")
        return alts

    _NO_RECORDS = object()          # _find_route's `delimiters` of the calls that have none

    # route -> the C call that gives positions, the one that gives records
    _FIND_CALLS = {"literal": ("hufgpu_find_pattern", "hufgpu_find_records"),
                   "classes": ("hufgpu_find_classes", "hufgpu_find_records_classes"),
                   "any": ("hufgpu_find_any", "hufgpu_find_records_any"),
                   "quant": ("hufgpu_find_any_quant", "hufgpu_find_records_quant"),
                   "expr": ("hufgpu_find_any_expr", "hufgpu_find_records_expr")}

    WORD_BYTES = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_"     # grep -w's: [A-Za-z0-9_]

    @staticmethod
    def _find_route(pattern, ignore_case, delimiters=_NO_RECORDS, select=False, anchors=None):
        """(route, key, st): which of _FIND_CALLS serves `pattern` - "any" for an AnyOf (and, with `select`, for every
        pattern: it is the one alternative), "classes" for a list / tuple or with `ignore_case`, else "literal" -, the
        pattern's part of the C argument list, and the delimiters' byte_set (None when no `delimiters` are given: no records).
        Raises what find_pattern and find_records raise for a pattern.
        `anchors`: the keywords (bol, eol, whole_line, word, word_bytes) of the calls that have them.  A fourth item then
        comes back, (bits, word_set): the `anchors` of hufgpu_find_any_anchored / hufgpu_find_records_anchored - 0: the call
        is the one it always was - and the word bytes' byte_set (None without `word`); any bit makes the route "any".  Raises
        ValueError for `word_bytes` without `word` and for alternatives that leave no bit of the matcher's state for the
        byte behind each of them (`eol`, `whole_line`, `word`)."""
        if anchors is not None:
            bol, eol, whole_line, word, word_bytes = anchors
            if word_bytes is not None and not word:
                raise ValueError("`word_bytes` says what `word` looks at: give `word=True` with it")
            bits = ((_native.ANCHOR_BOL if bol or whole_line else 0) | (_native.ANCHOR_EOL if eol or whole_line else 0) |
                    (_native.ANCHOR_WORD if word else 0))
            ws = GpuCodec.byte_set(GpuCodec.WORD_BYTES if word_bytes is None else word_bytes) if word else None
            if bits and GpuCodec._is_quant(pattern):
                raise ValueError("`bol`, `eol`, `whole_line` and `word` do not go with Opt / Rep: an anchored search has no optional positions")
            route, key, st = GpuCodec._find_route(pattern, ignore_case, delimiters, select or bits != 0)
            if bits & (_native.ANCHOR_EOL | _native.ANCHOR_WORD):
                total = int(np.frombuffer(key[1], np.uint32).sum()) + key[2]
                if total > _native.FIND_PATTERN_MAX:
                    raise ValueError(f"the alternatives' lengths and one position behind each of the {key[2]} sum to {total}, "
                                     f"above {_native.FIND_PATTERN_MAX}: `eol`, `whole_line` and `word` take a bit of the matcher's "
                                     "state an alternative")
            return route, key, st, (bits, ws)
        if select and not isinstance(pattern, GpuCodec.AnyOf):
            if isinstance(pattern, str):
                raise TypeError("a pattern is a bytes-like object or a list / tuple of classes, not a str")
            pattern = GpuCodec.AnyOf(pattern)
        alts = classes = optional = None
        if GpuCodec._is_quant(pattern):
            *alts, optional = GpuCodec.quant_classes(pattern, ignore_case)
        elif isinstance(pattern, GpuCodec.AnyOf):
            alts = GpuCodec.alt_classes(pattern, ignore_case)
        elif isinstance(pattern, (list, tuple)) or ignore_case:
            classes = GpuCodec.byte_classes(pattern, ignore_case)      # (raises for a wrong length)
        st = None if delimiters is GpuCodec._NO_RECORDS else GpuCodec.byte_set(delimiters)
        if alts is None and classes is None:
            pattern = bytes(pattern)
            plen = len(pattern)
            if not 1 <= plen <= _native.FIND_PATTERN_MAX:
                raise ValueError(f"a pattern has 1 to {_native.FIND_PATTERN_MAX} bytes, not {plen}")
            for v in pattern if st is not None else ():
                if st[v >> 3] >> (v & 7) & 1:
                    raise ValueError(f"byte value {v} of the pattern is a delimiter: a match lies inside one record")
            return "literal", (pattern, plen), st
        rows = classes if alts is None else alts[0]
        both = rows & np.frombuffer(st, np.uint8) if st is not None else None
        if both is not None and both.any():
            row = int(np.flatnonzero(both.any(axis=1))[0])
            v = int(np.flatnonzero(np.unpackbits(both[row], bitorder="little"))[0])
            where = f"class {row} of the pattern"
            if alts is not None:
                j = int(np.searchsorted(np.cumsum(alts[1]), row, side="right"))
                where = f"class {row - int(alts[1][:j].sum())} of alternative {j}"
            raise ValueError(f"{where} holds a delimiter (value {v}): a match lies inside one record")
        if alts is None:
            return "classes", (classes.tobytes(), len(classes)), st
        if optional is not None:
            return "quant", (alts[0].tobytes(), alts[1].tobytes(), len(alts[1]), optional.tobytes()), st
        return "any", (alts[0].tobytes(), alts[1].tobytes(), len(alts[1])), st

    @staticmethod
    def _find_context(before, after, context):
        """(before, after) of hufgpu_find_records_context from the three keywords of find_records / count_records / grep:
        `context` sets both.  Raises ValueError for `context` next to one of the two, and for a distance that is negative
        or above 2^32 - 1."""
        if context is not None:
            if before or after:
                raise ValueError("`context` sets both `before` and `after`: give it or them")
            before = after = context
        before, after = int(before), int(after)
        for name, v in (("before", before), ("after", after)):
            if not 0 <= v <= 0xFFFFFFFF:
                raise ValueError(f"`{name if context is None else 'context'}` is 0 to 2^32 - 1 records, not {v}")
        return before, after

    def find_pattern(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                     sub_index: torch.Tensor, raw_size: int, blocksize: int, pattern, max_positions: int = 0,
                     block_counts: bool = False, relaxed: bool = False, out: torch.Tensor | None = None,
                     ignore_case: bool = False, bol: bool = False, eol: bool = False, whole_line: bool = False,
                     word: bool = False, word_bytes=None, delimiters=b"\n"):
        """The positions in the original data at which `pattern` (1 to FIND_PATTERN_MAX bytes) starts, overlapping
        occurrences included, on torch's current stream and without a synchronisation (hufgpu_find_pattern).  Returns
        what find_bytes returns, (positions, totals, block_errs, block_counts): a match counts for the block that holds
        its start, and it is reported only when every block it touches is served - totals[2] and block_errs say which
        seams are open.  Raises ValueError for an empty or over-long pattern.
        A `list` / `tuple` pattern is one of CLASSES, a set of byte values a position as byte_classes takes them, and
        `ignore_case` makes classes of a literal's letters (hufgpu_find_classes): a match is a start p with data[p + k] in
        class k for every k.  A bytes-like pattern without `ignore_case` makes the literal call.
        A GpuCodec.AnyOf pattern looks for SEVERAL alternatives in the one walk (hufgpu_find_any): a start at which at least
        one of them lies is reported once; which one is not reported.  `ignore_case` applies to every alternative.
        GpuCodec.Opt and GpuCodec.Rep items in a `list` / `tuple` pattern or in an alternative are positions that may be left
        out or repeated - 'colou?r', '[0-9]{1,3}', GpuCodec.regex() writes them - (hufgpu_find_any_quant): a start is reported
        once when any way of leaving optional positions out lies there.  They are a ValueError next to `bol`, `eol`,
        `whole_line` or `word`.
        `bol`, `eol` ('^', '$'), `whole_line` (grep -x: both) and `word` (grep -w) keep the occurrences whose neighbours allow
        it (hufgpu_find_any_anchored): the byte in front is absent or one of `delimiters`, the byte behind is, neither is one
        of `word_bytes` ([A-Za-z0-9_] when not given).  The reported position is still the pattern's own start.  `delimiters`
        matters with `bol`, `eol` or `whole_line` only; with none of the five set the call is the one it always was.  Raises
        ValueError for `word_bytes` without `word`, and with `eol`, `whole_line` or `word` for alternatives whose lengths plus
        one each exceed FIND_PATTERN_MAX.  An AllOf or a Seq is a TypeError: a conjunction has no position of its own."""
        if isinstance(pattern, GpuCodec._Terms) or (isinstance(pattern, GpuCodec.Expr) and len(pattern) > 1):
            raise TypeError(f"{type(pattern).__name__} selects records: find_records, count_records and grep take it, a search for "
                            "positions does not")
        if isinstance(pattern, GpuCodec.Expr):
            self._expr_alone(pattern, bol, eol, whole_line, word, word_bytes)
            x = self.expr_arrays(pattern, ignore_case, None)
            route, anchors = "expr", 0
            key = (x["classes"].tobytes(), x["alt_lens"].tobytes(), len(x["alt_lens"]), x["optional"].tobytes(),
                   self.byte_set(delimiters), x["word_set"], x["anchors"])
        else:
            route, key, st, (anchors, ws) = self._find_route(pattern, ignore_case, anchors=(bol, eol, whole_line, word, word_bytes))
        max_positions = int(max_positions)
        pos = self._find_buffer(out, max_positions, torch.int64)
        head, tail, totals, errs, counts = self._find_args(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize,
                                                           block_counts, relaxed)
        if anchors:
            key = key + (self.byte_set(delimiters), ws, anchors)
        call = self.lib.hufgpu_find_any_anchored if anchors else getattr(self.lib, self._FIND_CALLS[route][0])
        err = call(*head, *key, pos.data_ptr() if max_positions else None, max_positions, *tail)
        self._check(err, "Failed to enqueue the search")
        return pos, totals, errs, counts

    def count_pattern(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                      sub_index: torch.Tensor, raw_size: int, blocksize: int, pattern, relaxed: bool = False,
                      ignore_case: bool = False, bol: bool = False, eol: bool = False, whole_line: bool = False,
                      word: bool = False, word_bytes=None, delimiters=b"\n"):
        """How often `pattern` occurs in the original data: find_pattern without positions, enqueue-only.  Returns CUDA
        tensors (totals[4], block_errs[nblocks]) as find_pattern does.  `bol` to `delimiters`: as for find_pattern."""
        _, totals, errs, _ = self.find_pattern(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                               relaxed=relaxed, ignore_case=ignore_case, bol=bol, eol=eol, whole_line=whole_line,
                                               word=word, word_bytes=word_bytes, delimiters=delimiters)
        return totals, errs

    SPAN_MAX = _native.FIND_PATTERN_MAX     # no reported length is above it: the max_len of gather / scatter behind find_spans

    @staticmethod
    def _span_key(pattern, ignore_case, bol, eol, whole_line, word, word_bytes, delimiters):
        """(key, fixed): `pattern` - whatever find_pattern takes - as hufgpu_find_any_spans' part of the C argument list, classes
        to anchors, and the one length of all its forms (None when there are several).  Raises what find_pattern raises."""
        if isinstance(pattern, GpuCodec._Terms) or (isinstance(pattern, GpuCodec.Expr) and len(pattern) > 1):
            raise TypeError(f"{type(pattern).__name__} selects records: find_records, count_records and grep take it, a search for "
                            "positions does not")
        if isinstance(pattern, GpuCodec.Expr):
            GpuCodec._expr_alone(pattern, bol, eol, whole_line, word, word_bytes)
            x = GpuCodec.expr_arrays(pattern, ignore_case, None)
            classes, alt_lens, optional = x["classes"].tobytes(), x["alt_lens"], x["optional"]
            anchors, ws = x["anchors"], x["word_set"]
        else:
            route, key, _, (anchors, ws) = GpuCodec._find_route(pattern, ignore_case, anchors=(bol, eol, whole_line, word, word_bytes))
            optional = None
            if route == "literal":
                classes, alt_lens = GpuCodec.byte_classes(key[0]).tobytes(), np.array([key[1]], np.uint32)
            elif route == "classes":
                classes, alt_lens = key[0], np.array([key[1]], np.uint32)
            else:
                classes, alt_lens = key[0], np.frombuffer(key[1], np.uint32)
                optional = np.frombuffer(key[3], np.uint8) if route == "quant" else None
        lens = set(alt_lens.tolist())
        fixed = lens.pop() if len(lens) == 1 and (optional is None or not optional.any()) else None
        key = (classes, alt_lens.tobytes(), len(alt_lens), None if optional is None else optional.tobytes(),
               GpuCodec.byte_set(delimiters), ws, anchors)
        return key, fixed

    def find_spans(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                   sub_index: torch.Tensor, raw_size: int, blocksize: int, pattern, max_positions: int = 0,
                   block_counts: bool = False, relaxed: bool = False, out=None, want_open: bool = True,
                   ignore_case: bool = False, bol: bool = False, eol: bool = False, whole_line: bool = False,
                   word: bool = False, word_bytes=None, delimiters=b"\n"):
        """find_pattern with the LENGTH of what lies at every start (hufgpu_find_any_spans): the same patterns - a literal,
        classes, an AnyOf, Opt / Rep items, regex(), a one-term Expr / egrep() - and keywords, the same starts in the same order.
        Returns CUDA tensors (positions int64, lengths int32, totals, block_errs, block_counts, open): lengths[r], for
        r < totals[1], is the length of the LONGEST form of any alternative that lies at positions[r], qualifies under the
        anchors and has its tested span in served blocks - 1 to SPAN_MAX, a boundary byte not counted -, so gather() and
        scatter() take the tensor as it is with max_len = SPAN_MAX.  open[r] (uint8; None with `want_open=False`) is 1 when a
        longer form could not be ruled out because a byte it needs lies in a block that is not served; totals[3] counts those.
        `out`: (positions, lengths) or (positions, lengths, open), contiguous [max_positions] buffers; made when not given.
        Every start is reported, overlapping ones included: the leftmost-longest selection of grep -o is select_spans' - or
        find_matches, which runs both.
        Raises what find_pattern raises."""
        key, _ = self._span_key(pattern, ignore_case, bol, eol, whole_line, word, word_bytes, delimiters)
        max_positions = int(max_positions)
        given = tuple(out) if out is not None else ()
        if out is not None and len(given) not in (2, 3):
            raise ValueError("`out` is (positions, lengths) or (positions, lengths, open)")
        pos = self._find_buffer(given[0] if given else None, max_positions, torch.int64)
        lens = self._find_buffer(given[1] if given else None, max_positions, torch.int32)
        opn = self._find_buffer(given[2] if len(given) == 3 else None, max_positions, torch.uint8) if want_open else None
        head, tail, totals, errs, counts = self._find_args(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize,
                                                           block_counts, relaxed)
        err = self.lib.hufgpu_find_any_spans(*head, *key, pos.data_ptr() if max_positions else None,
                                             lens.data_ptr() if max_positions else None,
                                             opn.data_ptr() if want_open and max_positions else None, max_positions, *tail)
        self._check(err, "Failed to enqueue the search")
        return pos, lens, totals, errs, counts, opn

    def _spans_for(self, stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern, max_matches, relaxed, find,
                   nonoverlapping=False):
        """find_spans for the pipelines: (positions, lengths, totals) with the entries behind totals[1] made harmless on the
        device - a record at raw_size of length 0 reads and writes nothing.  With `nonoverlapping` select_spans stands behind
        the search and makes them harmless itself (its pad rows); the totals are still the search's."""
        pos, lens, totals = self.find_spans(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                            max_positions=max_matches, relaxed=relaxed, want_open=False, **find)[:3]
        if nonoverlapping:
            pos, lens, _, _ = self.select_spans(pos, lens, totals[1:2], pad_pos=raw_size)
            return pos, lens, totals
        written = torch.arange(max_matches, device=self.tdev) < totals[1]
        return torch.where(written, pos, raw_size), torch.where(written, lens, 0), totals

    SELECT_MAX = _native.SELECT_MAX         # spans a select_spans call takes at most

    def select_geometry(self):
        """(ranks a tile, tiles a composition group) of select_spans' kernels (hufgpu_select_geometry)"""
        out = (C.c_uint32 * 2)()
        self.lib.hufgpu_select_geometry(out)
        return int(out[0]), int(out[1])

    def select_spans(self, positions: torch.Tensor, lengths: torch.Tensor, count: torch.Tensor | None = None, *,
                     max_selected: int | None = None, pad_pos: int | None = None, want_ranks: bool = False, out=None):
        """grep -o's non-overlapping leftmost-longest matches, chosen on the device from what find_spans reports
        (hufgpu_select_spans), on torch's current stream and without a synchronisation.  `positions` (int64 / uint64) and
        `lengths` (int32) are find_spans' tensors: positions strictly ascending, lengths 1 to SPAN_MAX.  `count` says how many
        of their rows hold spans: a one-element CUDA int64 / uint64 tensor or a view such as find_spans' totals[1:2]; None:
        all of them.  Rank 0 is selected, and behind a selected span the first one that starts at or behind its end.
        `max_selected` (default: the number of rows) caps the rows written; with `pad_pos` - for gather() / scatter():
        raw_size - the rows behind the written ones become (pad_pos, 0), records that read and write nothing.
        `out`: (positions, lengths) or (positions, lengths, ranks), contiguous [max_selected] buffers; made when not given.
        Returns CUDA tensors (positions int64, lengths int32, ranks int64 or None, totals int64 [4]): ranks[r] (with
        `want_ranks`) is the input rank of row r, totals = [selected, written, status, lowest offending rank] -
        select_result(totals) waits and reads them.  Eager only: the results are allocated inside the call."""
        assert positions.is_cuda and positions.dtype in (torch.int64, torch.uint64) and positions.dim() == 1 and positions.is_contiguous()
        n_cap = positions.numel()
        assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.dim() == 1 and lengths.numel() == n_cap and lengths.is_contiguous()
        if count is not None:
            assert count.is_cuda and count.dtype in (torch.int64, torch.uint64) and count.numel() == 1
        sel_cap = n_cap if max_selected is None else int(max_selected)
        given = tuple(out) if out is not None else ()
        if out is not None and len(given) not in (2, 3):
            raise ValueError("`out` is (positions, lengths) or (positions, lengths, ranks)")
        pos = self._find_buffer(given[0] if given else None, sel_cap, torch.int64)
        lens = self._find_buffer(given[1] if given else None, sel_cap, torch.int32)
        ranks = self._find_buffer(given[2] if len(given) == 3 else None, sel_cap, torch.int64) if want_ranks else None
        totals = torch.empty(4, dtype=torch.int64, device=self.tdev)
        if n_cap == 0:                                  # the C call wants the two arrays even when it reads nothing of them
            positions, lengths = torch.empty(1, dtype=torch.int64, device=self.tdev), torch.empty(1, dtype=torch.int32, device=self.tdev)
        err = self.lib.hufgpu_select_spans(self._ctx, positions.data_ptr(), lengths.data_ptr(),
                                           count.data_ptr() if count is not None else None, n_cap,
                                           pos.data_ptr() if sel_cap else None, lens.data_ptr() if sel_cap else None,
                                           ranks.data_ptr() if want_ranks and sel_cap else None, sel_cap,
                                           0 if pad_pos is None else int(pad_pos), totals.data_ptr(),
                                           0 if pad_pos is None else _native.SELECT_PAD, self._stream())
        self._check(err, "Failed to enqueue the selection")
        return pos, lens, ranks, totals

    def select_result(self, totals: torch.Tensor):
        """The one wait behind select_spans / find_matches / count_matches: (selected, written) of their `totals`; raises
        HuffmanGpuError on a status that is not 0 and names the offending rank."""
        selected, written, status, rank = (int(v) for v in totals.cpu().tolist())
        if status:
            raise HuffmanGpuError(status, "The selection refused its input",
                                  f"rank {rank}: positions are not strictly ascending there, or its length is not 1 to {self.SPAN_MAX}")
        return selected, written

    def find_matches(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                     sub_index: torch.Tensor, raw_size: int, blocksize: int, pattern, max_positions: int = 0,
                     block_counts: bool = False, relaxed: bool = False, out=None, want_open: bool = True,
                     ignore_case: bool = False, bol: bool = False, eol: bool = False, whole_line: bool = False,
                     word: bool = False, word_bytes=None, delimiters=b"\n"):
        """What grep -o -E prints: find_spans followed by select_spans, with no host wait in between.  The arguments are
        find_spans' (`max_positions` caps the STARTS the search reports; `out` is the selection's).  Returns CUDA tensors
        (positions, lengths, sel_totals, find_totals, block_errs, ranks): the selected matches, select_spans' totals, the
        search's totals and block statuses, and for every selected row its rank among the search's starts (None with
        `want_open=False`).  This is grep's set when find_totals[0] == find_totals[1] and find_totals[2] == 0; otherwise it
        is the greedy selection over what the search reported."""
        spos, slens, ftotals, errs, _, _ = self.find_spans(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                                           max_positions=max_positions, block_counts=block_counts, relaxed=relaxed,
                                                           want_open=False, ignore_case=ignore_case, bol=bol, eol=eol,
                                                           whole_line=whole_line, word=word, word_bytes=word_bytes, delimiters=delimiters)
        pos, lens, ranks, totals = self.select_spans(spos, slens, ftotals[1:2], want_ranks=want_open, out=out)
        return pos, lens, totals, ftotals, errs, ranks

    def count_matches(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                      sub_index: torch.Tensor, raw_size: int, blocksize: int, pattern, max_positions: int = 0,
                      relaxed: bool = False, **find):
        """grep -o -E | wc -l: find_matches without position buffers for the selection (the search still needs
        `max_positions` rows: the lengths are its).  Returns CUDA tensors (sel_totals, find_totals, block_errs)."""
        spos, slens, ftotals, errs, _, _ = self.find_spans(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                                           max_positions=max_positions, relaxed=relaxed, want_open=False, **find)
        totals = self.select_spans(spos, slens, ftotals[1:2], max_selected=0)[3]
        return totals, ftotals, errs

    def extract(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, sub_index: torch.Tensor,
                raw_size: int, blocksize: int, pattern, max_matches: int, *, out: torch.Tensor | None = None,
                relaxed: bool = False, nonoverlapping: bool = False, **find):
        """What a search finds, byte for byte: find_spans followed by gather(), on torch's current stream with no host wait
        in between - grep -o without its selection of non-overlapping matches: EVERY start is a row.  With
        `nonoverlapping=True` select_spans stands between the two: grep -o, a row a match.  `max_matches` is the
        search's cap, `**find` are its keywords (`ignore_case`, `bol`, `word`, ...).  Returns CUDA tensors (slots uint8
        [max_matches, >= SPAN_MAX] - row r holds lengths[r] bytes -, positions, lengths, statuses, totals): statuses are
        gather()'s per row, totals the search's, and the rows behind totals[1] - behind the selected ones with
        `nonoverlapping` - are made harmless on the device (position raw_size, length 0)."""
        max_matches = int(max_matches)
        pos, lens, totals = self._spans_for(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                            max_matches, relaxed, find, nonoverlapping)
        slots, statuses, _ = self.gather(stream, stream_len, offsets, nblocks, pos, lens, sub_index=sub_index, raw_size=raw_size,
                                         blocksize=blocksize, max_len=self.SPAN_MAX, out=out, relaxed=relaxed)
        return slots, pos, lens, statuses, totals

    def find_records(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                     sub_index: torch.Tensor, raw_size: int, blocksize: int, pattern, delimiters=b"\n",
                     max_records: int = 0, max_len: int = 0, block_counts: bool = False, relaxed: bool = False, out=None,
                     ignore_case: bool = False, before: int = 0, after: int = 0, context: int | None = None,
                     bol: bool = False, eol: bool = False, whole_line: bool = False, word: bool = False, word_bytes=None,
                     invert: bool = False, line_numbers: bool = False):
        """The records of the original data - the pieces between the bytes of `delimiters` (an iterable of ints or a
        `bytes`; empty: the data is one record) - that hold `pattern` at least once, each record ONCE, on torch's current
        stream and without a synchronisation (hufgpu_find_records): one walk of the stream, no decoded byte written.
        Returns CUDA tensors (positions[max_records] int64 - the records' starts, ascending, the first totals[1] written -,
        lengths[max_records] int32 - their lengths without the delimiter, cut at max_len when that is not 0 (read
        lengths above 2^31 - 1 as unsigned) -, totals[4] = matching records, records written, blocks not served, written
        records longer than max_len; block_errs[nblocks]; block_counts[nblocks] int64 - by the block of the record's
        start - or None).  A record is reported only when every block from the delimiter in front of it to the one that
        ends it is served.  (positions, lengths, max_len) are what gather() takes.  `out`: a pair of contiguous buffers
        (int64 [max_records], int32 [max_records]); made when not given.  Raises ValueError for a pattern that is empty,
        too long or holds a delimiter.
        A `list` / `tuple` pattern is one of classes and `ignore_case` makes classes of a literal's letters, as for
        find_pattern (hufgpu_find_records_classes); a class that holds a delimiter is a ValueError that names its position:
        subtract the delimiters from a wide class.
        A GpuCodec.AnyOf pattern reports the records that hold at least one of its alternatives, each record once
        (hufgpu_find_records_any): grep -e A -e B.  No class of any alternative may hold a delimiter.
        A pattern with GpuCodec.Opt / GpuCodec.Rep items - as find_pattern takes it, as GpuCodec.regex() writes it - makes the
        call hufgpu_find_records_quant, whatever else is asked for: `invert`, `line_numbers` and the distances apply unchanged;
        `bol`, `eol`, `whole_line`, `word` next to it and such an item inside an AllOf / Seq are a ValueError.
        `invert` reports the NON-EMPTY records that hold NO match (grep -v, but for the empty lines): a record whose extent
        is known lies in exactly one of the two answers.  `line_numbers` appends one tensor to the returned tuple,
        numbers[max_records] int64: the delimiters in front of each written record, 0-based (grep -n prints it plus 1), -1
        when a block in front of the record's is not served.  Either makes the call hufgpu_find_records_select, a `bytes` or
        `list` pattern being its one alternative; with both False the call and what it returns are what they always were.
        `out` may then hold a third buffer, contiguous int64 [max_records], for the numbers.
        `before`, `after` (grep -B, -A) and `context` (grep -C: both) also report the non-empty records of known extent that
        lie at most that many records in front of or behind a record of the answer - the matching ones, or with `invert`
        the ones without a match - when every block between the two is served; distances count empty records, which are
        never reported.  Any of them non-zero makes the call hufgpu_find_records_context and appends one more tensor,
        behind the numbers: selected[max_records] uint8, 1 for a record of the answer itself and 0 for context (grep's ':'
        and '-'); a buffer for it may come last in `out`.  `context` next to `before` or `after`, a negative distance and one
        above 2^32 - 1 are a ValueError.  With all three at their defaults nothing changes.
        `bol`, `eol` (grep '^...', '...$'), `whole_line` (grep -x: both) and `word` (grep -w) select on the occurrences whose
        neighbours allow it: the byte in front is absent or a delimiter, the byte behind is, neither is one of `word_bytes`
        ([A-Za-z0-9_] when not given).  Every overlapping occurrence is tested, so `word` selects b"foofoo foo" for b"foo" as
        GNU grep does.  Any of them makes the call hufgpu_find_records_anchored; everything else - `invert`, `line_numbers`,
        the distances, what is returned - applies to that selection unchanged.  `word_bytes` without `word` is a ValueError,
        and so are, with `eol`, `whole_line` or `word`, alternatives whose lengths plus one each exceed FIND_PATTERN_MAX.
        A GpuCodec.AllOf pattern selects the records that hold EVERY one of its 1 to FIND_TERMS_MAX items (grep A | grep B), a
        GpuCodec.Seq pattern those that hold them one behind the other without overlap (grep 'A.*B'), still in one walk
        (hufgpu_find_records_terms); an item is a bytes-like literal, a list / tuple of classes or an AnyOf, and all items'
        alternatives together share the FIND_PATTERN_MAX positions.  `ignore_case`, `invert`, `line_numbers` and the distances
        apply to that selection unchanged; one item makes the call that the item alone makes.  ValueError: any of `bol`, `eol`,
        `whole_line`, `word` next to them, more than FIND_TERMS_MAX items, and a Seq item whose alternatives differ in
        length; TypeError: an AllOf or a Seq inside another one or inside an AnyOf.
        A GpuCodec.Expr pattern - GpuCodec.egrep() writes one - has anchors, terms and optional positions together
        (hufgpu_find_records_expr); it carries its anchors, so an anchor keyword next to it is a ValueError, and `ignore_case`,
        `invert`, `line_numbers` and the distances apply to its selection unchanged."""
        before, after = self._find_context(before, after, context)
        widens = bool(before or after)
        select = bool(invert) or bool(line_numbers) or widens
        terms = expr = None
        if isinstance(pattern, GpuCodec.Expr):
            self._expr_alone(pattern, bol, eol, whole_line, word, word_bytes)
            expr = self.expr_arrays(pattern, ignore_case, delimiters)
            route, st, anchors, ws = "expr", expr["delim_set"], 0, None
        elif isinstance(pattern, GpuCodec._Terms):
            terms = self._find_terms(pattern, ignore_case, delimiters, (bol, eol, whole_line, word, word_bytes))
            if terms[3] == 1:                                           # one item: the call that it makes today
                (pattern,), terms = pattern, None
        if terms is not None:
            key, st, term_alts, n_terms, mode = terms
            anchors, ws = 0, None
        elif expr is None:
            route, key, st, (anchors, ws) = self._find_route(pattern, ignore_case, delimiters, select,
                                                             (bol, eol, whole_line, word, word_bytes))
        max_records, max_len = int(max_records), int(max_len)
        out = tuple(out) if out is not None else (None, None)
        numbers = self._find_buffer(out[2] if len(out) > 2 else None, max_records, torch.int64) if line_numbers else None
        at = 3 if line_numbers else 2
        selected = self._find_buffer(out[at] if len(out) > at else None, max_records, torch.uint8) if widens else None
        pos = self._find_buffer(out[0], max_records, torch.int64)
        lens = self._find_buffer(out[1], max_records, torch.int32)
        head, tail, totals, errs, counts = self._find_args(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize,
                                                           block_counts, relaxed)
        ptrs = (pos.data_ptr() if max_records else None, lens.data_ptr() if max_records else None)
        if expr is not None:
            x = expr
            err = getattr(self.lib, self._FIND_CALLS[route][1])(
                *head, st, x["classes"].tobytes(), x["alt_lens"].tobytes(), len(x["alt_lens"]), x["optional"].tobytes(),
                x["term_alts"].tobytes(), len(x["term_alts"]), _native.TERMS_ORDERED if x["ordered"] else _native.TERMS_ALL,
                x["word_set"], x["anchors"], _native.SELECT_INVERT if invert else 0, before, after, *ptrs,
                numbers.data_ptr() if line_numbers and max_records else None,
                selected.data_ptr() if widens and max_records else None, max_records, max_len, *tail)
        elif terms is not None:
            err = self.lib.hufgpu_find_records_terms(*head, st, *key, term_alts, n_terms, mode, _native.SELECT_INVERT if invert else 0,
                                                     before, after, *ptrs, numbers.data_ptr() if line_numbers and max_records else None,
                                                     selected.data_ptr() if widens and max_records else None, max_records, max_len,
                                                     *tail)
        elif anchors:
            err = self.lib.hufgpu_find_records_anchored(*head, st, *key, ws, anchors, _native.SELECT_INVERT if invert else 0, before,
                                                        after, *ptrs, numbers.data_ptr() if line_numbers and max_records else None,
                                                        selected.data_ptr() if widens and max_records else None, max_records, max_len,
                                                        *tail)
        elif route == "quant":
            err = self.lib.hufgpu_find_records_quant(*head, st, *key, _native.SELECT_INVERT if invert else 0, before, after, *ptrs,
                                                     numbers.data_ptr() if line_numbers and max_records else None,
                                                     selected.data_ptr() if widens and max_records else None, max_records, max_len,
                                                     *tail)
        elif widens:
            err = self.lib.hufgpu_find_records_context(*head, st, *key, _native.SELECT_INVERT if invert else 0, before, after, *ptrs,
                                                       numbers.data_ptr() if line_numbers and max_records else None,
                                                       selected.data_ptr() if max_records else None, max_records, max_len, *tail)
        elif select:
            err = self.lib.hufgpu_find_records_select(*head, st, *key, _native.SELECT_INVERT if invert else 0, *ptrs,
                                                      numbers.data_ptr() if line_numbers and max_records else None,
                                                      max_records, max_len, *tail)
        else:
            err = getattr(self.lib, self._FIND_CALLS[route][1])(*head, st, *key, *ptrs, max_records, max_len, *tail)
        self._check(err, "Failed to enqueue the search")
        return (pos, lens, totals, errs, counts) + ((numbers,) if line_numbers else ()) + ((selected,) if widens else ())

    def count_records(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int,
                      sub_index: torch.Tensor, raw_size: int, blocksize: int, pattern, delimiters=b"\n",
                      relaxed: bool = False, ignore_case: bool = False, before: int = 0, after: int = 0,
                      context: int | None = None, bol: bool = False, eol: bool = False, whole_line: bool = False,
                      word: bool = False, word_bytes=None, invert: bool = False, line_numbers: bool = False):
        """How many records hold `pattern` (grep -c; with `invert` grep -v -c, but for the empty lines): find_records
        without positions, enqueue-only.  Returns CUDA tensors (totals[4], block_errs[nblocks]) as find_records does, and
        with `line_numbers` the empty tensor of numbers behind them.  `before`, `after`, `context`: the records that
        find_records reports with them are counted, and the empty tensor of flags comes last.  `bol`, `eol`, `whole_line`,
        `word`, `word_bytes`: as for find_records (grep -c -w, grep -c -x)."""
        res = self.find_records(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                delimiters, relaxed=relaxed, ignore_case=ignore_case, before=before, after=after, context=context,
                                bol=bol, eol=eol, whole_line=whole_line, word=word, word_bytes=word_bytes,
                                invert=invert, line_numbers=line_numbers)
        return (res[2], res[3]) + tuple(res[5:])

    def grep(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, sub_index: torch.Tensor,
             raw_size: int, blocksize: int, pattern, max_records: int, max_len: int, delimiters=b"\n",
             relaxed: bool = False, ignore_case: bool = False, before: int = 0, after: int = 0, context: int | None = None,
             bol: bool = False, eol: bool = False, whole_line: bool = False, word: bool = False, word_bytes=None,
             invert: bool = False, line_numbers: bool = False):
        """The first `max_len` bytes of the first `max_records` records that hold `pattern`: find_records followed by
        gather, on torch's current stream and without a synchronisation.  Returns CUDA tensors (lines uint8 [max_records,
        max_len], raw_lens int32 [max_records] - the bytes of row i that are the record's -, errs int32 [max_records] -
        gather's per record -, totals[4] and block_errs[nblocks] as find_records gives them).  Rows from totals[1] on are
        records of 0 bytes at raw_size.  `invert`: the non-empty records that do NOT hold it (grep -v); `line_numbers`: one
        more tensor at the end, numbers int64 [max_records] as find_records gives them, -1 from row totals[1] on.
        `before`, `after`, `context` (grep -B, -A, -C): the rows around those records as well, as find_records reports them,
        and one more tensor behind the numbers, selected uint8 [max_records]: 1 for a row of the answer itself, 0 for a row of
        context and from row totals[1] on.
        `bol`, `eol`, `whole_line`, `word`, `word_bytes` (grep '^...', '...$', -x, -w): as for find_records."""
        max_records, max_len = int(max_records), int(max_len)
        if max_len < 1:
            raise ValueError("grep needs max_len, the bytes of a row")
        found = self.find_records(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize,
                                  pattern, delimiters, max_records=max_records, max_len=max_len,
                                  relaxed=relaxed, ignore_case=ignore_case, before=before, after=after, context=context,
                                  bol=bol, eol=eol, whole_line=whole_line, word=word, word_bytes=word_bytes,
                                  invert=invert, line_numbers=line_numbers)
        pos, lens, totals, block_errs = found[:4]
        written = torch.arange(max_records, device=self.tdev) < totals[1]
        pos = torch.where(written, pos, raw_size)
        lens = torch.where(written, lens, 0)
        lines, errs, raw_lens = self.gather(stream, stream_len, offsets, nblocks, pos, lens, sub_index=sub_index, raw_size=raw_size,
                                            blocksize=blocksize, max_len=max_len, relaxed=relaxed)
        more = found[5:]
        if line_numbers:
            more = (torch.where(written, more[0], -1),) + more[1:]
        if len(more) > int(bool(line_numbers)):                         # the flags: 0 behind the written rows
            more = more[:-1] + (torch.where(written, more[-1], 0),)
        return (lines, raw_lens, errs, totals, block_errs) + more

    # -- overwrite: bytes [lo, hi) of the original data replaced in one indexed stream ---------------
    def update_ranges(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, ranges,
                      data: torch.Tensor, src_offsets=None, sub_index: torch.Tensor | None = None, raw_size: int = 0,
                      blocksize: int = 0, out: torch.Tensor | None = None, want_sub_index: bool = False,
                      relaxed: bool = False):
        """Overwrite the byte ranges `ranges` = [(lo, hi), ...] of the original data with the bytes of `data`, range i
        from data[src_offsets[i]:] (default: the ranges' bytes back to back), out of place (hufgpu_update_ranges).  Only
        the blocks a range touches are encoded again.  `sub_index` is the OLD stream's (optional); `want_sub_index`
        asks for the new stream's and needs (raw_size, blocksize).  Without `out` the output is sized from `blocksize`,
        which must then be the length of the stream's longest block.  Returns (new stream view, its length, new offsets,
        new sub-index or None, blocks re-encoded).  Raises HuffmanGpuError."""
        ranges = [(int(lo), int(hi)) for lo, hi in ranges]
        n = len(ranges)
        assert data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()
        if src_offsets is not None:
            src_offsets = [int(x) for x in src_offsets]
            assert len(src_offsets) == n
        if out is None:
            # include/huffman_gpu.h: the old length + every touched block at its encode_bound always fits.  The block
            # lengths are not known here, so both are bounded from above: a touched block holds a byte of a range (at
            # most `grow` of them, and nblocks), and the touched blocks hold the ranges' bytes plus, per range, what two
            # cut blocks of at most `blocksize` bytes hold besides.
            if not blocksize:
                raise ValueError("update_ranges sizes its output from `blocksize` (the longest block): pass it, or pass `out`")
            grow = sum(max(0, hi - lo) for lo, hi in ranges)
            touched = min(nblocks, grow)
            per_block = self.encode_bound(1, 0)                        # header, the longest tree, padding
            held = grow + 2 * n * blocksize
            out = torch.empty(stream_len + touched * per_block + (9 * held + 7) // 8 + 64, dtype=torch.uint8, device=self.tdev)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        new_offsets = torch.empty(nblocks + 1, dtype=torch.int64, device=self.tdev)
        new_sub = self.new_sub_index(raw_size, blocksize) if want_sub_index else None
        out_len, count = C.c_uint64(0), C.c_uint64(0)
        flags = _native.RELAXED_TREE if relaxed else _native.STRICT_TREE
        with_layout = sub_index is not None or want_sub_index
        err = self.lib.hufgpu_update_ranges(self._ctx, stream.data_ptr() if stream.numel() else None, stream_len,
                                            offsets.data_ptr(), nblocks, n, _u64_array(lo for lo, _ in ranges),
                                            _u64_array(hi for _, hi in ranges),
                                            _u64_array(src_offsets) if src_offsets is not None else None,
                                            data.data_ptr() if data.numel() else None,
                                            sub_index.data_ptr() if sub_index is not None else None,
                                            raw_size if with_layout else 0, blocksize if with_layout else 0,
                                            out.data_ptr(), out.numel(), new_offsets.data_ptr(),
                                            new_sub.data_ptr() if new_sub is not None else None, flags,
                                            C.byref(out_len), C.byref(count), self._stream())
        self._pending_decode = None
        self._check(err, "Failed to update the ranges")
        return out[: out_len.value], int(out_len.value), new_offsets, new_sub, int(count.value)

    def update_range(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, lo: int,
                     data: torch.Tensor, **kwargs):
        """update_ranges for the one range [lo, lo + data.numel())."""
        return self.update_ranges(stream, stream_len, offsets, nblocks, [(lo, lo + data.numel())], data, **kwargs)

    # -- scatter: records at device-resident positions overwritten, enqueue-only ---------------------
    def scatter_touched_bound(self, nblocks: int, blocksize: int, nrecords: int, max_len: int) -> int:
        """The blocks that `nrecords` records of up to `max_len` bytes can touch at most (hufgpu_scatter_touched_bound)."""
        return int(self.lib.hufgpu_scatter_touched_bound(nblocks, blocksize, nrecords, max_len))

    @staticmethod
    def _scatter_source(data, fill, n: int, max_len):
        """(data as [n, >= max_len] rows or None, fill byte or None, max_len, stride) of scatter's `data` / `fill`; raises
        ValueError / TypeError for what scatter documents."""
        if (data is None) == (fill is None):
            raise ValueError("scatter takes exactly one of `data` (the records' new bytes) and `fill` (one byte value for all)")
        if fill is not None:
            if isinstance(fill, (bytes, bytearray)):
                if len(fill) != 1:
                    raise ValueError(f"`fill` is one byte, not {len(fill)}")
                fill = fill[0]
            fill = int(fill)
            if not 0 <= fill <= 255:
                raise ValueError(f"`fill` is a byte value, not {fill}")
            return None, fill, max_len, 0
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8:
            raise TypeError("`data` is a uint8 tensor: [nrecords, >= max_len] slots, or 1-D with `max_len`")
        if data.dim() == 1:
            if max_len is None:
                raise ValueError("a 1-D `data` needs `max_len`, the bytes of a slot")
            if data.numel() != n * int(max_len):
                raise ValueError(f"a 1-D `data` holds nrecords x max_len = {n * int(max_len)} bytes, not {data.numel()}")
            data = data.contiguous().view(n, int(max_len))
        if data.dim() != 2 or data.size(0) != n:
            raise ValueError(f"`data` has one slot a record: [{n}, >= max_len], not {list(data.shape)}")
        if data.size(1) > 1 and data.stride(1) != 1:
            raise ValueError("a slot of `data` is contiguous")
        if max_len is not None and data.size(1) < int(max_len):
            raise ValueError(f"a slot of `data` has {data.size(1)} bytes, fewer than max_len = {int(max_len)}")
        stride = data.stride(0) if n > 1 else max(data.stride(0), data.size(1))
        return data, None, (data.size(1) if max_len is None else max_len), stride

    def scatter(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, positions: torch.Tensor,
                lengths, *, data: torch.Tensor | None = None, fill=None, raw_size: int, blocksize: int,
                sub_index: torch.Tensor | None = None, max_len: int | None = None, touched_cap: int | None = None,
                out: torch.Tensor | None = None, want_sub_index: bool = False, relaxed: bool = False):
        """Overwrite record i = bytes [positions[i], positions[i] + length_i) of the original data, out of place, on torch's
        current stream and without a synchronisation (hufgpu_scatter): the write side of gather().  `positions` is a CUDA
        int64 / uint64 tensor, `lengths` an int (every record that long), None (every record `max_len` long) or a CUDA
        int32 tensor with `max_len` their host-known bound - what find_pattern / find_records leave on the device.
        Exactly one of `data` and `fill`: `data` is a uint8 CUDA tensor of slots [nrecords, >= max_len] (its row stride is
        the call's src_stride: what gather() returns goes in as it is) or 1-D with `max_len`; `fill` is one byte value
        (an int or a `bytes` of one) that every covered byte becomes.  Records may overlap, repeat and come in any order;
        with `data`, a byte that several records cover gets the byte of one of them.  `touched_cap` bounds the distinct
        blocks the records touch and sizes the scratch area; it defaults to scatter_touched_bound().  `sub_index` is the
        OLD stream's (optional), `want_sub_index` asks for the new stream's.  Without `out` the output is stream_len +
        touched_cap x encode_bound(blocksize) bytes, which always suffices.
        Returns (out, new_offsets int64 [nblocks + 1], result int64 [4], new sub-index or None), all CUDA tensors; nothing
        has been waited for, so `out` is the whole buffer and result[1] the new length: scatter_result(result) reads it."""
        assert positions.is_cuda and positions.dtype in (torch.int64, torch.uint64) and positions.dim() == 1
        positions = positions.contiguous()
        n = positions.numel()
        len_ptr = None
        if isinstance(lengths, torch.Tensor):
            if max_len is None:
                raise ValueError("lengths on the device need max_len, their bound")
            assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.numel() == n
            lengths = lengths.contiguous()
            len_ptr = lengths.data_ptr() if n else None
        elif lengths is not None:
            if max_len is not None and int(max_len) != int(lengths):
                raise ValueError("a fixed record size is max_len")
            max_len = int(lengths)
        data, fill, max_len, stride = self._scatter_source(data, fill, n, max_len)
        if max_len is None:
            raise ValueError("scatter needs the records' length: `lengths`, or `max_len`")
        max_len = int(max_len)
        if touched_cap is None:
            touched_cap = max(1, self.scatter_touched_bound(nblocks, blocksize, n, max_len))
        touched_cap = int(touched_cap)
        if out is None:
            per_block = self.encode_bound(min(blocksize, raw_size) if blocksize else raw_size, 0)
            out = torch.empty(stream_len + min(touched_cap, nblocks) * per_block + 64, dtype=torch.uint8, device=self.tdev)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        new_offsets = torch.empty(nblocks + 1, dtype=torch.int64, device=self.tdev)
        new_sub = self.new_sub_index(raw_size, blocksize) if want_sub_index else None
        result = torch.empty(4, dtype=torch.int64, device=self.tdev)
        flags = (_native.RELAXED_TREE if relaxed else _native.STRICT_TREE) | (_native.SCATTER_FILL if fill is not None else 0)
        err = self.lib.hufgpu_scatter(self._ctx, stream.data_ptr() if stream.numel() else None, stream_len,
                                      offsets.data_ptr(), nblocks, sub_index.data_ptr() if sub_index is not None else None,
                                      raw_size, blocksize, n, positions.data_ptr() if n else result.data_ptr(),   # (no record: never read)
                                      len_ptr, max_len,
                                      None if data is None else (data.data_ptr() if data.numel() else result.data_ptr()), stride,
                                      fill or 0, touched_cap, out.data_ptr(), out.numel(), new_offsets.data_ptr(),
                                      new_sub.data_ptr() if new_sub is not None else None, result.data_ptr(), flags, self._stream())
        self._pending_decode = None
        self._check(err, "Failed to enqueue the scatter")
        return out, new_offsets, result, new_sub

    def scatter_result(self, result: torch.Tensor):
        """Reads the four result words of a scatter() once (this waits for the call): returns (new length, touched blocks),
        or raises HuffmanGpuError with the status; the exception's `.raw` is the record or block that caused it (None when
        the status names none) and `.touched` the number of touched blocks."""
        status, length, touched, who = (int(x) for x in result.cpu().tolist())
        if status:
            who = None if who == -1 else who
            detail = {_native.HUF_ERROR_INVALID_ARGUMENT: f"record {who} is longer than max_len",
                      _native.HUF_ERROR_MEMORY_ALLOCATION: f"{touched} blocks are touched, or the new stream does not fit the output"
                      }.get(status, f"block {who} cannot be served")
            e = HuffmanGpuError(status, "The scatter failed", detail)
            e.raw, e.touched = who, touched
            raise e
        return length, touched

    def redact(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, nblocks: int, sub_index: torch.Tensor,
               raw_size: int, blocksize: int, pattern, fill=b"*", *, max_matches: int, lines: bool = False, max_len: int = 0,
               touched_cap: int | None = None, out: torch.Tensor | None = None, want_sub_index: bool = False,
               relaxed: bool = False, spans: bool = False, nonoverlapping: bool = False, **find):
        """Blank what a search finds: find_pattern (or, with `lines=True`, find_records) followed by scatter(fill=...), on
        torch's current stream with no host wait in between.  Every byte of every occurrence of `pattern` becomes `fill`;
        with `lines=True` the first `max_len` bytes of every selected record do (the delimiter stays).  `max_matches` is
        the search's cap (occurrences or records behind it are not blanked: the returned totals say how many there
        were); `**find` are the search's keywords (`ignore_case`, `bol`, `word`, ... and with `lines` `delimiters`,
        `invert`, ...).
        A search for positions reports where a match STARTS; where it ends is known only for a pattern of one length - a
        literal, a list / tuple of classes, an AnyOf whose alternatives all have that length.  Opt / Rep items, an Expr
        and an AnyOf of unequal lengths raise ValueError without `lines=True` - or `spans=True`: then the search is
        find_spans, which takes every positions pattern, and the LONGEST form at every start is blanked (scatter with the
        lengths tensor, max_len = SPAN_MAX).  Every start counts, overlapping ones included: what is blanked is the union of
        the spans.  `spans=True` with `lines=True` is a ValueError.  With `nonoverlapping=True` (which needs `spans=True`)
        select_spans stands between the search and the scatter: grep -o's matches are blanked and no others, so with
        scatter's `data=` in the place of a fill the records could not overlap.
        The scatter is given the search's cap as its number of records, not the found count, which is on the device.  The
        entries behind the found count are made harmless on the device before it runs: positions from totals[1] on are
        replaced by raw_size (and lengths by 0) - a record that starts at raw_size writes nothing.
        What it costs in memory: the scatter cannot know how many blocks the matches touch, so with `touched_cap=None` it
        takes scatter_touched_bound(nblocks, blocksize, max_matches, length), which is EVERY block as soon as max_matches
        reaches nblocks / 2.  The context's scratch area then grows to touched_cap x blocksize - the whole raw size - and an
        `out` made here is stream_len + touched_cap x encode_bound(blocksize) bytes, however few matches there are.  A
        caller who knows that the matches are few passes `touched_cap=` (a status of HUF_ERROR_MEMORY_ALLOCATION in
        `result`, and nothing written outside the buffers, if more blocks are touched) and may pass `out=`.
        Returns (out, new_offsets, result, new sub-index or None, totals): scatter()'s, and the search's totals."""
        max_matches = int(max_matches)
        if spans and lines:
            raise ValueError("redact(spans=True) blanks what matched, redact(lines=True) the records that hold it: give one")
        if nonoverlapping and not spans:
            raise ValueError("redact(nonoverlapping=True) selects among spans: give spans=True")
        if spans:
            pos, lengths, totals = self._spans_for(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                                   max_matches, relaxed, find, nonoverlapping)
            mlen = self.SPAN_MAX
        elif lines:
            if int(max_len) < 1:
                raise ValueError("redact(lines=True) needs max_len, the bytes of a record that are blanked at most")
            found = self.find_records(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                      max_records=max_matches, max_len=int(max_len), relaxed=relaxed, **find)
            pos, lens, totals = found[0], found[1], found[2]
            written = torch.arange(max_matches, device=self.tdev) < totals[1]
            pos = torch.where(written, pos, raw_size)
            lens = torch.where(written, lens, 0).clamp_(max=int(max_len))
            lengths, mlen = lens, int(max_len)
        else:
            if isinstance(pattern, GpuCodec.Expr):
                raise ValueError("an Expr has no one match length (where a match ends is not reported): redact it with lines=True")
            if not isinstance(pattern, GpuCodec._Terms):
                if self._is_quant(pattern):
                    raise ValueError("a pattern with Opt / Rep items has no one match length (where a match ends is not reported): "
                                     "redact it with lines=True")
                route, key, _ = self._find_route(pattern, find.get("ignore_case", False))
                if route == "any":
                    alt_lens = np.frombuffer(key[1], np.uint32)
                    if len(set(alt_lens.tolist())) != 1:
                        raise ValueError(f"the alternatives have lengths {sorted(set(alt_lens.tolist()))}, not one (where a match ends "
                                         "is not reported): redact them with lines=True")
                    mlen = int(alt_lens[0])
                else:
                    mlen = int(key[1])
            pos, totals = self.find_pattern(stream, stream_len, offsets, nblocks, sub_index, raw_size, blocksize, pattern,
                                            max_positions=max_matches, relaxed=relaxed, **find)[:2]
            written = torch.arange(max_matches, device=self.tdev) < totals[1]
            pos = torch.where(written, pos, raw_size)
            lengths = mlen
        res = self.scatter(stream, stream_len, offsets, nblocks, pos, lengths, fill=fill, raw_size=raw_size, blocksize=blocksize,
                           sub_index=sub_index, max_len=mlen, touched_cap=touched_cap, out=out, want_sub_index=want_sub_index,
                           relaxed=relaxed)
        return res + (totals,)

    # -- append and truncate: an indexed stream made longer or shorter in place ----------------------
    def append(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, raw_size: int, blocksize: int,
               data: torch.Tensor, sub_index: torch.Tensor | None = None, new_sub_index: bool = False,
               relaxed: bool = False):
        """Append the bytes of `data` to the stream of `raw_size` bytes encoded in blocks of `blocksize`
        (hufgpu_append): afterwards stream and offsets are what encode() writes for the old data plus `data`.  Works in
        place on `stream` and `offsets` when they are large enough (the old length plus encode_bound of the tail block
        and the new bytes; one entry per block and one more); otherwise tensors of that size are allocated and the
        old content copied.  `sub_index` is the OLD stream's (optional); `new_sub_index` asks for the new stream's.
        Returns (stream, offsets, new length, new raw size[, new sub-index]).  Raises HuffmanGpuError, and then the
        stream and its index are unchanged."""
        assert data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()
        assert stream.dtype == torch.uint8 and stream.is_cuda and stream.is_contiguous()
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous()
        n = data.numel()
        new_raw = raw_size + n
        nb_old, nb_new = self.block_count(raw_size, blocksize), self.block_count(new_raw, blocksize)
        tail = raw_size % blocksize if blocksize else 0
        if n and stream.numel() < stream_len + self.encode_bound(tail + n, blocksize):
            grown = torch.empty(stream_len + self.encode_bound(tail + n, blocksize), dtype=torch.uint8, device=self.tdev)
            grown[:stream_len] = stream[:stream_len]
            stream = grown
        if offsets.numel() < nb_new + 1:
            grown = torch.empty(nb_new + 1, dtype=torch.int64, device=self.tdev)
            grown[: nb_old + 1] = offsets[: nb_old + 1]
            offsets = grown
        new_sub = self.new_sub_index(new_raw, blocksize) if new_sub_index else None
        out_len = C.c_uint64(0)
        flags = _native.RELAXED_TREE if relaxed else _native.STRICT_TREE
        err = self.lib.hufgpu_append(self._ctx, stream.data_ptr() if stream.numel() else None, stream_len, stream.numel(),
                                     offsets.data_ptr(), raw_size, blocksize, data.data_ptr() if n else None, n,
                                     sub_index.data_ptr() if sub_index is not None else None,
                                     new_sub.data_ptr() if new_sub is not None else None, flags, C.byref(out_len),
                                     self._stream())
        self._pending_decode = None
        self._check(err, "Failed to append to the stream")
        res = (stream, offsets, int(out_len.value), new_raw)
        return res + (new_sub,) if new_sub_index else res

    def truncate(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, raw_size: int, blocksize: int,
                 new_raw_size: int, sub_index: torch.Tensor | None = None, new_sub_index: bool = False,
                 relaxed: bool = False):
        """Cut the stream of `raw_size` bytes encoded in blocks of `blocksize` to its first `new_raw_size` bytes, in
        place (hufgpu_truncate): afterwards stream and offsets are what encode() writes for them.  Returns what
        append() returns."""
        assert stream.dtype == torch.uint8 and stream.is_cuda and stream.is_contiguous()
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous()
        new_sub = self.new_sub_index(new_raw_size, blocksize) if new_sub_index else None
        out_len = C.c_uint64(0)
        flags = _native.RELAXED_TREE if relaxed else _native.STRICT_TREE
        err = self.lib.hufgpu_truncate(self._ctx, stream.data_ptr() if stream.numel() else None, stream_len,
                                       offsets.data_ptr(), raw_size, blocksize, new_raw_size,
                                       sub_index.data_ptr() if sub_index is not None else None,
                                       new_sub.data_ptr() if new_sub is not None else None, flags, C.byref(out_len),
                                       self._stream())
        self._pending_decode = None
        self._check(err, "Failed to truncate the stream")
        res = (stream, offsets, int(out_len.value), new_raw_size)
        return res + (new_sub,) if new_sub_index else res

    # -- the sub-index of a stream that came without one -------------------------------------------
    def build_sub_index(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, raw_size: int, blocksize: int,
                        raw: torch.Tensor | None = None, sub_index: torch.Tensor | None = None, relaxed: bool = False):
        """The sub-index hufgpu_encode_sub would have written for `stream` (raw_size bytes encoded in blocks of
        `blocksize`), rebuilt from the stream and its block index: from the decoded data when the caller holds it
        (`raw`: hufgpu_sub_index_from_raw), else by decoding slabs of blocks into scratch memory
        (hufgpu_build_sub_index).  Returns (sub_index, unbuilt): the tensor for decode(..., sub_index=) and
        decode_ranges(..., sub_index=), and the blocks whose rows could not be built (they decode the slow way)."""
        if sub_index is None:
            sub_index = self.new_sub_index(raw_size, blocksize)
        assert sub_index.numel() * sub_index.element_size() >= self.sub_index_bytes(raw_size, blocksize)
        unbuilt = C.c_uint64(0)
        flags = _native.RELAXED_TREE if relaxed else _native.STRICT_TREE
        sp = stream.data_ptr() if stream.numel() else None
        if raw is not None:
            assert raw.dtype == torch.uint8 and raw.is_cuda and raw.is_contiguous() and raw.numel() >= raw_size
            err = self.lib.hufgpu_sub_index_from_raw(self._ctx, sp, stream_len, offsets.data_ptr(), raw.data_ptr(), raw_size,
                                                     blocksize, sub_index.data_ptr(), flags, C.byref(unbuilt), self._stream())
        else:
            err = self.lib.hufgpu_build_sub_index(self._ctx, sp, stream_len, offsets.data_ptr(), raw_size, blocksize,
                                                  sub_index.data_ptr(), flags, C.byref(unbuilt), self._stream())
            self._pending_decode = None
        self._check(err, "Failed to build the sub-index")
        return sub_index, int(unbuilt.value)

    def decode_build_sub(self, stream: torch.Tensor, stream_len: int, offsets: torch.Tensor, out: torch.Tensor, raw_size: int,
                         blocksize: int, sub_index: torch.Tensor | None = None, relaxed: bool = False):
        """decode() - same result, same HuffmanGpuError with the delivered bytes in `.raw` - that also builds the
        stream's sub-index from the output it writes (hufgpu_decode_build_sub).  Returns (raw_len, sub_index, unbuilt)."""
        if sub_index is None:
            sub_index = self.new_sub_index(raw_size, blocksize)
        assert sub_index.numel() * sub_index.element_size() >= self.sub_index_bytes(raw_size, blocksize)
        raw, unbuilt = C.c_uint64(0), C.c_uint64(0)
        flags = _native.RELAXED_TREE if relaxed else _native.STRICT_TREE
        err = self.lib.hufgpu_decode_build_sub(self._ctx, stream.data_ptr() if stream.numel() else None, stream_len,
                                               offsets.data_ptr(), raw_size, blocksize, out.data_ptr(), out.numel(),
                                               sub_index.data_ptr(), flags, C.byref(raw), C.byref(unbuilt), self._stream())
        self._pending_decode = None
        self._check(err, "Failed to decode the data", raw=int(raw.value))
        return int(raw.value), sub_index, int(unbuilt.value)

    CALIB_VARIANTS = 8

    def calib_bandwidth(self, kind: str, variant: int, a: torch.Tensor | None, b: torch.Tensor | None, nbytes: int):
        """One launch of the bandwidth calibration kernel (kind: "copy" a -> b, "read" a, "fill" b)."""
        k = {"copy": 0, "read": 1, "fill": 2}[kind]
        self._check(self.lib.hufgpu_calib_bandwidth(self._ctx, k, variant, a.data_ptr() if a is not None else None,
                                                    b.data_ptr() if b is not None else None, nbytes, self._stream()),
                    "calibration launch failed")

    def decode_counters(self):
        """(blocks the exact decoder took, blocks the one-pass index-only decoder handed on) of the last decode."""
        c = (C.c_uint32 * 2)()
        self._check(self.lib.hufgpu_decode_counters(self._ctx, c), "counter readout failed")
        return int(c[0]), int(c[1])

    def decode_stream(self, stream: torch.Tensor, avail: int, length: int, out: torch.Tensor,
                      relaxed: bool = False, sequential: bool = False):
        """Raw-stream decode (no index). Returns (err, bytes written, bytes consumed).
        sequential=True forces the in-order decoder (same results, for cross-checking)."""
        raw, used = C.c_uint64(0), C.c_uint64(0)
        flags = (_native.RELAXED_TREE if relaxed else _native.STRICT_TREE) | (2 if sequential else 0)
        err = self.lib.hufgpu_decode_stream(self._ctx, stream.data_ptr() if stream.numel() else None,
                                            avail, length, out.data_ptr(), out.numel(), flags,
                                            C.byref(raw), C.byref(used), self._stream())
        return int(err), int(raw.value), int(used.value)

    def stream_counters(self):
        """What the block discovery of the last decode_stream / hufgpu_block_index did (hufgpu_stream_counters): (ran,
        candidates found, candidates held, sent to the exact probe, links that are not "the next candidate", blocks
        validated, output bytes the probes left in place or 2**64 - 1, passes)."""
        c = (C.c_uint64 * 8)()
        self._check(self.lib.hufgpu_stream_counters(self._ctx, c), "counter readout failed")
        return tuple(int(x) for x in c)

    def fill(self, out: torch.Tensor, kind: str, first: int = 0, seed: int | None = None):
        seed = FILL_SEEDS[kind] if seed is None else seed
        self._check(self.lib.hufgpu_fill(self._ctx, out.data_ptr(), out.numel(), FILL_KINDS[kind],
                                         seed, first, self._stream()), "fill failed")
        return out

    def set_profiling(self, on: bool, resume: bool = False):
        """on: record HIP events around every kernel; resume=True keeps what was recorded so far."""
        self.lib.hufgpu_set_profiling(self._ctx, (2 if resume else 1) if on else 0)

    ENCODE_KERNELS = ("hist256", "tree", "scan_sizes", "pack")
    DECODE_KERNELS = ("prepare_scan", "decode")

    def profile(self, kind: str):
        """Per-kernel milliseconds summed over the profiled calls -> (dict name->ms, calls)."""
        ms = (C.c_float * 8)()
        n, calls = C.c_int(0), C.c_int(0)
        k = 0 if kind == "encode" else 1
        self._check(self.lib.hufgpu_get_profile(self._ctx, k, ms, 8, C.byref(n), C.byref(calls)),
                    "profile readout failed")
        names = self.ENCODE_KERNELS if k == 0 else self.DECODE_KERNELS
        return {names[i]: float(ms[i]) for i in range(min(n.value, len(names)))}, calls.value
