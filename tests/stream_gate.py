"""What tests/test_gpu_streams.py needs to put a call on a side stream behind a gate, or into a captured graph, without a
wrong library doing harm: inputs that are built on the CPU alone (the oracle's stream and index, the sub-index of
tests/sub_index_ref.py), static device buffers that hold a decoy until the gated copies replace it, the gate and the
capture themselves.  Not a test module.

The gate: on a side stream, a bounded spin (torch.cuda._sleep), an event `opened`, device-to-device copies of the real input
over the decoy, the call.  A launch that does not go to the side stream runs at once - the gate holds back nothing on any other
stream - and reads the decoy: a complete, valid input of the same geometry whose stream is not longer than the real one, so
the host-passed stream_len covers every index entry it can read.  Its answer differs from the real one, which is what the
comparison sees.  A call that must only enqueue is seen not to have waited: `opened` has not happened when it returns; a case
whose gate was open by then has proved nothing and fails.
"""
import contextlib
import ctypes
import gc
import re
import time

import numpy as np

import sub_index_ref as R

GUARD = 0xA5
GUARD64 = int(np.array([GUARD] * 8, np.uint8).view(np.int64)[0])
MIN_GATE_MS = 20.0                      # the gate is the larger of this and GATE_FACTOR times the warm-up's host time
GATE_FACTOR = 20.0
HIP_STREAM_NON_BLOCKING = 1


# ---- inputs built without the library under test ---------------------------------------------------------------------------
class Input:
    """data in blocks of `bs` with the oracle's stream and block index and the CPU reference's sub-index"""

    def __init__(self, oracle, data, bs):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.bs, self.n = bs, int(self.data.size)
        stream, offs = oracle.encode(self.data, bs, with_offsets=True)
        self.stream, self.offs = np.asarray(stream, np.uint8), np.asarray(offs).astype(np.int64)
        self.length = int(self.stream.size)
        self.exp = R.expected(self.stream, np.asarray(offs), self.data, bs)
        self.nb = self.exp.lay.nb
        self.sub = sub_index_bytes(self.exp)


def sub_index_bytes(exp):
    """the bytes of the sub-index buffer for an Expected: the written set, zeros elsewhere, a whole number of words"""
    buf = np.zeros(-(-exp.lay.size // 8) * 8, np.uint8)
    tiles, groups, lens = R.views(buf, exp.lay)
    tiles[:], groups[:], lens[:] = exp.tiles, exp.groups, exp.lens
    return buf


def rolled(data, bs, k):
    """every block rotated by k bytes: the same histograms, so the same trees, sizes and index, another payload"""
    out = data.copy()
    for b in range(0, data.size, bs):
        out[b:b + bs] = np.roll(data[b:b + bs], k)
    return out


def shuffled(data, bs, seed):
    """the bytes shuffled inside each block: the encoders' decoy"""
    rng = np.random.default_rng(seed)
    out = data.copy()
    for b in range(0, data.size, bs):
        out[b:b + bs] = rng.permutation(data[b:b + bs])
    return out


class Slots:
    """The static device buffers a call reads - stream, index, sub-index, raw data - and every input uploaded next to them,
    padded to the buffers' sizes.  load(name) copies one input in, device to device, on torch's current stream.  What the
    host passes - n, blocksize, block count, stream_len - is the real inputs'; the decoy's stream is checked not to be
    longer.  The attributes are those find_support's caller reads of an encoded input."""

    def __init__(self, torch, inputs, decoy, reals, extra_stream=0, extra_blocks=0, same_length=True):
        """same_length=False: for a call that reads the raw data alone (an encoder); the streams may then differ in length"""
        self.torch = torch
        first = inputs[reals[0]]
        self.n = self.raw_size = first.n
        self.bs = self.row_bs = first.bs
        self.nb = first.nb
        self.length = first.length
        names = [decoy] + list(reals)
        for name in names:
            assert (inputs[name].n, inputs[name].bs) == (self.n, self.bs), name
        if same_length:
            for name in reals:
                assert inputs[name].length == self.length, (name, "the real inputs' streams differ in length")
            assert inputs[decoy].length <= self.length, ("the decoy's stream is longer than the real one", inputs[decoy].length, self.length)
        cap = max(inputs[name].length for name in names) + extra_stream
        words = first.sub.size // 8
        self.stream = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        self.offsets = torch.zeros(self.nb + 1 + extra_blocks, dtype=torch.int64, device="cuda")
        self.sub = torch.zeros(max(1, words), dtype=torch.int64, device="cuda")
        self.data = torch.zeros(self.n, dtype=torch.uint8, device="cuda")
        self.src = {}
        for name in names:
            i = inputs[name]
            st = np.zeros(cap, np.uint8)
            st[:i.length] = i.stream
            offs = np.full(self.nb + 1 + extra_blocks, i.offs[-1], np.int64)
            offs[:self.nb + 1] = i.offs
            sub = np.zeros(max(1, words) * 8, np.uint8)
            sub[:i.sub.size] = i.sub
            self.src[name] = tuple(torch.from_numpy(a).cuda() for a in (st, offs, sub.view(np.int64), i.data))
        torch.cuda.synchronize()

    def load(self, name):
        for dst, src in zip((self.stream, self.offsets, self.sub, self.data), self.src[name]):
            dst.copy_(src)


# ---- the HIP runtime the process has loaded ----------------------------------------------------------------------------------
def loaded_hip():
    """the libamdhip64 that is mapped into this process (torch's), opened again by its path: the same handle.  Two
    runtimes in one process would each own their streams: exactly one must be mapped."""
    import os
    with open("/proc/self/maps") as f:
        paths = sorted({os.path.realpath(m.group(1)) for m in re.finditer(r"(/\S*libamdhip64\.so[^\s]*)", f.read())})
    assert len(paths) == 1, ("one HIP runtime is expected in the process", paths)
    return ctypes.CDLL(paths[0])


def stream_flags(stream):
    flags = ctypes.c_uint(0xFFFFFFFF)
    err = loaded_hip().hipStreamGetFlags(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags))
    assert err == 0, f"hipStreamGetFlags: {err}"
    return flags.value


# ---- the gate and the capture --------------------------------------------------------------------------------------------
class Gate:
    def __init__(self, torch):
        self.torch = torch
        self.cycles_per_ms = self.measure()
        self.log = []                   # (case, the warm-up's host time, the gate, the host time behind the gate; ms)

    def measure(self):
        """cycles of torch.cuda._sleep a millisecond, by two events; the spin is made longer until it takes 2 ms"""
        torch = self.torch
        cycles, ms = 1_000_000, 0.0
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 2.0:
                break
            cycles *= 10
        assert ms >= 2.0, ("torch.cuda._sleep does not hold a stream", cycles, ms)
        return cycles / ms

    def warm_up(self, slots, decoy, enqueue):
        """the call on the decoy on the null stream, twice: the first makes the workspaces (and loads the kernels), the host
        time of the second sizes the gate.  Returns the gate's length in ms."""
        torch = self.torch
        slots.load(decoy)
        enqueue()
        slots.load(decoy)               # (a call that works in place has changed it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enqueue()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return host_ms, max(MIN_GATE_MS, GATE_FACTOR * host_ms)

    def prime(self, s, slots, decoy, enqueue):
        """The call once more on the decoy, now on s itself, and a wait: the state it leaves is the warm-up's.  The first
        launch on a stream of a kernel that needs scratch memory (decode_fast_kernel, decode_fix_kernel) was seen to take
        1.5 ms of host time instead of 0.1, and once longer than the gate - presumably the runtime sizing the queue's scratch
        behind what the queue still holds.  That is the stream's first use, not the call, so it happens in front of the gate."""
        torch = self.torch
        with torch.cuda.stream(s):
            slots.load(decoy)
            enqueue()
            slots.load(decoy)
            s.synchronize()
        torch.cuda.synchronize()

    @contextlib.contextmanager
    def quiet(self):
        """no garbage collection between the closing of a gate and the look at it: a full collection in a process that holds
        torch takes tens of milliseconds of host time, more than the gate, and says nothing about the call"""
        collecting = gc.isenabled()
        gc.disable()
        try:
            yield
        finally:
            if collecting:
                gc.enable()

    def close(self, s, ms):
        """the gate on stream s; returns the event behind it"""
        torch = self.torch
        opened = torch.cuda.Event()
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
            opened.record(s)
        return opened

    def run(self, label, s, slots, decoy, real, enqueue, check, enqueue_only):
        """warm-up on the decoy; then on s: the gate, the copies of the real input, the call; the answer is fetched and
        compared on s.  enqueue_only: the call has returned with the gate still closed, or the case fails."""
        torch = self.torch
        host_ms, gate_ms = self.warm_up(slots, decoy, enqueue)
        self.prime(s, slots, decoy, enqueue)
        with self.quiet(), torch.cuda.stream(s):
            opened = self.close(s, gate_ms)
            t0 = time.perf_counter()
            slots.load(real)
            outs = enqueue()
            closed = not opened.query()
            behind_ms = (time.perf_counter() - t0) * 1e3
        self.log.append((label, host_ms, gate_ms, behind_ms))
        print(f"[gate] {label}: warm-up enqueue {host_ms:.3f} ms, gate {gate_ms:.1f} ms, copies and call behind it {behind_ms:.3f} ms")
        with torch.cuda.stream(s):
            s.synchronize()
            if enqueue_only:
                assert closed, (label, "the gate had opened before the call returned: this run has proved nothing", gate_ms)
            check(outs, real)

    def capture(self, label, s, slots, decoy, reals, enqueue, check):
        """warm-up on the decoy; the call captured on s in global mode - any wait ends the capture with an error; a launch
        on the null stream does not (s is non-blocking), it runs at once on the decoy and is missing from the graph -; then
        one replay per real input, the static buffers overwritten before each: the outputs, guard-filled inside the graph,
        show whatever the graph does not carry.

        A capture that fails must fail the case and nothing else.  torch.cuda.graph() is not used for it: when the end of a
        capture raises, it leaves s the current stream for the rest of the process.  And nothing may be finalised while s
        captures - the destructor of a torch CUDAGraph waits for the device, which a capturing process may not do, and an
        exception in a destructor ends the process: a failed case's graph lives on in a cycle with its traceback, so the
        garbage is collected in front of the capture, the collector rests during it, and a graph that failed is dropped
        here, after the capture."""
        torch = self.torch
        self.warm_up(slots, decoy, enqueue)
        graph, outs, error = torch.cuda.CUDAGraph(), None, None
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(s):
                graph.capture_begin(capture_error_mode="global")
                try:
                    outs = enqueue()
                except Exception as e:
                    error = e
                try:
                    graph.capture_end()
                except Exception as e:
                    error = error or e
        finally:
            if collecting:
                gc.enable()
        if error is not None:
            message = f"{label}: the call could not be captured: {type(error).__name__}: {error}"
            outs = error = None
            del graph
            torch.cuda.synchronize()
            raise AssertionError(message)
        for real in reals:
            with torch.cuda.stream(s):
                slots.load(real)
                graph.replay()
                s.synchronize()
                check(outs, real)
        return graph
