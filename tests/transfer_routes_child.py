"""Child process of test_gpu_transfer_routes.py: ONE huf_encode() and ONE huf_decode() between huf_memopen()
streams, with the transfer switches (HUF_GPU_DUPLEX, HUF_GPU_COPY_LANES, HUF_GPU_REGISTER, HUF_GPU_DUPLEX_LANES)
of this process's environment - they are read once per process, so every configuration is a process of its
own.  Prints a digest of the stream and of the decoded bytes; HUF_GPU_DX_TRACE=1 adds the duplex routes' own
lines on stderr."""
import ctypes as C
import hashlib
import sys

import numpy as np

N_BYTES = (33 << 20) + 7
BLOCKSIZE = 65536


def flat_zipf(n: int, seed: int = 11) -> np.ndarray:
    """Zipf-like bytes with exponent 1/4 over the values 0..254 (weight of rank r: 2^32 / r^(1/4); 255 never occurs: a
    block with all 256 values has a 1025-entry tree, which huf_decode refuses like the reference does), drawn like
    datagen.zipf255 from the counter-based splitmix64 stream: 4 MiB + 1 of them, repeated (an odd period, so that no
    two pieces or rounds of a transfer hold the same bytes).  About 7.9 bits a byte: with a 255-leaf tree in front
    of every block of 64 KiB the stream is LONGER than the input, which the test needs - huf_decode takes
    the duplex route, and the copy lanes, from 32 MiB of STREAM on."""
    from libhuffman_amd import datagen
    period = min(n, (4 << 20) + 1)
    r = np.arange(1, 256, dtype=np.float64)
    cum = np.cumsum(np.floor(float(1 << 32) / r ** 0.25).astype(np.uint64), dtype=np.uint64)
    u = datagen.splitmix64(seed, period) % cum[-1]
    return np.resize(np.searchsorted(cum, u, side="right").astype(np.uint8), n)


def digest(a) -> str:
    return hashlib.sha256(a).hexdigest()


def main() -> int:
    from libhuffman_amd import _native as N
    L = N.load()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    data = flat_zipf(N_BYTES)
    n = data.size
    rin, rout, rback = C.POINTER(N.ReadWriter)(), C.POINTER(N.ReadWriter)(), C.POINTER(N.ReadWriter)()
    bin_, bout, bback = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.huf_memopen(C.byref(rin), C.byref(bin_), n) == 0
    assert L.huf_memopen(C.byref(rout), C.byref(bout), n) == 0
    assert L.huf_memopen(C.byref(rback), C.byref(bback), n) == 0
    assert rin.contents.write(rin.contents.stream, data.ctypes.data_as(C.c_void_p), n) == 0
    cfg = N.Config(n, BLOCKSIZE, 0, 0, rin, rout)
    e1 = L.huf_encode(C.byref(cfg))
    m = C.c_size_t()
    L.huf_memlen(rout, C.byref(m))
    stream_len = m.value
    stream = np.frombuffer(C.string_at(bout.value, stream_len), np.uint8)
    dcfg = N.Config(stream_len, 0, 0, 0, rout, rback)
    e2 = L.huf_decode(C.byref(dcfg))
    L.huf_memlen(rback, C.byref(m))
    back = np.frombuffer(C.string_at(bback.value, m.value), np.uint8)
    for r in (rin, rout, rback):
        L.huf_memclose(C.byref(r))
    for b in (bin_, bout, bback):
        libc.free(b)
    print(f"encode={e1} decode={e2} stream_len={stream_len} stream={digest(stream)} decoded_len={back.size} decoded={digest(back)}")
    return 0 if e1 == 0 and e2 == 0 else 1


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    sys.exit(main())
