"""Every host <-> device route of huf_encode() / huf_decode() between two memory streams gives the same bytes.

The routes are chosen by switches that are read once per process, so each configuration is one child process
(tests/transfer_routes_child.py): the same input is encoded and decoded back, and the child prints a digest of the
stream and of the decoded bytes.

The input is 33 MiB + 7 bytes in blocks of 64 KiB, its stream 38 MiB.  From csrc/drop_in:
  - the duplex routes want at least DX_MIN_BYTES (32 MiB) and more than 1.5 rounds; dx_round_bytes() gives rounds of
    16 MiB for both calls (a quarter of the call, but not below 16 MiB; blocks of 64 KiB do not enlarge it), so the
    encode runs three rounds of 16, 16 and 1 MiB + 7 and the decode three rounds of its 38 MiB of stream;
  - with HUF_GPU_DUPLEX=0 both calls go through lane_copy() in both directions: every transfer (33 MiB of input or
    output, 38 MiB of stream) is above LANE_MIN (32 MiB), in pieces of LANE_SLOT (8 MiB) - five of them, so with the
    default six lanes one lane has nothing to move, and the last piece is short;
  - with HUF_GPU_COPY_LANES=0 as well, the same transfers are single plain copies: the baseline.
HUF_GPU_DX_TRACE=1 makes a duplex route that took the call say so on stderr, one line per call.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("HUF_GPU_DUPLEX", "HUF_GPU_COPY_LANES", "HUF_GPU_REGISTER", "HUF_GPU_DUPLEX_LANES", "HUF_GPU_DX_TRACE",
            "HUF_GPU_ROUND_MB", "HUF_GPU_BATCH_MB", "HUF_GPU_ZERO_COPY", "HUF_GPU_DEVICES", "HUF_GPU_PREFAULT_THREADS")
CONFIGS = [                                   # (name, environment, the duplex routes must report themselves)
    ("default", {"HUF_GPU_DX_TRACE": "1"}, True),
    ("duplex_off", {"HUF_GPU_DUPLEX": "0"}, False),
    ("plain_copies", {"HUF_GPU_DUPLEX": "0", "HUF_GPU_COPY_LANES": "0"}, False),
    ("staged_duplex", {"HUF_GPU_REGISTER": "0", "HUF_GPU_DX_TRACE": "1"}, True),
    ("one_duplex_lane", {"HUF_GPU_DUPLEX_LANES": "1"}, False),
]
CHILD_SECONDS = 120


@pytest.fixture(scope="module")
def runs():
    """name -> (return code, fields of the child's line, stderr), one child after the other; a child that is killed
    by a signal or runs into its time limit is the last one started"""
    out = {}
    for name, extra, _ in CONFIGS:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(extra)
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "transfer_routes_child.py"), ROOT],
                               env=env, capture_output=True, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired as e:
            out[name] = (None, {}, "time limit of %d s: %s" % (CHILD_SECONDS, e.stderr))
            break
        lines = r.stdout.strip().splitlines()
        fields = dict(f.split("=", 1) for f in lines[-1].split()) if lines and "=" in lines[-1] else {}
        out[name] = (r.returncode, fields, r.stderr)
        print("\n  %-16s rc=%s %s" % (name, r.returncode, lines[-1] if lines else ""))
        if r.returncode < 0:
            break
    return out


@pytest.fixture(scope="module")
def input_digest():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import transfer_routes_child as child
    return child.digest(child.flat_zipf(child.N_BYTES)), child.N_BYTES


def test_every_configuration_ran_and_succeeded(runs):
    for name, _, _ in CONFIGS:
        assert name in runs, f"{name} was not started: {sorted(runs)} ran, the last one died"
        rc, fields, err = runs[name]
        assert rc == 0 and fields.get("encode") == "0" and fields.get("decode") == "0", (name, rc, fields, err[-2000:])


def test_all_routes_write_the_same_stream(runs):
    digests = {name: runs[name][1].get("stream") for name, _, _ in CONFIGS if name in runs}
    assert len(digests) == len(CONFIGS) and None not in digests.values(), digests
    assert len(set(digests.values())) == 1, digests
    assert len({runs[name][1]["stream_len"] for name in digests}) == 1
    assert int(runs["default"][1]["stream_len"]) >= 32 << 20          # (or huf_decode would not take the routes under test)


def test_all_routes_decode_back_to_the_input(runs, input_digest):
    want, n = input_digest
    for name, _, _ in CONFIGS:
        assert name in runs, name
        fields = runs[name][1]
        assert fields.get("decoded") == want and fields.get("decoded_len") == str(n), (name, fields)


def test_the_duplex_routes_took_their_calls(runs):
    for name, _, traced in CONFIGS:
        if not traced:
            continue
        assert name in runs, name
        err = runs[name][2]
        assert err.count("encode_duplex:") == 1 and err.count("decode_duplex:") == 1, (name, err[-2000:])
        assert "ok=1" in [ln for ln in err.splitlines() if ln.startswith("decode_duplex:")][0], err[-2000:]
