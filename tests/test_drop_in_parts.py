"""csrc/drop_in/parts.hpp on its own (no HIP, no GPU): tests/drop_in_parts_main.cpp is a stand-alone program that
includes that one header and checks split_parts (contiguous parts that cover [0, n) once, whole 2 MiB but for the last,
never more parts than threads), run_parts (every part runs exactly once, on helper threads) and env_int (the answers of
the hand-written environment readers it replaced).  Built once with AddressSanitizer + UndefinedBehaviorSanitizer and
once with ThreadSanitizer; a build that cannot be made because the compiler has no runtime for the sanitizer - tried
first with an empty program - is skipped, everything else has to exit 0 with "ok" as its last line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "drop_in_parts_main.cpp")


def compiler():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if cand and os.path.exists(cand):
            return cand
    return None


def run(cmd, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_parts_under_sanitizers(sanitizer, tmp_path):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-pthread"]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe = run([cxx] + flags + [str(empty), "-o", str(tmp_path / "empty")])
    if probe.returncode != 0 or run([str(tmp_path / "empty")], env=env).returncode != 0:
        pytest.skip(f"{cxx} has no usable runtime for -fsanitize={sanitizer} here: {probe.stderr[-300:]}")
    exe = str(tmp_path / "drop_in_parts")
    built = run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-Wno-unused-function", SOURCE, "-o", exe])
    assert built.returncode == 0, built.stderr[-4000:]
    r = run([exe], env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().splitlines()[-1:] == ["ok"], out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-4000:]
