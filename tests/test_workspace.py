"""csrc/host/workspace.hpp on its own (no HIP, no GPU): tests/workspace_main.cpp is a stand-alone program that includes
that one header and drives it over malloc-backed hooks - the capacities each growth rule gives for the requests
1, 17, 18, 400, 3 and, for a group of two capacities, (2,1), (2,40), (100,1), (1,1); no allocation and no wait for a
request that fits; every allocation of every group failing in turn (the group is left empty, the others untouched, the
next growth works); zero fills there when grow returns; the wait before the first free; release_all, twice.  Built with
AddressSanitizer + UndefinedBehaviorSanitizer; a build that cannot be made because the compiler has no runtime for the
sanitizer - tried first with an empty program - is skipped, everything else has to exit 0 with "ok" as its last line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "workspace_main.cpp")


def compiler():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if cand and os.path.exists(cand):
            return cand
    return None


def run(cmd, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)


def test_workspace_under_sanitizers(tmp_path):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe = run([cxx] + flags + [str(empty), "-o", str(tmp_path / "empty")])
    if probe.returncode != 0 or run([str(tmp_path / "empty")], env=env).returncode != 0:
        pytest.skip(f"{cxx} has no usable runtime for -fsanitize=address,undefined here: {probe.stderr[-300:]}")
    exe = str(tmp_path / "workspace")
    built = run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-Wno-unused-function", SOURCE, "-o", exe])
    assert built.returncode == 0, built.stderr[-4000:]
    r = run([exe], env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().splitlines()[-1:] == ["ok"], out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-4000:]
