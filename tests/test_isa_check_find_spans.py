"""The kernels that hufgpu_find_any_spans added (kernels/find.hpp) in the shipped build: present once each, free of the gfx950
last-VGPR shift hazard (libhuffman_amd/isa_check.py), within the walk's resources - and every OLDER kernel of
the search family exactly as profiles/find/kernel_resources_expr.txt has it: the seventeen older calls launch what they
launched.  CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check_find_expr.py does; nothing
but the register counts is read.
"""
import os
import re

import pytest

from libhuffman_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("find_span_kernel", "find_emit_len_kernel")
WALK = "find_opt_sub_kernel"


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + "E" in n]


def committed(name):
    """{mangled name: (VGPRs, scratch, LDS)} of a table that tools/kernel_resources.sh wrote"""
    text = open(os.path.join(ROOT, "profiles", "find", name)).read()
    out = {}
    for block in text.split("Function Name: ")[1:]:
        field = lambda key: int(re.search(key + r"[^:]*: (\d+)", block).group(1))      # noqa: E731
        out[block.split()[0]] = (field("VGPRs"), field("ScratchSize"), field("LDS Size"))
    return out


def test_the_new_kernels_are_present_once_each_without_new_scratch(shipped_table):
    (walk,) = rows_of(shipped_table, WALK)
    for k in NEW:
        (r,) = rows_of(shipped_table, k)
        assert r["scratch"] <= walk["scratch"], (k, r)


def test_the_span_kernel_keeps_the_walks_waves_and_lds(shipped_table):
    """the forward table in the place of the walk's, the decode tables and the tile slices: no more LDS than the walk, so three
    workgroups a CU, and at least the walk's waves a SIMD (512 registers a lane in all)"""
    (r,), (walk,) = rows_of(shipped_table, NEW[0]), rows_of(shipped_table, WALK)
    assert r["lds"] <= walk["lds"] and 3 * r["lds"] <= 160 * 1024, (r, walk)
    assert 512 // r["allocated"] >= 512 // walk["allocated"], (r, walk)


def test_the_older_find_kernels_are_what_they_were(shipped_table):
    before, now = committed("kernel_resources_expr.txt"), committed("kernel_resources_spans.txt")
    assert len(before) >= 30 and set(now) - set(before) == {n for n in now if any(k + "E" in n for k in NEW)} and set(before) <= set(now)
    for name, row in before.items():
        assert now[name] == row, name
        r = shipped_table[name]
        assert (r["vgprs"], r["scratch"], r["lds"]) == row, (name, r, row)
