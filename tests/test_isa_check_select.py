"""The kernels that hufgpu_select_spans added (kernels/select.hpp) in the shipped build: present once each, without scratch,
free of the gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py, DESIGN.md 3.3: build.check_isa raises on a hit) - and
every kernel of profiles/find/kernel_resources_spans.txt exactly as that table has it: the search family launches what it
launched.  CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check_find_spans.py does;
nothing but the register counts is read.
"""
import pytest

from libhuffman_amd import build
from test_isa_check_find_spans import committed, rows_of

NEW = ("select_tile_kernel", "select_compose_kernel", "select_mark_kernel", "select_emit_kernel", "select_finish_kernel")


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def test_the_new_kernels_are_present_once_each_without_scratch(shipped_table):
    for k in NEW:
        (r,) = rows_of(shipped_table, k)
        assert r["scratch"] == 0, (k, r)


def test_the_tile_kernels_leave_room_on_a_compute_unit(shipped_table):
    """a tile's positions, pointers and marks: eight workgroups of four waves fit a compute unit's LDS and registers; the
    composition holds a group's 64 maps in registers and still runs four waves a SIMD"""
    for k in ("select_tile_kernel", "select_mark_kernel"):
        (r,) = rows_of(shipped_table, k)
        assert 8 * r["lds"] <= 160 * 1024 and r["allocated"] <= 64, (k, r)
    (r,) = rows_of(shipped_table, "select_compose_kernel")
    assert r["lds"] == 0 and r["allocated"] <= 128, r


def test_the_find_kernels_are_what_they_were(shipped_table):
    before, now = committed("kernel_resources_spans.txt"), committed("kernel_resources_select.txt")
    assert len(before) >= 30 and set(before) <= set(now)
    assert set(now) - set(before) == {n for n in now if any(k + "E" in n for k in NEW)} and len(set(now) - set(before)) == len(NEW)
    for name, row in before.items():
        assert now[name] == row, name
        r = shipped_table[name]
        assert (r["vgprs"], r["scratch"], r["lds"]) == row, (name, r, row)
