"""The kernels that hufgpu_scatter added (kernels/scatter.hpp) in the shipped build: present once each, free of the gfx950
last-VGPR shift hazard (libhuffman_amd/isa_check.py), and within the resources their launches count on.
CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check_find_quant.py does.
"""
import pytest

from libhuffman_amd import build

PLAIN = ("scat_zero_kernel", "scat_mark_kernel", "scat_class_kernel", "scat_overlay_kernel", "scat_fail_kernel", "scat_tree_wave_kernel",
         "scat_result_kernel", "scat_copy_result_kernel")
# the guarded row kernels and the kernels of hufgpu_update_ranges whose bodies they share: (twin, older, instantiations)
ROWS = (("scat_hist_lanes_kernel", "hist_lanes_pairs_kernel", 1), ("scat_hist_tree_kernel", "hist_tree_pairs_kernel", 2),
        ("scat_pack_rows_kernel", "pack_pairs_kernel", 2))


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel, template=False):
    """by the mangled name, with its length in front: tree_wave_kernel is not scat_tree_wave_kernel"""
    return [r for n, r in sorted(table.items()) if f"{len(kernel)}{kernel}" + ("I" if template else "E") in n]


def test_the_kernels_are_present_once_each(shipped_table):
    for k in PLAIN:
        assert len(rows_of(shipped_table, k)) == 1, k
    for twin, older, count in ROWS:
        assert len(rows_of(shipped_table, twin, True)) == count == len(rows_of(shipped_table, older, True)), twin


def test_overlay_and_class_kernels_use_no_scratch(shipped_table):
    """the overlay is a store kernel: no spill, no LDS, and registers for eight waves a SIMD; the small kernels likewise"""
    for k in ("scat_overlay_kernel", "scat_class_kernel", "scat_mark_kernel", "scat_fail_kernel", "scat_result_kernel"):
        (r,) = rows_of(shipped_table, k)
        assert r["scratch"] == 0 and r["lds"] == 0 and r["allocated"] <= 64, (k, r)


def test_the_guard_costs_the_row_kernels_nothing(shipped_table):
    """a row at or above the device's row count returns at once; the rows that work run the older kernels' bodies at the
    older kernels' occupancy: the same LDS, the same scratch, as many waves a SIMD by registers"""
    for twin, older, _ in ROWS:
        for r, o in zip(rows_of(shipped_table, twin, True), rows_of(shipped_table, older, True)):
            assert r["scratch"] == o["scratch"] and r["lds"] == o["lds"], (twin, r, o)
            assert 512 // r["allocated"] == 512 // o["allocated"], (twin, r, o)
    (r,), (o,) = rows_of(shipped_table, "scat_tree_wave_kernel"), rows_of(shipped_table, "tree_wave_kernel")
    assert r["scratch"] == o["scratch"] and r["lds"] == o["lds"] and 512 // r["allocated"] == 512 // o["allocated"], (r, o)
