"""The kernels of hufgpu_find_records_context (kernels/find.hpp) in the shipped build: present once each next to the older
record kernels, free of the gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py), and - as
find_rec_mark_kernel and find_rec_emit_kernel - at eight waves a SIMD without scratch or LDS.
CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check_find_select.py does.
"""
import pytest

from libhuffman_amd import build

NEW = ("find_ctx_dscan_kernel", "find_rec_ctx_kernel", "find_ctx_emit_kernel", "find_ctx_emit_no_kernel")
OLDER = ("find_rec_dscan_kernel", "find_rec_mark_kernel", "find_rec_invert_kernel", "find_rec_first_bad_kernel", "find_rec_emit_kernel",
         "find_rec_emit_no_kernel", "find_scan_kernel", "find_finish_kernel", "find_emit_kernel", "find_rec_alt_sub_kernel",
         "find_alt_seam_kernel")


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + "E" in n]       # (the mangled name: the kernel's, then its argument's)


def test_the_context_kernels_are_present(shipped_table):
    """... and no new name ends in an older one's: every kernel, old and new, is found exactly once by its name"""
    for k in NEW + OLDER:
        assert len(rows_of(shipped_table, k)) == 1, k


def test_the_context_kernels_have_no_hazard(shipped_table):
    """check_isa has returned: no kernel of the build has a hit.  (The new kernels shift 32-bit words only; the 64-bit values
    they divide are the wave's, in scalar registers.)"""
    assert all(rows_of(shipped_table, k) for k in NEW)


def test_the_context_kernels_run_at_eight_waves_a_simd(shipped_table):
    """at most 64 VGPRs, no scratch and no LDS: a wave a tile and a lane a word - the scan kernel a wave a group of tiles -,
    everything in registers"""
    for k in NEW:
        (r,) = rows_of(shipped_table, k)
        assert r["vgprs"] <= 64 and r["scratch"] == 0 and r["lds"] == 0, (k, r)
