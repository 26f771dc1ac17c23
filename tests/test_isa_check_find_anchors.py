"""The kernels of hufgpu_find_any_anchored and hufgpu_find_records_anchored (kernels/find.hpp) in the shipped build: present
once each next to the older find kernels, free of the gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py, DESIGN.md
3.3), at most 64 VGPRs and without scratch.
CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check_find_context.py does.
"""
import pytest

from libhuffman_amd import build

NEW = ("find_anchor_kernel", "find_anc_seam_kernel")
OLDER = ("find_rec_dscan_kernel", "find_rec_mark_kernel", "find_rec_invert_kernel", "find_rec_first_bad_kernel", "find_rec_emit_kernel",
         "find_rec_emit_no_kernel", "find_scan_kernel", "find_finish_kernel", "find_emit_kernel", "find_sub_kernel", "find_alt_sub_kernel",
         "find_rec_alt_sub_kernel", "find_alt_seam_kernel", "find_ctx_dscan_kernel", "find_rec_ctx_kernel", "find_ctx_emit_kernel",
         "find_ctx_emit_no_kernel")


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + "E" in n]       # (the mangled name: the kernel's, then its argument's)


def test_the_anchor_kernels_are_present(shipped_table):
    """... and no new name ends in an older one's: every kernel, old and new, is found exactly once by its name"""
    for k in NEW + OLDER:
        assert len(rows_of(shipped_table, k)) == 1, k


def test_the_anchor_kernels_have_no_hazard(shipped_table):
    """check_isa has returned: no kernel of the build has a hit.  (find_anchor_kernel shifts 32-bit words by constants; the
    64-bit values it divides are the wave's, in scalar registers; its one DPP move is made by every lane.)"""
    assert all(rows_of(shipped_table, k) for k in NEW)


def test_the_anchor_kernels_run_at_eight_waves_a_simd(shipped_table):
    """at most 64 VGPRs and no scratch: a wave a tile; find_anchor_kernel a lane a word and no LDS, find_anc_seam_kernel a
    lane a start with find_alt_seam_kernel's table in LDS.  These two are all the kernels the anchored calls add: the third
    mask of a records call with HUFGPU_ANCHOR_WORD comes from find_sub_kernel, the bytes call's walk"""
    for k in NEW:
        (r,) = rows_of(shipped_table, k)
        assert r["vgprs"] <= 64 and r["scratch"] == 0, (k, r)
    assert rows_of(shipped_table, "find_anchor_kernel")[0]["lds"] == 0
    assert rows_of(shipped_table, "find_anc_seam_kernel")[0]["lds"] == rows_of(shipped_table, "find_alt_seam_kernel")[0]["lds"]
    assert not any("find_rec_anc_sub" in n or "find_anc_sub" in n for n in shipped_table)       # no walk kernel of their own
