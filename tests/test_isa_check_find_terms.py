"""The kernels that hufgpu_find_records_terms added (kernels/find.hpp) in the shipped build: present once each, free of the
gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py), and within the resources their launch counts on.
CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check_find.py does for the older ones.
"""
import pytest

from libhuffman_amd import build

LDS_A_CU = 160 * 1024
MASKS = ("find_term_seam_kernel", "find_rec_all_kernel", "find_rec_seq_kernel")
WALKS = ("find_rec_term_sub_kernelILj2E", "find_rec_term_sub_kernelILj3E", "find_rec_term_sub_kernelILj4E")


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + ("" if kernel.endswith("E") else "E") in n]


def test_the_kernels_are_present_once_each(shipped_table):
    for k in MASKS + WALKS + ("find_rec_alt_sub_kernel", "find_alt_seam_kernel", "find_rec_mark_kernel", "find_rec_invert_kernel"):
        assert len(rows_of(shipped_table, k)) == 1, k
    assert sum("find_rec_term_sub_kernel" in n for n in shipped_table) == 3      # a kernel for two, three and four terms


def test_the_kernels_over_the_masks_run_eight_waves_a_simd(shipped_table):
    """a wave a tile, a lane a word or a start: at most 64 VGPRs and no scratch; the seam kernel with find_alt_seam_kernel's LDS"""
    for k in MASKS:
        (r,) = rows_of(shipped_table, k)
        assert r["vgprs"] <= 64 and r["scratch"] == 0, (k, r)
    assert rows_of(shipped_table, "find_term_seam_kernel")[0]["lds"] == rows_of(shipped_table, "find_alt_seam_kernel")[0]["lds"]
    assert rows_of(shipped_table, "find_rec_all_kernel")[0]["lds"] == rows_of(shipped_table, "find_rec_seq_kernel")[0]["lds"] == 0


def test_the_walk_spills_nothing(shipped_table):
    """the masks of all terms stay in registers: the walk has the scratch of the any-of records' walk - the registers saved
    around the out-of-line step-by-step tile decode that all walk kernels share - and not a byte more, its LDS, and at least
    three waves a SIMD (512 registers a lane in all): a workgroup of eight waves fits a CU"""
    (older,) = rows_of(shipped_table, "find_rec_alt_sub_kernel")
    for k in WALKS:
        (r,) = rows_of(shipped_table, k)
        assert r["scratch"] == older["scratch"] and r["lds"] == older["lds"] and 3 * r["lds"] <= LDS_A_CU, (k, r)
        assert 3 * r["allocated"] <= 512, (k, r)
