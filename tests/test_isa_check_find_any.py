"""The kernels of hufgpu_find_any / hufgpu_find_records_any (kernels/find.hpp) in the shipped build: present once each next to
the older find kernels, free of the gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py), and the two
walks at an LDS size that leaves three workgroups a CU.  CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here,
as tests/test_isa_check.py does.
"""
import pytest

from libhuffman_amd import build

LDS_A_CU = 160 * 1024
WALKS = ("find_alt_sub_kernel", "find_rec_alt_sub_kernel")
NEW = WALKS + ("find_alt_seam_kernel",)
OLDER = ("find_sub_kernel", "find_pat_sub_kernel", "find_rec_sub_kernel", "find_seam_kernel", "find_cls_sub_kernel",
         "find_rec_cls_sub_kernel", "find_cls_seam_kernel")


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + "E" in n]       # (the mangled name: the kernel's, then its argument's)


def test_the_any_of_kernels_are_present(shipped_table):
    for k in NEW + OLDER:
        assert len(rows_of(shipped_table, k)) == 1, k


def test_the_any_of_kernels_have_no_hazard(shipped_table):
    """check_isa has returned: no kernel of the build has a hit.  (The state of several alternatives is the class kernels'
    two 32-bit halves, shifted by constants; the seam kernel's bit masks are the wave's, in scalar registers.)"""
    assert all(rows_of(shipped_table, k) for k in NEW)


def test_the_walks_leave_three_workgroups_a_cu(shipped_table):
    """the class walks' 2 KiB table and nothing more: still three workgroups of 512 in 160 KiB of LDS"""
    for k in WALKS:
        (r,) = rows_of(shipped_table, k)
        assert 3 * r["lds"] <= LDS_A_CU, (k, r)
        assert r["lds"] >= 2048, (k, r)
