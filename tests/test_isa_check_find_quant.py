"""The kernels that hufgpu_find_any_quant and hufgpu_find_records_quant added (kernels/find.hpp) in the shipped build: present
once each, free of the gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py), and within the resources
their launch counts on.  CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check_find.py
does for the older ones.
"""
import pytest

from libhuffman_amd import build

LDS_A_CU = 160 * 1024
WALKS = {"find_opt_sub_kernel": "find_alt_sub_kernel", "find_rec_opt_sub_kernel": "find_rec_alt_sub_kernel"}
SEAM = "find_opt_seam_kernel"


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + "E" in n]


def test_the_kernels_are_present_once_each(shipped_table):
    for k in tuple(WALKS) + tuple(WALKS.values()) + (SEAM, "find_alt_seam_kernel"):
        assert len(rows_of(shipped_table, k)) == 1, k


def test_the_walks_leave_three_workgroups_a_cu(shipped_table):
    """the closure costs temporaries, not state: the any-of walk's LDS and scratch - the registers saved around the out-of-line
    step-by-step tile decode that all walk kernels share - and not a byte more, three workgroups of eight waves a CU by LDS
    and by registers (512 a lane in all), and the any-of walk's waves a SIMD"""
    for k, older in WALKS.items():
        (r,), (o,) = rows_of(shipped_table, k), rows_of(shipped_table, older)
        assert r["scratch"] == o["scratch"] and r["lds"] == o["lds"] and 3 * r["lds"] <= LDS_A_CU, (k, r)
        assert 3 * r["allocated"] <= 512 and 512 // r["allocated"] == 512 // o["allocated"], (k, r, o)


def test_the_seam_kernel_runs_eight_waves_a_simd(shipped_table):
    """a wave a tile, a lane a start: at most 64 VGPRs, no scratch, the table and a window of 128 bytes a wave in LDS"""
    (r,), (o,) = rows_of(shipped_table, SEAM), rows_of(shipped_table, "find_alt_seam_kernel")
    assert r["vgprs"] <= 64 and r["scratch"] == 0 and r["lds"] == 2048 + 4 * 128 and r["lds"] <= o["lds"] + 256, r
