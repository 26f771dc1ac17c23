"""The kernels that hufgpu_find_any_expr and hufgpu_find_records_expr added (kernels/find.hpp) in the shipped build: present
once each, free of the gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py), and within the resources
of the same kernels without the closure.  CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as
tests/test_isa_check_find_quant.py does for the quant calls' kernels; nothing but the register counts is read.
"""
import pytest

from libhuffman_amd import build

LDS_A_CU = 160 * 1024
# the terms' walk with the closure, a kernel a number of terms -> the same walk without it
WALKS = {"find_rec_term_opt_sub_kernelILj%dE" % nt: "find_rec_term_sub_kernelILj%dE" % nt for nt in (2, 3, 4)}
SEAMS = ("find_opt_anc_seam_kernel", "find_term_opt_seam_kernel")


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + "E" in n]


def test_the_kernels_are_present_once_each(shipped_table):
    for k in tuple(WALKS) + tuple(WALKS.values()):
        assert len(rows_of(shipped_table, k[:-1])) == 1, k
    for k in SEAMS + ("find_opt_seam_kernel",):
        assert len(rows_of(shipped_table, k)) == 1, k


def test_the_walks_keep_the_waves_and_the_scratch_of_the_walks_without_the_closure(shipped_table):
    """the closure costs temporaries, not state: no fewer waves a SIMD (512 registers a lane in all), no more scratch and no
    more LDS than the terms' walk of as many terms"""
    for k, older in WALKS.items():
        (r,), (o,) = rows_of(shipped_table, k[:-1]), rows_of(shipped_table, older[:-1])
        assert r["scratch"] <= o["scratch"] and r["lds"] <= o["lds"] and 3 * r["lds"] <= LDS_A_CU, (k, r, o)
        assert 512 // r["allocated"] >= 512 // o["allocated"], (k, r, o)


def test_the_seam_kernels_run_eight_waves_a_simd(shipped_table):
    """the quant calls' seam kernel with a seed: at most 64 VGPRs, no scratch, the table and a window of 128 bytes a wave"""
    (o,) = rows_of(shipped_table, "find_opt_seam_kernel")
    for k in SEAMS:
        (r,) = rows_of(shipped_table, k)
        assert r["vgprs"] <= 64 and r["scratch"] == 0 and r["lds"] == o["lds"] == 2048 + 4 * 128, (k, r)
