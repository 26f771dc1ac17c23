"""The kernels that each feature of the search family added (kernels/find.hpp) in the shipped build: present once each next to
the older find kernels, free of the gfx950 last-VGPR shift hazard (libhuffman_amd/isa_check.py), and within
the resources their launch counts on.  One table, a row a feature; one cross-compile for all of them.
CPU-only: hipcc cross-compiles the kernels to gfx950 assembly here, as tests/test_isa_check.py does.
"""
import pytest

from libhuffman_amd import build

LDS_A_CU = 160 * 1024


def three_workgroups_a_cu(rows, kernels):
    """the class table's 2 KiB (in the place of 64 pattern bytes) and nothing more: still three workgroups of 512 in 160 KiB of LDS"""
    for k in kernels:
        (r,) = rows(k)
        assert 3 * r["lds"] <= LDS_A_CU, (k, r)
        assert r["lds"] >= 2048, (k, r)


def eight_waves_a_simd(lds):
    """at most 64 VGPRs and no scratch - and no LDS where `lds` says so: a wave a tile, a lane a word, everything in registers"""
    def bound(rows, kernels):
        for k in kernels:
            (r,) = rows(k)
            assert r["vgprs"] <= 64 and r["scratch"] == 0 and (lds or r["lds"] == 0), (k, r)
    return bound


def anchor_bound(rows, kernels):
    """find_anchor_kernel a lane a word and no LDS, find_anc_seam_kernel a lane a start with find_alt_seam_kernel's table in
    LDS.  These two are all the kernels the anchored calls add: the third mask of a records call with HUFGPU_ANCHOR_WORD comes
    from find_sub_kernel, the bytes call's walk"""
    eight_waves_a_simd(lds=True)(rows, kernels)
    assert rows("find_anchor_kernel")[0]["lds"] == 0
    assert rows("find_anc_seam_kernel")[0]["lds"] == rows("find_alt_seam_kernel")[0]["lds"]
    assert not any("find_rec_anc_sub" in n or "find_anc_sub" in n for n in rows.table)       # no walk kernel of their own


LITERAL = ("find_sub_kernel", "find_pat_sub_kernel", "find_rec_sub_kernel", "find_seam_kernel")
RECORDS = ("find_rec_dscan_kernel", "find_rec_mark_kernel", "find_rec_emit_kernel", "find_scan_kernel", "find_finish_kernel", "find_emit_kernel",
           "find_rec_alt_sub_kernel", "find_alt_seam_kernel")
SELECT = ("find_rec_invert_kernel", "find_rec_first_bad_kernel", "find_rec_emit_no_kernel")
CONTEXT = ("find_ctx_dscan_kernel", "find_rec_ctx_kernel", "find_ctx_emit_kernel", "find_ctx_emit_no_kernel")
# feature -> (the kernels it added, the older ones next to which each is found once, the kernels its bound is about, the bound)
FEATURES = {
    "classes": (("find_cls_sub_kernel", "find_rec_cls_sub_kernel", "find_cls_seam_kernel"), LITERAL,
                ("find_cls_sub_kernel", "find_rec_cls_sub_kernel"), three_workgroups_a_cu),
    "any": (("find_alt_sub_kernel", "find_rec_alt_sub_kernel", "find_alt_seam_kernel"),
            LITERAL + ("find_cls_sub_kernel", "find_rec_cls_sub_kernel", "find_cls_seam_kernel"),
            ("find_alt_sub_kernel", "find_rec_alt_sub_kernel"), three_workgroups_a_cu),
    "select": (SELECT, RECORDS, SELECT + ("find_rec_mark_kernel", "find_rec_emit_kernel"), eight_waves_a_simd(lds=False)),
    "context": (CONTEXT, RECORDS + SELECT, CONTEXT, eight_waves_a_simd(lds=False)),
    "anchors": (("find_anchor_kernel", "find_anc_seam_kernel"),
                RECORDS + SELECT + CONTEXT + ("find_sub_kernel", "find_alt_sub_kernel"), ("find_anchor_kernel", "find_anc_seam_kernel"),
                anchor_bound),
}
EVERY_FEATURE = pytest.mark.parametrize("feature", list(FEATURES))


@pytest.fixture(scope="module")
def shipped_table():
    """the library as __graft_entry__.build() compiles it: check_isa raises when any kernel has a hazard hit"""
    return build.check_isa(extra_flags=[])


def rows_of(table, kernel):
    return [r for n, r in table.items() if kernel + "E" in n]       # (the mangled name: the kernel's, then its argument's)


@EVERY_FEATURE
def test_the_kernels_are_present(shipped_table, feature):
    """... and no new name ends in an older one's: every kernel, old and new, is found exactly once by its name"""
    new, older, _, _ = FEATURES[feature]
    for k in new + older:
        assert len(rows_of(shipped_table, k)) == 1, k


@EVERY_FEATURE
def test_the_kernels_have_no_hazard(shipped_table, feature):
    """check_isa has returned: no kernel of the build has a hit.  (The 64-bit state of the class and any-of kernels is kept
    in 32-bit halves and shifted by constants - an earlier form of the class seam test was fused into a 64-bit shift by the
    last VGPR and refused here; the record, context and anchor kernels shift 32-bit words only, and the 64-bit values they
    divide are the wave's, in scalar registers; find_anchor_kernel's one DPP move is made by every lane.)"""
    assert all(rows_of(shipped_table, k) for k in FEATURES[feature][0])


@EVERY_FEATURE
def test_the_kernels_stay_within_their_resources(shipped_table, feature):
    _, _, kernels, bound = FEATURES[feature]

    def rows(kernel):
        return rows_of(shipped_table, kernel)
    rows.table = shipped_table
    bound(rows, kernels)
