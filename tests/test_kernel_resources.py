"""Occupancy guard (no GPU needed: hipcc cross-compiles): the register budgets the performance numbers rest on.

The band kernel's speed depends on resident waves per SIMD (512 VGPRs / wave budget): 5 for the float32 kernels
(<= 96 VGPRs, no scratch), 3 for the float64 ones (<= 168).  A change that silently pushes a kernel over the edge
would only show up as a slower benchmark; this test makes it a failure on the build machine."""

from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


def _find(meta, fragment):
    hits = [v for k, v in meta.items() if fragment in k and "vgpr_count" in v]
    assert hits, fragment
    return hits


def test_float32_band_kernels_keep_five_waves_per_simd(kernel_meta):
    for frag in ("k_bandsIfLi0ELi1E", "k_bandsIfLi1ELi1E", "k_bandsIfLi2ELi1E"):
        for k in _find(kernel_meta, frag):
            assert k["vgpr_count"] <= 96, (frag, k)
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (frag, k)


def test_float64_band_kernels_keep_three_waves_per_simd(kernel_meta):
    for k in _find(kernel_meta, "k_bandsIdLi0ELi1E"):
        assert k["vgpr_count"] <= 168, k
        assert k["private_segment_fixed_size"] <= 256, k       # a few dozen spilled values, not a spilled loop


def test_column_kernel_keeps_four_waves_per_simd(kernel_meta):
    """k_columns (canopy model at the sensor bands + SMAC + TOC->TOA in one wave): <= 128 VGPRs, at most a handful of
    spilled values (2 measured), never a spilled loop"""
    for k in _find(kernel_meta, "k_columnsI"):
        assert k["vgpr_count"] <= 128 and k["private_segment_fixed_size"] <= 32 and k["vgpr_spill_count"] <= 4, k
