"""Resource guard of the per-observation-weights LUT search (no GPU: hipcc cross-compiles): its K = 2 nb MFMA scan and
collect kernels keep everything in registers and LDS -- no scratch, no spills -- in both dtypes."""

import pytest

from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


@pytest.mark.parametrize("frag", ["k_lutow_gemmIfLb0E", "k_lutow_gemmIfLb1E", "k_lutow_gemmIdLb0E", "k_lutow_gemmIdLb1E",
                                  "k_lutow_obsIfE", "k_lutow_obsIdE", "k_lutow_qIfE", "k_lutow_qIdE",
                                  "k_lutw_selectIfLi32ELb0ELb1E", "k_lutw_selectIfLi32ELb1ELb1E",
                                  "k_lutw_selectIdLi16ELb0ELb1E", "k_lutw_selectIdLi16ELb1ELb1E"])
def test_obs_weights_kernels_use_no_scratch(kernel_meta, frag):
    hits = [v for k, v in kernel_meta.items() if frag in k and "vgpr_count" in v]
    assert hits, frag
    for k in hits:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (frag, k)
