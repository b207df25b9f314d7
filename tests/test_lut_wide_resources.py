"""Resource guard of the wide LUT search (no GPU: hipcc cross-compiles): the K-streamed MFMA scan and collect kernels of
spart_lut_topk_wide keep everything in registers and LDS -- no scratch, no spills -- in both dtypes."""

import pytest

from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


@pytest.mark.parametrize("frag", ["k_lutw_gemmIfLb0E", "k_lutw_gemmIfLb1E", "k_lutw_gemmIdLb0E", "k_lutw_gemmIdLb1E"])
def test_wide_scan_and_collect_use_no_scratch(kernel_meta, frag):
    hits = [v for k, v in kernel_meta.items() if frag in k and "vgpr_count" in v]
    assert hits, frag
    for k in hits:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (frag, k)
