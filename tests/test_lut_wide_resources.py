"""Resource guard of the wide LUT search (no GPU: hipcc cross-compiles): the K-streamed MFMA scan and collect kernels of
spart_lut_topk_wide keep everything in registers and LDS -- no scratch, no spills -- in both dtypes."""
import os
import shutil

import pytest


@pytest.fixture(scope="module")
def kernel_meta():
    if not any(c and os.path.exists(c) for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc"))):
        pytest.skip("hipcc not available")
    from helpers.kernel_meta import kernel_meta as compiled      # memoised: one device compile per pytest process
    return compiled()


@pytest.mark.parametrize("frag", ["k_lutw_gemmIfLb0E", "k_lutw_gemmIfLb1E", "k_lutw_gemmIdLb0E", "k_lutw_gemmIdLb1E"])
def test_wide_scan_and_collect_use_no_scratch(kernel_meta, frag):
    hits = [v for k, v in kernel_meta.items() if frag in k and "vgpr_count" in v]
    assert hits, frag
    for k in hits:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (frag, k)
