"""Resource guard of the parameter-summary kernel (no GPU: hipcc cross-compiles): every instantiation of k_lut_summarise
keeps its working set in registers and LDS -- no scratch, no spills -- and a launch with k <= 64 asks for at most 64 KiB of
LDS (static + the dynamic size its launcher requests, LUT_SUM_SMALL_LDS_BYTES of csrc/spart_lut.h), so that two workgroups
fit a CU's 160 KiB."""
import os
import re

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


def launcher_constants():
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_lut.h")).read()
    return {n: int(v) for n, v in re.findall(r"constexpr int (LUT_SUM_[A-Z_]+) = (\d+);", src)}


def test_summarise_kernel_uses_no_scratch_and_fits_two_workgroups_per_cu(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_lut_summarise" in k}
    assert hits
    c = launcher_constants()
    assert c["LUT_SUM_SMALL_K"] == 64 and c["LUT_SUM_MAXP"] == 64
    # the launcher's request for k <= LUT_SUM_SMALL_K: k doubles for each of at most 64 working lanes
    assert c["LUT_SUM_SMALL_LDS_BYTES"] == c["LUT_SUM_SMALL_K"] * 64 * 8
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] % 16 == 0, (name, k)            # the dynamic region starts 16-byte aligned
        assert k["group_segment_fixed_size"] + c["LUT_SUM_SMALL_LDS_BYTES"] <= 64 * 1024, (name, k)
