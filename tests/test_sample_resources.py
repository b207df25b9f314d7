"""Resource guard of the sampler's kernels (no GPU: hipcc cross-compiles): k_sample_init, k_sample_table and k_sample_step keep
their working set in registers and LDS -- no scratch, no spills -- and the static LDS of k_sample_step (the band tile of a
wave's 64 rows with the weights and observed values of its observations, re-computed here from the constants of
csrc/spart_sample.h) stays within the project's 40 KiB per workgroup, so that at least three workgroups share a CU's 160 KiB."""
import os
import re

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

LDS_BUDGET = 40960


def constants():
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_sample.h")).read()
    return {n: int(v) for n, v in re.findall(r"constexpr int (SAMPLE_[A-Z_]+) = (\d+);", src)}


def test_sample_kernels_use_no_scratch_and_share_a_cu(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_sample_" in k}
    assert all(any(n in k for k in hits) for n in ("k_sample_init", "k_sample_table", "k_sample_step")) and len(hits) == 3, sorted(hits)
    c = constants()
    assert c["SAMPLE_JT"] == 16 and c["SAMPLE_MAXOPW"] == 16                  # 64 / (W / 2) observations per wave at W = 8
    lds = (c["SAMPLE_JT"] * 65 + 2 * c["SAMPLE_JT"] * (c["SAMPLE_MAXOPW"] + 1)) * 8
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == (lds if "k_sample_step" in name else 0), (name, k)
        assert k["group_segment_fixed_size"] <= LDS_BUDGET and k["vgpr_count"] <= 128, (name, k)
        print(name, k)
