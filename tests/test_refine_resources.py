"""Resource guard of the refinement kernels (no GPU: hipcc cross-compiles): k_refine_views_init and k_refine_step keep their working
set in registers and LDS -- no scratch, no spills -- and the dynamic LDS the launcher asks for (refine_group / refine_lds_bytes
of csrc/spart_refine.h, re-computed here from its constants) stays within REFINE_LDS_BUDGET for every F, so that at least two
workgroups share a CU's 160 KiB."""
import os
import re

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


def constants():
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine.h")).read()
    c = {n: int(v) for n, v in re.findall(r"constexpr int (REFINE_[A-Z_]+) = (\d+);", src)}
    c.update({n: int(v) for n, v in re.findall(r"constexpr int (REFINE_[A-Z_]+) = (\d+), (?:REFINE_[A-Z_]+) = \d+;", src)})
    c.update({n: int(v) for n, v in re.findall(r"constexpr int REFINE_[A-Z_]+ = \d+, (REFINE_[A-Z_]+) = (\d+);", src)})
    return c


def lds_bytes(c, F, W):
    """refine_lds_bytes of refine_lds_rows(F + 1, F, 0): (F + 1) JT + 2 JT + P + ntri + 3 F + 1 rows of W + 1 doubles"""
    nt = F * (F + 1) // 2
    return ((F + 1) * c["REFINE_JT"] + 2 * c["REFINE_JT"] + (nt + F) + nt + 3 * F + 1) * (W + 1) * 8


def group(c, F):
    W = c["REFINE_MAX_GROUP"]
    while W > c["REFINE_MIN_GROUP"] and lds_bytes(c, F, W) > c["REFINE_LDS_BUDGET"]:
        W >>= 1
    return W


def test_refine_kernels_use_no_scratch_and_share_a_cu(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_refine_" in k}
    assert any("k_refine_views_init" in k for k in hits) and any("k_refine_step" in k for k in hits), sorted(hits)
    c = constants()
    assert c["REFINE_MAXF"] == 16 and c["REFINE_JT"] == 16 and c["REFINE_MIN_GROUP"] == 4 and c["REFINE_MAX_GROUP"] == 8
    most = max(lds_bytes(c, F, group(c, F)) for F in range(1, c["REFINE_MAXF"] + 1))
    assert most <= c["REFINE_LDS_BUDGET"] <= 80 * 1024, most
    assert all(64 % group(c, F) == 0 and group(c, F) * c["REFINE_JT"] >= 64 for F in range(1, 17))
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] % 16 == 0, (name, k)             # the dynamic region starts 16-byte aligned
        assert 2 * (k["group_segment_fixed_size"] + most) <= 160 * 1024, (name, k)
