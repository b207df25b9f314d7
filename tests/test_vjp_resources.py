"""The compiled resources of spart_vjp's two kernels (csrc/spart_vjp.h): no scratch, no spills, no static LDS, and the dynamic
LDS of k_vjp_reduce -- F tiles of vjp_fstride(W) doubles -- within the family's budget for every F."""
import os
import re

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

CSRC = os.path.join(ROOT, "spart-python_amd", "csrc")


def group(F):
    """vjp_group, restated (tests/test_vjp_host.py holds it against the header's)"""
    W = 64
    while W * F > 64:
        W >>= 1
    return W


def fstride(W):
    return 16 * (W + 1) + (((W - 16) & 31) if W < 32 else 0)


def test_vjp_kernels_use_no_scratch_and_no_static_lds(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_vjp_" in k}
    assert len(hits) == 2 and all(any(n in k for k in hits) for n in ("k_vjp_init", "k_vjp_reduce")), sorted(hits)
    for name, k in hits.items():
        print(f"{name}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs, {k['group_segment_fixed_size']} bytes of static LDS")
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] <= 0, (name, k)


def test_dynamic_lds_stays_within_the_family_budget():
    refine = open(os.path.join(CSRC, "spart_refine.h")).read()
    budget = int(re.search(r"constexpr int REFINE_LDS_BUDGET = (\d+);", refine).group(1))
    assert "constexpr int REFINE_JT = 16;" in refine
    src = open(os.path.join(CSRC, "spart_vjp.h")).read()
    assert "return 16 * (W + 1) + (W < 32 ? ((W - 16) & 31) : 0);" in src and "(size_t)F * (size_t)vjp_fstride(W) * 8" in src
    sizes = {F: F * fstride(group(F)) * 8 for F in range(1, 17)}
    print("dynamic LDS of k_vjp_reduce by F:", sizes)
    assert sizes[16] == 16 * 100 * 8 and max(sizes.values()) <= budget, sizes
