"""Resource guard of k_refine_posterior (no GPU: hipcc cross-compiles): its working set stays in registers and LDS -- no
scratch, no spills, in both group sizes it is instantiated for -- and the dynamic LDS the launcher asks for
(refine_posterior_group / refine_posterior_lds_bytes of csrc/spart_refine_posterior.h, re-computed here from its constants and
spart_refine.h's) stays within REFINE_POST_LDS_BUDGET for every F, so that at least two workgroups share a CU's 160 KiB."""
import os
import re

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

CSRC = os.path.join(ROOT, "spart-python_amd", "csrc")


def constants():
    c = {}
    for name in ("spart_refine.h", "spart_refine_posterior.h"):
        src = open(os.path.join(CSRC, name)).read()
        for line in re.findall(r"constexpr int (REFINE_[A-Z_]+ = \d+(?:, REFINE_[A-Z_]+ = \d+)*);", src):
            c.update({n: int(v) for n, v in re.findall(r"(REFINE_[A-Z_]+) = (\d+)", line)})
    return c


def lds_rows(c, F):
    """refine_posterior_lds_rows: the (F + 1) JT tile, 2 JT, three triangles, the full K, 2 F, the flags"""
    return (F + 1) * c["REFINE_JT"] + 2 * c["REFINE_JT"] + 3 * (F * (F + 1) // 2) + F * F + 2 * F + 1


def lds_bytes(c, F, W):
    return lds_rows(c, F) * (W + 1) * 8


def group(c, F):
    W = c["REFINE_POST_MAX_GROUP"]
    while W > c["REFINE_POST_MIN_GROUP"] and lds_bytes(c, F, W) > c["REFINE_POST_LDS_BUDGET"]:
        W >>= 1
    return W


def test_the_header_says_what_this_file_recomputes():
    src = open(os.path.join(CSRC, "spart_refine_posterior.h")).read()
    assert "return (F + 1) * REFINE_JT + 2 * REFINE_JT + 3 * refine_ntri(F) + F * F + 2 * F + 1;" in src
    assert "(size_t)refine_posterior_lds_rows(F) * (size_t)(W + 1) * 8" in src
    assert "W == 8 ? k_refine_posterior<8> : k_refine_posterior<4>" in open(os.path.join(CSRC, "spart_capi.hip")).read()


def test_posterior_kernel_uses_no_scratch_and_shares_a_cu(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_refine_posterior" in k}
    assert len(hits) == 2, sorted(hits)                                        # W = 4 and W = 8
    c = constants()
    assert c["REFINE_MAXF"] == 16 and c["REFINE_JT"] == 16 and c["REFINE_POST_MIN_GROUP"] == 4 and c["REFINE_POST_MAX_GROUP"] == 8
    groups = {F: group(c, F) for F in range(1, c["REFINE_MAXF"] + 1)}
    assert set(groups.values()) == {4, 8} and groups[6] == 8 and groups[16] == 4
    assert all(64 % W == 0 and W * c["REFINE_JT"] >= 64 for W in groups.values())
    most = max(lds_bytes(c, F, W) for F, W in groups.items())
    assert lds_bytes(c, 16, 4) == 40040 and most <= c["REFINE_POST_LDS_BUDGET"] <= 80 * 1024, most
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] % 16 == 0, (name, k)             # the dynamic region starts 16-byte aligned
        assert 2 * (k["group_segment_fixed_size"] + most) <= 160 * 1024, (name, k)
