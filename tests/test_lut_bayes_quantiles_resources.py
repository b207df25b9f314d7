"""Resource guard of the posterior-quantile kernels (no GPU: hipcc cross-compiles): the four instantiations of
k_lut_posterior_quant keep the intervals of their level group in registers -- no scratch memory, no VGPR spills, at most 128
VGPRs (four waves per SIMD, which the 8 KiB of sorted tile numbers per single-wave workgroup allows anyway) -- and use the
dynamic LDS of k_lut_bayes' launcher and nothing else."""
import os
import re

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

NWLS = 2162


def test_quantile_kernels_use_no_scratch_and_stay_within_128_vgprs(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_lut_posterior_quant" in k and "quant_empty" not in k}
    assert len(hits) == 4                                                        # float / double x filter / brute force
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_lut.h")).read()
    sort = int(re.search(r"constexpr int LUT_BAYES_SORT = (\d+);", src).group(1))
    group, most = (int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("LUT_BAYES_QG", "LUT_BAYES_MAXQ"))
    assert 1 <= group <= most == 8
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)                     # (the (row, omega) cache lives in the tile buffer)
        assert sort * 4 + 2 * NWLS * 8 <= 64 * 1024
