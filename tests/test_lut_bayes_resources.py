"""Resource guard of the posterior kernels (no GPU: hipcc cross-compiles): all four instantiations of k_lut_bayes keep their
working set in registers and LDS -- no scratch memory, no VGPR spills -- and the dynamic LDS their launcher asks for (the sorted tile
numbers, the observation and its weight row) stays within the 64 KiB a kernel gets without opting in, at the widest LUT."""
import os
import re

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

NWLS = 2162


def test_bayes_kernels_use_no_scratch_and_fit_the_default_lds(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_lut_bayes" in k}
    assert len([k for k in hits if "k_lut_bayes_empty" not in k]) == 4           # float / double x filter / brute force
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_lut.h")).read()
    sort = int(re.search(r"constexpr int LUT_BAYES_SORT = (\d+);", src).group(1))
    assert sort >= 4 * 256 + 64 and sort & (sort - 1) == 0                       # a whole candidate list, a power of two
    for name, k in hits.items():
        # (many wave-uniform values live in SGPRs here -- 106 of them; a few spill into VGPR lanes, which costs no memory traffic:
        # what is guarded is scratch memory)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] % 16 == 0, (name, k)
        assert k["group_segment_fixed_size"] + sort * 4 + 2 * NWLS * 8 <= 64 * 1024, (name, k)   # lut_bayes_lds_bytes, float64
