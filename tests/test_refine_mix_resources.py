"""The compiled resources of the spart_refine_mix kernels (no GPU needed): no scratch and no spills in the init kernel and in
both instantiations of the step kernel, and the LDS formula the launcher uses (refine_lds_rows(n, n, MIX_MAXV)), recomputed here, within the family's
budget for every (V, F, n) the call accepts."""
import os

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

HEADER = os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine_mix.h")
REFINE = os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine.h")
CAPI = os.path.join(ROOT, "spart-python_amd", "csrc", "spart_capi.hip")
JT, BUDGET, MAXV = 16, 40960, 8


def test_mix_kernels_use_no_scratch(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_refine_mix_" in k}
    assert sum("k_refine_mix_init" in k for k in hits) == 1, sorted(hits)
    assert sum("k_refine_mix_stepILi4E" in k for k in hits) == 1 and sum("k_refine_mix_stepILi8E" in k for k in hits) == 1, sorted(hits)
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)                   # all LDS is the launcher's dynamic region


def rows(n):
    nt = n * (n + 1) // 2
    return n * JT + 2 * JT + (nt + n) + nt + 3 * n + 1 + MAXV


def group(n):
    W = 8
    while W > 4 and rows(n) * (W + 1) * 8 > BUDGET:
        W //= 2
    return W


def test_mix_lds_stays_within_the_budget():
    """refine_lds_rows(n, n, MIX_MAXV) depends on n alone (the blocks are folded from global memory, not staged), so every admissible (V, F, n)
    is covered by n = 1 ... 16: the group rule picks a W whose LDS fits the budget, 8 pixels for small n and 4 at n = 16"""
    src = open(HEADER).read()
    assert "refine_lds_rows(n, n, MIX_MAXV)" in src and "rows = refine_lds_rows(n, n, MIX_MAXV), W = refine_group(rows)" in open(CAPI).read()
    assert "tile_rows * REFINE_JT + 2 * REFINE_JT + (refine_ntri(n) + n) + refine_ntri(n) + 3 * n + 1 + extra" in open(REFINE).read()
    assert "constexpr int MIX_MAXV = 8;" in src
    seen = set()
    for V in range(1, MAXV + 1):
        for F in range(1, 17):
            for Fs in range(F + 1):
                for fit in (0, 1):
                    for active in range(1 if F > Fs else 0, V * (F - Fs) + 1):      # active locals: between Fl (0 if none) and V Fl
                        if F > Fs and active < F - Fs:
                            continue
                        n = Fs + active + (V - 1 if fit else 0)
                        if 1 <= n <= 16:
                            seen.add(n)
                            assert rows(n) * (group(n) + 1) * 8 <= BUDGET, (V, F, Fs, n)
    assert seen == set(range(1, 17))
    assert group(4) == 8 and group(16) == 4 and rows(16) * 5 * 8 <= BUDGET < rows(16) * 9 * 8
