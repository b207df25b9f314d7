"""Resource guard of the leaf-fit kernel (no GPU: hipcc cross-compiles): every instantiation k_refine_leaf<1> ... <9> keeps its
up to 45 + 9 + 1 lane partials, its band tables and the F + 1 leaf evaluations in registers -- no scratch memory and no spilled
register of either kind -- and its per-wave state within a small static LDS block."""
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


def test_every_leaf_fit_instantiation_uses_no_scratch_and_spills_nothing(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_refine_leaf" in k}
    assert len(hits) == 9, sorted(hits)
    for name, k in sorted(hits.items()):
        print(name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 256, (name, k)                          # two waves per SIMD at the least, no AGPR parking
        assert k["group_segment_fixed_size"] <= 20 * 1024, (name, k)      # eight single-wave workgroups per CU within 160 KiB
