"""Resource guard of the products kernel (no GPU: hipcc cross-compiles): every k_products* kernel keeps its working set in
registers and LDS -- no scratch memory, no spilled register of either kind -- within the 128 VGPRs of four waves per SIMD, the
occupancy of the column kernels whose mapping it shares."""
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


def test_products_kernels_use_no_scratch_and_at_most_128_vgprs(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_products" in k}
    assert hits, sorted(kernel_meta)[:5]
    for name, k in hits.items():
        print(name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
        assert k["group_segment_fixed_size"] <= 40 * 1024, (name, k)      # four workgroups per CU within 160 KiB
