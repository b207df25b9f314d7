"""Register, scratch and LDS budget of k_columns_srf, the SRF-convolved column kernel (no GPU needed: device assembly
metadata).  It runs beside k_columns at the same four waves per SIMD: at most 128 VGPRs, nothing spilled, no scratch, and
no more LDS than the float64 k_columns itself."""
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)


def _find(meta, fragment):
    hits = {k: v for k, v in meta.items() if fragment in k}
    assert hits, fragment
    return hits


def test_srf_column_kernel_has_both_output_types(kernel_meta):
    names = _find(kernel_meta, "k_columns_srfI")
    assert any("k_columns_srfIff" in n for n in names) and any("k_columns_srfIdd" in n for n in names), sorted(names)


def test_srf_column_kernel_fits_four_waves_without_spills(kernel_meta):
    for name, k in _find(kernel_meta, "k_columns_srfI").items():
        assert k["vgpr_count"] <= 128, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)


def test_srf_column_kernel_uses_no_more_lds_than_k_columns(kernel_meta):
    lds = {n: k["group_segment_fixed_size"] for n, k in kernel_meta.items()}
    base = [v for n, v in lds.items() if "k_columnsId" in n]              # the float64 column kernels
    srf = {n: v for n, v in lds.items() if "k_columns_srfI" in n}
    assert base and srf
    for name, v in srf.items():
        assert 0 < v <= min(base), (name, v, base)
