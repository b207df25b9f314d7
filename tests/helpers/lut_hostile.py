"""LUT search inputs at the ends of the number range, built in numpy (IEEE arithmetic, subnormals kept): what
tests/test_gpu_lut_magnitudes.py runs on the GPU and tests/test_lut_topk_host.py runs through the two host brute forces.

A case is a Hostile: lut (B, nb), obs (M, nb), weights (None, (nb,) shared or (M, nb) per observation), row_ok (None, or the
(B,) verdict of the overflowing-norm rule, tools/lut_brute_force.py: norm_rule_numpy) and ``holds(idx, cost)``, which asserts
on the oracle's k = 10 answer that the case is what its name says -- a case that no longer reaches subnormal costs, say,
fails there, on the CPU, before any search is asked.  The base data are the builders of the other LUT tests: a LUT of
rng.uniform(0, 0.6) and observations = sampled rows x (1 + 0.02 N(0, 1))."""
import numpy as np

B_SMALL, B_LARGE, M_OBS = 3001, 20_011, 40
NORM_ROWS = (5, 700, 1500, 2999, 3000)         # the rows of the norm-rule case


class Hostile:
    def __init__(self, name, lut, obs, w=None, row_ok=None, holds=None):
        self.name, self.lut, self.obs, self.w, self.row_ok = name, np.ascontiguousarray(lut), np.ascontiguousarray(obs), w, row_ok
        self.holds = holds or (lambda idx, cost: None)
        assert self.lut.dtype == self.obs.dtype and (w is None or w.dtype == self.lut.dtype)

    @property
    def per_observation(self):
        return self.w is not None and self.w.ndim == 2


def npdt(dtype):
    return np.float32 if dtype == "float32" else np.float64


def base(dtype, nb, seed, B=B_SMALL, M=M_OBS):
    """the benign case in float64 (the callers scale it, then round it to the dtype) and the rows the observations came from"""
    rng = np.random.default_rng(seed)
    lut = rng.uniform(0.0, 0.6, (B, nb))
    pick = rng.integers(0, B, M)
    obs = lut[pick] * (1.0 + 0.02 * rng.standard_normal((M, nb)))
    return rng, lut, obs, pick


def _finite(idx, cost):
    assert (idx >= 0).all() and np.isfinite(cost).all()


def _subnormal(cost):
    return (cost > 0) & (cost < np.finfo(cost.dtype).tiny)


def scaled(dtype, nb, seed, factor, name, holds=None):
    t = npdt(dtype)
    _, lut, obs, _ = base(dtype, nb, seed)
    return Hostile(name, (lut * factor).astype(t), (obs * factor).astype(t), holds=holds)


def offset(dtype, nb, seed):
    """a large common offset: only the centring keeps the filter usable.  Observations are exact rows."""
    t = npdt(dtype)
    rng = np.random.default_rng(seed)
    off, amp = (1000.0, 1e-3) if dtype == "float32" else (1e6, 1e-6)
    lut = (off + amp * rng.uniform(0.0, 1.0, (B_SMALL, nb))).astype(t)
    obs = lut[rng.integers(0, B_SMALL, M_OBS)].copy()

    def holds(idx, cost):
        assert (cost[:, 0] == 0).all()
        assert np.mean([len(np.unique(c)) for c in cost]) >= 9.0        # the order among the 10 best is not a mass tie
    return Hostile("offset", lut, obs, holds=holds)


def band_scales(dtype, nb, seed, weighted):
    """column j in units 10^(-6 ... 6) (a radiance LUT); weighted by 1 / scale^2 the small bands count again"""
    t = npdt(dtype)
    _, lut, obs, _ = base(dtype, nb, seed)
    s = np.logspace(-6.0, 6.0, nb)
    w = (1.0 / (s * s)).astype(t) if weighted else None
    return Hostile("band_scales_weighted" if weighted else "band_scales", (lut * s).astype(t), (obs * s).astype(t), w, holds=_finite)


def weight_range(dtype, nb, seed):
    """per-observation weights over 24 decades (1 / sigma^2 with sigma from 1e-6 to 1e6)"""
    t = npdt(dtype)
    rng, lut, obs, _ = base(dtype, nb, seed)
    w = (10.0 ** rng.uniform(-12.0, 12.0, obs.shape)).astype(t)
    return Hostile("weight_range", lut.astype(t), obs.astype(t), w, holds=_finite)


def subnormal_costs(dtype, nb, seed):
    """LUT x 1e-19 / x 1e-160: at least 90 % of the 10 best costs are subnormal.  A cost is a sum over nb bands, so at 211
    bands in float32 the x 1e-19 costs (7e-41 ... 1e-37) straddle the smallest normal number instead (10 % subnormal): that
    input is kept as ``straddles_normal`` and the 90 % case is x 1e-20 there."""
    def holds(idx, cost):
        assert _subnormal(cost).mean() >= 0.9
    wide32 = dtype == "float32" and nb > 31
    return scaled(dtype, nb, seed, (1e-20 if wide32 else 1e-19) if dtype == "float32" else 1e-160, "subnormal_costs", holds)


def straddles_normal(dtype, nb, seed):
    def holds(idx, cost):
        assert _subnormal(cost).any() and (cost >= np.finfo(cost.dtype).tiny).any()
    return scaled(dtype, nb, seed, 1e-19, "straddles_normal", holds)


def mixed_zero_subnormal(dtype, nb, seed):
    def holds(idx, cost):
        assert (cost == 0).any() and _subnormal(cost).any()
    return scaled(dtype, nb, seed, 1e-21, "mixed_zero_subnormal", holds)


def all_zero(dtype, nb, seed):
    def holds(idx, cost):
        assert (cost == 0).all() and (idx == np.arange(idx.shape[1])[None, :]).all()
    return scaled(dtype, nb, seed, 1e-23 if dtype == "float32" else 1e-170, "all_zero", holds)


def huge_name(value, row, B):
    return f"huge_entry_{value:g}_row{row}_of_{B}"


def huge_entry(dtype, nb, seed, B, row, value):
    """ONE finite entry near the largest number, in column 2 of ``row``.  That row costs +inf against every observation here,
    so the plain brute force never returns it, and every answer is the clean LUT's with that row left out."""
    t = npdt(dtype)
    _, lut, obs, pick = base(dtype, nb, seed, B=B)
    lut, obs = lut.astype(t), obs.astype(t)
    lut[row, min(2, nb - 1)] = value
    row_ok = np.ones(B, dtype=bool)
    row_ok[row] = False

    def holds(idx, cost):
        assert np.isfinite(lut).all() and not (idx == row).any()
        assert (idx[pick != row] >= 0).all()
    return Hostile(huge_name(value, row, B), lut, obs, row_ok=row_ok, holds=holds)


def norm_rule(bf, dtype, nb, seed):
    """five rows with band 0 = 1e25 / 1e200 and five observations equal to them in band 0: their cost against those rows is
    finite, and the rows' centred norm overflows for every centre a moderate column can have -- so they never appear, and the
    five observations, 1e25 away from every other row, match nothing"""
    t = npdt(dtype)
    big = 1e25 if dtype == "float32" else 1e200
    _, lut, obs, _ = base(dtype, nb, seed)
    lut, obs = lut.astype(t), obs.astype(t)
    rows = np.array(NORM_ROWS)
    lut[rows, 0] = big
    obs[:5] = lut[rows]
    if nb > 1:
        obs[:5, 1:] *= t(1.02)
    moderate = np.delete(lut, rows, axis=0)
    verdicts = [bf.norm_rule_numpy(lut, c) for c in (moderate.min(axis=0), moderate.max(axis=0), moderate.mean(axis=0))]
    assert all(np.array_equal(v, verdicts[0]) for v in verdicts)
    row_ok = verdicts[0]
    assert (~row_ok).sum() == 5 and not row_ok[rows].any()

    def holds(idx, cost):
        assert (idx[:5] == -1).all() and np.isinf(cost[:5]).all() and (idx[5:] >= 0).all()
    return Hostile("norm_rule", lut, obs, row_ok=row_ok, holds=holds)


def builders(dtype, nb):
    """name -> build(bf, seed) of every case of the table for one dtype and width, in a fixed order; nothing is built here, so
    the names can parametrise a test.  ``bf`` is tools/lut_brute_force (the norm-rule case takes its norm_rule_numpy)."""
    f32 = dtype == "float32"
    out = {"offset": lambda bf, seed: offset(dtype, nb, seed),
           "band_scales": lambda bf, seed: band_scales(dtype, nb, seed, False),
           "band_scales_weighted": lambda bf, seed: band_scales(dtype, nb, seed, True),
           "weight_range": lambda bf, seed: weight_range(dtype, nb, seed),
           "subnormal_costs": lambda bf, seed: subnormal_costs(dtype, nb, seed),
           "all_zero": lambda bf, seed: all_zero(dtype, nb, seed),
           "norm_rule": lambda bf, seed: norm_rule(bf, dtype, nb, seed)}
    if f32:
        out["mixed_zero_subnormal"] = lambda bf, seed: mixed_zero_subnormal(dtype, nb, seed)
        if nb > 31:
            out["straddles_normal"] = lambda bf, seed: straddles_normal(dtype, nb, seed)
        for f in (1e-10, 1e-13, 1e-15, 1e-17):
            out[f"tiny_scale_{f:g}"] = lambda bf, seed, f=f: scaled(dtype, nb, seed, f, f"tiny_scale_{f:g}")
    for value in ((3e38,) if f32 else (1e160, 1e308)):
        # 3 001 rows: every row is sampled for the centre; 20 011 rows: stride 2, row 0 is sampled and row 1 is not
        for B, row in ((B_SMALL, 1500), (B_LARGE, 0), (B_LARGE, 1)):
            out[huge_name(value, row, B)] = lambda bf, seed, B=B, row=row, value=value: huge_entry(dtype, nb, seed, B, row, value)
    return out


def case_names(dtype, nb):
    return list(builders(dtype, nb))


def hostile_case(bf, dtype, nb, seed, name):
    case = builders(dtype, nb)[name](bf, seed)
    assert case.name == name
    return case


def hostile_cases(bf, dtype, nb, seed):
    return [hostile_case(bf, dtype, nb, seed, name) for name in case_names(dtype, nb)]


def oracle(bf, case, k):
    """the numpy brute force of the case's search: shared weights (or none) -> spart_lut_nearest / _topk / _topk_wide's
    definition; per-observation weights -> spart_lut_topk_obs_weights'"""
    if case.per_observation:
        return bf.brute_force_topk_obs_weights_numpy(case.lut, case.obs, k, case.w, row_ok=case.row_ok)
    return bf.brute_force_topk_numpy(case.lut, case.obs, k, case.w, row_ok=case.row_ok)
