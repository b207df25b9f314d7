"""The four LUT searches at the ends of the number range, on the MI355X: index AND cost bit-equal to the NUMPY brute force of
the defined cost (tools/lut_brute_force.py on the CPU: IEEE arithmetic, subnormals kept -- not the torch one, whose
elementwise kernels' treatment of float32 subnormals on the GPU nobody here has measured).

The cases (tests/helpers/lut_hostile.py builds them and asserts, on the oracle, that each is what it claims): a large common
offset, band scales over 12 decades with and without 1 / scale^2 weights, per-observation weights over 24 decades, costs that
are subnormal, zero, or both, LUTs scaled down to where the absolute slack of the rounding bound (LutNum<T>::tiny) takes
over, ONE finite entry near the largest number (in a row that is, and one that is not, sampled for the column centres), and
rows whose centred norm overflows although their cost against an observation is finite (the header's row rule, modelled by the
brute force's ``row_ok``).  B = 3 001 (20 011 for the sampled / unsampled huge entry), M = 40, nb = 13 and 211, k = 1 and 10.

What the library did with them on one MI355X before the centre cap and the row rule in the exact paths:
the huge-entry cases in a sampled row gave (-1, +inf) for 40 of 40 observations from spart_lut_topk_obs_weights and sent all 40
to the brute force in the other three searches; the norm-rule case returned the ruled-out rows for its 5 special observations
from spart_lut_nearest / _topk / _topk_wide.

Wall time on one MI355X: 5 s for all the cases (measured when they were four tests, one per width and dtype: 0.4 ... 1.8 s
each, most of it the numpy oracle on the CPU).  What else was and was not measured: DESIGN.md section 13."""
import numpy as np
import pytest

from helpers import lut_hostile as H
from helpers.lut_calls import ENTRIES, bf, eng, lut_call, torch_mod  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

WIDTHS = ((13, 0), (211, 1))            # (nb, seed of the builders)


def searches_for(case, nb):
    """the entry points a case goes to: per-observation weights -> the obs-weights search alone; otherwise all four that take nb
    (the obs-weights search with every weight row equal to the shared one, or to 1)"""
    if case.per_observation:
        return ["spart_lut_topk_obs_weights"]
    return [e for e, (_, widest, _) in ENTRIES.items() if nb <= widest]


def run(torch, eng, entry, case, k, dtype):
    dev = "cuda:0"
    lut, obs = torch.as_tensor(case.lut, device=dev), torch.as_tensor(case.obs, device=dev)
    w = None if case.w is None else torch.as_tensor(case.w, device=dev)
    if entry == "spart_lut_topk_obs_weights" and not case.per_observation:
        w = (torch.ones_like(obs) if w is None else w[None, :].repeat(obs.shape[0], 1)).contiguous()
    rc, idx, cost, st = lut_call(torch, eng, entry, lut, obs, None if entry == "spart_lut_nearest" else k, w, dtype, guard=True)
    assert rc == 0, (entry, case.name, eng.lib.spart_last_error(None))
    idx, cost = idx.cpu().numpy(), cost.cpu().numpy()
    return (idx[:, None], cost[:, None], st) if entry == "spart_lut_nearest" else (idx, cost, st)


CASES = [pytest.param(dtype, nb, seed, name, id=f"{dtype}-{nb}-{name}")
         for dtype in ("float32", "float64") for nb, seed in WIDTHS for name in H.case_names(dtype, nb)]


@pytest.mark.parametrize("dtype,nb,seed,name", CASES)
def test_hostile_magnitudes(torch_mod, eng, bf, dtype, nb, seed, name):
    case = H.hostile_case(bf, dtype, nb, seed, name)
    want_i, want_c = H.oracle(bf, case, 10)
    case.holds(want_i, want_c)                                         # not vacuous: checked on the CPU, before the GPU is asked
    huge = name.startswith("huge_entry")
    if huge:                                                           # the plain brute force already leaves that row out
        plain_i, plain_c = bf.brute_force_topk_numpy(case.lut, case.obs, 10)
        assert np.array_equal(plain_i, want_i) and np.array_equal(plain_c, want_c)
    wrong = []
    for entry in searches_for(case, nb):
        for k in (1, 10):
            if entry == "spart_lut_nearest" and k != 1:
                continue
            idx, cost, st = run(torch_mod, eng, entry, case, k, dtype)
            # by the (cost, row) order the oracle's first k columns are the k nearest, padding included
            if not (np.array_equal(idx, want_i[:, :k]) and np.array_equal(cost, want_c[:, :k])):
                bad = np.flatnonzero((idx != want_i[:, :k]).any(axis=1) | (cost != want_c[:, :k]).any(axis=1))
                m = int(bad[0])
                wrong.append((entry, k, f"{len(bad)} of {len(idx)} observations", f"m = {m}", idx[m].tolist(),
                              want_i[m, :k].tolist(), cost[m].tolist(), want_c[m, :k].tolist(), st))
            # one huge entry must not cost the filter: these observations are 2 % from a row of a uniform LUT, which the
            # filter settles alone when that entry is absent (so does a correct answer reached through the brute force not pass)
            if huge and st["brute_force"] != 0:
                wrong.append((entry, k, "observations left to the brute force", st))
    assert not wrong, "\n".join(map(str, wrong))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb,seed", WIDTHS)
def test_band_scale_weights_rerank_the_rows(bf, nb, seed, dtype):
    """band_scales is not band_scales_weighted in disguise: the two oracles agree on fewer than half of the places"""
    a, b = (H.oracle(bf, H.hostile_case(bf, dtype, nb, seed, n), 10)[0] for n in ("band_scales", "band_scales_weighted"))
    assert (a == b).mean() < 0.5
