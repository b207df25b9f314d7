"""spart_lut_bayes / Engine.lut_bayes / retrieve(bayes=...) on the MI355X: the likelihood-weighted LUT estimate against its
definition (tools/lut_bayes_defined.py) -- the exact parts bit for bit, the sums within a derived rounding bound --, the
filter path against the brute-force path, batch and chunk independence, hostile inputs, and the retrieval calls."""
import json
import math
import os

import numpy as np
import pytest

from helpers.lut_bayes_calls import FILL, OUTS, bayes_call, defined, noisy_case, same, to_np
from helpers.lut_calls import (bf, eng, torch_mod,  # noqa: F401  (fixtures)
                               equal_rows_case, lut_call, tdtype)

pytestmark = pytest.mark.gpu
DTYPES = ["float32", "float64"]
INVALID, WORKSPACE = -1, -3
B0 = 32 * 300 + 5


def run(torch, eng, lut, params, obs, w, dtype, **kw):
    rc, res, st = bayes_call(torch, eng, lut, params, obs, w, dtype=dtype, **kw)
    assert rc == 0, eng.lib.spart_last_error(None)
    return res, st


_cases = {}


def case(torch, eng, dtype, nb):
    """B0 rows, 257 observations, relative-noise weights: the call (filter path) and the definition, computed once"""
    if (dtype, nb) not in _cases:
        td = tdtype(torch, dtype)
        g = torch.Generator(device="cuda:0").manual_seed(1000 + nb)
        # (noise levels at which the sets within cut = 50 run from a few rows to thousands: at 211 bands the chi^2 of a random
        # row is 211 / (6 sigma^2) within a few per cent, so the set is one row or every row unless sigma is about 0.8)
        lut, params, obs, w = noisy_case(torch, g, B0, 257, nb, 5, td, rel=0.5, floor=0.55 if nb == 211 else 0.01)
        res, st = run(torch, eng, lut, params, obs, w, dtype)
        args = [t.cpu().numpy() for t in (lut, params, obs, w)]
        _cases[(dtype, nb)] = (lut, params, obs, w, res, st, defined.lut_bayes_defined(*args), defined.lut_bayes_exact(*args))
    return _cases[(dtype, nb)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [13, 211])
def test_exact_parts(torch_mod, eng, nb, dtype):
    """best_idx / best_cost = lut_topk(k = 1, (M, nb) weights) bit for bit, count = the definition's, all on the filter path"""
    torch = torch_mod
    lut, params, obs, w, res, st, want, _ = case(torch, eng, dtype, nb)
    assert st["brute_force"] == 0 and st["candidate_tiles"] > 0, st
    rc, idx, cost, _ = lut_call(torch, eng, "spart_lut_topk_obs_weights", lut, obs, 1, w, dtype)
    assert rc == 0
    assert torch.equal(res["best_idx"], idx[:, 0]) and torch.equal(res["best_cost"], cost[:, 0])
    got = to_np(res)
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["best_idx"], want["best_idx"])
    assert np.array_equal(got["best_cost"], want["best_cost"])
    assert want["count"].max() > 64 and want["count"].min() >= 1          # (the sums below are over real sets)


def check_values(got, want, exact, cut, tau):
    """The rounding bound of the ordered float64 sums against the exactly rounded ones (math.fsum) of the same terms.
    omega: the device's exp is within 3e-16 = 1.35 * 2^-52 of e^a (test_gpu_devmath), the reference's within 2^-53; the
    argument a = e / (2 tau) <= cut / (2 tau) carries one rounding, which moves omega by at most a * 2^-53 relative.  So every
    omega is within eps_w = (4 + cut / tau) * 2^-52 of the reference's (a slack of more than 2 on the constant).
    sum_w: n positive terms added in order lose at most (n - 1) * 2^-53 relative, so |sum_w - ref| <= (eps_w + n * 2^-53) ref;
      the bound asserted carries the factor 4:  f = 4 (eps_w + n * 2^-53).
    mean: the products omega x add 2^-53 each, the sum n * 2^-53 of sum |omega x|, the division f / 4 and 2^-53 of |mean| <= A,
      A = sum |omega x| / sum omega:  |mean - ref| <= 2 (eps_w + (n + 1) * 2^-53) A <= f A.
    ess = sum_w^2 / s2: s2's terms omega^2 carry 2 eps_w + 2^-53, so s2 is within 2 f, sum_w^2 within 2 f: 4 f relative.
    var = sum omega d^2 / sum_w, d = x - mean: positive terms, three roundings each and the sum: 2 f relative, plus the effect
      of the mean's own error delta <= f A on d: sum omega (d - delta)^2 / sum_w = var + delta^2 (the cross term vanishes with
      sum omega d = 0 up to the rounding of the reference mean, 2 delta A 2^-52, which the factor 3 covers):
      |std^2 - ref| <= 3 f var + 2 (f A)^2 (std^2 undoes the square root: 2^-51 relative, inside the same factor).
    cut = inf: omega underflows to 0 beyond a = 745, and is below 2^-1022 from a = 709 on, where its relative error does not
      matter against sum_w >= 1; the bound uses cut / tau <= 1500."""
    n = want["count"].astype(np.float64)
    eps_w = (4.0 + min(cut / tau, 1500.0)) * 2.0 ** -52
    f = 4.0 * (eps_w + n * 2.0 ** -53)
    ok = n > 0
    worst = {}
    for name, err, bound in (("sum_w", np.abs(got["sum_w"] - exact["sum_w"]), f * exact["sum_w"]),
                             ("ess", np.abs(got["ess"] - exact["ess"]), 4 * f * exact["ess"]),
                             ("mean", np.abs(got["mean"] - exact["mean"]), f[:, None] * exact["abs_mean"]),
                             ("var", np.abs(got["std"] ** 2 - exact["var"]),
                              3 * f[:, None] * exact["var"] + 2 * (f[:, None] * exact["abs_mean"]) ** 2)):
        worst[name] = float(np.max((err / np.maximum(bound, 1e-300))[ok]))
        print(f"{name}: worst error / bound = {worst[name]:.3g}")
    for name, r in worst.items():
        assert r <= 1.0, (name, r)
    # and the definition in plain numpy (its exp is not the device's: the same bound, twice)
    assert np.all(np.abs(got["sum_w"] - want["sum_w"])[ok] <= 2 * (f * exact["sum_w"])[ok])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [13, 211])
def test_values_against_the_definition(torch_mod, eng, nb, dtype):
    _, _, _, _, res, _, want, exact = case(torch_mod, eng, dtype, nb)
    check_values(to_np(res), want, exact, 50.0, 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_temperature_and_cut(torch_mod, eng, dtype):
    torch = torch_mod
    td = tdtype(torch, dtype)
    g = torch.Generator(device="cuda:0").manual_seed(5)
    lut, params, obs, w = noisy_case(torch, g, 2053, 33, 6, 27, td, rel=0.5)
    args = [t.cpu().numpy() for t in (lut, params, obs, w)]
    for cut, tau in ((3.5, 0.25), (200.0, 7.0)):
        res, st = run(torch, eng, lut, params, obs, w, dtype, cut=cut, temperature=tau)
        want = defined.lut_bayes_defined(*args, cut=cut, temperature=tau)
        assert st["brute_force"] == 0
        assert np.array_equal(to_np(res)["count"], want["count"])
        check_values(to_np(res), want, defined.lut_bayes_exact(*args, cut=cut, temperature=tau), cut, tau)
    r0, _ = run(torch, eng, lut, params, obs, w, dtype, cut=9.0, temperature=0.0)       # temperature 0 = 1.0
    r1, _ = run(torch, eng, lut, params, obs, w, dtype, cut=9.0, temperature=1.0)
    assert same(torch, r0, r1) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary(torch_mod, eng, dtype):
    """nb = 1, obs 0, w 1, LUT {0, 2, nextafter(2), ...}: e of the row at 2 is exactly 4"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    npdt = np.float32 if dtype == "float32" else np.float64
    two = npdt(2.0)
    rows = [npdt(0.0), two, np.nextafter(two, npdt(3.0)), npdt(2.5), npdt(3.0)] + [npdt(5.0 + i) for i in range(70)]
    lut = torch.as_tensor(np.array(rows, dtype=npdt)[:, None], device="cuda:0")
    params = torch.arange(1.0, lut.shape[0] + 1, dtype=torch.float64, device="cuda:0")[:, None].repeat(1, 3).contiguous()
    params[:, 1] = params[:, 0] * math.pi
    obs = torch.zeros((1, 1), dtype=td, device="cuda:0")
    w = torch.ones((1, 1), dtype=td, device="cuda:0")
    for bfc in (0, 1):
        res, _ = run(torch, eng, lut, params, obs, w, dtype, cut=4.0, brute_force=bfc)
        assert res["count"].tolist() == [2] and res["best_idx"].tolist() == [0] and res["best_cost"].tolist() == [0.0]
        res, _ = run(torch, eng, lut, params, obs, w, dtype, cut=4.000001, brute_force=bfc)
        assert res["count"].tolist() == [3]
        res, _ = run(torch, eng, lut, params, obs, w, dtype, cut=0.0, brute_force=bfc)          # a unique minimum
        assert res["count"].tolist() == [1] and res["ess"].tolist() == [1.0] and res["sum_w"].tolist() == [1.0]
        assert torch.equal(res["mean"][0], params[0]) and res["std"][0].tolist() == [0.0, 0.0, 0.0]
    g = torch.Generator(device="cuda:0").manual_seed(3)
    lut, obs = equal_rows_case(torch, g, td, nb=13, B=4101)                                     # exact ties
    params = torch.rand((4101, 2), generator=g, device="cuda:0", dtype=torch.float64)
    w = torch.ones_like(obs)
    res, _ = run(torch, eng, lut, params, obs, w, dtype, cut=0.0)
    ti, tc = lut_call(torch, eng, "spart_lut_topk_obs_weights", lut, obs, 2, w, dtype)[1:3]
    tied = tc[:, 0] == tc[:, 1]
    assert torch.equal(res["count"][tied], torch.full_like(res["count"][tied], 4100)) and bool(tied.any())
    assert torch.equal(res["count"][~tied], torch.ones_like(res["count"][~tied]))
    assert torch.equal(res["best_idx"], ti[:, 0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [13, 211])
def test_brute_force_and_batch_independence(torch_mod, eng, nb, dtype):
    torch = torch_mod
    lut, params, obs, w, res, _, _, _ = case(torch, eng, dtype, nb)
    sub = torch.arange(0, 257, 16, device="cuda:0")                       # (the brute force over 17 observations: seconds)
    part, _ = run(torch, eng, lut, params, obs[sub].contiguous(), w[sub].contiguous(), dtype)
    assert same(torch, res, part, rows=sub) is None                       # inside a batch of 257 or of 17
    brute, st = run(torch, eng, lut, params, obs[sub].contiguous(), w[sub].contiguous(), dtype, brute_force=1)
    assert st["brute_force"] == sub.numel() and st["candidate_tiles"] == 0
    assert same(torch, part, brute) is None
    one, _ = run(torch, eng, lut, params, obs[100:101].contiguous(), w[100:101].contiguous(), dtype)       # M = 1
    assert same(torch, res, one, rows=slice(100, 101)) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks(torch_mod, eng, dtype):
    """M = chunk + 37 against its slices: the observation's chunk does not matter"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    chunk, B, nb = 16_384, 4101, 5
    g = torch.Generator(device="cuda:0").manual_seed(77)
    lut, params, obs, w = noisy_case(torch, g, B, chunk + 37, nb, 3, td, rel=0.3)
    need = [int(eng.lib.spart_lut_bayes_workspace_bytes(0 if dtype == "float32" else 1, B, nb, m)) for m in (chunk, chunk + 37)]
    assert 4 * 37 <= need[1] - need[0] < 4 * 37 + 256
    res, st = run(torch, eng, lut, params, obs, w, dtype, cut=12.0)
    assert st["brute_force"] == 0
    for lo, hi in ((0, 37), (chunk - 5, chunk + 37), (chunk, chunk + 37)):
        part, _ = run(torch, eng, lut, params, obs[lo:hi].contiguous(), w[lo:hi].contiguous(), dtype, cut=12.0)
        assert same(torch, res, part, rows=slice(lo, hi)) is None, (lo, hi)
    assert int(res["count"].max()) > 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_bands(torch_mod, eng, dtype):
    """zero weights with NaN in obs = the LUT with those columns removed, bit for bit"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    g = torch.Generator(device="cuda:0").manual_seed(8)
    lut, params, obs, w = noisy_case(torch, g, 3001, 41, 13, 4, td, rel=0.5)
    keep = torch.ones(13, dtype=torch.bool, device="cuda:0")
    keep[[2, 7, 12]] = False
    w2, obs2 = w.clone(), obs.clone()
    w2[:, ~keep] = 0
    obs2[:, ~keep] = float("nan")
    a, _ = run(torch, eng, lut, params, obs2, w2, dtype)
    b, _ = run(torch, eng, lut[:, keep].contiguous(), params, obs[:, keep].contiguous(), w[:, keep].contiguous(), dtype)
    assert same(torch, a, b) is None and int(a["count"].max()) > 1


def plain_sums(bf, params, rows):
    """spart_lut_summarise's ordered sums over ``rows``: mean and std (ddof = 0)"""
    want = bf.summarise_defined(params, np.asarray(rows, dtype=np.int64)[None, :])
    return want[0][0], want[2][0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow_to_brute_force(torch_mod, eng, bf, dtype):
    """more rows than the candidate lists hold: cut = inf, and all-zero weights, are decided by the brute force"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    B, nb, M = 40_005, 5, 8
    g = torch.Generator(device="cuda:0").manual_seed(21)
    lut, params, obs, w = noisy_case(torch, g, B, M, nb, 3, td, rel=0.5)
    lut[777, 2] = float("nan")                                            # one row that is never accepted
    res, st = run(torch, eng, lut, params, obs, w, dtype, cut=float("inf"))
    assert st["brute_force"] == M, st
    assert res["count"].tolist() == [B - 1] * M
    args = [t.cpu().numpy() for t in (lut, params, obs, w)]
    want = defined.lut_bayes_defined(*args, cut=np.inf)
    assert np.array_equal(to_np(res)["best_idx"], want["best_idx"]) and np.array_equal(to_np(res)["count"], want["count"])
    check_values(to_np(res), want, defined.lut_bayes_exact(*args, cut=np.inf), np.inf, 1.0)
    zero = torch.zeros_like(w)
    obs[0, 1] = float("nan")                                              # (masked: allowed)
    res, st = run(torch, eng, lut, params, obs, zero, dtype, cut=0.0)
    assert st["brute_force"] == M, st
    rows = [r for r in range(B) if r != 777]
    mean, std = plain_sums(bf, params.cpu().numpy(), rows)
    got = to_np(res)
    for m in range(M):
        assert np.array_equal(got["mean"][m], mean) and np.array_equal(got["std"][m], std), m
    assert got["count"].tolist() == [B - 1] * M and got["sum_w"].tolist() == [float(B - 1)] * M
    assert got["ess"].tolist() == [float(B - 1)] * M and got["best_idx"].tolist() == [0] * M and (got["best_cost"] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 27, 64])
def test_hostile_inputs(torch_mod, eng, bf, P, dtype):
    """a NaN row, a row whose norm overflows, invalid observations between valid ones; B no multiple of the tile; P = 1 and 64"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    B, nb, M = 32 * 40 + 7, 6, 11
    g = torch.Generator(device="cuda:0").manual_seed(40 + P)
    lut, params, obs, w = noisy_case(torch, g, B, M, nb, P, td, rel=0.5)
    lut[5, 3] = float("nan")
    lut[B - 1, 0] = 1e30 if dtype == "float32" else 1e200                 # its centred norm overflows: rejected
    clean_w, clean_obs = w.clone(), obs.clone()
    w[2, 1] = -1.0                                                        # a negative weight
    w[4] = 0                                                              # every band masked: every accepted row, omega = 1
    obs[4] = float("nan")
    obs[6, 0] = float("inf")                                              # a non-finite value in a weighted band
    w[8, 5] = float("nan")
    res, st = run(torch, eng, lut, params, obs, w, dtype)
    got = to_np(res)
    for m in (2, 6, 8):                                                   # the empty-observation outputs
        assert got["count"][m] == 0 and got["best_idx"][m] == -1 and np.isinf(got["best_cost"][m]) and got["sum_w"][m] == 0
        assert np.isnan(got["ess"][m]) and np.isnan(got["mean"][m]).all() and np.isnan(got["std"][m]).all()
    rows = [r for r in range(B) if r not in (5, B - 1)]
    mean, std = plain_sums(bf, params.cpu().numpy(), rows)
    assert got["count"][4] == B - 2 and np.array_equal(got["mean"][4], mean) and np.array_equal(got["std"][4], std)
    good = torch.tensor([0, 1, 3, 5, 7, 9, 10], device="cuda:0")
    alone, _ = run(torch, eng, lut, params, clean_obs[good].contiguous(), clean_w[good].contiguous(), dtype)
    assert same(torch, res, alone, rows=good) is None                     # no neighbour's output changed
    row_ok = bf.norm_rule_numpy(lut.cpu().numpy(), np.full(nb, 0.5))
    assert row_ok.sum() == B - 2
    want = defined.lut_bayes_defined(lut.cpu().numpy(), params.cpu().numpy(), clean_obs[good].cpu().numpy(),
                                     clean_w[good].cpu().numpy(), row_ok=row_ok)
    assert np.array_equal(to_np(alone)["count"], want["count"]) and np.array_equal(to_np(alone)["best_idx"], want["best_idx"])
    assert 5 not in got["best_idx"] and B - 1 not in got["best_idx"]
    # only some outputs asked for: the others stay as they were, the ones written are the same
    rc, some, _ = bayes_call(torch, eng, lut, params, obs, w, dtype=dtype, outs=("mean", "count"))
    assert rc == 0 and same(torch, res, some, names=("mean", "count")) is None
    assert all(bool((some[n] == FILL).all()) for n in OUTS if n not in ("mean", "count"))


def test_refusals(torch_mod, eng):
    torch = torch_mod
    g = torch.Generator(device="cuda:0").manual_seed(1)
    lut, params, obs, w = noisy_case(torch, g, 500, 4, 7, 3, torch.float32)
    bad = [dict(dt=2), dict(dt=-1), dict(nb=0), dict(nb=2163), dict(P=0), dict(P=65), dict(B=-1), dict(M=-1),
           dict(B=2_000_000_001), dict(M=2_000_000_001), dict(null=("lut",)), dict(null=("params",)), dict(null=("obs",)),
           dict(null=("w",)), dict(null=("out",)), dict(opt=False), dict(outs=()), dict(cut=-1.0), dict(cut=float("nan")),
           dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(brute_force=2),
           dict(brute_force=-1)]
    for kw in bad:
        rc, res, _ = bayes_call(torch, eng, lut, params, obs, w, **kw)
        assert rc == INVALID, kw
        assert all(bool((t == FILL).all()) for t in res.values()), kw       # nothing was written
    rc, res, _ = bayes_call(torch, eng, lut, params, obs, w, ws_bytes=1000)
    assert rc == WORKSPACE and all(bool((t == FILL).all()) for t in res.values())
    # M = 0 launches nothing; B = 0 writes the empty-observation outputs
    rc, res, _ = bayes_call(torch, eng, lut, params, obs[:0], w[:0])
    assert rc == 0
    rc, res, _ = bayes_call(torch, eng, lut[:0], params[:0], obs, w)
    assert rc == 0
    assert res["count"].tolist() == [0] * 4 and res["best_idx"].tolist() == [-1] * 4 and res["sum_w"].tolist() == [0.0] * 4
    assert bool(torch.isinf(res["best_cost"]).all()) and bool(torch.isnan(res["mean"]).all()) and bool(torch.isnan(res["ess"]).all())


def test_engine_call(torch_mod, eng):
    """Engine.lut_bayes: None / (nb,) / (M, nb) weights are one C layout; the call is counted"""
    torch = torch_mod
    g = torch.Generator(device="cuda:0").manual_seed(2)
    lut, params, obs, w = noisy_case(torch, g, 1500, 9, 7, 3, torch.float32, rel=0.5)
    before = eng.calls["spart_lut_bayes"]
    a = eng.lut_bayes(lut, params, obs, cut=3.0)
    b, st = eng.lut_bayes(lut, params, obs, weights=torch.ones_like(obs), cut=3.0, stats=True)
    c = eng.lut_bayes(lut.cpu().numpy(), params.cpu().numpy(), obs.cpu().numpy(), weights=np.ones(7), cut=3.0)
    assert same(torch, a, b) is None and same(torch, a, c) is None and st["brute_force"] == 0
    assert eng.calls["spart_lut_bayes"] == before + 3
    raw, _ = run(torch, eng, lut, params, obs, w, "float32")
    assert same(torch, eng.lut_bayes(lut, params, obs, weights=w), raw) is None
    assert same(torch, eng.lut_bayes(lut, params, obs, weights=w, brute_force=True), raw) is None
    none = eng.lut_bayes(lut, params, obs[:0])                               # an empty batch: nothing launched
    assert none["mean"].shape == (0, 3) and none["count"].shape == (0,)
    empty, st = eng.lut_bayes(lut[:0], params[:0], obs, stats=True)          # an empty table: the empty-observation outputs
    assert empty["count"].tolist() == [0] * 9 and empty["best_idx"].tolist() == [-1] * 9 and st["brute_force"] == 0
    with pytest.raises(ValueError):
        eng.lut_bayes(lut, params[:-1], obs)
    with pytest.raises(ValueError):
        eng.lut_bayes(lut, params, obs, weights=np.ones(6))


def write_lut(path, lut, params, dtype):
    os.makedirs(path)
    np.save(os.path.join(path, "R_TOC.npy"), lut)
    np.save(os.path.join(path, "params.npy"), params)
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"sensor": "Sentinel2A-MSI", "dtype": dtype, "rows": int(lut.shape[0]), "columns": ["R_TOC"],
                   "band_model": "centre"}, f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_retrieve_and_retrieve_stream(torch_mod, eng, tmp_path, dtype):
    """bayes= maps = Engine.lut_bayes on the same tensors bit for bit (chunk sizes 1, 7, M); the other keys unchanged"""
    import spart_amd
    from spart_amd import workloads
    torch = torch_mod
    npdt = np.float32 if dtype == "float32" else np.float64
    rng = np.random.default_rng(6)
    B, nb, M = 700, 13, 23
    lut = rng.uniform(0.0, 0.6, (B, nb)).astype(npdt)
    params = rng.uniform(0.0, 8.0, (B, workloads.NPARAM))
    obs = (lut[rng.integers(0, B, M)] * (1 + 0.2 * rng.standard_normal((M, nb)))).astype(npdt)
    obs[3, 4] = np.nan                                                    # a masked band
    wts = spart_amd.noise_weights(obs, abs_sigma=0.01, rel_sigma=0.3)
    write_lut(str(tmp_path / "lut"), lut, params, dtype)
    cols = ["LAI", "Cab", "Cw"]
    ci = [workloads.PARAM_NAMES.index(n) for n in cols]
    opts = {"cut": 20.0, "temperature": 1.5}
    for weights in (wts, np.ones(nb)):
        o = obs if weights.ndim == 2 else np.nan_to_num(obs, nan=0.3)
        want = eng.lut_bayes(lut, params[:, ci], o, weights=torch.as_tensor(weights.astype(npdt)), dtype=dtype, **opts)
        for summary in ("host", "device"):
            plain = spart_amd.retrieve(str(tmp_path / "lut"), o, 5, weights=weights, summary=summary, params_cols=cols)
            got = spart_amd.retrieve(str(tmp_path / "lut"), o, 5, weights=weights, summary=summary, params_cols=cols, bayes=opts)
            for key, v in plain.items():
                assert key == "names" and got[key] == v or np.array_equal(got[key], v, equal_nan=True), (summary, key)
            for key, name in (("bayes_mean", "mean"), ("bayes_std", "std"), ("bayes_ess", "ess"), ("bayes_sum_w", "sum_w"),
                              ("bayes_count", "count")):
                assert np.array_equal(got[key], want[name].cpu().numpy(), equal_nan=True), (summary, key)
            assert got["bayes_count"].dtype == np.int64 and got["bayes_mean"].shape == (M, 3)
        plain = spart_amd.retrieve_stream(str(tmp_path / "lut"), o, 5, weights=weights, params_cols=cols)
        for chunk in (1, 7, M):
            got = spart_amd.retrieve_stream(str(tmp_path / "lut"), o, 5, weights=weights, params_cols=cols, chunk=chunk, bayes=opts)
            for key, v in plain.items():
                assert key == "names" and got[key] == v or np.array_equal(got[key], v, equal_nan=True), (chunk, key)
            for key, name in (("bayes_mean", "mean"), ("bayes_std", "std"), ("bayes_ess", "ess"), ("bayes_sum_w", "sum_w"),
                              ("bayes_count", "count")):
                assert np.array_equal(got[key], want[name].cpu().numpy(), equal_nan=True), (chunk, key)
    assert int(want["count"].max()) > 1
