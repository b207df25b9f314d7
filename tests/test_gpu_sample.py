"""spart_sample on the GPU: the raw C ABI against the definition tools/sample_defined.py, bit for bit in all eleven outputs under
the margin condition, with the library's own float64 pruned column path (Engine.run on the rows the definition builds) as the
definition's forward model; guard words behind every buffer; the chunk cut at 2^19 / (W/2) observations; independence, resume
and seed identities; every output alone; the refusals; Engine.sample / spart_amd.sample against the raw call; the example; and
a plausibility check against refine().  If a mismatch shows here and not in tests/test_sample_host.py, the cause is in the
kernels' index maps, the LDS staging or the cross-lane steps, not in the arithmetic."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import COLUMNS, bounds_of, cols_of, make_case, same
from helpers.refine_srf_calls import L8
from helpers.sample_calls import OUTS, check_sample, differing, sample_call, sd, untouched

pytestmark = pytest.mark.gpu

S2, S3, HYPER = "Sentinel2A-MSI", "Sentinel3A-OLCI", "hyper211"
F16 = ["Cab", "Cdm", "Cw", "Cs", "Cca", "Cant", "N", "B", "SMp", "LAI", "LIDFa", "LIDFb", "q", "aot550", "uo3", "uh2o"]
FREE = {1: ["LAI"], 2: ["LAI", "Cab"], 3: ["LAI", "Cab", "Cw"], 6: ["LAI", "Cab", "Cw", "Cdm", "N", "LIDFa"], 16: F16}
WEIGHTS = ("none", "shared", "per_observation")
PRIORS = ("none", "shared", "per_observation")


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {S2: get_engine(S2, 0), S3: get_engine(S3, 0), HYPER: get_engine(None, 0, sensor_info=hyper_si), L8: get_engine(L8, 0)}


def grid():
    """F x W (W >= 2 F) x M with the sensor (13, 21, 211 bands), the column, the weight form and the prior dealt round, so that
    every column, weight form and prior meets every sensor somewhere; F = 16 always has a prior (13 bands do not hold 16
    parameters in place); the SRF band model on two sensors"""
    out = []
    cases = [(F, W, M) for F in (1, 2, 6, 16) for W in sd.WALKERS if W >= 2 * F for M in (1, 3, 65)]
    combos = list(itertools.product(WEIGHTS, PRIORS))
    for g, (F, W, M) in enumerate(cases):
        kind, prior = combos[(2 * g + g // 9) % 9]
        if M == 65 and g % 2 == 0:
            kind = "per_observation"                               # (the planted weight rows need per-observation weights)
        if F == 16 and prior == "none":
            prior = "shared"
        out.append(((S2, S3, HYPER)[g % 3], F, W, M, (g // 3) % 3, 0, kind, prior))
    out += [(S2, 2, 8, 3, 0, 1, "shared", "none"), (L8, 3, 16, 3, 1, 1, "none", "per_observation"), (S2, 1, 8, 65, 2, 1, "per_observation", "none")]
    return out


def sample_case(torch, eng, names, M, column, kind, prior, seed, srf=False):
    """refine_calls.make_case (at M = 65: row 0 a start outside the bounds, 1 a start on hi, 3 a NaN observation in a weighted
    band (dead), 4 a NaN fixed parameter (dead), and with per-observation weights 2 an all-zero weight row, 5 a negative band
    weight (dead), 6 a NaN observation under a zero weight (alive)) with a prior and a radius: row 7 an infinite prior weight
    (per-observation prior; dead), row 8 a zero radius (dead), row 9 a NaN radius (dead)"""
    rng = np.random.default_rng(seed + 77)
    base, free, lo, hi, obs, w = (make_case_srf if srf else make_case)(torch, eng, names, M, COLUMNS[column], kind, seed)
    F = len(free)
    kw = dict(weights=w)
    sigma = 0.25 * (hi - lo)
    if prior == "shared":
        kw.update(prior_mean=0.5 * (lo + hi), prior_weight=1.0 / sigma ** 2)
        kw["prior_weight"][F - 1] = 0.0
        kw["prior_mean"][F - 1] = np.nan
    elif prior == "per_observation":
        kw.update(prior_mean=base[:, free] + rng.uniform(-0.05, 0.05, (M, F)) * (hi - lo), prior_weight=np.tile(1.0 / sigma ** 2, (M, 1)))
        kw["prior_weight"][0, 0] = 0.0
    dead = []
    if M >= 63:
        radius = np.tile(0.02 * (hi - lo), (M, 1))
        radius[8, F - 1], radius[9, 0] = 0.0, np.nan
        kw["init_radius"] = radius
        dead = [3, 4, 8, 9]
        if kind == "per_observation":
            dead.append(5)
        if prior == "per_observation":
            kw["prior_weight"][7, F // 2] = np.inf
            dead.append(7)
    return (base, free, lo, hi, obs), kw, sorted(dead)


def make_case_srf(torch, eng, names, M, column, kind, seed):
    """make_case with the SRF column as the model behind obs"""
    from helpers.refine_srf_calls import srf_forward_of
    base, free, lo, hi, obs, w = make_case(torch, eng, names, M, column, kind, seed)
    rng = np.random.default_rng(seed + 5)
    with np.errstate(all="ignore"):
        y = srf_forward_of(torch, eng, column)(base)
    keep = np.isnan(obs)
    y = np.where(np.isfinite(y), y, 0.3) * (1.0 + 0.01 * rng.normal(size=y.shape))
    return base, free, lo, hi, np.where(keep, np.nan, y), w


@pytest.mark.parametrize("sensor,F,W,M,column,band_model,kind,prior", grid())
def test_raw_call_against_the_definition(torch_mod, engines, sensor, F, W, M, column, band_model, kind, prior):
    eng = engines[sensor]
    args, kw, dead = sample_case(torch_mod, eng, FREE[F], M, column, kind, prior, seed=100 * F + W + M, srf=bool(band_model))
    what = f"{sensor} F {F} W {W} M {M} column {column} band_model {band_model} weights {kind} prior {prior}"
    ref, got = check_sample(torch_mod, eng, *args, what=what, column=column, band_model=band_model, W=W, seed=F * 64 + W, step0=3,
                            obs_offset=(1 << 33) + 5, **kw)
    assert np.array_equal(np.flatnonzero(ref["status"] == -1), dead), (what, np.flatnonzero(ref["status"]), dead)
    live = ref["status"] == 0
    assert np.isfinite(ref["chain"][live]).all() and np.isnan(ref["mean"][~live]).all() and (ref["n_accept"][~live] == -1).all()
    assert ref["chain"].shape == (M, 2, W, F) and (ref["n_accept"][live] >= 0).all()
    assert ref["n_accepted"] > 0 and (M < 65 or (ref["n_rejected"] > 0 and ref["n_outside"] > 0)), what


def test_the_chunk_cut(torch_mod, engines):
    """W = 64: chunks of 2^19 / 32 = 16 384 observations, so observation 16 384 of 16 385 is alone in the second chunk; it is the
    same observation sampled alone with obs_offset = 16 384, and so is one in the middle of the first chunk"""
    eng = engines[S2]
    M, W = (1 << 19) // 32 + 1, 64
    from spart_amd import workloads
    base = workloads.lhs_params(M, "full", seed=9)
    free, (lo, hi) = cols_of(FREE[1]), bounds_of(FREE[1])
    rng = np.random.default_rng(1)
    obs = rng.uniform(0.02, 0.5, (M, eng.nb))
    kw = dict(W=W, n_steps=2, burn=0, thin=1, seed=11, weights=np.full(eng.nb, 50.0))
    rc, whole = sample_call(torch_mod, eng, base, free, lo, hi, obs, **kw)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    assert (whole["status"] == 0).mean() > 0.9
    for m in (M - 1, 7777):
        rc, alone = sample_call(torch_mod, eng, base[m:m + 1], free, lo, hi, obs[m:m + 1], obs_offset=m, **kw)
        assert rc == 0 and whole["status"][m] == 0 and not differing({k: v[0] for k, v in alone.items()}, {k: v[m] for k, v in whole.items()}), m
    need = lambda M_: int(eng.lib.spart_sample_workspace_bytes(eng.ctx, M_, 1, W))      # noqa: E731
    assert need(M) == need(M - 1) == need(2000000000) and 0 < need(1) < need(M)


@pytest.fixture(scope="module")
def plain(torch_mod, engines):
    """F = 3, W = 8, M = 5 on R_TOC of Sentinel-2A, per-observation weights: the case of the identity, NULL, Python and refusal
    tests -> (args, kw, ref)"""
    eng = engines[S2]
    args, kw, _ = sample_case(torch_mod, eng, FREE[3], 5, 0, "per_observation", "shared", seed=21)
    kw.update(W=8, seed=5, n_steps=6, burn=2, thin=2)
    ref, _ = check_sample(torch_mod, eng, *args, what="plain", **kw)
    return args, kw, ref


def test_independence_resume_and_seeds(torch_mod, engines, plain):
    eng = engines[S2]
    (base, free, lo, hi, obs), kw, ref = plain
    rows = lambda v, m: v[m:m + 1] if isinstance(v, np.ndarray) and v.ndim == 2 and v.shape[0] == 5 else v     # noqa: E731
    rc, alone = sample_call(torch_mod, eng, base[3:4], free, lo, hi, obs[3:4], **dict({k: rows(v, 3) for k, v in kw.items()}, obs_offset=3))
    assert rc == 0 and not differing({k: v[0] for k, v in alone.items()}, {k: v[3] for k, v in ref.items() if k in OUTS})
    # n = 6 is 3 + 3 with init = last and step0 = 3 (burn 0, thin 1: every step kept)
    every = dict(kw, burn=0, thin=1)
    rc, whole = sample_call(torch_mod, eng, base, free, lo, hi, obs, **every)
    rc1, first = sample_call(torch_mod, eng, base, free, lo, hi, obs, **dict(every, n_steps=3))
    rc2, rest = sample_call(torch_mod, eng, base, free, lo, hi, obs, **dict(every, n_steps=3, init=first["last"], step0=3))
    assert rc == rc1 == rc2 == 0
    assert same(rest["last"], whole["last"]) and same(rest["last_cost"], whole["last_cost"])
    assert same(first["chain"], whole["chain"][:, :3]) and same(rest["chain"], whole["chain"][:, 3:])
    assert same(rest["chain_cost"], whole["chain_cost"][:, 3:]) and np.array_equal(first["n_accept"] + rest["n_accept"], whole["n_accept"])
    # a given ensemble with a NaN and with a coordinate outside the box: dead, against the definition
    bad = first["last"].copy()
    bad[1, 7, 2], bad[2, 0, 0] = np.nan, hi[0] + 1.0
    ref3, got3 = check_sample(torch_mod, eng, base, free, lo, hi, obs, what="init", **dict(every, n_steps=3, init=bad, step0=3))
    assert np.array_equal(ref3["status"], [0, -1, -1, 0, 0])
    rc, again = sample_call(torch_mod, eng, base, free, lo, hi, obs, **kw)
    rc2, other = sample_call(torch_mod, eng, base, free, lo, hi, obs, **dict(kw, seed=6))
    assert rc == rc2 == 0 and not differing(again, ref) and not same(other["chain"], ref["chain"])


def test_every_output_alone(torch_mod, engines, plain):
    eng = engines[S2]
    (base, free, lo, hi, obs), kw, ref = plain
    for k in OUTS:
        rc, got = sample_call(torch_mod, eng, base, free, lo, hi, obs, outputs=(k,), **kw)
        assert rc == 0 and list(got) == [k] and not differing(got, ref, keys=(k,)), k


def test_refusals_leave_the_outputs_untouched(torch_mod, engines, plain):
    from spart_amd import get_engine
    eng = engines[S2]
    (base, free, lo, hi, obs), kw, _ = plain
    need = int(eng.lib.spart_sample_workspace_bytes(eng.ctx, 5, 3, 8))
    cases = ((dict(ctx=get_engine(None, 0).ctx), -4, "no sensor"), (dict(ws_bytes=need - 1), -3, f"{need} bytes needed"),
             (dict(null=("ws",)), -3, "bytes needed"), (dict(F=0), -1, "F = 0"), (dict(F=17), -1, "F = 17"), (dict(null=("free",)), -1, "null"),
             (dict(column=3), -1, "column = 3"), (dict(nlayers=-1), -1, "nlayers"), (dict(prior_per_obs=2), -1, "prior_per_obs"),
             (dict(prior_weight=None), -1, "come together"), (dict(band_model=2), -1, "band_model = 2"), (dict(W=12), -1, "W = 12"),
             (dict(W=4), -1, "W = 4"), (dict(n_steps=0), -1, "n_steps = 0"), (dict(n_steps=(1 << 20) + 1), -1, "n_steps"),
             (dict(burn=6), -1, "burn = 6"), (dict(thin=0), -1, "thin = 0"), (dict(burn=4, thin=3), -1, "thin = 3"), (dict(a=1.0), -1, "a must"),
             (dict(a=np.nan), -1, "a must"), (dict(temperature=-1.0), -1, "temperature"), (dict(rel_init=np.inf), -1, "rel_init"),
             (dict(step0=-1), -1, "step0"), (dict(obs_offset=-2), -1, "obs_offset"), (dict(M=-1), -1, "M = -1"),
             (dict(null=("opt",)), -1, "W = 0"), (dict(null=("out",)), -1, "out is null"), (dict(null=("base",)), -1, "base is null"),
             (dict(null=("base[26]",)), -1, "base[26] is null"), (dict(null=("obs",)), -1, "obs is null"),
             (dict(weights=None, weights_per_obs=1), -1, "weights_per_obs"), (dict(outputs=()), -1, "every output is null"))
    for over, code, text in cases:
        args = dict(kw, **over)
        rc, got = sample_call(torch_mod, eng, base, free, lo, hi, obs, **args)
        assert rc == code and text in eng.lib.spart_last_error(eng.ctx).decode(), (over, rc, eng.lib.spart_last_error(eng.ctx))
        assert untouched(got), over
    # the order: band_model before W before n_steps before a before temperature before rel_init before step0 before M
    order = (("band_model", 2, "band_model"), ("W", 12, "W = 12"), ("n_steps", 0, "n_steps"), ("a", 0.5, "a must"),
             ("temperature", -1.0, "temperature"), ("rel_init", -1.0, "rel_init"), ("step0", -1, "step0"), ("M", -1, "M = -1"))
    for i in range(len(order)):
        rc, got = sample_call(torch_mod, eng, base, free, lo, hi, obs, **dict(kw, **{k: v for k, v, _ in order[i:]}))
        assert rc == -1 and order[i][2] in eng.lib.spart_last_error(eng.ctx).decode() and untouched(got), order[i]
    rc, got = sample_call(torch_mod, eng, base, free, lo, hi, obs, **dict(kw, M=0))
    assert rc == 0 and untouched(got)
    for sizes in ((0, 3, 8), (5, 0, 8), (5, 17, 64), (5, 3, 4), (5, 3, 12), (5, 5, 8), (2000000001, 3, 8)):
        assert eng.lib.spart_sample_workspace_bytes(eng.ctx, *sizes) == 0, sizes
    assert eng.lib.spart_sample_workspace_bytes(get_engine(None, 0).ctx, 5, 3, 8) == 0


def test_engine_and_host_forms_are_the_raw_call(torch_mod, engines, plain):
    import spart_amd
    eng = engines[S2]
    (base, free, lo, hi, obs), kw, ref = plain
    names = FREE[3]
    opts = dict(weights=kw["weights"], prior_mean=kw["prior_mean"], prior_weight=kw["prior_weight"], walkers=8, n_steps=6, burn=2, thin=2,
                seed=5, chain=True)
    want = {"mean": "mean", "std": "std", "cov": "cov", "best": "best_x", "best_cost": "best_cost", "status": "status", "last": "last",
            "last_cost": "last_cost", "chain": "chain", "chain_cost": "chain_cost"}
    res = eng.sample(torch_mod.as_tensor(base.T.copy(), device=eng.device), obs, names, **opts)
    host = spart_amd.sample(base.T, obs, S2, names, **opts)
    for r in ({k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}, host):
        assert r["names"] == names and all(same(r[k], ref[v]) for k, v in want.items()), [k for k, v in want.items() if not same(r[k], ref[v])]
        assert np.abs(r["accept_fraction"] - ref["n_accept"] / (8 * 6.0)).max() <= 2.0 ** -52      # (a division on the device)
    # defaults: the smallest W >= 2 F, burn = n_steps // 2, no chain; a scalar row broadcasts
    d = spart_amd.sample([np.float64(v) for v in base[0]], obs[:1], S2, names, n_steps=4, weights=kw["weights"][:1])
    assert "chain" not in d and d["last"].shape == (1, 8, 3) and d["status"][0] == 0
    rc, raw = sample_call(torch_mod, eng, base[:1], free, lo, hi, obs[:1], weights=kw["weights"][:1], W=8, n_steps=4, burn=2, thin=1, a=2.0,
                          temperature=1.0, rel_init=0.01)
    assert rc == 0 and same(d["mean"], raw["mean"]) and same(d["last"], raw["last"])


@pytest.mark.parametrize("lidf,nlayers", [("newton", None), ("literal", 1), ("literal", 30), ("newton", 30)])
def test_options_reach_the_forward_model(torch_mod, engines, plain, lidf, nlayers):
    """fast_prelude and nlayers: the raw call is the definition under the same options and not the default's, both together are
    neither alone, and Engine.sample / spart_amd.sample hand lidf and nlayers on.  What carries the forward model in these
    6 steps is the costs (chain_cost, last_cost, best_cost): a walker's position is a function of the random numbers and the
    accept decisions alone, and no decision of the plain case flips under any of the four options (accepted 191, rejected 41,
    outside 8 in each, as under the defaults), so chain has the default's bits (measured; the test prints which outputs
    differ)."""
    import spart_amd
    eng = engines[S2]
    (base, free, lo, hi, obs), kw, default = plain
    raw = dict(fast_prelude=1 if lidf == "newton" else 0, nlayers=nlayers or 0)
    ref, got = check_sample(torch_mod, eng, base, free, lo, hi, obs, what=f"plain, lidf {lidf} nlayers {nlayers}", **kw, **raw)
    moved = [k for k in OUTS if not same(got[k], default[k])]
    print(f"spart_sample plain, lidf {lidf} nlayers {nlayers}: outputs that differ from the default's: {moved}")
    assert all(not same(got[k], default[k]) for k in ("chain_cost", "last_cost", "best_cost")), (lidf, nlayers, moved)
    assert np.array_equal(ref["status"], default["status"]) and (ref["status"] == 0).any()
    if lidf == "newton" and nlayers == 30:
        for only in (dict(nlayers=30), dict(fast_prelude=1)):
            rc, one = sample_call(torch_mod, eng, base, free, lo, hi, obs, **kw, **only)
            assert rc == 0 and not same(got["chain_cost"], one["chain_cost"]) and not same(got["last_cost"], one["last_cost"]), only
    names = FREE[3]
    opts = dict(weights=kw["weights"], prior_mean=kw["prior_mean"], prior_weight=kw["prior_weight"], walkers=8, n_steps=6, burn=2, thin=2,
                seed=5, chain=True, lidf=lidf, nlayers=nlayers)
    want = {"mean": "mean", "std": "std", "cov": "cov", "best": "best_x", "best_cost": "best_cost", "status": "status", "last": "last",
            "last_cost": "last_cost", "chain": "chain", "chain_cost": "chain_cost"}
    res = eng.sample(torch_mod.as_tensor(base.T.copy(), device=eng.device), obs, names, **opts)
    host = spart_amd.sample(base.T, obs, S2, names, **opts)
    for r in ({k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}, host):
        assert r["names"] == names and all(same(r[k], got[v]) for k, v in want.items()), [k for k, v in want.items() if not same(r[k], got[v])]


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sample.py"), "120"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "dense canopy" in r.stdout and "sparse canopy" in r.stdout and r.stdout.count(" +- ") == 8 and "the bound is 7" in r.stdout


def test_plausible_against_refine(torch_mod, engines):
    """16 synthetic Sentinel-2A observations, 2 % noise, LAI and Cab free, W = 16, 400 steps, burn 200: every observation lives,
    the acceptance fraction is neither 0 nor 1, and on the 12 sparse canopies (LAI <= 3) the sampled mean lies within 5 of
    refine's linearised sigma of refine's point.  Measured: see DESIGN.md 19 (the figures this test prints)."""
    from spart_amd import workloads
    eng = engines[S2]
    names = FREE[2]
    truth = np.repeat(workloads.default_row(), 16, axis=0)
    truth[:, workloads.PARAM_NAMES.index("LAI")] = np.concatenate([np.linspace(0.5, 3.0, 12), np.linspace(5.5, 6.8, 4)])
    truth[:, workloads.PARAM_NAMES.index("Cab")] = np.tile([25.0, 40.0, 55.0, 65.0], 4)
    rng = np.random.default_rng(4)
    clean = eng.run(torch_mod.as_tensor(truth.T.copy(), device=eng.device), "float64", prune=True)["R_TOC"].cpu().numpy()
    sigma = 0.02 * np.maximum(clean, 0.01)
    obs, w = clean + sigma * rng.normal(size=clean.shape), 1.0 / sigma ** 2
    start = truth.copy()
    start[:, cols_of(names)] *= 1.2
    fit = eng.refine(torch_mod.as_tensor(start.T.copy(), device=eng.device), obs, names, weights=w, n_iter=15)
    x, std = fit["x"].cpu().numpy(), fit["std"].cpu().numpy()
    rows = start.copy()
    rows[:, cols_of(names)] = x
    res = eng.sample(torch_mod.as_tensor(rows.T.copy(), device=eng.device), obs, names, weights=w, walkers=16, n_steps=400, burn=200, seed=3)
    mean, acc, status = res["mean"].cpu().numpy(), res["accept_fraction"].cpu().numpy(), res["status"].cpu().numpy()
    dev = np.abs(mean - x) / std
    print("acceptance fraction", np.round(acc, 3))
    print("|mean - refined x| / refined std (LAI, Cab), sparse:", np.round(dev[:12], 2).tolist(), "dense:", np.round(dev[12:], 2).tolist())
    print("sampled std / refined std, sparse:", np.round((res["std"].cpu().numpy() / std)[:12], 2).tolist())
    assert (status == 0).all() and ((acc > 0.05) & (acc < 0.95)).all()
    assert (dev[:12] <= 5.0).all()
