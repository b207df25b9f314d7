"""The Gaussian prior of spart_refine on the GPU: the raw C ABI against the definition tools/refine_defined.py, bit for bit, with
shared and per-observation priors; the per-observation prior across the host chunk loop; zero weights against no prior; the
refusals; Engine.refine's two forms of the prior; retrieve(refine_opts={"prior": "knn"}); retrieve_stream(refine=...) against
retrieve for several chunk sizes; and the twin experiment's exact properties."""
import numpy as np
import pytest

from helpers.lut_calls import torch_mod  # noqa: F401 (fixture)
from helpers.refine_calls import F16, FILL, FREE, OUTS, S2, cols_of, forward_of, make_case, rd, refine_call, same
from helpers.refine_prior_calls import check_prior_against_definition, make_prior, prior_call

pytestmark = pytest.mark.gpu
S3 = "Sentinel3A-OLCI"
REFINED = ("refined", "refined_std", "refined_cost", "refined_cost0", "refined_accepts")


@pytest.fixture(scope="module")
def engines(torch_mod):
    from spart_amd import get_engine
    return {S2: get_engine(S2, 0), S3: get_engine(S3, 0)}


@pytest.mark.parametrize("F", [1, 2, 6, 16])
@pytest.mark.parametrize("sensor", [S2, S3])
def test_definition_with_a_prior_bit_for_bit(torch_mod, engines, sensor, F):
    """M = 70: eight full groups of 8 (F <= 6) or seventeen of 4 (F = 16) and a partial one; 13 bands are one band tile, 21 two.
    Planted beside make_case's rows 0 ... 6 (per-observation prior): 10 a negative prior weight (dead), 11 a NaN mean under a
    zero weight (alive), 12 a NaN mean under a weight (dead), 13 (per-observation band weights) no band counts and a full prior"""
    eng = engines[sensor]
    assert eng.nb == (13 if sensor == S2 else 21)
    M, n_iter = 70, 3
    for per_obs, kind, column in ((False, "shared", 0), (True, "per_observation", 1 + F % 2)):
        seed = 1000 * F + 10 * eng.nb + per_obs
        case = make_case(torch_mod, eng, FREE[F], M, ("R_TOC", "R_TOA", "L_TOA")[column], kind, seed)
        base, free, lo, hi, obs, w = case
        mean, weight = make_prior(M, free, lo, hi, seed, per_obs)
        if per_obs:
            weight[10, F - 1], mean[10, F - 1] = -1.0, 0.5 * (lo + hi)[F - 1]
            weight[11, 0], mean[11, 0] = 0.0, np.nan
            weight[12, F // 2], mean[12, F // 2] = 1.0 / (0.1 * (hi - lo)[F // 2]) ** 2, np.nan
            w[13] = 0.0
            weight[13] = 1.0 / (0.1 * (hi - lo)) ** 2
            mean[13] = 0.5 * (lo + hi)
            mean[13, 0] = hi[0] + 0.2 * (hi[0] - lo[0])                          # one mean outside the box
            assert 0.05 < (weight == 0).mean() < 0.4 and np.isnan(mean[weight == 0]).all()
        elif F > 1:
            weight[F - 1], mean[F - 1] = 0.0, np.nan                             # the shared form of "no prior on that parameter"
        ref, _ = check_prior_against_definition(torch_mod, eng, case, mean, weight, column, n_iter, (sensor, F, kind))
        alive = ref["n_accept"] >= 0
        assert alive.mean() > 0.5 and (ref["n_accept"] >= 1).any() and (ref["cost"][alive] <= ref["cost0"][alive]).all()
        assert (ref["n_accept"][[3, 4]] == -1).all()
        if per_obs:
            assert (ref["n_accept"][[5, 10, 12]] == -1).all() and np.isnan(ref["std"][[10, 12]]).all()
            assert np.isfinite(ref["cost0"][10]) and np.isnan(ref["cost0"][12]) and ref["n_accept"][11] >= 0
            # no band counts: the cost is the prior's alone, so every accepted step is a step towards the prior mean
            assert ref["n_accept"][13] >= 1 and ref["cost"][13] < ref["cost0"][13] and np.isfinite(ref["std"][13]).all()
            assert not same(ref["x"][13], rd.clip_defined(base[13, free], lo, hi))
            assert ref["n_accept"][2] >= 0 and (ref["cost0"][2] > 0 or (weight[2] == 0).all())      # make_case's weightless row
        # the prior is not a no-op: without it the same case ends elsewhere
        plain = rd.refine_defined(base, free, lo, hi, obs, forward_of(torch_mod, eng, ("R_TOC", "R_TOA", "L_TOA")[column]), weights=w,
                                  n_iter=n_iter)
        assert not same(plain["x"], ref["x"]) and not same(plain["cost0"], ref["cost0"])


def test_per_observation_prior_across_the_chunk_loop(torch_mod, engines):
    """F = 16: chunks of (1 << 19) // 17 = 30 840 observations, so M = chunk + 9 runs a second chunk of nine, whose prior rows
    start at chunk * F"""
    eng = engines[S2]
    chunk = (1 << 19) // 17
    assert chunk == 30840
    M, n_iter = chunk + 9, 1
    base, free, lo, hi, obs, w = make_case(torch_mod, eng, F16, M, "R_TOC", "none", 21)
    mean, weight = make_prior(M, free, lo, hi, 21, True)
    rc, got = prior_call(torch_mod, eng, base, free, lo, hi, obs, None, mean, weight, n_iter=n_iter, guard=True)
    assert rc == 0
    for sl in (slice(chunk, M), slice(0, 8)):
        rc, part = prior_call(torch_mod, eng, base[sl], free, lo, hi, obs[sl], None, mean[sl], weight[sl], n_iter=n_iter, guard=True)
        assert rc == 0
        for k in OUTS:
            assert same(part[k], got[k][sl]), (sl, k)
        ref = rd.refine_defined(base[sl], free, lo, hi, obs[sl], forward_of(torch_mod, eng, "R_TOC"), n_iter=n_iter, prior_mean=mean[sl],
                                prior_weight=weight[sl])
        assert all(same(part[k], ref[k]) for k in OUTS)
        assert (ref["n_accept"] >= 0).mean() > 0.5 and (ref["n_accept"] >= 1).any()
        # (the rows' own priors matter: with the first rows' priors the tail would come out differently)
    wrong = rd.refine_defined(base[chunk:], free, lo, hi, obs[chunk:], forward_of(torch_mod, eng, "R_TOC"), n_iter=n_iter,
                              prior_mean=mean[:9], prior_weight=weight[:9])
    assert not same(wrong["cost0"], got["cost0"][chunk:])


def test_zero_prior_weights_are_the_no_prior_path(torch_mod, engines):
    eng = engines[S2]
    for F, kind in ((6, "per_observation"), (16, "shared")):
        base, free, lo, hi, obs, w = make_case(torch_mod, eng, FREE[F], 70, "R_TOC", kind, 31 + F)
        rc, none = prior_call(torch_mod, eng, base, free, lo, hi, obs, w, None, None, n_iter=3)
        assert rc == 0
        rc, old = refine_call(torch_mod, eng, base, free, lo, hi, obs, w, n_iter=3)      # (the caller that knows no prior)
        assert rc == 0 and all(same(none[k], old[k]) for k in OUTS)
        for shape in ((F,), (70, F)):
            rc, zero = prior_call(torch_mod, eng, base, free, lo, hi, obs, w, np.full(shape, np.nan), np.zeros(shape), n_iter=3)
            assert rc == 0
            for k in OUTS:
                assert same(zero[k], none[k]), (F, shape, k)
        assert (none["n_accept"] >= 1).any()


def test_prior_refusals_leave_outputs_and_guard_untouched(torch_mod, engines):
    eng = engines[S2]
    base, free, lo, hi, obs, w = make_case(torch_mod, eng, FREE[2], 65, "R_TOC", "shared", 3)
    mean, weight = make_prior(65, free, lo, hi, 3, True)
    for kw in (dict(mean=mean, weight=None), dict(mean=None, weight=weight), dict(mean=mean, weight=weight, per_obs=2),
               dict(mean=mean, weight=weight, per_obs=-1), dict(mean=None, weight=None, per_obs=2)):
        rc, got = prior_call(torch_mod, eng, base, free, lo, hi, obs, w, guard=True, **kw)
        assert rc == -1, (kw.keys(), rc)
        assert all((got[k] == FILL).all() for k in OUTS), kw.keys()
        assert b"prior" in eng.lib.spart_last_error(eng.ctx)


def test_engine_refine_takes_the_prior_as_a_dict_or_as_device_tensors(torch_mod, engines):
    import spart_amd
    eng = engines[S2]
    names, M = FREE[6], 70
    base, free, lo, hi, obs, w = make_case(torch_mod, eng, names, M, "R_TOC", "per_observation", 41)
    mean, weight = make_prior(M, free, lo, hi, 41, False)
    sigma = 0.1 * (hi - lo)
    per = mean[1] + 0.01 * np.arange(M)
    prior = {names[0]: (mean[0], sigma[0]), names[1]: (per, sigma[1]), names[3]: (mean[3], np.where(np.arange(M) % 5 == 0, np.inf, sigma[3])),
             names[5]: (mean[5], np.inf)}
    pm, pw = np.zeros((M, 6)), np.zeros((M, 6))
    pm[:, 0], pw[:, 0] = mean[0], 1.0 / (sigma[0] * sigma[0])
    pm[:, 1], pw[:, 1] = per, 1.0 / (sigma[1] * sigma[1])
    pm[:, 3], pw[:, 3] = mean[3], np.where(np.arange(M) % 5 == 0, 0.0, 1.0 / (sigma[3] * sigma[3]))
    pm[:, 5] = mean[5]
    rc, raw = prior_call(torch_mod, eng, base, free, lo, hi, obs, w, pm, pw, n_iter=3)
    assert rc == 0 and (raw["n_accept"] >= 1).any()
    P = torch_mod.as_tensor(np.ascontiguousarray(base.T), device=eng.device)
    by_dict = eng.refine(P, obs, names, weights=w, n_iter=3, prior=prior)
    by_tensor = eng.refine(P, obs, names, weights=w, n_iter=3, prior_mean=torch_mod.as_tensor(pm, device=eng.device),
                           prior_weight=torch_mod.as_tensor(pw, device=eng.device))
    host = spart_amd.refine(base.T, obs, S2, names, weights=w, n_iter=3, prior=prior)
    for k in OUTS:
        assert same(by_dict[k].cpu().numpy(), raw[k]) and same(by_tensor[k].cpu().numpy(), raw[k]) and same(host[k], raw[k]), k
    # scalars only: the shared (F,) form
    shared = {n: (mean[i], sigma[i]) for i, n in enumerate(names)}
    rc, raw = prior_call(torch_mod, eng, base, free, lo, hi, obs, w, mean, 1.0 / (sigma * sigma), n_iter=2)
    got = eng.refine(P, obs, names, weights=w, n_iter=2, prior=shared)
    assert rc == 0 and all(same(got[k].cpu().numpy(), raw[k]) for k in OUTS)
    plain = eng.refine(P, obs, names, weights=w, n_iter=2)
    assert not same(plain["x"].cpu().numpy(), raw["x"])


# ---- retrieve and retrieve_stream
NAMES4 = ["LAI", "Cab", "Cw", "Cdm"]


@pytest.fixture(scope="module")
def small_lut(torch_mod, tmp_path_factory):
    """4096 LHS rows, Sentinel-2A, float64; 200 observations: the model at other LHS rows with 2 % noise"""
    import spart_amd
    from spart_amd import workloads
    P = workloads.lhs_params(4096, "full", seed=12)
    d = str(tmp_path_factory.mktemp("prior_lut") / "lut")
    spart_amd.generate_lut(P, S2, path=d, dtype="float64")
    truth = workloads.lhs_params(200, "full", seed=13)
    obs = forward_of(torch_mod, spart_amd.get_engine(S2, 0), "R_TOC")(truth)
    obs = obs * (1.0 + 0.02 * np.random.default_rng(14).normal(size=obs.shape))
    return d, P, obs


def test_retrieve_with_the_knn_prior(torch_mod, small_lut):
    import spart_amd
    d, P, obs = small_lut
    obs = obs[:64]
    eng = spart_amd.get_engine(S2, 0)
    cols = cols_of(NAMES4)
    opts = {"n_iter": 3, "prior": "knn"}
    got = {s: spart_amd.retrieve(d, obs, 5, summary=s, refine=NAMES4, refine_opts=opts) for s in ("host", "device")}
    for s in ("host", "device"):
        plain = spart_amd.retrieve(d, obs, 5, summary=s)
        for k, v in plain.items():
            assert (got[s][k] == v) if k == "names" else same(got[s][k], v), (s, k)
        assert got[s]["refined_names"] == NAMES4
    for k in REFINED:
        assert same(got["host"][k], got["device"][k]), k
    # by hand: Engine.refine from params[idx[:, 0]] with knn_prior of the device summary of the free columns
    idx = got["device"]["idx"]
    assert (idx[:, 0] >= 0).all()
    lo, hi = P[:, cols].min(axis=0), P[:, cols].max(axis=0)
    near = eng.lut_summarise(np.ascontiguousarray(P[:, cols]), idx)
    pm, pw = spart_amd.knn_prior(near["mean"], near["std"], lo, hi)
    hm, hw = spart_amd.knn_prior(near["mean"].cpu().numpy(), near["std"].cpu().numpy(), lo, hi)
    assert same(pm.cpu().numpy(), hm) and same(pw.cpu().numpy(), hw) and (hw > 0).all()       # numpy and torch: the same bits
    r = eng.refine(list(np.ascontiguousarray(P[idx[:, 0]].T)), obs, NAMES4, bounds=dict(zip(NAMES4, zip(lo, hi))), n_iter=3,
                   prior_mean=pm, prior_weight=pw)
    for key, name in (("refined", "x"), ("refined_std", "std"), ("refined_cost", "cost"), ("refined_cost0", "cost0"),
                      ("refined_accepts", "n_accept")):
        assert same(got["device"][key], r[name].cpu().numpy()), key
    assert (got["device"]["refined_accepts"] >= 1).any() and np.isfinite(got["device"]["refined_std"]).all()
    # the prior and its floor are not no-ops, and a dict prior goes through as it is
    none = spart_amd.retrieve(d, obs, 5, refine=NAMES4, refine_opts={"n_iter": 3})
    wide = spart_amd.retrieve(d, obs, 5, refine=NAMES4, refine_opts={"n_iter": 3, "prior": "knn", "prior_floor": 0.5})
    assert not same(none["refined"], got["host"]["refined"]) and not same(wide["refined"], got["host"]["refined"])
    assert (got["host"]["refined_cost0"] >= none["refined_cost0"]).all()
    fixed = spart_amd.retrieve(d, obs, 5, refine=NAMES4, refine_opts={"n_iter": 3, "prior": {"LAI": (hm[:, 0], 1.0 / np.sqrt(hw[:, 0]))}})
    pm1, pw1 = np.zeros_like(hm), np.zeros_like(hw)
    sig = 1.0 / np.sqrt(hw[:, 0])
    pm1[:, 0], pw1[:, 0] = hm[:, 0], 1.0 / (sig * sig)
    r = eng.refine(list(np.ascontiguousarray(P[idx[:, 0]].T)), obs, NAMES4, bounds=dict(zip(NAMES4, zip(lo, hi))), n_iter=3,
                   prior_mean=pm1, prior_weight=pw1)
    assert same(fixed["refined"], r["x"].cpu().numpy()) and same(fixed["refined_std"], r["std"].cpu().numpy())


def test_retrieve_stream_refines_like_retrieve(torch_mod, small_lut):
    import spart_amd
    d, P, obs = small_lut
    obs = obs.copy()
    M = obs.shape[0]
    w = spart_amd.noise_weights(obs, abs_sigma=1e-3, rel_sigma=0.02)
    obs[7] = np.nan                                      # not masked: matches nothing
    obs[9, 3], w[9, 3] = np.nan, 0.0                     # masked: fine
    opts = {"n_iter": 2, "prior": "knn"}
    want = spart_amd.retrieve(d, obs, 5, weights=w, summary="device", refine=NAMES4, refine_opts=opts)
    assert want["idx"][7, 0] == -1 and want["refined_accepts"][7] == -1 and np.isnan(want["refined"][7]).all()
    assert (want["refined_accepts"] >= 1).any() and (np.delete(want["refined_accepts"], 7) >= 0).all()
    keys = {"mean", "median", "std", "count", "best_cost", "names"}
    out = None
    for chunk in (200, 64, 1):
        got = spart_amd.retrieve_stream(d, obs, 5, weights=w, chunk=chunk, refine=NAMES4, refine_opts=opts, out=out)
        assert set(got) == keys | set(REFINED) | {"refined_names"} and got["refined_names"] == NAMES4
        for k in ("mean", "median", "std", "count") + REFINED:
            assert same(got[k], want[k]), (chunk, k)
        assert same(got["best_cost"], want["cost"][:, 0]) and got["refined_accepts"].dtype == np.int32
        if out is not None:
            assert all(got[k] is out[k] for k in REFINED)
        out = {k: v for k, v in got.items() if isinstance(v, np.ndarray)}
        for v in out.values():
            v[...] = 0                                   # (the next call must write every row again)
    # a dict prior with per-observation means, cut with the chunks; shared weights
    prior = {"LAI": (np.linspace(0.5, 6.0, M), 1.0), "Cab": (40.0, np.where(np.arange(M) % 3 == 0, np.inf, 15.0))}
    opts = {"n_iter": 1, "prior": prior}
    ws = w[0].copy()
    want = spart_amd.retrieve(d, obs, 3, weights=ws, summary="device", refine=NAMES4, refine_opts=opts)
    got = spart_amd.retrieve_stream(d, obs, 3, weights=ws, chunk=77, refine=NAMES4, refine_opts=opts)
    for k in REFINED:
        assert same(got[k], want[k]), k
    # without refine: exactly the keys the call had before
    plain = spart_amd.retrieve_stream(d, obs, 5, weights=w, chunk=64)
    assert set(plain) == keys
    ref = spart_amd.retrieve(d, obs, 5, weights=w, summary="device")
    assert all(same(plain[k], ref[k]) for k in ("mean", "median", "std", "count")) and same(plain["best_cost"], ref["cost"][:, 0])


def test_twin_experiment_with_a_prior_on_the_truth(torch_mod, engines):
    """exact properties only: the cost never goes up, and the posterior spread is finite wherever the unregularised one is"""
    from spart_amd import workloads
    eng = engines[S2]
    names, M = FREE[6], 70
    base, free, lo, hi, obs, w = make_case(torch_mod, eng, names, M, "R_TOC", "none", 51)
    truth = workloads.lhs_params(M, "full", seed=51)[:, free]
    sigma = 0.1 * (hi - lo)
    P = torch_mod.as_tensor(np.ascontiguousarray(base.T), device=eng.device)
    plain = eng.refine(P, obs, names, n_iter=5)
    prior = eng.refine(P, obs, names, n_iter=5, prior={n: (truth[:, i], sigma[i]) for i, n in enumerate(names)})
    na, cost, cost0, std = (prior[k].cpu().numpy() for k in ("n_accept", "cost", "cost0", "std"))
    alive = na >= 0
    assert alive.mean() > 0.5 and (na >= 1).any() and (cost[alive] <= cost0[alive]).all()
    finite = np.isfinite(plain["std"].cpu().numpy())
    assert finite.any() and np.isfinite(std[finite]).all()
    assert np.array_equal(alive, plain["n_accept"].cpu().numpy() >= 0)
    print("twin with a prior: finite std without / with the prior:", int(finite.sum()), int(np.isfinite(std).sum()), "of", std.size)
