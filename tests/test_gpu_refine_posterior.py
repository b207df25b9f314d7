"""spart_refine_posterior on the MI355X, bit for bit against the definition tools/refine_posterior_defined.py (all ten outputs
of the raw C call, np.array_equal with equal_nan; the definition's forward model is the engine's float64 pruned column path,
configured like the call; no tolerance anywhere), then Engine.posterior / jacobian / refine(posterior=True) and
retrieve / retrieve_stream(refine_opts={"posterior": True}).

Before any device call the definition alone must show that a case can fail.  A case of M >= 63 observations has more than half
of them at status 0 and at least one dead (-1: make_case plants an unmasked NaN observation and a NaN parameter in every case).
Status 1 needs a singular A in ONE row, which takes per-row weights: it is demanded wherever the case has per-observation band
weights and no shared prior (an all-zero weight row without a prior on it), and for R_TOC / R_TOA with a per-observation prior
(DOY, which only L_TOA knows of, as the last free column and no prior on it: the constant free column); the grid as a whole must show it for every
sensor and every F.  A case of one observation cannot show three statuses; it must be alive."""
import itertools

import numpy as np
import pytest

from helpers.lut_calls import hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import COLUMNS, FREE, S2, bounds_of, cols_of, forward_of
from helpers.refine_posterior_calls import (OUTS, POSTERIOR, assert_same, call, defined, make_posterior_case, posterior_call,
                                            retrieve_posterior_defined, same, untouched)
from helpers.refine_srf_calls import L8, raw_refine
from helpers.retrieve_defined import REFINED
from helpers.retrieve_defined import same as same_typed

pytestmark = pytest.mark.gpu

S3, HYPER = "Sentinel3A-OLCI", "hyper211"
KINDS = ("none", "shared", "per_observation")
PRIORS = ("none", "shared", "per_observation")
FS, MS = (1, 2, 6, 16), (1, 63, 65, 70)
SEEN = {}        # (sensor, F) -> the statuses the definition showed over the grid


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {S2: get_engine(S2, 0), S3: get_engine(S3, 0), HYPER: get_engine(None, 0, sensor_info=hyper_si), L8: get_engine(L8, 0)}


def grid():
    """sensor x F x M with the column, the weight form and the prior dealt round: every column, weight form and prior meets
    every sensor and F somewhere, and of the three cases of M >= 63 that a (sensor, F) has, one has per-observation weights
    without a shared prior (the all-zero weight row is then a singular A).  F = 16 always has a prior: 13 bands do not determine
    16 parameters"""
    combos = list(itertools.product(KINDS, PRIORS))
    plant = [("per_observation", "none"), ("per_observation", "per_observation")]
    rest = [c for c in combos if c not in plant]
    out = []
    for g, (sensor, F) in enumerate(itertools.product((S2, S3, HYPER), FS)):
        picks = [rest[(3 * g + j) % len(rest)] for j in range(3)]
        picks.insert(1 + g % 3, plant[1] if F == 16 else plant[g % 2])
        for j, (M, (kind, prior)) in enumerate(zip(MS, picks)):
            if F == 16 and prior == "none":
                prior = "shared" if kind == "per_observation" else "per_observation"
            out.append((sensor, F, M, (g + j) % 3, kind, prior))
    return out


def check_statuses(ref, M, kind, prior, what, constant=False):
    st = ref["status"]
    if M < 63:
        assert (st != -1).all(), (what, st)
        return
    assert (st == 0).mean() >= 0.5 and (st == -1).any(), (what, np.bincount(st + 1, minlength=3))
    assert st[3] == -1 and st[4] == -1 and st[0] != -1 and st[1] != -1
    if kind == "per_observation":
        assert st[5] == -1 and st[6] != -1 and ref["nband"][8] == 0
        assert st[8] == (1 if prior == "none" else 0) and st[2] == (0 if prior == "shared" else 1), (what, st[:10])
        if prior != "none":                                            # the prior alone: K = 0
            assert (ref["ak"][8] == 0).all() and ref["dfs"][8] == 0 and np.isfinite(ref["cov"][8]).all()
    if prior == "per_observation":
        assert st[7] == -1 and np.isfinite(ref["cost"][7])
        if constant:
            assert st[9] == 1 and (ref["jac"][9][:, -1] == 0).all() and np.isfinite(ref["jac"][9]).all()
    if (kind == "per_observation" and prior != "shared") or constant:
        assert (st == 1).any(), what
    one = st == 1
    assert np.isfinite(ref["jac"][one]).all() and np.isnan(ref["cov"][one]).all() and np.isnan(ref["jac"][st == -1]).all()


@pytest.mark.parametrize("sensor,F,M,column,kind,prior", grid())
def test_raw_call_against_the_definition(torch_mod, engines, sensor, F, M, column, kind, prior):
    eng = engines[sensor]
    what = (sensor, F, M, COLUMNS[column], kind, prior)
    constant = prior == "per_observation" and COLUMNS[column] != "L_TOA" and F >= 2 and M >= 63      # DOY as the last free column
    case = make_posterior_case(torch_mod, eng, FREE[F], M, COLUMNS[column], kind, prior, seed=1000 + 37 * F + M + column, constant=constant)
    ref = defined(torch_mod, eng, case, column)
    print(what, "statuses -1 / 0 / 1:", np.bincount(ref["status"] + 1, minlength=3))
    check_statuses(ref, M, kind, prior, what, constant)
    SEEN.setdefault((sensor, F), set()).update(int(s) for s in ref["status"])
    got = call(torch_mod, eng, case, column)
    assert_same(got, ref, what)
    ok = ref["status"] == 0
    assert same(got["cov"], np.swapaxes(got["cov"], 1, 2)) and same(got["std"][ok], np.sqrt(np.diagonal(got["cov"][ok], axis1=1, axis2=2)))


def test_the_grid_showed_every_status_for_every_sensor_and_f():
    assert len(SEEN) == 12, "run with the grid above"
    assert all(v == {-1, 0, 1} for v in SEEN.values()), SEEN
    used = {(c, k, p) for _, _, _, c, k, p in grid()}
    assert {c for c, _, _ in used} == {0, 1, 2} and {k for _, k, _ in used} == set(KINDS) and {p for _, _, p in used} == set(PRIORS)


def test_without_observations(torch_mod, engines):
    """obs = NULL: jac, y and everything derived from K equal the call's with obs; cost is the prior's term alone"""
    eng, F, M = engines[S2], 6, 70
    case = make_posterior_case(torch_mod, eng, FREE[F], M, "R_TOC", "per_observation", "per_observation", seed=5)
    base, free, lo, hi, obs, w, mean, weight = case
    with_obs, ref = defined(torch_mod, eng, case, 0), defined(torch_mod, eng, case, 0, with_obs=False)
    both = (with_obs["status"] == 0) & (ref["status"] == 0)
    assert both.sum() > M // 2 and ref["status"][3] == 0 and with_obs["status"][3] == -1      # the NaN observation: alive without obs
    want, _ = rd_prior_cost(case)
    assert same(ref["cost"], want) and (ref["cost"][both] > 0).all() and not same(ref["cost"], with_obs["cost"])
    got = call(torch_mod, eng, case, 0, with_obs=False)
    assert_same(got, ref, "obs = NULL")
    full = call(torch_mod, eng, case, 0)
    alive = with_obs["status"] != -1
    assert same(got["y"], full["y"]) and same(got["jac"][alive], full["jac"][alive]) and same(got["nband"], full["nband"])
    for k in ("cov", "ak", "std", "dfs"):
        assert same(got[k][both], full[k][both]), k
    # no observation, no prior, no weights: the cost is exactly 0
    rc, bare = posterior_call(torch_mod, eng, base, free, lo, hi, None)
    assert rc == 0 and (bare["cost"][bare["status"] != -1] == 0).all() and (bare["nband"] == 13).all()


def rd_prior_cost(case):
    from helpers.refine_calls import rd
    base, free, lo, hi, obs, w, mean, weight = case
    mu, p = rd.prior_defined(mean, weight, base.shape[0], len(free))
    return rd.prior_cost_defined(np.zeros(base.shape[0]), rd.clip_defined(base[:, free], lo, hi), mu, p)


def test_every_output_alone_gives_the_bits_of_the_full_call(torch_mod, engines):
    """each output requested alone (the other nine NULL): the same bits; posterior_call checks the guard elements behind every
    buffer and the guard bytes behind the workspace in each of the calls"""
    eng, F, M = engines[S2], 6, 70
    case = make_posterior_case(torch_mod, eng, FREE[F], M, "R_TOA", "per_observation", "per_observation", seed=6)
    full = call(torch_mod, eng, case, 1)
    assert set(full["status"]) == {-1, 0, 1}
    for k in OUTS:
        alone = call(torch_mod, eng, case, 1, outputs=(k,))
        assert list(alone) == [k] and same(alone[k], full[k]), k
    pair = call(torch_mod, eng, case, 1, outputs=("y", "jac"))
    assert same(pair["jac"], full["jac"]) and same(pair["y"], full["y"])


@pytest.mark.parametrize("sensor,column,kind,prior", [(S2, 0, "per_observation", "per_observation"), (S2, 1, "shared", "none"),
                                                     (L8, 2, "none", "shared"), (L8, 0, "per_observation", "none")])
def test_srf_band_model_against_the_definition(torch_mod, engines, sensor, column, kind, prior):
    eng, F, M = engines[sensor], 6, 65
    case = make_posterior_case(torch_mod, eng, FREE[F], M, COLUMNS[column], kind, prior, seed=70 + column, srf=True)
    ref = defined(torch_mod, eng, case, column, srf=True)
    check_statuses(ref, M, kind, prior, (sensor, column, kind, prior))
    got = call(torch_mod, eng, case, column, srf=True)
    assert_same(got, ref, (sensor, column, kind, prior))
    centre = call(torch_mod, eng, case, column)
    assert not same(centre["y"], got["y"]) and not same(centre["jac"], got["jac"])       # the band model is not ignored


@pytest.mark.parametrize("srf", (False, True))
@pytest.mark.parametrize("prior", ("none", "per_observation"))
def test_on_the_rows_a_fit_returned_std_y_and_cost_are_the_fits(torch_mod, engines, srf, prior):
    eng, F, M = engines[S2], 6, 70
    case = make_posterior_case(torch_mod, eng, FREE[F], M, "R_TOC", "per_observation", prior, seed=21, srf=srf)
    base, free, lo, hi, obs, w, mean, weight = case
    rc, fit = raw_refine(torch_mod, eng, "spart_refine_srf" if srf else "spart_refine", base, free, lo, hi, obs, w, mean, weight, column=0,
                         n_iter=3)
    assert rc == 0 and (fit["n_accept"] >= 1).sum() > M // 2 and (fit["n_accept"] == -1).any()
    rows = base.copy()
    rows[:, free] = fit["x"]
    got = call(torch_mod, eng, (rows, free, lo, hi, obs, w, mean, weight), 0, srf=srf)
    for k in ("x", "std", "y", "cost"):
        assert same(got[k], fit[k]), (k, srf, prior)
    assert ((got["status"] == -1) == (fit["n_accept"] == -1)).all() and np.isfinite(got["std"][got["status"] == 0]).all()


def test_the_chunk_cut(torch_mod, engines):
    """F = 16: observations go in chunks of (1 << 19) // 17 = 30 840.  Nine more, per-observation weights and prior, dead rows
    on both sides of the cut: jac's offsets (m nb F) and the prior rows of the second chunk"""
    eng, F, chunk = engines[S2], 16, (1 << 19) // 17
    M = chunk + 9
    case = make_posterior_case(torch_mod, eng, FREE[F], M, "R_TOA", "per_observation", "per_observation", seed=33)
    base, free, lo, hi, obs, w, mean, weight = case
    for p, s in {chunk - 2: 8, chunk - 1: 3, chunk: 5, chunk + 1: 7, chunk + 2: 2, chunk + 3: 0}.items():      # copies of planted rows
        base[p], obs[p], w[p], mean[p], weight[p] = base[s], obs[s], w[s], mean[s], weight[s]
    ref = defined(torch_mod, eng, case, 1)
    st = ref["status"]
    assert list(st[chunk - 2:chunk + 4]) == [0, -1, -1, -1, 1, st[0]] and st[0] != -1
    assert (st[chunk:] == 0).sum() >= 3 and (st == 0).mean() >= 0.5
    got = call(torch_mod, eng, case, 1)
    assert_same(got, ref, "chunk cut")
    assert not same(got["jac"][chunk + 4:], got["jac"][4:9])


def test_refusals_leave_every_output_untouched(torch_mod, engines):
    eng = engines[S2]
    names = FREE[2]
    free, (lo, hi) = cols_of(names), bounds_of(names)
    from spart_amd import get_engine, workloads
    base = workloads.lhs_params(8, "full", seed=3)
    obs, w2 = np.full((8, 13), 0.2), np.ones((8, 13))
    mu = np.zeros(2)
    INVALID, WORKSPACE, NOSENSOR = -1, -3, -4                         # include/spart_hip.h: SPART_ERR_*
    bare = get_engine(None, 0)
    cases = [(dict(ctx=None), INVALID), (dict(M=-1), INVALID), (dict(M=2000000001), INVALID), (dict(F=0), INVALID), (dict(F=17), INVALID),
             (dict(null=("base",)), INVALID), (dict(null=("free",)), INVALID), (dict(null=("lo",)), INVALID), (dict(null=("hi",)), INVALID),
             (dict(null=("opt",)), INVALID), (dict(null=("out",)), INVALID), (dict(column=3), INVALID), (dict(n_iter=101), INVALID),
             (dict(nlayers=-1), INVALID), (dict(rel_step=-1.0), INVALID), (dict(lambda0=float("inf")), INVALID), (dict(per_obs=2), INVALID),
             (dict(mean=mu), INVALID), (dict(weight=mu), INVALID), (dict(band_model=2), INVALID), (dict(band_model=-1), INVALID),
             (dict(outputs=()), INVALID), (dict(weights_per_obs=1), INVALID), (dict(null=("ws",)), WORKSPACE), (dict(ws_bytes=1024), WORKSPACE)]
    for kw, code in cases:
        kw = dict(kw)
        outputs = kw.pop("outputs", OUTS)
        rc, got = posterior_call(torch_mod, eng, base, free, lo, hi, obs, outputs=outputs, **kw)
        assert rc == code, (kw, rc, eng.lib.spart_last_error(eng.ctx))
        assert untouched(got), kw
    for bad in ([15, 15], [15, 27], [-1, 0]):
        rc, got = posterior_call(torch_mod, eng, base, bad, lo, hi, obs)
        assert rc == INVALID and untouched(got), bad
    for blo, bhi in ((hi, lo), (lo, lo), (np.array([np.nan, 0.0]), hi), (lo, np.array([1.0, np.inf]))):
        rc, got = posterior_call(torch_mod, eng, base, free, blo, bhi, obs)
        assert rc == INVALID and untouched(got)
    rc, got = posterior_call(torch_mod, bare, base, free, lo, hi, obs, nb=13, ws_bytes=1 << 20)
    assert rc == NOSENSOR and untouched(got)
    rc, got = posterior_call(torch_mod, eng, base[:0], free, lo, hi, obs[:0], w2[:0])                # M = 0 launches nothing
    assert rc == 0 and untouched(got)
    rc, got = posterior_call(torch_mod, eng, base, free, lo, hi, obs)                                # ... and the good call works
    assert rc == 0 and not untouched(got) and (got["status"] == 0).all()


def test_the_first_refusal_wins(torch_mod, engines):
    """calls with two faults: the one that is checked first is the one reported, and nothing is written"""
    from spart_amd import get_engine, workloads
    eng, bare = engines[S2], get_engine(None, 0)
    free, (lo, hi) = cols_of(FREE[2]), bounds_of(FREE[2])
    base, obs = workloads.lhs_params(8, "full", seed=3), np.full((8, 13), 0.2)
    for e, kw, text in [(eng, dict(F=17, null=("free",)), "F = 17, expected"),
                        (eng, dict(M=-1, F=0), "M = -1, expected"),
                        (eng, dict(band_model=2, n_iter=101), "n_iter = 101"),
                        (bare, dict(outputs=(), nb=13, ws_bytes=1 << 20), "every output is null")]:
        rc, got = posterior_call(torch_mod, e, base, free, lo, hi, obs, **kw)
        msg = e.lib.spart_last_error(e.ctx).decode()
        assert rc == -1 and msg.startswith(f"spart_refine_posterior: {text}"), (kw, rc, msg)
        assert untouched(got), kw
    rc, got = posterior_call(torch_mod, eng, base, free, lo, hi, None)                               # obs is optional here
    assert rc == 0 and not untouched(got) and (got["status"] == 0).all()


def test_engine_posterior_jacobian_and_refine(torch_mod, engines):
    import spart_amd
    eng, F, M = engines[S2], 6, 70
    names = FREE[F]
    case = make_posterior_case(torch_mod, eng, names, M, "R_TOC", "per_observation", "per_observation", seed=44)
    base, free, lo, hi, obs, w, mean, weight = case
    P = torch_mod.as_tensor(np.ascontiguousarray(base.T), device=eng.device)
    raw = call(torch_mod, eng, case, 0)
    n0 = eng.calls["spart_refine_posterior"]
    res = eng.posterior(P, obs, names, weights=w, prior_mean=mean, prior_weight=weight)
    assert eng.calls["spart_refine_posterior"] == n0 + 1 and res["names"] == names
    for k in OUTS:
        assert same(res[k].cpu().numpy(), raw[k]), k
    corr, ok = res["corr"].cpu().numpy(), raw["status"] == 0
    assert (np.diagonal(corr[ok], axis1=1, axis2=2) == 1.0).all() and np.isnan(corr[~ok]).all() and (np.abs(corr[ok]) <= 1.0 + 1e-12).all()
    off = ~np.eye(F, dtype=bool)
    with np.errstate(all="ignore"):
        assert same(corr[ok][:, off], (raw["cov"] / (raw["std"][:, :, None] * raw["std"][:, None, :]))[ok][:, off])
    # the dict prior and the host form give the same numbers
    host = spart_amd.posterior(base.T, obs, S2, names, weights=w, prior_mean=mean, prior_weight=weight)
    assert all(same(host[k], raw[k]) for k in OUTS) and same(host["corr"], corr)
    # jacobian: no observation, no weights, no prior
    rc, bare = posterior_call(torch_mod, eng, base, free, lo, hi, None)
    n0 = eng.calls["spart_refine_posterior"]
    jac = eng.jacobian(P, names)
    assert eng.calls["spart_refine_posterior"] == n0 + 1 and sorted(jac) == ["jac", "names", "y"]
    assert same(jac["jac"].cpu().numpy(), bare["jac"]) and same(jac["y"].cpu().numpy(), bare["y"])
    hj = spart_amd.jacobian(base.T, S2, names)
    assert same(hj["jac"], bare["jac"]) and same(hj["y"], bare["y"]) and hj["names"] == names
    # refine(posterior=True): the old keys keep their bits, one more call of each kind, the new keys are posterior()'s at the fitted rows
    kw = dict(weights=w, n_iter=3, prior_mean=mean, prior_weight=weight)
    plain = eng.refine(P, obs, names, **kw)
    before = dict(eng.calls)
    more = eng.refine(P, obs, names, posterior=True, **kw)
    assert eng.calls["spart_refine"] == before["spart_refine"] + 1 and eng.calls["spart_refine_posterior"] == before["spart_refine_posterior"] + 1
    assert sorted(more) == sorted(list(plain) + ["cov", "corr", "ak", "dfs"])
    for k in plain:
        assert more[k] == plain[k] if k == "names" else same(more[k].cpu().numpy(), plain[k].cpu().numpy()), k
    rows = base.copy()
    rows[:, free] = plain["x"].cpu().numpy()
    at = call(torch_mod, eng, (rows, free, lo, hi, obs, w, mean, weight), 0)
    assert same(at["std"], plain["std"].cpu().numpy()) and same(at["cost"], plain["cost"].cpu().numpy())
    for k in ("cov", "ak", "dfs"):
        assert same(more[k].cpu().numpy(), at[k]), k
    live = at["status"] == 0
    assert live.sum() > M // 2 and (np.diagonal(more["corr"].cpu().numpy()[live], axis1=1, axis2=2) == 1.0).all()
    assert ((at["dfs"][live] >= 0) & (at["dfs"][live] < F)).all() and at["dfs"][8] == 0      # (row 8: the prior alone)


# ---- retrieve / retrieve_stream
NAMES4 = ["LAI", "Cab", "Cw", "Cdm"]


@pytest.fixture(scope="module")
def lut(torch_mod, tmp_path_factory):
    import spart_amd
    from spart_amd import workloads
    P = workloads.lhs_params(4096, "full", seed=12)
    d = str(tmp_path_factory.mktemp("lut") / "lut")
    spart_amd.generate_lut(P, S2, path=d, dtype="float64")
    _, _, tabs = spart_amd.load_lut(d, mmap=False)
    return d, P, tabs


@pytest.mark.parametrize("weights,prior", [("per_observation", "knn"), ("shared", None), ("none", {"LAI": (3.0, 1.0), "Cab": (40.0, 15.0)})])
def test_retrieve_and_retrieve_stream_with_the_posterior(torch_mod, engines, lut, weights, prior):
    import spart_amd
    from spart_amd import workloads
    eng, (d, P, tabs) = engines[S2], lut
    M, K = 96, 5
    rng = np.random.default_rng(14)
    with np.errstate(all="ignore"):
        obs = forward_of(torch_mod, eng, "R_TOC")(workloads.lhs_params(M, "full", seed=13))
    obs = np.where(np.isfinite(obs), obs, 0.3) * (1.0 + 0.02 * rng.normal(size=obs.shape))
    w = None
    if weights == "shared":
        w = rng.uniform(0.5, 2.0, 13)
        w[4] = 0.0
    elif weights == "per_observation":
        w = spart_amd.noise_weights(obs, 1e-3, 0.02)
        obs[7] = np.nan                                                           # matches nothing
        obs[9, 3], w[9, 3] = np.nan, 0.0
        w[11, 0] = -1.0                                                           # matches nothing
    cols = cols_of(NAMES4)
    lo, hi = P[:, cols].min(axis=0), P[:, cols].max(axis=0)
    opts = {"n_iter": 3, "posterior": True}
    if prior is not None:
        opts["prior"] = prior
    ref = retrieve_posterior_defined(P, tabs["R_TOC"], obs, K, w, NAMES4, lo, hi, forward_of(torch_mod, eng, "R_TOC"), n_iter=3, prior=prior)
    matched = ref["idx"][:, 0] >= 0
    live = matched & np.isfinite(ref["refined_dfs"])
    assert live.mean() > 0.5 and np.isnan(ref["refined_cov"][~matched]).all() and np.isnan(ref["refined_dfs"][~matched]).all()
    assert (matched.all() if weights != "per_observation" else (not matched[7] and matched[9] and not matched[11]))
    if prior is not None:
        assert ((ref["refined_dfs"][live] > 0) & (ref["refined_dfs"][live] < 4)).all()
    kw = dict(column="R_TOC", weights=w, refine=NAMES4)
    got = spart_amd.retrieve(d, obs, K, summary="device", refine_opts=opts, **kw)
    for key in ("idx", "cost", "mean", "median", "std", "count") + REFINED + POSTERIOR:
        assert same_typed(got[key], ref[key]), ("device", key)
    plain = spart_amd.retrieve(d, obs, K, summary="device", refine_opts={k: v for k, v in opts.items() if k != "posterior"}, **kw)
    assert sorted(got) == sorted(list(plain) + list(POSTERIOR))
    for key in plain:
        assert got[key] == plain[key] if isinstance(plain[key], list) else same_typed(got[key], plain[key]), key
    host = spart_amd.retrieve(d, obs, K, summary="host", refine_opts=opts, **kw)
    for key in REFINED + POSTERIOR:
        assert same_typed(host[key], ref[key]), ("host", key)
    for chunk in (M, 64, 7, 1):
        res = spart_amd.retrieve_stream(d, obs, K, chunk=chunk, refine_opts=opts, **kw)
        assert sorted(res) == sorted(("mean", "median", "std", "count", "best_cost", "names", "refined_names") + REFINED + POSTERIOR)
        for key in ("mean", "median", "std", "count") + REFINED + POSTERIOR:
            assert same_typed(res[key], got[key]), ("stream", chunk, key)
