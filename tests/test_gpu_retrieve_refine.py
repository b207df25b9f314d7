"""retrieve(refine=...) and retrieve_stream(refine=...) end to end on the MI355X against tests/helpers/retrieve_defined.py -- the
search, the summary, the "knn" prior and the fit composed in numpy of their four definitions -- bit for bit, through three
callers: retrieve(summary="device"), retrieve(summary="host") and retrieve_stream in chunks of M, 64, 7 and 1.  The cases are the
configurations the join in spart_amd/lut.py had never run in: float32 LUTs (whose chunks go up a second time as float64), the
columns R_TOA and L_TOA, a 21-band and a custom 211-band sensor, the options handed through, and the edges of the join."""
import json
import os

import numpy as np
import pytest

from helpers.lut_calls import hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import S2, cols_of, forward_of
from helpers.retrieve_defined import REFINED, retrieve_defined, same

pytestmark = pytest.mark.gpu
S3, HYPER = "Sentinel3A-OLCI", "hyper211"
NAMES4 = ["LAI", "Cab", "Cw", "Cdm"]
K, M = 5, 96
SEARCHED = ("idx", "cost", "mean", "median", "std", "count")
MAPS = ("mean", "median", "std", "count")
WEIGHTS = ("none", "shared", "per_observation")


@pytest.fixture(scope="module")
def engine_of(torch_mod, hyper_si):
    from spart_amd import get_engine
    return lambda sensor: get_engine(sensor, 0, sensor_info=hyper_si) if sensor == HYPER else get_engine(sensor, 0)


@pytest.fixture(scope="module")
def luts(torch_mod, tmp_path_factory, hyper_si):
    """luts(sensor, dtype) -> (directory, params, {column: table}, sensor_info or None): 4096 LHS rows written by generate_lut,
    once per module; ``rows``: only the first so many of them; ``const``: {name: value} columns made constant"""
    import spart_amd
    from spart_amd import workloads
    made = {}

    def get(sensor, dtype, rows=4096, const=()):
        key = (sensor, dtype, rows, tuple(dict(const).items()))
        if key not in made:
            P = workloads.lhs_params(4096, "full", seed=12)[:rows].copy()
            for n, v in dict(const).items():
                P[:, workloads.PARAM_NAMES.index(n)] = v
            d = str(tmp_path_factory.mktemp("lut") / "lut")
            si = hyper_si if sensor == HYPER else None
            spart_amd.generate_lut(P, sensor, path=d, dtype=dtype, **({"sensor_info": si} if si is not None else {}))
            _, _, tabs = spart_amd.load_lut(d, mmap=False)
            assert all(t.dtype == np.dtype(dtype) and t.shape[0] == rows for t in tabs.values())
            made[key] = (d, P, tabs, si)
        return made[key]
    return get


def scene(torch, eng, column, weights, m=M, seed=13, all_nan=False):
    """m observations: the model at LHS rows that are not the LUT's, 2 % noise.  weights: "none", "shared" ((nb,), one band of
    weight 0) or "per_observation" (noise_weights(obs, 1e-3, 0.02)) with planted rows: 7 an unmasked NaN observation (matches
    nothing), 9 a NaN under a zero weight (fine), 11 a negative weight (matches nothing) -> (obs, weights)"""
    import spart_amd
    from spart_amd import workloads
    rng = np.random.default_rng(seed + 1)
    with np.errstate(all="ignore"):
        obs = forward_of(torch, eng, column)(workloads.lhs_params(m, "full", seed=seed))
    obs = np.where(np.isfinite(obs), obs, 0.3) * (1.0 + 0.02 * rng.normal(size=obs.shape))
    nb = obs.shape[1]
    w = None
    if weights == "shared":
        w = rng.uniform(0.5, 2.0, nb)
        w[nb // 3] = 0.0
    elif weights == "per_observation":
        w = spart_amd.noise_weights(obs, 1e-3, 0.02)
        obs[7] = np.nan
        obs[9, 3], w[9, 3] = np.nan, 0.0
        w[11, 0] = -1.0
    if all_nan:
        obs[...] = np.nan
    return obs, w


def check(torch, lut, eng, obs, w, column="R_TOC", k=K, names=NAMES4, opts=None, params_cols=None, callers=("device", "host", "stream"),
          chunks=None, vacuous=False):
    """One case through the callers, every array against the definition bit for bit -> (the definition's arrays, the device
    caller's).  Before any call the definition alone must show that the case can fail: among the matched observations more
    than half alive, an accepted step, a fit that moved; and on a float32 LUT other bits in ``refined`` when obs (and, where
    they are given, the weights) are rounded to float32 first -- which is what a lost float64 upload would compute."""
    import spart_amd
    from spart_amd import workloads
    d, P, tabs, si = lut
    table = tabs[column]
    opts = dict(opts or {})
    cols = cols_of(names)
    lo, hi = (P[:, cols].min(axis=0), P[:, cols].max(axis=0)) if P.shape[0] else (np.full(len(names), np.nan), np.full(len(names), np.nan))
    for n, (a, b) in (opts.get("bounds") or {}).items():
        lo[names.index(n)], hi[names.index(n)] = a, b
    fit = dict(n_iter=opts.get("n_iter", 10), rel_step=opts.get("rel_step", 1e-3), lambda0=opts.get("lambda0", 1e-2),
               prior=opts.get("prior"), prior_floor=opts.get("prior_floor", 0.05), params_cols=params_cols,
               torch_device="cuda:0" if table.shape[1] > 31 else None)
    fwd = forward_of(torch, eng, column, lidf=opts.get("lidf", "literal"), nlayers=opts.get("nlayers"))
    ref = retrieve_defined(P, table, obs, k, w, names, lo, hi, fwd, **fit)
    m = obs.shape[0]
    matched = ref["idx"][:, 0] >= 0
    assert (ref["refined_accepts"][~matched] == -1).all() and np.isnan(ref["refined"][~matched]).all()
    if not vacuous:
        acc = ref["refined_accepts"][matched]
        assert matched.mean() > 0.9 and (acc >= 0).mean() > 0.5 and (acc >= 1).any(), (matched.mean(), (acc >= 0).mean(), int((acc >= 1).sum()))
        assert not same(ref["refined"], ref["start"])
        if w is not None and np.ndim(w) == 2:
            assert not matched[7] and matched[9] and not matched[11]
        if table.dtype == np.float32:
            rounded = retrieve_defined(P, table, obs.astype(np.float32), k, w, names, lo, hi, fwd, **fit)
            assert same(rounded["idx"], ref["idx"]) and not same(rounded["refined"], ref["refined"])
            if w is not None:
                rounded = retrieve_defined(P, table, obs, k, w.astype(np.float32), names, lo, hi, fwd, **fit)
                assert same(rounded["idx"], ref["idx"]) and not same(rounded["refined"], ref["refined"])
    kw = dict(column=column, weights=w, params_cols=params_cols, refine=names, refine_opts=opts)
    if si is not None:
        kw["sensor_info"] = si
    summary_names = list(workloads.PARAM_NAMES) if params_cols is None else list(params_cols)
    got = None
    if "device" in callers:
        got = spart_amd.retrieve(d, obs, k, summary="device", **kw)
        for key in SEARCHED + REFINED:
            assert same(got[key], ref[key]), ("device", key)
        assert got["names"] == summary_names and got["refined_names"] == names
    if "host" in callers:
        host = spart_amd.retrieve(d, obs, k, summary="host", **kw)
        for key in ("idx", "cost", "median") + REFINED:
            assert same(host[key], ref[key]), ("host", key)
        plain = spart_amd.retrieve(d, obs, k, summary="host", column=column, weights=w, params_cols=params_cols)
        assert same(host["mean"], plain["mean"]) and same(host["std"], plain["std"]) and "count" not in host
        assert host["names"] == summary_names and host["refined_names"] == names
    if "stream" in callers:
        for chunk in (m, 64, 7, 1) if chunks is None else chunks:
            res = spart_amd.retrieve_stream(d, obs, k, chunk=chunk, **kw)
            assert sorted(res) == sorted(MAPS + REFINED + ("best_cost", "names", "refined_names"))
            for key in MAPS + REFINED:
                assert same(res[key], ref[key]), ("stream", chunk, key)
            assert same(res["best_cost"], ref["cost"][:, 0]), ("stream", chunk)
            assert res["names"] == summary_names and res["refined_names"] == names
    return ref, got


# ---- A. Sentinel-2A, a float32 LUT: every weight form with every prior
def prior_of(kind, lut):
    if kind != "dict":
        return kind
    lai = lut[1][:, cols_of(["LAI"])[0]]
    return {"LAI": (np.linspace(lai.min(), lai.max(), M), 1.0), "Cab": (40.0, np.inf)}


@pytest.mark.parametrize("prior", [None, "knn", "dict"])
@pytest.mark.parametrize("weights", WEIGHTS)
def test_float32_lut_every_weight_form_and_prior(torch_mod, luts, engine_of, weights, prior):
    lut, eng = luts(S2, "float32"), engine_of(S2)
    obs, w = scene(torch_mod, eng, "R_TOC", weights)
    opts = {"n_iter": 2}
    if prior is not None:
        opts["prior"] = prior_of(prior, lut)
    ref, got = check(torch_mod, lut, eng, obs, w, opts=opts, params_cols=["LAI"] if (weights, prior) == ("shared", "knn") else None)
    assert got["cost"].dtype == np.float32 and got["mean"].shape == (M, 1 if (weights, prior) == ("shared", "knn") else 27)
    if prior is not None:                                           # the prior is not a no-op
        plain = retrieve_defined(lut[1], lut[2]["R_TOC"], obs, K, w, NAMES4, *bounds_of_lut(lut), forward_of(torch_mod, eng, "R_TOC"), n_iter=2)
        assert same(plain["idx"], ref["idx"]) and not same(plain["refined"], ref["refined"])


def bounds_of_lut(lut, names=NAMES4):
    P = lut[1]
    return P[:, cols_of(names)].min(axis=0), P[:, cols_of(names)].max(axis=0)


# ---- B. the columns: the plan is made for R_TOC and re-indexed by both callers
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("column", ["R_TOA", "L_TOA"])
def test_columns_r_toa_and_l_toa(torch_mod, luts, engine_of, column, dtype):
    lut, eng = luts(S2, dtype), engine_of(S2)
    obs, w = scene(torch_mod, eng, column, "shared")
    ref, got = check(torch_mod, lut, eng, obs, w, column=column, opts={"n_iter": 2})
    other = retrieve_defined(lut[1], lut[2]["R_TOC"], obs, K, w, NAMES4, *bounds_of_lut(lut), forward_of(torch_mod, eng, "R_TOC"), n_iter=2)
    assert not same(other["idx"], ref["idx"]) and not same(other["refined_cost0"], ref["refined_cost0"])    # (the column matters)


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("column", ["R_TOC", "R_TOA", "L_TOA"])
def test_float64_lut_cost_at_the_start_is_the_search_cost(torch_mod, luts, engine_of, column, weights):
    """retrieve's docstring: refined_cost0 == cost[:, 0] of a float64 LUT bit for bit -- for every column and weight form, in
    the definition and in both callers (the stream's best_cost is cost[:, 0])"""
    import spart_amd
    lut, eng = luts(S2, "float64"), engine_of(S2)
    obs, w = scene(torch_mod, eng, column, weights)
    ref, got = check(torch_mod, lut, eng, obs, w, column=column, opts={"n_iter": 1}, callers=("device",))
    ok = ref["idx"][:, 0] >= 0
    assert ok.sum() >= M - 2 and ref["cost"].dtype == np.float64
    assert same(ref["refined_cost0"][ok], ref["cost"][ok, 0]) and same(got["refined_cost0"][ok], got["cost"][ok, 0])
    res = spart_amd.retrieve_stream(lut[0], obs, K, column=column, weights=w, chunk=40, refine=NAMES4, refine_opts={"n_iter": 1})
    assert same(res["refined_cost0"][ok], res["best_cost"][ok]) and same(res["refined_cost0"], ref["refined_cost0"])
    assert np.isnan(res["refined_cost0"][~ok]).all() and np.isinf(res["best_cost"][~ok]).all()


# ---- C. 21 bands: two band tiles of the fit behind the narrow search
def test_olci_two_band_tiles_float32_knn(torch_mod, luts, engine_of):
    lut, eng = luts(S3, "float32"), engine_of(S3)
    assert eng.nb == 21
    obs, w = scene(torch_mod, eng, "R_TOC", "per_observation")
    search = engine_of(None)
    before = search.calls["spart_lut_topk_obs_weights"], eng.calls["spart_refine"]
    check(torch_mod, lut, eng, obs, w, opts={"n_iter": 2, "prior": "knn"})
    assert search.calls["spart_lut_topk_obs_weights"] > before[0] and eng.calls["spart_refine"] > before[1]
    obs, w = scene(torch_mod, eng, "R_TOC", "none")
    before = search.calls["spart_lut_topk"]
    check(torch_mod, lut, eng, obs, w, opts={"n_iter": 2, "prior": "knn"}, callers=("device", "stream"), chunks=(64,))
    assert search.calls["spart_lut_topk"] > before


# ---- D. a custom sensor of 211 bands: the wide search and a 14-tile fit in one pipeline, on two engines
@pytest.mark.parametrize("weights", ["shared", "per_observation"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_custom_211_band_sensor(torch_mod, luts, engine_of, dtype, weights):
    lut, eng, search = luts(HYPER, dtype), engine_of(HYPER), engine_of(None)
    assert eng.nb == 211 and eng is not search
    with open(os.path.join(lut[0], "meta.json")) as f:
        assert json.load(f)["sensor"] == HYPER
    obs, w = scene(torch_mod, eng, "R_TOC", weights, m=48)
    entry = "spart_lut_topk_wide" if weights == "shared" else "spart_lut_topk_obs_weights"
    other = "spart_lut_topk_obs_weights" if weights == "shared" else "spart_lut_topk_wide"
    before = {e: (e.calls[entry], e.calls[other], e.calls["spart_refine"], e.calls["spart_lut_topk"]) for e in (eng, search)}
    check(torch_mod, lut, eng, obs, w, opts={"n_iter": 2, "prior": "knn"})
    after = {e: (e.calls[entry], e.calls[other], e.calls["spart_refine"], e.calls["spart_lut_topk"]) for e in (eng, search)}
    # the searches ran on the engine without a sensor, the intended one and no other; the fit on the sensor's engine only
    assert after[search][0] >= before[search][0] + 7 and after[search][1:] == before[search][1:]
    assert after[eng][2] >= before[eng][2] + 7 and after[eng][0] == before[eng][0] and after[eng][1] == before[eng][1]


# ---- E. the options handed through
def test_refine_opts_reach_the_fit(torch_mod, luts, engine_of):
    lut, eng = luts(S2, "float32"), engine_of(S2)
    obs, w = scene(torch_mod, eng, "R_TOC", "per_observation")
    lo, hi = bounds_of_lut(lut)
    bounds = {"LAI": (float(lo[0] + 0.1 * (hi[0] - lo[0])), float(hi[0] - 0.1 * (hi[0] - lo[0]))),
              "Cw": (float(lo[2] + 0.05 * (hi[2] - lo[2])), float(hi[2] - 0.2 * (hi[2] - lo[2])))}
    opts = {"n_iter": 2, "lidf": "newton", "nlayers": 30, "bounds": bounds, "rel_step": 5e-4, "lambda0": 1.0}
    ref, got = check(torch_mod, lut, eng, obs, w, opts=opts)
    l2, h2 = lo.copy(), hi.copy()
    (l2[0], h2[0]), (l2[2], h2[2]) = bounds["LAI"], bounds["Cw"]
    assert ((got["refined"][ref["idx"][:, 0] >= 0] >= l2) & (got["refined"][ref["idx"][:, 0] >= 0] <= h2)).all()
    # none of the options is a no-op: the definition with each one alone, and with all, ends elsewhere than the default
    args = (lut[1], lut[2]["R_TOC"], obs, K, w, NAMES4)
    default = retrieve_defined(*args, lo, hi, forward_of(torch_mod, eng, "R_TOC"), n_iter=2)
    assert not same(default["refined"], ref["refined"])
    alone = {"lidf": retrieve_defined(*args, lo, hi, forward_of(torch_mod, eng, "R_TOC", lidf="newton"), n_iter=2),
             "nlayers": retrieve_defined(*args, lo, hi, forward_of(torch_mod, eng, "R_TOC", nlayers=30), n_iter=2),
             "bounds": retrieve_defined(*args, l2, h2, forward_of(torch_mod, eng, "R_TOC"), n_iter=2),
             "rel_step": retrieve_defined(*args, lo, hi, forward_of(torch_mod, eng, "R_TOC"), n_iter=2, rel_step=5e-4),
             "lambda0": retrieve_defined(*args, lo, hi, forward_of(torch_mod, eng, "R_TOC"), n_iter=2, lambda0=1.0)}
    for name, r in alone.items():
        assert same(r["idx"], default["idx"]) and not same(r["refined"], default["refined"]), name
    # ... and the callers with one option alone, the ones the stream hands on by name
    import spart_amd
    for name in ("lidf", "nlayers"):
        one = {"n_iter": 2, name: opts[name]}
        for res in (spart_amd.retrieve(lut[0], obs, K, weights=w, summary="device", refine=NAMES4, refine_opts=one),
                    spart_amd.retrieve_stream(lut[0], obs, K, weights=w, chunk=50, refine=NAMES4, refine_opts=one)):
            assert all(same(res[key], alone[name][key]) for key in REFINED), name


# ---- F. the edges of the join
def test_fewer_rows_than_k(torch_mod, luts, engine_of):
    """B = 3, k = 5: idx carries two places of padding, which the start, the summary and the "knn" prior must skip"""
    lut, eng = luts(S2, "float32", rows=3), engine_of(S2)
    for weights in ("none", "per_observation"):
        obs, w = scene(torch_mod, eng, "R_TOC", weights)
        ref, got = check(torch_mod, lut, eng, obs, w, opts={"n_iter": 2, "prior": "knn"})
        ok = ref["idx"][:, 0] >= 0
        assert (got["idx"][:, 3:] == -1).all() and (got["idx"][ok, :3] >= 0).all() and np.isinf(got["cost"][:, 3:]).all()
        assert (got["count"][ok] == 3).all() and (got["count"][~ok] == 0).all()
        assert (np.sort(got["idx"][ok, :3], axis=1) == np.arange(3)).all()


def test_k_of_one_rests_the_prior_on_its_floor(torch_mod, luts, engine_of):
    lut, eng = luts(S2, "float32"), engine_of(S2)
    obs, w = scene(torch_mod, eng, "R_TOC", "per_observation")
    ref, got = check(torch_mod, lut, eng, obs, w, k=1, opts={"n_iter": 2, "prior": "knn"})
    ok = ref["idx"][:, 0] >= 0
    assert (got["std"][ok] == 0).all() and (got["count"][ok] == 1).all() and same(got["mean"][ok], lut[1][got["idx"][ok, 0]])
    # sigma = floor x range: the "knn" prior at k = 1 IS the dict prior (start row, 0.05 (hi - lo)), and the floor matters
    lo, hi = bounds_of_lut(lut)
    start = np.where(ok[:, None], lut[1][np.maximum(ref["idx"][:, 0], 0)][:, cols_of(NAMES4)], 0.5 * (lo + hi))
    as_dict = {n: (start[:, i], 0.05 * (hi[i] - lo[i])) for i, n in enumerate(NAMES4)}
    by_dict = retrieve_defined(lut[1], lut[2]["R_TOC"], obs, 1, w, NAMES4, lo, hi, forward_of(torch_mod, eng, "R_TOC"), n_iter=2, prior=as_dict)
    assert all(same(by_dict[key], ref[key]) for key in REFINED)
    check(torch_mod, lut, eng, obs, w, k=1, opts={"n_iter": 2, "prior": "knn", "prior_floor": 0.5}, callers=("device", "stream"), chunks=(7,))
    wide = retrieve_defined(lut[1], lut[2]["R_TOC"], obs, 1, w, NAMES4, lo, hi, forward_of(torch_mod, eng, "R_TOC"), n_iter=2, prior="knn",
                            prior_floor=0.5)
    assert not same(wide["refined"], ref["refined"])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_nothing_matches_or_nothing_is_asked(torch_mod, luts, engine_of, dtype):
    """every observation NaN; M = 0: all -1 / NaN / empty in every caller, and nothing raises"""
    lut, eng = luts(S2, dtype), engine_of(S2)
    for weights in ("none", "per_observation"):
        obs, w = scene(torch_mod, eng, "R_TOC", weights, all_nan=True)
        ref, got = check(torch_mod, lut, eng, obs, w, opts={"n_iter": 2, "prior": "knn"}, vacuous=True, chunks=(M, 7))
        assert (got["idx"] == -1).all() and np.isinf(got["cost"]).all() and (got["count"] == 0).all() and (got["refined_accepts"] == -1).all()
        assert all(np.isnan(got[key]).all() for key in ("mean", "median", "std") + REFINED[:4])
    prior = {"LAI": (np.zeros(0), 1.0)}
    for w, opts in ((None, {"prior": "knn"}), (np.ones(13), {"prior": prior}), (np.ones((0, 13)), {})):
        ref, got = check(torch_mod, lut, eng, np.empty((0, 13)), w, opts=opts, vacuous=True, chunks=(1,))
        assert got["idx"].shape == (0, K) and got["refined"].shape == (0, 4) and got["refined_accepts"].dtype == np.int32


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_an_empty_lut_with_explicit_bounds(torch_mod, engine_of, tmp_path, dtype):
    """B = 0: the documented shapes and dtypes, NaN, -1, count 0, +inf costs, from retrieve in both summaries and from the stream"""
    import spart_amd
    from spart_amd import workloads
    eng = engine_of(S2)
    d = str(tmp_path / "empty")
    os.makedirs(d)
    P = np.empty((0, 27))
    tabs = {c: np.empty((0, 13), dtype=dtype) for c in ("R_TOC", "R_TOA", "L_TOA")}
    np.save(os.path.join(d, "params.npy"), P)
    for c, t in tabs.items():
        np.save(os.path.join(d, c + ".npy"), t)
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump({"sensor": S2, "dtype": dtype, "columns": list(tabs), "rows": 0, "param_names": workloads.PARAM_NAMES}, f)
    obs, w = scene(torch_mod, eng, "R_TOC", "per_observation")
    for call in (spart_amd.retrieve, spart_amd.retrieve_stream):
        with pytest.raises(ValueError, match="constant"):
            call(d, obs, K, weights=w, refine=NAMES4)
    bounds = {n: workloads.RANGES[n] for n in NAMES4}
    for opts in ({"bounds": bounds}, {"bounds": bounds, "prior": "knn", "n_iter": 2}):
        ref, got = check(torch_mod, (d, P, tabs, None), eng, obs, w, column="R_TOA", opts=opts, vacuous=True, chunks=(M, 7))
        assert got["idx"].shape == (M, K) and (got["idx"] == -1).all() and got["cost"].dtype == np.dtype(dtype) and (got["cost"] == np.inf).all()
        assert got["refined"].shape == got["refined_std"].shape == (M, 4) and np.isnan(got["refined"]).all()
        assert (got["refined_accepts"] == -1).all() and (got["count"] == 0).all() and np.isnan(got["mean"]).all()
    res = spart_amd.retrieve_stream(d, obs, K, weights=w, refine=NAMES4, refine_opts={"bounds": bounds})
    assert res["best_cost"].dtype == np.dtype(dtype) and (res["best_cost"] == np.inf).all() and res["refined_accepts"].dtype == np.int32


def test_out_arrays_across_lut_dtypes(torch_mod, luts, engine_of):
    """retrieve_stream(out=): the arrays of a float64-LUT call are refused by a float32-LUT call for best_cost's dtype, and
    accepted once that one array is replaced; every row is written again"""
    import spart_amd
    l64, l32, eng = luts(S2, "float64"), luts(S2, "float32"), engine_of(S2)
    obs, w = scene(torch_mod, eng, "R_TOC", "per_observation")
    kw = dict(weights=w, refine=NAMES4, refine_opts={"n_iter": 2, "prior": "knn"})
    first = spart_amd.retrieve_stream(l64[0], obs, K, chunk=50, **kw)
    out = {key: v for key, v in first.items() if isinstance(v, np.ndarray)}
    assert sorted(out) == sorted(MAPS + REFINED + ("best_cost",)) and out["best_cost"].dtype == np.float64
    with pytest.raises(ValueError, match="best_cost"):
        spart_amd.retrieve_stream(l32[0], obs, K, chunk=50, out=out, **kw)
    out["best_cost"] = np.zeros(M, dtype=np.float32)
    for a in out.values():
        a[...] = 0
    again = spart_amd.retrieve_stream(l32[0], obs, K, chunk=50, out=out, **kw)
    lo, hi = bounds_of_lut(l32)
    ref = retrieve_defined(l32[1], l32[2]["R_TOC"], obs, K, w, NAMES4, lo, hi, forward_of(torch_mod, eng, "R_TOC"), n_iter=2, prior="knn")
    assert all(again[key] is out[key] for key in out) and all(same(again[key], ref[key]) for key in MAPS + REFINED)
    assert same(again["best_cost"], ref["cost"][:, 0]) and (ref["refined_accepts"] >= 1).any()
    short = dict(out, refined=np.zeros((M, 3)))
    with pytest.raises(ValueError, match="refined"):
        spart_amd.retrieve_stream(l32[0], obs, K, out=short, **kw)


def test_a_constant_free_column_needs_bounds(torch_mod, luts, engine_of):
    import spart_amd
    lut, eng = luts(S2, "float32", rows=512, const={"Cw": 0.02}), engine_of(S2)
    obs, w = scene(torch_mod, eng, "R_TOC", "shared")
    for call in (spart_amd.retrieve, spart_amd.retrieve_stream):
        with pytest.raises(ValueError, match="constant"):
            call(lut[0], obs, K, weights=w, refine=NAMES4)
    ref, got = check(torch_mod, lut, eng, obs, w, opts={"n_iter": 2, "bounds": {"Cw": (0.005, 0.05)}}, chunks=(M, 7))
    ok = ref["idx"][:, 0] >= 0
    assert not same(ref["refined"][ok, 2], ref["start"][ok, 2]) and (ref["start"][ok, 2] == 0.02).all()   # the constant column moves
