"""retrieve_stream(refine=...) without a GPU: the chunk arithmetic of a float32 LUT -- every chunk goes up twice, in the LUT's
dtype for the search and as float64 of the caller's arrays for the fit -- with an injected stage that records what it is handed
and answers with the definition tests/helpers/retrieve_defined.py over a toy forward model; that definition's own invariants;
the edges of retrieve_stream(refine=...) that are settled before a device is asked for; and retrieve(refine=...) itself, the
join of search, summary, prior and fit, over a stand-in engine that answers with the definitions under tools/."""
import json
import os

import numpy as np
import pytest

from helpers.retrieve_defined import REFINED, retrieve_defined, same

NB, B, K, M = 6, 300, 4, 23
NAMES = ["LAI", "Cab", "Cw", "Cdm"]
MAPS = ("mean", "median", "std", "count", "best_cost")
_W = np.random.default_rng(11).normal(size=(27, NB))


def forward(rows):
    """the toy forward model of tests/test_refine_prior_host.py on NB bands"""
    return np.tanh(rows @ _W * 0.05) + 0.1 * np.sin(rows[:, [0]] * np.arange(1, NB + 1) * 0.01)


def write_lut(d, params, dtype, table=None, **meta):
    from spart_amd import workloads
    os.makedirs(d)
    table = (forward(params) if table is None else table).astype(dtype)
    np.save(os.path.join(d, "params.npy"), params)
    np.save(os.path.join(d, "R_TOC.npy"), table)
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(dict({"sensor": "Sentinel2A-MSI", "dtype": dtype, "columns": ["R_TOC"], "rows": params.shape[0],
                        "param_names": workloads.PARAM_NAMES}, **meta), f)
    return str(d), table


def free_bounds(params, names=NAMES):
    from spart_amd import workloads
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    return params[:, cols].min(axis=0), params[:, cols].max(axis=0)


def toy_scene(weights, seed=9):
    """M observations: the toy model at rows that are not in the LUT, 2 % noise; values that float32 does not hold.  Planted:
    5 a NaN band (masked under per-observation weights, otherwise unmatched), 6 a negative weight, 8 an unmasked NaN row"""
    rng = np.random.default_rng(seed)
    obs = forward(rng.uniform(0.0, 1.0, (M, 27))) * (1.0 + 0.02 * rng.normal(size=(M, NB)))
    w = {"none": None, "shared": rng.uniform(0.5, 2.0, NB), "per_observation": rng.uniform(0.5, 2.0, (M, NB))}[weights]
    obs[5, 2] = np.nan
    obs[8] = np.nan
    if weights == "per_observation":
        w[5, 2] = 0.0
        w[6, 1] = -1.0
    return obs, w


class WideStage:
    """the stage interface of spart_amd.lut._stream_chunks for a float32 LUT with a refinement (``wide``): it checks and records
    both copies of every chunk against the caller's arrays and answers with retrieve_defined on the float64 copy"""
    wide = True

    def __init__(self, params, table, obs, weights, lo, hi, **fit):
        self.params, self.table, self.caller_obs, self.caller_w, self.lo, self.hi, self.fit = params, table, obs, weights, lo, hi, fit
        self.per_obs = weights is not None and np.ndim(weights) == 2
        self.inp, self.res, self.sizes, self.uploads, self.row = [None, None], [None, None], [], [], 0

    def upload(self, j, obs, w, obs64=None, w64=None):
        n, dt = obs.shape[0], self.table.dtype
        rows = slice(self.row, self.row + n)
        self.row += n
        want = np.asarray(self.caller_obs[rows])
        for a, d in ((obs, dt), (obs64, np.float64)):
            assert isinstance(a, np.ndarray) and a.shape == (n, NB) and a.dtype == d and a.flags.c_contiguous, (rows, d)
        assert same(obs, want.astype(dt)) and same(obs64, np.ascontiguousarray(want, dtype=np.float64))
        if np.isfinite(want).any():                                              # the caller's numbers, not the rounded ones
            assert not same(obs64, want.astype(dt).astype(np.float64))
        if self.per_obs:
            ww = np.asarray(self.caller_w[rows])
            for a, d in ((w, dt), (w64, np.float64)):
                assert isinstance(a, np.ndarray) and a.shape == (n, NB) and a.dtype == d and a.flags.c_contiguous, (rows, d)
            assert same(w, ww.astype(dt)) and same(w64, np.ascontiguousarray(ww, dtype=np.float64))
            assert not same(w64, ww.astype(dt).astype(np.float64))
        else:
            assert w is None and w64 is None
        self.inp[j] = (obs, w, obs64, w64)
        self.uploads.append((rows.start, n, w64 is not None))

    def launch(self, j, n):
        obs, w, obs64, w64 = self.inp[j]
        assert obs.shape[0] == n
        self.sizes.append(n)
        r = retrieve_defined(self.params, self.table, obs64, K, w64 if self.per_obs else self.caller_w, NAMES, self.lo, self.hi,
                             forward, **self.fit)
        self.res[j] = dict({k: r[k] for k in MAPS[:4] + REFINED}, best_cost=r["cost"][:, 0].copy())

    def download(self, j, n, dest):
        for name, a in dest.items():
            assert a.shape[0] == n
            a[...] = self.res[j][name]


def rounded_numbers_end_elsewhere(params, table, obs, w, lo, hi, fit, want):
    """the float64 copies matter: with the rounded numbers the definition ends elsewhere"""
    rounded = retrieve_defined(params, table, obs.astype(np.float32), K, w, NAMES, lo, hi, forward, **fit)
    assert same(rounded["idx"], want["idx"]) and not same(rounded["refined"], want["refined"])
    if w is not None and w.ndim == 2:
        rounded = retrieve_defined(params, table, obs, K, w.astype(np.float32), NAMES, lo, hi, forward, **fit)
        assert same(rounded["idx"], want["idx"]) and not same(rounded["refined"], want["refined"])


@pytest.fixture(scope="module")
def toy_lut(tmp_path_factory):
    params = np.random.default_rng(5).uniform(0.0, 1.0, (B, 27))
    d, table = write_lut(tmp_path_factory.mktemp("wide") / "lut", params, "float32")
    return d, params, table


@pytest.mark.parametrize("prior", [None, "knn"])
@pytest.mark.parametrize("weights", ["none", "shared", "per_observation"])
def test_a_float32_lut_sends_every_chunk_up_twice(toy_lut, weights, prior):
    from spart_amd import retrieve_stream
    d, params, table = toy_lut
    obs, w = toy_scene(weights)
    lo, hi = free_bounds(params)
    fit = dict(n_iter=3, rel_step=2e-3, lambda0=0.1, prior=prior, prior_floor=0.1 if prior else 0.05)
    opts = {k: v for k, v in fit.items() if k != "prior_floor" and v is not None}
    if prior:
        opts["prior_floor"] = 0.1
    want = retrieve_defined(params, table, obs, K, w, NAMES, lo, hi, forward, **fit)
    want["best_cost"] = want["cost"][:, 0].copy()
    matched = want["idx"][:, 0] >= 0
    assert not matched[8] and matched[5] == (weights == "per_observation") and matched[6] == (weights != "per_observation")
    assert (want["refined_accepts"][matched] >= 0).mean() > 0.5 and (want["refined_accepts"] >= 1).any()
    assert not same(want["refined"], want["start"])
    assert np.isnan(want["refined"][~matched]).all() and (want["refined_accepts"][~matched] == -1).all()
    rounded_numbers_end_elsewhere(params, table, obs, w, lo, hi, fit, want)
    scene = np.asfortranarray(obs)                                   # (not C-contiguous: the chunks must be made so)
    for chunk, sizes in ((1, [1] * M), (7, [7, 7, 7, 2]), (M, [M]), (M + 1, [M])):
        stage = WideStage(params, table, scene, w, lo, hi, **fit)
        got = retrieve_stream(d, scene, K, weights=w, chunk=chunk, refine=NAMES, refine_opts=opts, _stage=stage)
        assert stage.sizes == sizes and stage.row == M and got["refined_names"] == NAMES
        assert stage.uploads == [(lo_, n, weights == "per_observation") for lo_, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
        assert sorted(got) == sorted(MAPS + REFINED + ("names", "refined_names"))
        for name in MAPS + REFINED:
            assert same(got[name], want[name]), (chunk, name)
    assert got["best_cost"].dtype == np.float32 and got["refined_accepts"].dtype == np.int32


def test_a_float64_lut_or_no_refinement_sends_one_copy(toy_lut, tmp_path):
    """``wide`` is the stage's word: a stage without it is handed (obs, w) only, refined or not"""
    from spart_amd import retrieve_stream
    _, params, _ = toy_lut
    d, table = write_lut(tmp_path / "f64", params, "float64")
    obs, w = toy_scene("per_observation")
    lo, hi = free_bounds(params)
    seen = []

    class Narrow(WideStage):
        wide = False

        def upload(self, j, o, ww):
            assert o.dtype == np.float64 and ww.dtype == np.float64 and o.flags.c_contiguous and ww.flags.c_contiguous
            seen.append(o.shape[0])
            self.inp[j] = (o, ww, o, ww)
    want = retrieve_defined(params, table, obs, K, w, NAMES, lo, hi, forward, n_iter=2)
    got = retrieve_stream(d, obs, K, weights=w, chunk=10, refine=NAMES, refine_opts={"n_iter": 2},
                          _stage=Narrow(params, table, obs, w, lo, hi, n_iter=2))
    assert seen == [10, 10, 3] and all(same(got[k], want[k]) for k in REFINED + MAPS[:4])


def test_the_definitions_own_invariants(toy_lut):
    _, params, table = toy_lut
    lo, hi = free_bounds(params)
    obs, w = toy_scene("per_observation")
    kw = dict(n_iter=3, lambda0=0.1)
    full = retrieve_defined(params, table, obs, K, w, NAMES, lo, hi, forward, **kw)
    # the first k - 1 places at k are the answer at k - 1; without a prior the fit only knows place 0
    less = retrieve_defined(params, table, obs, K - 1, w, NAMES, lo, hi, forward, **kw)
    assert same(full["idx"][:, :K - 1], less["idx"]) and same(full["cost"][:, :K - 1], less["cost"])
    assert all(same(full[k], less[k]) for k in REFINED)
    assert not same(full["mean"], less["mean"])
    knn = [retrieve_defined(params, table, obs, k, w, NAMES, lo, hi, forward, prior="knn", **kw) for k in (K, K - 1)]
    assert not same(knn[0]["refined"], knn[1]["refined"]) and not same(knn[0]["refined"], full["refined"])
    # unmatched rows: NaN and -1, whatever the prior
    for r in (full, knn[0]):
        none = r["idx"][:, 0] < 0
        assert list(np.flatnonzero(none)) == [6, 8] and (r["count"][none] == 0).all() and np.isinf(r["cost"][none]).all()
        assert all(np.isnan(r[k][none]).all() for k in REFINED[:4]) and (r["refined_accepts"][none] == -1).all()
        assert np.isfinite(r["refined"][~none]).all() and (r["refined_accepts"][~none] >= 0).mean() > 0.5
        assert (r["refined_cost"][~none] <= r["refined_cost0"][~none]).all()
    # a float64 table: the cost at the start IS the search's cost of place 0 (the same sum over the same numbers)
    t64 = forward(params)
    r64 = retrieve_defined(params, t64, obs, K, w, NAMES, lo, hi, forward, **kw)
    ok = r64["idx"][:, 0] >= 0
    assert same(r64["refined_cost0"][ok], r64["cost"][ok, 0]) and not same(full["refined_cost0"][ok], full["cost"][ok, 0].astype(np.float64))
    # one weight row for all, or the same row repeated: the same bits where no band is masked
    clean = np.where(np.isnan(obs), 0.2, obs)
    ws = np.abs(w[0])
    assert (ws > 0).all()
    a = retrieve_defined(params, table, clean, K, ws, NAMES, lo, hi, forward, prior="knn", **kw)
    b = retrieve_defined(params, table, clean, K, np.tile(ws, (M, 1)), NAMES, lo, hi, forward, prior="knn", **kw)
    assert all(same(a[k], b[k]) for k in ("idx", "cost", "mean", "median", "std", "count") + REFINED)
    # params_cols cuts the summary and nothing else
    c = retrieve_defined(params, table, clean, K, ws, NAMES, lo, hi, forward, prior="knn", params_cols=["Cw", "LAI"], **kw)
    assert same(c["mean"], a["mean"][:, [2, 15]]) and same(c["median"], a["median"][:, [2, 15]]) and same(c["refined"], a["refined"])
    # a dict prior: a name that is not listed and a sigma of inf are no prior
    p1 = {"LAI": (np.linspace(0.2, 0.8, M), 0.1), "Cab": (0.5, np.inf)}
    p2 = {"LAI": (np.linspace(0.2, 0.8, M), 0.1)}
    d1, d2 = (retrieve_defined(params, table, clean, K, ws, NAMES, lo, hi, forward, prior=p, **kw) for p in (p1, p2))
    assert same(d1["refined"], d2["refined"]) and not same(d1["refined"], a["refined"])


def stream_shapes(got, m, F, dt, P=27):
    assert got["mean"].shape == got["median"].shape == got["std"].shape == (m, P)
    assert got["refined"].shape == got["refined_std"].shape == (m, F)
    assert got["count"].shape == got["best_cost"].shape == got["refined_cost"].shape == got["refined_cost0"].shape == got["refined_accepts"].shape == (m,)
    assert got["count"].dtype == got["refined_accepts"].dtype == np.int32 and got["best_cost"].dtype == dt
    assert all(got[k].dtype == np.float64 for k in ("mean", "median", "std", "refined", "refined_std", "refined_cost", "refined_cost0"))


def test_stream_edges_that_need_no_device(toy_lut, tmp_path):
    """M = 0; B = 0 with explicit bounds; out= across LUT dtypes; a constant free column"""
    from spart_amd import retrieve_stream
    d32, params, table = toy_lut
    lo, hi = free_bounds(params)
    # no observations: nothing is launched, the arrays have their shapes
    stage = WideStage(params, table, np.empty((0, NB)), None, lo, hi)
    got = retrieve_stream(d32, np.empty((0, NB)), K, refine=NAMES, refine_opts={"prior": "knn"}, _stage=stage)
    assert stage.sizes == [] and got["refined_names"] == NAMES
    stream_shapes(got, 0, 4, np.float32)
    # an empty table matches nothing; its free columns have no extent, so the bounds must be given
    for dtype in ("float32", "float64"):
        d0, _ = write_lut(tmp_path / ("empty" + dtype), np.empty((0, 27)), dtype, table=np.empty((0, NB)))
        obs, w = toy_scene("per_observation")
        with pytest.raises(ValueError, match="constant"):
            retrieve_stream(d0, obs, K, weights=w, refine=NAMES)
        bounds = {n: (0.0, 1.0) for n in NAMES}
        got = retrieve_stream(d0, obs, K, weights=w, refine=NAMES, refine_opts={"bounds": bounds, "prior": "knn"}, params_cols=["LAI"])
        stream_shapes(got, M, 4, np.dtype(dtype), P=1)
        assert all(np.isnan(got[k]).all() for k in ("mean", "median", "std", "refined", "refined_std", "refined_cost", "refined_cost0"))
        assert (got["count"] == 0).all() and (got["refined_accepts"] == -1).all() and (got["best_cost"] == np.inf).all()
    # out= of a float64-LUT call offered to a float32-LUT call: best_cost has the other dtype; replacing that array is enough
    d64, t64 = write_lut(tmp_path / "f64", params, "float64")
    obs, w = toy_scene("shared")

    class Narrow(WideStage):
        wide = False

        def upload(self, j, o, ww):
            self.inp[j] = (o, ww, o, ww)
    first = retrieve_stream(d64, obs, K, weights=w, refine=NAMES, refine_opts={"n_iter": 1}, chunk=9,
                            _stage=Narrow(params, t64, obs, w, lo, hi, n_iter=1))
    want64 = retrieve_defined(params, t64, obs, K, w, NAMES, lo, hi, forward, n_iter=1)
    assert all(same(first[k], want64[k]) for k in REFINED) and first["best_cost"].dtype == np.float64
    out = {k: v for k, v in first.items() if isinstance(v, np.ndarray)}
    with pytest.raises(ValueError, match="best_cost"):
        retrieve_stream(d32, obs, K, weights=w, refine=NAMES, refine_opts={"n_iter": 1}, out=out,
                        _stage=WideStage(params, table, obs, w, lo, hi, n_iter=1))
    out["best_cost"] = np.empty(M, dtype=np.float32)
    for a in out.values():
        a[...] = 0
    again = retrieve_stream(d32, obs, K, weights=w, refine=NAMES, refine_opts={"n_iter": 1}, out=out, chunk=9,
                            _stage=WideStage(params, table, obs, w, lo, hi, n_iter=1))
    want32 = retrieve_defined(params, table, obs, K, w, NAMES, lo, hi, forward, n_iter=1)
    assert all(again[k] is out[k] for k in MAPS + REFINED) and all(same(again[k], want32[k]) for k in MAPS[:4] + REFINED)
    assert same(again["best_cost"], want32["cost"][:, 0]) and (want32["refined_accepts"] >= 1).any()
    # a free column that is constant in the LUT has no default bounds
    flat = params.copy()
    flat[:, 2] = 0.3                                                 # Cw
    dc, tc = write_lut(tmp_path / "flat", flat, "float32")
    with pytest.raises(ValueError, match="constant"):
        retrieve_stream(dc, obs, K, refine=NAMES, _stage=WideStage(flat, tc, obs, None, lo, hi))
    with pytest.raises(ValueError, match="constant"):
        from spart_amd import retrieve
        retrieve(dc, obs, K, refine=NAMES)
    l2, h2 = lo.copy(), hi.copy()
    l2[2], h2[2] = 0.1, 0.9
    got = retrieve_stream(dc, obs, K, refine=NAMES, refine_opts={"bounds": {"Cw": (0.1, 0.9)}, "n_iter": 2},
                          _stage=WideStage(flat, tc, obs, None, l2, h2, n_iter=2))
    want = retrieve_defined(flat, tc, obs, K, None, NAMES, l2, h2, forward, n_iter=2)
    assert all(same(got[k], want[k]) for k in REFINED) and (want["refined_accepts"] >= 1).any()
    assert not same(want["refined"][:, 2], want["start"][:, 2])     # the bounded constant column moves


class HostEngine:
    """Engine's part in retrieve(refine=...) on the host: lut_topk, lut_summarise and refine answer with the definitions under
    tools/ wrapped in CPU tensors (the fit over the toy forward model, whatever the column), and ``fits`` records what every
    refine call was handed"""
    device = "cpu"

    def __init__(self):
        self.fits = []

    def lut_topk(self, lut, obs, k, weights=None, dtype="float32", stats=False):
        import torch
        from helpers.retrieve_defined import bf
        lut = np.ascontiguousarray(np.asarray(lut))
        assert lut.dtype == np.dtype(dtype) and not stats
        o = np.ascontiguousarray(np.asarray(obs), dtype=lut.dtype)
        w = None if weights is None else np.ascontiguousarray(np.asarray(weights), dtype=lut.dtype)
        search = bf.brute_force_topk_obs_weights_numpy if w is not None and w.ndim == 2 else bf.brute_force_topk_numpy
        return tuple(torch.as_tensor(a) for a in search(lut, o, k, w))

    def lut_summarise(self, params, idx):
        import torch
        from helpers.retrieve_defined import bf
        res = bf.summarise_defined(np.asarray(params), np.asarray(idx))
        return {n: torch.as_tensor(a) for n, a in zip(("mean", "median", "std", "count"), res)}

    def refine(self, params, obs, free, **kw):
        import torch
        from helpers.retrieve_defined import rd
        plan = kw["_plan"]
        assert list(free) == plan["names"] and plan["prior"] is None and all(torch.is_tensor(t) for t in (params, obs))
        num = lambda t: None if t is None else t.numpy().copy()      # noqa: E731
        self.fits.append(dict(kw, params=num(params), obs=num(obs), weights=num(kw["weights"])))
        r = rd.refine_defined(num(params).T, plan["cols"], plan["lo"], plan["hi"], num(obs), forward, weights=num(kw["weights"]),
                              n_iter=plan["n_iter"], rel_step=plan["rel_step"], lambda0=plan["lambda0"],
                              prior_mean=num(kw["prior_mean"]), prior_weight=num(kw["prior_weight"]))
        return dict({n: torch.as_tensor(r[n]) for n in ("x", "cost", "cost0", "std", "n_accept", "y")}, names=list(free))


@pytest.fixture()
def host_engine(monkeypatch):
    """spart_amd.lut.get_engine answers with ONE HostEngine; ``asked`` lists (sensor, keyword arguments) of every call"""
    from spart_amd import lut
    eng = HostEngine()
    eng.asked = []

    def get_engine(sensor=None, device=None, **kw):
        eng.asked.append((sensor, kw))
        return eng
    monkeypatch.setattr(lut, "get_engine", get_engine)
    return eng


@pytest.mark.parametrize("prior", [None, "knn", "dict"])
@pytest.mark.parametrize("weights", ["none", "shared", "per_observation"])
def test_retrieve_joins_search_summary_prior_and_fit_as_defined(toy_lut, host_engine, tmp_path, weights, prior):
    """retrieve(refine=...) on the host and on the device summary against retrieve_defined, bit for bit, with what the fit
    was handed: the column's number, lidf, nlayers, the band model, the sensor_info, and float64 of the caller's arrays"""
    from spart_amd import retrieve
    _, params, table = toy_lut
    d, _ = write_lut(tmp_path / "lut", params, "float32", columns=["R_TOC", "L_TOA"])
    np.save(os.path.join(d, "L_TOA.npy"), table)
    obs, w = toy_scene(weights)
    lo, hi = free_bounds(params)
    if prior == "dict":
        prior = {"LAI": (np.linspace(0.2, 0.8, M), 0.1), "Cab": (0.5, 0.2)}
    fit = dict(n_iter=3, rel_step=2e-3, lambda0=0.1, prior=prior, prior_floor=0.1 if prior == "knn" else 0.05)
    opts = {k: v for k, v in fit.items() if k != "prior_floor" and v is not None}
    if prior == "knn":
        opts["prior_floor"] = 0.1
    opts.update(lidf="newton", nlayers=30)
    want = retrieve_defined(params, table, obs, K, w, NAMES, lo, hi, forward, **fit)
    matched = want["idx"][:, 0] >= 0
    assert not matched[8] and matched.sum() >= M - 3 and (want["refined_accepts"] >= 1).any()
    assert np.isnan(want["refined"][~matched]).all() and (want["refined_accepts"][~matched] == -1).all()
    rounded_numbers_end_elsewhere(params, table, obs, w, lo, hi, fit, want)
    sinfo = {"a sensorinfo": "handed on as it is"}
    for summary in ("host", "device"):
        del host_engine.fits[:], host_engine.asked[:]
        got = retrieve(d, obs, K, column="L_TOA", weights=w, summary=summary, refine=NAMES, refine_opts=opts, sensor_info=sinfo)
        assert got["refined_names"] == NAMES and same(got["idx"], want["idx"]) and same(got["cost"], want["cost"])
        for name in REFINED:
            assert same(got[name], want[name]), (summary, name)
        assert [a for a in host_engine.asked if a[0] is not None] == [("Sentinel2A-MSI", {"sensor_info": sinfo})]
        (seen,) = host_engine.fits                                       # one call for all M observations
        assert seen["_plan"]["column"] == 2 and seen["lidf"] == "newton" and seen["nlayers"] == 30 and seen["band_model"] == "centre"
        assert same(seen["obs"], np.asarray(obs, dtype=np.float64)) and seen["params"].shape == (27, M)
        assert same(seen["params"][:, matched], np.ascontiguousarray(params[want["idx"][matched, 0]].T))
        assert (seen["weights"] is None) if w is None else (same(seen["weights"], w) and not same(seen["weights"], w.astype(np.float32).astype(np.float64)))


def test_retrieve_without_a_row_or_an_observation_asks_for_no_fit(toy_lut, host_engine, tmp_path):
    from spart_amd import retrieve
    d32, params, table = toy_lut
    dn, _ = write_lut(tmp_path / "nan", params, "float32", table=np.full((B, NB), np.nan))
    obs, w = toy_scene("per_observation")
    for d, o, ww, m in ((dn, obs, w, M), (d32, np.empty((0, NB)), None, 0)):
        for summary in ("host", "device"):
            got = retrieve(d, o, K, weights=ww, summary=summary, refine=NAMES, refine_opts={"prior": "knn"})
            assert host_engine.fits == [] and all(a[0] is None for a in host_engine.asked) and got["refined_names"] == NAMES
            assert got["idx"].shape == (m, K) and (got["idx"] == -1).all() and np.isinf(got["cost"]).all()
            assert got["refined"].shape == got["refined_std"].shape == (m, 4) and got["refined_accepts"].dtype == np.int32
            assert all(np.isnan(got[k]).all() for k in REFINED[:4]) and (got["refined_accepts"] == -1).all()
            assert all(got[k].shape == (m,) and got[k].dtype == np.float64 for k in ("refined_cost", "refined_cost0"))
