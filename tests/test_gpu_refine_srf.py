"""spart_refine_srf on the MI355X: the SRF-convolved column as the fitted quantity.
  (4) the raw C ABI against the definition tools/refine_defined.py with forward = Engine.run(float64, prune=True,
      materialize=[column + "_srf"]), all six outputs bit for bit, over F x M x n_iter, the three columns, the three weight forms
      and the three prior forms, on three sensors;
  (5) across the host chunk loop;
  (6) the centre model is what it was, and the two options that reach the forward model reach the SRF one;
  (7) generate_lut(band_model="srf") -> retrieve / retrieve_stream(refine_opts={"band_model": "srf"}) against
      helpers/retrieve_defined.py with the SRF forward model, bit for bit;
  (8) the twin experiment with the engine's own SRF columns as the truth."""
import itertools

import numpy as np
import pytest

from helpers.lut_calls import torch_mod  # noqa: F401 (fixture)
from helpers.refine_calls import COLUMNS, F16, FREE, OUTS, S2, bounds_of, cols_of, forward_of, rd, same
from helpers.refine_srf_calls import L8, aligned_olci, assert_same, call_srf, defined_srf, make_srf_case, srf_forward_of
from helpers.retrieve_defined import REFINED, retrieve_defined
from helpers.retrieve_defined import same as same_typed

pytestmark = pytest.mark.gpu

KINDS = ("none", "shared", "per_observation")
SENSORS = ("s2", "l8", "olci21")
FS, MS, ITERS = (1, 6, 16), (1, 63, 65), (0, 2)
NAMES4 = ["LAI", "Cab", "Cw", "Cdm"]
ENTRY = "spart_refine_srf"


@pytest.fixture(scope="module")
def engines(torch_mod):
    """s2: 13 bands, so the last band group of k_columns_srf has three idle waves; l8: negative SRF weights, supports of up to
    319 entries; olci21: 21 bands (two band tiles of the step kernel) handed in as a sensor_info= dict mended by align_srf"""
    from spart_amd import get_engine
    e = {"s2": get_engine(S2, 0), "l8": get_engine(L8, 0), "olci21": get_engine(None, 0, sensor_info=aligned_olci())}
    assert e["s2"].nb == 13 and e["olci21"].nb == 21 and all(x.srf_aligned.all() for x in e.values())
    return e


def combos(si, fi, mi):
    """three (column, weights, prior) triples per (sensor, F, M): every column once, the weight and prior forms rotated, so that
    the grid holds all 27 triples"""
    return [(c, KINDS[(c + fi + mi) % 3], KINDS[(c + si + 2 * fi + mi) % 3]) for c in range(3)]


def test_the_grid_holds_every_column_weight_and_prior_form():
    grid = {t for si in range(3) for fi in range(3) for mi in range(3) for t in combos(si, fi, mi)}
    assert grid == set(itertools.product(range(3), KINDS, KINDS))
    for si in range(3):                                    # ... and every sensor sees every pair of forms
        assert {t[1:] for fi in range(3) for mi in range(3) for t in combos(si, fi, mi)} == set(itertools.product(KINDS, KINDS))


# ---- 4. bit for bit against the definition
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("sensor", SENSORS)
def test_definition_bit_for_bit(torch_mod, engines, sensor, F):
    eng = engines[sensor]
    si, fi = SENSORS.index(sensor), FS.index(F)
    names = FREE[F]
    for mi, M in enumerate(MS):
        for column, kind, prior in combos(si, fi, mi):
            what = (sensor, F, M, COLUMNS[column], kind, prior)
            case = make_srf_case(torch_mod, eng, names, M, COLUMNS[column], kind, prior, 100 * eng.nb + 10 * F + M + column)
            base, free, lo, hi, obs, w, mean, weight = case
            refs = {n: defined_srf(torch_mod, eng, case, column, n) for n in ITERS}
            # before any call: the definition alone shows that the case can fail
            ref = refs[2]
            alive = ref["n_accept"] >= 0
            assert alive.mean() > 0.5, what
            assert (ref["n_accept"] >= 1).any() and not same(ref["x"], refs[0]["x"]), (what, ref["n_accept"])
            assert (ref["cost"][alive] <= ref["cost0"][alive]).all() and same(refs[0]["cost0"], ref["cost0"])
            assert same(refs[0]["x"], rd.clip_defined(base[:, free], lo, hi)) and (refs[0]["n_accept"][alive] == 0).all()
            if kind == "per_observation" and M >= 63:
                assert (ref["n_accept"][[3, 5]] == -1).all() and ref["n_accept"][6] >= 0 and np.isnan(obs[6, -1]) and w[6, -1] == 0, what
                assert np.isnan(ref["cost0"][3])
            for n in ITERS:
                got = call_srf(torch_mod, eng, case, column, n, guard=(n == 2))
                assert_same(got, refs[n], what + (n,))
            # the band model is not a no-op: the centre entry point ends elsewhere on the same arguments
            centre = call_srf(torch_mod, eng, case, column, 2, entry="spart_refine")
            assert not same(centre["y"], ref["y"]) and not same(centre["cost0"], ref["cost0"]), what


# ---- 5. the chunk cut
def test_chunk_cut(torch_mod, engines):
    """F = 16: chunks of (1 << 19) // 17 = 30 840 observations, so M = 31 000 runs a second chunk of 160, whose prior rows start
    at chunk * F and whose forward call has another batch size"""
    eng = engines["s2"]
    chunk, M = (1 << 19) // 17, 31000
    assert chunk == 30840
    case = make_srf_case(torch_mod, eng, F16, M, "R_TOC", "per_observation", "per_observation", 51)
    for p, s in ((chunk - 1, 3), (chunk, 5), (chunk + 1, 6)):       # dead rows on both sides of the cut, a live masked one behind
        for a in (case[0], case[4], case[5], case[6], case[7]):
            a[p] = a[s]
    ref = defined_srf(torch_mod, eng, case, 0, 1)
    alive = ref["n_accept"] >= 0
    assert alive.mean() > 0.5 and (ref["n_accept"][:chunk] >= 1).any() and (ref["n_accept"][chunk:] >= 1).any()
    assert ref["n_accept"][chunk - 1] == -1 and ref["n_accept"][chunk] == -1 and ref["n_accept"][chunk + 1] >= 0
    got = call_srf(torch_mod, eng, case, 0, 1, guard=True)
    assert_same(got, ref, "M = 31000")
    tail = tuple(a[chunk:] if np.ndim(a) == 2 and a.shape[0] == M else a for a in case)
    assert_same(call_srf(torch_mod, eng, tail, 0, 1), {k: got[k][chunk:] for k in OUTS}, "[chunk:] alone")


# ---- 6. the centre model is untouched; the options reach the SRF forward model
def test_centre_model_untouched_and_options(torch_mod, engines):
    import spart_amd
    eng = engines["s2"]
    names = FREE[6]
    case = make_srf_case(torch_mod, eng, names, 65, "R_TOA", "per_observation", "none", 61)
    base, free, lo, hi, obs, w, _, _ = case
    P = torch_mod.as_tensor(np.ascontiguousarray(base.T), device=eng.device)
    host = lambda r: {k: r[k].cpu().numpy() for k in OUTS}      # noqa: E731
    kw = dict(weights=w, column="R_TOA", n_iter=2)
    before = dict(eng.calls)
    default = host(eng.refine(P, obs, names, **kw))
    assert eng.calls["spart_refine"] == before.get("spart_refine", 0) + 1 and eng.calls[ENTRY] == before.get(ENTRY, 0)
    centre = host(eng.refine(P, obs, names, band_model="centre", **kw))
    assert eng.calls["spart_refine"] == before.get("spart_refine", 0) + 2 and eng.calls[ENTRY] == before.get(ENTRY, 0)
    assert_same(centre, default, "band_model='centre' is the default")
    centre_ref = rd.refine_defined(base, free, lo, hi, obs, forward_of(torch_mod, eng, "R_TOA"), weights=w, n_iter=2)
    assert_same(default, centre_ref, "the centre definition")
    srf = host(eng.refine(P, obs, names, band_model="srf", **kw))
    assert eng.calls["spart_refine"] == before.get("spart_refine", 0) + 2 and eng.calls[ENTRY] == before.get(ENTRY, 0) + 1
    plain = defined_srf(torch_mod, eng, case, 1, 2)
    assert (plain["n_accept"] >= 1).mean() > 0.5
    assert_same(srf, plain, "Engine.refine(band_model='srf')")
    assert not same(srf["x"], default["x"]) and not same(srf["y"], default["y"])
    res = spart_amd.refine(base.T, obs, S2, names, band_model="srf", **kw)
    assert res["names"] == names
    assert_same({k: np.asarray(res[k]) for k in OUTS}, plain, "spart_amd.refine(band_model='srf')")
    # fast_prelude / nlayers change the SRF bits, and each matches the definition configured like it
    for lidf, nlayers in (("newton", None), ("literal", 30), ("newton", 30)):
        ref = defined_srf(torch_mod, eng, case, 1, 2, lidf, nlayers)
        assert not same(ref["x"], plain["x"]) and not same(ref["y"], plain["y"]), (lidf, nlayers)
        assert_same(call_srf(torch_mod, eng, case, 1, 2, lidf, nlayers), ref, (lidf, nlayers))
        got = host(eng.refine(P, obs, names, band_model="srf", lidf=lidf, nlayers=nlayers, **kw))
        assert_same(got, ref, ("Engine.refine", lidf, nlayers))


def test_a_misaligned_sensor_is_refused(torch_mod):
    import spart_amd
    from spart_amd import get_engine, workloads
    eng = get_engine("TerraAqua-MODIS", 0)
    P = workloads.lhs_params(4, "full", seed=1)
    obs = np.full((4, eng.nb), 0.2)
    before = dict(eng.calls)
    with pytest.raises(ValueError, match="align_srf"):
        eng.refine(list(P.T), obs, ["LAI"], band_model="srf")
    with pytest.raises(ValueError, match="align_srf"):
        spart_amd.refine(P.T, obs, "TerraAqua-MODIS", ["LAI"], band_model="srf")
    assert dict(eng.calls) == before
    assert eng.refine(list(P.T), obs, ["LAI"], n_iter=1)["x"].shape == (4, 1)      # the centre model does not mind


# ---- 7. end to end
@pytest.fixture(scope="module")
def srf_luts(torch_mod, tmp_path_factory):
    """dtype -> (directory, params, {column: table}): 4096 LHS rows written by generate_lut(band_model="srf"), once per module"""
    import spart_amd
    from spart_amd import workloads
    made = {}

    def get(dtype):
        if dtype not in made:
            P = workloads.lhs_params(4096, "full", seed=12)
            d = str(tmp_path_factory.mktemp("srf_lut") / "lut")
            spart_amd.generate_lut(P, S2, path=d, dtype=dtype, band_model="srf")
            meta, _, tabs = spart_amd.load_lut(d, mmap=False)
            assert meta["band_model"] == "srf" and all(t.dtype == np.dtype(dtype) for t in tabs.values())
            made[dtype] = (d, P, tabs)
        return made[dtype]
    return get


def srf_scene(torch, eng, column, weights, m=96, seed=13):
    """m observations: the SRF model at LHS rows that are not the LUT's, 2 % noise; per-observation weights with planted rows: 7
    an unmasked NaN observation (matches nothing), 9 a NaN under a zero weight (fine), 11 a negative weight (matches nothing)"""
    import spart_amd
    from spart_amd import workloads
    rng = np.random.default_rng(seed + 1)
    with np.errstate(all="ignore"):
        obs = srf_forward_of(torch, eng, column)(workloads.lhs_params(m, "full", seed=seed))
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
    return obs, w


E2E = [("float64", "R_TOC", "per_observation", None), ("float64", "R_TOA", "shared", "knn"), ("float64", "L_TOA", "none", "dict"),
       ("float32", "R_TOC", "shared", "dict"), ("float32", "R_TOA", "none", None), ("float32", "L_TOA", "per_observation", "knn")]


@pytest.mark.parametrize("dtype,column,weights,prior", E2E, ids=["-".join(map(str, c)) for c in E2E])
def test_end_to_end(torch_mod, engines, srf_luts, dtype, column, weights, prior):
    import spart_amd
    eng = engines["s2"]
    d, P, tabs = srf_luts(dtype)
    table = tabs[column]
    K, M = 5, 96
    obs, w = srf_scene(torch_mod, eng, column, weights, m=M)
    cols = cols_of(NAMES4)
    lo, hi = P[:, cols].min(axis=0), P[:, cols].max(axis=0)
    if prior == "dict":
        prior = {"LAI": (np.linspace(lo[0], hi[0], M), 1.0), "Cab": (40.0, np.inf)}
    opts = {"n_iter": 2, "band_model": "srf"}
    if prior is not None:
        opts["prior"] = prior
    ref = retrieve_defined(P, table, obs, K, w, NAMES4, lo, hi, srf_forward_of(torch_mod, eng, column), n_iter=2, prior=prior)
    # before any call: the definition alone shows that the case can fail, and that the band model matters
    matched = ref["idx"][:, 0] >= 0
    acc = ref["refined_accepts"][matched]
    assert matched.mean() > 0.9 and (acc >= 0).mean() > 0.5 and (acc >= 1).any() and not same_typed(ref["refined"], ref["start"])
    if weights == "per_observation":
        assert not matched[7] and matched[9] and not matched[11]
    other = retrieve_defined(P, table, obs, K, w, NAMES4, lo, hi, forward_of(torch_mod, eng, column), n_iter=2, prior=prior)
    assert same_typed(other["idx"], ref["idx"]) and not same_typed(other["refined"], ref["refined"])
    if dtype == "float64":
        # the LUT's rows ARE the fit's forward model: without a prior (whose term cost0 includes) the start's cost is the search's
        start = retrieve_defined(P, table, obs, K, w, NAMES4, lo, hi, srf_forward_of(torch_mod, eng, column), n_iter=0)
        assert same_typed(start["refined_cost0"][matched], ref["cost"][matched, 0])
        assert (prior is None) == same_typed(ref["refined_cost0"], start["refined_cost0"])
        assert not same_typed(other["refined_cost0"][matched], ref["cost"][matched, 0])
    kw = dict(column=column, weights=w, refine=NAMES4, refine_opts=opts)
    before = eng.calls[ENTRY], eng.calls["spart_refine"]
    got = spart_amd.retrieve(d, obs, K, summary="device", **kw)
    for key in ("idx", "cost", "mean", "median", "std", "count") + REFINED:
        assert same_typed(got[key], ref[key]), ("device", key)
    assert got["refined_names"] == NAMES4
    host = spart_amd.retrieve(d, obs, K, summary="host", **kw)
    for key in ("idx", "cost", "median") + REFINED:
        assert same_typed(host[key], ref[key]), ("host", key)
    for chunk in (M, 64, 7, 1):
        res = spart_amd.retrieve_stream(d, obs, K, chunk=chunk, **kw)
        for key in ("mean", "median", "std", "count") + REFINED:
            assert same_typed(res[key], ref[key]), ("stream", chunk, key)
        assert same_typed(res["best_cost"], ref["cost"][:, 0]) and res["refined_names"] == NAMES4
    assert eng.calls[ENTRY] == before[0] + 2 + (1 + 2 + 14 + 96) and eng.calls["spart_refine"] == before[1]
    if dtype == "float64":
        bare = dict(kw, refine_opts={"n_iter": 0, "band_model": "srf"})
        got = spart_amd.retrieve(d, obs, K, summary="device", **bare)
        assert same_typed(got["refined_cost0"], start["refined_cost0"]) and same_typed(got["refined_cost0"][matched], got["cost"][matched, 0])
        res = spart_amd.retrieve_stream(d, obs, K, chunk=40, **bare)
        assert same_typed(res["refined_cost0"], start["refined_cost0"]) and same_typed(res["refined_cost0"][matched], res["best_cost"][matched])
        assert np.isnan(res["refined_cost0"][~matched]).all() and np.isinf(res["best_cost"][~matched]).all()
    # the refusals, with a device at hand
    for call in (spart_amd.retrieve, spart_amd.retrieve_stream):
        with pytest.raises(ValueError, match="srf"):
            call(d, obs, K, column=column, weights=w, refine=NAMES4)
        with pytest.raises(ValueError, match="srf"):
            call(d, obs, K, column=column, weights=w, refine=NAMES4, refine_opts={"band_model": "centre"})
    assert eng.calls["spart_refine"] == before[1]


# ---- 8. the twin experiment on the GPU
def test_twin_experiment_on_the_gpu(torch_mod, engines):
    """tests/test_refine_srf_host.py's experiment with the engine's own SRF columns as the truth, through Engine.refine: the SRF
    model started 15 % of the range away returns to the truth in every row (cost <= 1e-8 cost0, |x - truth| <= 1e-6 of the range,
    no exceptions); the centre model started AT the truth leaves it in every row by >= 1 % of the range in some parameter, with
    a median error per parameter of >= 2 %."""
    from spart_amd import workloads
    eng = engines["s2"]
    free = cols_of(NAMES4)
    lo, hi = bounds_of(NAMES4)
    truth = workloads.lhs_params(48, "full", seed=5)
    obs = srf_forward_of(torch_mod, eng, "R_TOC")(truth)
    assert np.isfinite(obs).all()
    start = truth.copy()
    start[:, free] = truth[:, free] + 0.15 * (hi - lo) * np.sign(0.5 * (lo + hi) - truth[:, free])
    up = lambda a: torch_mod.as_tensor(np.ascontiguousarray(a.T), device=eng.device)      # noqa: E731
    res = {k: v.cpu().numpy() for k, v in eng.refine(up(start), obs, NAMES4, n_iter=10, band_model="srf").items() if k != "names"}
    err = np.abs(res["x"] - truth[:, free]) / (hi - lo)
    print("srf model: max cost / cost0", float((res["cost"] / res["cost0"]).max()), " max |x - truth| / range", float(err.max()),
          " accepted steps", int(res["n_accept"].min()), "...", int(res["n_accept"].max()))
    assert (res["n_accept"] >= 0).all() and (res["cost"] <= res["cost0"]).all()
    assert (res["cost"] <= 1e-8 * res["cost0"]).all(), float((res["cost"] / res["cost0"]).max())
    assert (err <= 1e-6).all(), float(err.max())
    off = {k: v.cpu().numpy() for k, v in eng.refine(up(truth), obs, NAMES4, n_iter=10).items() if k != "names"}
    e = np.abs(off["x"] - truth[:, free]) / (hi - lo)
    print("centre model from the truth: median error / range per parameter", np.median(e, axis=0), " worst parameter of the best row",
          float(e.max(axis=1).min()), " median cost0", float(np.median(off["cost0"])), "-> cost", float(np.median(off["cost"])))
    assert (off["n_accept"] >= 1).all() and (off["cost"] < off["cost0"]).all()
    assert (e.max(axis=1) >= 0.01).all(), float(e.max(axis=1).min())
    assert (np.median(e, axis=0) >= 0.02).all(), np.median(e, axis=0)
