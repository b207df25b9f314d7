"""spart_refine_mix on the GPU: the raw C ABI against the definition tools/refine_mix_defined.py, bit for bit in all eight
outputs, with the engine's own forward call as the definition's forward model: every shape of shared / local / masked unknowns
with given and fitted fractions, the planted pixels, 13, 21 and 211 bands, the SRF band model, one component against
spart_refine / spart_refine_srf themselves, fractions (1, 0) against spart_refine, the simplex, the chunk cut, the prefix
property, the refusals, Engine.refine_mix / spart_amd.refine_mix and the example.  If a mismatch shows here and not in
tests/test_refine_mix_host.py, the cause is in the kernel's index maps or in contraction, not in the formula."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import FILL, S2, refine_call
from helpers.refine_mix_calls import OUTS, call_mix, check_mix, defined_mix, make_mix_case, mix_call, not_vacuous, same
from helpers.refine_srf_calls import raw_refine

pytestmark = pytest.mark.gpu
FIT_OUTS = OUTS[:6]
CROP_SOIL = [[1, 1], [0, 0]]

# (V, shared, local, mask, fitted, weights, prior, column, n_iter, M): an n_iter = 1 case starts far away with lambda0 = 1e-9
SHAPES = [(1, [], ["LAI", "Cab", "Cw"], None, False, "none", "none", 0, 4, 63),
          (2, ["B"], ["LAI", "Cab"], CROP_SOIL, True, "per_pixel", "shared", 0, 4, 65),
          (2, ["B", "aot550"], ["LAI"], None, False, "shared", "per_pixel", 1, 1, 70),
          (3, [], ["LAI"], [[1], [0], [1]], True, "per_pixel", "none", 2, 4, 63),
          (4, ["B"], ["LAI", "Cab", "Cw"], None, True, "shared", "shared", 0, 1, 65),
          (8, ["B"], ["LAI"], None, True, "none", "per_pixel", 1, 4, 70),
          (8, ["B", "SMp", "aot550", "uo3", "uh2o", "Cdm", "N", "LIDFa", "q"], [], None, True, "per_pixel", "none", 2, 0, 63)]


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {"s2": get_engine(S2, 0), "olci": get_engine("Sentinel3A-OLCI", 0), "hyper": get_engine(None, 0, sensor_info=hyper_si)}


def far(n_iter):
    """what makes one proposal enough to see an accepted and a rejected step: a start far away, almost no damping and a prior
    too weak to hold the step back"""
    return dict(move=0.35, lambda0=1e-9, prior_sigma=3.0) if n_iter == 1 else {}


@pytest.fixture(scope="module")
def crop_soil(torch_mod, engines):
    """V = 2 crop / soil with fitted fractions: the case of the prefix, single-output and Engine tests, and its definition"""
    case = make_mix_case(torch_mod, engines["s2"], 2, ["B"], ["LAI", "Cab"], CROP_SOIL, True, 65, "R_TOC", "per_pixel", "none", 41)
    hist = []
    return case, defined_mix(torch_mod, engines["s2"], case, 0, 5, history=hist), hist


@pytest.mark.parametrize("V,shared,local,mask,fit,kind,prior,column,n_iter,M", SHAPES,
                         ids=[f"V{s[0]}-Fs{len(s[1])}-Fl{len(s[2])}-{'fit' if s[4] else 'given'}" for s in SHAPES])
def test_definition_bit_for_bit(torch_mod, engines, V, shared, local, mask, fit, kind, prior, column, n_iter, M):
    eng = engines["s2"]
    case = make_mix_case(torch_mod, eng, V, shared, local, mask, fit, M, ("R_TOC", "R_TOA", "L_TOA")[column], kind, prior,
                         7 * V + len(shared), **far(n_iter))
    ref, _ = check_mix(torch_mod, eng, case, column, n_iter, (V, shared, local))
    assert ref["n_accept"][0] >= 0 and np.isfinite(ref["x"][0]).all() and ref["x"][0, 0] <= case["hi"][0]      # the NaNs are not read
    assert ref["n_accept"][1] == -1 and np.isnan(ref["std"][1]).all()
    if fit and V >= 3:
        assert np.isposinf(ref["cost"][3]) and np.isposinf(ref["cost0"][3]) and ref["frac"][3, -1] < 0
    live = ref["n_accept"] >= 0
    if fit:
        assert (np.abs(ref["frac"][live].sum(axis=1) - 1.0) <= 2.0 ** -52).all() and (ref["frac"][live, -1] >= 0).all()


@pytest.mark.parametrize("sensor,M", [("olci", 63), ("hyper", 65)])
def test_other_band_counts(torch_mod, engines, sensor, M):
    """21 bands: one whole 16-band tile and a partial one; 211 bands: 13 tiles and a partial one"""
    eng = engines[sensor]
    assert eng.nb == (21 if sensor == "olci" else 211) and eng.nb % 16 != 0
    case = make_mix_case(torch_mod, eng, 2, ["B"], ["LAI", "Cab"], CROP_SOIL, True, M, "R_TOC", "per_pixel", "shared", 3)
    check_mix(torch_mod, eng, case, 0, 4, sensor)


def test_srf_band_model(torch_mod, engines):
    eng = engines["s2"]
    case = make_mix_case(torch_mod, eng, 2, ["B"], ["LAI", "Cab"], CROP_SOIL, True, 63, "R_TOA", "shared", "none", 8, srf=True)
    check_mix(torch_mod, eng, case, 1, 4, "srf", band_model=1)


def test_one_component_is_spart_refine_itself(torch_mod, engines):
    """consequence (a), against the existing entry points, with and without fit_fractions"""
    eng = engines["s2"]
    for shared, local, kind, column, fit in ((["LAI", "Cab", "Cw"], [], "per_pixel", 0, True), (["B"], ["LAI", "Cab"], "shared", 1, False)):
        case = make_mix_case(torch_mod, eng, 1, shared, local, None, fit, 63, ("R_TOC", "R_TOA")[column], kind, "none", 11 + column)
        case["frac"] = np.ones((63, 1))
        got = call_mix(torch_mod, eng, case, column, 3)
        rc, ref = refine_call(torch_mod, eng, case["base"][0], case["shared"] + case["local"], case["lo"], case["hi"], case["obs"],
                              case["w"], column=column, n_iter=3)
        assert rc == 0
        for k in FIT_OUTS:
            assert same(got[k], ref[k]), (shared, local, k)
        assert same(got["y_comp"][:, 0], ref["y"]) and (got["frac"] == 1.0).all() and (ref["n_accept"] >= 1).mean() >= 0.5
    case = make_mix_case(torch_mod, eng, 1, ["LAI", "Cab"], [], None, True, 63, "R_TOC", "none", "shared", 5, srf=True)
    got = call_mix(torch_mod, eng, case, 0, 2, band_model=1)
    rc, ref = raw_refine(torch_mod, eng, "spart_refine_srf", case["base"][0], case["shared"], case["lo"], case["hi"], case["obs"], None,
                         case["mean"], case["weight"], column=0, n_iter=2)
    assert rc == 0 and all(same(got[k], ref[k]) for k in FIT_OUTS) and (ref["n_accept"] >= 1).mean() >= 0.5


def test_fractions_one_zero_are_spart_refine_of_component_zero(torch_mod, engines):
    """consequence (b): given fractions (1, 0), the locals active in component 0 only, positive finite spectra of component 1"""
    eng = engines["s2"]
    case = make_mix_case(torch_mod, eng, 2, ["B"], ["LAI", "Cab"], CROP_SOIL, False, 63, "R_TOC", "per_pixel", "none", 21)
    case["frac"] = np.tile([1.0, 0.0], (63, 1))
    from spart_amd import workloads
    case["base"][1] = np.repeat(workloads.default_row(), 63, axis=0)              # component 1: a finite, positive spectrum
    case["base"][0, 1, 20] = np.nan                                               # component 0's pixel 1 is dead
    got = call_mix(torch_mod, eng, case, 0, 3)
    assert np.isfinite(got["y_comp"][:, 1]).all() and (got["y_comp"][:, 1] > 0).all()
    rc, ref = refine_call(torch_mod, eng, case["base"][0], case["shared"] + case["local"], case["lo"], case["hi"], case["obs"], case["w"],
                          column=0, n_iter=3)
    assert rc == 0
    for k in FIT_OUTS:
        assert same(got[k], ref[k]), k
    assert (ref["n_accept"] >= 1).mean() >= 0.5 and ref["n_accept"][1] == -1 and ref["n_accept"][2] == -1


def test_the_simplex(torch_mod, engines):
    """three components, a true last fraction below 0.03 and 2 % noise: on the definition alone, some trial is infeasible and no
    live pixel ends with a negative fraction; then the library against the definition"""
    eng = engines["s2"]
    case = make_mix_case(torch_mod, eng, 3, [], ["LAI"], [[1], [0], [1]], True, 63, "R_TOC", "none", "none", 13, noise=0.02,
                         last_below=0.03)
    case["frac"] = np.where(np.isnan(case["frac"]), np.nan, case["a"])            # start on the truth, next to the edge
    case["frac"][3, :2] = 0.8
    hist = []
    ref = defined_mix(torch_mod, eng, case, 0, 4, history=hist)
    live = ref["n_accept"] >= 0
    infeasible = sum(int((~h[2][live]).sum()) for h in hist)
    print(f"[refine_mix] simplex: {infeasible} infeasible trials of {int(live.sum())} live pixels in 5 decisions")
    assert infeasible >= 1 and (ref["frac"][live] >= 0.0).all() and live.sum() >= 55
    got = call_mix(torch_mod, eng, case, 0, 4)
    for k in OUTS:
        assert same(got[k], ref[k]), k


def test_chunk_cut_and_guard(torch_mod, engines):
    """V = 8, Fs = 9: a chunk is (1 << 19) // (10 * 8) = 6553 pixels, so M = 6560 runs a chunk of 6553 and one of 7, the planted
    pixels on both sides of the cut; the bytes behind the workspace survive, and a pixel's bits are those of the same pixel in a
    batch of 70, which are the definition's"""
    eng = engines["s2"]
    assert (1 << 19) // (10 * 8) == 6553
    V, shared = SHAPES[6][0], SHAPES[6][1]
    case = make_mix_case(torch_mod, eng, V, shared, [], None, True, 6560, "R_TOA", "per_pixel", "none", 9, at=6551)
    big = call_mix(torch_mod, eng, case, 1, 1, guard=True)
    pick = np.r_[0:30, 6530:6560, 3000:3010]
    sub = dict(case, base=case["base"][:, pick], obs=case["obs"][pick], frac=case["frac"][pick], w=case["w"][pick],
               planted={list(pick).index(m) for m in case["planted"]})
    ref, small = check_mix(torch_mod, eng, sub, 1, 1, "chunk cut, batch of 70")
    for k in OUTS:
        assert same(big[k][pick], small[k]), k
    assert list(big["n_accept"][6551:6556] >= 0) == [True, False, False, False, True]
    size = lambda m, v=8, f=9, n=16: int(eng.lib.spart_mix_workspace_bytes(eng.ctx, m, v, f, n))      # noqa: E731
    assert size(6553) == size(6560) == size(2_000_000_000) > size(100) > 0


def test_prefix_cost_and_single_outputs(torch_mod, engines, crop_soil):
    eng = engines["s2"]
    case, ref5, hist = crop_soil
    not_vacuous(ref5, case, 5, "crop / soil")
    got5 = call_mix(torch_mod, eng, case, 0, 5)
    assert all(same(got5[k], ref5[k]) for k in OUTS)
    live = ref5["n_accept"] >= 0
    assert (got5["cost"][live] <= got5["cost0"][live]).all()
    # the prefix property: n_iter = 3 is where n_iter = 5 was after its fourth decision
    got3 = call_mix(torch_mod, eng, case, 0, 3)
    assert same(got3["x"], hist[3][0]) and same(got3["cost"], hist[3][1]) and (got5["cost"] <= got3["cost"])[live].all()
    # every optional output alone, the others NULL
    for k in OUTS[2:]:
        one = call_mix(torch_mod, eng, case, 0, 3, only=(k,))
        assert same(one[k], got3[k]) and same(one["x"], got3["x"]) and same(one["cost"], got3["cost"]), k
        assert all((one[o] == FILL).all() for o in OUTS[2:] if o != k), k


def test_refusals_leave_outputs_untouched(torch_mod, engines):
    from spart_amd import get_engine
    eng = engines["s2"]
    case = make_mix_case(torch_mod, eng, 3, ["B"], ["LAI", "Cab"], None, True, 63, "R_TOC", "per_pixel", "none", 2)
    a = (case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], case["frac"])
    kw0 = dict(w=case["w"])
    need = int(eng.lib.spart_mix_workspace_bytes(eng.ctx, 63, 3, 3, 9))
    assert need > 0
    INVALID, WORKSPACE, NOSENSOR = -1, -3, -4
    for kw, want in [(dict(V=0), INVALID), (dict(V=9), INVALID), (dict(n_shared=-1), INVALID), (dict(n_shared=4), INVALID),
                     (dict(band_model=2), INVALID), (dict(band_model=-1), INVALID), (dict(fit=2), INVALID), (dict(fit=-1), INVALID),
                     (dict(active=[[1, 1], [2, 1], [1, 1]]), INVALID), (dict(active=[[1, 0], [1, 0], [1, 0]]), INVALID),
                     (dict(V=8), INVALID), (dict(frac_lo=0.5, frac_hi=0.5), INVALID), (dict(frac_lo=-0.1, frac_hi=1.0), INVALID),
                     (dict(frac_lo=0.2, frac_hi=1.5), INVALID), (dict(null=("frac",)), INVALID),
                     (dict(F=0), INVALID), (dict(F=17), INVALID), (dict(M=-1), INVALID), (dict(n_iter=101), INVALID), (dict(column=3), INVALID),
                     *[(dict(null=(k,)), INVALID) for k in ("base", "free", "lo", "hi", "obs", "opt", "out", "x", "cost")],
                     (dict(ctx=None), INVALID), (dict(null=("ws",)), WORKSPACE), (dict(ws_bytes=need - 1), WORKSPACE),
                     (dict(ctx=get_engine(None, 0).ctx), NOSENSOR)]:
        rc, got = mix_call(torch_mod, eng, *a, **{**kw0, **kw})
        assert rc == want, (kw, rc, eng.lib.spart_last_error(eng.ctx))
        assert all((got[k] == FILL).all() for k in OUTS), kw
    rc, got = mix_call(torch_mod, eng, *a, M=0, **kw0)
    assert rc == 0 and all((got[k] == FILL).all() for k in OUTS)
    size = lambda m=63, v=3, f=3, n=9, ctx=eng.ctx: int(eng.lib.spart_mix_workspace_bytes(ctx, m, v, f, n))      # noqa: E731
    for bad in (dict(m=0), dict(m=-1), dict(v=0), dict(v=9), dict(f=0), dict(f=17), dict(n=0), dict(n=17),
                dict(ctx=get_engine(None, 0).ctx), dict(ctx=None)):
        assert size(**bad) == 0, bad
    assert size(v=8, f=16, n=16) > 0 and size(v=1, f=1, n=1) > 0
    assert size(v=1, f=5, n=5) == int(eng.lib.spart_refine_workspace_bytes(eng.ctx, 63, 5))


def test_the_first_refusal_wins(torch_mod, engines):
    """calls with two faults: the one that is checked first is the one reported, and nothing is written"""
    eng = engines["s2"]
    case = make_mix_case(torch_mod, eng, 3, ["B"], ["LAI", "Cab"], None, True, 63, "R_TOC", "none", "none", 2)
    a = (case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], case["frac"])
    for kw, text in [(dict(F=17, null=("free",)), "F = 17, expected"), (dict(M=-1, F=0), "M = -1, expected"),
                     (dict(V=0, column=3), "V = 0, expected"), (dict(n_shared=4, band_model=2), "n_shared = 4, expected"),
                     (dict(band_model=2, fit=2), "band_model = 2"), (dict(fit=2, active=[[2, 1], [1, 1], [1, 1]]), "fit_fractions = 2"),
                     (dict(active=[[2, 0], [1, 0], [1, 0]]), "local_active[0] = 2"),
                     (dict(active=[[1, 0], [1, 0], [1, 0]], frac_lo=0.5, frac_hi=0.5), "a local name is active in no component"),
                     (dict(V=8, frac_lo=0.5, frac_hi=0.5), "the unknowns per pixel"),
                     (dict(frac_lo=0.5, frac_hi=0.5, null=("frac",)), "fraction box"), (dict(null=("frac",), n_iter=101), "frac is null"),
                     (dict(n_iter=101, null=("obs",)), "n_iter = 101")]:
        rc, got = mix_call(torch_mod, eng, *a, **kw)
        msg = eng.lib.spart_last_error(eng.ctx).decode()
        assert rc == -1 and msg.startswith(f"spart_refine_mix: {text}"), (kw, rc, msg)
        assert all((got[k] == FILL).all() for k in OUTS), kw


def test_engine_and_host_form_are_the_raw_call(torch_mod, engines, crop_soil):
    import spart_amd
    eng = engines["s2"]
    case, _, _ = crop_soil
    M = 65
    shared, local = ["B"], ["LAI", "Cab"]
    n = 4
    mean = np.tile(np.array([0.5, 3.0, 40.0, 0.5]), (M, 1))
    weight = np.tile(np.array([4.0, 0.25, 0.0, 16.0]), (M, 1))
    raw = call_mix(torch_mod, eng, dict(case, mean=mean, weight=weight), 0, 3)
    P = torch_mod.as_tensor(np.ascontiguousarray(np.moveaxis(case["base"], 2, 0)), device=eng.device)          # (27, V, M)
    prior = {"B": (0.5, 0.5), "LAI": (3.0, 2.0), "fractions": (0.5, 0.25)}                                      # weight = 1 / sigma^2, exactly
    res = eng.refine_mix(P, case["obs"], shared, local, active=np.array(CROP_SOIL), fractions=case["frac"], weights=case["w"], n_iter=3,
                         prior=prior)
    for k, r in zip(("x", "cost", "cost0", "std", "n_accept", "y", "fractions", "y_comp"), OUTS):
        assert same(res[k].cpu().numpy(), raw[r]), k
    assert res["names"] == shared + local and eng.calls["spart_refine_mix"] >= 1 and raw["x"].shape == (M, n)
    host = spart_amd.refine_mix(list(np.moveaxis(case["base"], 2, 0)), case["obs"], S2, shared, local, active={"LAI": [0], "Cab": [0]},
                                fractions=case["frac"], weights=case["w"], n_iter=3, prior=prior)
    assert all(same(host[k], raw[r]) for k, r in zip(("x", "cost", "cost0", "std", "n_accept", "y", "fractions", "y_comp"), OUTS))
    assert same(host["shared"], raw["x"][:, :1]) and same(host["shared_std"], raw["std"][:, :1])
    assert same(host["fractions_std"], raw["std"][:, 3:]) and host["local"].shape == (M, 2, 2)
    assert same(host["local"][:, 0], raw["x"][:, 1:3]) and same(host["local_std"][:, 0], raw["std"][:, 1:3])
    assert same(host["local"][:, 1], case["base"][1][:, case["local"]]) and np.isnan(host["local_std"][:, 1]).all()


def test_example_runs_and_the_mixture_beats_one_canopy(torch_mod):
    """examples/refine_mix.py as a user runs it, then its twin data: the fitted fraction is nearer the truth than the start, and
    the mixture's cost is below the single-canopy fit's on more than half of the pixels"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_mix.py"), "128"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cover fraction" in r.stdout and "fitted 128 pixels as a mixture of 2 components" in r.stdout
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import refine_mix as ex
    import spart_amd
    truth, frac, start, frac0 = ex.twin(128)
    obs = ex.observe(truth, frac, S2)
    single = spart_amd.refine(start[0].T, obs, S2, ex.SHARED + ex.LOCAL, n_iter=10)
    mix = spart_amd.refine_mix(np.moveaxis(start, 2, 0), obs, S2, ex.SHARED, ex.LOCAL, active=ex.ACTIVE,
                               fractions=np.stack([frac0, 1.0 - frac0], axis=1), n_iter=10)
    before, after = np.median(np.abs(frac0 - frac)), np.median(np.abs(mix["fractions"][:, 0] - frac))
    print(f"[refine_mix] example twin: median |fraction - truth| {before:.4f} -> {after:.4f}; "
          f"mixture cost below one canopy's on {(mix['cost'] < single['cost']).mean():.2f} of the pixels")
    assert after < before and (mix["cost"] < single["cost"]).mean() > 0.5
