"""spart_refine_views on the GPU: the raw C ABI against the definition tools/refine_views_defined.py, bit for bit, with the
library's own float64 pruned column path as the definition's forward model (helpers/refine_calls.forward_of): every shape of
shared / local unknowns, the view boundaries inside 16-band tiles, the special pixels, V = 1 against spart_refine /
spart_refine_srf themselves, the chunk cut, the masked view, the prefix property, Engine.refine_views / spart_amd.refine_views,
the refusals and the example.  If a mismatch shows here and not in tests/test_refine_views_host.py, the cause is in the kernel's
index maps or in contraction, not in the formula."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import F16, FILL, OUTS, S2, rd, refine_call, same
from helpers.refine_srf_calls import raw_refine
from helpers.refine_views_calls import call_views, check_views, defined_views, make_views_case, not_vacuous, views_call

pytestmark = pytest.mark.gpu
M = 67             # not a multiple of 4 or 8: the last group is partial

# (V, shared, local, weights, prior, column, n_iter): nb = 13 puts the view boundaries of V >= 2 inside 16-band tiles
SHAPES = [(1, ["LAI", "Cab"], [], "none", "none", 0, 4),
          (2, ["LAI", "Cab"], [], "shared", "shared", 1, 1),
          (3, ["LAI", "Cab", "LIDFa"], ["aot550"], "per_pixel", "none", 0, 4),
          (3, ["LAI", "Cab", "Cw", "Cdm"], ["aot550", "uh2o", "uo3", "SMp"], "per_pixel", "per_pixel", 2, 1),
          (5, ["Cab"], ["LAI", "aot550"], "shared", "none", 1, 4),
          (2, [], ["LAI", "aot550"], "per_pixel", "shared", 2, 0),
          (64, ["LAI"], [], "none", "per_pixel", 0, 1),
          (4, F16, [], "per_pixel", "none", 1, 1)]


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {"s2": get_engine(S2, 0), "hyper": get_engine(None, 0, sensor_info=hyper_si)}


@pytest.fixture(scope="module")
def masked(torch_mod, engines):
    """V = 3, Fs = 3, Fl = 1 with per-pixel weights: the case of the masked-view, prefix and Engine tests, and its definition"""
    case = make_views_case(torch_mod, engines["s2"], ["LAI", "Cab", "LIDFa"], ["aot550"], M, 3, "R_TOC", "per_pixel", "none", 41)
    hist = []
    return case, defined_views(torch_mod, engines["s2"], case, 0, 5, history=hist), hist


@pytest.mark.parametrize("V,shared,local,kind,prior,column,n_iter", SHAPES, ids=[f"V{s[0]}-Fs{len(s[1])}-Fl{len(s[2])}" for s in SHAPES])
def test_definition_bit_for_bit(torch_mod, engines, V, shared, local, kind, prior, column, n_iter):
    eng = engines["s2"]
    case = make_views_case(torch_mod, eng, shared, local, M, V, ("R_TOC", "R_TOA", "L_TOA")[column], kind, prior, 7 * V + len(shared))
    ref, _ = check_views(torch_mod, eng, case, column, n_iter, (V, shared, local))
    Fs, Fl = len(shared), len(local)
    assert ref["n_accept"][1] == -1 and np.isnan(ref["std"][1]).all() and ref["n_accept"][0] >= 0       # NaN fixed parameter; outside start
    assert (ref["x"][0, 0] <= case["hi"][0]) and np.isfinite(ref["x"][0]).all()                        # (view 1's NaN shared entry not read)
    if kind == "per_pixel":
        assert ref["n_accept"][2] == -1 and ref["n_accept"][3] >= 0
        if Fl and prior == "none":
            own = slice(Fs + (V - 1) * Fl, Fs + V * Fl)
            start = rd.clip_defined(case["base"][V - 1, 3, case["local"]], case["lo"][Fs:], case["hi"][Fs:])
            assert same(ref["x"][3, own], start) and np.isnan(ref["std"][3]).all()
    if Fl:
        assert ref["n_accept"][4] >= 0


def test_hyperspectral_sensor_two_views(torch_mod, engines):
    """nb = 211 is no multiple of 16: view 1 starts inside the 14th tile"""
    eng = engines["hyper"]
    assert eng.nb % 16 != 0
    case = make_views_case(torch_mod, eng, ["LAI", "Cab"], ["aot550"], 19, 2, "R_TOC", "per_pixel", "shared", 3)
    check_views(torch_mod, eng, case, 0, 2, "hyper")


def test_one_view_is_spart_refine_itself(torch_mod, engines):
    eng = engines["s2"]
    for shared, local, kind, column in ((["LAI", "Cab", "Cw"], [], "per_pixel", 0), (["LAI"], ["Cab", "aot550"], "shared", 1)):
        case = make_views_case(torch_mod, eng, shared, local, M, 1, ("R_TOC", "R_TOA")[column], kind, "none", 11 + column)
        got = call_views(torch_mod, eng, case, column, 3)
        w = case["w"]
        rc, ref = refine_call(torch_mod, eng, case["base"][0], case["shared"] + case["local"], case["lo"], case["hi"], case["obs"][:, 0],
                              w if w is None or w.ndim == 1 else w[:, 0], column=column, n_iter=3)
        assert rc == 0
        for k in OUTS:
            assert same(got[k].reshape(ref[k].shape), ref[k]), (shared, local, k)
        assert (ref["n_accept"] >= 1).mean() >= 0.5
    # band_model = 1 against spart_refine_srf
    case = make_views_case(torch_mod, eng, ["LAI", "Cab"], [], 19, 1, "R_TOC", "none", "shared", 5, srf=True)
    got = call_views(torch_mod, eng, case, 0, 2, band_model=1)
    rc, ref = raw_refine(torch_mod, eng, "spart_refine_srf", case["base"][0], case["shared"], case["lo"], case["hi"], case["obs"][:, 0],
                         None, case["mean"], case["weight"], column=0, n_iter=2)
    assert rc == 0 and all(same(got[k].reshape(ref[k].shape), ref[k]) for k in OUTS) and (ref["n_accept"] >= 1).mean() >= 0.5


def test_srf_columns_two_views(torch_mod, engines):
    eng = engines["s2"]
    case = make_views_case(torch_mod, eng, ["LAI", "Cab"], ["aot550"], 19, 2, "R_TOA", "shared", "none", 8, srf=True)
    check_views(torch_mod, eng, case, 1, 2, "srf", band_model=1)


def test_chunk_cut_and_guard(torch_mod, engines):
    """V = 64, Fs = 16: a chunk is (1 << 19) // (17 * 64) = 481 pixels, so M = 484 runs a chunk of 481 and one of 3; the special
    pixels sit at 480 ... 483, on both sides of the cut"""
    eng = engines["s2"]
    assert (1 << 19) // (17 * 64) == 481
    case = make_views_case(torch_mod, eng, F16, [], 484, 64, "R_TOC", "per_pixel", "none", 9, at=480)
    ref, _ = check_views(torch_mod, eng, case, 0, 1, "chunk cut", guard=True)
    assert list(ref["n_accept"][480:484] >= 0) == [True, False, False, True]
    size = lambda m, v=64, f=16, fs=16: int(eng.lib.spart_views_workspace_bytes(eng.ctx, m, v, f, fs))      # noqa: E731
    assert size(481) == size(484) == size(2_000_000_000) > size(100) > 0


def test_masked_view_prior_and_prefix(torch_mod, engines, masked):
    eng = engines["s2"]
    case, ref5, hist = masked
    not_vacuous(ref5, 5, "masked")
    got5 = call_views(torch_mod, eng, case, 0, 5)
    assert all(same(got5[k], ref5[k]) for k in OUTS)
    start = rd.clip_defined(case["base"][2, 3, case["local"]], case["lo"][3:], case["hi"][3:])
    assert same(got5["x"][3, 5:6], start) and np.isnan(got5["std"][3]).all() and got5["n_accept"][3] >= 1
    # a prior weight on the masked view's local: std is finite
    n = 6
    withp = dict(case, mean=np.full(n, 0.2), weight=np.array([0, 0, 0, 0, 0, 25.0]))
    refp, gotp = check_views(torch_mod, eng, withp, 0, 5, "masked with a prior")
    assert np.isfinite(gotp["std"][3]).all() and refp["n_accept"][3] >= 1
    # the prefix property: n_iter = 3 is where n_iter = 5 was after its fourth decision
    got3 = call_views(torch_mod, eng, case, 0, 3)
    assert same(got3["x"], hist[3][0]) and same(got3["cost"], hist[3][1]) and (got5["cost"] <= got3["cost"])[ref5["n_accept"] >= 0].all()


def test_engine_and_host_form_are_the_raw_call(torch_mod, engines, masked):
    import spart_amd
    eng = engines["s2"]
    case, _, _ = masked
    shared, local = ["LAI", "Cab", "LIDFa"], ["aot550"]
    mean = np.tile(np.array([3.0, 40.0, 0.0, 0.2, 0.2, 0.2]), (M, 1))
    weight = np.tile(np.array([0.25, 0.0, 1.0, 16.0, 16.0, 16.0]), (M, 1))
    raw = call_views(torch_mod, eng, dict(case, mean=mean, weight=weight), 0, 3)
    P = torch_mod.as_tensor(np.ascontiguousarray(np.moveaxis(case["base"], 2, 0)), device=eng.device)          # (27, V, M)
    res = eng.refine_views(P, case["obs"], shared, local, weights=case["w"], n_iter=3, prior_mean=mean, prior_weight=weight)
    for k in OUTS:
        assert same(res[k].cpu().numpy(), raw[k]), k
    assert res["names"] == shared + local and eng.calls["spart_refine_views"] >= 1
    assert same(res["shared"].cpu().numpy(), raw["x"][:, :3]) and same(res["local"].cpu().numpy(), raw["x"][:, 3:].reshape(M, 3, 1))
    assert same(res["shared_std"].cpu().numpy(), raw["std"][:, :3]) and same(res["local_std"].cpu().numpy(), raw["std"][:, 3:].reshape(M, 3, 1))
    # the prior as a dict says the same; the host form takes the 27 entries as a list
    prior = {"LAI": (3.0, 2.0), "LIDFa": (0.0, 1.0), "aot550": (np.full(3, 0.2), 0.25)}          # weight = 1 / sigma^2, exactly
    host = spart_amd.refine_views(list(np.moveaxis(case["base"], 2, 0)), case["obs"], S2, shared, local, weights=case["w"], n_iter=3,
                                  prior=prior)
    assert all(same(host[k], raw[k]) for k in OUTS) and same(host["local"], raw["x"][:, 3:].reshape(M, 3, 1))


def test_refusals_leave_outputs_untouched(torch_mod, engines):
    from spart_amd import get_engine
    eng = engines["s2"]
    case = make_views_case(torch_mod, eng, ["LAI", "Cab"], ["aot550"], 9, 3, "R_TOC", "per_pixel", "none", 2)
    a = (case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], case["w"])
    need = int(eng.lib.spart_views_workspace_bytes(eng.ctx, 9, 3, 3, 2))
    assert need > 0
    INVALID, WORKSPACE, NOSENSOR = -1, -3, -4
    for kw, want in [(dict(V=0), INVALID), (dict(V=65), INVALID), (dict(n_shared=-1), INVALID), (dict(n_shared=4), INVALID),
                     (dict(V=15), INVALID), (dict(n_shared=0, V=6), INVALID), (dict(band_model=2), INVALID), (dict(band_model=-1), INVALID),
                     (dict(F=0), INVALID), (dict(F=17), INVALID), (dict(M=-1), INVALID), (dict(n_iter=101), INVALID), (dict(column=3), INVALID),
                     *[(dict(null=(k,)), INVALID) for k in ("base", "free", "lo", "hi", "obs", "opt", "x", "cost")],
                     (dict(ctx=None), INVALID), (dict(null=("ws",)), WORKSPACE), (dict(ws_bytes=need - 1), WORKSPACE),
                     (dict(ctx=get_engine(None, 0).ctx), NOSENSOR)]:
        rc, got = views_call(torch_mod, eng, *a, **kw)
        assert rc == want, (kw, rc, eng.lib.spart_last_error(eng.ctx))
        assert all((got[k] == FILL).all() for k in OUTS), kw
    rc, got = views_call(torch_mod, eng, *a, M=0)
    assert rc == 0 and all((got[k] == FILL).all() for k in OUTS)
    size = lambda m=9, v=3, f=3, fs=2, ctx=eng.ctx: int(eng.lib.spart_views_workspace_bytes(ctx, m, v, f, fs))      # noqa: E731
    for bad in (dict(m=0), dict(m=-1), dict(v=0), dict(v=65), dict(f=0), dict(f=17), dict(fs=-1), dict(fs=4), dict(v=15), dict(v=6, fs=0),
                dict(ctx=get_engine(None, 0).ctx), dict(ctx=None)):
        assert size(**bad) == 0, bad
    assert size(v=64, f=16, fs=16) > 0 and size(v=16, f=1, fs=0) > 0 and size(v=1, f=16, fs=0) > 0 and size(v=64, f=1, fs=1) > 0


def test_the_first_refusal_wins(torch_mod, engines):
    """calls with two faults: the one that is checked first is the one reported, and nothing is written"""
    eng = engines["s2"]
    case = make_views_case(torch_mod, eng, ["LAI", "Cab"], ["aot550"], 9, 3, "R_TOC", "per_pixel", "none", 2)
    a = (case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], case["w"])
    twice = (case["base"], case["shared"], case["shared"][:1], case["lo"], case["hi"], case["obs"], case["w"])     # F = 3, column 0 twice
    for args, kw, text in [(a, dict(F=17, null=("free",)), "F = 17, expected"),
                           (a, dict(M=-1, F=0), "M = -1, expected"),
                           (a, dict(V=0, column=3), "V = 0, expected"),
                           (a, dict(band_model=2, n_iter=101), "band_model = 2"),
                           (twice, dict(n_shared=4), "n_shared = 4, expected")]:
        rc, got = views_call(torch_mod, eng, *args, **kw)
        msg = eng.lib.spart_last_error(eng.ctx).decode()
        assert rc == -1 and msg.startswith(f"spart_refine_views: {text}"), (kw, rc, msg)
        assert all((got[k] == FILL).all() for k in OUTS), kw


@pytest.mark.parametrize("sensor", ["s2", "hyper"])
def test_one_view_is_sized_like_spart_refine(engines, sensor):
    """V = 1 carves spart_refine's workspace: the same bytes for every M around the chunk and for either n_shared"""
    eng = engines[sensor]
    for F in (1, 7, 16):
        c = (1 << 19) // (F + 1)
        for M in (1, c - 1, c, c + 1, 2_000_000_000):
            one = int(eng.lib.spart_refine_workspace_bytes(eng.ctx, M, F))
            assert one > 0, (F, M)
            for n_shared in (F, 0):
                assert int(eng.lib.spart_views_workspace_bytes(eng.ctx, M, 1, F, n_shared)) == one, (F, M, n_shared)


def test_refine_views_example_runs():
    """examples/refine_views.py as a user runs it: its own process, exit code 0, the expected last line"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_views.py"), "256"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "joint fit" in r.stdout and "fitted 3 shared parameters of 256 pixels from 3 views" in r.stdout
