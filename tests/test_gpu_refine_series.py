"""spart_refine_series on the GPU: the raw C ABI against the definition tools/refine_series_defined.py, bit for bit in all ten
outputs, with the library's own float64 pruned column path as the definition's forward model: every shape of shared / local
unknowns at M = 67 in series of 1, 2, 7, 8, 9, 39 and 1 rows with the three link kinds and the special rows, the 211-band
sensor and the SRF model, gamma = 0 against spart_refine_tiles itself, one-row series against spart_refine / spart_refine_srf,
dead series, a series run alone and the prefix, the chunk cut, a maximal series, the refusals, Engine.refine_series /
spart_amd.refine_series and the example.  If a mismatch shows here and not in tests/test_refine_series_host.py, the cause is in
the kernels' index maps, their staging or their order of summation, not in the formula."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import F16, FILL, S2, rd, same
from helpers.refine_series_calls import (LENGTHS, ROW_KEYS, SERIES_KEYS, call_series, check_series, defined_series, differing,
                                         make_series_case, not_vacuous, series_call)
from helpers.refine_srf_calls import raw_refine
from helpers.refine_tiles_calls import OUTS, call_tiles, fwd_of

pytestmark = pytest.mark.gpu
M = 67
F15 = [n for n in F16 if n != "LAI"]

# (shared, local, weights, local prior, shared prior, link, column, n_iter, seed, further arguments of the case).  A first step
# from a start near the truth at the default damping is never rejected, so the n_iter = 1 case starts up to half the range away
# with lambda0 = 1e-9; the n_iter = 4 cases take their rejection where the fit has converged or a far start overshoots.
SHAPES = [([], ["LAI"], "per_pixel", "none", "none", "none", 0, 4, 1, dict(move=0.5)),
          (["LIDFa"], ["LAI", "Cab"], "none", "none", "shared", "varied", 1, 4, 2, dict(move=0.5)),
          (["LIDFa", "SMp"], ["LAI", "Cab"], "per_pixel", "per_row", "none", "zero", 0, 1, 3, dict(move=0.5, lambda0=1e-9)),
          (["aot550", "uh2o", "LIDFa", "SMp"], ["LAI", "Cab", "Cw", "Cdm"], "shared", "shared", "per_row", "varied", 2, 4, 4, dict(move=0.5)),
          ([], F16, "per_pixel", "shared", "none", "zero", 1, 4, 5, dict(move=1.0, lambda0=1e-4)),
          (F15, ["LAI"], "shared", "per_row", "shared", "none", 0, 0, 6, {})]


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {"s2": get_engine(S2, 0), "hyper": get_engine(None, 0, sensor_info=hyper_si)}


def case_of(torch, eng, shared, local, kind, lprior, sprior, link, column, seed, sizes=LENGTHS, srf=False, **kw):
    kw.setdefault("special", 12)                # rows 12, 13, 14 of the series of 8 (rows 10 ... 17)
    return make_series_case(fwd_of(torch, eng, column, srf), shared, local, sizes, kind, lprior, sprior, link, seed, **kw)


@pytest.fixture(scope="module")
def plain(torch_mod, engines):
    """Fs = 1, Fl = 2 on R_TOA with per-row weights and varied links: the case of the alone, prefix, dead and Engine tests"""
    case = case_of(torch_mod, engines["s2"], ["LIDFa"], ["LAI", "Cab"], "per_pixel", "none", "none", "varied", 1, 21, move=0.3)
    hist = []
    return case, defined_series(fwd_of(torch_mod, engines["s2"], 1), case, 5, history=hist), hist


@pytest.mark.parametrize("shared,local,kind,lprior,sprior,link,column,n_iter,seed,more", SHAPES,
                         ids=[f"Fs{len(s[0])}-Fl{len(s[1])}" for s in SHAPES])
def test_definition_bit_for_bit(torch_mod, engines, shared, local, kind, lprior, sprior, link, column, n_iter, seed, more):
    eng = engines["s2"]
    case = case_of(torch_mod, eng, shared, local, kind, lprior, sprior, link, column, seed, **more)
    ref, _ = check_series(torch_mod, eng, case, column, n_iter, (shared, local))
    assert (ref["status"] == 0).all() and (ref["n_accept"] >= 0).all()
    # the start outside the box, the masked date over NaN observations, the NaNs that are never read
    assert np.isfinite(ref["local"]).all() and np.isfinite(ref["shared"]).all()
    assert case["base"][12, (case["shared"] + case["local"])[0]] > case["hi"][0]
    if kind == "per_pixel":
        assert (case["w"][13] == 0.0).all() and np.isnan(case["obs"][13]).all() and (lprior != "none" or ref["pixel_cost"][13] == 0.0)
    if shared:
        assert np.isnan(case["base"][14, case["shared"][0]])
    if link != "none":
        assert np.isnan(case["link"][case["series_start"][1:] - 1]).all()


def test_hyperspectral_sensor(torch_mod, engines):
    eng = engines["hyper"]
    assert eng.nb % 16 != 0
    case = case_of(torch_mod, eng, ["LIDFa"], ["LAI", "Cab"], "per_pixel", "shared", "shared", "varied", 0, 3, sizes=[7, 12, 3], special=8)
    # 211 bands pin three parameters well: every step is accepted until the fit has converged, at 6 proposals and from far starts
    # alike, so the fit runs 20 proposals, by which a converged series proposes a step that no longer lowers its cost
    ref, _ = check_series(torch_mod, eng, case, 0, 20, "hyper")
    assert (ref["n_accept"] >= 1).all()


def test_srf_band_model(torch_mod, engines):
    eng = engines["s2"]
    case = case_of(torch_mod, eng, ["LIDFa"], ["LAI", "Cab"], "per_pixel", "none", "none", "zero", 1, 7, sizes=[9, 2, 12], srf=True, special=3, move=0.5,
                   lambda0=1e-9)
    check_series(torch_mod, eng, case, 1, 6, "srf", band_model=1)


def test_without_smoothing_it_is_spart_refine_tiles_itself(torch_mod, engines, plain):
    """gamma = 0, and separately link = 0 under gamma > 0: every output of spart_refine_tiles on tiles equal to the series"""
    eng = engines["s2"]
    case, _, _ = plain
    tiles = {k: v for k, v in case.items() if k not in ("series_start", "smooth", "link")}
    want = call_tiles(torch_mod, eng, dict(tiles, tile_start=case["series_start"]), 1, 4)
    got = call_series(torch_mod, eng, dict(case, smooth=np.zeros(2)), 1, 4)
    assert not differing(got, want), differing(got, want)
    got = call_series(torch_mod, eng, dict(case, link=np.zeros(M)), 1, 4)
    assert not differing(got, want), differing(got, want)
    assert (want["n_accept"] >= 1).mean() >= 0.5


@pytest.mark.parametrize("srf", [False, True])
def test_one_row_series_are_spart_refine_itself(torch_mod, engines, srf):
    eng = engines["s2"]
    case = case_of(torch_mod, eng, ["LIDFa"], ["LAI", "Cab"], "per_pixel", "per_row", "per_row", "varied", 1, 31, sizes=[1] * M, srf=srf,
                   special=3)
    got = call_series(torch_mod, eng, case, 1, 3, band_model=int(srf))
    perm = [1, 2, 0]
    mean = np.concatenate([case["mean"], case["smean"]], axis=1)
    weight = np.concatenate([case["weight"], case["sweight"]], axis=1)
    rc, ref = raw_refine(torch_mod, eng, "spart_refine_srf" if srf else "spart_refine", case["base"], case["local"] + case["shared"],
                         case["lo"][perm], case["hi"][perm], case["obs"], case["w"], mean, weight, column=1, n_iter=3)
    assert rc == 0 and (ref["n_accept"] >= 0).all()
    assert same(got["local"], ref["x"][:, :2]) and same(got["shared"], ref["x"][:, 2:])
    assert same(got["local_std"], ref["std"][:, :2]) and same(got["shared_std"], ref["std"][:, 2:])
    assert same(got["n_accept"], ref["n_accept"]) and same(got["y"], ref["y"]) and (got["status"] == 0).all()
    assert same(got["cost"], ref["cost"]) and same(got["cost0"], ref["cost0"])
    assert (ref["n_accept"] >= 1).mean() >= 0.5


@pytest.mark.parametrize("what", ["link", "weight"])
def test_a_bad_row_kills_exactly_its_series(torch_mod, engines, plain, what):
    """a negative link entry (row 30 of the series of 39) / a negative band weight (row 20 of the series of 9): the series is dead
    as a whole with status -1 on the bad row and 1 on the others; the neighbours keep their bits"""
    eng = engines["s2"]
    case, ref5, _ = plain
    bad = dict(case, link=case["link"].copy(), w=case["w"].copy())
    if what == "link":
        bad["link"][30], t, row = -1.0, 5, 30
    else:
        bad["w"][20, 3], t, row = -1.0, 4, 20
    ts = case["series_start"]
    ref = defined_series(fwd_of(torch_mod, eng, 1), bad, 5)
    got = call_series(torch_mod, eng, bad, 1, 5)
    assert not differing(got, ref), differing(got, ref)
    rows = np.arange(ts[t], ts[t + 1])
    assert got["n_accept"][t] == -1 and got["status"][row] == -1 and (got["status"][rows[rows != row]] == 1).all()
    assert np.isnan(got["local_std"][rows]).all() and np.isnan(got["shared_std"][t]).all() and got["cost"][t] == got["cost0"][t]
    assert same(got["local"][rows], rd.clip_defined(case["base"][rows][:, case["local"]], case["lo"][1:], case["hi"][1:]))
    others = [s for s in range(len(LENGTHS)) if s != t]
    keep = np.ones(M, dtype=bool)
    keep[rows] = False
    assert all(same(got[k][others], ref5[k][others]) for k in SERIES_KEYS) and all(same(got[k][keep], ref5[k][keep]) for k in ROW_KEYS)


def test_a_series_alone_and_the_prefix(torch_mod, engines, plain):
    """the 39-row series run alone gives the same bits; n_iter = 3 is where n_iter = 5 was"""
    eng = engines["s2"]
    case, ref5, hist = plain
    not_vacuous(fwd_of(torch_mod, eng, 1), case, ref5, 5, "plain")
    got5 = call_series(torch_mod, eng, case, 1, 5)
    assert not differing(got5, ref5), differing(got5, ref5)
    cut = slice(27, 66)
    alone = dict(case, base=case["base"][cut], obs=case["obs"][cut], w=case["w"][cut], link=case["link"][cut], series_start=np.array([0, 39]))
    one = call_series(torch_mod, eng, alone, 1, 5)
    assert all(same(one[k][0], got5[k][5]) for k in SERIES_KEYS) and all(same(one[k], got5[k][cut]) for k in ROW_KEYS)
    got3 = call_series(torch_mod, eng, case, 1, 3)
    assert same(got3["shared"], hist[3][0]) and same(got3["local"], hist[3][1]) and same(got3["cost"], hist[3][2])
    assert (got5["cost"] <= got3["cost"]).all() and (got5["cost"] <= got5["cost0"]).all()


def test_a_masked_date_is_filled_by_its_neighbours(torch_mod, engines, plain):
    """row 13 is fully masked: with gamma = 0 its locals stay at the clipped start exactly and the series' std is NaN; with
    gamma > 0 they move and every std of the series is finite"""
    eng = engines["s2"]
    case, ref5, _ = plain
    start = rd.clip_defined(case["base"][13, case["local"]], case["lo"][1:], case["hi"][1:])
    flat = call_series(torch_mod, eng, dict(case, smooth=np.zeros(2)), 1, 5)
    got = call_series(torch_mod, eng, case, 1, 5)
    assert same(flat["local"][13], start) and np.isnan(flat["local_std"][10:18]).all() and np.isnan(flat["shared_std"][3]).all()
    assert (got["local"][13] != start).all() and np.isfinite(got["local_std"][10:18]).all() and np.isfinite(got["shared_std"][3]).all()


def test_chunk_cut_and_guard(torch_mod, engines):
    """F = 16: a chunk holds (1 << 19) // 17 = 30840 rows, so 120 series of 256 rows fill the first chunk (the next series of
    200 would cross the cap) and the series of 200 and of 10 are the second.  The call runs on all 30930 rows between guard
    bytes; the definition runs on the two series before the cut and the two behind it, which a series' independence of the
    others allows (test_a_series_alone_and_the_prefix pins that)."""
    eng = engines["s2"]
    assert (1 << 19) // 17 == 30840 and 120 * 256 + 200 > 30840
    sizes = [256] * 120 + [200, 10]
    case = make_series_case(fwd_of(torch_mod, eng, 0), F15, ["LAI"], sizes, "per_pixel", "none", "none", "varied", 9, special=30718,
                            move=1.0, lambda0=1e-9)
    assert case["base"].shape[0] == 30930
    got = call_series(torch_mod, eng, case, 0, 1, guard=True)
    assert all((got[k] != FILL).all() for k in OUTS) and (got["cost"] <= got["cost0"]).all() and (got["n_accept"] >= 0).all()
    rows, ser = slice(118 * 256, 30930), slice(118, 122)
    near = dict(case, base=case["base"][rows], obs=case["obs"][rows], w=case["w"][rows], link=case["link"][rows],
                series_start=np.array([0, 256, 512, 712, 722]))
    fwd = fwd_of(torch_mod, eng, 0)
    ref = defined_series(fwd, near, 1)
    assert all(same(got[k][ser], ref[k]) for k in SERIES_KEYS) and all(same(got[k][rows], ref[k]) for k in ROW_KEYS)
    assert (ref["n_accept"] == 1).any() and (case["w"][30719] == 0.0).all()
    size = lambda m, f=16, fs=15: int(eng.lib.spart_series_workspace_bytes(eng.ctx, m, f, fs))      # noqa: E731
    assert size(30840) == size(30930) == size(2_000_000_000) > size(100) > 0


def test_a_maximal_series(torch_mod, engines):
    eng = engines["s2"]
    """256 rows in one series, a broken chain in its middle: the walk of 256 steps and the quadratic std recurrence.  A series of
    514 unknowns finds a better point for many steps, so the fit runs 25 proposals to where it rejects one"""
    case = make_series_case(fwd_of(torch_mod, eng, 1), ["LIDFa"], ["LAI", "Cab"], [256], "none", "none", "none", "zero", 14,
                            special=100, move=0.1)
    ref, _ = check_series(torch_mod, eng, case, 1, 25, "maximal series")
    assert 1 <= ref["n_accept"][0] < 25


def test_engine_and_host_form_are_the_raw_call(torch_mod, engines, plain):
    import spart_amd
    eng = engines["s2"]
    case, _, _ = plain
    shared, local = ["LIDFa"], ["LAI", "Cab"]
    ts, link = case["series_start"], np.nan_to_num(case["link"], nan=0.0)
    sig = np.array([0.5, 8.0])
    mean, weight = np.array([3.0, 40.0]), np.array([0.25, 0.0])
    raw = call_series(torch_mod, eng, dict(case, smooth=1.0 / (sig * sig), link=link, mean=mean, weight=weight), 1, 3)
    P = torch_mod.as_tensor(np.ascontiguousarray(case["base"].T), device=eng.device)
    kw = dict(series_start=ts, smooth={"LAI": 0.5, "Cab": 8.0}, link=link, weights=case["w"], column="R_TOA", n_iter=3,
              prior={"LAI": (3.0, 2.0)})
    res = eng.refine_series(P, case["obs"], shared, local, **kw)
    assert all(same(res[k].cpu().numpy(), raw[k]) for k in OUTS), [k for k in OUTS if not same(res[k].cpu().numpy(), raw[k])]
    assert res["names"] == shared + local and same(res["series_start"], ts) and eng.calls["spart_refine_series"] >= 1
    host = spart_amd.refine_series(list(case["base"].T), case["obs"], S2, shared, local, **kw)
    assert all(same(host[k], raw[k]) for k in OUTS)
    # n_dates: uniform series; a local that is not named is not tied; link = None
    sub = slice(0, 60)
    uni = spart_amd.refine_series(case["base"][sub].T, case["obs"][sub], S2, shared, local, n_dates=12, smooth={"LAI": 0.5},
                                  weights=case["w"][sub], column="R_TOA", n_iter=2)
    assert same(uni["series_start"], np.arange(0, 61, 12))
    raw = call_series(torch_mod, eng, dict(case, base=case["base"][sub], obs=case["obs"][sub], w=case["w"][sub], link=None,
                                           smooth=np.array([4.0, 0.0]), series_start=uni["series_start"]), 1, 2)
    assert all(same(uni[k], raw[k]) for k in OUTS)


def refusal_case(torch_mod, eng):
    case = make_series_case(fwd_of(torch_mod, eng, 0), ["LIDFa"], ["LAI", "Cab"], [2, 3, 4], "per_pixel", "none", "shared", "varied", 2)
    return {k: v for k, v in case.items() if k not in ("truth", "lambda0")}


def test_refusals_leave_outputs_untouched(torch_mod, engines):
    from spart_amd import get_engine
    eng = engines["s2"]
    a = refusal_case(torch_mod, eng)
    need = int(eng.lib.spart_series_workspace_bytes(eng.ctx, 9, 3, 1))
    assert need > int(eng.lib.spart_tiles_workspace_bytes(eng.ctx, 9, 3, 1)) > 0
    INVALID, WORKSPACE, NOSENSOR = -1, -3, -4
    for kw, want in [(dict(n_shared=-1), INVALID), (dict(n_shared=4), INVALID), (dict(n_shared=3), INVALID), (dict(band_model=2), INVALID),
                     (dict(S=-1), INVALID), (dict(S=0), INVALID), (dict(null=("series_start",)), INVALID),
                     (dict(smooth=None), INVALID), (dict(smooth=[1.0, -1.0]), INVALID), (dict(smooth=[np.nan, 1.0]), INVALID),
                     (dict(smooth=[1.0, np.inf]), INVALID), (dict(F=0), INVALID), (dict(F=17), INVALID), (dict(M=-1), INVALID),
                     (dict(n_iter=101), INVALID), (dict(column=3), INVALID),
                     *[(dict(null=(k,)), INVALID) for k in ("base", "free", "lo", "hi", "obs", "opt", "out", "shared", "cost", "local")],
                     (dict(ctx=None), INVALID), (dict(null=("ws",)), WORKSPACE), (dict(ws_bytes=need - 1), WORKSPACE),
                     (dict(ctx=get_engine(None, 0).ctx), NOSENSOR)]:
        rc, got = series_call(torch_mod, eng, **{**a, **kw})
        assert rc == want, (kw, rc, eng.lib.spart_last_error(eng.ctx))
        assert all((got[k] == FILL).all() for k in OUTS), kw
    for ts in ([1, 2, 5, 9], [0, 2, 2, 9], [0, 5, 3, 9], [0, 2, 5, 8], [0, 2, 5, 10]):
        rc, got = series_call(torch_mod, eng, **{**a, "series_start": np.array(ts)})
        assert rc == INVALID and all((got[k] == FILL).all() for k in OUTS), ts
    # 257 rows in one series
    rc, _ = series_call(torch_mod, eng, **{**a, "base": np.repeat(a["base"][:1], 257, axis=0), "obs": np.repeat(a["obs"][:1], 257, axis=0),
                                           "w": None, "link": None, "series_start": np.array([0, 257])})
    assert rc == INVALID and b"series_start[1]" in eng.lib.spart_last_error(eng.ctx)
    rc, got = series_call(torch_mod, eng, **{**a, "M": 0, "S": 0})
    assert rc == 0 and all((got[k] == FILL).all() for k in OUTS)
    size = lambda m=9, f=3, fs=1, ctx=eng.ctx: int(eng.lib.spart_series_workspace_bytes(ctx, m, f, fs))      # noqa: E731
    for bad in (dict(m=0), dict(m=-1), dict(m=2_000_000_001), dict(f=0), dict(f=17), dict(fs=-1), dict(fs=4), dict(fs=3),
                dict(ctx=get_engine(None, 0).ctx), dict(ctx=None)):
        assert size(**bad) == 0, bad
    assert size() == need and size(f=16, fs=15) > 0 and size(f=16, fs=0) > 0 and size(f=1, fs=0) > 0
    # the optional outputs may be NULL; without either std the result is the same
    rc, got = series_call(torch_mod, eng, **{**a, "null": ("shared_std", "local_std", "cost0", "n_accept", "pixel_cost", "status", "y")})
    rc2, full = series_call(torch_mod, eng, **a)
    assert rc == rc2 == 0 and all(same(got[k], full[k]) for k in ("shared", "local", "cost")) and (got["y"] == FILL).all()


def test_the_first_refusal_wins(torch_mod, engines):
    eng = engines["s2"]
    a = refusal_case(torch_mod, eng)
    bad_ts = {**a, "series_start": np.array([0, 2, 2, 9])}
    for args, kw, text in [(a, dict(F=17, null=("free",)), "F = 17, expected"),
                           (a, dict(n_shared=4, column=3), "column = 3"),
                           (a, dict(n_shared=4, smooth=None), "n_shared = 4, expected"),
                           (a, dict(n_shared=3, smooth=None), "n_shared = F = 3, nothing to link: use spart_refine_tiles"),
                           (a, dict(band_model=2, n_shared=3), "band_model = 2"),
                           (bad_ts, dict(n_shared=3), "series_start[2] = 2 after 2"),
                           (bad_ts, dict(S=-1), "S = -1 series"),
                           (a, dict(smooth=None, ws_bytes=16), "smooth is null"),
                           (a, dict(smooth=[1.0, -2.0], ws_bytes=16), "smooth[1] = -2"),
                           (a, dict(smooth=[np.nan, -2.0]), "smooth[0] = nan"),
                           (a, dict(null=("obs",), smooth=None), "null argument")]:
        rc, got = series_call(torch_mod, eng, **{**args, **kw})
        msg = eng.lib.spart_last_error(eng.ctx).decode()
        assert rc in (-1, -3) and msg.startswith(f"spart_refine_series: {text}"), (kw, rc, msg)
        assert all((got[k] == FILL).all() for k in OUTS), kw


def test_refine_series_example_runs():
    """examples/refine_series.py as a user runs it: its own process, exit code 0, the expected last line"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_series.py"), "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "LAI error" in r.stdout and r.stdout.rstrip().endswith("fitted 24 dates of 4 pixels three ways")
