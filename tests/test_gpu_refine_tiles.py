"""spart_refine_tiles on the GPU: the raw C ABI against the definition tools/refine_tiles_defined.py, bit for bit, with the
library's own float64 pruned column path as the definition's forward model (helpers/refine_calls.forward_of): every shape of
shared / local unknowns at M = 67 in tiles of 1, 1, 2, 7, 8, 9 and 39 pixels, the special pixels, one-pixel tiles against
spart_refine / spart_refine_srf themselves, a tile run alone, the chunk cut, a maximal tile, Engine.refine_tiles /
spart_amd.refine_tiles, the refusals and the example.  If a mismatch shows here and not in tests/test_refine_tiles_host.py, the
cause is in the kernels' index maps, their order of summation or contraction, not in the formula."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import F16, FILL, S2, rd, same
from helpers.refine_srf_calls import raw_refine
from helpers.refine_tiles_calls import (OUTS, PARTITION, PIXEL_KEYS, TILE_KEYS, call_tiles, check_tiles, defined_tiles, differing,
                                        fwd_of, make_tiles_case, not_vacuous, tiles_call)

pytestmark = pytest.mark.gpu
M = 67
REST15 = [n for n in F16 if n != "aot550"]

# (shared, local, weights, local prior, shared prior, column, n_iter, seed, further arguments of the case); the seeds are those
# for which the DEFINITION satisfies helpers.refine_tiles_calls.not_vacuous.  A first step from a start near the truth at the
# default damping is never rejected, so the n_iter = 1 case starts up to half the range away with lambda0 = 1e-9.
SHAPES = [(["aot550"], ["LAI", "Cab"], "none", "none", "none", 1, 4, 1, {}),
          (["aot550", "uh2o"], [], "shared", "none", "shared", 2, 0, 2, {}),
          ([], ["LAI", "Cab"], "per_pixel", "per_row", "none", 0, 1, 1, dict(move=0.5, lambda0=1e-9)),
          (["aot550", "uh2o", "LIDFa", "SMp"], ["LAI", "Cab", "Cw", "Cdm"], "per_pixel", "shared", "per_row", 1, 4, 4, {}),
          (F16, [], "none", "none", "shared", 0, 4, 1, {}),
          (["aot550"], REST15, "shared", "per_row", "none", 1, 4, 6, {})]


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {"s2": get_engine(S2, 0), "hyper": get_engine(None, 0, sensor_info=hyper_si)}


def case_of(torch, eng, shared, local, kind, lprior, sprior, column, seed, sizes=PARTITION, srf=False, **kw):
    kw.setdefault("special", 11)
    kw.setdefault("dead_tile", 1)
    return make_tiles_case(fwd_of(torch, eng, column, srf), shared, local, sizes, kind, lprior, sprior, seed, **kw)


@pytest.fixture(scope="module")
def plain(torch_mod, engines):
    """Fs = 1, Fl = 2 on R_TOA with per-pixel weights: the case of the alone, prefix and Engine tests, and its definition"""
    case = case_of(torch_mod, engines["s2"], ["aot550"], ["LAI", "Cab"], "per_pixel", "none", "none", 1, 21)
    hist = []
    return case, defined_tiles(fwd_of(torch_mod, engines["s2"], 1), case, 5, history=hist), hist


@pytest.mark.parametrize("shared,local,kind,lprior,sprior,column,n_iter,seed,more", SHAPES, ids=[f"Fs{len(s[0])}-Fl{len(s[1])}" for s in SHAPES])
def test_definition_bit_for_bit(torch_mod, engines, shared, local, kind, lprior, sprior, column, n_iter, seed, more):
    eng = engines["s2"]
    case = case_of(torch_mod, eng, shared, local, kind, lprior, sprior, column, seed, **more)
    ref, _ = check_tiles(torch_mod, eng, case, column, n_iter, (shared, local))
    Fs = len(shared)
    # the dead one-pixel tile; the dead pixel in a live tile; the start outside the box; the NaN shared entry that is not read
    assert ref["n_accept"][1] == -1 and ref["status"][1] == -1 and np.isnan(ref["shared_std"][1]).all()
    assert ref["status"][12] == -1 and ref["n_accept"][4] >= 0 and (ref["status"][np.r_[11, 13:19]] == 0).all()
    if Fs:
        assert ref["shared"][4, 0] <= case["hi"][0] and np.isfinite(ref["shared"][4]).all() and np.isnan(case["base"][14, case["shared"][0]])
    else:
        assert ref["local"][11, 0] <= case["hi"][0]
    if kind == "per_pixel":
        assert ref["status"][13] == 0 and (case["w"][13] == 0.0).all()          # fully masked, alive


def test_hyperspectral_sensor_two_tiles(torch_mod, engines):
    """nb = 211 is no multiple of 16, and the y rows of a pixel are dealt to the lanes of its packed entries"""
    eng = engines["hyper"]
    assert eng.nb % 16 != 0
    case = case_of(torch_mod, eng, ["aot550"], ["LAI", "Cab"], "per_pixel", "shared", "shared", 0, 3, sizes=[7, 12], special=8, dead_tile=None)
    ref, _ = check_tiles(torch_mod, eng, case, 0, 6, "hyper")           # (six proposals: a fit that has converged rejects)
    assert ref["status"][9] == -1 and (ref["n_accept"] >= 1).all()


def as_single_pixels(case):
    """the arguments of spart_refine that a call with one pixel per tile stands for: local names then shared names, the two
    priors concatenated per observation in that order"""
    Fs, Fl, m = len(case["shared"]), len(case["local"]), case["base"].shape[0]
    perm = list(range(Fs, Fs + Fl)) + list(range(Fs))
    mean = weight = None
    if case["mean"] is not None or case["smean"] is not None:
        parts = [(case["mean"], case["weight"], Fl), (case["smean"], case["sweight"], Fs)]
        mean = np.concatenate([np.broadcast_to(np.zeros(n) if mu is None else mu, (m, n)) for mu, _, n in parts], axis=1)
        weight = np.concatenate([np.broadcast_to(np.zeros(n) if pw is None else pw, (m, n)) for _, pw, n in parts], axis=1)
    return case["local"] + case["shared"], case["lo"][perm], case["hi"][perm], mean, weight


@pytest.mark.parametrize("lprior,sprior,srf", [("none", "none", False), ("per_row", "per_row", False), ("none", "none", True)])
def test_one_pixel_tiles_are_spart_refine_itself(torch_mod, engines, lprior, sprior, srf):
    eng = engines["s2"]
    case = case_of(torch_mod, eng, ["aot550"], ["LAI", "Cab"], "per_pixel", lprior, sprior, 1, 31, sizes=[1] * M, srf=srf, special=3,
                   dead_tile=None)
    got = call_tiles(torch_mod, eng, case, 1, 3, band_model=int(srf))
    free, lo, hi, mean, weight = as_single_pixels(case)
    rc, ref = raw_refine(torch_mod, eng, "spart_refine_srf" if srf else "spart_refine", case["base"], free, lo, hi, case["obs"], case["w"],
                         mean, weight, column=1, n_iter=3)
    assert rc == 0
    live = ref["n_accept"] >= 0
    assert same(got["local"], ref["x"][:, :2]) and same(got["shared"], ref["x"][:, 2:])
    assert same(got["local_std"], ref["std"][:, :2]) and same(got["shared_std"], ref["std"][:, 2:])
    assert same(got["n_accept"], ref["n_accept"]) and same(got["y"], ref["y"]) and same(got["status"], np.where(live, 0, -1).astype(np.int32))
    assert same(got["cost"][live], ref["cost"][live]) and same(got["cost0"][live], ref["cost0"][live])
    assert same(got["pixel_cost"][~live], ref["cost"][~live]) if sprior == "none" else True       # (a dead tile's cost holds no pixel's)
    assert not live[4] and live[3] and (ref["n_accept"] >= 1).mean() >= 0.5 and (ref["n_accept"][live] < 3).any()


def test_a_tile_alone_and_the_prefix(torch_mod, engines, plain):
    """consequences (b) and (c): the 39-pixel tile run alone gives the same bits; n_iter = 3 is where n_iter = 5 was"""
    eng = engines["s2"]
    case, ref5, hist = plain
    not_vacuous(ref5, 5, "plain")
    got5 = call_tiles(torch_mod, eng, case, 1, 5)
    assert not differing(got5, ref5)
    cut = slice(28, 67)
    alone = dict(case, base=case["base"][cut], obs=case["obs"][cut], w=case["w"][cut], tile_start=np.array([0, 39]))
    one = call_tiles(torch_mod, eng, alone, 1, 5)
    assert all(same(one[k][0], got5[k][6]) for k in TILE_KEYS) and all(same(one[k], got5[k][cut]) for k in PIXEL_KEYS)
    got3 = call_tiles(torch_mod, eng, case, 1, 3)
    live = ref5["n_accept"] >= 0
    assert same(got3["shared"], hist[3][0]) and same(got3["local"], hist[3][1]) and same(got3["cost"], hist[3][2])
    assert (got5["cost"] <= got3["cost"])[live].all() and (got5["cost"] <= got5["cost0"])[live].all()


def test_a_dead_pixel_changes_only_itself(torch_mod, engines, plain):
    """consequence (d): the tile of 8 with its dead pixel 12 removed gives the tile's result"""
    eng = engines["s2"]
    case, ref5, _ = plain
    keep = np.r_[11, 13:19]
    less = dict(case, base=case["base"][keep], obs=case["obs"][keep], w=case["w"][keep], tile_start=np.array([0, 7]))
    one = call_tiles(torch_mod, eng, less, 1, 5)
    assert all(same(one[k][0], ref5[k][4]) for k in TILE_KEYS) and all(same(one[k], ref5[k][keep]) for k in PIXEL_KEYS)


def test_live_pixels_of_a_dead_tile(torch_mod, engines):
    """the first shape with a shared prior that is absent (weight 0 over a NaN mean) everywhere but in the tile of 9 pixels, where
    its weight is negative: that tile is dead, its pixels are alive and get status 1, y, pixel_cost and NaN stds; the other tiles
    are what they are without a prior"""
    eng = engines["s2"]
    shared, local, kind, lprior, sprior, column, n_iter, seed, more = SHAPES[0]
    case = case_of(torch_mod, eng, shared, local, kind, lprior, sprior, column, seed, **more)
    T = len(PARTITION)
    smean, sweight = np.full((T, 1), np.nan), np.zeros((T, 1))
    smean[5, 0], sweight[5, 0] = 0.2, -1.0
    ref, got = check_tiles(torch_mod, eng, dict(case, smean=smean, sweight=sweight), column, n_iter, "dead tile")
    plain_ref = defined_tiles(fwd_of(torch_mod, eng, column), case, n_iter)
    px = slice(19, 28)
    assert got["n_accept"][5] == -1 and (got["status"][px] == 1).all() and np.isnan(got["local_std"][px]).all() and np.isnan(got["shared_std"][5]).all()
    assert np.isfinite(got["y"][px]).all() and np.isfinite(got["pixel_cost"][px]).all() and got["cost"][5] == got["cost0"][5]
    assert same(got["local"][px], rd.clip_defined(case["base"][px][:, case["local"]], case["lo"][1:], case["hi"][1:]))
    others = [t for t in range(T) if t != 5]
    assert all(same(got[k][others], plain_ref[k][others]) for k in TILE_KEYS)


def test_forward_scratch_bounds_every_row_count(engines):
    """the forward call's block of the workspace, recovered from the layout (every block rounded up to 256 bytes), is at least
    spart_workspace_bytes of EVERY batch up to the chunk's rows: the partition decides a chunk's row count, and the forward
    workspace is not monotonic in the batch"""
    eng = engines["s2"]
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731
    for M, F, Fs in ((100, 3, 1), (30850, 16, 15), (300000, 1, 0)):
        mc = min(M, (1 << 19) // (F + 1))
        rows, Fl, P, Ps, nb = mc * (F + 1), F - Fs, F * (F + 1) // 2 + F, Fs * (Fs + 1) // 2 + Fs, eng.nb
        rest = [27 * rows * 8] + [rows * nb * 8] * 3 + [48 * 8, 16 * 4, mc * Fl * 8, mc * 8, mc * P * 8, mc * P * 8, mc * Fs * 8,
                                                     mc * Ps * 8, mc * Ps * 8, mc * 8] + [mc * 4] * 4 + [(mc + 1) * 4, mc * 4]
        fwd = int(eng.lib.spart_tiles_workspace_bytes(eng.ctx, M, F, Fs)) - sum(up(b) for b in rest)
        worst = max(int(eng.lib.spart_workspace_bytes(eng.ctx, 1, B)) for B in range(1, rows + 1))
        assert 0 < worst <= fwd, (M, F, Fs, worst, fwd)
        assert fwd <= 2 * worst, (M, F, Fs, worst, fwd)            # (a bound, not a guess far above)


def test_chunk_cut_and_guard(torch_mod, engines):
    """F = 16: a chunk holds (1 << 19) // 17 = 30840 pixels, so seven tiles of 4096 and one of 2168 fill the first chunk and the
    tile of 10 is the second; special pixels sit on both sides of the cut.  n_iter = 1: the starts lie anywhere in the box and
    lambda0 = 1e-9, so that some tiles reject their first step (seed chosen on the definition: 7 of 9 accept)"""
    eng = engines["s2"]
    assert (1 << 19) // 17 == 30840 == 7 * 4096 + 2168
    sizes = [4096] * 7 + [2168, 10]
    case = make_tiles_case(fwd_of(torch_mod, eng, 0), [n for n in F16 if n != "LAI"], ["LAI"], sizes, "per_pixel", "none", "none", 9,
                           special=30838, move=1.0, lambda0=1e-9)
    assert case["base"].shape[0] == 30850
    ref, _ = check_tiles(torch_mod, eng, case, 0, 1, "chunk cut", guard=True)
    assert list(ref["status"][30838:30842]) == [0, -1, 0, 0] and (case["w"][30840] == 0.0).all() and (ref["n_accept"] >= 0).all()
    size = lambda m, f=16, fs=15: int(eng.lib.spart_tiles_workspace_bytes(eng.ctx, m, f, fs))      # noqa: E731
    assert size(30840) == size(30850) == size(2_000_000_000) > size(100) > 0


def test_a_maximal_tile(torch_mod, engines):
    """4096 pixels in one tile: the ordered walk over 512 groups; the seed is one for which the definition accepts some steps
    and rejects others"""
    eng = engines["s2"]
    case = make_tiles_case(fwd_of(torch_mod, eng, 1), ["aot550", "uh2o"], ["LAI", "Cab"], [4096], "none", "none", "none", 14, special=100)
    ref, _ = check_tiles(torch_mod, eng, case, 1, 4, "maximal tile")
    assert 1 <= ref["n_accept"][0] < 4 and ref["status"][101] == -1


def test_engine_and_host_form_are_the_raw_call(torch_mod, engines, plain):
    import spart_amd
    eng = engines["s2"]
    case, _, _ = plain
    shared, local = ["aot550"], ["LAI", "Cab"]
    T = len(PARTITION)
    smean, sweight = np.linspace(0.1, 0.4, T)[:, None], np.full((T, 1), 16.0)
    mean, weight = np.array([3.0, 40.0]), np.array([0.25, 0.0])
    raw = call_tiles(torch_mod, eng, dict(case, mean=mean, weight=weight, smean=smean, sweight=sweight), 1, 3)
    P = torch_mod.as_tensor(np.ascontiguousarray(case["base"].T), device=eng.device)
    prior = {"LAI": (3.0, 2.0), "aot550": (smean[:, 0], 0.25)}                      # weight = 1 / sigma^2, exactly
    res = eng.refine_tiles(P, case["obs"], shared, local, tile_start=case["tile_start"], weights=case["w"], column="R_TOA", n_iter=3,
                           prior=prior)
    assert all(same(res[k].cpu().numpy(), raw[k]) for k in OUTS), [k for k in OUTS if not same(res[k].cpu().numpy(), raw[k])]
    assert res["names"] == shared + local and same(res["tile_start"], case["tile_start"]) and eng.calls["spart_refine_tiles"] >= 1
    host = spart_amd.refine_tiles(list(case["base"].T), case["obs"], S2, shared, local, tile_start=list(case["tile_start"]),
                                  weights=case["w"], column="R_TOA", n_iter=3, prior=prior)
    assert all(same(host[k], raw[k]) for k in OUTS)
    # tile_size: uniform runs with a shorter last one
    uni = spart_amd.refine_tiles(case["base"].T, case["obs"], S2, shared, local, tile_size=16, weights=case["w"], column="R_TOA", n_iter=2)
    assert same(uni["tile_start"], np.array([0, 16, 32, 48, 64, 67]))
    raw = call_tiles(torch_mod, eng, dict(case, tile_start=uni["tile_start"]), 1, 2)
    assert all(same(uni[k], raw[k]) for k in OUTS)


def refusal_case(torch_mod, eng):
    case = make_tiles_case(fwd_of(torch_mod, eng, 0), ["aot550"], ["LAI", "Cab"], [2, 3, 4], "per_pixel", "none", "shared", 2)
    return (case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["tile_start"], case["obs"], case["w"], None, None,
            case["smean"], case["sweight"])


def test_refusals_leave_outputs_untouched(torch_mod, engines):
    from spart_amd import get_engine
    eng = engines["s2"]
    a = refusal_case(torch_mod, eng)
    need = int(eng.lib.spart_tiles_workspace_bytes(eng.ctx, 9, 3, 1))
    assert need > 0
    INVALID, WORKSPACE, NOSENSOR = -1, -3, -4
    bad_starts = [[1, 2, 5, 9], [0, 2, 2, 9], [0, 5, 3, 9], [0, 2, 5, 8], [0, 2, 5, 10]]
    for kw, want in [(dict(n_shared=-1), INVALID), (dict(n_shared=4), INVALID), (dict(band_model=2), INVALID), (dict(band_model=-1), INVALID),
                     (dict(T=-1), INVALID), (dict(T=0), INVALID), (dict(null=("tile_start",)), INVALID),
                     (dict(null=("smean",)), INVALID), (dict(null=("sweight",)), INVALID), (dict(sper=2), INVALID),
                     (dict(F=0), INVALID), (dict(F=17), INVALID), (dict(M=-1), INVALID), (dict(n_iter=101), INVALID), (dict(column=3), INVALID),
                     *[(dict(null=(k,)), INVALID) for k in ("base", "free", "lo", "hi", "obs", "opt", "out", "shared", "cost", "local")],
                     (dict(ctx=None), INVALID), (dict(null=("ws",)), WORKSPACE), (dict(ws_bytes=need - 1), WORKSPACE),
                     (dict(ctx=get_engine(None, 0).ctx), NOSENSOR)]:
        rc, got = tiles_call(torch_mod, eng, *a, **kw)
        assert rc == want, (kw, rc, eng.lib.spart_last_error(eng.ctx))
        assert all((got[k] == FILL).all() for k in OUTS), kw
    for ts in bad_starts:
        rc, got = tiles_call(torch_mod, eng, *a[:5], np.array(ts), *a[6:])
        assert rc == INVALID and all((got[k] == FILL).all() for k in OUTS), ts
    # 4097 pixels in one tile
    rc, _ = tiles_call(torch_mod, eng, np.repeat(a[0][:1], 4097, axis=0), *a[1:5], np.array([0, 4097]), np.repeat(a[6][:1], 4097, axis=0))
    assert rc == INVALID and b"tile_start[1]" in eng.lib.spart_last_error(eng.ctx)
    rc, got = tiles_call(torch_mod, eng, *a, M=0, T=0)
    assert rc == 0 and all((got[k] == FILL).all() for k in OUTS)
    # the workspace size: 0 exactly for refused sizes
    size = lambda m=9, f=3, fs=1, ctx=eng.ctx: int(eng.lib.spart_tiles_workspace_bytes(ctx, m, f, fs))      # noqa: E731
    for bad in (dict(m=0), dict(m=-1), dict(m=2_000_000_001), dict(f=0), dict(f=17), dict(fs=-1), dict(fs=4),
                dict(ctx=get_engine(None, 0).ctx), dict(ctx=None)):
        assert size(**bad) == 0, bad
    assert size() == need and size(f=16, fs=16) > 0 and size(f=16, fs=0) > 0 and size(f=1, fs=0) > 0 and size(f=1, fs=1) > 0
    # the optional outputs may be NULL
    rc, got = tiles_call(torch_mod, eng, *a, null=("shared_std", "local_std", "cost0", "n_accept", "pixel_cost", "status", "y"))
    rc2, full = tiles_call(torch_mod, eng, *a)
    assert rc == rc2 == 0 and all(same(got[k], full[k]) for k in ("shared", "local", "cost")) and (got["y"] == FILL).all()


def test_the_first_refusal_wins(torch_mod, engines):
    """calls with two faults: the one that is checked first is the one reported, and nothing is written"""
    eng = engines["s2"]
    a = refusal_case(torch_mod, eng)
    bad_ts = a[:5] + (np.array([0, 2, 2, 9]),) + a[6:]
    for args, kw, text in [(a, dict(F=17, null=("free",)), "F = 17, expected"),
                           (a, dict(M=-1, F=0), "M = -1, expected"),
                           (a, dict(n_shared=4, column=3), "column = 3"),
                           (a, dict(n_shared=4, ws_bytes=16), "n_shared = 4, expected"),
                           (a, dict(sper=2, ws_bytes=16), "shared_prior_per_tile = 2"),
                           (a, dict(null=("cost",), n_shared=4), "null argument"),
                           (a, dict(null=("obs",), T=-1), "null argument"),
                           (a, dict(null=("base[3]",), band_model=2), "base[3] is null"),
                           (a, dict(n_shared=4, band_model=2), "n_shared = 4, expected"),
                           (a, dict(band_model=2, T=0), "band_model = 2"),
                           (bad_ts, dict(T=-1), "T = -1 tiles"),
                           (bad_ts, dict(null=("smean",)), "tile_start[2] = 2 after 2"),
                           (a, dict(null=("smean", "shared")), "null argument"),
                           (a, dict(null=("smean",), sper=2), "shared_prior_mean and shared_prior_weight come together")]:
        rc, got = tiles_call(torch_mod, eng, *args, **kw)
        msg = eng.lib.spart_last_error(eng.ctx).decode()
        assert rc in (-1, -3) and msg.startswith(f"spart_refine_tiles: {text}"), (kw, rc, msg)
        assert all((got[k] == FILL).all() for k in OUTS), kw


def test_refine_tiles_example_runs():
    """examples/refine_tiles.py as a user runs it: its own process, exit code 0, the expected last line"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_tiles.py"), "16", "20"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "aot550 per window" in r.stdout and r.stdout.rstrip().endswith("fitted 1 shared parameter of 6 tiles and 2 local parameters of 320 pixels")
