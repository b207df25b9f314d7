"""spart_refine_mix without a GPU: the definition tools/refine_mix_defined.py against tools/refine_defined.py where the two
must agree (one component; fractions (1, 0)), its simplex and prefix properties; the g++ build (-ffp-contract=off) of part 1 of
csrc/spart_refine_mix.h driven pixel by pixel (tests/hostmath/refine_mix_host.cpp) against the definition bit for bit, and the
same driver as a stand-alone program under the address and undefined-behaviour sanitizers; the refusals of
spart_amd.refine_mix / Engine.refine_mix that need no device; struct, signature and header agreement."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402
import refine_mix_defined as rmd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "refine_mix_host.cpp")
OUTS = ("x", "cost", "cost0", "std", "n_accept", "y", "frac", "y_comp")
FIT_OUTS = OUTS[:6]
c_dp, c_ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
GXX = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1"]


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def dp(a):
    return None if a is None else a.ctypes.data_as(c_dp)


def ip(a):
    return None if a is None else a.ctypes.data_as(c_ip)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refine_mix_host") / "librefine_mix_host.so")
    subprocess.check_call(GXX + ["-shared", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rmh_forward.argtypes = [ctypes.c_int64, c_dp, ctypes.c_int, c_dp]
    L.rmh_forward.restype = None
    L.rmh_maps.argtypes = [ctypes.c_int] * 3 + [c_ip, ctypes.c_int] + [c_ip] * 5
    L.rmh_pixel.argtypes = ([ctypes.c_int] * 3 + [c_ip, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_dp, c_ip, c_dp, c_dp,
                             ctypes.c_double, ctypes.c_double, ctypes.c_int] + [c_dp] * 5 + [c_dp] * 4 + [c_ip, c_dp, c_dp, c_dp, c_ip])
    L.rmh_pixel.restype = None
    return L


def forward_of(lib, nb):
    def forward(rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        out = np.empty((rows.shape[0], nb))
        lib.rmh_forward(rows.shape[0], dp(rows), nb, dp(out))
        return out
    return forward


def mask_of(name, V, Fl):
    """all: None; crop_soil: the locals live in component 0 only; one: local 0 lives in the last component only, the others
    everywhere"""
    if isinstance(name, np.ndarray):
        return name
    if name == "all" or Fl == 0:
        return None
    act = np.ones((V, Fl), dtype=np.int32)
    if name == "crop_soil":
        act[1:] = 0
    else:
        act[:, 0] = 0
        act[V - 1, 0] = 1
    return act


def toy_case(lib, V, Fs, Fl, mask, fit, kind, with_prior, seed, M=11, nb=21):
    """random mixed pixels on the toy forward.  nb = 21: one whole 16-band tile and a partial one.  Special pixels: 0 a start
    outside its box, 3 a NaN fixed parameter in the last component (dead), 4 a negative weight (per-pixel weights; dead), 5 a NaN
    in the last component's entry of a shared column (never read when V > 1), 6 a NaN in frac[:, V - 1] (never read when the
    fractions are fitted), 7 an infeasible start (fitted, V >= 3; dead, cost +inf), 8 a given fraction of -0.1 (dead)"""
    rng = np.random.default_rng(seed)
    free = [15, 0, 2, 1][:Fs + Fl]
    shared, local = free[:Fs], free[Fs:]
    F = Fs + Fl
    lo, hi = np.zeros(F), np.array([2.0, 1.0, 1.0, 1.0])[:F]
    forward = forward_of(lib, nb)
    active = mask_of(mask, V, Fl)
    kindu, name, comp, unknown = rmd.maps_defined(V, Fs, Fl, active, fit)
    n = kindu.size
    truth = rng.uniform(0.0, 1.0, (V, M, 27))
    truth[1:, :, shared] = truth[0][None][:, :, shared]
    a = rng.dirichlet(np.full(V, 3.0), M)
    Yt = forward(truth.reshape(-1, 27)).reshape(V, M, nb)
    obs = np.einsum("mv,vmj->mj", a, Yt) * (1 + 0.01 * rng.normal(size=(M, nb)))
    base = truth.copy()
    move = rng.uniform(-0.1, 0.1, (V, M, F)) * (hi - lo)
    move[1:, :, :Fs] = move[0][None][:, :, :Fs]
    base[:, :, free] = rd.clip_defined(truth[:, :, free] + move, lo, hi)
    frac = 0.8 * a + 0.2 / V if fit else a.copy()
    base[0, 0, free[0]] = 5.0
    base[V - 1, 3, 20] = np.nan
    if V > 1 and Fs:
        base[V - 1, 5, shared[0]] = np.nan
    if fit:
        frac[6, V - 1] = np.nan
        if V >= 3:
            frac[7, :2] = 0.8
    else:
        frac[8, 0] = -0.1
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 1, nb)
        w[2] = 0.0
    elif kind == "per_pixel":
        w = 10.0 ** rng.uniform(-1, 1, (M, nb))
        w[rng.random((M, nb)) < 0.15] = 0.0
        w[4, 1] = -2.0
        obs[w == 0.0] = np.nan
    mu = pw = None
    if with_prior:
        mu = rng.uniform(0.0, 1.0, (M, n))
        pw = 10.0 ** rng.uniform(-2, 1, (M, n))
        pw[:, 0] = 0.0
        mu[9, 0] = np.nan                                                        # under a zero weight
    return dict(base=base, shared=shared, local=local, lo=lo, hi=hi, obs=obs, frac=frac, active=active, fit_fractions=fit, weights=w,
                prior_mean=mu, prior_weight=pw), forward


def planted_dead(case):
    """the pixels of toy_case that must be dead"""
    V, fit, w = case["base"].shape[0], case["fit_fractions"], case["weights"]
    dead = {3}
    if w is not None and w.ndim == 2:
        dead.add(4)
    if fit and V >= 3:
        dead.add(7)
    if not fit:
        dead.add(8)
    return dead


# ---- the definition against refine_defined
@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("kind", ["none", "shared", "per_pixel"])
@pytest.mark.parametrize("Fs,Fl", [(2, 0), (1, 2), (0, 3)])
def test_one_component_is_refine_defined(lib, Fs, Fl, kind, fit):
    """consequence (a): 1 z and 1 - 0 are exact"""
    case, forward = toy_case(lib, 1, Fs, Fl, "all", fit, kind, Fl == 2, 10 * Fs + Fl)
    case["frac"] = np.ones_like(case["frac"])
    got = rmd.refine_mix_defined(forward=forward, n_iter=4, **case)
    ref = rd.refine_defined(case["base"][0], case["shared"] + case["local"], case["lo"], case["hi"], case["obs"], forward,
                            weights=case["weights"], n_iter=4, prior_mean=case["prior_mean"], prior_weight=case["prior_weight"])
    for k in FIT_OUTS:
        assert same(got[k], ref[k]), k
    assert same(got["y_comp"][:, 0], ref["y"]) and (got["frac"] == 1.0).all()
    assert (ref["n_accept"] >= 1).sum() >= 6 and (ref["n_accept"] == -1).sum() >= 1


@pytest.mark.parametrize("kind", ["none", "per_pixel"])
def test_fractions_one_zero_are_refine_defined_of_component_zero(lib, kind):
    """consequence (b): given fractions (1, 0), locals active in component 0 only, positive finite spectra of component 1"""
    case, forward = toy_case(lib, 2, 1, 2, "crop_soil", False, kind, True, 77)
    case["frac"] = np.tile([1.0, 0.0], (case["obs"].shape[0], 1))
    case["base"][1, 3, 20] = 0.5                                                  # component 1 stays finite everywhere
    case["base"][0, 3, 20] = np.nan
    got = rmd.refine_mix_defined(forward=forward, n_iter=4, **case)
    assert np.isfinite(got["y_comp"][:, 1]).all() and (got["y_comp"][:, 1] > 0).all()
    ref = rd.refine_defined(case["base"][0], case["shared"] + case["local"], case["lo"], case["hi"], case["obs"], forward,
                            weights=case["weights"], n_iter=4, prior_mean=case["prior_mean"], prior_weight=case["prior_weight"])
    for k in FIT_OUTS:
        assert same(got[k], ref[k]), k
    assert (ref["n_accept"] >= 1).sum() >= 6 and ref["n_accept"][3] == -1


def test_definition_properties(lib):
    """(c) the fractions sum to 1 to within a rounding and the last is >= 0 on live pixels; (d) cost <= cost0 and the prefix
    property; a pixel does not depend on its batch; an infeasible start is dead with cost +inf"""
    case, forward = toy_case(lib, 3, 1, 2, "crop_soil", True, "per_pixel", False, 5)
    h3, h5 = [], []
    r3 = rmd.refine_mix_defined(forward=forward, n_iter=3, history=h3, **case)
    r5 = rmd.refine_mix_defined(forward=forward, n_iter=5, history=h5, **case)
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(h3, h5)) and same(r3["x"], h5[3][0])
    live = r5["n_accept"] >= 0
    assert sorted(np.flatnonzero(~live)) == sorted(planted_dead(case))
    assert (r5["cost"][live] <= r5["cost0"][live]).all() and (r5["n_accept"][live] >= 1).sum() >= 5
    assert (np.abs(r5["frac"][live].sum(axis=1) - 1.0) <= 2.0 ** -52).all() and (r5["frac"][live, -1] >= 0.0).all()
    assert np.isposinf(r5["cost"][7]) and np.isposinf(r5["cost0"][7]) and r5["frac"][7, -1] < 0 and np.isnan(r5["std"][7]).all()
    assert r5["n_accept"][5] >= 0 and r5["n_accept"][6] >= 0                       # the planted NaNs are never read
    pick = [2, 9, 0]
    sub = dict(case, base=case["base"][:, pick], obs=case["obs"][pick], frac=case["frac"][pick], weights=case["weights"][pick])
    rs = rmd.refine_mix_defined(forward=forward, n_iter=5, **sub)
    for k in OUTS:
        assert same(rs[k], r5[k][pick]), k


def test_an_infeasible_proposal_is_rejected(lib):
    """three components with a tiny true last fraction: some trial leaves the simplex, is rejected, and no live pixel ends
    with a negative fraction"""
    case, forward = toy_case(lib, 3, 0, 1, np.array([[1], [0], [1]], dtype=np.int32), True, "none", False, 9, M=48)
    rng = np.random.default_rng(3)
    M = 48
    a = np.stack([rng.uniform(0.3, 0.7, M), np.zeros(M), rng.uniform(0.0, 0.03, M)], axis=1)
    a[:, 1] = 1.0 - a[:, 0] - a[:, 2]
    base = case["base"]
    base[np.isnan(base)] = 0.5
    base[0, 0, 15] = 1.0
    Y = forward(base.reshape(-1, 27)).reshape(3, M, -1)
    case["obs"] = np.einsum("mv,vmj->mj", a, Y) * (1 + 0.02 * rng.normal(size=(M, Y.shape[2])))
    case["frac"] = a.copy()
    hist = []
    res = rmd.refine_mix_defined(forward=forward, n_iter=6, history=hist, **case)
    live = res["n_accept"] >= 0
    assert live.all() and sum(int((~h[2]).sum()) for h in hist) >= 1
    assert (res["frac"] >= 0.0).all() and (res["cost"] <= res["cost0"]).all()


# ---- the g++ build against the definition
def test_maps(lib):
    for V, Fs, Fl, mask, fit in [(1, 2, 0, "all", 1), (2, 1, 2, "crop_soil", 1), (3, 0, 1, "one", 1), (4, 1, 3, "all", 1), (8, 1, 1, "all", 1),
                                 (8, 9, 0, "all", 1), (2, 2, 1, "all", 0), (3, 1, 2, "one", 0)]:
        act = mask_of(mask, V, Fl)
        kind, name, comp, unknown = rmd.maps_defined(V, Fs, Fl, act, bool(fit))
        k, nm_, c, nm = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int32), ctypes.c_int32(0)
        u = np.zeros(V * (Fs + Fl), np.int32)
        n = lib.rmh_maps(V, Fs, Fl, ip(act), fit, ip(k), ip(nm_), ip(c), ip(u), ctypes.byref(nm))
        assert n == kind.size and nm.value == int((kind != rmd.FRACTION).sum())
        assert list(k[:n]) == list(kind) and list(nm_[:n]) == list(name) and list(c[:n]) == list(comp)
        assert list(u) == list(unknown.reshape(-1))
    none = np.array([[1, 0], [1, 0]], dtype=np.int32)
    args = [ip(np.zeros(16, np.int32)) for _ in range(3)] + [ip(np.zeros(8, np.int32)), ctypes.byref(ctypes.c_int32(0))]
    assert lib.rmh_maps(2, 1, 2, ip(none), 1, *args) == -1                       # a local that is active nowhere
    assert lib.rmh_maps(8, 1, 2, None, 1, *[ip(np.zeros(16, np.int32)) for _ in range(3)], ip(np.zeros(24, np.int32)),
                        ctypes.byref(ctypes.c_int32(0))) == -2                   # 1 + 16 + 7 unknowns
    with pytest.raises(ValueError, match="no component"):
        rmd.maps_defined(2, 1, 2, none)
    assert lib.rmh_max_v() == rmd.MAX_V == 8


def host_loop(lib, case, n_iter, rel_step=1e-3, lambda0=1e-2, frac_lo=0.0, frac_hi=1.0):
    """the fit of every pixel from the g++ driver -> the definition's dict"""
    base, obs, w, act, fit = case["base"], case["obs"], case["weights"], case["active"], case["fit_fractions"]
    V, M, _ = base.shape
    nb = obs.shape[1]
    Fs, Fl = len(case["shared"]), len(case["local"])
    n = rmd.maps_defined(V, Fs, Fl, act, fit)[0].size
    free = np.array(case["shared"] + case["local"], dtype=np.int32)
    res = {"x": np.zeros((M, n)), "cost": np.zeros(M), "cost0": np.zeros(M), "std": np.zeros((M, n)), "n_accept": np.zeros(M, np.int32),
           "y": np.zeros((M, nb)), "frac": np.zeros((M, V)), "y_comp": np.zeros((M, V, nb))}
    for m in range(M):
        bm = np.ascontiguousarray(base[:, m])
        wm = None if w is None else np.ascontiguousarray(w[m] if w.ndim == 2 else w)
        mu = pw = None
        if case["prior_weight"] is not None:
            mu, pw = (np.ascontiguousarray(np.broadcast_to(case[k], (M, n))[m]) for k in ("prior_mean", "prior_weight"))
        c, c0, na, inf = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int32(0), ctypes.c_int32(0)
        x, sd, y, fo, yc = np.zeros(n), np.zeros(n), np.zeros(nb), np.zeros(V), np.zeros((V, nb))
        lib.rmh_pixel(V, Fs, Fl, ip(act), int(fit), frac_lo, frac_hi, nb, dp(bm), ip(free), dp(case["lo"]), dp(case["hi"]), rel_step,
                      lambda0, n_iter, dp(np.ascontiguousarray(obs[m])), dp(wm), dp(np.ascontiguousarray(case["frac"][m])), dp(mu), dp(pw),
                      dp(x), dp(sd), ctypes.cast(ctypes.byref(c), c_dp), ctypes.cast(ctypes.byref(c0), c_dp), ctypes.byref(na), dp(y),
                      dp(fo), dp(yc), ctypes.byref(inf))
        res["x"][m], res["std"][m], res["cost"][m], res["cost0"][m], res["n_accept"][m] = x, sd, c.value, c0.value, na.value
        res["y"][m], res["frac"][m], res["y_comp"][m] = y, fo, yc
    return res


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind", ["none", "shared", "per_pixel"])
@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("mask", ["all", "crop_soil", "one"])
@pytest.mark.parametrize("V", [1, 2, 3, 8])
def test_per_pixel_driver_from_the_header_matches_the_definition(lib, V, mask, fit, kind, with_prior):
    Fs, Fl = (1, 1) if V == 8 else (1, 2)
    case, forward = toy_case(lib, V, Fs, Fl, mask, fit, kind, with_prior, 100 * V + 7 * len(mask) + fit)
    n_iter = 8 if V == 8 else 4                                # (16 unknowns take longer to find a first accepted step)
    ref = rmd.refine_mix_defined(forward=forward, n_iter=n_iter, **case)
    got = host_loop(lib, case, n_iter)
    for k in OUTS:
        assert same(got[k], ref[k]), (k, got[k], ref[k])
    live = ref["n_accept"] >= 0
    assert sorted(np.flatnonzero(~live)) == sorted(planted_dead(case)), ref["n_accept"]
    assert (ref["n_accept"] >= 1).sum() >= 5 and (ref["cost"][live] <= ref["cost0"][live]).all(), ref["n_accept"]


def test_fraction_box_and_steps(lib):
    """a narrow fraction box, another rel_step and lambda0 reach the driver and the definition alike"""
    case, forward = toy_case(lib, 2, 1, 2, "crop_soil", True, "shared", False, 31)
    ref = rmd.refine_mix_defined(forward=forward, n_iter=3, rel_step=5e-3, lambda0=1e-9, frac_lo=0.25, frac_hi=0.75, **case)
    got = host_loop(lib, case, 3, rel_step=5e-3, lambda0=1e-9, frac_lo=0.25, frac_hi=0.75)
    for k in OUTS:
        assert same(got[k], ref[k]), k
    live = ref["n_accept"] >= 0
    assert (ref["x"][live, -1] >= 0.25).all() and (ref["x"][live, -1] <= 0.75).all() and (ref["n_accept"] >= 1).sum() >= 5


def test_stand_alone_driver_under_the_sanitizers(tmp_path):
    """the same file with its own main, built with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "refine_mix_host_asan")
    subprocess.check_call(GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRMH_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refine_mix_host: 64 fits" in out.stdout and "ERROR" not in out.stderr, (out.stdout, out.stderr)


# ---- refusals that need no device
def test_refine_mix_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    M, V = 4, 3
    P = np.repeat(workloads.lhs_params(M, "full", seed=1).T[:, None, :], V, axis=1)          # (27, V, M)
    obs = np.zeros((M, 13))
    ok = dict(shared=["B"], local=["LAI", "Cab"], active={"LAI": [0], "Cab": [0, 1]})
    for kw, text in ((dict(shared=[], local=[]), "free"), (dict(shared=["LAI"], local=["nope"]), "unknown"),
                     (dict(shared=["LAI"], local=["LAI"]), "twice"),
                     (dict(shared=["B"], local=["LAI", "Cab", "Cw", "Cdm", "N"]), "unknowns"),
                     (dict(ok, obs=np.zeros((M, V, 13))), "obs"), (dict(ok, active={"Cw": [0]}), "not local"),
                     (dict(ok, active={"LAI": [3]}), "components"), (dict(ok, active={"LAI": []}), "no component"),
                     (dict(ok, active=np.ones((2, 2))), "active"), (dict(ok, active=np.full((V, 2), 2)), "active"),
                     (dict(ok, active=np.array([[1, 0], [1, 0], [1, 0]])), "no component"),
                     (dict(ok, fractions=np.ones(2)), "fractions"), (dict(ok, fractions=np.ones((M + 1, V))), "fractions"),
                     (dict(ok, fit_fractions=1), "fit_fractions"), (dict(ok, fraction_bounds=(0.5, 0.5)), "fraction_bounds"),
                     (dict(ok, fraction_bounds=(-0.1, 1.0)), "fraction_bounds"), (dict(ok, fraction_bounds=0.5), "fraction_bounds"),
                     (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"), (dict(ok, bounds={"Cw": (0.0, 1.0)}), "not free"),
                     (dict(ok, n_iter=101), "n_iter"), (dict(ok, column="rso"), "column"), (dict(ok, rel_step=-1e-3), "rel_step"),
                     (dict(ok, lidf="fast"), "lidf"), (dict(ok, band_model="wide"), "band_model"),
                     (dict(ok, weights=np.ones((V, 13))), "weights"), (dict(ok, prior={"Cw": (0.0, 1.0)}), "not free"),
                     (dict(ok, prior={"LAI": (1.0, -1.0)}), "sigma"), (dict(ok, prior={"B": (np.zeros(M + 1), 1.0)}), "pixels"),
                     (dict(ok, prior={"LAI": (np.zeros(V + 1), 1.0)}), "shape"), (dict(ok, prior={"fractions": (np.zeros(V), 1.0)}), "shape"),
                     (dict(ok, fit_fractions=False, prior={"fractions": (0.5, 1.0)}), "fractions")):
        kw = dict(kw)
        o = kw.pop("obs", obs)
        with pytest.raises(ValueError, match=text):
            spart_amd.refine_mix(P, o, "Sentinel2A-MSI", **kw)
    with pytest.raises(ValueError, match="27"):
        spart_amd.refine_mix(P[:26], obs, "Sentinel2A-MSI", **ok)
    with pytest.raises(ValueError, match="components"):
        spart_amd.refine_mix(np.repeat(P, 3, axis=1), obs, "Sentinel2A-MSI", shared=["B"])
    with pytest.raises(ValueError, match="broadcast"):
        spart_amd.refine_mix([0.0] * 26 + [np.zeros(M + 1)], obs, "Sentinel2A-MSI", fractions=np.ones(V) / V, **ok)
    e = engine.Engine.__new__(engine.Engine)                   # an Engine object that never saw a device
    e.nb = 13
    with pytest.raises(ValueError, match="unknown"):
        e.refine_mix(P, obs, ["LAI", "nope"])
    with pytest.raises(ValueError, match="obs"):
        e.refine_mix(P, np.zeros((M, 12)), ["LAI"])
    # what the checks hand on: the maps, the fractions and the prior per unknown
    plan, _, (M_, V_, Fs, nm, n), act, fr, box, wper, mean, weight, per = engine.refine_mix_args(
        P, obs, ["B"], ["LAI", "Cab"], ok["active"], None, True, (0, 1), None, None, "R_TOC", 4, 1e-3, 1e-2, "literal",
        {"B": (0.5, 2.0), "Cab": (np.array([40.0, 30.0, 99.0]), 10.0), "fractions": (np.array([0.6, 0.3]), 0.5)}, "centre")
    assert (M_, V_, Fs, nm, n) == (M, V, 1, 4, 6) and act.tolist() == [[1, 1], [0, 1], [0, 0]] and box == (0.0, 1.0) and wper == 0
    assert np.allclose(fr, 1.0 / 3) and fr.shape == (M, V) and per == 0
    assert mean.tolist() == [0.5, 0.0, 40.0, 30.0, 0.6, 0.3] and weight.tolist() == [0.25, 0.0, 0.01, 0.01, 4.0, 4.0]
    assert engine.mix_maps(V, 1, 2, act, True)[0].tolist() == [[1, 2], [-1, 3], [-1, -1]]


def test_signatures_structs_and_header_agree():
    from spart_amd import _lib
    opt = ["fit", "V", "n_shared", "band_model", "fit_fractions", "local_active", "frac_lo", "frac_hi"]
    out = ["x", "cost", "cost0", "std", "n_accept", "y", "frac", "y_comp"]
    assert [f[0] for f in _lib.SpartRefineMixOpt._fields_] == opt and _lib.SpartRefineMixOpt._fields_[0][1] is _lib.SpartRefineOpt
    assert [f[0] for f in _lib.SpartRefineMixOut._fields_] == out == list(_lib.MIX_OUTS) and _lib.MIX_MAXV == 8
    res, args = _lib.SIGNATURES["spart_refine_mix"]
    ref = list(_lib.SIGNATURES["spart_refine"][1])
    assert res is ctypes.c_int and len(args) == 15 and args[:9] == ref[:9] and args[12:] == ref[16:]
    assert len(_lib.SIGNATURES["spart_mix_workspace_bytes"][1]) == 5
    header = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, fields in (("spart_refine_mix_opt", opt), ("spart_refine_mix_out", out)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), plain, flags=re.S).group(1)
        assert re.findall(r"\b([A-Za-z_0-9]+)\s*[,;]", body) == fields, name
    decl = re.search(r"int spart_refine_mix\((.*?)\);", plain, flags=re.S).group(1)
    assert decl.count(",") + 1 == 15
    assert "#define SPART_ABI_VERSION 14" in header and "spart_refine_mix and" in header
    # the header carries the definition's text
    for phrase in ("a_{V-1} = 1 - s", "FEASIBLE iff", "J_ja = Y_(v,0)j - Y_(V-1,0)j", "the chosen column itself is\n * mixed"):
        assert phrase.lower() in header.lower(), phrase
    src = open(os.path.join(ROOT, "spart-python_amd", "build.py")).read()
    assert '"spart_refine_mix.h"' in src


def test_null_context_is_refused_without_a_gpu():
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    L = ctypes.CDLL(build.build(verbose=False))
    f = L.spart_mix_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert f(None, 100, 2, 3, 4) == 0
    L.spart_refine_mix.restype = ctypes.c_int
    L.spart_last_error.restype = ctypes.c_char_p
    assert L.spart_refine_mix(*([None] * 15)) == -1 and b"spart_refine_mix: null context" in L.spart_last_error(None)
