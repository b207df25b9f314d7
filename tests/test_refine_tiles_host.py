"""spart_refine_tiles without a GPU: the definition tools/refine_tiles_defined.py against tools/refine_defined.py where the two
must agree (one pixel per tile); the g++ build (-ffp-contract=off) of part 1 of csrc/spart_refine_tiles.h, driven tile by tile
(tests/hostmath/refine_tiles_host.cpp), against the definition on a cheap nonlinear forward, bit for bit; the consequences the
GPU tests rely on; the host helpers; the refusals of Engine.refine_tiles / spart_amd.refine_tiles that need no device; the
structs, the workspace size and the kernels' resources."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402
import refine_tiles_defined as rtd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "refine_tiles_host.cpp")
OUTS = ("shared", "shared_std", "local", "local_std", "cost", "cost0", "n_accept", "pixel_cost", "status", "y")
TILE_KEYS = ("shared", "shared_std", "cost", "cost0", "n_accept")
PIXEL_KEYS = ("local", "local_std", "pixel_cost", "status", "y")
PARTITION = [1, 1, 2, 7, 8, 9, 39]
c_dp, c_ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def dp(a):
    return None if a is None else a.ctypes.data_as(c_dp)


def ip(a):
    return a.ctypes.data_as(c_ip)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refine_tiles_host") / "librefine_tiles_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rth_chunk.restype = ctypes.c_int64
    for f in (L.rth_clip, L.rth_step, L.rth_lambda, L.rth_pixel_cost, L.rth_tile_cost):
        f.restype = ctypes.c_double
    L.rth_clip.argtypes = L.rth_step.argtypes = [ctypes.c_double] * 3
    L.rth_lambda.argtypes = [ctypes.c_double, ctypes.c_int]
    L.rth_pixel_cost.argtypes = [ctypes.c_int] * 2 + [c_dp] * 6 + [c_ip]
    L.rth_pixel_sums.argtypes = [ctypes.c_int] * 3 + [c_dp] * 8
    L.rth_tile_cost.argtypes = [ctypes.c_int, c_ip, c_dp, ctypes.c_int, c_dp, c_dp, c_dp, c_ip, c_ip]
    L.rth_tile_sums.argtypes = [ctypes.c_int, c_ip, c_dp, ctypes.c_int, ctypes.c_int] + [c_dp] * 4
    L.rth_tile_propose.argtypes = [ctypes.c_int, c_ip, c_dp, c_dp, ctypes.c_int, ctypes.c_int, ctypes.c_double] + [c_dp] * 6
    L.rth_tile_std.argtypes = [ctypes.c_int, c_ip, c_dp, c_dp, ctypes.c_int, ctypes.c_int, c_dp, c_dp]
    return L


def toy_forward(nb, seed=0):
    Wm = np.random.default_rng(seed).normal(size=(27, nb))

    def forward(rows):
        with np.errstate(all="ignore"):
            return np.tanh(rows @ Wm * 0.05) + 0.1 * np.sin(rows[:, [0]] * np.arange(1, nb + 1) * 0.01)
    return forward


def toy_case(Fs, Fl, sizes, kind, lprior, sprior, seed, nb=7, special=True):
    """random pixels on the toy forward, every shared name constant over a tile.  Special pixels (``special``, M >= 20): 11 a
    start outside the box (the first pixel of the tile of 8), 12 a NaN fixed parameter (a dead pixel in a live tile), 13 a fully
    masked pixel (per-pixel weights), 14 a NaN in the shared column (not read), 1 a NaN fixed parameter in a tile of its own (a
    dead tile), 15 a negative band weight (per-pixel weights; dead)"""
    rng = np.random.default_rng(seed)
    free = [15, 0, 2, 1, 5, 7][:Fs + Fl]
    shared, local = free[:Fs], free[Fs:]
    F = Fs + Fl
    ts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    M, T = int(ts[-1]), len(sizes)
    tile_of = np.repeat(np.arange(T), sizes)
    lo, hi = np.zeros(F), np.array([2.0, 1.0, 1.0, 1.0, 1.5, 1.0])[:F]
    base = rng.uniform(0.0, 1.0, (M, 27))
    truth = base.copy()
    truth[:, free] = rng.uniform(lo, hi, (M, F))
    truth[:, shared] = truth[ts[:-1]][tile_of][:, shared]
    forward = toy_forward(nb, seed)
    obs = forward(truth) * (1.0 + 0.02 * rng.normal(size=(M, nb)))
    base[:, free] = rd.clip_defined(truth[:, free] + rng.uniform(-0.3, 0.3, (M, F)) * (hi - lo), lo, hi)
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 1, nb)
        w[2] = 0.0
    elif kind == "per_pixel":
        w = 10.0 ** rng.uniform(-1, 1, (M, nb))
        w[rng.random((M, nb)) < 0.15] = 0.0
        w[:, 1] = np.where(w[:, 1] == 0.0, 1.0, w[:, 1])
    if special and M >= 20:
        base[11, free[0]] = 5.0
        base[12, 20] = np.nan
        base[1, 20] = np.nan
        if Fs and 14 not in ts[:-1]:
            base[14, free[0]] = np.nan
        if kind == "per_pixel":
            w[13] = 0.0
            w[15, 3] = -1.0
    if kind == "per_pixel":
        obs[w == 0.0] = np.nan
    kw = {}
    if lprior != "none" and Fl:
        shape = (M, Fl) if lprior == "per_row" else (Fl,)
        kw["prior_mean"] = rng.uniform(lo[Fs:], hi[Fs:], shape)
        kw["prior_weight"] = np.full(shape, 4.0)
        if lprior == "per_row":
            zero = rng.random(shape) < 0.2
            kw["prior_mean"], kw["prior_weight"] = np.where(zero, np.nan, kw["prior_mean"]), np.where(zero, 0.0, kw["prior_weight"])
    if sprior != "none" and Fs:
        shape = (T, Fs) if sprior == "per_row" else (Fs,)
        kw["shared_prior_mean"] = rng.uniform(lo[:Fs], hi[:Fs], shape)
        kw["shared_prior_weight"] = np.full(shape, 2.0)
    return dict(base=base, shared=shared, local=local, lo=lo, hi=hi, tile_start=ts, obs=obs, weights=w, **kw), forward


# ---- consequence (a): one pixel per tile is refine_defined
@pytest.mark.parametrize("priors", [False, True])
@pytest.mark.parametrize("Fs,Fl", [(1, 2), (2, 0), (0, 2), (3, 3)])
def test_one_pixel_tiles_are_refine_defined(Fs, Fl, priors):
    M = 24
    case, forward = toy_case(Fs, Fl, [1] * M, "per_pixel", "per_row" if priors else "none", "per_row" if priors else "none", 10 * Fs + Fl)
    got = rtd.refine_tiles_defined(forward=forward, n_iter=5, **case)
    perm = list(range(Fs, Fs + Fl)) + list(range(Fs))
    mean = weight = None
    if priors:
        parts = [(case.get("prior_mean"), case.get("prior_weight"), Fl), (case.get("shared_prior_mean"), case.get("shared_prior_weight"), Fs)]
        mean = np.concatenate([np.zeros((M, n)) if mu is None else mu for mu, _, n in parts], axis=1)
        weight = np.concatenate([np.zeros((M, n)) if pw is None else pw for _, pw, n in parts], axis=1)
    ref = rd.refine_defined(case["base"], case["local"] + case["shared"], case["lo"][perm], case["hi"][perm], case["obs"], forward,
                            weights=case["weights"], n_iter=5, prior_mean=mean, prior_weight=weight)
    live = ref["n_accept"] >= 0
    assert same(got["local"], ref["x"][:, :Fl]) and same(got["shared"], ref["x"][:, Fl:])
    assert same(got["local_std"], ref["std"][:, :Fl]) and same(got["shared_std"], ref["std"][:, Fl:])
    assert same(got["n_accept"], ref["n_accept"]) and same(got["y"], ref["y"]) and same(got["status"], np.where(live, 0, -1).astype(np.int32))
    assert same(got["cost"][live], ref["cost"][live]) and same(got["cost0"][live], ref["cost0"][live])
    assert same(got["pixel_cost"][live], ref["cost"][live]) if not (priors and Fs) else True
    assert not live[[1, 12, 15]].any() and live.sum() == M - 3 and (ref["n_accept"] >= 1).mean() >= 0.5 and (ref["n_accept"][live] < 5).any()
    assert not (got["status"] == 1).any()


# ---- part 1 of the header, driven tile by tile
def host_loop(lib, case, forward, n_iter, rel_step=1e-3, lambda0=1e-2):
    base, obs, w = case["base"], case["obs"], case["weights"]
    shared, local, lo, hi, ts = case["shared"], case["local"], case["lo"], case["hi"], case["tile_start"]
    free = shared + local
    Fs, Fl, F, (M, nb), T = len(shared), len(local), len(free), obs.shape, ts.size - 1
    nt, nts = F * (F + 1) // 2, Fs * (Fs + 1) // 2
    P, h = nt + F, rel_step * (hi - lo)
    pm, pw, sm, sw = (case.get(k) for k in ("prior_mean", "prior_weight", "shared_prior_mean", "shared_prior_weight"))
    row = lambda a, i: None if a is None else np.ascontiguousarray(a[i] if a.ndim == 2 else a)     # noqa: E731
    res = {"shared": np.zeros((T, Fs)), "shared_std": np.full((T, Fs), np.nan), "local": np.zeros((M, Fl)),
           "local_std": np.full((M, Fl), np.nan), "cost": np.zeros(T), "cost0": np.zeros(T), "n_accept": np.zeros(T, dtype=np.int32),
           "pixel_cost": np.full(M, np.nan), "status": np.zeros(M, dtype=np.int32), "y": np.full((M, nb), np.nan)}
    for t in range(T):
        m0, G = int(ts[t]), int(ts[t + 1] - ts[t])
        z = np.array([lib.rth_clip(base[m0, shared[a]], lo[a], hi[a]) for a in range(Fs)])
        l = np.array([[lib.rth_clip(base[m0 + m, local[b]], lo[Fs + b], hi[Fs + b]) for b in range(Fl)] for m in range(G)]).reshape(G, Fl)
        zt, lt = z.copy(), l.copy()
        live = np.ones(G, dtype=np.int32)
        Ap, St = np.zeros((G, P)), np.zeros(nts + Fs)
        C, lam, na, dead = np.inf, lambda0, 0, False
        smu, spw = row(sm, t), row(sw, t)
        for it in range(n_iter + 1):
            tn = np.concatenate([np.broadcast_to(zt, (G, Fs)), lt], axis=1)                  # (G, F) by name
            sh = np.array([[lib.rth_step(tn[m, f], h[f], hi[f]) for f in range(F)] for m in range(G)]).reshape(G, F)
            rows = np.repeat(base[m0:m0 + G][:, None], F + 1, axis=1)                        # (G, F + 1, 27)
            rows[:, :, free] = tn[:, None]
            for f in range(F):
                rows[:, f + 1, free[f]] = tn[:, f] + sh[:, f]
            Y = forward(rows.reshape(-1, 27)).reshape(G, F + 1, nb)
            c = np.zeros(G)
            for m in range(G):
                if it > 0 and not live[m]:
                    continue
                b = ctypes.c_int32(0)
                wm = row(w, m0 + m)
                c[m] = lib.rth_pixel_cost(nb, Fl, dp(np.ascontiguousarray(Y[m, 0])), dp(np.ascontiguousarray(obs[m0 + m])), dp(wm),
                                          dp(np.ascontiguousarray(lt[m])), dp(row(pm, m0 + m)), dp(row(pw, m0 + m)), ctypes.byref(b))
                if it == 0 and not (c[m] < np.inf and not b.value):
                    live[m] = 0
                    res["status"][m0 + m], res["pixel_cost"][m0 + m], res["y"][m0 + m] = -1, c[m], Y[m, 0]
            bad, some = ctypes.c_int32(0), ctypes.c_int32(0)
            Ct = lib.rth_tile_cost(G, ip(live), dp(c), Fs, dp(zt), dp(smu), dp(spw), ctypes.byref(bad), ctypes.byref(some))
            if it == 0:
                res["cost0"][t] = Ct
                if not (some.value and not bad.value and Ct < np.inf):
                    dead, C, na = True, Ct, -1
                    for m in np.flatnonzero(live):
                        res["status"][m0 + m], res["pixel_cost"][m0 + m], res["y"][m0 + m] = 1, c[m], Y[m, 0]
            if dead:
                break
            acc = Ct < C
            if acc:
                z, C = zt.copy(), Ct
                for m in np.flatnonzero(live):
                    l[m] = lt[m]
                    res["pixel_cost"][m0 + m], res["y"][m0 + m] = c[m], Y[m, 0]
                    lib.rth_pixel_sums(F, Fs, nb, dp(np.ascontiguousarray(Y[m])), dp(np.ascontiguousarray(obs[m0 + m])), dp(row(w, m0 + m)),
                                       dp(np.ascontiguousarray(sh[m])), dp(np.ascontiguousarray(l[m])), dp(row(pm, m0 + m)),
                                       dp(row(pw, m0 + m)), dp(Ap[m]))
                lib.rth_tile_sums(G, ip(live), dp(Ap), F, Fs, dp(z), dp(smu), dp(spw), dp(St))
            if it > 0:
                lam, na = lib.rth_lambda(lam, int(acc)), na + int(acc)
            if it < n_iter:
                lib.rth_tile_propose(G, ip(live), dp(Ap), dp(St), F, Fs, lam, dp(z), dp(l), dp(lo), dp(hi), dp(zt), dp(lt))
        res["shared"][t], res["local"][m0:m0 + G], res["cost"][t], res["n_accept"][t] = z, l, C, na
        if not dead:
            ss, ls = np.full(Fs, np.nan), np.full((G, Fl), np.nan)
            lib.rth_tile_std(G, ip(live), dp(Ap), dp(St), F, Fs, dp(ss), dp(ls))
            res["shared_std"][t], res["local_std"][m0:m0 + G] = ss, ls
    return res


HOST_CASES = [(1, 2, "none", "none", "none"), (2, 0, "shared", "none", "shared"), (0, 2, "per_pixel", "per_row", "none"),
              (3, 3, "per_pixel", "shared", "per_row"), (1, 5, "per_pixel", "per_row", "shared")]


@pytest.mark.parametrize("Fs,Fl,kind,lprior,sprior", HOST_CASES, ids=[f"Fs{c[0]}-Fl{c[1]}" for c in HOST_CASES])
def test_tile_loop_from_the_header_matches_the_definition(lib, Fs, Fl, kind, lprior, sprior):
    case, forward = toy_case(Fs, Fl, PARTITION, kind, lprior, sprior, 100 + 10 * Fs + Fl)
    ref = rtd.refine_tiles_defined(forward=forward, n_iter=4, **case)
    got = host_loop(lib, case, forward, 4)
    for k in OUTS:
        assert same(got[k], ref[k]), (k, got[k], ref[k])
    live = ref["n_accept"] >= 0
    assert ref["n_accept"][1] == -1 and live.sum() == 6 and ref["status"][12] == -1 and ref["status"][11] == 0
    assert (ref["n_accept"][live] >= 1).mean() >= 0.5 and (ref["n_accept"][live] < 4).any(), ref["n_accept"]
    assert (ref["cost"][live] <= ref["cost0"][live]).all()


def test_one_tile_of_67(lib):
    case, forward = toy_case(2, 2, [67], "per_pixel", "none", "none", 5)
    ref = rtd.refine_tiles_defined(forward=forward, n_iter=4, **case)
    got = host_loop(lib, case, forward, 4)
    for k in OUTS:
        assert same(got[k], ref[k]), k
    assert 1 <= ref["n_accept"][0] and (ref["status"][[1, 12, 15]] == -1).all() and (ref["status"] == 0).sum() == 64


def test_live_pixels_of_a_dead_tile_from_the_header(lib):
    case, forward = toy_case(1, 2, [4, 5, 6], "none", "none", "per_row", 8, special=False)
    case["shared_prior_weight"][1, 0] = -1.0
    ref = rtd.refine_tiles_defined(forward=forward, n_iter=3, **case)
    got = host_loop(lib, case, forward, 3)
    for k in OUTS:
        assert same(got[k], ref[k]), k
    assert ref["n_accept"][1] == -1 and (ref["n_accept"][[0, 2]] >= 1).all() and ref["status"].tolist() == [0] * 4 + [1] * 5 + [0] * 6


def test_index_maps(lib):
    assert lib.rth_max_tile() == 4096 == rtd.MAX_TILE and lib.rth_chunk(16) == 30840 and lib.rth_chunk(1) == 262144
    for Fs, Fl in ((0, 3), (2, 0), (1, 2), (4, 12)):
        F = Fs + Fl
        sol, name = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
        pa, pb = np.zeros(F * (F + 1) // 2, dtype=np.int32), np.zeros(F * (F + 1) // 2, dtype=np.int32)
        lib.rth_maps(Fs, Fl, ip(sol), ip(name), ip(pa), ip(pb))
        assert name.tolist() == list(range(Fs, F)) + list(range(Fs)) and (name[sol] == np.arange(F)).all()
        ia, ib = rd.packed_pairs(F)
        assert same(pa, ia.astype(np.int32)) and same(pb, ib.astype(np.int32))


# ---- consequences (b), (c), (d) on the definition
@pytest.fixture(scope="module")
def plain():
    case, forward = toy_case(1, 2, PARTITION, "per_pixel", "none", "shared", 3)
    hist = []
    return case, forward, rtd.refine_tiles_defined(forward=forward, n_iter=5, history=hist, **case), hist


def cut_case(case, pixels, ts):
    out = dict(case, base=case["base"][pixels], obs=case["obs"][pixels], weights=case["weights"][pixels], tile_start=np.asarray(ts))
    return out


def test_a_tile_does_not_depend_on_the_others(plain):
    case, forward, ref, _ = plain
    for t in (4, 6):
        a, b = int(case["tile_start"][t]), int(case["tile_start"][t + 1])
        one = rtd.refine_tiles_defined(forward=forward, n_iter=5, **cut_case(case, slice(a, b), [0, b - a]))
        assert all(same(one[k][0], ref[k][t]) for k in TILE_KEYS) and all(same(one[k], ref[k][a:b]) for k in PIXEL_KEYS), t


def test_cost_falls_and_n_iter_is_a_prefix(plain):
    case, forward, ref, hist = plain
    live = ref["n_accept"] >= 0
    assert (ref["cost"][live] <= ref["cost0"][live]).all() and len(hist) == 6
    for k in (0, 2, 4):
        short = rtd.refine_tiles_defined(forward=forward, n_iter=k, **case)
        assert same(short["shared"], hist[k][0]) and same(short["local"], hist[k][1]) and same(short["cost"], hist[k][2])
        assert (ref["cost"][live] <= short["cost"][live]).all()


def test_a_dead_pixel_changes_only_itself(plain):
    case, forward, ref, _ = plain
    assert ref["status"][12] == -1 and ref["n_accept"][4] >= 1
    keep = np.r_[11, 13:19]
    one = rtd.refine_tiles_defined(forward=forward, n_iter=5, **cut_case(case, keep, [0, 7]))
    assert all(same(one[k][0], ref[k][4]) for k in TILE_KEYS) and all(same(one[k], ref[k][keep]) for k in PIXEL_KEYS)
    assert ref["status"][1] == -1 and ref["n_accept"][1] == -1 and np.isnan(ref["shared_std"][1]).all()


def test_a_dead_tile_marks_its_live_pixels():
    case, forward = toy_case(1, 2, [4, 5], "none", "none", "per_row", 8, special=False)
    case["shared_prior_weight"][1, 0] = -1.0
    ref = rtd.refine_tiles_defined(forward=forward, n_iter=3, **case)
    assert ref["n_accept"].tolist()[1] == -1 and ref["n_accept"][0] >= 0 and ref["status"].tolist() == [0] * 4 + [1] * 5
    start = rd.clip_defined(case["base"][4:, case["local"]], case["lo"][1:], case["hi"][1:])
    assert same(ref["local"][4:], start) and np.isnan(ref["local_std"][4:]).all() and np.isfinite(ref["y"][4:]).all()
    assert ref["cost"][1] == ref["cost0"][1] and np.isfinite(ref["pixel_cost"][4:]).all()


# ---- the host helpers
def test_tiles_from_labels_and_window_tiles():
    import spart_amd
    labels = np.array([7, 3, 7, 7, 1, 3, 1])
    order, ts = spart_amd.tiles_from_labels(labels)
    assert order.tolist() == [4, 6, 1, 5, 0, 2, 3] and ts.tolist() == [0, 2, 4, 7] and order.dtype == ts.dtype == np.int64
    order, ts = spart_amd.tiles_from_labels(np.array(["b", "a", "b"]))
    assert order.tolist() == [1, 0, 2] and ts.tolist() == [0, 1, 3]
    order, ts = spart_amd.tiles_from_labels(np.zeros(0))
    assert order.size == 0 and ts.tolist() == [0]
    with pytest.raises(ValueError, match="labels"):
        spart_amd.tiles_from_labels(np.zeros((2, 2)))
    order, ts = spart_amd.window_tiles(5, 7, 4)
    assert np.diff(ts).tolist() == [16, 12, 4, 3] and sorted(order.tolist()) == list(range(35))
    assert order[:16].tolist() == [r * 7 + c for r in range(4) for c in range(4)] and order[-3:].tolist() == [32, 33, 34]
    order, ts = spart_amd.window_tiles(8, 8, 8)
    assert ts.tolist() == [0, 64] and order.tolist() == list(range(64))
    for bad in ((5, 7, 0), (5, 7, 65), (-1, 7, 2), (5, 2.5, 2)):
        with pytest.raises(ValueError):
            spart_amd.window_tiles(*bad)


# ---- refusals that need no device
def test_refine_tiles_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    M = 6
    P = workloads.lhs_params(M, "full", seed=1).T
    obs = np.zeros((M, 13))
    ok = dict(shared=["aot550"], local=["LAI", "Cab"], tile_size=4)
    for kw, text in ((dict(ok, shared=[], local=[]), "free"), (dict(ok, local=["nope"]), "unknown"), (dict(ok, local=["aot550"]), "twice"),
                     (dict(ok, obs=np.zeros((M, 2, 13))), "obs"), (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"),
                     (dict(ok, bounds={"Cw": (0.0, 1.0)}), "not free"), (dict(ok, n_iter=101), "n_iter"), (dict(ok, column="rso"), "column"),
                     (dict(ok, rel_step=-1e-3), "rel_step"), (dict(ok, lidf="fast"), "lidf"), (dict(ok, band_model="wide"), "band_model"),
                     (dict(ok, weights=np.ones((M + 1, 13))), "weights"),
                     (dict(ok, tile_size=None), "exactly one"), (dict(ok, tile_start=[0, 6]), "exactly one"),
                     (dict(ok, tile_size=0), "tile_size"), (dict(ok, tile_size=4097), "tile_size"), (dict(ok, tile_size=2.5), "tile_size"),
                     (dict(ok, tile_size=None, tile_start=[0, 3, 5]), "expected 0 ... M"), (dict(ok, tile_size=None, tile_start=[1, 6]), "expected 0 ... M"),
                     (dict(ok, tile_size=None, tile_start=[0, 3, 3, 6]), "tile 1 has 0 pixels"),
                     (dict(ok, tile_size=None, tile_start=[0, 4, 2, 6]), "tile 1 has -2 pixels"),
                     (dict(ok, tile_size=None, tile_start=[0.0, 6.0]), "integer"), (dict(ok, tile_size=None, tile_start=[[0, 6]]), "integer"),
                     (dict(ok, prior={"Cw": (0.0, 1.0)}), "not free"), (dict(ok, prior={"LAI": (1.0, -1.0)}), "sigma"),
                     (dict(ok, prior=[1.0]), "dict"),
                     (dict(ok, prior={"aot550": (np.zeros(M), 1.0)}), "2 tiles"), (dict(ok, prior={"LAI": (np.zeros(2), 1.0)}), "6 pixels")):
        kw = dict(kw)
        o = kw.pop("obs", obs)
        with pytest.raises(ValueError, match=text):
            spart_amd.refine_tiles(P, o, "Sentinel2A-MSI", **kw)
    with pytest.raises(ValueError, match="27"):
        spart_amd.refine_tiles(P[:26], obs, "Sentinel2A-MSI", **ok)
    with pytest.raises(ValueError, match="4096"):
        spart_amd.refine_tiles(np.zeros((27, 5000)), np.zeros((5000, 13)), "Sentinel2A-MSI", ["aot550"], tile_start=[0, 5000])
    e = engine.Engine.__new__(engine.Engine)                   # an Engine object that never saw a device
    e.nb = 13
    with pytest.raises(ValueError, match="unknown"):
        e.refine_tiles(P, obs, ["aot550"], ["nope"], tile_size=2)
    with pytest.raises(ValueError, match="obs"):
        e.refine_tiles(P, np.zeros((M, 12)), ["aot550"], tile_size=2)
    with pytest.raises(ValueError, match="exactly one"):
        e.refine_tiles(P, obs, ["aot550"])
    # the partition and the two priors as the device call gets them
    plan, _, m, Fs, wper, ts, lprior, sprior = engine.refine_tiles_args(
        P, obs, ["aot550"], ["LAI", "Cab"], 4, None, None, np.ones((M, 13)), "R_TOA", 3, 1e-3, 1e-2, "literal",
        {"aot550": (np.array([0.1, 0.2]), 0.5), "Cab": (40.0, 2.0)}, "centre")
    assert (m, Fs, wper, ts.tolist()) == (M, 1, 1, [0, 4, 6]) and plan["names"] == ["aot550", "LAI", "Cab"]
    assert lprior[2] == 0 and lprior[0].tolist() == [0.0, 40.0] and lprior[1].tolist() == [0.0, 0.25]
    assert sprior[2] == 1 and sprior[0].tolist() == [[0.1], [0.2]] and sprior[1].tolist() == [[4.0], [4.0]]
    assert engine.tile_starts(0, 5, None).tolist() == [0] and engine.tile_starts(10, 5, None).tolist() == [0, 5, 10]
    assert engine.tile_starts(11, 5, None).tolist() == [0, 5, 10, 11] and engine.tile_starts(3, 4096, None).tolist() == [0, 3]


def test_signatures_structs_and_header_agree():
    from spart_amd import _lib
    opt = ["fit", "n_shared", "band_model", "shared_prior_per_tile", "shared_prior_mean", "shared_prior_weight"]
    out = ["shared", "shared_std", "local", "local_std", "cost", "cost0", "n_accept", "pixel_cost", "status", "y"]
    assert [f[0] for f in _lib.SpartRefineTilesOpt._fields_] == opt and _lib.SpartRefineTilesOpt._fields_[0][1] is _lib.SpartRefineOpt
    assert [f[0] for f in _lib.SpartTilesOut._fields_] == out == list(_lib.TILES_OUTS)
    res, args = _lib.SIGNATURES["spart_refine_tiles"]
    ref = list(_lib.SIGNATURES["spart_refine"][1])
    assert res is ctypes.c_int and len(args) == 16 and args[:7] == ref[:7] and args[7] is ctypes.c_int64 and args[9:11] == ref[7:9]
    assert args[13:] == ref[16:]
    res, args = _lib.SIGNATURES["spart_tiles_workspace_bytes"]
    assert res is ctypes.c_size_t and len(args) == 4
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spart_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct spart_refine_tiles_opt \{(.*?)\} spart_refine_tiles_opt;", header, flags=re.S).group(1)
    assert re.findall(r"\b([A-Za-z_0-9]+)\s*[;,]", body) == opt
    body = re.search(r"typedef struct spart_tiles_out \{(.*?)\} spart_tiles_out;", header, flags=re.S).group(1)
    assert re.findall(r"\b([A-Za-z_0-9]+)\s*[;,]", body) == out
    assert re.search(r"int spart_refine_tiles\(spart_ctx \*ctx, int64_t M, .*?int64_t T, const int64_t \*tile_start", header, flags=re.S)
    full = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    assert "#define SPART_ABI_VERSION 14" in full and "spart_refine_tiles and spart_tiles_workspace_bytes" in full
    assert _lib.TILES_MAXG == 4096 == rtd.MAX_TILE


def test_null_context_is_refused_without_a_gpu():
    """no context: the workspace size is 0 and the call is refused (the sizes of a real context, which needs a device, are in
    tests/test_gpu_refine_tiles.py)"""
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    L = ctypes.CDLL(build.build(verbose=False))
    f = L.spart_tiles_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    assert f(None, 100, 3, 1) == 0
    L.spart_refine_tiles.restype = ctypes.c_int
    L.spart_last_error.restype = ctypes.c_char_p
    assert L.spart_refine_tiles(*([None] * 16)) == -1 and b"spart_refine_tiles: null context" in L.spart_last_error(None)


def test_tiles_kernels_use_no_scratch_and_little_lds(kernel_meta):
    names = ("k_tiles_init", "k_tiles_cost", "k_tiles_decide", "k_tiles_normal", "k_tiles_eliminate", "k_tiles_schur", "k_tiles_local",
             "k_tiles_apply")
    hits = {k: v for k, v in kernel_meta.items() if "k_tiles_" in k}
    assert len(hits) == len(names) and all(any(n in k for k in hits) for n in names), sorted(hits)
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] <= 40960, (name, k)                # static LDS within REFINE_LDS_BUDGET (k_tiles_schur's stage)
    # the dynamic LDS of the two staged kernels stays far inside REFINE_LDS_BUDGET at F = 16
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine_tiles.h")).read()
    assert "(size_t)(refine_ntri(F) + 2 * F) * (TILES_GROUP + 1) * 8" in src and "constexpr int TILES_GROUP = 8;" in src
    assert (136 + 32) * 9 * 8 <= 40960
