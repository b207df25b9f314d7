"""spart_refine_views without a GPU: the definition tools/refine_views_defined.py against tools/refine_defined.py where the two
must agree (V = 1); the g++ build (-ffp-contract=off) of the index maps of csrc/spart_refine_views.h and of a per-pixel loop
built from them (tests/hostmath/refine_views_host.cpp) against the definition on a cheap nonlinear forward, bit for bit; the
refusals of Engine.refine_views / spart_amd.refine_views that need no device; the workspace size; and the kernels' resources."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402
import refine_views_defined as rvd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "refine_views_host.cpp")
OUTS = ("x", "cost", "cost0", "std", "n_accept", "y")
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
    so = str(tmp_path_factory.mktemp("refine_views_host") / "librefine_views_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rvh_chunk.restype = ctypes.c_int64
    L.rvh_cost.restype = L.rvh_prior_cost.restype = L.rvh_lambda.restype = ctypes.c_double
    L.rvh_cost.argtypes = [ctypes.c_int] * 3 + [c_dp] * 3 + [ctypes.c_int, c_ip]
    L.rvh_sums.argtypes = [ctypes.c_int] * 4 + [c_dp] * 3 + [ctypes.c_int, c_dp, c_dp]
    L.rvh_prior_cost.argtypes = [ctypes.c_int, ctypes.c_double, c_dp, c_dp, c_dp, c_ip]
    L.rvh_lambda.argtypes = [ctypes.c_double, ctypes.c_int]
    L.rvh_propose.argtypes = [ctypes.c_int, c_dp, ctypes.c_double] + [c_dp] * 4
    return L


def toy_forward(nb, seed=0):
    Wm = np.random.default_rng(seed).normal(size=(27, nb))

    def forward(rows):
        with np.errstate(all="ignore"):
            return np.tanh(rows @ Wm * 0.05) + 0.1 * np.sin(rows[:, [0]] * np.arange(1, nb + 1) * 0.01)
    return forward


def toy_case(V, Fs, Fl, kind, with_prior, seed, M=9, nb=7):
    """random pixels on the toy forward.  nb = 7: a 16-band tile holds two whole views and a part of a third.  Special pixels:
    0 a shared (else local) start outside the box, 1 the last free name on hi in the last view only, 2 a masked last view
    (per-pixel weights), 3 a NaN fixed parameter in the last view (dead), 4 a negative weight (per-pixel weights; dead), 5 a NaN
    in view V-1's entry of a shared column (ignored when V > 1)"""
    rng = np.random.default_rng(seed)
    free = [15, 0, 2, 1][:Fs + Fl]
    shared, local = free[:Fs], free[Fs:]
    F, n = Fs + Fl, Fs + V * Fl
    lo, hi = np.zeros(F), np.array([2.0, 1.0, 1.0, 1.0])[:F]
    forward = toy_forward(nb)
    base = rng.uniform(0.0, 1.0, (V, M, 27))
    base[:, :, shared] = base[0][None][:, :, shared]
    truth = base.copy()
    obs = np.moveaxis(forward(truth.reshape(-1, 27)).reshape(V, M, nb), 0, 1) * (1 + 0.01 * rng.normal(size=(M, V, nb)))
    base[:, :, free] = rd.clip_defined(base[:, :, free] + rng.uniform(-0.1, 0.1, (V, M, F)) * (hi - lo), lo, hi)
    base[1:, :, shared] = base[0][None][:, :, shared]
    base[0, 0, free[0]] = 5.0
    base[V - 1, 1, free[-1]] = hi[-1]
    base[V - 1, 3, 20] = np.nan
    if V > 1 and Fs:
        base[V - 1, 5, shared[0]] = np.nan
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 1, nb)
        w[2] = 0.0
    elif kind == "per_pixel":
        w = 10.0 ** rng.uniform(-1, 1, (M, V, nb))
        w[rng.random((M, V, nb)) < 0.15] = 0.0
        w[2, V - 1] = 0.0
        w[4, 0, 1] = -2.0
        obs[w == 0.0] = np.nan
    mu = pw = None
    if with_prior:
        mu = rng.uniform(0.0, 1.0, (M, n))
        pw = 10.0 ** rng.uniform(-2, 1, (M, n))
        pw[:, 0] = 0.0
        mu[6, 0] = np.nan                                                        # under a zero weight
    return dict(base=base, shared=shared, local=local, lo=lo, hi=hi, obs=obs, weights=w, prior_mean=mu, prior_weight=pw), forward


# ---- the definition against refine_defined
@pytest.mark.parametrize("kind", ["none", "shared", "per_pixel"])
@pytest.mark.parametrize("Fs,Fl", [(2, 0), (4, 0), (1, 2), (0, 3)])
def test_one_view_is_refine_defined(Fs, Fl, kind):
    case, forward = toy_case(1, Fs, Fl, kind, Fl == 2, 10 * Fs + Fl)
    got = rvd.refine_views_defined(forward=forward, n_iter=4, **case)
    w = case["weights"]
    ref = rd.refine_defined(case["base"][0], case["shared"] + case["local"], case["lo"], case["hi"], case["obs"][:, 0], forward,
                            weights=w if w is None or w.ndim == 1 else w[:, 0], n_iter=4, prior_mean=case["prior_mean"],
                            prior_weight=case["prior_weight"])
    for k in OUTS:
        assert same(got[k].reshape(ref[k].shape), ref[k]), k
    assert (ref["n_accept"] >= 1).sum() >= 4 and (ref["n_accept"] == -1).sum() >= 1


def test_definition_properties():
    """locals of different views do not couple; a masked view keeps its locals; prefix property; cost <= cost0"""
    case, forward = toy_case(3, 1, 2, "per_pixel", False, 5)
    h3, h5 = [], []
    r3 = rvd.refine_views_defined(forward=forward, n_iter=3, history=h3, **case)
    r5 = rvd.refine_views_defined(forward=forward, n_iter=5, history=h5, **case)
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(h3, h5)) and same(r3["x"], h5[3][0])
    alive = r5["n_accept"] >= 0
    assert (r5["cost"][alive] <= r5["cost0"][alive]).all() and list(np.flatnonzero(~alive)) == [3, 4]
    start = rd.clip_defined(case["base"][2, 2, case["local"]], case["lo"][1:], case["hi"][1:])
    assert same(r5["x"][2, 5:7], start) and np.isnan(r5["std"][2]).all() and r5["n_accept"][2] >= 1
    assert r5["n_accept"][5] >= 0 and np.isfinite(r5["x"][5]).all()                  # the NaN in view 2's shared entry is not read
    case["prior_mean"], case["prior_weight"] = np.full(7, 0.5), np.array([0, 0, 0, 0, 0, 4.0, 4.0])
    rp = rvd.refine_views_defined(forward=forward, n_iter=5, **case)
    assert np.isfinite(rp["std"][2]).all() and not same(rp["x"][2, 5:7], start)
    act = rvd.active_defined(3, 1, 2, 7)
    assert act.shape == (21, 7) and act[:, 0].all() and act[7:14, 3:5].all() and not act[7:14, [1, 2, 5, 6]].any()


# ---- the g++ build against the definition
def test_index_maps(lib):
    for V, Fs, Fl in [(1, 2, 0), (2, 2, 0), (3, 3, 1), (3, 4, 4), (5, 1, 2), (2, 0, 2), (64, 1, 0), (4, 16, 0), (16, 0, 1)]:
        n, F = Fs + V * Fl, Fs + Fl
        name, view, unk = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(V * F, np.int32)
        lib.rvh_maps(V, Fs, Fl, ip(name), ip(view), ip(unk))
        assert list(name) == [rvd.name_of(a, Fs, Fl) for a in range(n)] and list(view) == [rvd.view_of(a, Fs, Fl) for a in range(n)]
        assert list(unk) == [rvd.unknown_of(v, f, Fs, Fl) for v in range(V) for f in range(F)]
        assert sorted(set(unk)) == list(range(n))
        assert all(unk[view[a] * F + name[a]] == a for a in range(n) if view[a] >= 0)
    assert lib.rvh_max_v() == rvd.MAX_V == 64
    assert lib.rvh_chunk(64, 16) == 481 and lib.rvh_chunk(1, 5) == (1 << 19) // 6 and lib.rvh_chunk(64, 16) * 17 * 64 <= 1 << 19


def host_loop(lib, case, forward, n_iter, rel_step=1e-3, lambda0=1e-2):
    """refine_views_defined's loop, one pixel at a time, from the g++ functions -> the same dict"""
    base, obs, w = case["base"], case["obs"], case["weights"]
    V, M, _ = base.shape
    nb = obs.shape[2]
    Fs, Fl = len(case["shared"]), len(case["local"])
    F, n = Fs + Fl, Fs + V * Fl
    P = n * (n + 1) // 2 + n
    free = np.array(case["shared"] + case["local"], dtype=np.int32)
    lo, hi = case["lo"], case["hi"]
    h = rel_step * (hi - lo)
    wper = int(w is not None and w.ndim == 3)
    res = {"x": np.zeros((M, n)), "cost": np.zeros(M), "cost0": np.zeros(M), "std": np.full((M, n), np.nan),
           "n_accept": np.zeros(M, np.int32), "y": np.zeros((M, V, nb))}
    for m in range(M):
        bm, om = np.ascontiguousarray(base[:, m]), np.ascontiguousarray(obs[m]).reshape(-1)
        wm = None if w is None else np.ascontiguousarray(w[m] if wper else w).reshape(-1)
        mu = pw = None
        if case["prior_weight"] is not None:
            mu, pw = (np.ascontiguousarray(np.broadcast_to(case[k], (M, n))[m]) for k in ("prior_mean", "prior_weight"))
        x, lo_n, hi_n, h_n = (np.zeros(n) for _ in range(4))
        lib.rvh_start(V, Fs, Fl, dp(bm), ip(free), dp(lo), dp(hi), dp(h), dp(x), dp(lo_n), dp(hi_n), dp(h_n))
        t, c, lam, na, dead = x.copy(), np.inf, lambda0, 0, False
        packed, y = np.zeros(P), None
        for it in range(n_iter + 1):
            sh, rows = np.zeros(n), np.zeros((V, F + 1, 27))
            lib.rvh_rows(V, Fs, Fl, dp(bm), ip(free), dp(t), dp(h_n), dp(hi_n), dp(sh), dp(rows))
            Y = np.ascontiguousarray(forward(rows.reshape(-1, 27)).reshape(V, F + 1, nb))
            b = ctypes.c_int32(0)
            ct = lib.rvh_cost(V, F, nb, dp(Y), dp(om), dp(wm), wper, ctypes.byref(b))
            if pw is not None:
                ct = lib.rvh_prior_cost(n, ct, dp(t), dp(mu), dp(pw), ctypes.byref(b))
            if it == 0:
                res["cost0"][m] = ct
                if not (ct < np.inf and not b.value):
                    dead, c, na, y = True, ct, -1, Y[:, 0].copy()
            if dead:
                break
            acc = ct < c
            if acc:
                x, c, y = t.copy(), ct, Y[:, 0].copy()
                lib.rvh_sums(V, Fs, Fl, nb, dp(Y), dp(om), dp(wm), wper, dp(sh), dp(packed))
                if pw is not None:
                    lib.rvh_prior_normal(n, dp(packed), dp(x), dp(mu), dp(pw))
            if it > 0:
                lam, na = lib.rvh_lambda(lam, int(acc)), na + int(acc)
            if it < n_iter:
                t = np.zeros(n)
                lib.rvh_propose(n, dp(packed), lam, dp(x), dp(lo_n), dp(hi_n), dp(t))
        res["x"][m], res["cost"][m], res["n_accept"][m], res["y"][m] = x, c, na, y
        if not dead:
            lib.rvh_std(n, dp(packed), dp(res["std"][m]))
    return res


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind", ["none", "shared", "per_pixel"])
@pytest.mark.parametrize("Fs,Fl", [(2, 0), (1, 2), (0, 3), (3, 1)])
@pytest.mark.parametrize("V", [1, 2, 5])
def test_per_pixel_loop_from_the_header_matches_the_definition(lib, V, Fs, Fl, kind, with_prior):
    case, forward = toy_case(V, Fs, Fl, kind, with_prior, 100 * V + 10 * Fs + Fl)
    ref = rvd.refine_views_defined(forward=forward, n_iter=4, **case)
    got = host_loop(lib, case, forward, 4)
    for k in OUTS:
        assert same(got[k], ref[k]), (k, got[k], ref[k])
    live = ref["n_accept"] >= 0
    assert live.sum() >= 6 and (ref["n_accept"] >= 1).sum() >= 5, ref["n_accept"]
    assert ref["n_accept"][3] == -1 and (kind != "per_pixel" or ref["n_accept"][4] == -1)
    assert ref["n_accept"][5] >= 0 and (ref["cost"][live] <= ref["cost0"][live]).all()


# ---- refusals that need no device
def test_refine_views_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    M, V = 4, 3
    P = np.repeat(workloads.lhs_params(M, "full", seed=1).T[:, None, :], V, axis=1)          # (27, V, M)
    obs = np.zeros((M, V, 13))
    ok = dict(shared=["LAI", "Cab"], local=["aot550"])
    for kw, text in ((dict(shared=[], local=[]), "free"), (dict(shared=["LAI"], local=["nope"]), "unknown"),
                     (dict(shared=["LAI"], local=["LAI"]), "twice"), (dict(shared=["LAI"], local=["Cab", "Cw", "Cdm", "N", "B", "q"]), "unknowns"),
                     (dict(ok, obs=np.zeros((M, 13))), "obs"), (dict(ok, obs=np.zeros((M, 65, 13)), shared=["LAI"], local=[]), "views"),
                     (dict(ok, obs=np.zeros((M, 0, 13))), "views"), (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"),
                     (dict(ok, bounds={"Cw": (0.0, 1.0)}), "not free"), (dict(ok, n_iter=101), "n_iter"), (dict(ok, column="rso"), "column"),
                     (dict(ok, rel_step=-1e-3), "rel_step"), (dict(ok, lidf="fast"), "lidf"), (dict(ok, band_model="wide"), "band_model"),
                     (dict(ok, weights=np.ones((M, 13))), "weights"), (dict(ok, weights=np.ones((V, 13))), "weights"),
                     (dict(ok, prior={"Cw": (0.0, 1.0)}), "not free"), (dict(ok, prior={"LAI": (1.0, -1.0)}), "sigma"),
                     (dict(ok, prior={"LAI": (np.zeros(V), 1.0)}), "pixels"), (dict(ok, prior={"aot550": (np.zeros(M + 1), 1.0)}), "shape"),
                     (dict(ok, prior={"LAI": (np.zeros(M + 1), 1.0)}), "pixels"),
                     (dict(ok, prior={"LAI": (1.0, 1.0)}, prior_mean=np.zeros(5), prior_weight=np.zeros(5)), "exclude"),
                     (dict(ok, prior_mean=np.zeros(4), prior_weight=np.zeros(4)), "prior_mean"),
                     (dict(ok, prior_mean=np.zeros(5)), "come together")):
        kw = dict(kw)
        o = kw.pop("obs", obs)
        with pytest.raises(ValueError, match=text):
            spart_amd.refine_views(P, o, "Sentinel2A-MSI", **kw)
    with pytest.raises(ValueError, match="27"):
        spart_amd.refine_views(P[:26], obs, "Sentinel2A-MSI", **ok)
    with pytest.raises(ValueError, match="broadcast"):
        spart_amd.refine_views([0.0] * 26 + [np.zeros(M + 1)], obs, "Sentinel2A-MSI", **ok)
    e = engine.Engine.__new__(engine.Engine)                   # an Engine object that never saw a device
    e.nb = 13
    with pytest.raises(ValueError, match="unknown"):
        e.refine_views(P, obs, ["LAI", "nope"])
    with pytest.raises(ValueError, match="unknowns"):
        e.refine_views(P, obs, ["LAI"], ["Cab", "Cw", "Cdm", "N", "B", "q"])
    with pytest.raises(ValueError, match="obs"):
        e.refine_views(P, np.zeros((M, V, 12)), ["LAI"])
    # the prior per unknown: a shared scalar, a local (V,) and a local (M, V)
    mean, weight = engine._views_prior(["LAI", "aot550", "uo3"], 1, V, {"LAI": (3.0, 2.0), "aot550": (np.arange(V), 0.5)})
    assert mean.tolist() == [3.0, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0] and weight.tolist() == [0.25, 4.0, 0.0, 4.0, 0.0, 4.0, 0.0]
    mean, weight = engine._views_prior(["LAI", "aot550"], 1, V, {"aot550": (np.arange(M * V).reshape(M, V), np.inf)})
    assert mean.shape == (M, 4) and (mean[:, 1:] == np.arange(M * V).reshape(M, V)).all() and (weight == 0).all()


def test_signatures_struct_and_header_agree():
    import re
    from spart_amd import _lib
    assert [f[0] for f in _lib.SpartRefineViewsOpt._fields_] == ["fit", "V", "n_shared", "band_model"]
    assert _lib.SpartRefineViewsOpt._fields_[0][1] is _lib.SpartRefineOpt
    res, args = _lib.SIGNATURES["spart_refine_views"]
    ref = list(_lib.SIGNATURES["spart_refine"][1])
    assert res is ctypes.c_int and len(args) == 19 and [a for i, a in enumerate(args) if i != 9] == [a for i, a in enumerate(ref) if i != 9]
    assert len(_lib.SIGNATURES["spart_views_workspace_bytes"][1]) == 5
    header = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    body = re.search(r"typedef struct spart_refine_views_opt \{(.*?)\} spart_refine_views_opt;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b([A-Za-z_0-9]+)\s*;", body) == ["fit", "V", "n_shared", "band_model"]
    assert "#define SPART_ABI_VERSION 14" in header and "spart_refine_views_opt were added by the same rule" in header


def test_null_context_is_refused_without_a_gpu():
    """no context: the workspace size is 0 and the call is refused (the sizes of a real context, which needs a device, are in
    tests/test_gpu_refine_views.py)"""
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    L = ctypes.CDLL(build.build(verbose=False))
    f = L.spart_views_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert f(None, 100, 2, 3, 1) == 0
    L.spart_refine_views.restype = ctypes.c_int
    L.spart_last_error.restype = ctypes.c_char_p
    assert L.spart_refine_views(*([None] * 19)) == -1 and b"spart_refine_views: null context" in L.spart_last_error(None)


def test_views_kernels_use_no_scratch(kernel_meta):
    hits = {k: v for k, v in kernel_meta.items() if "k_refine_views_" in k}
    assert any("k_refine_views_init" in k for k in hits) and any("k_refine_views_step" in k for k in hits), sorted(hits)
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)                   # all LDS is the launcher's dynamic region


def test_views_lds_stays_within_the_budget_of_k_refine_step():
    """refine_lds_rows(F + 1, n, 0) is at most refine_lds_rows(17, 16, 0) for every (V, Fs, Fl) the call accepts, so the
    budget rule picks a W whose LDS k_refine_step already takes at F = 16"""
    def rows(F, n):
        nt = n * (n + 1) // 2
        return (F + 1) * 16 + 2 * 16 + (nt + n) + nt + 3 * n + 1
    csrc = os.path.join(ROOT, "spart-python_amd", "csrc")
    assert "tile_rows * REFINE_JT + 2 * REFINE_JT + (refine_ntri(n) + n) + refine_ntri(n) + 3 * n + 1 + extra" in open(os.path.join(csrc, "spart_refine.h")).read()
    assert "rows = refine_lds_rows(F + 1, n, 0), W = refine_group(rows)" in open(os.path.join(csrc, "spart_capi.hip")).read()
    worst = 0
    for V in range(1, 65):
        for F in range(1, 17):
            for Fs in range(F + 1):
                n = Fs + V * (F - Fs)
                if 1 <= n <= 16:
                    worst = max(worst, rows(F, n))
    assert worst == rows(16, 16) and worst * 5 * 8 <= 40960
