"""The Gaussian prior of spart_refine without a GPU: the g++ build (-ffp-contract=off) of refine_prior_cost / refine_prior_gain
beside the step functions of csrc/spart_refine.h (tests/hostmath/refine_prior_host.cpp) against the definition
tools/refine_defined.py, bit for bit; the whole loop with a prior on the toy forward model; the definition's own invariants,
with a verbatim copy of the loop as it was before the prior; the same loop as a stand-alone -fsanitize=address,undefined
program; and the argument refusals of refine_plan, spart_amd.refine, retrieve and retrieve_stream that need no device."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "refine_prior_host.cpp")
FS = (1, 2, 6, 16)
D = ctypes.POINTER(ctypes.c_double)


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def dp(a):
    return a.ctypes.data_as(D)


def ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refine_prior_host") / "librefine_prior_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rh_cost.restype = ctypes.c_double
    L.rh_cost.argtypes = [ctypes.c_int, D, D, D, ctypes.POINTER(ctypes.c_int32)]
    L.rh_propose.argtypes = [ctypes.c_int, D, ctypes.c_double] + [D] * 4
    L.rp_prior_cost.restype = ctypes.c_double
    L.rp_prior_cost.argtypes = [ctypes.c_int, ctypes.c_double, D, D, D, ctypes.POINTER(ctypes.c_int32)]
    L.rp_prior_normal.argtypes = [ctypes.c_int, D, D, D, D]
    return L


def prior_case(rng, M, F, lo, hi, truth, per_obs):
    """means = truth + noise of 10 % of the range, sigma = 10 % of the range, about 20 % zero weights with NaN means under them"""
    shape = (M, F) if per_obs else (F,)
    mu = (truth if per_obs else truth[0]) + 0.1 * rng.normal(size=shape) * (hi - lo)
    sigma = np.broadcast_to(0.1 * (hi - lo), shape)
    p = 1.0 / (sigma * sigma)
    zero = rng.random(shape) < 0.2
    return np.where(zero, np.nan, mu), np.where(zero, 0.0, p)


@pytest.mark.parametrize("per_obs", (False, True))
@pytest.mark.parametrize("F", FS)
def test_prior_cost_and_augmented_sums_bit_for_bit(lib, F, per_obs):
    rng = np.random.default_rng(100 * F + per_obs)
    M, nb = 24, 13
    lo, hi = -rng.uniform(0.5, 2.0, F), rng.uniform(0.5, 2.0, F)
    t = rng.uniform(lo, hi, (M, F))
    mu, p = prior_case(rng, M, F, lo, hi, t, per_obs)
    mu, p = rd.prior_defined(mu, p, M, F)
    assert (p == 0).any() or F < 6
    assert np.isnan(mu[p == 0]).all() and np.isfinite(mu[p != 0]).all()
    p[3, F - 1], mu[3, F - 1] = -1.0, 0.0                                          # bad weights: flagged, still summed
    p[4, 0], mu[4, 0] = np.inf, 0.0
    p[5, 0], mu[5, 0] = np.nan, 0.0
    p[6, F // 2], mu[6, F // 2] = 7.0, np.nan                                      # a NaN mean under a weight: a NaN cost
    p[7, :] = 0.0
    p[8, 0] = -0.0                                                                 # (minus zero is zero: skipped)
    c0 = rng.uniform(0.0, 5.0, M)
    c, e = rd.prior_cost_defined(c0, t, mu, p)
    got, bad = np.zeros(M), np.zeros(M, dtype=bool)
    for m in range(M):
        b = ctypes.c_int32(0)
        got[m] = lib.rp_prior_cost(F, float(c0[m]), dp(np.ascontiguousarray(t[m])), dp(mu[m]), dp(p[m]), ctypes.byref(b))
        bad[m] = b.value != 0
    assert same(got, c) and np.array_equal(bad, rd.bad_weights_defined(p))
    assert list(np.flatnonzero(bad)) == [3, 4, 5] and np.isnan(c[6]) and c[7] == c0[7] and np.isfinite(c[[0, 1, 2, 8]]).all()
    # the packed sums: random band sums, then the prior's terms
    J = rng.normal(0.0, 1.0, (M, nb, F)) * rng.uniform(0.01, 30.0, F)
    r = rng.normal(0.0, 0.05, (M, nb))
    w = 10.0 ** rng.uniform(-3, 3, (M, nb))
    w[9] = 0.0                                                                     # the prior alone
    packed = rd.normal_defined(J, r, w)
    want = rd.prior_normal_defined(packed, e, p)
    out = packed.copy()
    for m in range(M):
        lib.rp_prior_normal(F, dp(np.ascontiguousarray(t[m])), dp(mu[m]), dp(p[m]), dp(out[m]))
    assert same(out, want)
    nt = F * (F + 1) // 2
    diag = [rd.tri(a, a) for a in range(F)]
    assert same(want[7], packed[7])                                                # all weights zero: nothing added
    assert same(want[9, diag], p[9]) and same(want[9, nt:], np.where(p[9] == 0, 0.0, p[9] * e[9]))
    off = np.setdiff1d(np.arange(nt), diag)
    assert same(want[:, off], packed[:, off])                                      # only the diagonal and g change
    assert np.isnan(want[6, nt + F // 2]) and (want[0, diag] >= packed[0, diag]).all()


# ---- today's loop without the prior, verbatim (tools/refine_defined.py as it was before prior_mean / prior_weight)
def refine_defined_before_the_prior(base, free, lo, hi, obs, forward, weights=None, n_iter=10, rel_step=1e-3, lambda0=1e-2, history=None):
    base = np.ascontiguousarray(base, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    free = [int(f) for f in free]
    F, (M, nb) = len(free), obs.shape
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not 1 <= F <= rd.MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[1]:
        raise ValueError("free: 1 ... 16 distinct column numbers")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    if not 0 <= int(n_iter) <= rd.MAX_ITER:
        raise ValueError("n_iter: 0 ... 100")
    w = rd.weights_defined(weights, M, nb)
    bad = rd.bad_weights_defined(w)
    h = rel_step * (hi - lo)
    x = rd.clip_defined(base[:, free], lo, hi)
    t = x.copy()
    c = np.full(M, np.inf)
    cost0 = np.full(M, np.nan)
    lam = np.full(M, float(lambda0))
    n_accept = np.zeros(M, dtype=np.int32)
    dead = np.zeros(M, dtype=bool)
    packed = np.zeros((M, F * (F + 1) // 2 + F))
    y = np.full((M, nb), np.nan)
    for it in range(int(n_iter) + 1):
        sh = rd.step_sign(t, h, hi) * h
        rows = np.repeat(base[None], F + 1, axis=0)                 # (F + 1, M, 27): p_0, p_1 ... p_F
        rows[:, :, free] = t[None]
        with np.errstate(all="ignore"):
            for f in range(F):
                rows[f + 1, :, free[f]] = t[:, f] + sh[:, f]
        Y = np.asarray(forward(rows.reshape(-1, base.shape[1])), dtype=np.float64).reshape(F + 1, M, nb)
        ct, d = rd.cost_defined(Y[0], obs, w)
        with np.errstate(all="ignore"):
            accept = (ct < c) & ~dead & ~bad
        if it == 0:
            cost0 = ct.copy()
            dead = ~accept
            c = np.where(dead, ct, c)
            y = np.where(dead[:, None], Y[0], y)
            n_accept[dead] = -1
        if accept.any():
            with np.errstate(all="ignore"):
                J = np.moveaxis((Y[1:] - Y[0][None]) / sh.T[:, :, None], 0, 2)       # (M, nb, F)
            packed = np.where(accept[:, None], rd.normal_defined(J, d, w), packed)
        x = np.where(accept[:, None], t, x)
        c = np.where(accept, ct, c)
        y = np.where(accept[:, None], Y[0], y)
        if it > 0:
            lam = np.where(dead, lam, rd.lambda_defined(lam, accept))
            n_accept = n_accept + accept.astype(np.int32)
        if history is not None:
            history.append((x.copy(), c.copy()))
        if it == int(n_iter):
            break
        t = np.where(dead[:, None], t, rd.propose_defined(packed, lam, x, lo, hi))
    std = np.where(dead[:, None], np.nan, rd.std_defined(packed, F))
    return {"x": x, "cost": c, "cost0": cost0, "std": std, "n_accept": n_accept, "y": y}


def toy_case():
    """the toy forward model and rows of test_refine_host's whole-loop test, with a per-observation prior.  Rows: 0 a start
    outside the box, 1 a start on hi, 2 a masked NaN band, 3 all band weights zero, 4 a NaN observation (dead), 5 a negative
    band weight (dead), 6 a NaN fixed parameter (dead), 7 a negative prior weight (dead), 8 a NaN mean under a weight (dead),
    9 a NaN mean under a zero weight (alive)"""
    rng = np.random.default_rng(11)
    M, nb, F = 12, 13, 4
    free = [15, 0, 2, 1]
    Wm = rng.normal(size=(27, nb))

    def forward(rows):
        return np.tanh(rows @ Wm * 0.05) + 0.1 * np.sin(rows[:, [0]] * np.arange(1, nb + 1) * 0.01)
    base = rng.uniform(0.0, 1.0, (M, 27))
    lo, hi = np.zeros(F), np.array([2.0, 1.0, 1.0, 1.0])
    truth = base.copy()
    truth[:, free] = rng.uniform(lo, hi, (M, F))
    obs = forward(truth)
    base[0, free[0]] = 5.0
    base[1, free[1]] = hi[1]
    w = 10.0 ** rng.uniform(-1, 1, (M, nb))
    w[2, 3], obs[2, 3] = 0.0, np.nan
    w[3] = 0.0
    obs[4, 5] = np.nan
    w[5, 1] = -2.0
    base[6, 20] = np.nan
    mu, p = prior_case(rng, M, F, lo, hi, truth[:, free], True)
    mu[3], p[3] = truth[3, free], 100.0                                         # a full prior where no band counts
    mu[3, 0] = 2.5                                                              # ... one mean outside the box
    p[7, 1], mu[7, 1] = -1.0, 0.5
    p[8, 2], mu[8, 2] = 50.0, np.nan
    p[9, 0], mu[9, 0] = 0.0, np.nan
    for m in (0, 1, 2, 9, 10, 11):                                              # (rows that must stay alive)
        mu[m] = np.where(p[m] == 0, np.nan, np.where(np.isnan(mu[m]), 0.5, mu[m]))
    return base, free, lo, hi, obs, w, mu, p, forward


def test_whole_loop_with_a_prior_matches_a_scalar_transcription(lib):
    base, free, lo, hi, obs, w, mu, p, forward = toy_case()
    M, nb = obs.shape
    F, n_iter = len(free), 6
    hist = []
    res = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=n_iter, history=hist, prior_mean=mu, prior_weight=p)
    dead = [4, 5, 6, 7, 8]
    assert list(np.flatnonzero(res["n_accept"] == -1)) == dead and np.isnan(res["std"][dead]).all()
    assert np.isnan(res["cost0"][8]) and np.isfinite(res["cost0"][7]) and same(res["cost"][dead], res["cost0"][dead])
    alive = res["n_accept"] >= 0
    assert (res["cost"][alive] <= res["cost0"][alive]).all() and (res["n_accept"][alive] >= 1).sum() >= 5
    assert np.isfinite(res["std"][3]).all() and res["n_accept"][3] >= 1         # the prior makes the weightless row solvable
    h = 1e-3 * (hi - lo)
    for m in range(M):
        x = np.zeros(F)
        lib.rh_clip(ctypes.c_int64(F), dp(np.ascontiguousarray(base[m, free])), dp(lo), dp(hi), dp(x))
        t, c, lam, na, gone = x.copy(), np.inf, 1e-2, 0, False
        packed = np.zeros(F * (F + 1) // 2 + F)
        for it in range(n_iter + 1):
            sh = np.zeros(F)
            lib.rh_fd_step(ctypes.c_int64(F), dp(t), dp(h), dp(hi), dp(sh))
            rows = np.repeat(base[m][None], F + 1, axis=0)
            rows[:, free] = t
            for f in range(F):
                rows[f + 1, free[f]] = t[f] + sh[f]
            Y = np.ascontiguousarray(forward(rows))
            b, pb = ctypes.c_int32(0), ctypes.c_int32(0)
            ct = lib.rh_cost(nb, dp(Y[0]), dp(obs[m]), dp(w[m]), ctypes.byref(b))
            ct = lib.rp_prior_cost(F, ct, dp(t), dp(mu[m]), dp(p[m]), ctypes.byref(pb))
            if it == 0 and not (ct < np.inf and not b.value and not pb.value):
                gone, c, na = True, ct, -1
            if gone:
                continue
            acc = ct < c
            if acc:
                x, c = t.copy(), ct
                J, r = np.zeros((nb, F)), np.zeros(nb)
                lib.rh_jacobian(F, nb, dp(Y), dp(obs[m]), dp(w[m]), dp(sh), dp(J), dp(r))
                lib.rh_normal(F, nb, dp(J), dp(r), dp(w[m]), dp(packed))
                lib.rp_prior_normal(F, dp(t), dp(mu[m]), dp(p[m]), dp(packed))
            if it > 0:
                o = np.zeros(1)
                lib.rh_lambda(ctypes.c_int64(1), dp(np.array([lam])), ip(np.array([int(acc)], dtype=np.int32)), dp(o))
                lam, na = float(o[0]), na + int(acc)
            assert same(x, hist[it][0][m]) and same(np.float64(c), hist[it][1][m]), (m, it)
            if it < n_iter:
                t = np.zeros(F)
                lib.rh_propose(F, dp(packed), lam, dp(x), dp(lo), dp(hi), dp(t))
        assert same(x, res["x"][m]) and same(np.float64(c), res["cost"][m]) and na == res["n_accept"][m], m
        if not gone:
            s = np.zeros(F)
            lib.rh_std(F, dp(packed), dp(s))
            assert same(s, res["std"][m]), m


def test_the_definitions_own_invariants():
    base, free, lo, hi, obs, w, mu, p, forward = toy_case()
    F = len(free)
    # without a prior: today's file, bit for bit (both spellings of "no prior")
    old = refine_defined_before_the_prior(base, free, lo, hi, obs, forward, weights=w, n_iter=6)
    for kw in ({}, dict(prior_mean=None, prior_weight=None)):
        new = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=6, **kw)
        assert all(same(new[k], old[k]) for k in old)
    # weights that are all exactly 0 skip every term of the prior, NaN means included
    zero = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=6, prior_mean=np.full(F, np.nan), prior_weight=np.zeros(F))
    assert all(same(zero[k], old[k]) for k in old)
    # a shared prior is the per-observation prior with equal rows
    a = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=4, prior_mean=mu[0], prior_weight=p[0])
    b = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=4, prior_mean=np.tile(mu[0], (12, 1)),
                          prior_weight=np.tile(p[0], (12, 1)))
    assert all(same(a[k], b[k]) for k in a)
    # the prefix property and cost <= cost0, with a prior
    h3, h5 = [], []
    r3 = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=3, history=h3, prior_mean=mu, prior_weight=p)
    r5 = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=5, history=h5, prior_mean=mu, prior_weight=p)
    assert same(r3["x"], h5[3][0]) and same(r3["cost"], h5[3][1])
    assert all(same(u[0], v[0]) and same(u[1], v[1]) for u, v in zip(h3, h5))
    for r in (r3, r5):
        alive = r["n_accept"] >= 0
        assert alive.sum() == 7 and (r["cost"][alive] <= r["cost0"][alive]).all()
    assert (r5["cost"][alive] <= r3["cost"][alive]).all()
    with pytest.raises(ValueError):
        rd.refine_defined(base, free, lo, hi, obs, forward, prior_mean=mu)
    with pytest.raises(ValueError):
        rd.refine_defined(base, free, lo, hi, obs, forward, prior_mean=mu[:5], prior_weight=p[:5])


def test_without_band_weights_the_fit_goes_to_the_clipped_prior_mean():
    """all band weights zero and a full prior: the cost is the prior's quadratic, so the loop must end at clip(mu) and std at
    1 / sqrt(p) = sigma; 1e-6 of the range after 12 iterations is a closed-form property (the damping alone leaves a factor
    lambda / (1 + lambda) <= 1e-2 per accepted step)"""
    base, free, lo, hi, obs, w, mu, p, forward = toy_case()
    M, F = mu.shape
    rng = np.random.default_rng(5)
    mu = rng.uniform(lo - 0.3, hi + 0.3, (M, F))                                 # some means outside the box
    sigma = rng.uniform(0.05, 0.5, (M, F)) * (hi - lo)
    p = 1.0 / (sigma * sigma)
    base = np.where(np.isnan(base), 0.5, base)
    res = rd.refine_defined(base, free, lo, hi, np.where(np.isnan(obs), 0.1, obs), forward, weights=np.zeros(13), n_iter=12,
                            prior_mean=mu, prior_weight=p)
    assert (res["n_accept"] >= 0).all()
    want = rd.clip_defined(mu, lo, hi)
    err = np.abs(res["x"] - want) / (hi - lo)
    assert (err <= 1e-6).all(), float(err.max())
    assert (want != mu).any() and (want == mu).any()
    assert np.allclose(res["std"], sigma, rtol=1e-12)


def test_the_loop_with_priors_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """the .cpp's own main (the whole loop on a toy model, with shared, masked, negative and NaN priors, heap buffers of exact
    size) as a stand-alone -fsanitize=address,undefined program in a child process; the sanitizer runtimes are linked into the
    program itself, so nothing is preloaded and nothing sanitised is loaded into python"""
    exe = str(tmp_path / "refine_prior_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-DREFINE_PRIOR_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "WRONG" not in r.stdout and r.stdout.count(" ok") == 10 and "Sanitizer" not in r.stderr
    assert "obs 2: n_accept -1" in r.stdout and "obs 3: n_accept -1" in r.stdout


# ---- refusals that need no device
def test_prior_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    P = workloads.lhs_params(4, "full", seed=1)
    obs = np.zeros((4, 13))
    free = ["LAI", "Cab"]
    good = {"LAI": (3.0, 1.0), "Cab": (np.full(4, 40.0), np.array([10.0, np.inf, 5.0, 1.0]))}
    plan = engine.refine_plan(free, None, 3, "R_TOC", 1e-3, 1e-2, prior=good)
    mean, weight = engine.prior_arrays(plan["prior"], 4)
    assert same(mean, np.array([[3.0, 40.0]] * 4)) and same(weight, np.array([[1.0, 0.01], [1.0, 0.0], [1.0, 0.04], [1.0, 1.0]]))
    mean, weight = engine.prior_arrays(engine.refine_plan(free, None, 3, "R_TOC", 1e-3, 1e-2, prior={"Cab": (40.0, 0.3)})["prior"], 4)
    assert same(mean, [0.0, 40.0]) and same(weight, [0.0, 1.0 / (0.3 * 0.3)])   # names not listed: weight 0
    assert engine.refine_plan(free, None, 3, "R_TOC", 1e-3, 1e-2)["prior"] is None
    bad = (({"Cw": (0.01, 0.01)}, "not free"), ({"LAI": (3.0, 0.0)}, "sigma"), ({"LAI": (3.0, -1.0)}, "sigma"),
           ({"LAI": (3.0, np.nan)}, "sigma"), ({"LAI": (3.0, np.array([1.0, 1.0, 0.0, 1.0]))}, "sigma"),
           ({"LAI": (np.zeros(3), 1.0)}, r"\(M,\)"), ({"LAI": (np.zeros((4, 1)), 1.0)}, r"\(M,\)"),
           ({"LAI": (np.zeros(4), 1.0), "Cab": (1.0, np.ones(5))}, r"\(M,\)"), ({"LAI": 3.0}, "mean, sigma"), ("knn", "dict"))
    for prior, text in bad:
        with pytest.raises(ValueError, match=text):
            spart_amd.refine(P.T, obs, "Sentinel2A-MSI", free, prior=prior)
    with pytest.raises(ValueError, match="not free"):
        engine.refine_plan(free, None, 3, "R_TOC", 1e-3, 1e-2, prior={"N": (1.5, 0.1)})
    ready = dict(prior_mean=np.zeros(2), prior_weight=np.ones(2))
    with pytest.raises(ValueError, match="exclude"):
        spart_amd.refine(P.T, obs, "Sentinel2A-MSI", free, prior=good, **ready)
    for kw, text in ((dict(prior_mean=np.zeros(2)), "together"), (dict(prior_weight=np.zeros(2)), "together"),
                     (dict(prior_mean=np.zeros(3), prior_weight=np.zeros(3)), "expected both"),
                     (dict(prior_mean=np.zeros((4, 2)), prior_weight=np.zeros(2)), "expected both"),
                     (dict(prior_mean=np.zeros((3, 2)), prior_weight=np.zeros((3, 2))), "expected both")):
        with pytest.raises(ValueError, match=text):
            spart_amd.refine(P.T, obs, "Sentinel2A-MSI", free, **kw)
    # Engine.refine itself, on an Engine object that was never initialised
    e = engine.Engine.__new__(engine.Engine)
    e.nb = 13
    with pytest.raises(ValueError, match="exclude"):
        e.refine(list(P.T), obs, free, prior=good, **ready)
    with pytest.raises(ValueError, match="not free"):
        e.refine(list(P.T), obs, free, prior={"Cw": (0.01, 0.01)})
    with pytest.raises(ValueError, match=r"\(M,\)"):
        e.refine(list(P.T), obs, free, prior={"LAI": (np.zeros(5), 1.0)})
    with pytest.raises(ValueError, match="together"):
        e.refine(list(P.T), obs, free, prior_mean=np.zeros(2))


def test_the_binding_speaks_abi_14_and_old_keywords_still_build_the_struct():
    from spart_amd import _lib
    assert _lib.ABI_VERSION == 14
    names = [n for n, _ in _lib.SpartRefineOpt._fields_]
    assert names[-3:] == ["prior_per_obs", "prior_mean", "prior_weight"] and names[:7] == [
        "column", "n_iter", "weights_per_obs", "fast_prelude", "nlayers", "rel_step", "lambda0"]
    o = _lib.SpartRefineOpt(column=1, n_iter=3, weights_per_obs=0, fast_prelude=0, nlayers=0, rel_step=1e-3, lambda0=1e-2)
    assert o.prior_per_obs == 0 and o.prior_mean is None and o.prior_weight is None
    assert ctypes.sizeof(_lib.SpartRefineOpt) == 64 and _lib.SpartRefineOpt.prior_mean.offset == 48
    header = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    assert "#define SPART_ABI_VERSION 14" in header and " *  14: spart_refine_opt.prior_per_obs" in header


def write_lut(d, P, rng, **meta):
    os.makedirs(d)
    np.save(os.path.join(d, "params.npy"), P)
    np.save(os.path.join(d, "R_TOC.npy"), rng.random((P.shape[0], 13)))
    json.dump(dict({"sensor": "Sentinel2A-MSI", "dtype": "float64", "columns": ["R_TOC"], "rows": P.shape[0]}, **meta),
              open(os.path.join(d, "meta.json"), "w"))
    return str(d)


def test_retrieve_and_retrieve_stream_prior_refusals(tmp_path):
    from spart_amd import lut, workloads
    rng = np.random.default_rng(0)
    P = workloads.lhs_params(32, "full", seed=2)
    plain = write_lut(tmp_path / "plain", P, rng)
    obs = rng.random((3, 13))
    assert "prior" in lut.REFINE_OPTS and "prior_floor" in lut.REFINE_OPTS
    for call in (lut.retrieve, lut.retrieve_stream):
        for opts, text in (({"prior": "nearest"}, "prior"), ({"prior": 3.0}, "prior"), ({"prior": {"Cab": (40.0, 1.0)}}, "not free"),
                           ({"prior": {"LAI": (3.0, 0.0)}}, "sigma"), ({"prior": {"LAI": (3.0, np.nan)}}, "sigma"),
                           ({"prior": {"LAI": (np.zeros(4), 1.0)}}, r"\(M,\)"), ({"prior": "knn", "prior_floor": -1.0}, "floor"),
                           ({"prior_floor": 0.1}, "prior_floor"), ({"prior_mean": np.zeros(1)}, "refine_opts")):
            with pytest.raises(ValueError, match=text):
                call(plain, obs, 3, refine=["LAI"], refine_opts=opts)
    # retrieve_stream(refine=...) refuses what retrieve refuses
    with pytest.raises(ValueError, match="unknown"):
        lut.retrieve_stream(plain, obs, 3, refine=["nope"])
    with pytest.raises(ValueError, match="constant"):
        lut.retrieve_stream(plain, obs, 3, refine=["LAI", "SMC"])
    with pytest.raises(ValueError, match="refine_opts"):
        lut.retrieve_stream(plain, obs, 3, refine=["LAI"], refine_opts={"iterations": 3})
    with pytest.raises(ValueError, match="refine_opts"):
        lut.retrieve_stream(plain, obs, 3, refine_opts={"n_iter": 3})
    with pytest.raises(ValueError, match="srf"):
        lut.retrieve_stream(write_lut(tmp_path / "srf", P, rng, band_model="srf"), obs, 3, refine=["LAI"])
    with pytest.raises(ValueError, match="sensor"):
        lut.retrieve_stream(write_lut(tmp_path / "custom", P, rng, sensor=None), obs, 3, refine=["LAI"])
    bad_out = {n: np.zeros((3, 27)) for n in lut.STREAM_MAPS}
    bad_out.update(count=np.zeros(3, dtype=np.int32), best_cost=np.zeros(3))
    with pytest.raises(ValueError, match="refined"):                              # out= must carry the refined arrays too
        lut.retrieve_stream(plain, obs, 3, refine=["LAI"], out=bad_out)


def test_knn_prior_is_its_two_line_definition():
    import torch
    from spart_amd import knn_prior
    rng = np.random.default_rng(8)
    M, F = 50, 5
    lo, hi = rng.uniform(-1, 0, F), rng.uniform(0.5, 80, F)
    mean = rng.uniform(lo, hi, (M, F))
    std = rng.uniform(0.0, 0.3, (M, F)) * (hi - lo)
    std[0] = 0.0                                                                   # k identical rows
    mean[1], std[1] = np.nan, np.nan                                               # an observation without rows
    std[2, 3] = np.nan
    for floor in (0.05, 0.2, 0.0):
        kw = {} if floor == 0.05 else {"floor": floor}
        pm, pw = knn_prior(mean, std, lo, hi, **kw)
        with np.errstate(all="ignore"):
            sigma = np.maximum(std, floor * (hi - lo))
            weight = 1.0 / (sigma * sigma)
        none = np.isnan(mean) | np.isnan(std)
        assert same(pm, np.where(none, 0.0, mean)) and same(pw, np.where(none, 0.0, weight))
        assert (pw[1] == 0).all() and (pm[1] == 0).all() and pw[2, 3] == 0 and pm[2, 3] == 0 and pw.dtype == np.float64
        if floor > 0:
            assert same(pw[0], 1.0 / ((floor * (hi - lo)) * (floor * (hi - lo)))) and np.isfinite(pw).all()
        else:
            assert np.isinf(pw[0]).all()                                           # no floor: identical rows pin the parameter
        tm, tw = knn_prior(torch.as_tensor(mean), torch.as_tensor(std), lo, hi, **kw)     # torch on the host: the same bits
        assert same(tm.numpy(), pm) and same(tw.numpy(), pw)
    with pytest.raises(ValueError, match="floor"):
        knn_prior(mean, std, lo, hi, floor=np.nan)
