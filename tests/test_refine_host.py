"""spart_refine without a GPU: the g++ build (-ffp-contract=off) of the per-observation step functions of csrc/spart_refine.h
(tests/hostmath/refine_host.cpp) against the definition tools/refine_defined.py, bit for bit; the twin experiment with the
oracle as the forward model; and the argument refusals of Engine.refine, spart_amd.refine and retrieve(refine=...) that need
no device."""
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

SRC = os.path.join(ROOT, "tests", "hostmath", "refine_host.cpp")
FS, NBS = (1, 2, 6, 16), (1, 13, 211)


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refine_host") / "librefine_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rh_cost.restype = ctypes.c_double
    L.rh_cost.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                          ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    L.rh_propose.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_double] + [ctypes.POINTER(ctypes.c_double)] * 4
    return L


def host_normal(lib, J, r, w):
    M, nb, F = J.shape
    out = np.zeros((M, F * (F + 1) // 2 + F))
    for m in range(M):
        Jm, rm, wm = (np.ascontiguousarray(a[m]) for a in (J, r, w))
        lib.rh_normal(F, nb, dp(Jm), dp(rm), dp(wm), dp(out[m]))
    return out


def host_propose(lib, packed, lam, x, lo, hi):
    M, F = x.shape
    out = np.zeros((M, F))
    lo, hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
    for m in range(M):
        lib.rh_propose(F, dp(np.ascontiguousarray(packed[m])), float(lam[m]), dp(np.ascontiguousarray(x[m])), dp(lo), dp(hi), dp(out[m]))
    return out


def host_std(lib, packed, F):
    out = np.zeros((packed.shape[0], F))
    for m in range(packed.shape[0]):
        lib.rh_std(F, dp(np.ascontiguousarray(packed[m])), dp(out[m]))
    return out


def jacobian_case(F, nb, seed, M=24):
    """random J / r / w with, by observation: 0-1 plain; 2 zero weights over NaN residuals and NaN J rows; 3 a zero column of J
    (D = 1); 4 a rank-deficient J (two equal columns; one column when F = 1: all zero); 5 a NaN in J under a non-zero weight;
    6 all weights zero; the rest plain with weights over six decades"""
    rng = np.random.default_rng(seed)
    J = rng.normal(0.0, 1.0, (M, nb, F)) * rng.uniform(0.01, 30.0, F)
    r = rng.normal(0.0, 0.05, (M, nb))
    w = 10.0 ** rng.uniform(-3, 3, (M, nb))
    z = rng.random(nb) < 0.4
    z[0] = True
    w[2, z], r[2, z], J[2, z, :] = 0.0, np.nan, np.nan
    J[3, :, F - 1] = 0.0
    J[4, :, 0] = J[4, :, F - 1] if F > 1 else 0.0
    J[5, nb // 2, F // 2] = np.nan
    w[6] = 0.0
    return J, r, w


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("F", FS)
def test_normal_equations_solve_and_std_bit_for_bit(lib, F, nb):
    J, r, w = jacobian_case(F, nb, 1000 * F + nb)
    M = J.shape[0]
    packed = rd.normal_defined(J, r, w)
    assert same(host_normal(lib, J, r, w), packed)
    nt = F * (F + 1) // 2
    assert (packed[6] == 0).all() and packed[3, rd.tri(F - 1, F - 1)] == 0            # all-zero weights; the zero column
    assert np.isnan(packed[5]).any() and (np.isfinite(packed[2]).all() or nb == 1)
    rng = np.random.default_rng(F + nb)
    lo, hi = -rng.uniform(0.5, 2.0, F), rng.uniform(0.5, 2.0, F)
    x = rng.uniform(lo, hi, (M, F))
    x[7], x[8] = lo, hi                                                                # on both bounds
    for lam in (1e-2, rd.LAMBDA_MIN, rd.LAMBDA_MAX, 0.3):
        lamv = np.full(M, lam)
        t = rd.propose_defined(packed, lamv, x, lo, hi)
        assert same(host_propose(lib, packed, lamv, x, lo, hi), t), lam
        assert same(t[5], x[5]) and same(t[6], x[6])                                   # NaN system, zero system: delta = 0
        assert ((t >= lo) & (t <= hi)).all()
    # steps that run into both bounds: a huge gradient with little damping
    big = packed.copy()
    big[:, nt:] *= 1e6
    t = rd.propose_defined(big, np.full(M, 1e-9), x, lo, hi)
    assert same(host_propose(lib, big, np.full(M, 1e-9), x, lo, hi), t)
    if nb >= F:
        assert (t[:2] == lo).any() or (t[:2] == hi).any() or F == 1
    # std on good and singular A
    s = rd.std_defined(packed, F)
    assert same(host_std(lib, packed, F), s)
    assert np.isnan(s[3]).all() and np.isnan(s[6]).all() and np.isnan(s[5]).all()      # D = 1 is for the solve, not for std
    if nb >= F + 4:
        assert np.isfinite(s[:2]).all() and (s[:2] > 0).all()
    if F > 1:
        assert np.isnan(s[4]).all() or nb < F or np.isfinite(s[4]).all()               # rank-deficient: rounding decides which


def test_std_is_the_inverse_diagonal():
    rng = np.random.default_rng(3)
    F = 6
    Jm = rng.normal(size=(1, 40, F))
    packed = rd.normal_defined(Jm, np.zeros((1, 40)), np.ones((1, 40)))
    want = np.sqrt(np.diag(np.linalg.inv(Jm[0].T @ Jm[0])))
    assert np.allclose(rd.std_defined(packed, F)[0], want, rtol=1e-10)
    t = rd.propose_defined(np.concatenate([packed[:, :21], (Jm[0].T @ np.arange(40.0))[None]], axis=1), np.zeros(1) + 1e-300,
                           np.zeros((1, F)), np.full(F, -1e9), np.full(F, 1e9))
    assert np.allclose(t[0], -np.linalg.solve(Jm[0].T @ Jm[0], Jm[0].T @ np.arange(40.0)), rtol=1e-9)


@pytest.mark.parametrize("nb", NBS)
def test_cost_jacobian_and_scalars_bit_for_bit(lib, nb):
    rng = np.random.default_rng(nb)
    M, F = 16, 6
    Y = rng.uniform(0.0, 0.6, (F + 1, M, nb))
    obs = rng.uniform(0.0, 0.6, (M, nb))
    w = 10.0 ** rng.uniform(-2, 4, (M, nb))
    w[1, 0], obs[1, 0] = 0.0, np.nan                         # a masked band
    w[2, nb - 1] = -1.0                                      # dead: negative weight
    w[3, 0] = np.inf
    w[4, 0] = np.nan
    obs[5, nb // 2] = np.nan                                 # dead: NaN observation under a weight
    w[6] = 0.0
    w[7, 0] = -0.0                                           # (minus zero is zero: skipped)
    c, d = rd.cost_defined(Y[0], obs, w)
    bad = rd.bad_weights_defined(w)
    got, gbad = np.zeros(M), np.zeros(M, dtype=np.int32)
    for m in range(M):
        b = ctypes.c_int32(0)
        got[m] = lib.rh_cost(nb, dp(np.ascontiguousarray(Y[0, m])), dp(obs[m]), dp(w[m]), ctypes.byref(b))
        gbad[m] = b.value
    assert same(got, c) and np.array_equal(gbad != 0, bad)
    assert list(np.flatnonzero(bad)) == [2, 3, 4] and np.isnan(c[5]) and c[6] == 0 and np.isfinite(c[1])
    sh = rng.choice([-1.0, 1.0], (M, F)) * rng.uniform(1e-4, 1e-2, F)
    Jd = np.moveaxis((Y[1:] - Y[0][None]) / sh.T[:, :, None], 0, 2)
    for m in range(M):
        J, r = np.zeros((nb, F)), np.zeros(nb)
        lib.rh_jacobian(F, nb, dp(np.ascontiguousarray(Y[:, m])), dp(obs[m]), dp(w[m]), dp(np.ascontiguousarray(sh[m])), dp(J), dp(r))
        assert same(J, Jd[m]) and same(r[w[m] != 0], d[m][w[m] != 0])
    # clip, step sign and the lambda clamps
    n = 64
    lo, hi = np.full(n, -1.0), np.full(n, 2.0)
    v = np.concatenate([rng.uniform(-3, 4, n - 6), [-1.0, 2.0, np.nan, np.inf, -np.inf, 2.0 - 1e-2]])
    out = np.zeros(n)
    lib.rh_clip(ctypes.c_int64(n), dp(v), dp(lo), dp(hi), dp(out))
    assert same(out, rd.clip_defined(v, lo, hi)) and np.isnan(out[n - 4]) and out[n - 3] == 2.0 and out[n - 2] == -1.0
    h = np.full(n, 3e-3)
    t = rd.clip_defined(v, lo, hi)
    lib.rh_fd_step(ctypes.c_int64(n), dp(t), dp(h), dp(hi), dp(out))
    assert same(out, rd.step_sign(t, h, hi) * h) and out[n - 5] == -3e-3 and out[n - 1] == 3e-3 and out[n - 6] == 3e-3
    lam = np.array([1e-2, 1e-12, 5e-12, 1e12, 5e11, 1.0])
    for acc in (0, 1):
        o = np.zeros(lam.size)
        lib.rh_lambda(ctypes.c_int64(lam.size), dp(lam), ip(np.full(lam.size, acc, dtype=np.int32)), dp(o))
        assert same(o, rd.lambda_defined(lam, np.full(lam.size, bool(acc))))
        assert o.min() >= 1e-12 and o.max() <= 1e12


def decide_defined(it, ct, bad, c, lam, na):
    """one observation through the decision lines of refine_defined's loop -> (code, na, lam); code as the kernels flag it:
    0 dead already, 1 accepted, 2 dead from the start, 3 rejected"""
    dead = na < 0
    with np.errstate(all="ignore"):
        accept = bool(ct < c) and not dead and not bad
    if it == 0:
        dead = not accept
        if dead:
            na = -1
    else:
        if not dead:
            lam = float(rd.lambda_defined(np.float64(lam), accept))
        na = na + int(accept)
    return (1 if accept else 2 if it == 0 else 0 if dead else 3), na, lam


DECIDE_CASES = [
    # it, ct, bad, cost, lam, na -> code
    (0, 0.25, 0, np.inf, 1e-2, 0, 1),                        # it = 0: a finite cost
    (0, 0.0, 0, np.inf, 1e-2, 0, 1),
    (0, np.inf, 0, np.inf, 1e-2, 0, 2),                      # +inf
    (0, np.nan, 0, np.inf, 1e-2, 0, 2),                      # NaN
    (0, 0.25, 1, np.inf, 1e-2, 0, 2),                        # finite under a bad weight
    (3, 0.5, 0, 1.0, 1e-2, 2, 1),                            # it > 0: lower
    (3, 1.0, 0, 1.0, 1e-2, 2, 3),                            # equal
    (3, 2.0, 0, 1.0, 1e-2, 2, 3),                            # higher
    (3, np.nan, 0, 1.0, 1e-2, 2, 3),                         # NaN
    (3, np.inf, 0, 1.0, 1e-2, 0, 3),
    (3, 0.5, 0, 1.0, 1e-2, -1, 0),                           # dead already: nothing moves
    (3, np.nan, 0, np.nan, 0.3, -1, 0),
    (1, 0.5, 0, 1.0, rd.LAMBDA_MIN, 0, 1),                   # lambda at its floor, accepted
    (1, 0.5, 0, 1.0, 5e-12, 0, 1),                           # ... and one step above it
    (1, 2.0, 0, 1.0, rd.LAMBDA_MAX, 7, 3),                   # lambda at its cap, rejected
    (1, 2.0, 0, 1.0, 5e11, 7, 3),
]


def test_decision_against_the_definition(lib):
    """refine_decide, the decision every step kernel of the family takes, case by case against the definition's lines"""
    lib.rh_decide.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]
    for it, ct, bad, cost, lam, na, code in DECIDE_CASES:
        out, lo = np.zeros(2, dtype=np.int32), np.zeros(1)
        lib.rh_decide(it, ct, bad, 0.0 if it == 0 else cost, lam, na, ip(out), dp(lo))     # (at it = 0 no cost exists yet)
        want = decide_defined(it, ct, bool(bad), cost, lam, na)
        case = (it, ct, bad, cost, lam, na)
        assert want[0] == code and (int(out[0]), int(out[1])) == want[:2] and same(lo[0], np.float64(want[2])), (case, out, lo, want)
        if code == 0:
            assert out[1] == -1 and same(lo[0], np.float64(lam)), case
        if code == 2:
            assert out[1] == -1 and same(lo[0], np.float64(lam)), case
        if it == 0 and code == 1:
            assert out[1] == 0 and same(lo[0], np.float64(lam)), case              # the first call moves neither
    clamp = {c[4]: decide_defined(*c[:6])[2] for c in DECIDE_CASES if c[0] == 1}
    assert clamp[rd.LAMBDA_MIN] == rd.LAMBDA_MIN == clamp[5e-12] and clamp[rd.LAMBDA_MAX] == rd.LAMBDA_MAX == clamp[5e11]


def test_whole_loop_on_a_toy_model_matches_a_scalar_transcription(lib):
    """refine_defined's loop against a per-observation loop built from the g++ functions, on a cheap nonlinear forward"""
    rng = np.random.default_rng(11)
    M, nb, F, n_iter = 12, 13, 4, 6
    free = [15, 0, 2, 1]
    Wm = rng.normal(size=(27, nb))

    def forward(rows):
        return np.tanh(rows @ Wm * 0.05) + 0.1 * np.sin(rows[:, [0]] * np.arange(1, nb + 1) * 0.01)
    base = rng.uniform(0.0, 1.0, (M, 27))
    lo, hi = np.zeros(F), np.array([2.0, 1.0, 1.0, 1.0])
    truth = base.copy()
    truth[:, free] = rng.uniform(lo, hi, (M, F))
    obs = forward(truth)
    base[0, free[0]] = 5.0                                                      # a start outside the box
    base[1, free[1]] = hi[1]                                                    # exactly on hi: s = -1
    w = 10.0 ** rng.uniform(-1, 1, (M, nb))
    w[2, 3], obs[2, 3] = 0.0, np.nan
    w[3] = 0.0
    obs[4, 5] = np.nan                                                          # dead
    w[5, 1] = -2.0                                                              # dead
    base[6, 20] = np.nan                                                        # dead: a NaN parameter that is not free
    hist = []
    res = rd.refine_defined(base, free, lo, hi, obs, forward, weights=w, n_iter=n_iter, history=hist)
    assert list(res["n_accept"][[4, 5, 6]]) == [-1, -1, -1] and np.isnan(res["std"][[4, 5, 6]]).all()
    assert same(res["x"][4], rd.clip_defined(base[4, free], lo, hi)) and same(res["cost"][[4, 5, 6]], res["cost0"][[4, 5, 6]])
    assert res["cost0"][3] == 0 and res["n_accept"][3] == 0
    alive = res["n_accept"] >= 0
    assert (res["cost"][alive] <= res["cost0"][alive]).all() and (res["cost"][alive][[0, 1]] < 1e-3 * res["cost0"][alive][[0, 1]]).all()
    # the scalar transcription
    h = 1e-3 * (hi - lo)
    for m in range(M):
        x = np.zeros(F)
        lib.rh_clip(ctypes.c_int64(F), dp(np.ascontiguousarray(base[m, free])), dp(lo), dp(hi), dp(x))
        t, c, lam, na, dead = x.copy(), np.inf, 1e-2, 0, False
        packed = np.zeros(F * (F + 1) // 2 + F)
        for it in range(n_iter + 1):
            sh = np.zeros(F)
            lib.rh_fd_step(ctypes.c_int64(F), dp(t), dp(h), dp(hi), dp(sh))
            rows = np.repeat(base[m][None], F + 1, axis=0)
            rows[:, free] = t
            for f in range(F):
                rows[f + 1, free[f]] = t[f] + sh[f]
            Y = np.ascontiguousarray(forward(rows))
            b = ctypes.c_int32(0)
            ct = lib.rh_cost(nb, dp(Y[0]), dp(obs[m]), dp(w[m]), ctypes.byref(b))
            if it == 0 and not (ct < np.inf and not b.value):
                dead, c, na = True, ct, -1
            if dead:
                continue
            acc = ct < c
            if acc:
                x, c = t.copy(), ct
                J, r = np.zeros((nb, F)), np.zeros(nb)
                lib.rh_jacobian(F, nb, dp(Y), dp(obs[m]), dp(w[m]), dp(sh), dp(J), dp(r))
                lib.rh_normal(F, nb, dp(J), dp(r), dp(w[m]), dp(packed))
            if it > 0:
                o = np.zeros(1)
                lib.rh_lambda(ctypes.c_int64(1), dp(np.array([lam])), ip(np.array([int(acc)], dtype=np.int32)), dp(o))
                lam, na = float(o[0]), na + int(acc)
            assert same(x, hist[it][0][m]) and same(np.float64(c), hist[it][1][m]), (m, it)
            if it < n_iter:
                t = np.zeros(F)
                lib.rh_propose(F, dp(packed), lam, dp(x), dp(lo), dp(hi), dp(t))
        assert same(x, res["x"][m]) and same(np.float64(c), res["cost"][m]) and na == res["n_accept"][m], m
        if not dead:
            s = np.zeros(F)
            lib.rh_std(F, dp(packed), dp(s))
            assert same(s, res["std"][m]), m


def test_twin_experiment_with_the_oracle(oracle, tables):
    """48 LHS rows, free = LAI, Cab, Cw, Cdm over their RANGES, starts moved 15 % of the range towards the box centre, ten
    iterations: every observation is back at the truth (the oracle alone: cost / cost0 <= 1.2e-26, |x - truth| <= 4.3e-14
    of the range; the caps below are loose on purpose and allow no exceptions)"""
    from spart_amd import workloads
    names = ["LAI", "Cab", "Cw", "Cdm"]
    free = [workloads.PARAM_NAMES.index(n) for n in names]
    lo = np.array([workloads.RANGES[n][0] for n in names], dtype=np.float64)
    hi = np.array([workloads.RANGES[n][1] for n in names], dtype=np.float64)
    truth = workloads.lhs_params(48, "full", seed=5)
    cache = {}

    def forward(rows):
        key = rows.tobytes()
        if key not in cache:
            with np.errstate(all="ignore"):
                cache[key] = np.asarray(oracle.spart_run(rows, "Sentinel2A-MSI", tables, pso="gl")["R_TOC"], dtype=np.float64)
        return cache[key]
    obs = forward(truth)
    start = truth.copy()
    centre = 0.5 * (lo + hi)
    start[:, free] = truth[:, free] + 0.15 * (hi - lo) * np.sign(centre - truth[:, free])
    res = rd.refine_defined(start, free, lo, hi, obs, forward, n_iter=10)
    assert (res["n_accept"] >= 0).all() and (res["cost"] <= res["cost0"]).all()
    assert (res["cost"] <= 1e-8 * res["cost0"]).all(), float((res["cost"] / res["cost0"]).max())
    err = np.abs(res["x"] - truth[:, free]) / (hi - lo)
    assert (err <= 1e-6).all(), float(err.max())
    # the prefix property: n_iter = 3 is where n_iter = 5 was after its fourth decision, and the cost does not go up
    h3, h5 = [], []
    r3 = rd.refine_defined(start, free, lo, hi, obs, forward, n_iter=3, history=h3)
    r5 = rd.refine_defined(start, free, lo, hi, obs, forward, n_iter=5, history=h5)
    assert same(r3["x"], h5[3][0]) and same(r3["cost"], h5[3][1]) and (r5["cost"] <= r3["cost"]).all()
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(h3, h5))


# ---- refusals that need no device
def test_refine_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    P = workloads.lhs_params(4, "full", seed=1)
    obs = np.zeros((4, 13))
    ok = dict(free=["LAI", "Cab"])
    for kw, text in ((dict(free=[]), "free"), (dict(free=["LAI", "nope"]), "unknown"), (dict(free=["LAI", "LAI"]), "twice"),
                     (dict(free=[workloads.PARAM_NAMES[i] for i in range(17)]), "free"),
                     (dict(free=["SMC"]), "no range"), (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"),
                     (dict(ok, bounds={"LAI": (0.0, np.inf)}), "lo < hi"), (dict(ok, bounds={"Cw": (0.0, 1.0)}), "not free"),
                     (dict(ok, n_iter=101), "n_iter"), (dict(ok, n_iter=-1), "n_iter"), (dict(ok, column="rso"), "column"),
                     (dict(ok, rel_step=-1e-3), "rel_step"), (dict(ok, lambda0=np.nan), "lambda0"), (dict(ok, lidf="fast"), "lidf"),
                     (dict(ok, weights=np.ones((3, 13))), "weights"), (dict(ok, obs=np.zeros((5, 13))), "obs")):
        kw = dict(kw)
        o = kw.pop("obs", obs)
        with pytest.raises(ValueError, match=text):
            spart_amd.refine(P.T, o, "Sentinel2A-MSI", **kw)
    with pytest.raises(ValueError, match="27"):
        spart_amd.refine(P.T[:26], obs, "Sentinel2A-MSI", **ok)
    # Engine.refine itself: the same checks, ahead of any use of the device (an Engine object that was never initialised)
    e = engine.Engine.__new__(engine.Engine)
    e.nb = 13
    with pytest.raises(ValueError, match="unknown"):
        e.refine(list(P.T), obs, ["LAI", "nope"])
    with pytest.raises(ValueError, match="n_iter"):
        e.refine(list(P.T), obs, ["LAI"], n_iter=1000)
    assert engine.refine_plan(["SMC"], {"SMC": (5, 55)}, 3, "L_TOA", 1e-3, 1e-2)["column"] == 2


def test_retrieve_refine_refusals(tmp_path):
    from spart_amd import lut, workloads
    rng = np.random.default_rng(0)
    P = workloads.lhs_params(32, "full", seed=2)

    def write(d, **meta):
        os.makedirs(d)
        np.save(os.path.join(d, "params.npy"), P)
        np.save(os.path.join(d, "R_TOC.npy"), rng.random((32, 13)))
        json.dump(dict({"sensor": "Sentinel2A-MSI", "dtype": "float64", "columns": ["R_TOC"], "rows": 32}, **meta),
                  open(os.path.join(d, "meta.json"), "w"))
        return str(d)
    plain = write(tmp_path / "plain")
    obs = rng.random((3, 13))
    with pytest.raises(ValueError, match="unknown"):
        lut.retrieve(plain, obs, 3, refine=["nope"])
    with pytest.raises(ValueError, match="constant"):
        lut.retrieve(plain, obs, 3, refine=["LAI", "SMC"])                       # SMC is fixed in the LHS: no range in the LUT
    with pytest.raises(ValueError, match="refine_opts"):
        lut.retrieve(plain, obs, 3, refine=["LAI"], refine_opts={"iterations": 3})
    with pytest.raises(ValueError, match="refine_opts"):
        lut.retrieve(plain, obs, 3, refine_opts={"n_iter": 3})                   # options without refine=
    with pytest.raises(ValueError, match="srf"):
        lut.retrieve(write(tmp_path / "srf", band_model="srf"), obs, 3, refine=["LAI"])
    with pytest.raises(ValueError, match="sensor"):
        lut.retrieve(write(tmp_path / "custom", sensor=None), obs, 3, refine=["LAI"])
