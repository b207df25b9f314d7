"""spart_sample without a GPU: the Philox known answers; the g++ build (-ffp-contract=off) of part 1 of csrc/spart_sample.h
(tests/hostmath/sample_host.cpp) driven through whole runs against the definition tools/sample_defined.py, bit for bit, with the
CPU oracle as forward model (the 48-row twin case of test_refine_posterior_host); the same driver as a stand-alone
-fsanitize=address,undefined program; the sampler against posteriors that are known in closed form; the prefix / resume and
obs_offset identities; chain_summary on synthetic chains; header, binding and the argument refusals that need no device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sample_defined as sd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "sample_host.cpp")
D = ctypes.POINTER(ctypes.c_double)
S2 = "Sentinel2A-MSI"
MARGIN = 1e-12
F16 = ["Cab", "Cdm", "Cw", "Cs", "Cca", "Cant", "N", "B", "SMp", "LAI", "LIDFa", "LIDFb", "q", "aot550", "uo3", "uh2o"]
FREE = {1: ["LAI"], 2: ["LAI", "Cab"], 4: ["LAI", "Cab", "Cw", "Cdm"], 6: ["LAI", "Cab", "Cw", "Cdm", "N", "LIDFa"], 16: F16}
CASES = [(F, W) for F in (1, 2, 6, 16) for W in sd.WALKERS if W >= 2 * F]
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def dp(a):
    return None if a is None else a.ctypes.data_as(D)


class SphState(ctypes.Structure):
    _fields_ = [("S", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in ("x", "c", "sum", "Q", "x0", "bx", "bc", "na", "dead", "zp", "u2",
                                                                         "inside")]


class SphOut(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in sd.OUTS]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sample_host") / "libsample_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    U = ctypes.POINTER(ctypes.c_uint32)
    i, i64, u64, dbl = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    L.sph_philox.argtypes = [U, U, U]
    L.sph_u53.restype, L.sph_u53.argtypes = dbl, [ctypes.c_uint32, ctypes.c_uint32]
    L.sph_keep.restype, L.sph_keep.argtypes = i64, [i64, i64, i64]
    L.sph_chunk.restype, L.sph_chunk.argtypes = i64, [i]
    L.sph_init.argtypes = [i, i, i, u64, u64, u64, dbl, D, D, D, D, D, ctypes.POINTER(SphState)]
    L.sph_table.argtypes = [i, i, i, i, i, u64, u64, u64, dbl, D, D, ctypes.POINTER(SphState), D]
    L.sph_step.argtypes = [i, i, i, i, i, i, i, i64, i64, dbl, dbl, D, D, D, D, i, D, D, i, ctypes.POINTER(SphState), ctypes.POINTER(SphOut)]
    return L


def host_run(lib, base, free, lo, hi, obs, forward, weights=None, prior_mean=None, prior_weight=None, W=8, n_steps=4, burn=0, thin=1,
             a=0.0, temperature=0.0, rel_init=0.0, init_radius=None, init=None, step0=0, obs_offset=0, seed=0, S=1):
    """the whole run of sample_defined through the g++ build, the way the chunk loop of the library drives its kernels"""
    base, obs = np.ascontiguousarray(base, dtype=np.float64), np.ascontiguousarray(obs, dtype=np.float64)
    F, (M, nb), H = len(free), obs.shape, W // 2
    a, temperature, rel_init, n_keep = sd.check_options(F, W, n_steps, burn, thin, a, temperature, rel_init, step0, obs_offset)
    nt = F * (F + 1) // 2
    strided = lambda n: np.full(max((n - 1) * S + 1, 1), -3.0)     # noqa: E731
    st = {"x": strided(M * W * F), "c": strided(M * W), "sum": strided(M * F), "Q": strided(M * nt), "x0": np.zeros(M * F),
          "bx": np.zeros(M * F), "bc": np.zeros(M), "na": np.zeros(M, dtype=np.int64), "dead": np.zeros(M, dtype=np.int32),
          "zp": np.zeros(M * H), "u2": np.zeros(M * H), "inside": np.zeros(M * H, dtype=np.int32)}
    state = SphState(S=S, **{k: v.ctypes.data for k, v in st.items()})
    shapes = {"mean": (M, F), "cov": (M, F, F), "std": (M, F), "best_x": (M, F), "best_cost": (M,), "n_accept": (M,), "status": (M,),
              "chain": (M, n_keep, W, F), "chain_cost": (M, n_keep, W), "last": (M, W, F), "last_cost": (M, W)}
    res = {k: np.full(shapes[k], -7, dtype={"n_accept": np.int64, "status": np.int32}.get(k, np.float64)) for k in sd.OUTS}
    out = SphOut(**{k: v.ctypes.data for k, v in res.items()})
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    pm = None if prior_mean is None else np.ascontiguousarray(prior_mean, dtype=np.float64)
    pw = None if prior_weight is None else np.ascontiguousarray(prior_weight, dtype=np.float64)
    rad = None if init_radius is None else np.ascontiguousarray(init_radius, dtype=np.float64)
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
    lib.sph_init(M, F, W, seed, obs_offset, step0, rel_init, dp(np.ascontiguousarray(base[:, free])), dp(lo), dp(hi), dp(rad), dp(ini),
                 ctypes.byref(state))
    rows = np.zeros((M * H, F))
    for rel in range(n_steps + 1):
        for h in (0, 1):
            lib.sph_table(M, F, W, h, int(rel == 0), seed, obs_offset, step0 + rel, a, dp(lo), dp(hi), ctypes.byref(state), dp(rows))
            table = np.repeat(base, H, axis=0)
            table[:, free] = rows
            Y = np.ascontiguousarray(forward(table), dtype=np.float64)
            lib.sph_step(M, F, nb, W, h, int(rel == 0), int(rel == n_steps), -1 if rel == 0 else lib.sph_keep(rel, burn, thin), n_keep,
                         2.0 * temperature, float(n_keep * W), dp(Y), dp(rows), dp(obs), dp(w), int(w is not None and w.ndim == 2),
                         dp(pm), dp(pw), int(pw is not None and pw.ndim == 2), ctypes.byref(state), ctypes.byref(out))
    return res


def differing(got, ref):
    return [k for k in sd.OUTS if not same(got[k], ref[k])]


# ---- known answers
def test_philox_and_u53_known_answers(lib):
    for ctr, key, want in KNOWN:
        assert tuple(int(v) for v in sd.philox4x32(*ctr, *key)) == want
        c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
        lib.sph_philox(c, k, o)
        assert tuple(o) == want
    for u53 in (sd.u53, lib.sph_u53):
        assert float(u53(0, 0)) == 0.0 and float(u53(0xffffffff, 0xffffffff)) == 1.0 - 2.0 ** -53
    # the block of the definition is the counter layout of the header
    w = sd.block((7 << 32) | 5, np.array([(3 << 32) | 9], dtype=np.uint64), (1 << 32) + 11, 33, 2)
    assert [int(v[0]) for v in w] == [int(v) for v in sd.philox4x32(9, 3, 11, (33 << 8) | 2, 5, 7)]
    assert [lib.sph_keep(r, 2, 2) for r in range(1, 7)] == [-1, -1, -1, 0, -1, 1] and lib.sph_chunk(64) == (1 << 19) // 32


# ---- the g++ build against the definition, the oracle as forward model
@pytest.fixture(scope="module")
def twin(oracle, tables):
    """test_refine_posterior_host's case: Sentinel-2A, 48 LHS rows; obs is the model at the truth"""
    from spart_amd import workloads
    truth = workloads.lhs_params(48, "full", seed=5)
    cache = {}

    def forward(rows):
        """row by row through a cache: the definition and the g++ run ask for the same rows"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        keys = [r.tobytes() for r in rows]
        miss = sorted({k for k in keys if k not in cache})
        if miss:
            with np.errstate(all="ignore"):
                Y = np.asarray(oracle.spart_run(np.frombuffer(b"".join(miss), dtype=np.float64).reshape(len(miss), -1), S2, tables,
                                                pso="gl")["R_TOC"], dtype=np.float64)
            cache.update(zip(miss, Y))
        return np.stack([cache[k] for k in keys])
    obs = forward(truth)
    return {"truth": truth, "forward": forward, "obs": obs, "w": 1.0 / (0.02 * np.maximum(obs, 0.01)) ** 2}


def fit_of(names):
    from spart_amd import workloads
    return ([workloads.PARAM_NAMES.index(n) for n in names], np.array([workloads.RANGES[n][0] for n in names], dtype=np.float64),
            np.array([workloads.RANGES[n][1] for n in names], dtype=np.float64))


def twin_case(twin, F, W, rows=slice(0, 48)):
    """the arguments of one run on the rows of the twin: per-observation weights with masked bands (one of them a NaN
    observation), a prior per observation, the start 30 % of the range off the truth where that is near a bound, and planted dead
    rows: 1 a negative band weight, 2 an infinite prior weight, 3 a zero radius"""
    free, lo, hi = fit_of(FREE[F])
    base, obs, w = twin["truth"][rows].copy(), twin["obs"][rows].copy(), twin["w"][rows].copy()
    M = base.shape[0]
    w[:, 3] = 0.0
    obs[0, 3] = np.nan
    sigma = 0.3 * (hi - lo)
    pm, pw = base[:, free] + 0.05 * (hi - lo), np.tile(1.0 / (sigma * sigma), (M, 1))
    pw[0, F - 1] = 0.0
    pm[0, F - 1] = np.nan
    radius = np.tile(0.02 * (hi - lo), (M, 1))
    w[1, 5], pw[2, 0], radius[3, 0] = -1.0, np.inf, 0.0
    base[4, free[0]] = hi[0]                                     # a start ON the bound: proposals leave the box
    kw = dict(weights=w, prior_mean=pm, prior_weight=pw, W=W, n_steps=4, burn=1, thin=2, init_radius=radius, step0=5, obs_offset=1000,
              seed=F * 1000 + W)
    return (base, free, lo, hi, obs, twin["forward"]), kw


@pytest.mark.parametrize("F,W", CASES)
def test_the_compiled_run_is_the_definition_bit_for_bit(lib, twin, F, W):
    args, kw = twin_case(twin, F, W)
    ref = sd.sample_defined(*args, **kw)
    assert ref["margin"] > MARGIN, ref["margin"]
    assert np.array_equal(np.flatnonzero(ref["status"]), [1, 2, 3]) and (ref["status"][1:4] == -1).all()
    assert np.isnan(ref["mean"][1:4]).all() and (ref["n_accept"][1:4] == -1).all()
    assert np.isfinite(np.delete(ref["chain"], [1, 2, 3], axis=0)).all() and ref["chain"].shape == (48, 1, W, F)
    # non-vacuity, on the definition: some proposals accepted, some rejected by u2, some outside the box
    assert ref["n_accepted"] > 0 and ref["n_rejected"] > 0 and ref["n_outside"] > 0, [ref[k] for k in ("n_accepted", "n_rejected", "n_outside")]
    for S in (1, 3):
        got = host_run(lib, *args, S=S, **kw)
        assert not differing(got, ref), (S, differing(got, ref))
    # a given ensemble, resumed: three live observations of the run above from its own last
    live = [0, 4, 5]
    args2 = (args[0][live],) + args[1:4] + (args[4][live], args[5])
    kw2 = {k: (v[live] if k in ("weights", "prior_mean", "prior_weight", "init_radius") else v) for k, v in kw.items()}
    kw2.update(init=ref["last"][live], step0=9, n_steps=2, burn=0, thin=1)
    ref2 = sd.sample_defined(*args2, **kw2)
    assert ref2["margin"] > MARGIN and (ref2["status"] == 0).all()
    got2 = host_run(lib, *args2, S=2, **kw2)
    assert not differing(got2, ref2), differing(got2, ref2)
    bad = ref["last"][live].copy()
    bad[1, W - 1, 0] = np.nan                                    # a NaN coordinate of a given ensemble kills its observation
    bad[2, 0, F - 1] = args[3][F - 1] + 1.0                      # and so does one outside the box
    kw2["init"] = bad
    ref3, got3 = sd.sample_defined(*args2, **kw2), host_run(lib, *args2, **kw2)
    assert np.array_equal(ref3["status"], [0, -1, -1]) and not differing(got3, ref3)


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """the .cpp's own main (every F and W, two strides, a dead row; heap buffers of exact size) as a stand-alone
    -fsanitize=address,undefined program in a child process; the sanitizer runtimes are linked into the program itself, so
    nothing is preloaded and nothing sanitised is loaded into python"""
    exe = str(tmp_path / "sample_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-DSAMPLE_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "WRONG" not in r.stdout and r.stdout.count(" ok") == len(CASES) and "Sanitizer" not in r.stderr


# ---- the identities, on a linear forward model
def linear_case(F, nb, M, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    A = rng.normal(0.0, 1.0, (nb, F))
    base = np.zeros((M, 27))
    free = list(range(2, 2 + F))
    base[:, free] = rng.uniform(0.3, 0.7, (M, F))
    forward = lambda rows: rows[:, free] @ A.T     # noqa: E731
    obs = forward(base) + rng.normal(0.0, sigma, (M, nb))
    return A, (base, free, np.zeros(F), np.ones(F), obs, forward), dict(weights=np.full(nb, 1.0 / sigma ** 2))


@pytest.mark.parametrize("compiled", (False, True))
def test_prefix_resume_and_obs_offset(lib, compiled):
    _, args, kw = linear_case(3, 6, 5, 11)
    run = (lambda *a, **k: host_run(lib, *a, **k)) if compiled else sd.sample_defined
    kw.update(W=8, seed=99, rel_init=0.05)
    whole = run(*args, n_steps=10, burn=0, thin=1, **kw)
    first = run(*args, n_steps=6, burn=0, thin=1, **kw)
    rest = run(*args, n_steps=4, burn=0, thin=1, init=first["last"], step0=6, **kw)
    assert same(rest["last"], whole["last"]) and same(rest["last_cost"], whole["last_cost"])
    assert same(first["chain"], whole["chain"][:, :6]) and same(rest["chain"], whole["chain"][:, 6:])
    assert same(rest["chain_cost"], whole["chain_cost"][:, 6:])
    assert np.array_equal(first["n_accept"] + rest["n_accept"], whole["n_accept"]) and 0 < whole["n_accept"].min()
    # rows [2, 5) with obs_offset = 2 are rows 2 ... 4 of the whole call, in every output
    part = run(args[0][2:], *args[1:4], args[4][2:], args[5], n_steps=10, burn=0, thin=1, obs_offset=2, **kw)
    assert not [k for k in sd.OUTS if not same(part[k], whole[k][2:])]
    other = run(*args, n_steps=10, burn=0, thin=1, **dict(kw, seed=100))
    assert not same(other["chain"], whole["chain"])


# ---- the algorithm samples what it claims
def chain_summary(chain, **kw):
    from spart_amd import chain_summary as cs
    return cs(chain, **kw)


def test_a_gaussian_posterior_well_inside_the_box():
    """F = 3, nb = 6, W = 16, 6000 steps, burn 1000; y = A x with noise sigma: the posterior is N(xhat, (A^T A / sigma^2)^-1).
    Observed: acceptance 0.65, tau about 47 steps, the mean within 1.2 standard errors, variance ratios 0.96 - 0.98."""
    sigma = 0.02
    A, args, kw = linear_case(3, 6, 1, 3, sigma)
    res = sd.sample_defined(*args, W=16, n_steps=6000, burn=1000, seed=1, **kw)
    cov = np.linalg.inv(A.T @ A / sigma ** 2)
    xhat = cov @ (A.T @ args[4][0] / sigma ** 2)
    assert ((xhat - 6 * np.sqrt(np.diag(cov)) > 0) & (xhat + 6 * np.sqrt(np.diag(cov)) < 1)).all()        # well inside
    s = chain_summary(res["chain"][0])
    var = np.diag(cov)
    print("acceptance", res["n_accept"][0] / (16 * 6000), "tau", s["tau"], "ess", s["ess"], "mean error / se",
          (res["mean"][0] - xhat) / np.sqrt(var / s["ess"]), "variance ratios", np.diag(res["cov"][0]) / var)
    assert (np.abs(res["mean"][0] - xhat) <= 5 * np.sqrt(var / s["ess"])).all()
    assert (np.abs(np.diag(res["cov"][0]) / var - 1) <= 5 * np.sqrt(2 / s["ess"])).all()
    assert same(res["std"][0], np.sqrt(np.diag(res["cov"][0]))) and same(res["cov"][0], res["cov"][0].T)


def test_a_gaussian_posterior_cut_by_a_bound():
    """F = 2, W = 8, 8000 steps, burn 1000; a correlated Gaussian (rho = 0.6) with its mode 0.6 sigma below hi_0, against the
    moments of the TRUNCATED Gaussian by grid integration.  Rejection at the bound samples the truncated density; clipping, or
    no bound at all, would not: the untruncated mode must FAIL the bound the sample mean meets."""
    s0, s1, rho = 0.05, 0.08, 0.6
    C = np.array([[s0 * s0, rho * s0 * s1], [rho * s0 * s1, s1 * s1]])
    mode = np.array([1.0 - 0.6 * s0, 0.5])
    Lc = np.linalg.cholesky(np.linalg.inv(C))                    # cost = |L^T (x - mode)|^2: y = L^T x, unit weights
    base = np.zeros((1, 27))
    free = [4, 9]
    base[0, free] = mode
    forward = lambda rows: rows[:, free] @ Lc     # noqa: E731
    res = sd.sample_defined(base, free, np.zeros(2), np.ones(2), forward(base), forward, W=8, n_steps=8000, burn=1000, seed=2, rel_init=0.02)
    g0, g1 = np.linspace(0.0, 1.0, 4001), np.linspace(0.0, 1.0, 2001)
    X0, X1 = np.meshgrid(g0, g1, indexing="ij")
    d = np.stack([X0 - mode[0], X1 - mode[1]], axis=-1)
    p = np.exp(-0.5 * np.einsum("...a,ab,...b->...", d, np.linalg.inv(C), d))
    p /= p.sum()
    true_mean = np.array([(p * X0).sum(), (p * X1).sum()])
    true_var = np.array([(p * (X0 - true_mean[0]) ** 2).sum(), (p * (X1 - true_mean[1]) ** 2).sum()])
    s = chain_summary(res["chain"][0])
    se = np.sqrt(true_var / s["ess"])
    print("acceptance", res["n_accept"][0] / (8 * 8000), "tau", s["tau"], "mean error / se", (res["mean"][0] - true_mean) / se,
          "mode distance / se", (mode - true_mean) / se, "variance ratios", np.diag(res["cov"][0]) / true_var)
    assert (res["chain"][0] <= 1.0).all() and (res["chain"][0] >= 0.0).all() and not (res["chain"][0] == 1.0).any()
    assert (np.abs(res["mean"][0] - true_mean) <= 5 * se).all()
    assert (np.abs(np.diag(res["cov"][0]) / true_var - 1) <= 5 * np.sqrt(2 / s["ess"])).all()
    assert np.abs(mode[0] - true_mean[0]) > 5 * se[0]


# ---- chain_summary
def test_chain_summary_on_synthetic_chains():
    rng = np.random.default_rng(0)
    phi, T = 0.5, 100000
    e = rng.normal(0.0, 1.0, T)
    x = np.empty(T)
    x[0] = e[0]
    for t in range(1, T):
        x[t] = phi * x[t - 1] + e[t]
    s = chain_summary(x[:, None, None])
    want = (1 + phi) / (1 - phi)
    assert abs(s["tau"][0] / want - 1) <= 0.2 and abs(s["ess"][0] * s["tau"][0] / T - 1) < 1e-12, s
    assert abs(s["rhat"][0] - 1) < 0.01
    assert np.allclose(s["quantiles"][:, 0], np.quantile(x, [0.05, 0.5, 0.95]))
    two = rng.normal(0.0, 1.0, (3, 400, 8, 2))
    two[:, 200:, :, 1] += 2.0                                    # the halves of parameter 1 disagree
    s = chain_summary(two, q=(0.5,))
    assert s["quantiles"].shape == (3, 1, 2) and s["rhat"].shape == s["tau"].shape == s["ess"].shape == (3, 2)
    assert (s["rhat"][:, 1] > 1.1).all() and (np.abs(s["rhat"][:, 0] - 1) < 0.05).all()
    import torch
    t = chain_summary(torch.as_tensor(two), q=(0.5,))
    assert all(same(t[k], s[k]) for k in s)
    with pytest.raises(ValueError):
        chain_summary(np.zeros((3, 2)))


# ---- header, binding, loader, refusals without a device
def test_struct_signature_and_header_agree(tmp_path):
    from spart_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    assert "spart_sample_workspace_bytes" in hdr and "int spart_sample(" in hdr
    assert _lib.SAMPLE_OUTS == sd.OUTS and tuple(n for n, _ in SphOut._fields_) == sd.OUTS
    # the ctypes mirror against the compiler's layout of the header's structs
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spart_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(spart_sample_opt), offsetof(spart_sample_opt, prior_mean), offsetof(spart_sample_opt, W), "
                   "offsetof(spart_sample_opt, n_steps), offsetof(spart_sample_opt, seed), sizeof(spart_sample_out)); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    O = _lib.SpartSampleOpt
    assert got == [ctypes.sizeof(O), O.prior_mean.offset, O.W.offset, O.n_steps.offset, O.seed.offset, ctypes.sizeof(_lib.SpartSampleOut)], got
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct spart_sample_opt \{(.*?)\} spart_sample_opt;", hdr, re.S).group(1), flags=re.S)
    assert [n for n, _ in O._fields_] == re.findall(r"(\w+)\s*[;,]", body)
    assert _lib.SAMPLE_WALKERS == sd.WALKERS and _lib.SAMPLE_MAX_STEPS == sd.MAX_STEPS


def test_the_built_library_exports_the_symbols():
    from spart_amd import _lib
    so = os.path.join(ROOT, "spart-python_amd", "libspart_hip.so")
    if not os.path.exists(so):
        import build
        build.build(verbose=False)
    names = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert " spart_sample\n" in names and " spart_sample_workspace_bytes\n" in names
    assert "spart_sample" in _lib.SIGNATURES and "spart_sample_workspace_bytes" in _lib.SIGNATURES


def test_sample_arguments_are_checked_before_the_gpu_is_asked_for(monkeypatch):
    import spart_amd
    from spart_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: pytest.fail("a device was asked for"))
    monkeypatch.setattr(spart_amd.lut, "get_engine", lambda *a, **k: pytest.fail("a device was asked for"))
    P = np.tile(spart_amd.workloads.default_row().T, (1, 3))
    obs = np.zeros((3, 13))
    ok = dict(free=["LAI", "Cab"], n_steps=10)
    for bad, what in ((dict(walkers=12), "walkers"), (dict(walkers=8, free=["LAI", "Cab", "Cw", "Cdm", "N"]), "walkers"),
                      (dict(n_steps=0), "n_steps"), (dict(n_steps=(1 << 20) + 1), "n_steps"), (dict(burn=10), "burn"),
                      (dict(thin=0), "thin"), (dict(burn=8, thin=3), "thin"), (dict(a=1.0), "a ="), (dict(temperature=0.0), "temperature"),
                      (dict(rel_init=np.inf), "rel_init"), (dict(step0=-1), "step0"), (dict(obs_offset=-1), "obs_offset"),
                      (dict(seed=-1), "seed"), (dict(init=np.zeros((3, 8, 3))), "init"), (dict(init_radius=np.zeros((2, 2))), "init_radius"),
                      (dict(free=["LAI", "LAI"]), "twice"), (dict(column="R"), "column"), (dict(band_model="x"), "band_model")):
        with pytest.raises(ValueError, match=what):
            spart_amd.sample(P, obs, S2, **dict(ok, **bad))
    opt = engine.sample_args(P, obs, ["LAI", "Cab", "Cw", "Cdm", "N"], None, None, None, None, None, None, 11, None, 1, 2.0, 1.0, 0.01,
                             None, None, 0, 0, 0, "R_TOC", "centre", "literal")[-1]
    assert opt["W"] == 16 and opt["burn"] == 5 and opt["n_keep"] == 6
