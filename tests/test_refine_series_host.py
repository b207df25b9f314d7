"""spart_refine_series without a GPU: the definition tools/refine_series_defined.py against tools/refine_tiles_defined.py and
tools/refine_defined.py where they must agree (no smoothing; one-row series); its proposed step and std against a dense solve
of the assembled matrix; the g++ build (-ffp-contract=off) of part 1 of csrc/spart_refine_series.h, driven series by series
(tests/hostmath/refine_series_host.cpp) on the definition's own intermediate sums, bit for bit; the same driver as a
stand-alone -fsanitize=address,undefined program; the consequences the GPU tests rely on; date_links; the refusals of
Engine.refine_series / spart_amd.refine_series that need no device; the structs, the header and the kernels' resources."""
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
import refine_series_defined as rsd  # noqa: E402
import refine_tiles_defined as rtd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "refine_series_host.cpp")
OUTS = ("shared", "shared_std", "local", "local_std", "cost", "cost0", "n_accept", "pixel_cost", "status", "y")
SERIES_KEYS = ("shared", "shared_std", "cost", "cost0", "n_accept")
ROW_KEYS = ("local", "local_std", "pixel_cost", "status", "y")
LENGTHS = [1, 2, 3, 8, 9, 39, 67]
NAMES = [15, 0, 2, 1, 5, 7, 3, 4, 6, 8, 9, 10, 11, 12, 13, 14]
EPS = 2.0 ** -52
c_dp, c_ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def dp(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(c_dp)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refine_series_host") / "librefine_series_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rsh_series_cost.restype = ctypes.c_double
    L.rsh_series_cost.argtypes = [ctypes.c_int, c_dp, ctypes.c_int, c_dp, c_dp, c_dp, ctypes.c_int, c_dp, c_dp, c_dp, c_ip]
    L.rsh_augment.argtypes = [ctypes.c_int] * 3 + [c_dp] * 4
    L.rsh_series_propose.argtypes = [ctypes.c_int, c_dp, c_dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_dp, c_dp, ctypes.c_int] + [c_dp] * 6
    L.rsh_series_std.argtypes = [ctypes.c_int, c_dp, c_dp, ctypes.c_int, ctypes.c_int, c_dp, c_dp, ctypes.c_int, c_dp, c_dp]
    L.rsh_bad_link.argtypes = [ctypes.c_double]
    return L


def toy_forward(nb, seed=0):
    Wm = np.random.default_rng(seed).normal(size=(27, nb))

    def forward(rows):
        with np.errstate(all="ignore"):
            return np.tanh(rows @ Wm * 0.05) + 0.1 * np.sin(rows[:, [0]] * np.arange(1, nb + 1) * 0.01)
    return forward


def toy_case(Fs, Fl, sizes, linkkind, priors, seed, masked=(), gamma=4.0, nb=7, noise=0.02, move=0.3):
    """random rows on a cheap nonlinear forward, every shared name constant over a series, the locals a random walk along it;
    per-row weights with zeros over NaN observations; ``masked``: rows with every weight zero; ``linkkind``: "none" (NULL),
    "varied", or "zero" (a zero in the middle of every series of 3 rows or more); the last link of a series is NaN"""
    rng = np.random.default_rng(seed)
    free = NAMES[:Fs + Fl]
    shared, local, F = free[:Fs], free[Fs:], Fs + Fl
    ts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    M, T = int(ts[-1]), len(sizes)
    series_of = np.repeat(np.arange(T), sizes)
    lo, hi = np.zeros(F), np.linspace(1.0, 2.0, F)
    base = rng.uniform(0.0, 1.0, (M, 27))
    truth = base.copy()
    walk = np.cumsum(rng.normal(size=(M, Fl)) * 0.05, axis=0)
    truth[:, local] = rd.clip_defined(0.5 * hi[Fs:] + walk - walk[ts[:-1]][series_of], lo[Fs:], hi[Fs:])
    truth[:, shared] = rng.uniform(lo[:Fs], hi[:Fs], (T, Fs))[series_of]
    forward = toy_forward(nb, seed)
    obs = forward(truth) * (1.0 + noise * rng.normal(size=(M, nb)))
    base[:, free] = rd.clip_defined(truth[:, free] + rng.uniform(-move, move, (M, F)) * (hi - lo), lo, hi)
    w = 10.0 ** rng.uniform(-1, 1, (M, nb))
    w[rng.random((M, nb)) < 0.15] = 0.0
    w[:, 1] = np.where(w[:, 1] == 0.0, 1.0, w[:, 1])
    for m in masked:
        w[m] = 0.0
    obs[w == 0.0] = np.nan
    link = None
    if linkkind != "none":
        link = 2.0 ** rng.uniform(-2, 2, M)
        if linkkind == "zero":
            for t in range(T):
                if sizes[t] >= 3:
                    link[(ts[t] + ts[t + 1]) // 2] = 0.0
        link[ts[1:] - 1] = np.nan
    smooth = np.full(Fl, gamma) * (1.0 + np.arange(Fl))
    if Fl >= 3:
        smooth[-1] = 0.0
    kw = {}
    if priors:
        zero = rng.random((M, Fl)) < 0.2
        kw["prior_mean"] = np.where(zero, np.nan, rng.uniform(lo[Fs:], hi[Fs:], (M, Fl)))
        kw["prior_weight"] = np.where(zero, 0.0, 4.0)
        if Fs:
            kw["shared_prior_mean"], kw["shared_prior_weight"] = rng.uniform(lo[:Fs], hi[:Fs], (T, Fs)), np.full((T, Fs), 2.0)
    return dict(base=base, shared=shared, local=local, lo=lo, hi=hi, series_start=ts, obs=obs, weights=w, smooth=smooth, link=link, **kw), forward


def as_tiles(case):
    return {("tile_start" if k == "series_start" else k): v for k, v in case.items() if k not in ("smooth", "link")}


# ---- the definition where it must be another definition
@pytest.mark.parametrize("priors", [False, True])
@pytest.mark.parametrize("Fs,Fl", [(0, 2), (1, 2), (3, 3)])
def test_without_smoothing_it_is_refine_tiles_defined(Fs, Fl, priors):
    case, forward = toy_case(Fs, Fl, [1, 2, 7, 8, 9, 39], "varied", priors, 10 * Fs + Fl, masked=() if not priors else (5,))
    ref = rtd.refine_tiles_defined(forward=forward, n_iter=5, **as_tiles(case))
    got = rsd.refine_series_defined(forward=forward, n_iter=5, **dict(case, smooth=np.zeros(Fl)))
    assert all(same(got[k], ref[k]) for k in OUTS), [k for k in OUTS if not same(got[k], ref[k])]
    got = rsd.refine_series_defined(forward=forward, n_iter=5, **dict(case, link=np.zeros(66)))
    assert all(same(got[k], ref[k]) for k in OUTS)
    assert (ref["n_accept"] >= 1).mean() >= 0.5 and (ref["n_accept"] < 5).any()
    tied = rsd.refine_series_defined(forward=forward, n_iter=5, **case)
    assert not same(tied["local"], ref["local"])


@pytest.mark.parametrize("priors", [False, True])
def test_one_row_series_are_refine_defined(priors):
    M, Fs, Fl = 24, 1, 2
    case, forward = toy_case(Fs, Fl, [1] * M, "varied", priors, 5)
    got = rsd.refine_series_defined(forward=forward, n_iter=5, **case)
    perm = [1, 2, 0]
    mean = weight = None
    if priors:
        mean = np.concatenate([case["prior_mean"], case["shared_prior_mean"]], axis=1)
        weight = np.concatenate([case["prior_weight"], case["shared_prior_weight"]], axis=1)
    ref = rd.refine_defined(case["base"], case["local"] + case["shared"], case["lo"][perm], case["hi"][perm], case["obs"], forward,
                            weights=case["weights"], n_iter=5, prior_mean=mean, prior_weight=weight)
    assert same(got["local"], ref["x"][:, :Fl]) and same(got["shared"], ref["x"][:, Fl:])
    assert same(got["local_std"], ref["std"][:, :Fl]) and same(got["shared_std"], ref["std"][:, Fl:])
    assert same(got["n_accept"], ref["n_accept"]) and same(got["y"], ref["y"]) and same(got["cost"], ref["cost"]) and same(got["cost0"], ref["cost0"])
    assert (ref["n_accept"] >= 1).mean() >= 0.5


# ---- the chain solve against a dense one
def dense_of(packed, S, kap, Fs, Fl):
    """the n x n matrix and right-hand side of one series in the unknown order, from the rows' packed sums (already augmented)"""
    G, F = packed.shape[0], Fs + Fl
    nt, nts, n = F * (F + 1) // 2, Fs * (Fs + 1) // 2, packed.shape[0] * Fl + Fs
    B, g = np.zeros((n, n)), np.zeros(n)
    for m in range(G):
        o = m * Fl
        for i in range(F):
            for j in range(min(i + 1, Fl)):
                r = o + i if i < Fl else G * Fl + i - Fl
                B[r, o + j] = B[o + j, r] = packed[m, rd.tri(i, j)]
        g[o:o + Fl] = packed[m, nt:nt + Fl]
        if m + 1 < G:
            for b in range(Fl):
                B[o + Fl + b, o + b] = B[o + b, o + Fl + b] = -kap[m, b]
    for a in range(Fs):
        for b in range(a + 1):
            B[G * Fl + a, G * Fl + b] = B[G * Fl + b, G * Fl + a] = S[rd.tri(a, b)]
    g[G * Fl:] = S[nts:]
    return B, g


@pytest.mark.parametrize("Fs,Fl,G", [(1, 2, 9), (2, 2, 39), (0, 3, 8), (3, 3, 20)])
def test_the_chain_solve_is_a_dense_solve(Fs, Fl, G):
    """delta of series_factor_defined / series_solve_defined against numpy's dense solve of the assembled damped matrix, and std
    against the dense inverse's diagonal, both within n^2 eps cond_2(B) relative to the largest entry -- the bound of a backward
    stable solve, derived and not tuned (the form tests/test_refine_posterior_host.py uses)"""
    case, forward = toy_case(Fs, Fl, [G], "zero", True, 100 + G)
    trace = []
    rsd.refine_series_defined(forward=forward, n_iter=2, trace=trace, **case)
    kap = rsd.kappa_defined(case["smooth"], case["link"], case["series_start"])[0]
    nt, nts = (Fs + Fl) * (Fs + Fl + 1) // 2, Fs * (Fs + 1) // 2
    worst = 0.0
    for rec in trace:
        if rec[0] not in ("propose", "std"):
            continue
        packed, S = rec[2], rec[3]
        A, Bs = packed[:, :nt].copy(), S[:nts].copy()
        lam = rec[4] if rec[0] == "propose" else 0.0
        for j in range(Fl):
            A[:, rd.tri(j, j)] += lam * np.where(A[:, rd.tri(j, j)] > 0, A[:, rd.tri(j, j)], 1.0)
        for a in range(Fs):
            Bs[rd.tri(a, a)] += lam * (Bs[rd.tri(a, a)] if Bs[rd.tri(a, a)] > 0 else 1.0)
        B, g = dense_of(np.concatenate([A, packed[:, nt:]], axis=1), np.concatenate([Bs, S[nts:]]), kap, Fs, Fl)
        n = B.shape[0]
        bound = n * n * EPS * np.linalg.cond(B)
        L, X, Ls, ok = rsd.series_factor_defined(A, kap, Bs, Fs, Fl)
        assert ok
        if rec[0] == "propose":
            ds, dl = rsd.series_solve_defined(L, X, Ls, packed[:, nt:nt + Fl], S[nts:], Fs, Fl)
            got, want = np.concatenate([np.ravel(dl), ds]), np.linalg.solve(B, -g)
        else:
            ss, ls = rsd.series_std_defined(L, X, Ls, Fs, Fl)
            got, want = np.concatenate([np.ravel(ls), ss]), np.sqrt(np.diag(np.linalg.inv(B)))
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= bound, (rec[0], err, bound)
        worst = max(worst, err / bound)
    assert 0.0 < worst <= 1.0


# ---- part 1 of the header on the definition's own sums, series by series
SHAPES = [(0, 1), (1, 2), (2, 2), (0, 16), (15, 1)]


@pytest.mark.parametrize("priors", [False, True])
@pytest.mark.parametrize("linkkind", ["none", "varied", "zero"])
@pytest.mark.parametrize("Fs,Fl", SHAPES)
def test_the_gxx_build_is_the_definition(lib, Fs, Fl, linkkind, priors):
    """every cost sum, augmentation, proposal (taken or refused) and std of the definition's run over series of 1, 2, 3, 8, 9, 39
    and 67 rows, masked dates at a series' start, interior and end, fed to the g++ build at strides 1 and 5"""
    masked = (3, 10, 13, 22, 40, 61, 128)       # the start of the series of 8, its interior and its end 13; interior and end elsewhere
    sizes = LENGTHS if Fl < 16 else [1, 2, 3, 8, 9, 39]
    case, forward = toy_case(Fs, Fl, sizes, linkkind, priors, 7 * Fs + Fl, masked=[m for m in masked if m < sum(sizes)])
    F, ts = Fs + Fl, case["series_start"]
    trace = []
    ref = rsd.refine_series_defined(forward=forward, n_iter=3, trace=trace, **case)
    assert (ref["n_accept"] >= 1).mean() >= 0.5
    gam, lo, hi = case["smooth"], case["lo"], case["hi"]
    seen = {"cost": 0, "augment": 0, "propose": 0, "std": 0}
    for rec in trace:
        t = rec[1]
        G = int(ts[t + 1] - ts[t])
        lk = None if case["link"] is None else case["link"][ts[t]:ts[t + 1]]
        seen[rec[0]] += 1
        if rec[0] == "cost":
            _, _, ct, lt, zt, C = rec
            sm = case.get("shared_prior_mean")
            bad = ctypes.c_int32(0)
            got = lib.rsh_series_cost(G, dp(ct), Fl, dp(gam), dp(lk), dp(lt), Fs, dp(zt), dp(None if sm is None else sm[t]),
                                      dp(None if sm is None else case["shared_prior_weight"][t]), ctypes.byref(bad))
            assert same(got, C) and bad.value == 0
        elif rec[0] == "augment":
            Ap = np.ascontiguousarray(rec[2].copy())
            lib.rsh_augment(G, F, Fs, dp(gam), dp(lk), dp(rec[3]), Ap.ctypes.data_as(c_dp))
            assert same(Ap, rec[4])
        elif rec[0] == "propose":
            _, _, packed, S, lam, z, l, zt, lt, ok = rec
            for SW in (1, 5):
                gz, gl = np.zeros(max(Fs, 1)), np.zeros((G, Fl))
                took = lib.rsh_series_propose(G, dp(packed), dp(S if S.size else np.zeros(1)), F, Fs, lam, dp(gam), dp(lk), SW,
                                              dp(z if Fs else np.zeros(1)), dp(l), dp(lo), dp(hi), gz.ctypes.data_as(c_dp), gl.ctypes.data_as(c_dp))
                assert bool(took) == bool(ok) and same(gz[:Fs], zt) and same(gl, lt), (t, SW)
        else:
            _, _, packed, S, ss, ls = rec
            for SW in (1, 5):
                gs, gl = np.zeros(max(Fs, 1)), np.zeros((G, Fl))
                lib.rsh_series_std(G, dp(packed), dp(S if S.size else np.zeros(1)), F, Fs, dp(gam), dp(lk), SW, gs.ctypes.data_as(c_dp),
                                   gl.ctypes.data_as(c_dp))
                assert same(gs[:Fs], ss) and same(gl, ls), (t, SW)
    assert min(seen.values()) >= len(sizes)
    assert [lib.rsh_bad_link(v) for v in (0.0, 1.0, -0.0, -1.0, np.nan, np.inf)] == [0, 0, 0, 1, 1, 1] and lib.rsh_max_rows() == 256 == rsd.MAX_SERIES


def test_the_functions_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """the .cpp's own main (every shape, length, link kind and two strides, heap buffers of exact size, a singular twin) as a
    stand-alone -fsanitize=address,undefined program in a child process; the sanitizer runtimes are linked into the program
    itself, so nothing is preloaded and nothing sanitised is loaded into python"""
    exe = str(tmp_path / "refine_series_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-DREFINE_SERIES_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "WRONG" not in r.stdout and r.stdout.count(" ok") == 5 * 7 * 3 * 2 and "Sanitizer" not in r.stderr


# ---- the consequences
@pytest.fixture(scope="module")
def plain():
    case, forward = toy_case(1, 2, [1, 2, 7, 8, 9, 39], "varied", False, 3, masked=(12,))
    hist = []
    return case, forward, rsd.refine_series_defined(forward=forward, n_iter=5, history=hist, **case), hist


def test_a_series_does_not_depend_on_the_others(plain):
    case, forward, ref, _ = plain
    cut = slice(27, 66)
    alone = dict(case, base=case["base"][cut], obs=case["obs"][cut], weights=case["weights"][cut], link=case["link"][cut],
                 series_start=np.array([0, 39]))
    one = rsd.refine_series_defined(forward=forward, n_iter=5, **alone)
    assert all(same(one[k][0], ref[k][5]) for k in SERIES_KEYS) and all(same(one[k], ref[k][cut]) for k in ROW_KEYS)


def test_cost_falls_and_the_prefix_holds(plain):
    case, forward, ref, hist = plain
    assert (ref["cost"] <= ref["cost0"]).all() and (ref["n_accept"] >= 1).all() and (ref["n_accept"] < 5).any()
    for k in (0, 2, 3):
        got = rsd.refine_series_defined(forward=forward, n_iter=k, **case)
        assert same(got["shared"], hist[k][0]) and same(got["local"], hist[k][1]) and same(got["cost"], hist[k][2])
    costs = np.array([h[2] for h in hist])
    assert (np.diff(costs, axis=0) <= 0).all()


@pytest.mark.parametrize("what", ["link nan", "link negative", "link inf", "weight", "fixed nan", "shared prior"])
def test_a_series_dies_as_a_whole(plain, what):
    case, forward, ref, _ = plain
    bad = dict(case, link=case["link"].copy(), weights=case["weights"].copy(), base=case["base"].copy())
    t, row = 4, 20                                # the series of 9 rows, 18 ... 26
    if what.startswith("link"):
        bad["link"][row] = {"nan": np.nan, "negative": -0.5, "inf": np.inf}[what.split()[1]]
    elif what == "weight":
        bad["weights"][row, 3] = -1.0
    elif what == "fixed nan":
        bad["base"][row, 20] = np.nan
    else:
        bad["shared_prior_mean"], bad["shared_prior_weight"] = np.full((6, 1), np.nan), np.zeros((6, 1))
        bad["shared_prior_mean"][t], bad["shared_prior_weight"][t] = 0.3, -1.0
    got = rsd.refine_series_defined(forward=forward, n_iter=5, **bad)
    rows = np.arange(18, 27)
    assert got["n_accept"][t] == -1 and np.isnan(got["local_std"][rows]).all() and np.isnan(got["shared_std"][t]).all()
    assert same(got["cost"][t], got["cost0"][t])
    if what == "shared prior":
        assert (got["status"][rows] == 1).all()
    else:
        assert got["status"][row] == -1 and (got["status"][rows[rows != row]] == 1).all()
    assert same(got["local"][rows], rd.clip_defined(case["base"][rows][:, case["local"]], case["lo"][1:], case["hi"][1:]))
    assert np.isfinite(got["y"][rows[rows != row]]).all()
    others, keep = [s for s in range(6) if s != t], np.r_[0:18, 27:66]
    assert all(same(got[k][others], ref[k][others]) for k in SERIES_KEYS) and all(same(got[k][keep], ref[k][keep]) for k in ROW_KEYS)
    # the last link of a series is never read
    assert np.isnan(case["link"][case["series_start"][1:] - 1]).all()


def test_a_masked_date_stays_without_a_tie_and_moves_with_one(plain):
    case, forward, ref, _ = plain
    start = rd.clip_defined(case["base"][12, case["local"]], case["lo"][1:], case["hi"][1:])
    assert (case["weights"][12] == 0.0).all() and np.isnan(case["obs"][12]).all() and ref["status"][12] == 0 and ref["pixel_cost"][12] == 0.0
    flat = rsd.refine_series_defined(forward=forward, n_iter=5, **dict(case, smooth=np.zeros(2)))
    assert same(flat["local"][12], start) and np.isnan(flat["local_std"][10:18]).all() and np.isnan(flat["shared_std"][3]).all()
    assert np.isfinite(flat["local_std"][18:27]).all()
    assert (ref["local"][12] != start).all() and np.isfinite(ref["local_std"][10:18]).all() and np.isfinite(ref["shared_std"][3]).all()
    half = rsd.refine_series_defined(forward=forward, n_iter=5, **dict(case, smooth=np.array([4.0, 0.0])))
    assert half["local"][12, 0] != start[0] and half["local"][12, 1] == start[1]
    # a tie on one side is enough
    one = case["link"].copy()
    one[12] = 0.0
    got = rsd.refine_series_defined(forward=forward, n_iter=5, **dict(case, link=one))
    assert (got["local"][12] != start).all() and np.isfinite(got["local_std"][10:18]).all()


# ---- the host helpers and the refusals that need no device
def test_date_links():
    import spart_amd
    days = np.array([1.0, 3.0, 7.0, 2.0, 2.5, 10.0])
    assert spart_amd.date_links(days, [0, 3, 6]).tolist() == [0.5, 0.25, 0.0, 2.0, 1.0 / 7.5, 0.0]
    assert spart_amd.date_links(days, [0, 3, 6], power=2).tolist() == [0.25, 0.0625, 0.0, 4.0, 1.0 / 7.5 ** 2, 0.0]
    assert spart_amd.date_links(days[:1], [0, 1]).tolist() == [0.0] and spart_amd.date_links(np.zeros(0), [0]).size == 0
    for bad_days, ts in ((days, [0, 6]), (np.array([1.0, 1.0]), [0, 2]), (np.array([1.0, np.nan]), [0, 2]), (days, [0, 3]), (days, [1, 6]),
                         (days.reshape(2, 3), [0, 6])):
        with pytest.raises(ValueError):
            spart_amd.date_links(bad_days, ts)


def test_refine_series_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    M = 6
    P = workloads.lhs_params(M, "full", seed=1).T
    obs = np.zeros((M, 13))
    ok = dict(shared=["LIDFa"], local=["LAI", "Cab"], n_dates=3)
    for kw, text in ((dict(ok, local=[]), "nothing to link"), (dict(ok, local=["nope"]), "unknown"), (dict(ok, local=["LIDFa"]), "twice"),
                     (dict(ok, obs=np.zeros((M, 2, 13))), "obs"), (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"),
                     (dict(ok, n_iter=101), "n_iter"), (dict(ok, column="rso"), "column"), (dict(ok, band_model="wide"), "band_model"),
                     (dict(ok, n_dates=None), "exactly one"), (dict(ok, series_start=[0, 6]), "exactly one"),
                     (dict(ok, n_dates=0), "n_dates"), (dict(ok, n_dates=257), "n_dates"), (dict(ok, n_dates=2.5), "n_dates"),
                     (dict(ok, n_dates=4), "does not divide"),
                     (dict(ok, n_dates=None, series_start=[0, 3, 5]), "expected 0 ... M"),
                     (dict(ok, n_dates=None, series_start=[0, 3, 3, 6]), "series 1 has 0 rows"),
                     (dict(ok, n_dates=None, series_start=[0.0, 6.0]), "integer"),
                     (dict(ok, smooth=[1.0, 1.0]), "dict"), (dict(ok, smooth={"LIDFa": 1.0}), "not local"), (dict(ok, smooth={"Cw": 1.0}), "not local"),
                     (dict(ok, smooth={"LAI": 0.0}), "sigma"), (dict(ok, smooth={"LAI": -1.0}), "sigma"), (dict(ok, smooth={"LAI": np.nan}), "sigma"),
                     (dict(ok, smooth={"LAI": np.inf}), "sigma"), (dict(ok, smooth={"LAI": 1e-200}), "sigma"), (dict(ok, smooth={"LAI": "x"}), "sigma"),
                     (dict(ok, link=np.ones(M + 1)), "link"), (dict(ok, link=np.ones((M, 1))), "link"),
                     (dict(ok, prior={"Cw": (0.0, 1.0)}), "not free"), (dict(ok, prior={"LIDFa": (np.zeros(M), 1.0)}), "2 series"),
                     (dict(ok, prior={"LAI": (np.zeros(2), 1.0)}), "6 rows")):
        kw = dict(kw)
        o = kw.pop("obs", obs)
        with pytest.raises(ValueError, match=text):
            spart_amd.refine_series(P, o, "Sentinel2A-MSI", **kw)
    with pytest.raises(ValueError, match="256"):
        spart_amd.refine_series(np.zeros((27, 300)), np.zeros((300, 13)), "Sentinel2A-MSI", [], ["LAI"], series_start=[0, 300])
    e = engine.Engine.__new__(engine.Engine)                   # an Engine object that never saw a device
    e.nb = 13
    with pytest.raises(ValueError, match="unknown"):
        e.refine_series(P, obs, ["LIDFa"], ["nope"], n_dates=2)
    with pytest.raises(ValueError, match="obs"):
        e.refine_series(P, np.zeros((M, 12)), [], ["LAI"], n_dates=2)
    with pytest.raises(ValueError, match="nothing to link"):
        e.refine_series(P, obs, ["LIDFa"], n_dates=2)
    out = engine.refine_series_args(P, obs, ["LIDFa"], ["LAI", "Cab"], 3, None, {"Cab": 2.0}, np.ones(M), None, np.ones((M, 13)), "R_TOA", 3,
                                    1e-3, 1e-2, "literal", {"LIDFa": (np.array([0.1, 0.2]), 0.5), "Cab": (40.0, 2.0)}, "centre")
    plan, _, m, Fs, wper, ts, lprior, sprior, gamma = out
    assert (m, Fs, wper, ts.tolist(), gamma.tolist()) == (M, 1, 1, [0, 3, 6], [0.0, 0.25]) and plan["names"] == ["LIDFa", "LAI", "Cab"]
    assert lprior[1].tolist() == [0.0, 0.25] and sprior[2] == 1 and sprior[0].tolist() == [[0.1], [0.2]]
    assert engine.series_starts(0, 5, None).tolist() == [0] and engine.series_starts(10, 5, None).tolist() == [0, 5, 10]
    # the tiles' own partition and messages are what they were
    assert engine.tile_starts(11, 5, None).tolist() == [0, 5, 10, 11]


def test_signatures_structs_and_header_agree():
    from spart_amd import _lib
    assert [f[0] for f in _lib.SpartRefineSeriesOpt._fields_] == ["tiles", "smooth", "link"]
    assert _lib.SpartRefineSeriesOpt._fields_[0][1] is _lib.SpartRefineTilesOpt
    assert ctypes.sizeof(_lib.SpartRefineSeriesOpt) == ctypes.sizeof(_lib.SpartRefineTilesOpt) + 16
    res, args = _lib.SIGNATURES["spart_refine_series"]
    ref = list(_lib.SIGNATURES["spart_refine_tiles"][1])
    assert res is ctypes.c_int and len(args) == 16 and args[:11] == ref[:11] and args[12:] == ref[12:]
    assert args[11]._type_ is _lib.SpartRefineSeriesOpt
    res, args = _lib.SIGNATURES["spart_series_workspace_bytes"]
    assert res is ctypes.c_size_t and len(args) == 4
    full = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    body = re.search(r"typedef struct spart_refine_series_opt \{(.*?)\} spart_refine_series_opt;", header, flags=re.S).group(1)
    assert re.findall(r"\b([A-Za-z_0-9]+)\s*[;,]", body) == ["tiles", "smooth", "link"]
    assert re.search(r"int spart_refine_series\(spart_ctx \*ctx, int64_t M, .*?int64_t S, const int64_t \*series_start", header, flags=re.S)
    assert "#define SPART_ABI_VERSION 14" in full and "spart_refine_series and spart_series_workspace_bytes" in full
    assert _lib.SERIES_MAXT == 256 == rsd.MAX_SERIES and _lib.ABI_VERSION == 14
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine_series.h")).read()
    assert "constexpr int SERIES_MAXT = 256;" in src
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    assert any(d.endswith("spart_refine_series.h") for d in build.DEPS)


def test_null_context_is_refused_without_a_gpu():
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    L = ctypes.CDLL(build.build(verbose=False))
    f = L.spart_series_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    assert f(None, 100, 3, 1) == 0
    L.spart_refine_series.restype = ctypes.c_int
    L.spart_last_error.restype = ctypes.c_char_p
    assert L.spart_refine_series(*([None] * 16)) == -1 and b"spart_refine_series: null context" in L.spart_last_error(None)


def test_series_kernels_use_no_scratch_and_little_lds(kernel_meta):
    names = ("k_series_decide", "k_series_augment", "k_series_sums", "k_series_factor", "k_series_shared", "k_series_back", "k_series_std")
    hits = {k: v for k, v in kernel_meta.items() if "k_series_" in k}
    assert len(hits) == len(names) + 2 and all(any(n in k for k in hits) for n in names), sorted(hits)      # (factor and back: W = 4 and 8)
    for name, k in hits.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)                  # (all LDS is dynamic)
    # the dynamic LDS of the three staged kernels, by the header's own formulas, stays inside the family's 40 KiB at every shape
    tri = lambda n: n * (n + 1) // 2      # noqa: E731
    worst = 0
    for F in range(1, 17):
        W = 8 if F <= 8 else 4
        for Fs in range(F):
            Fl, P, Ps = F - Fs, tri(F) + F, tri(Fs) + Fs
            worst = max(worst, (2 * P + Fl * Fl + Ps) * (W + 1) * 8 + W * 8 + 3 * W * 4 + (Fl + W) * 8, (P + Fl * Fl + Fl + Fs) * (W + 1) * 8 + 3 * W * 4,
                        (2 * Fl + Fs) * 64 * 8)
    assert worst <= 40960, worst
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine_series.h")).read()
    assert "return (size_t)(2 * P + Fl * Fl + Ps) * (W + 1) * 8 + W * 8 + 3 * W * 4 + (size_t)(Fl + W) * 8;" in src and "return F <= 8 ? 8 : 4;" in src
    assert "return (size_t)(P + Fl * Fl + Fl + Fs) * (W + 1) * 8 + 3 * W * 4;" in src
    assert "return (size_t)(2 * (F - Fs) + Fs) * SERIES_STD_THREADS * 8;" in src and "constexpr int SERIES_STD_THREADS = 64;" in src
