"""spart_refine_posterior without a GPU: the g++ build (-ffp-contract=off) of part 1 of csrc/spart_refine_posterior.h
(tests/hostmath/refine_posterior_host.cpp) against the definition tools/refine_posterior_defined.py, bit for bit; the
definition's own properties with the CPU oracle as forward model (the 48-row twin case of test_refine_host); the same functions
as a stand-alone -fsanitize=address,undefined program; header, binding and loader; and the argument refusals of
Engine.posterior, spart_amd.posterior / jacobian, retrieve and retrieve_stream that need no device."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402
import refine_posterior_defined as rpd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "refine_posterior_host.cpp")
FS = (1, 2, 6, 16)
D = ctypes.POINTER(ctypes.c_double)
EPS = np.finfo(np.float64).eps
S2 = "Sentinel2A-MSI"


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def dp(a):
    return a.ctypes.data_as(D)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("refine_posterior_host") / "librefine_posterior_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rq_posterior.restype = ctypes.c_int
    L.rq_posterior.argtypes = [ctypes.c_int, ctypes.c_int, D, D, D, ctypes.c_int] + [D] * 5
    L.rh_std.argtypes = [ctypes.c_int, D, D]
    return L


def host_posterior(lib, J, w, p, S):
    """rq_posterior row by row -> (status, K, cov, ak, std, dfs)"""
    M, nb, F = J.shape
    st = np.zeros(M, dtype=np.int32)
    K, cov, ak = np.zeros((M, F, F)), np.zeros((M, F, F)), np.zeros((M, F, F))
    sd, dfs = np.zeros((M, F)), np.zeros(M)
    for m in range(M):
        one = np.zeros(1)
        st[m] = lib.rq_posterior(F, nb, dp(np.ascontiguousarray(J[m])), dp(np.ascontiguousarray(w[m])),
                                 None if p is None else dp(np.ascontiguousarray(p[m])), S, dp(K[m]), dp(cov[m]), dp(ak[m]), dp(sd[m]),
                                 dp(one))
        dfs[m] = one[0]
    return st, K, cov, ak, sd, dfs


@pytest.mark.parametrize("prior", (False, True))
@pytest.mark.parametrize("F", FS)
def test_part_one_bit_for_bit(lib, F, prior):
    """random Jacobians with columns of very different size; rows: 3 a zero column of J (singular without a prior), 4 a NaN in
    J under a weight (A is NaN: status 1), 5 a NaN in J under a zero weight (alive), 6 all band weights zero (K = 0)"""
    rng = np.random.default_rng(10 * F + prior)
    M, nb, nt = 24, 21, F * (F + 1) // 2
    J = rng.normal(0.0, 1.0, (M, nb, F)) * 10.0 ** rng.uniform(-2, 2, F)
    w = 10.0 ** rng.uniform(-2, 2, (M, nb))
    w[rng.random((M, nb)) < 0.2] = 0.0
    w[:, :F + 2] = np.where(w[:, :F + 2] == 0.0, 1.0, w[:, :F + 2])          # (enough bands for F unknowns)
    J[3, :, F - 1] = 0.0
    J[4, 2, 0], w[4, 2] = np.nan, 1.0
    J[5, nb - 1, :], w[5, nb - 1] = np.nan, 0.0
    w[6] = 0.0
    p = None
    if prior:
        p = 10.0 ** rng.uniform(-2, 2, (M, F))
        p[7, F // 2] = 0.0
        p[8] = 0.0
    Kp = rd.normal_defined(J, np.zeros((M, nb)), w)[:, :nt]
    A, ok, cov, ak, sd, dfs = rpd.posterior_of_normal(Kp, p, F)
    assert not ok[4] and ok[5] and ok[3] == prior and ok[6] == prior and ok[[0, 1, 2]].all() and ok.sum() >= M - 3
    for S in (1, 5):
        st, K, gcov, gak, gsd, gdfs = host_posterior(lib, J, w, p, S)
        assert np.array_equal(st, np.where(ok, 0, 1))
        assert same(K, rpd.full_defined(Kp, F))
        assert same(gcov, cov) and same(gak, ak) and same(gsd, sd) and same(gdfs, dfs)
    assert np.isnan(cov[~ok]).all() and np.isnan(dfs[~ok]).all() and np.isfinite(cov[ok]).all()
    assert same(cov, np.swapaxes(cov, 1, 2))                                  # exactly symmetric
    # std is refine_std's number: the definition's and the compiled one's, on the same packed A
    packed = np.concatenate([A, np.zeros((M, F))], axis=1)
    assert same(sd, rd.std_defined(packed, F))
    for m in range(M):
        s = np.zeros(F)
        lib.rh_std(F, dp(np.ascontiguousarray(packed[m])), dp(s))
        assert same(s, sd[m]), m
    if prior:                                                                 # K = 0: ak and dfs exactly 0, cov = diag(1 / p)
        assert (ak[6] == 0).all() and dfs[6] == 0 and not np.signbit(dfs[6])
        assert (np.abs(np.diagonal(cov[6]) * p[6] - 1.0) <= 4 * EPS).all()
        assert (cov[6][~np.eye(F, dtype=bool)] == 0).all()
    else:
        # no prior: ak = A^-1 A.  F^2 eps kappa is the bound of a backward-stable inverse; the 4 eps on top are the roundings
        # that remain at kappa = 1 (F = 1: sqrt, two divisions, two products, each <= eps / 2, and one to spare)
        cond = np.array([np.linalg.cond(rpd.full_defined(A[m:m + 1], F)[0]) for m in np.flatnonzero(ok)])
        err = np.abs(ak[ok] - np.eye(F)).max(axis=(1, 2))
        assert (err <= (F * F + 4) * EPS * cond).all(), float((err / cond).max())


def test_the_functions_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """the .cpp's own main (every F, three strides, with / without a prior, a singular case; heap buffers of exact size) as a
    stand-alone -fsanitize=address,undefined program in a child process; the sanitizer runtimes are linked into the program
    itself, so nothing is preloaded and nothing sanitised is loaded into python"""
    exe = str(tmp_path / "refine_posterior_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-DREFINE_POSTERIOR_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "WRONG" not in r.stdout and r.stdout.count(" ok") == 36 and "Sanitizer" not in r.stderr


# ---- the definition with the oracle as forward model
@pytest.fixture(scope="module")
def twin(oracle, tables):
    """test_twin_experiment_with_the_oracle's case: Sentinel-2A, 48 LHS rows, free = LAI, Cab, Cw, Cdm over their RANGES"""
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
                cache[key] = np.asarray(oracle.spart_run(rows, S2, tables, pso="gl")["R_TOC"], dtype=np.float64)
        return cache[key]
    obs = forward(truth)
    w = 1.0 / (0.02 * np.maximum(obs, 0.01)) ** 2
    return {"free": free, "lo": lo, "hi": hi, "truth": truth, "forward": forward, "obs": obs, "w": w}


def prior_of(twin, frac):
    """sigma = frac of the range around the truth -> (mean, weight), per observation"""
    sigma = frac * (twin["hi"] - twin["lo"])
    return twin["truth"][:, twin["free"]].copy(), np.tile(1.0 / (sigma * sigma), (48, 1))


def test_the_definition_at_the_truth_of_the_twin_experiment(twin):
    F, M = 4, 48
    args = (twin["truth"], twin["free"], twin["lo"], twin["hi"], twin["obs"], twin["forward"])
    res = rpd.posterior_defined(*args, weights=twin["w"])
    assert (res["status"] == 0).all() and (res["nband"] == 13).all() and np.isfinite(res["jac"]).all()
    assert same(res["cov"], np.swapaxes(res["cov"], 1, 2))
    # cov is the inverse of A, to the bound of a backward-stable solve of the diagonally scaled system
    Kp = rd.normal_defined(res["jac"], np.zeros((M, 13)), twin["w"])[:, :F * (F + 1) // 2]
    A = rpd.full_defined(Kp, F)
    worst = 0.0
    for m in range(M):
        d = np.sqrt(np.diagonal(A[m]))
        As, Cs = A[m] / np.outer(d, d), res["cov"][m] * np.outer(d, d)
        err, bound = np.abs(Cs @ As - np.eye(F)).max(), F * F * EPS * np.linalg.cond(As)
        worst = max(worst, err / bound)
        assert err <= bound, (m, err, bound)
    print("worst |cov A - I| / (F^2 eps kappa):", worst)
    assert same(res["std"], np.sqrt(np.diagonal(res["cov"], axis1=1, axis2=2)))
    assert same(res["std"], rd.std_defined(np.concatenate([Kp, np.zeros((M, F))], axis=1), F))
    # without a prior the measurement decides everything
    assert (np.abs(res["ak"] - np.eye(F)) <= 1e-9).all() and (np.abs(res["dfs"] - F) <= 1e-9).all()
    assert (res["cost"] == 0).all()                                              # obs is the model at the truth
    # a prior takes degrees of freedom away, a tighter one more
    dfs = {}
    for frac in (0.3, 0.03):
        mu, p = prior_of(twin, frac)
        r = rpd.posterior_defined(*args, weights=twin["w"], prior_mean=mu, prior_weight=p)
        assert (r["status"] == 0).all() and ((0 < r["dfs"]) & (r["dfs"] < F)).all()
        assert same(r["jac"], res["jac"]) and same(r["y"], res["y"])
        dfs[frac] = r["dfs"]
        print("prior sigma", frac, "of the range: dfs", float(r["dfs"].min()), "...", float(r["dfs"].max()), "median",
              float(np.median(r["dfs"])))
    assert (dfs[0.03] <= dfs[0.3] + 1e-9).all()
    # no band counts: the prior alone
    mu, p = prior_of(twin, 0.3)
    z = rpd.posterior_defined(*args, weights=np.zeros(13), prior_mean=mu, prior_weight=p)
    assert (z["status"] == 0).all() and (z["nband"] == 0).all() and (z["ak"] == 0).all() and (z["dfs"] == 0).all()
    assert (np.abs(np.diagonal(z["cov"], axis1=1, axis2=2) * p - 1.0) <= 4 * EPS).all()
    # obs = None: the cost is the prior's term alone, everything else unchanged
    mu2 = mu + 0.1 * (twin["hi"] - twin["lo"])
    a = rpd.posterior_defined(*args, weights=twin["w"], prior_mean=mu2, prior_weight=p)
    b = rpd.posterior_defined(*args[:4], None, twin["forward"], weights=twin["w"], prior_mean=mu2, prior_weight=p)
    want, _ = rd.prior_cost_defined(np.zeros(M), rd.clip_defined(twin["truth"][:, twin["free"]], twin["lo"], twin["hi"]), mu2, p)
    assert same(b["cost"], want) and (b["cost"] > 0).all()
    assert all(same(a[k], b[k]) for k in rpd.OUTS if k != "cost")


@pytest.mark.parametrize("prior", (False, True))
def test_on_the_rows_a_fit_returned_std_y_and_cost_are_the_fits(twin, prior):
    start = twin["truth"].copy()
    centre = 0.5 * (twin["lo"] + twin["hi"])
    f = twin["free"]
    start[:, f] = twin["truth"][:, f] + 0.15 * (twin["hi"] - twin["lo"]) * np.sign(centre - twin["truth"][:, f])
    kw = dict(weights=twin["w"])
    if prior:
        kw["prior_mean"], kw["prior_weight"] = prior_of(twin, 0.3)
    fit = rd.refine_defined(start, f, twin["lo"], twin["hi"], twin["obs"], twin["forward"], n_iter=3, **kw)
    assert (fit["n_accept"] >= 0).all() and (fit["n_accept"] >= 1).sum() >= 40
    rows = start.copy()
    rows[:, f] = fit["x"]
    res = rpd.posterior_defined(rows, f, twin["lo"], twin["hi"], twin["obs"], twin["forward"], **kw)
    assert (res["status"] == 0).all()
    assert same(res["x"], fit["x"]) and same(res["std"], fit["std"]) and same(res["y"], fit["y"]) and same(res["cost"], fit["cost"])


def test_dead_and_indefinite_rows_of_the_definition():
    """a toy forward model: 1 a NaN observation (dead), 2 a negative band weight (dead), 3 a negative prior weight (dead), 4 a
    NaN fixed parameter (dead), 5 a NaN observation under a zero weight (alive), 6 a free column the model ignores (status 1
    without a prior on it)"""
    rng = np.random.default_rng(3)
    M, nb, F = 8, 13, 3
    free = [15, 0, 26]
    Wm = rng.normal(size=(27, nb))
    Wm[26] = 0.0                                                                 # column 26 does not enter the model

    def forward(rows):
        return np.tanh(rows @ Wm * 0.05)
    base = rng.uniform(0.0, 1.0, (M, 27))
    lo, hi = np.zeros(F), np.ones(F)
    obs = forward(base) + 0.01
    w = 10.0 ** rng.uniform(-1, 1, (M, nb))
    p = np.tile([0.0, 0.0, 4.0], (M, 1))
    mu = np.full((M, F), 0.5)
    obs[1, 4] = np.nan
    w[2, 0] = -1.0
    p[3, 1] = -2.0
    base[4, 20] = np.nan
    obs[5, 7], w[5, 7] = np.nan, 0.0
    p[6, 2] = 0.0
    r = rpd.posterior_defined(base, free, lo, hi, obs, forward, weights=w, prior_mean=mu, prior_weight=p)
    assert list(r["status"]) == [0, -1, -1, -1, -1, 0, 1, 0]
    dead = r["status"] == -1
    assert np.isnan(r["jac"][dead]).all() and np.isnan(r["cov"][dead]).all() and np.isnan(r["dfs"][dead]).all()
    assert np.isfinite(r["y"][[1, 2, 3]]).all() and np.isfinite(r["cost"][[2, 3]]).all() and np.isnan(r["cost"][[1, 4]]).all()
    assert np.isfinite(r["jac"][6]).all() and (r["jac"][6][:, 2] == 0).all() and np.isnan(r["cov"][6]).all() and np.isnan(r["std"][6]).all()
    assert list(r["nband"]) == [13, 13, 13, 13, 13, 12, 13, 13] and np.isfinite(r["jac"][5]).all()
    assert np.isfinite(r["cov"][[0, 5, 7]]).all() and ((0 < r["dfs"][[0, 5, 7]]) & (r["dfs"][[0, 5, 7]] < F)).all()


# ---- header, binding and loader
def test_struct_signature_and_header_agree():
    from spart_amd import _lib
    fields = ["x", "y", "jac", "cov", "ak", "std", "dfs", "cost", "nband", "status"]
    assert [n for n, _ in _lib.SpartPosteriorOut._fields_] == fields == list(_lib.POSTERIOR_OUTS) == list(rpd.OUTS)
    assert ctypes.sizeof(_lib.SpartPosteriorOut) == 80
    header = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct spart_posterior_out \{(.*?)\} spart_posterior_out;", code, flags=re.S).group(1)
    assert re.findall(r"\b([A-Za-z_0-9]+)\s*;", body) == fields
    res, args = _lib.SIGNATURES["spart_refine_posterior"]
    ref = list(_lib.SIGNATURES["spart_refine"][1])
    assert res is ctypes.c_int and len(args) == 15 and list(args[:10]) == ref[:10] and list(args[12:]) == ref[16:]
    assert args[10] is ctypes.c_int and args[11]._type_ is _lib.SpartPosteriorOut
    decl = re.search(r"\bint\s+spart_refine_posterior\s*\(([^;]*)\)\s*;", code).group(1)
    assert len(decl.split(",")) == 15 and "int band_model" in decl and "const spart_posterior_out *out" in decl
    assert _lib.ABI_VERSION == 14 and "#define SPART_ABI_VERSION 14" in header and "spart_posterior_out likewise" in header


def test_a_library_without_the_symbol_is_refused_by_name(tmp_path):
    """a foreign library of interface version 14 that lacks spart_refine_posterior: load() names the symbol"""
    from spart_amd import _lib
    src = tmp_path / "old.c"
    src.write_text("int spart_abi_version(void) { return 14; }\nconst char *spart_build_id(void) { return \"x\"; }\n"
                   + "".join(f"int {n}(void) {{ return 0; }}\n" for n in _lib.SIGNATURES
                             if n not in ("spart_abi_version", "spart_build_id", "spart_refine_posterior")))
    so = str(tmp_path / "libold.so")
    subprocess.check_call(["g++", "-x", "c", "-shared", "-fPIC", "-o", so, str(src)])
    with pytest.raises(RuntimeError, match="spart_refine_posterior"):
        _lib.load(so)
    assert os.path.abspath(so) not in _lib._libs


def test_the_built_library_exports_the_symbol():
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    assert hasattr(ctypes.CDLL(build.build(verbose=False)), "spart_refine_posterior")


# ---- refusals that need no device
def test_posterior_arguments_are_checked_before_the_gpu_is_asked_for(monkeypatch):
    import spart_amd
    from spart_amd import engine, lut, workloads

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(lut, "get_engine", no_engine)
    monkeypatch.setattr(engine, "get_engine", no_engine)
    P = workloads.lhs_params(4, "full", seed=1)
    obs = np.zeros((4, 13))
    ok = dict(free=["LAI", "Cab"])
    for kw, text in ((dict(free=[]), "free"), (dict(free=["LAI", "nope"]), "unknown"), (dict(free=["LAI", "LAI"]), "twice"),
                     (dict(free=[workloads.PARAM_NAMES[i] for i in range(17)]), "free"), (dict(free=["SMC"]), "no range"),
                     (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"), (dict(ok, bounds={"Cw": (0.0, 1.0)}), "not free"),
                     (dict(ok, column="rso"), "column"), (dict(ok, rel_step=-1e-3), "rel_step"), (dict(ok, rel_step=np.nan), "rel_step"),
                     (dict(ok, lidf="fast"), "lidf"), (dict(ok, band_model="SRF"), "band_model"),
                     (dict(ok, weights=np.ones((3, 13))), "weights"), (dict(ok, obs=np.zeros((5, 13))), "obs"),
                     (dict(ok, obs=np.zeros(13)), "obs"), (dict(ok, prior={"Cw": (0.01, 0.01)}), "not free"),
                     (dict(ok, prior={"LAI": (3.0, 0.0)}), "sigma"), (dict(ok, prior_mean=np.zeros(2)), "together"),
                     (dict(ok, prior={"LAI": (3.0, 1.0)}, prior_mean=np.zeros(2), prior_weight=np.ones(2)), "exclude"),
                     (dict(ok, prior_mean=np.zeros(3), prior_weight=np.zeros(3)), "expected both")):
        kw = dict(kw)
        o = kw.pop("obs", obs)
        with pytest.raises(ValueError, match=text):
            spart_amd.posterior(P.T, o, S2, **kw)
    with pytest.raises(ValueError, match="27"):
        spart_amd.posterior(P.T[:26], obs, S2, **ok)
    for kw, text in ((dict(free=["nope"]), "unknown"), (dict(ok, column="x"), "column"), (dict(ok, rel_step=0.0), "rel_step"),
                     (dict(ok, band_model=None), "band_model"), (dict(ok, lidf=1), "lidf")):
        with pytest.raises(ValueError, match=text):
            spart_amd.jacobian(P.T, S2, **kw)
        with pytest.raises(ValueError, match=text):
            spart_amd.posterior(P.T, None, S2, **kw)
    with pytest.raises(ValueError, match="27"):
        spart_amd.jacobian(P.T[:26], S2, **ok)
    with pytest.raises(ValueError, match="weights"):                            # obs=None: the rows come from params
        spart_amd.posterior(P.T, None, S2, weights=np.ones((3, 13)), **ok)
    # Engine.posterior / jacobian / refine(posterior=True) themselves, on an Engine object that was never initialised
    e = engine.Engine.__new__(engine.Engine)
    e.nb, e.srf_aligned = 13, np.ones(13, dtype=bool)
    with pytest.raises(ValueError, match="unknown"):
        e.posterior(list(P.T), obs, ["LAI", "nope"])
    with pytest.raises(ValueError, match="obs"):
        e.posterior(list(P.T), np.zeros((4, 12)), ["LAI"])
    with pytest.raises(ValueError, match="weights"):
        e.posterior(list(P.T), None, ["LAI"], weights=np.ones(12))
    with pytest.raises(ValueError, match="exclude"):
        e.posterior(list(P.T), obs, ["LAI"], prior={"LAI": (3.0, 1.0)}, prior_mean=np.zeros(1), prior_weight=np.ones(1))
    with pytest.raises(ValueError, match="band_model"):
        e.jacobian(list(P.T), ["LAI"], band_model="x")
    with pytest.raises(ValueError, match="twice"):
        e.jacobian(list(P.T), ["LAI", "LAI"])
    with pytest.raises(ValueError, match="n_iter"):
        e.refine(list(P.T), obs, ["LAI"], n_iter=1000, posterior=True)
    e.srf_aligned = np.arange(13) != 4
    with pytest.raises(ValueError, match="align_srf"):
        e.posterior(list(P.T), obs, ["LAI"], band_model="srf")


def test_retrieve_and_retrieve_stream_posterior_option(tmp_path):
    from spart_amd import lut, workloads
    rng = np.random.default_rng(0)
    P = workloads.lhs_params(32, "full", seed=2)
    d = str(tmp_path / "plain")
    os.makedirs(d)
    np.save(os.path.join(d, "params.npy"), P)
    np.save(os.path.join(d, "R_TOC.npy"), rng.random((32, 13)))
    json.dump({"sensor": S2, "dtype": "float64", "columns": ["R_TOC"], "rows": 32}, open(os.path.join(d, "meta.json"), "w"))
    obs = rng.random((3, 13))
    assert "posterior" in lut.REFINE_OPTS and list(lut.POSTERIOR_KEYS) == ["refined_cov", "refined_ak", "refined_dfs"]
    for call in (lut.retrieve, lut.retrieve_stream):
        for value in (1, "yes", None):
            with pytest.raises(ValueError, match="posterior"):
                call(d, obs, 3, refine=["LAI"], refine_opts={"posterior": value})
        with pytest.raises(ValueError, match="refine_opts"):
            call(d, obs, 3, refine_opts={"posterior": True})                     # options without refine=
    shapes = lut._refined_shapes(5, 3, True)
    assert shapes["refined_cov"] == ((5, 3, 3), np.float64) and shapes["refined_ak"] == ((5, 3, 3), np.float64)
    assert shapes["refined_dfs"] == ((5,), np.float64) and "refined_cov" not in lut._refined_shapes(5, 3)
    empty = lut._unmatched(shapes)
    assert np.isnan(empty["refined_cov"]).all() and np.isnan(empty["refined_ak"]).all() and np.isnan(empty["refined_dfs"]).all()
    bad_out = {n: np.zeros(s, dtype=t) for n, (s, t) in lut._refined_shapes(3, 1).items()}
    bad_out.update({n: np.zeros((3, 27)) for n in lut.STREAM_MAPS}, count=np.zeros(3, dtype=np.int32), best_cost=np.zeros(3))
    with pytest.raises(ValueError, match="refined_"):                             # out= must carry the posterior arrays too
        lut.retrieve_stream(d, obs, 3, refine=["LAI"], refine_opts={"posterior": True}, out=bad_out)
