"""The likelihood-weighted LUT estimate without a GPU: its numpy definition (tools/lut_bayes_defined.py) against a long-double /
math.fsum evaluation and by hand, spart_lut_bayes_workspace_bytes, the refusals of spart_lut_bayes that come before anything
touches a device, and the argument refusals of retrieve(bayes=...)."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))

import lut_bayes_defined as defined  # noqa: E402
import lut_brute_force as bf  # noqa: E402


def small_case(dt, seed, B=300, nb=7, M=12, P=4, rel=0.5):
    rng = np.random.default_rng(seed)
    lut = rng.uniform(0.0, 0.6, (B, nb)).astype(dt)
    lut[[11, 12, 40]] = lut[5]                               # ties
    lut[17, 2] = np.nan                                      # a row that is never accepted
    params = rng.uniform(-3.0, 8.0, (B, P))
    obs = (lut[rng.integers(0, B, M)] + rng.normal(0, 0.05, (M, nb))).astype(dt)
    obs[0] = lut[5]
    w = (1.0 / (rel * np.abs(obs.astype(np.float64)) + 0.01) ** 2).astype(dt)
    w[1] = 0                                                 # all masked: every accepted row, omega = 1
    obs[1, 3] = np.nan
    w[2, 0] = -1.0                                           # invalid observations
    obs[3, 3] = np.inf
    w[4, 2], obs[4, 2] = 0, np.nan                           # one masked band
    return lut, params, obs, w


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("cut,tau", [(50.0, 1.0), (3.0, 0.25), (np.inf, 2.0), (0.0, 1.0)])
def test_definition_against_long_double(dt, cut, tau):
    lut, params, obs, w = small_case(dt, 3)
    B, M = lut.shape[0], obs.shape[0]
    got = defined.lut_bayes_defined(lut, params, obs, w, cut=cut, temperature=tau)
    idx, cost = bf.brute_force_topk_obs_weights_numpy(lut, obs, B, w)
    for m in range(M):
        rows = [int(r) for r in idx[m] if r >= 0]
        if not rows:                                         # the empty-observation outputs
            assert m in (2, 3)
            assert got["count"][m] == 0 and got["best_idx"][m] == -1 and np.isinf(got["best_cost"][m]) and got["sum_w"][m] == 0
            assert np.isnan(got["ess"][m]) and np.isnan(got["mean"][m]).all() and np.isnan(got["std"][m]).all()
            continue
        c = {int(r): cost[m, i] for i, r in enumerate(idx[m]) if r >= 0}
        cstar = min(c.values())
        best = min(r for r in rows if c[r] == cstar)
        assert got["best_idx"][m] == best and got["best_cost"][m] == cstar and got["best_cost"].dtype == dt
        S = sorted(r for r in rows if float(c[r]) - float(cstar) <= cut)
        assert got["count"][m] == len(S) and 17 not in S
        ld = np.longdouble
        om = [np.exp(-((ld(float(c[r])) - ld(float(cstar))) / (2 * ld(tau)))) for r in S]
        sw = math.fsum(float(o) for o in om)
        n = len(S)
        # the ordered float64 sums against the exact ones: (n - 1) roundings of the sum, one per term, exp within 1 ulp, and
        # the rounding of its argument a <= cut / (2 tau), which moves omega by a * 2^-53 (omega = 0 beyond a = 750)
        tol = (n + 4 + min(cut / tau, 1500.0)) * 2.0 ** -52
        assert abs(got["sum_w"][m] - sw) <= tol * sw
        s2 = math.fsum(float(o) ** 2 for o in om)
        assert abs(got["ess"][m] - sw * sw / s2) <= 4 * tol * sw * sw / s2
        for p in range(params.shape[1]):
            x = params[S, p]
            mean = math.fsum(float(o) * v for o, v in zip(om, x)) / sw
            a = math.fsum(float(o) * abs(v) for o, v in zip(om, x)) / sw
            assert abs(got["mean"][m, p] - mean) <= 2 * tol * a
            var = math.fsum(float(o) * (v - mean) ** 2 for o, v in zip(om, x)) / sw
            assert abs(got["std"][m, p] ** 2 - var) <= 4 * tol * var + 2 * (2 * tol * a) ** 2
    if cut == 0.0:                                           # consequences the header states
        assert got["count"][0] == 4                          # the tied rows 5, 11, 12, 40, exactly
        one = got["count"] == 1
        assert one.any()
        assert np.array_equal(got["mean"][one], params[got["best_idx"][one]]) and (got["std"][one] == 0).all()
        assert (got["ess"][one] == 1).all() and (got["sum_w"][one] == 1).all()
    # all weights zero: omega = 1, spart_lut_summarise's ordered sums over every accepted row
    rows = np.array([[r for r in range(B) if r != 17]], dtype=np.int64)
    mean, _, std, count = bf.summarise_defined(params, rows)
    assert got["count"][1] == count[0] == B - 1 and got["sum_w"][1] == B - 1 and got["ess"][1] == B - 1
    assert np.array_equal(got["mean"][1], mean[0]) and np.array_equal(got["std"][1], std[0]) and got["best_idx"][1] == 0


def test_definition_by_hand():
    """nb = 1, obs 0, w 1: e = x^2 exactly; the sums in the order of the rows"""
    lut = np.array([[1.0], [0.0], [2.0], [np.nextafter(2.0, 3.0)], [3.0]])
    params = np.array([[10.0], [20.0], [40.0], [80.0], [160.0]])
    obs, w = np.zeros((1, 1)), np.ones((1, 1))
    r = defined.lut_bayes_defined(lut, params, obs, w, cut=4.0, temperature=1.0)
    assert r["count"].tolist() == [3] and r["best_idx"].tolist() == [1] and r["best_cost"].tolist() == [0.0]
    o1, o2 = np.exp(-(1.0 / 2.0)), np.exp(-(4.0 / 2.0))
    sw = (o1 + 1.0) + o2
    assert r["sum_w"][0] == sw and r["ess"][0] == (sw * sw) / ((o1 * o1 + 1.0) + o2 * o2)
    mean = ((o1 * 10.0 + 1.0 * 20.0) + o2 * 40.0) / sw
    assert r["mean"][0, 0] == mean
    d = [10.0 - mean, 20.0 - mean, 40.0 - mean]
    assert r["std"][0, 0] == np.sqrt((((o1 * d[0]) * d[0] + (1.0 * d[1]) * d[1]) + (o2 * d[2]) * d[2]) / sw)
    r = defined.lut_bayes_defined(lut, params, obs, w, cut=4.0, temperature=0.0)          # 0 = 1.0
    assert r["sum_w"][0] == sw
    r = defined.lut_bayes_defined(lut[:0], params[:0], obs, w)                             # an empty table
    assert r["count"].tolist() == [0] and r["best_idx"].tolist() == [-1] and np.isnan(r["mean"]).all()


@pytest.fixture(scope="module")
def lib():
    import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.spart_last_error.restype = ctypes.c_char_p
    lib.spart_lut_bayes_workspace_bytes.restype = ctypes.c_size_t
    lib.spart_lut_bayes_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
    from spart_amd import _lib
    lib.spart_lut_bayes.restype = ctypes.c_int
    lib.spart_lut_bayes.argtypes = _lib.SIGNATURES["spart_lut_bayes"][1]
    lib.spart_lut_bayes_stats.restype = ctypes.c_int
    lib.spart_lut_bayes_stats.argtypes = _lib.SIGNATURES["spart_lut_bayes_stats"][1]
    return lib


def test_workspace_bytes_is_zero_exactly_for_refused_sizes(lib):
    f = lib.spart_lut_bayes_workspace_bytes

    def size(dtype=0, B=1000, nb=13, M=10):
        return f(dtype, B, nb, M)
    for bad in ({"nb": 0}, {"nb": 2163}, {"dtype": 2}, {"dtype": -1}, {"B": -1}, {"M": -1}, {"B": 2_000_000_001},
                {"M": 2_000_000_001}, {"B": 0}, {"M": 0}):          # (the last two: nothing to search)
        assert size(**bad) == 0, bad
    for nb in (1, 13, 2162):
        assert size(nb=nb) > 0 and size(dtype=1, nb=nb) > 0, nb
    assert size(0, 2_000_000_000, 2162, 1_000_000) > 0 and size(1, 1, 1, 1) > 0 and size(0, 1000, 13, 2_000_000_000) > 0


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("nb,chunk", [(13, 16_384), (211, 16_384), (2162, None)])
def test_workspace_grows_by_four_bytes_per_observation_past_the_first_chunk(lib, nb, chunk, dtype):
    f = lib.spart_lut_bayes_workspace_bytes
    if chunk is None:                                  # 2162 bands: the operand rows of a chunk stay within 256 MiB
        chunk = 15_360 if dtype == 0 else 7_168
    at = f(dtype, 20_011, nb, chunk)
    sizes = [f(dtype, 20_011, nb, M) for M in (chunk - 1, chunk, chunk + 1, chunk + 37, 2 * chunk, 10 * chunk)]
    assert at > 0 and sizes == sorted(sizes)
    for extra in (1, 37, 64, 1000, chunk + 37, 1_000_000):
        grown = f(dtype, 20_011, nb, chunk + extra) - at
        assert 4 * extra <= grown < 4 * extra + 256, (extra, grown)


def test_refusals_that_need_no_device(lib):
    """every refusal of spart_lut_bayes comes before the context is used: a NULL context first, then -- with a stand-in that
    is never dereferenced -- the sizes, the structs and the options, in the header's order"""
    from spart_amd import _lib
    opt = _lib.SpartLutBayesOpt(50.0, 1.0, 0)
    buf = (ctypes.c_double * 8)()
    out = _lib.SpartLutBayesOut(*([ctypes.addressof(buf)] * 7))
    fake = ctypes.addressof((ctypes.c_char * 4096)())
    ptr = ctypes.addressof(buf)

    def call(ctx=fake, dtype=0, B=10, nb=3, P=2, M=4, opt=opt, out=out, lut=ptr):
        return lib.spart_lut_bayes(ctx, dtype, B, nb, lut, P, ptr, M, ptr, ptr, None if opt is None else ctypes.byref(opt),
                                   None if out is None else ctypes.byref(out), None, 0, None)
    assert call(ctx=None) == -1
    msg = lib.spart_last_error(None)
    assert msg.startswith(b"spart_lut_bayes") and b"null context" in msg
    for kw, word in ((dict(dtype=2), b"dtype"), (dict(nb=0), b"sizes"), (dict(nb=2163), b"sizes"), (dict(P=0), b"sizes"),
                     (dict(P=65), b"sizes"), (dict(B=-1), b"sizes"), (dict(M=-1), b"sizes"), (dict(B=2_000_000_001), b"sizes"),
                     (dict(M=2_000_000_001), b"sizes"), (dict(opt=None), b"null"), (dict(out=None), b"null"),
                     (dict(out=_lib.SpartLutBayesOut()), b"every output"),
                     (dict(opt=_lib.SpartLutBayesOpt(-1.0, 1.0, 0)), b"cut"), (dict(opt=_lib.SpartLutBayesOpt(math.nan, 1.0, 0)), b"cut"),
                     (dict(opt=_lib.SpartLutBayesOpt(1.0, -1.0, 0)), b"temperature"),
                     (dict(opt=_lib.SpartLutBayesOpt(1.0, math.nan, 0)), b"temperature"),
                     (dict(opt=_lib.SpartLutBayesOpt(1.0, math.inf, 0)), b"temperature"),
                     (dict(opt=_lib.SpartLutBayesOpt(1.0, 1.0, 2)), b"brute_force"),
                     (dict(opt=_lib.SpartLutBayesOpt(1.0, 1.0, -1)), b"brute_force"),
                     (dict(lut=None), b"null argument")):
        assert call(**kw) == -1, kw
        assert word in lib.spart_last_error(None), (kw, lib.spart_last_error(None))
    assert call() == -3 and b"workspace" in lib.spart_last_error(None)           # SPART_ERR_WORKSPACE: all else was accepted
    assert call(M=0) == 0                                                         # nothing to do, nothing launched
    assert call(opt=_lib.SpartLutBayesOpt(math.inf, 0.0, 1)) == -3                # cut = +inf and temperature 0 are values
    cnt, word = ctypes.c_int64(), ctypes.c_double()
    assert lib.spart_lut_bayes_stats(None, 0, 10, 3, 4, ptr, cnt, cnt, cnt, word) == -1
    assert lib.spart_lut_bayes_stats(fake, 0, 0, 3, 4, ptr, cnt, cnt, cnt, word) == -1       # sizes without a search


def test_struct_layouts_follow_the_header():
    import re
    from spart_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spart_hip.h")).read(), flags=re.S)
    for name, cls in (("spart_lut_bayes_opt", _lib.SpartLutBayesOpt), ("spart_lut_bayes_out", _lib.SpartLutBayesOut)):
        members = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
        assert re.findall(r"\*?\b([A-Za-z_0-9]+)\s*[,;]", members) == [f[0] for f in cls._fields_], name
    assert ctypes.sizeof(_lib.SpartLutBayesOpt) == 24 and ctypes.sizeof(_lib.SpartLutBayesOut) == 56


def write_lut(path, B=20, nb=4):
    os.makedirs(path)
    rng = np.random.default_rng(0)
    np.save(os.path.join(path, "R_TOC.npy"), rng.uniform(0, 1, (B, nb)).astype(np.float32))
    np.save(os.path.join(path, "params.npy"), rng.uniform(0, 1, (B, 27)))
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"sensor": "Sentinel2A-MSI", "dtype": "float32", "rows": B, "columns": ["R_TOC"], "band_model": "centre"}, f)


def test_retrieve_refuses_bad_bayes_arguments_before_any_device(tmp_path, monkeypatch):
    import spart_amd
    import spart_amd.lut as L

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(L, "get_engine", no_engine)
    path = str(tmp_path / "lut")
    write_lut(path)
    obs = np.zeros((3, 4), dtype=np.float32)
    for call in (spart_amd.retrieve, spart_amd.retrieve_stream):
        for bad, word in (({"cutt": 1.0}, "unknown option"), ({"cut": 1.0, "k": 3}, "unknown option"), ("knn", "expected a dict"),
                          ({"cut": -1.0}, "cut"), ({"cut": math.nan}, "cut"), ({"temperature": 0.0}, "temperature"),
                          ({"temperature": -2.0}, "temperature"), ({"temperature": math.inf}, "temperature"),
                          ({"temperature": math.nan}, "temperature")):
            with pytest.raises(ValueError, match=word):
                call(path, obs, 3, bayes=bad)
    assert L._bayes_setup(None) is None
    assert L._bayes_setup({}) == {"cut": 50.0, "temperature": 1.0}
    assert L._bayes_setup({"cut": math.inf, "temperature": 2}) == {"cut": math.inf, "temperature": 2.0}
    monkeypatch.setattr(L, "_group_info", lambda shard, group: (2, 0) if shard else (1, 0))
    with pytest.raises(ValueError, match="shard=True"):
        spart_amd.retrieve(path, obs, 3, shard=True, bayes={})
    # an empty table and M = 0: the definition's empty outputs, no device
    empty = str(tmp_path / "empty")
    write_lut(empty, B=0)
    r = spart_amd.retrieve_stream(empty, obs, 3, bayes={}, params_cols=["LAI", "Cab"])
    assert r["bayes_count"].tolist() == [0, 0, 0] and r["bayes_count"].dtype == np.int64 and r["bayes_sum_w"].tolist() == [0, 0, 0]
    assert np.isnan(r["bayes_mean"]).all() and r["bayes_mean"].shape == (3, 2) and np.isnan(r["bayes_ess"]).all()
    r = spart_amd.retrieve_stream(path, obs[:0], 3, bayes={})
    assert r["bayes_mean"].shape == (0, 27) and r["bayes_count"].shape == (0,)
    assert L._retrieve_bayes(empty, obs, "R_TOC", None, None, [0, 1], {"cut": 1.0, "temperature": 1.0})["bayes_std"].shape == (3, 2)
