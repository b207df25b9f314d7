"""spart_refine_srf without a GPU: the binding and the header; the refusals of retrieve / retrieve_stream / Engine.refine /
spart_amd.refine that need no device (the fit's band model must be the LUT's, and is never chosen silently); and the twin
experiment with the oracle that says why the SRF model has to be the fitted quantity for SRF observations."""
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import srf_numpy as S

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402

S2 = "Sentinel2A-MSI"
CANOPY = ("rso", "rdo", "rsd", "rdd")


# ---- 1. binding and header
def test_binding_and_header():
    from spart_amd import _lib
    assert "spart_refine_srf" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["spart_refine_srf"]
    assert (res, list(args)) == (_lib.SIGNATURES["spart_refine"][0], list(_lib.SIGNATURES["spart_refine"][1])) and len(args) == 19
    assert _lib.ABI_VERSION == 14
    hdr = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    assert "#define SPART_ABI_VERSION 14" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", code) for n in ("spart_refine", "spart_refine_srf")}
    assert decl["spart_refine"] and decl["spart_refine_srf"]
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()      # noqa: E731
    assert squeeze(decl["spart_refine_srf"].group(1)) == squeeze(decl["spart_refine"].group(1))      # argument for argument
    assert len(re.findall(r"\bspart_refine\w*_workspace_bytes\s*\(", code)) == 1                       # one size query for both
    # the version list says that the symbol came without a new number
    versions = hdr[hdr.index("Version of THIS interface"):hdr.index("#define SPART_ABI_VERSION")]
    assert "spart_refine_srf" in versions


def test_a_library_without_the_symbol_is_refused_by_name(tmp_path):
    """a foreign library of interface version 14 that lacks spart_refine_srf: load() names the symbol"""
    import subprocess
    from spart_amd import _lib
    src = tmp_path / "old.c"
    src.write_text("int spart_abi_version(void) { return 14; }\nconst char *spart_build_id(void) { return \"x\"; }\n"
                   + "".join(f"int {n}(void) {{ return 0; }}\n" for n in _lib.SIGNATURES
                             if n not in ("spart_abi_version", "spart_build_id", "spart_refine_srf")))
    so = str(tmp_path / "libold.so")
    subprocess.check_call(["g++", "-x", "c", "-shared", "-fPIC", "-o", so, str(src)])
    with pytest.raises(RuntimeError, match="spart_refine_srf"):
        _lib.load(so)
    assert os.path.abspath(so) not in _lib._libs


# ---- 2. refusals before any device
def write_lut(d, P, rng, **meta):
    os.makedirs(d)
    np.save(os.path.join(d, "params.npy"), P)
    np.save(os.path.join(d, "R_TOC.npy"), rng.random((P.shape[0], 13)))
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(dict({"sensor": S2, "dtype": "float64", "columns": ["R_TOC"], "rows": int(P.shape[0])}, **meta), f)
    return str(d)


def test_the_band_model_of_the_fit_is_the_luts_and_is_said(tmp_path, monkeypatch):
    from spart_amd import engine, lut, workloads

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(lut, "get_engine", no_device)
    monkeypatch.setattr(engine, "get_engine", no_device)
    rng = np.random.default_rng(0)
    P = workloads.lhs_params(32, "full", seed=2)
    obs = rng.random((3, 13))
    assert "band_model" in lut.REFINE_OPTS
    srf = write_lut(tmp_path / "srf", P, rng, band_model="srf")
    centre = write_lut(tmp_path / "centre", P, rng, band_model="centre")
    old = write_lut(tmp_path / "old", P, rng)                                # (no band_model in meta.json: a centre LUT)
    for call in (lut.retrieve, lut.retrieve_stream):
        for opts in (None, {"n_iter": 2}, {"band_model": "centre"}, {"band_model": "SRF"}):
            with pytest.raises(ValueError, match="srf") as e:
                call(srf, obs, 3, refine=["LAI"], refine_opts=opts)
            if opts is None or opts.get("band_model") == "centre" or "n_iter" in opts:
                assert '"band_model": "srf"' in str(e.value) and "refine_opts" in str(e.value)     # what to pass
        for d in (centre, old):
            with pytest.raises(ValueError, match="srf") as e:
                call(d, obs, 3, refine=["LAI"], refine_opts={"band_model": "srf"})
            assert '"band_model": "centre"' in str(e.value)
            for value in ("SRF", "center", None, 1):
                with pytest.raises(ValueError, match="band_model"):
                    call(d, obs, 3, refine=["LAI"], refine_opts={"band_model": value})
        with pytest.raises(ValueError, match="refine_opts"):
            call(srf, obs, 3, refine_opts={"band_model": "srf"})              # options without refine=


def test_refine_band_model_is_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    P = workloads.lhs_params(4, "full", seed=1)
    obs = np.zeros((4, 13))
    for value in ("x", "SRF", None):
        with pytest.raises(ValueError, match="band_model"):
            spart_amd.refine(P.T, obs, S2, ["LAI"], band_model=value)
    e = engine.Engine.__new__(engine.Engine)                                 # an Engine object that was never initialised
    e.nb, e.srf_aligned = 13, np.ones(13, dtype=bool)
    with pytest.raises(ValueError, match="band_model"):
        e.refine(list(P.T), obs, ["LAI"], band_model="x")
    with pytest.raises(ValueError, match="unknown"):                         # a good band model: the next check is reached
        e.refine(list(P.T), obs, ["LAI", "nope"], band_model="srf")
    e.srf_aligned = np.arange(13) != 4
    with pytest.raises(ValueError, match="align_srf"):
        e.refine(list(P.T), obs, ["LAI"], band_model="srf")
    with pytest.raises(ValueError, match="unknown"):                         # the centre model does not look at the SRFs' order
        e.refine(list(P.T), obs, ["LAI", "nope"])
    e.nb, e.srf_aligned = 0, np.zeros(0, dtype=bool)
    with pytest.raises(ValueError, match="sensor"):
        e.refine(list(P.T), np.zeros((4, 0)), ["LAI"], band_model="srf")


# ---- 3. the twin experiment with the oracle
def test_twin_experiment_with_the_oracle_srf_model(oracle, tables):
    """Sentinel-2A, 48 LHS rows, free = LAI, Cab, Cw, Cdm over their RANGES, observations = the SRF-convolved R_TOC of the truth
    (the oracle's full spectra -> srf_numpy.convolve -> the oracle's SMAC -> srf_numpy.toc_to_toa), ten iterations.
    The SRF model started 15 % of the range away is back at the truth in every row (the oracle alone: cost / cost0 <= 3.3e-27,
    |x - truth| <= 5.6e-14 of the range; the caps are those of test_refine_host's centre twin and allow no exceptions).
    The centre model fitted to the same observations FROM the truth leaves it: every row ends with a parameter off by >= 1 % of
    its range (the oracle alone: >= 3.2 %), the median error per parameter is >= 2 % (4.2 ... 7.5 %), while its cost falls."""
    from spart_amd import workloads
    names = ["LAI", "Cab", "Cw", "Cdm"]
    free = [workloads.PARAM_NAMES.index(n) for n in names]
    lo = np.array([workloads.RANGES[n][0] for n in names], dtype=np.float64)
    hi = np.array([workloads.RANGES[n][1] for n in names], dtype=np.float64)
    truth = workloads.lhs_params(48, "full", seed=5)
    sens = oracle.sensor_tables(tables, S2)
    lists = S.support(sens["wl_srf"], sens["p_srf"])
    econv = oracle.et_convolution(tables, sens)

    def forward_srf(rows):
        with np.errstate(all="ignore"):
            full = oracle.spart_run(rows, S2, tables, pso="gl", full=True)
            conv = {x: S.convolve(full[x], sens["wl_srf"], sens["p_srf"], lists) for x in CANOPY}
            at = oracle.smac(rows[:, 19:22], rows[:, 22:26], sens)
            La = (oracle.et_correction(rows[:, 26]) * np.cos(rows[:, 19] * np.pi / 180) / np.pi)[:, None] * econv[None, :]
            return S.toc_to_toa(at, conv["rso"], conv["rdo"], conv["rsd"], conv["rdd"], La)[0]

    def forward_centre(rows):
        with np.errstate(all="ignore"):
            return np.asarray(oracle.spart_run(rows, S2, tables, pso="gl")["R_TOC"], dtype=np.float64)
    obs = forward_srf(truth)
    assert np.isfinite(obs).all()
    start = truth.copy()
    centre = 0.5 * (lo + hi)
    start[:, free] = truth[:, free] + 0.15 * (hi - lo) * np.sign(centre - truth[:, free])
    res = rd.refine_defined(start, free, lo, hi, obs, forward_srf, n_iter=10)
    err = np.abs(res["x"] - truth[:, free]) / (hi - lo)
    print("srf model: max cost / cost0", float((res["cost"] / res["cost0"]).max()), " max |x - truth| / range", float(err.max()),
          " accepted steps", int(res["n_accept"].min()), "...", int(res["n_accept"].max()))
    assert (res["n_accept"] >= 0).all() and (res["cost"] <= res["cost0"]).all()
    assert (res["cost"] <= 1e-8 * res["cost0"]).all(), float((res["cost"] / res["cost0"]).max())
    assert (err <= 1e-6).all(), float(err.max())
    # the centre model, started AT the truth
    off = rd.refine_defined(truth, free, lo, hi, obs, forward_centre, n_iter=10)
    e = np.abs(off["x"] - truth[:, free]) / (hi - lo)
    print("centre model from the truth: median error / range per parameter", np.median(e, axis=0), " worst parameter of the best row",
          float(e.max(axis=1).min()), " median cost0", float(np.median(off["cost0"])), "-> cost", float(np.median(off["cost"])))
    assert (off["n_accept"] >= 1).all() and (off["cost"] < off["cost0"]).all()      # it reports an improvement ...
    assert (e.max(axis=1) >= 0.01).all(), float(e.max(axis=1).min())                 # ... while every row leaves the truth
    assert (np.median(e, axis=0) >= 0.02).all(), np.median(e, axis=0)
