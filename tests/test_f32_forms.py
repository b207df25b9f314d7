"""CPU build (g++) of the float32 forms of csrc/spart_math.h that the float32 band kernel's sample loop uses, against their
float64 forms over the benchmark's parameter ranges and all 2001 bands, and the common-case sample loop (k_bands: film shared
by the stage, cbc = prot = 0) against the general one.  No GPU needed; tests/test_gpu_common_body.py runs the kernel."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostmath", "f32_forms.cpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("f32_forms") / "libf32_forms.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.f32_common_body_mismatches.restype = ctypes.c_int64
    return L


def dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.fixture(scope="module")
def tab(tables):
    """the band tables as the kernels see them, derived by tests/hostmath (hm_derive_tables)"""
    so = os.path.join(ROOT, "tests", "hostmath", "libhostmath.so")
    if not os.path.exists(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so,
                               os.path.join(ROOT, "tests", "hostmath", "hostmath.cpp")])
    hm = ctypes.CDLL(so)
    t = np.zeros((17, 2001))
    args = [np.ascontiguousarray(tables[k], dtype=np.float64)
            for k in ["nr", "nw", "Kab", "Kca", "Kdm", "Kw", "Ks", "Kant", "cbc", "prot", "GSV"]]
    hm.hm_derive_tables(*[dp(a) for a in args], dp(t))
    return t


def _params(n, kind, seed, film=None):
    from spart_amd import workloads
    P = np.ascontiguousarray(workloads.lhs_params(n, kind, seed=seed))
    if film is not None:
        P[:, workloads.PARAM_NAMES.index("film")] = film
    return P


def test_soil_film_series_float32_against_float64(lib, tab):
    """soil_band<float>: sum_k f_k x_k / (1 - p x_k) = (sum_k f_k / (1 - p x_k) - F) / p cancels where p x_k is small; over the
    LHS ranges (SMp 5..55: wet and dry soils; film 0.0001..0.05) and all bands the float32 wet-soil reflectance stays within
    a few float32 ulp of 1 (absolute) of the float64 evaluation of the same inputs"""
    worst = 0.0
    for film in (None, 1e-4, 5e-3, 0.05):
        P = _params(256, "full", 11, film)
        out = np.zeros((len(P), 2001, 2))
        lib.f32_soil(ctypes.c_int64(len(P)), dp(tab), dp(P), dp(out))
        rf, rd = out[..., 0], out[..., 1]
        assert np.isfinite(rf).all() and np.isfinite(rd).all()
        worst = max(worst, float(np.max(np.abs(rf - rd))))
    assert worst < 1e-6, worst


def test_common_body_equals_general_body(lib, tab):
    """leaf_band<float, false> (the two PRO terms of K left off) and the film transmittance formed once per stage give the same
    bits as the general body for every band of cbc = prot = 0 samples"""
    for film in (None, 1e-4, 0.05):
        P = _params(64, "full", 12, film)
        assert lib.f32_common_body_mismatches(ctypes.c_int64(len(P)), dp(tab), dp(P)) == 0
