"""CPU build (g++) of SAILH's J2 under the float32 band kernel's per-stage vote (sail_j2_possible, csrc/spart_math.h) against a
copy of the form it replaced, kept in tests/hostmath/diet3_forms.cpp, bit for bit.  Inputs: the LHS ranges over all 2001 bands
with LAI drawn from [0.005, 0.2] (ks LAI and ko LAI on both sides of the J2 threshold) and samples with a NaN C_KSL or C_KOL
row.  (The wet / dry select from a voted bit and the plate model's K clamp inside its small-K branch were compared the same
way and then dropped with the cuts themselves: profiles/EXPERIMENTS.md, round 9.)  No GPU needed; tests/test_gpu_diet3.py runs
the kernel."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostmath", "diet3_forms.cpp")
LAI = 15
NAMES = ("cases", "j2", "taylor", "skipped", "core")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("diet3_forms") / "libdiet3_forms.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    L = ctypes.CDLL(so)
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


def _compare(lib, tab, P, flags):
    P = np.ascontiguousarray(P, dtype=np.float64)
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    out = np.zeros(5, dtype=np.int64)
    lib.diet3_compare(ctypes.c_int64(len(P)), dp(tab), dp(P), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return dict(zip(NAMES, (int(v) for v in out)))


def _low_lai(n, kind, seed):
    from spart_amd import workloads
    P = np.ascontiguousarray(workloads.lhs_params(n, kind, seed=seed))
    P[:, LAI] = np.random.default_rng(seed + 1).uniform(0.005, 0.2, n)
    return P


@pytest.mark.parametrize("kind", ["full", "pro"])
def test_shortcuts_equal_the_forms_they_replace(lib, tab, kind):
    """LAI in [0.005, 0.2]: at least 1 % of the (sample, band) cases take a J2's Taylor side by the old form's own test, the
    vote's bit lets others skip the test -- and nothing differs in any bit"""
    P = _low_lai(192, kind, 21)
    r = _compare(lib, tab, P, np.zeros(len(P)))
    assert r["cases"] == len(P) * 2001
    assert r["taylor"] >= 0.01 * r["cases"], r
    assert r["skipped"] >= 0.01 * r["cases"], r
    assert r["j2"] == r["core"] == 0, r


def test_usual_lai_skips_the_j2_test(lib, tab):
    """the benchmark's own ranges (LAI 0.5..7): no case is on the Taylor side and nearly every sample's bit is clear"""
    from spart_amd import workloads
    P = np.ascontiguousarray(workloads.lhs_params(96, "full", seed=22))
    r = _compare(lib, tab, P, np.zeros(len(P)))
    assert r["taylor"] == 0 and r["skipped"] >= 0.9 * r["cases"], r
    assert r["j2"] == r["core"] == 0, r


def test_nan_constants_take_the_old_path(lib, tab):
    """a NaN C_KSL or C_KOL sets the bit: the per-band test runs as before"""
    P = np.concatenate([_low_lai(32, "full", 23), _low_lai(32, "full", 24)])
    flags = np.zeros(len(P), dtype=np.int32)
    flags[0::4] |= 1
    flags[1::4] |= 2
    flags[2::4] |= 3
    r = _compare(lib, tab, P, flags)
    assert 0 < r["skipped"] <= (len(P) // 4) * 2001, r   # only the quarter with neither row NaN can skip the test
    assert r["taylor"] > 0 and r["j2"] == r["core"] == 0, r
