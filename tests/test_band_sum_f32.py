"""CPU build (g++) of the float32 sample of the headline band kernel k_bands<float, 0, 1>, composed as its sample loop composes
it (tests/hostmath/hostmath.cpp hm_band_sum_f32: leaf_band<float, PRO>, canopy_core_l with the prelude's C_KSL / C_KOL,
soil_dry -> soil_band_tw, canopy_soil_sum), per sample and band against the float64 oracle on the domain grid of
tests/helpers/domain_grid.py, at the conditioning-aware float32 bound that tests/test_gpu_band_sums.py holds the GPU kernel
to.  A failure there that does not show here points at GPU intrinsics or contraction, not at the formula."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import domain_grid as G

HM = os.path.join(ROOT, "tests", "hostmath")


@pytest.fixture(scope="module")
def hm():
    so = os.path.join(HM, "libhostmath.so")
    src = os.path.join(HM, "hostmath.cpp")
    hdr = os.path.join(ROOT, "spart-python_amd", "csrc", "spart_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, src])
    return ctypes.CDLL(so)


def dp(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.fixture(scope="module")
def grid(oracle, tables):
    return G.build_grid(oracle, tables)


@pytest.fixture(scope="module")
def sums(hm, tables, grid):
    """(common-case body, general body) outputs, (rows, 2002) each"""
    t = np.zeros((17, 2001))
    args = [np.ascontiguousarray(tables[k], dtype=np.float64)
            for k in ["nr", "nw", "Kab", "Kca", "Kdm", "Kw", "Ks", "Kant", "cbc", "prot", "GSV"]]
    hm.hm_derive_tables(*[dp(a) for a in args], t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    P, rho, tau = (np.ascontiguousarray(grid[k], dtype=np.float64) for k in ("P", "rho", "tau"))
    out = []
    for common in (1, 0):
        o = np.zeros((len(P), G.NEV))
        hm.hm_band_sum_f32(ctypes.c_int(common), ctypes.c_int64(len(P)), t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                           dp(P), dp(rho), dp(tau), o.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        out.append(o)
    return out


def test_grid_covers_both_bodies_and_every_kind(grid):
    kinds = {k: int((grid["kind"] == k).sum()) for k in np.unique(grid["kind"])}
    assert kinds == {"ota_full": 44, "ota_pro": 46, "past": 72, "corner_full": 128, "corner_pro": 128, "golden": 125}, kinds
    assert grid["common"].sum() >= 300 and (~grid["common"]).sum() >= 100
    assert (grid["common"] & grid["inside"]).sum() >= 150 and (~grid["common"] & grid["inside"]).sum() >= 90
    assert G.bare_soil(grid["P"]).sum() == G.BARE_SOIL_ROWS


def test_headline_sample_vs_oracle(grid, sums):
    """rso + rdo + rsd + rdd of the general body, every row and band of the grid, within max(1e-4, C32 delta) of the oracle
    (floor 1e-2; the bare-soil rows within 4e-4, domain_grid.bare_soil)"""
    ex = G.excess(sums[1], grid)
    assert np.isfinite(sums[1]).all()
    r, b = np.unravel_index(np.argmax(ex), ex.shape)
    assert ex.max() <= 1.0, (int(r), grid["kind"][r], int(b), float(G.rel(sums[1], grid["sum"])[r, b]), float(grid["d_sum"][r, b]))


def test_common_body_equals_general_body(grid, sums):
    """cbc = prot = 0 rows: the common-case body (PRO = false) gives the general body's bits in every band"""
    c = grid["common"]
    assert np.array_equal(sums[0][c], sums[1][c])
