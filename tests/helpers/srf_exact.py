"""The SRF band sums of k_columns_srf pinned exactly (tests/test_srf_exact_host.py on the CPU, tests/test_gpu_srf_sums.py on
the GPU).  Imports no part of the HIP library except the packaged Sentinel-2A table (for SMAC coefficients).

Two questions, each with one answer:
  1. what the kernel evaluates at evaluation e of row s: probe_sensor() has 2002 bands, band e ONE SRF sample of weight 1 at
     400 + e nm (e = 2001: 2500 nm, the thermal evaluation), so fma(1, x, 0) / 1 == x and the probe's rso_srf ... rdd_srf ARE
     the kernel's per-evaluation values X[s, e];
  2. whether a sensor's band sum combines them as include/spart_hip.h defines: srf_chain(X, support) is that definition as
     a chain of correctly rounded FMAs from 0 (std::fma, tests/hostmath/srf_chain.cpp) and one IEEE division -- ONE float64
     answer per row and band.
"""
import ctypes
import os
import subprocess

import numpy as np

from helpers import srf_numpy

HM = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hostmath"))
NEV = 2002                      # evaluations 0..2001 (2001 = the thermal evaluation)
_LIB = None


def lib():
    """tests/hostmath/libsrfchain.so, built with g++ as tests/test_hostmath.py builds libhostmath.so (kept out of git)"""
    global _LIB
    if _LIB is None:
        so, src = os.path.join(HM, "libsrfchain.so"), os.path.join(HM, "srf_chain.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-o", so, src])
        _LIB = ctypes.CDLL(so)
        _LIB.srf_chain.restype = None
    return _LIB


def srf_chain(X, lists):
    """X (B, ne) float64 per-evaluation values, lists = (start, ev, q, Q) of srf_numpy.support ->
    (out (B, nb) the band sums by the definition, S (B, nb) = sum |q_e| |X[s, e]| / |Q_j|, n (nb,) support lengths)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    start, ev, q, Q = lists
    start, ev = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(ev, dtype=np.int32)
    q, Q = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    B, ne = X.shape
    nb = Q.size
    assert start.shape == (nb + 1,) and start[0] == 0 and start[-1] == ev.size == q.size and np.all(np.diff(start) >= 0)
    assert ev.size == 0 or (ev.min() >= 0 and ev.max() < ne)
    out, S = np.empty((B, nb)), np.empty((B, nb))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    lib().srf_chain(ctypes.c_int64(B), ctypes.c_int64(ne), X.ctypes.data_as(dp), start.ctypes.data_as(ip), ev.ctypes.data_as(ip),
                    q.ctypes.data_as(dp), Q.ctypes.data_as(dp), ctypes.c_int32(nb), out.ctypes.data_as(dp), S.ctypes.data_as(dp))
    return out, S, np.diff(start).astype(np.int64)


def chain_bound(S, n):
    """|chain - any other evaluation of the same sum in the same order| <= (n_j + 1) 2^-53 S: n roundings of the accumulate
    and one of the division, each at most half an ulp of a partial result that S bounds (first order)"""
    return (np.asarray(n, dtype=np.float64)[None, :] + 1.0) * 2.0 ** -53 * S


def _sensor(centres, wl_srf, p_srf, tag):
    """a reference-style sensorinfo dict; SMAC coefficients of the nearest Sentinel-2A band (the rule of
    test_gpu_hyperspectral.synthetic_sensor)"""
    from spart_amd import tables
    s2 = tables.load_sensor_info("Sentinel2A-MSI")
    c = np.asarray(centres, dtype=np.float64)
    s2c = np.asarray(s2["wl_smac"], dtype=np.float64).reshape(-1)
    near = np.argmin(np.abs(np.minimum(c, 2500.0)[:, None] - s2c[None, :]), axis=1)
    return {"wl_smac": c[:, None], "band_id_smac": [f"{tag}{j}" for j in range(c.size)],
            "SMAC_coef": {n: np.asarray(v, dtype=np.float64).reshape(1, -1)[:, near].copy() for n, v in s2["SMAC_coef"].items()},
            "wl_srf_smac": np.ascontiguousarray(wl_srf, dtype=np.float64), "p_srf_smac": np.ascontiguousarray(p_srf, dtype=np.float64)}


def probe_sensor():
    """2002 bands: band e has one SRF sample of weight 1 at 400 + e nm (e <= 2000) or at 2500 nm (e = 2001)"""
    c = np.concatenate([np.arange(400.0, 2401.0), [2500.0]])
    return _sensor(c, c[None, :].copy(), np.ones((1, NEV)), "E")


def hostile_table():
    """(nsrf, 3): NaN, +-tiny, negative, x.5 ties, the 2400 / 2500 gap (2450 and just above), thermal-pad ties, 60000, zero,
    negative and duplicated weights -- every |w| < 1e15, where the literal argmin is the definition"""
    tiny = np.nextafter(0.0, 1.0)
    col0 = [np.nan, tiny, -tiny, -5.0, 0.0, 399.5, 400.0, 400.5, 401.5, 401.5, 1000.5, 1000.4999999999999, 1000.5000000000001,
            2399.5, 2400.0, 2400.5, 2450.0, 2450.01, np.nextafter(2450.0, 3000.0), np.nextafter(2450.0, 0.0), 2499.9, 2500.0]
    col1 = [2550.0, 2550.0000001, 2549.9999, 14950.0, 15000.0, 15500.0, 15500.0001, 16000.0, 16500.0, 16500.5, 49500.0, 49501.0,
            50000.0, 60000.0, 1e14, -1e14, np.nan, np.nan, 700.0, 700.0, 700.2, 699.8]
    col2 = [np.nan] * 21 + [865.0]
    w = np.array([col0, col1, col2], dtype=np.float64).T
    rng = np.random.default_rng(7)
    p = rng.uniform(-1.0, 1.0, w.shape)
    p[0, 0] = 0.0                                          # a zero weight on the NaN wavelength: the entry stays
    p[4, 0] = -0.0
    p[5:8, 0] = [0.25, -0.25, 1e-300]
    p[16, 1], p[17, 1] = 0.0, 0.0
    p[:21, 2] = 0.0                                        # band 2: Q from one sample, index 0 entry of weight 0 kept
    return w, p


DEAL_BANDS = ("long", "one_700", "one_thermal", "one_1650", "plus_minus", "zero_weight", "hostile")


def dealing_sensor():
    """7 bands (not a multiple of 4) of 2002 SRF samples each, by DEAL_BANDS:
      long         every evaluation 0..2001 once, weights in (0.2, 1): the longest support there is
      one_700, one_thermal, one_1650   one entry each (700 nm; 2500 nm, the thermal evaluation alone; 1650 nm with q = Q = 0.75)
      plus_minus   +1 at 600 nm, -1 at 601 nm: Q = 0
      zero_weight  a sample of weight 0 at 450 nm beside weight 1 at 865 nm: the entry stays, 0 * NaN is NaN
      hostile      column 0 of hostile_table() (NaN wavelength, ties, the 2400 / 2500 gap) with one NaN and one infinite weight
    Bands shorter than 2002 samples are padded with weight-0 repeats of their first wavelength (no new entry, q unchanged:
    x + 0 == x for the sums srf_numpy.support forms; the hostile band's padding goes to its NaN wavelength, evaluation 0)."""
    n = NEV
    w, p = np.empty((n, 7)), np.zeros((n, 7))
    w[:, 0] = np.concatenate([np.arange(400.0, 2401.0), [2500.0]])
    p[:, 0] = np.random.default_rng(11).uniform(0.2, 1.0, n)
    for j, (wl, wt) in ((1, (700.0, 1.0)), (2, (2500.0, 1.0)), (3, (1650.0, 0.75))):
        w[:, j], p[0, j] = wl, wt
    w[:, 4] = 600.0
    w[1, 4] = 601.0
    p[0, 4], p[1, 4] = 1.0, -1.0
    w[:, 5] = 450.0
    w[1, 5], p[1, 5] = 865.0, 1.0
    hw, hp = hostile_table()
    m = hw.shape[0]
    w[:, 6] = hw[0, 0]
    w[:m, 6], p[:m, 6] = hw[:, 0], hp[:, 0]
    p[3, 6], p[10, 6] = np.nan, np.inf
    return _sensor([1400.0, 700.0, 2500.0, 1650.0, 600.0, 865.0, 1000.0], w, p, "D")
