"""The definition of the canopy products (tools/products_defined.py; include/spart_hip.h: spart_products) without a GPU: its
restated flux terms are the oracle's bit for bit, the fCover exponent is volscatt at nadir view, and the values are finite
and span a useful range on the LHS rows.  No physical limit is asserted anywhere: sailh.py:189 (denom = 1 - rinf2 ** 2, which
the oracle and the kernels reproduce) makes the isolated canopy non-conservative, and the products are defined on that model as
it is ("Canopy products")."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import products_defined as pd  # noqa: E402


@pytest.fixture(scope="module")
def rows():
    from spart_amd import workloads
    return workloads.lhs_params(192, "full", seed=7)


@pytest.fixture(scope="module")
def terms(oracle, tables, rows):
    return pd.spectra(oracle, tables, rows)


def test_rsd_and_rdd_are_the_oracles_bit_for_bit(oracle, tables, rows, terms):
    full = oracle.spart_run(rows, "Sentinel2A-MSI", tables, pso="gl", full=True)
    assert terms["rsd"].shape == (192, 2001)
    assert np.array_equal(terms["rsd"], full["rsd"][:, :2001]) and np.array_equal(terms["rdd"], full["rdd"][:, :2001])
    assert np.array_equal(terms["rs"], full["soil_refl"])


def test_rho_dd_is_rdd_over_a_black_soil(oracle, tables, rows, terms):
    with np.errstate(all="ignore"):
        refl, tran, _ = oracle.prospect_5d(rows[:, 0:9], tables)
    rho, tau = oracle.pad_leaf(refl, tran)
    can = oracle.sailh(rho, tau, np.zeros_like(rho), rows[:, 15:19], rows[:, 19:22], pso="gl")
    assert np.array_equal(terms["rho_dd"], can["rdd"][:, :2001])


def test_sun_geometry_does_not_read_the_view(oracle, tables, rows):
    """k, bf and tau_ss of the definition are the oracle's own (aux of sailh) whatever tto and psi are"""
    with np.errstate(all="ignore"):
        refl, tran, _ = oracle.prospect_5d(rows[:4, 0:9], tables)
    rho, tau = oracle.pad_leaf(refl, tran)
    aux = oracle.sailh(rho, tau, np.zeros_like(rho), rows[:4, 15:19], rows[:4, 19:22], pso="gl")["aux"]
    k, bf, lidf = pd.sun_geometry(oracle, rows[:4])
    assert np.array_equal(k, aux["k"]) and np.array_equal(bf, aux["bf"]) and np.array_equal(lidf, aux["lidf"])


def test_fcover_exponent_is_volscatt_at_nadir_view(oracle, rows):
    lidf = oracle.calculate_leafangles(rows[:, 16], rows[:, 17])
    d2r = np.pi / 180
    one = np.ones((len(rows), 1))
    tts = rows[:, 19:20]
    _, chi_o, _, _ = oracle.volscatt(np.sin(tts * d2r), np.cos(tts * d2r), 0.0 * one, one, 0.0 * one,
                                     np.sin(pd.LITAB[None, :] * d2r), np.cos(pd.LITAB[None, :] * d2r))
    K = np.sum(chi_o / 1.0 * lidf, axis=1)                  # sailh.py:86, 94 with cos(tto) = 1
    assert np.max(np.abs(pd.fcover_exponent(lidf) - K)) <= 1e-15


def test_values_are_finite_and_span_a_useful_range(oracle, tables, rows):
    p = pd.products_defined(oracle, tables, rows)
    assert tuple(p) == pd.PRODUCT_NAMES
    for n, v in p.items():
        assert v.shape == (192,) and np.isfinite(v).all(), n
    f = p["fAPAR_bs"]
    print("fAPAR_bs: %d rows below 0.3, %d above 0.8, range %.3f ... %.3f" % ((f < 0.3).sum(), (f > 0.8).sum(), f.min(), f.max()))
    assert (f < 0.3).any() and (f > 0.8).any()              # (measured: 7 and 136 rows, 0.119 ... 0.977)


def test_names_match_the_package():
    from spart_amd import _lib
    assert tuple(_lib.PRODUCT_NAMES) == pd.PRODUCT_NAMES
