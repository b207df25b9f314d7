"""spart_products without a GPU: the g++ build (-ffp-contract=off) of canopy_flux / products_band
(csrc/spart_products.h through tests/hostmath/products_host.cpp) against canopy_band band by band on the domain grid and
against the numpy definition; the same source as a stand-alone -fsanitize=address,undefined program; header, binding and build
id; and the checks of the Python layer that need no device.

Measured on this CPU build over the 543 rows x 2001 bands of helpers/domain_grid.py (rsd and rdd composed from canopy_flux
against canopy_band's): the largest relative difference is 1.84e-11 (rdd = -4.2e-4, a corner row where the terms cancel; rsd
2.80e-12), and 9.33e-13 on the grid's own metric |d| / max(|ref|, 1e-2).  Only the grouping of three reciprocals differs, so
the test asserts 8 x each figure."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import domain_grid as G

sys.path.insert(0, os.path.join(ROOT, "tools"))
import products_defined as pd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "hostmath", "products_host.cpp")
D = ctypes.POINTER(ctypes.c_double)
MEASURED_REL, MEASURED_GRID = 1.84e-11, 9.33e-13
MARGIN = 8.0


def dp(a):
    return a.ctypes.data_as(D)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("products_host") / "libproducts_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-o", so, SRC])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def tab(lib, tables):
    t = np.zeros((17, 2001))
    args = [np.ascontiguousarray(tables[k], dtype=np.float64)
            for k in ["nr", "nw", "Kab", "Kca", "Kdm", "Kw", "Ks", "Kant", "cbc", "prot", "GSV"]]
    lib.hm_derive_tables(*[dp(a) for a in args], dp(t))
    return t


def bands(lib, tab, P):
    P = np.ascontiguousarray(P, dtype=np.float64)
    out = np.zeros((len(P), 2001, 8))
    lib.ph_bands(ctypes.c_int64(len(P)), dp(tab), dp(P), dp(out))
    return out


def test_canopy_flux_against_canopy_band_on_the_domain_grid(lib, tab):
    P, _ = G.grid_params()
    out = bands(lib, tab, P)
    assert np.isfinite(out).all()
    worst = {}
    for q, name in ((0, "rsd"), (1, "rdd")):
        got, ref = out[:, :, 2 + q], out[:, :, q]
        worst[name] = (float(np.max(np.abs(got - ref) / np.abs(ref))), float(np.max(G.rel(got, ref))))
    print("canopy_flux vs canopy_band over %d rows: (relative, grid metric) %r" % (len(P), worst))
    for name, (r, g) in worst.items():
        assert r <= MARGIN * MEASURED_REL and g <= MARGIN * MEASURED_GRID, (name, r, g)
    # rho_dd itself: the same operations but the grouping of 1 / (a + m) (exactly 0 in both at LAI = 0)
    assert (np.abs(out[:, :, 6] - out[:, :, 7]) <= MARGIN * MEASURED_REL * np.abs(out[:, :, 7])).all()


def test_host_chain_against_the_definition(lib, tab, oracle, tables):
    """the five products from the g++ chain (numpy sums over its per-band terms) against tools/products_defined.py: the 1e-7
    absolute contract of the GPU test, here with the CPU's libm"""
    from spart_amd import workloads
    P = np.ascontiguousarray(workloads.lhs_params(130, "full", seed=7))
    P[:3, 15] = (1e-6, 0.01, 8.0)
    out = bands(lib, tab, P)
    want = pd.products_defined(oracle, tables, P)
    Ea = np.asarray(tables["Ea"], dtype=np.float64)
    got = {"fAPAR_bs": (Ea[:301] * out[:, :301, 4]).sum(1) / Ea[:301].sum(), "fAPAR_ws": (Ea[:301] * out[:, :301, 5]).sum(1) / Ea[:301].sum(),
           "albedo_bs": (Ea * out[:, :, 2]).sum(1) / Ea.sum(), "albedo_ws": (Ea * out[:, :, 3]).sum(1) / Ea.sum()}
    fc = np.zeros(len(P))
    lib.ph_fcover(ctypes.c_int64(len(P)), dp(P), dp(fc))
    got["fCover"] = fc
    for n in pd.PRODUCT_NAMES:
        err = float(np.max(np.abs(got[n] - want[n])))
        print(f"{n}: max |host chain - definition| = {err:.2e}")
        assert err <= 1e-7, n


def test_sanitized_program(tmp_path):
    exe = str(tmp_path / "products_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1", "-DPRODUCTS_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 4 and "WRONG" not in r.stdout and "runtime error" not in r.stderr


def test_header_binding_and_build_id():
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    from spart_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spart_hip.h")).read(), flags=re.S)
    members = re.search(r"typedef struct spart_products_out \{(.*?)\} spart_products_out;", hdr, flags=re.S).group(1)
    assert re.findall(r"\*\s*([a-z_]+)\s*[,;]", members) == [f for f, _ in _lib.SpartProductsOut._fields_]
    assert "spart_products" in _lib.SIGNATURES and len(_lib.SIGNATURES["spart_products"][1]) == 7
    assert int(re.search(r"#define\s+SPART_ABI_VERSION\s+(\d+)", hdr).group(1)) == 14 == _lib.ABI_VERSION
    assert any(os.path.basename(d) == "spart_products.h" for d in build.DEPS)


# ------------------------------------------------------------------ the Python layer, before any device is asked for
def test_product_names_validation_and_order():
    import spart_amd
    from spart_amd.engine import product_names
    assert spart_amd.PRODUCT_NAMES == ("fAPAR_bs", "fAPAR_ws", "albedo_bs", "albedo_ws", "fCover")
    assert product_names(None) == spart_amd.PRODUCT_NAMES
    assert product_names(["fCover", "fAPAR_bs"]) == ("fCover", "fAPAR_bs")
    for bad in (["LAI"], ["fCover", "fCover"], [], "fCover", ["fapar_bs"]):
        with pytest.raises(ValueError):
            product_names(bad)


def test_products_argument_checks_need_no_device():
    import spart_amd
    from spart_amd import workloads
    P = workloads.lhs_params(4, "full", seed=1)
    with pytest.raises(ValueError, match="names"):
        spart_amd.products(P.T, names=["nope"])
    with pytest.raises(ValueError, match=r"\(27, B\)"):
        spart_amd.products(P)                               # (4, 27): rows where columns are expected
    cols = list(P.T)
    with pytest.raises(ValueError, match=r"params\[19\] is None"):
        spart_amd.products(cols[:19] + [None] + cols[20:])
    with pytest.raises(ValueError, match="27 entries"):
        spart_amd.products(cols[:22])
    with pytest.raises(ValueError, match="broadcast"):
        spart_amd.products([np.zeros(3)] + [np.zeros(2)] + cols[2:])


def write_lut(path, rows=6, nb=3, products=False):
    from spart_amd import workloads
    os.makedirs(path)
    rng = np.random.default_rng(0)
    np.save(os.path.join(path, "R_TOC.npy"), rng.uniform(0, 0.5, (rows, nb)))
    np.save(os.path.join(path, "params.npy"), rng.uniform(0, 1, (rows, workloads.NPARAM)))
    if products:
        np.save(os.path.join(path, "products.npy"), rng.uniform(0, 1, (rows, 5)))
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"sensor": "Sentinel2A-MSI", "dtype": "float64", "rows": rows, "columns": ["R_TOC"], "band_model": "centre"}, f)


def test_params_cols_order_and_the_missing_products_file(tmp_path):
    import spart_amd
    from spart_amd import lut as L
    names, cols = L._param_columns(["fCover", "LAI", "fAPAR_bs", "Cab"])
    assert names == ["LAI", "Cab", "fCover", "fAPAR_bs"] and cols == [15, 0, 27 + 4, 27 + 0]
    assert L._param_columns(["LAI", "Cab"]) == (["LAI", "Cab"], [15, 0])
    assert L._param_columns(None)[1] == list(range(27))
    with pytest.raises(ValueError, match="unknown"):
        L._param_columns(["LAI", "fapar"])
    path = str(tmp_path / "lut")
    write_lut(path)
    obs = np.zeros((2, 3))
    for call in (lambda: spart_amd.retrieve(path, obs, 2, params_cols=["LAI", "fCover"]),
                 lambda: spart_amd.retrieve(path, obs, 2, params_cols=["fAPAR_ws"], summary="device"),
                 lambda: spart_amd.retrieve_stream(path, obs, 2, params_cols=["LAI", "albedo_bs"])):
        with pytest.raises(ValueError, match="lut_products"):
            call()


def test_stacked_table_reads_rows_from_both_files(tmp_path):
    from spart_amd import lut as L
    path = str(tmp_path / "lut")
    write_lut(path, products=True)
    _, params, _ = L.load_lut(path)
    assert L._summary_table(path, params, [15, 0]) is params            # parameters only: the table every result came from so far
    t = L._summary_table(path, params, [15, 27 + 4])
    prod = np.load(os.path.join(path, "products.npy"))
    assert t.shape == (6, 32)
    assert np.array_equal(np.asarray(t), np.concatenate([np.asarray(params), prod], axis=1))
    assert np.array_equal(t[np.array([4, 1])], np.concatenate([np.asarray(params)[[4, 1]], prod[[4, 1]]], axis=1))
    mean, median, std = L.summarise_rows(t, np.array([[0, 1, 2], [3, -1, 5]]))
    assert mean.shape == (2, 32) and np.allclose(mean[0, 27:], prod[:3].mean(axis=0), rtol=1e-14, atol=0.0)


def test_lut_products_refuses_a_bad_chunk_before_the_device(tmp_path):
    import spart_amd
    path = str(tmp_path / "lut")
    write_lut(path)
    with pytest.raises(ValueError, match="chunk"):
        spart_amd.lut_products(path, chunk=0)
