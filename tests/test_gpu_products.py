"""spart_products / Engine.products / spart_amd.products / lut_products / retrieve(params_cols=[... products ...]) on the MI355X.
Values are compared with the definition (tools/products_defined.py) and with nothing else: no physical limit is asserted --
sailh.py:189 makes the model's isolated canopy non-conservative and the products are defined on it as it is.
Everything else is bit for bit: a row's five values do not depend on the batch, on what the call does not read, on which
outputs are asked for, or on the layer that makes the call.

Measured on one MI355X: the largest |kernel - definition| over the 137 rows of
test_values_against_the_definition is 1.29e-14 (fAPAR_bs), 1.50e-14 (fAPAR_ws), 4.08e-15 (albedo_bs), 4.86e-15 (albedo_ws) and
2.22e-16 (fCover); the test prints them again; the tolerance is 1e-7 absolute on every product."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import retrieve_defined as RD
from helpers.lut_bayes_quantile_calls import bracket_violations
from helpers.lut_calls import eng, torch_mod  # noqa: F401  (fixtures; eng is a context WITHOUT a sensor, nb = 0)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import lut_bayes_defined as bayes_defined  # noqa: E402
import lut_brute_force as bf  # noqa: E402
import products_defined as pd  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = pd.PRODUCT_NAMES
FILL = -7.0
GUARD = 8                 # float64 words behind every output buffer
TOL = 1e-7                # absolute, every product (the issue's bound: 4e-9 x three terms of magnitude <= 1, 8 x margin)


def products_call(torch, eng, cols, outs=NAMES, null_params=(), null_out=False, B=None, ws_bytes=None):
    """One spart_products through ctypes.  ``cols``: (27, n) float64 device tensor; ``outs``: the outputs that are not NULL;
    ``null_params``: parameter columns handed over as NULL; ``B``: the batch size passed in place of n -> (rc, {name: (n + GUARD,)
    buffer, FILL where nothing was written})"""
    from spart_amd import _lib
    n = cols.shape[1]
    B = n if B is None else B
    bufs = {name: torch.full((n + GUARD,), FILL, dtype=torch.float64, device=cols.device) for name in NAMES}
    ptrs = (_lib.vp * _lib.NPARAM)(*[None if i in null_params else cols.data_ptr() + 8 * n * i for i in range(_lib.NPARAM)])
    po = _lib.SpartProductsOut(*[bufs[name].data_ptr() if name in outs else None for name in NAMES])
    need = int(eng.lib.spart_workspace_bytes(eng.ctx, _lib.SPART_F64, B))
    size = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(size, 256), dtype=torch.uint8, device=cols.device)
    rc = eng.lib.spart_products(eng.ctx, B, ptrs, None if null_out else ctypes.byref(po), ws.data_ptr(), ctypes.c_size_t(size), None)
    torch.cuda.synchronize()
    return rc, bufs


def up(torch, P):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(P, dtype=np.float64).T), device="cuda:0")


def run(torch, eng, P, **kw):
    """-> {name: (B,) numpy}; asserts success and intact guard words"""
    rc, bufs = products_call(torch, eng, up(torch, P), **kw)
    assert rc == 0, eng.lib.spart_last_error(None)
    B = len(P)
    for name, b in bufs.items():
        assert bool((b[B:] == FILL).all()), name
    return {name: b[:B].cpu().numpy() for name, b in bufs.items()}


def same(a, b, rows=None):
    for n in NAMES:
        x = a[n] if rows is None else a[n][rows]
        if not (x.shape == b[n].shape and np.array_equal(x.view(np.uint64), b[n].view(np.uint64))):
            return n
    return None


@pytest.fixture(scope="module")
def lhs():
    from spart_amd import workloads
    return workloads.lhs_params(130, "full", seed=7)


@pytest.fixture(scope="module")
def base(torch_mod, eng, lhs):
    return run(torch_mod, eng, lhs)


def edge_rows():
    from spart_amd import workloads
    D = workloads.default_row
    return np.concatenate([D(LAI=1e-6), D(LAI=0.01), D(LAI=8.0), D(tts=0.0), D(tts=60.0), D(LAI=8.0, tts=60.0), D(LAI=1e-6, tts=0.0)])


def test_values_against_the_definition(torch_mod, eng, oracle, tables, lhs, base):
    P = np.concatenate([lhs, edge_rows()])
    assert P.shape == (137, 27)
    got = run(torch_mod, eng, P)
    assert same(got, base, slice(0, 130)) is None
    want = pd.products_defined(oracle, tables, P)
    worst = {n: float(np.max(np.abs(got[n] - want[n]))) for n in NAMES}
    print("max |kernel - definition| over 137 rows:", {n: f"{v:.2e}" for n, v in worst.items()})
    print("rows at LAI = 1e-6:", {n: got[n][[130, 136]] for n in NAMES})
    for n in NAMES:
        assert np.isfinite(got[n]).all() and worst[n] <= TOL, (n, worst[n])


def test_a_nan_parameter_gives_nan(torch_mod, eng, lhs):
    P = lhs[:4].copy()
    P[0, 0], P[1, 9], P[2, 15], P[3, 19] = np.nan, np.nan, np.nan, np.nan        # Cab, soil brightness B, LAI, tts
    got = run(torch_mod, eng, P)
    for r in range(4):
        assert all(np.isnan(got[n][r]) for n in NAMES[:4]), r
    assert np.isnan(got["fCover"][2]) and np.isfinite(got["fCover"][[0, 1, 3]]).all()        # fCover reads LAI, LIDFa, LIDFb


def test_batch_independence_bit_for_bit(torch_mod, eng, lhs, base):
    for r in (0, 63, 64, 129):
        alone = run(torch_mod, eng, lhs[r:r + 1])
        assert same(base, alone, slice(r, r + 1)) is None, r
    moved = lhs.copy()
    for r in (0, 63, 64, 129):
        moved[r] = lhs[17]
    got = run(torch_mod, eng, moved)
    for r in (0, 63, 64, 129):
        assert same(got, {n: base[n][17:18] for n in NAMES}, slice(r, r + 1)) is None, r
    for B in (63, 64, 65):
        assert same(base, run(torch_mod, eng, lhs[:B]), slice(0, B)) is None, B


def test_what_is_not_read_does_not_matter(torch_mod, eng, lhs, base):
    other = lhs.copy()
    rng = np.random.default_rng(5)
    other[:, 20] = rng.uniform(0.0, 75.0, 130)              # tto
    other[:, 21] = rng.uniform(-400.0, 400.0, 130)          # psi
    other[:, 22:26] = rng.uniform(0.1, 2.0, (130, 4)) * (1.0, 1.0, 1.0, 900.0)
    other[:, 26] = 200.0
    assert same(run(torch_mod, eng, other), base) is None
    assert same(run(torch_mod, eng, lhs, null_params=(22, 23, 24, 25, 26)), base) is None


def test_every_output_alone_and_both_kinds_of_context(torch_mod, eng, lhs, base):
    from spart_amd import get_engine
    assert eng.nb == 0
    for name in NAMES:
        rc, bufs = products_call(torch_mod, eng, up(torch_mod, lhs), outs=(name,))
        assert rc == 0
        for other, b in bufs.items():
            if other == name:
                assert np.array_equal(b[:130].cpu().numpy().view(np.uint64), base[name].view(np.uint64)), name
                assert bool((b[130:] == FILL).all()), name
            else:
                assert bool((b == FILL).all()), (name, other)
    sensor = get_engine("Sentinel2A-MSI", 0)
    assert sensor.nb == 13 and same(run(torch_mod, sensor, lhs), base) is None


def test_refusals(torch_mod, eng, lhs):
    cols = up(torch_mod, lhs)

    def refused(code, text, **kw):
        rc, bufs = products_call(torch_mod, eng, cols, **kw)
        msg = eng.lib.spart_last_error(None).decode()
        assert rc == code and text in msg, (kw, rc, msg)
        assert all(bool((b == FILL).all()) for b in bufs.values()), kw
    refused(-1, "null out", null_out=True)
    refused(-1, "every output is null", outs=())
    refused(-1, "params[5] is null", null_params=(5, 9))
    refused(-1, "params[21] is null", null_params=(21, 22))
    refused(-3, "workspace", ws_bytes=64)
    refused(-1, "negative", B=-1)
    rc, bufs = products_call(torch_mod, eng, cols, B=0)                       # an empty batch: nothing launched, nothing written
    assert rc == 0 and all(bool((b == FILL).all()) for b in bufs.values())
    rc, bufs = products_call(torch_mod, eng, cols, B=0, null_out=True)
    assert rc == -1


def test_python_layer(torch_mod, eng, lhs, base):
    import spart_amd
    torch = torch_mod
    cols = up(torch, lhs)
    got = eng.products(cols)
    assert tuple(got) == NAMES and same({n: v.cpu().numpy() for n, v in got.items()}, base) is None
    as_list = eng.products(list(lhs.T[:22]) + [None] * 5, names=["fCover", "albedo_ws"])
    assert list(as_list) == ["fCover", "albedo_ws"]
    for n, v in as_list.items():
        assert v.shape == (130,) and np.array_equal(v.cpu().numpy().view(np.uint64), base[n].view(np.uint64)), n
    mine = torch.full((130,), FILL, dtype=torch.float64, device="cuda:0")
    res = eng.products(cols, names=["fAPAR_ws"], out={"fAPAR_ws": mine})
    assert res["fAPAR_ws"] is mine and np.array_equal(mine.cpu().numpy(), base["fAPAR_ws"])
    with pytest.raises(ValueError):
        eng.products(cols, names=["fAPAR_ws"], out={"fAPAR_ws": mine[:64]})
    host = spart_amd.products(lhs.T, names=["albedo_bs", "fAPAR_bs"])
    assert list(host) == ["albedo_bs", "fAPAR_bs"] and all(isinstance(v, np.ndarray) for v in host.values())
    assert all(np.array_equal(host[n].view(np.uint64), base[n].view(np.uint64)) for n in host)
    scalar = spart_amd.products([float(v) for v in lhs[3]])
    assert all(np.array_equal(scalar[n].view(np.uint64), base[n][3:4].view(np.uint64)) for n in NAMES)


# ------------------------------------------------------------------ the LUT
COLS = ["LAI", "fAPAR_bs", "fCover"]


@pytest.fixture(scope="module")
def lut(torch_mod, tmp_path_factory):
    """a 512-row float64 Sentinel-2A LUT, 23 noisy observations with per-observation weights, and what retrieve gives for
    params_cols=["LAI"] BEFORE products.npy exists"""
    import spart_amd
    from spart_amd import workloads
    path = str(tmp_path_factory.mktemp("products") / "lut")
    P = workloads.lhs_params(512, "full", seed=11)
    spart_amd.generate_lut(P, "Sentinel2A-MSI", path, dtype="float64")
    meta, params, cols = spart_amd.load_lut(path)
    rng = np.random.default_rng(3)
    M = 23
    table = np.asarray(cols["R_TOC"])
    obs = table[rng.integers(0, 512, M)] * (1 + 0.05 * rng.standard_normal((M, table.shape[1])))
    wts = spart_amd.noise_weights(obs, abs_sigma=0.002, rel_sigma=0.05)
    before = {s: spart_amd.retrieve(path, obs, 5, weights=wts, summary=s, params_cols=["LAI"]) for s in ("host", "device")}
    return dict(path=path, P=P, table=table, obs=obs, wts=wts, before=before, meta=dict(meta))


def test_lut_products_files_and_meta(torch_mod, eng, lut):
    import spart_amd
    path = lut["path"]
    first = spart_amd.lut_products(path, chunk=512)
    blob = open(os.path.join(path, "products.npy"), "rb").read()
    for chunk in (200, 1):
        again = spart_amd.lut_products(path, chunk=chunk)
        assert np.array_equal(again.view(np.uint64), first.view(np.uint64)), chunk
        assert open(os.path.join(path, "products.npy"), "rb").read() == blob, chunk
    on_disk = np.load(os.path.join(path, "products.npy"))
    assert on_disk.shape == (512, 5) and on_disk.dtype == np.float64 and np.array_equal(on_disk, first)
    direct = run(torch_mod, eng, lut["P"])
    assert all(np.array_equal(first[:, j].view(np.uint64), direct[n].view(np.uint64)) for j, n in enumerate(NAMES))
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    assert meta.pop("product_names") == list(NAMES) and meta == lut["meta"]


def stacked(lut):
    prod = np.load(os.path.join(lut["path"], "products.npy"))
    both = np.concatenate([lut["P"], prod], axis=1)
    return both[:, [15, 27 + 0, 27 + 4]]


def test_retrieve_over_product_columns(torch_mod, eng, lut):
    import spart_amd
    spart_amd.lut_products(lut["path"])
    path, obs, wts = lut["path"], lut["obs"], lut["wts"]
    table3 = stacked(lut)
    idx, cost = RD.search_defined(lut["table"], obs, 5, wts)
    mean, median, std, count = bf.summarise_defined(table3, idx)
    dev = spart_amd.retrieve(path, obs, 5, weights=wts, summary="device", params_cols=COLS)
    assert dev["names"] == COLS
    for key, want in (("idx", idx), ("cost", cost), ("mean", mean), ("median", median), ("std", std), ("count", count)):
        assert RD.same(dev[key], want), key
    # given out of order: the parameter columns as given, then the product columns as given
    host = spart_amd.retrieve(path, obs, 5, weights=wts, summary="host", params_cols=["fCover", "LAI", "fAPAR_bs"])
    order = [0, 2, 1]
    assert host["names"] == ["LAI", "fCover", "fAPAR_bs"] and RD.same(host["idx"], idx) and RD.same(host["cost"], cost)
    assert RD.same(host["median"], median[:, order])
    for key, want in (("mean", mean), ("std", std)):       # numpy's own order of summation: rounding only
        assert np.allclose(host[key], want[:, order], rtol=1e-12, atol=1e-14), key
    assert RD.same(spart_amd.retrieve(path, obs, 5, weights=wts, summary="host", params_cols=COLS)["median"], median)
    # parameters only: the bits of the call made before products.npy existed
    for s in ("host", "device"):
        now = spart_amd.retrieve(path, obs, 5, weights=wts, summary=s, params_cols=["LAI"])
        assert set(now) == set(lut["before"][s])
        for key, v in lut["before"][s].items():
            assert key == "names" and now[key] == v or RD.same(now[key], v), (s, key)
    # the stream, in chunks of M, 7 and 1
    whole = spart_amd.retrieve_stream(path, obs, 5, weights=wts, params_cols=COLS, chunk=len(obs))
    assert whole["names"] == COLS
    for key in ("mean", "median", "std", "count"):
        assert RD.same(whole[key], dev[key]), key
    for chunk in (7, 1):
        s = spart_amd.retrieve_stream(path, obs, 5, weights=wts, params_cols=COLS, chunk=chunk)
        for key, v in whole.items():
            assert key == "names" and s[key] == v or RD.same(s[key], v), (chunk, key)


def test_posterior_over_product_columns(torch_mod, eng, lut):
    import spart_amd
    spart_amd.lut_products(lut["path"])
    path, obs, wts = lut["path"], lut["obs"], lut["wts"]
    table3 = stacked(lut)
    levels = [0.05, 0.5, 0.95]
    opts = {"cut": 50, "quantiles": levels}
    got = spart_amd.retrieve(path, obs, 5, weights=wts, summary="device", params_cols=COLS, bayes=opts)
    w = np.ascontiguousarray(wts, dtype=np.float64)
    want = bayes_defined.lut_bayes_defined(lut["table"], table3, obs, w, cut=50.0)
    members = bayes_defined.members_defined(lut["table"], obs, w, 50.0)
    assert np.array_equal(got["bayes_count"], want["count"]) and int(want["count"].max()) > 1
    # an ordered sum of n omegas against numpy's, each omega within (4 + cut) 2^-52 of the definition's (the bound of
    # tests/test_gpu_lut_bayes.py): f; every column here is positive, so the mean keeps the relative bound, and the spread is a
    # weighted RMS of differences whose error is f max|x|
    f = 4.0 * ((4.0 + 50.0) * 2.0 ** -52 + 512 * 2.0 ** -53)
    for key in ("sum_w", "ess"):
        assert np.all(np.abs(got["bayes_" + key] - want[key]) <= 4 * f * np.abs(want[key])), key
    assert np.all(np.abs(got["bayes_mean"] - want["mean"]) <= 4 * f * np.abs(want["mean"]))
    assert np.all(np.abs(got["bayes_std"] - want["std"]) <= 4 * f * (np.abs(table3).max(axis=0) + want["std"]))
    assert got["bayes_quantiles"].shape == (len(obs), 3, 3)
    assert bracket_violations(members, table3, got["bayes_quantiles"], levels, 50.0, 1.0) == []
    for chunk in (len(obs), 7, 1):
        s = spart_amd.retrieve_stream(path, obs, 5, weights=wts, params_cols=COLS, chunk=chunk, bayes=opts)
        for key in ("bayes_mean", "bayes_std", "bayes_ess", "bayes_sum_w", "bayes_count", "bayes_quantiles"):
            assert RD.same(s[key], got[key]), (chunk, key)


def test_the_example_runs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "products.py"), "2000", str(tmp_path / "lut")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fAPAR_bs" in r.stdout and "fCover" in r.stdout
