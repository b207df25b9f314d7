"""spart_lut_summarise on the MI355X: the raw C ABI against its definition (tools/lut_brute_force.summarise_defined) bit for
bit over the parameter counts, k and the kinds of index it is defined for; its refusals; at size behind a real lut_topk; and
the two callers, retrieve(summary="device") and retrieve_stream.

The out-of-range indices below (B, B + 1, -2, 2^40) are the kernel's DEFINED input: it skips every index outside 0 ... B-1
after a range check and before any address is formed (csrc/spart_lut.h, k_lut_summarise), which is what the cases pin."""
import ctypes
import math

import numpy as np
import pytest

from helpers.lut_calls import bf, eng, torch_mod  # noqa: F401  (fixtures)
from test_lut_summarise_host import assert_within_bounds, same

pytestmark = pytest.mark.gpu

FILL = -7.0         # what summarise_call writes into every output before the call: a refused call leaves it there
NAMES = ("mean", "median", "std", "count")


def summarise_call(torch, eng, params, idx, null=(), **sizes):
    """One spart_lut_summarise through ctypes -> (rc, {name: tensor}).  ``null``: which of params / idx / mean / median / std /
    count to pass as NULL; ``sizes``: B / P / M / k to pass in place of the tensors' own (the refusal cases, which return
    before anything is read)."""
    B, P, M, k = (sizes.get(n, v) for n, v in zip("BPMk", (*params.shape, *idx.shape)))
    out = {n: torch.full((idx.shape[0], params.shape[1]), FILL, dtype=torch.float64, device=params.device) for n in NAMES[:3]}
    out["count"] = torch.full((idx.shape[0],), int(FILL), dtype=torch.int32, device=params.device)
    p = {"params": params, "idx": idx, **out}
    p = {n: None if n in null else t.data_ptr() for n, t in p.items()}
    rc = eng.lib.spart_lut_summarise(eng.ctx, B, P, p["params"], M, k, p["idx"], p["mean"], p["median"], p["std"], p["count"], None)
    torch.cuda.synchronize()
    return rc, out


def untouched(out, names=NAMES):
    return all(bool((out[n] == FILL).all()) for n in names)


def index_case(B, P, k, M, seed):
    """a table with NaN and +-inf entries; indices with a padding suffix of every length (all-padding rows among them),
    padding in the middle, duplicates, and a few values equal to B, B + 1, -2 and 2^40"""
    rng = np.random.default_rng(seed)
    params = rng.normal(0.0, 1.0, (B, P)) * rng.uniform(0.01, 100.0, P)
    params[7, 0], params[8, P - 1], params[9, P // 2], params[10, 0] = np.nan, np.inf, -np.inf, np.inf
    idx = rng.integers(0, B, (M, k)).astype(np.int64)
    for m in range(M):
        L = (m * 7) % (k + 1) if M > 1 else 0
        idx[m, k - L:] = -1
        if m % 3 == 1:
            idx[m, k // 2] = -1                                    # padding in the middle
        if m % 4 == 2 and k >= 2:
            idx[m, 1] = idx[m, 0]                                  # a duplicated row
    bad = np.array([B, B + 1, -2, 1 << 40], dtype=np.int64)
    hit = rng.random((M, k)) < 0.03
    idx[hit] = bad[rng.integers(0, 4, int(hit.sum()))]
    if M > 1:
        idx[M // 2, :] = -1
        idx[M // 2 + 1, :] = bad[np.arange(k) % 4]                 # nothing in range either
    return params, idx


@pytest.mark.parametrize("k", [1, 2, 3, 10, 63, 64, 65, 255, 256])
@pytest.mark.parametrize("P", [1, 5, 27, 32, 33, 64])
def test_summarise_equals_its_definition(torch_mod, eng, bf, P, k):
    torch = torch_mod
    B = 300
    for M in (1, 63, 1000):
        params, idx = index_case(B, P, k, M, 1000 * P + 10 * k + M)
        want = dict(zip(NAMES, bf.summarise_defined(params, idx)))
        if M > 1:
            assert want["count"][M // 2] == 0 and want["count"][M // 2 + 1] == 0 and want["count"].max() > 0
        rc, out = summarise_call(torch, eng, torch.as_tensor(params, device="cuda:0"), torch.as_tensor(idx, device="cuda:0"))
        assert rc == 0, eng.lib.spart_last_error(None)
        for n in NAMES:
            got = out[n].cpu().numpy()
            assert got.dtype == want[n].dtype and same(got, want[n]), (P, k, M, n, int((~((got == want[n]) | (np.isnan(got) & np.isnan(want[n])))).sum()))


def test_null_outputs_leave_the_others_correct(torch_mod, eng, bf):
    torch = torch_mod
    params, idx = index_case(300, 27, 10, 200, 77)
    want = dict(zip(NAMES, bf.summarise_defined(params, idx)))
    pt, it = torch.as_tensor(params, device="cuda:0"), torch.as_tensor(idx, device="cuda:0")
    for null in (("median",), ("mean", "std"), ("count",), ("mean", "median", "std")):
        rc, out = summarise_call(torch, eng, pt, it, null=null)
        assert rc == 0, eng.lib.spart_last_error(None)
        assert untouched(out, null)
        for n in NAMES:
            if n not in null:
                assert same(out[n].cpu().numpy(), want[n]), (null, n)


def test_summarise_refusals(torch_mod, eng):
    torch = torch_mod
    entry = "spart_lut_summarise"
    params = torch.rand((100, 27), device="cuda:0", dtype=torch.float64)
    idx = torch.randint(0, 100, (3, 4), device="cuda:0", dtype=torch.int64)

    def refused(text, **kw):
        rc, out = summarise_call(torch, eng, params, idx, **kw)
        msg = eng.lib.spart_last_error(None).decode()
        assert rc == -1 and text in msg and msg.startswith(entry + ": "), (kw, rc, msg)
        assert untouched(out), kw                                  # nothing was written

    for bad_p in (0, 65):
        refused("bad sizes", P=bad_p)
    for bad_k in (0, 257):
        refused(f"k = {bad_k}, expected 1 <= k <= 256", k=bad_k)
    refused("bad sizes", B=-1)
    refused("bad sizes", M=-1)
    refused("bad sizes", B=2_000_000_001)
    refused("empty table", B=0, M=1)
    refused("null argument", null=("params",))
    refused("null argument", null=("idx",))
    refused("null argument", null=NAMES)
    rc, out = summarise_call(torch, eng, params, idx, M=0)         # nothing to do, no error, the outputs untouched
    assert rc == 0 and untouched(out)
    rc, out = summarise_call(torch, eng, params, idx)
    assert rc == 0 and not untouched(out, ("mean",)) and out["count"].tolist() == [4, 4, 4]


# ---- behind a real search: a generated Sentinel-2A LUT of 1M rows
@pytest.fixture(scope="module")
def s2_lut(tmp_path_factory, torch_mod):
    import spart_amd
    from spart_amd import workloads
    d = str(tmp_path_factory.mktemp("s2sum") / "lut")
    spart_amd.generate_lut(workloads.lhs_params(1_000_000, "full", seed=21), "Sentinel2A-MSI", path=d, dtype="float32")
    return d


def noisy_rows(lut, M, seed, noise=0.02):
    rng = np.random.default_rng(seed)
    return (lut[rng.integers(0, len(lut), M)] * (1 + noise * rng.standard_normal((M, lut.shape[1])))).astype(np.float32)


@pytest.mark.parametrize("k", [10, 64])
def test_summarise_at_size(s2_lut, torch_mod, eng, bf, k):
    """B = 1M, P = 27, M = 65 536 from a real lut_topk: the definition on 512 sampled observations bit for bit, and
    summarise_rows (numpy, another summation order) on all of them within the rounding bounds"""
    import spart_amd
    torch = torch_mod
    _, params, cols = spart_amd.load_lut(s2_lut)
    params = np.asarray(params)
    lut = np.asarray(cols["R_TOC"])
    M = 65536
    obs = noisy_rows(lut, M, 31 + k)
    idx_t, _ = eng.lut_topk(torch.as_tensor(lut, device="cuda:0"), torch.as_tensor(obs, device="cuda:0"), k)
    rc, out = summarise_call(torch, eng, torch.as_tensor(params, device="cuda:0"), idx_t)
    assert rc == 0, eng.lib.spart_last_error(None)
    got = {n: out[n].cpu().numpy() for n in NAMES}
    idx = idx_t.cpu().numpy()
    pick = np.random.default_rng(k).choice(M, 512, replace=False)
    want = dict(zip(NAMES, bf.summarise_defined(params, idx[pick])))
    for n in NAMES:
        assert same(got[n][pick], want[n]), (k, n)
    hm, hmed, hs = spart_amd.lut.summarise_rows(params, idx)
    assert same(got["median"], hmed) and np.array_equal(got["count"], (idx >= 0).sum(axis=1))
    assert_within_bounds(params, idx, got["mean"], got["std"], hm, hs, k)


def test_retrieve_on_the_device_against_the_host(s2_lut, torch_mod):
    import spart_amd
    from spart_amd import workloads
    _, params, cols = spart_amd.load_lut(s2_lut)
    obs = noisy_rows(np.asarray(cols["R_TOC"]), 3000, 41)
    obs[17] = np.nan                                               # matches nothing: count 0, NaN maps on both paths
    for k in (1, 10, 64):
        h = spart_amd.retrieve(s2_lut, obs, k)
        d = spart_amd.retrieve(s2_lut, obs, k, summary="device")
        assert sorted(d) == sorted(list(h) + ["count"]) and d["names"] == h["names"] == list(workloads.PARAM_NAMES)
        assert np.array_equal(d["idx"], h["idx"]) and np.array_equal(d["cost"], h["cost"]) and same(d["median"], h["median"])
        assert d["count"][17] == 0 and np.isnan(d["mean"][17]).all() and np.array_equal(d["count"], (h["idx"] >= 0).sum(axis=1))
        assert_within_bounds(np.asarray(params), h["idx"], d["mean"], d["std"], h["mean"], h["std"], k)
    two = spart_amd.retrieve(s2_lut, obs, 64, summary="device", params_cols=["LAI", "Cab"])
    c = [workloads.PARAM_NAMES.index(n) for n in ("LAI", "Cab")]
    assert two["names"] == ["LAI", "Cab"] and np.array_equal(two["idx"], d["idx"]) and np.array_equal(two["count"], d["count"])
    for n in ("mean", "median", "std"):
        assert two[n].shape == (3000, 2) and same(two[n], d[n][:, c]), n
    th = spart_amd.retrieve(s2_lut, obs, 64, params_cols=["LAI", "Cab"])          # the host path takes the argument too
    assert th["names"] == ["LAI", "Cab"] and all(same(th[n], h[n][:, c]) for n in ("mean", "median", "std"))


def test_engine_lut_summarise_uses_a_resident_table_as_it_is(torch_mod, eng, bf):
    torch = torch_mod
    params, idx = index_case(300, 27, 10, 50, 5)
    pt = torch.as_tensor(params, device="cuda:0")
    before = eng.calls["spart_lut_summarise"]
    res = eng.lut_summarise(pt, idx)
    assert eng.calls["spart_lut_summarise"] == before + 1
    want = dict(zip(NAMES, bf.summarise_defined(params, idx)))
    assert sorted(res) == sorted(NAMES) and all(same(res[n].cpu().numpy(), want[n]) for n in NAMES)
    assert res["count"].dtype == torch.int32 and res["mean"].device == pt.device
    f32 = eng.lut_summarise(params.astype(np.float32), idx)        # converted to float64 on the way in
    want32 = bf.summarise_defined(params.astype(np.float32), idx)
    assert same(f32["mean"].cpu().numpy(), want32[0])
    with pytest.raises(RuntimeError, match="spart_lut_summarise: bad sizes"):
        eng.lut_summarise(torch.zeros((10, 65), device="cuda:0", dtype=torch.float64), idx)


@pytest.mark.parametrize("chunk", [4096, 3333])
def test_retrieve_stream_equals_one_call(s2_lut, torch_mod, chunk):
    import spart_amd
    _, _, cols = spart_amd.load_lut(s2_lut)
    M, k = 10_000, 10
    obs = noisy_rows(np.asarray(cols["R_TOC"]), M, 51)
    rng = np.random.default_rng(52)
    obs[rng.random(obs.shape) < 0.02] = np.nan                     # NaN pixels: masked by the noise weights
    obs[123] = np.nan                                              # (every band masked: all rows cost 0)
    w = spart_amd.noise_weights(obs, abs_sigma=0.002, rel_sigma=0.02)
    w[77, 3] = -1.0                                                # a negative weight: the pixel matches nothing
    one = spart_amd.retrieve(s2_lut, obs, k, weights=w, summary="device")
    e = spart_amd.get_engine(None, None)
    before = dict(e.calls)
    got = spart_amd.retrieve_stream(s2_lut, obs, k, weights=w, chunk=chunk)
    n = math.ceil(M / chunk)
    assert e.calls["spart_lut_topk_obs_weights"] - before.get("spart_lut_topk_obs_weights", 0) == n
    assert e.calls["spart_lut_summarise"] - before.get("spart_lut_summarise", 0) == n
    assert sorted(got) == ["best_cost", "count", "mean", "median", "names", "std"] and got["names"] == one["names"]
    for name in ("mean", "median", "std", "count"):
        assert got[name].dtype == one[name].dtype and same(got[name], one[name]), name
    assert got["best_cost"].dtype == one["cost"].dtype and np.array_equal(got["best_cost"], one["cost"][:, 0])
    assert got["count"][77] == 0 and np.isnan(got["mean"][77]).all() and np.isinf(got["best_cost"][77])
    assert got["count"][123] == k and (got["count"] == k).sum() >= M - 2
    # shared weights and no weights take the other searches; caller-owned arrays are reused
    for ww in (None, np.linspace(0.5, 2.0, obs.shape[1])):
        clean = np.nan_to_num(obs, nan=0.1)
        clean[5] = np.nan                                          # without a mask a NaN pixel matches nothing
        one = spart_amd.retrieve(s2_lut, clean, k, weights=ww, summary="device", params_cols=["LAI"])
        out = {n_: a for n_, a in got.items() if n_ != "names"}
        out = {n_: (np.empty((M, 1)) if a.ndim == 2 else a) for n_, a in out.items()}
        again = spart_amd.retrieve_stream(s2_lut, clean, k, weights=ww, chunk=chunk, params_cols=["LAI"], out=out)
        assert all(again[n_] is out[n_] for n_ in out) and again["count"][5] == 0 and np.isnan(again["median"][5]).all()
        assert all(same(again[n_], one[n_]) for n_ in ("mean", "median", "std", "count"))
        assert np.array_equal(again["best_cost"], one["cost"][:, 0])
