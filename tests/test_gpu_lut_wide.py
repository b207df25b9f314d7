"""spart_lut_topk_wide / Engine.lut_nearest / lut_topk above 31 bands on the MI355X: the k nearest LUT rows for hyperspectral
nb, index AND cost bit-equal to the brute force of the defined cost (tools/lut_brute_force.py), ordered by (cost, row), padded
with (-1, +inf); for nb <= 31 the wide entry point equals spart_lut_topk / spart_lut_nearest bit for bit."""
import numpy as np
import pytest

from helpers.lut_calls import (bf, eng, hyper_si, spectra, torch_mod,  # noqa: F401  (fixtures)
                               equal_rows_case, lut_call, near_rows_case, tdtype)

pytestmark = pytest.mark.gpu


def wide(torch, eng, lut, obs, k, w=None, dtype="float32", ws_bytes=None):
    return lut_call(torch, eng, "spart_lut_topk_wide", lut, obs, k, w, dtype, ws_bytes)


def check(torch, eng, bf, lut, obs, k, w=None, dtype="float32"):
    rc, idx, cost, st = wide(torch, eng, lut, obs, k, w, dtype)
    assert rc == 0, eng.lib.spart_last_error(None)
    ti, tc = bf.brute_force_topk_torch(lut, obs, k, w)
    bad = int((idx != ti).any(dim=1).sum())
    assert torch.equal(idx, ti), (dtype, tuple(lut.shape), k, bad, st)
    assert torch.equal(cost, tc), (dtype, tuple(lut.shape), k, st)
    return st


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb", [32, 33, 64, 211, 2001, 2162])
def test_wide_grid_uniform(torch_mod, eng, bf, nb, dtype):
    torch = torch_mod
    g = torch.Generator(device="cuda:0").manual_seed(nb)
    B, M = (1537, 53) if nb > 300 else (3001, 71)
    lut, obs = near_rows_case(torch, g, B, M, nb, tdtype(torch, dtype))
    for k in (1, 2, 10, 256):
        check(torch, eng, bf, lut, obs, k, dtype=dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_wide_weights_and_edges(torch_mod, eng, bf, dtype):
    """weights with one zero; a NaN row; exact members; a row repeated so that ties straddle the k-th place"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    nb, B, M = 97, 2049, 40
    g = torch.Generator(device="cuda:0").manual_seed(5)
    lut = torch.rand((B, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    lut[17] = float("nan")
    lut[100:112] = lut[99]                              # 13 equal rows: ties across k = 10
    obs = lut[torch.arange(M, device="cuda:0") * 37 % B].clone()
    obs[0] = lut[99] + 1e-3
    obs[1] = lut[17 + 1]                                 # an exact member next to the NaN row
    obs[2, 5] = float("nan")                             # a non-finite observation: (-1, +inf) everywhere
    w = torch.rand((nb,), generator=g, device="cuda:0", dtype=torch.float64).to(td) + 0.5
    w[3] = 0
    for k in (1, 10, 256):
        check(torch, eng, bf, lut, obs, k, None, dtype)
        check(torch, eng, bf, lut, obs, k, w, dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_wide_on_spectra(torch_mod, eng, bf, spectra, dtype):
    """a LUT of real R_TOC spectra of the 211-band sensor, observations = other rows x (1 + 0.02 N(0, 1))"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    lut = spectra[:3900].to(td).contiguous()
    g = torch.Generator(device="cuda:0").manual_seed(8)
    obs = (spectra[3900:] * (1 + 0.02 * torch.randn(spectra[3900:].shape, generator=g, device="cuda:0",
                                                    dtype=torch.float64))).to(td).contiguous()
    for k in (1, 10, 256):
        st = check(torch, eng, bf, lut, obs, k, dtype=dtype)
        assert st["brute_force"] <= obs.shape[0]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb", [1, 13, 31])
def test_wide_equals_narrow(torch_mod, eng, nb, dtype):
    torch = torch_mod
    td = tdtype(torch, dtype)
    g = torch.Generator(device="cuda:0").manual_seed(100 + nb)
    lut = torch.rand((5003, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    lut[3] = float("nan")
    obs = torch.rand((77, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    w = torch.rand((nb,), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    for k in (1, 10, 256):
        for ww in (None, w):
            rc, idx, cost, _ = wide(torch, eng, lut, obs, k, ww, dtype)
            assert rc == 0
            i2, c2 = eng.lut_topk(lut, obs, k, ww, dtype)
            assert torch.equal(idx, i2) and torch.equal(cost, c2), (nb, k, dtype)
            if k == 1:
                i1, c1 = eng.lut_nearest(lut, obs, ww, dtype)
                assert torch.equal(idx[:, 0], i1) and torch.equal(cost[:, 0], c1)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_wide_fallback_is_exercised(torch_mod, eng, bf, dtype):
    """all rows equal but one: every tile is a candidate, the lists overflow, the brute force decides (and is checked)"""
    torch = torch_mod
    lut, obs = equal_rows_case(torch, torch.Generator(device="cuda:0").manual_seed(3), tdtype(torch, dtype))
    for k in (1, 10):
        st = check(torch, eng, bf, lut, obs, k, dtype=dtype)
        assert st["brute_force"] > 0, st
    # fewer rows than k: found < k, decided by the brute force, padded with (-1, +inf)
    st = check(torch, eng, bf, lut[:100].contiguous(), obs, 256, dtype=dtype)
    assert st["brute_force"] == obs.shape[0], st


def test_wide_64bit_indices(torch_mod, eng):
    """1 000 000 x 2162 float32 LUT (8.6 GB): observations copied from rows past 993 300 (element offsets > 2^31) come back
    as those rows (the lowest duplicate index) at cost 0"""
    torch = torch_mod
    B, nb = 1_000_000, 2162
    g = torch.Generator(device="cuda:0").manual_seed(11)
    lut = torch.rand((B, nb), generator=g, device="cuda:0", dtype=torch.float32)
    rows = torch.tensor([993_301, 995_000, 999_998, 999_999, 996_000], device="cuda:0")
    lut[999_999] = lut[996_000]                          # a duplicate: the lower index wins
    obs = lut[rows].clone()
    want = torch.tensor([993_301, 995_000, 999_998, 996_000, 996_000], device="cuda:0")
    rc, idx, cost, st = wide(torch, eng, lut, obs, 2)
    assert rc == 0
    assert torch.equal(idx[:, 0], want), (idx, st)
    assert bool((cost[:, 0] == 0).all())
    assert int(idx[3, 1]) == 999_999 and float(cost[3, 1]) == 0.0
    i1, c1 = eng.lut_nearest(lut, obs)
    assert torch.equal(i1, want) and bool((c1 == 0).all())
    del lut
    torch.cuda.empty_cache()


def test_wide_rejections(torch_mod, eng):
    torch = torch_mod
    lut = torch.rand((100, 2163), device="cuda:0")
    obs = lut[:3].clone()
    assert wide(torch, eng, lut, obs, 1)[0] == -1                         # nb = 2163: a bad size
    assert eng.lib.spart_lut_topk_wide_workspace_bytes(0, 100, 2163, 3, 1) == 0
    lut2, obs2 = lut[:, :2162].contiguous(), obs[:, :2162].contiguous()
    assert wide(torch, eng, lut2, obs2, 257)[0] == -1                     # k = 257
    assert wide(torch, eng, lut2, obs2, 4, ws_bytes=64)[0] == -3          # short workspace
    assert wide(torch, eng, lut2, obs2, 4)[0] == 0


def test_engine_dispatch_at_211_bands(torch_mod, eng, bf, spectra):
    torch = torch_mod
    lut, obs = spectra[:4000].float().contiguous(), (spectra[4000:] * 1.01).float().contiguous()
    before = eng.calls["spart_lut_topk_wide"]
    i, c = eng.lut_nearest(lut, obs)
    ti, tc = bf.brute_force_torch(lut, obs)
    assert torch.equal(i, ti) and torch.equal(c, tc)
    i, c, st = eng.lut_topk(lut, obs, 10, stats=True)
    ti, tc = bf.brute_force_topk_torch(lut, obs, 10)
    assert torch.equal(i, ti) and torch.equal(c, tc)
    assert set(st) >= {"brute_force", "candidate_tiles", "max_candidate_tiles", "nmax"}
    assert eng.calls["spart_lut_topk_wide"] == before + 2


def test_generate_invert_retrieve_end_to_end(torch_mod, bf, hyper_si, tmp_path):
    from spart_amd import workloads
    from spart_amd.lut import generate_lut, invert_lut, load_lut, retrieve
    torch = torch_mod
    P = workloads.lhs_params(6000, "full", seed=4)
    path = str(tmp_path / "hyper211")
    generate_lut(P, "hyper211", path=path, sensor_info=hyper_si)
    meta, params, cols = load_lut(path)
    assert meta["sensor"] == "hyper211" and len(meta["wavelengths"]) == 211 and meta["bands"][0] == "H400"
    table = np.nan_to_num(np.asarray(cols["R_TOC"]), nan=0.5)      # (a NaN spectrum can never win anyway)
    rng = np.random.default_rng(1)
    obs = (table[rng.integers(0, 6000, 50)] * (1 + 0.02 * rng.standard_normal((50, 211)))).astype(np.float32)
    idx, cost = invert_lut(path, obs, k=10)
    L = torch.as_tensor(np.array(cols["R_TOC"]), device="cuda:0")
    ti, tc = bf.brute_force_topk_torch(L, torch.as_tensor(obs, device="cuda:0"), 10)
    assert np.array_equal(idx, ti.cpu().numpy()) and np.array_equal(cost, tc.cpu().numpy())
    r = retrieve(path, obs, 10)
    assert np.array_equal(r["idx"], idx)
    assert np.allclose(r["mean"], np.asarray(params)[idx].mean(axis=1))
