"""spart_lut_topk_obs_weights / Engine.lut_topk with (M, nb) weights on the MI355X: one weight row per observation, a band of
weight zero skipped (the observation may be NaN there); index AND cost bit-equal to the brute force of the defined cost
(tools/lut_brute_force.py), ordered by (cost, row), padded with (-1, +inf); the identities with the shared-weights search."""
import numpy as np
import pytest

from helpers.lut_calls import (bf, eng, hyper_si, spectra, torch_mod,  # noqa: F401  (fixtures)
                               equal_rows_case, lut_call, near_rows_case, tdtype)

pytestmark = pytest.mark.gpu


def obsw(torch, eng, lut, obs, w, k, dtype="float32", ws_bytes=None):
    return lut_call(torch, eng, "spart_lut_topk_obs_weights", lut, obs, k, w, dtype, ws_bytes)


def wide(torch, eng, lut, obs, w, k, dtype):
    rc, idx, cost, _ = lut_call(torch, eng, "spart_lut_topk_wide", lut, obs, k, w, dtype)
    assert rc == 0
    return idx, cost


def check(torch, eng, bf, lut, obs, w, k, dtype="float32"):
    rc, idx, cost, st = obsw(torch, eng, lut, obs, w, k, dtype)
    assert rc == 0, eng.lib.spart_last_error(None)
    ti, tc = bf.brute_force_topk_obs_weights_torch(lut, obs, k, w)
    bad = int((idx != ti).any(dim=1).sum())
    assert torch.equal(idx, ti), (dtype, tuple(lut.shape), k, bad, st)
    assert torch.equal(cost, tc), (dtype, tuple(lut.shape), k, st)
    return st


def masked_weights(torch, g, M, nb, td, obs):
    """weights in [0.5, 2] with ~10 % zeros; NaN / inf written into the observations at the zeroed bands"""
    w = (0.5 + 1.5 * torch.rand((M, nb), generator=g, device="cuda:0", dtype=torch.float64)).to(td)
    zero = torch.rand((M, nb), generator=g, device="cuda:0") < 0.1
    w[zero] = 0
    r = torch.rand((M, nb), generator=g, device="cuda:0")
    obs[zero & (r < 0.4)] = float("nan")
    obs[zero & (r > 0.7)] = float("inf")
    return w.contiguous()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb", [1, 6, 13, 31, 32, 97, 211, 2162])
def test_obs_weights_grid(torch_mod, eng, bf, nb, dtype):
    torch = torch_mod
    td = tdtype(torch, dtype)
    g = torch.Generator(device="cuda:0").manual_seed(nb)
    B, M = (1537, 37) if nb > 300 else (3001, 53)
    lut, obs = near_rows_case(torch, g, B, M, nb, td)
    w = masked_weights(torch, g, M, nb, td, obs)
    for k in (1, 10, 256):
        check(torch, eng, bf, lut, obs, w, k, dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb", [13, 211])
def test_identities(torch_mod, eng, nb, dtype):
    """(I1) every weight row = w: lut_topk(weights=w)'s answer; (I2) zero weight on a band set S: the wide search over the
    columns outside S with the remaining weights -- bit for bit"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    g = torch.Generator(device="cuda:0").manual_seed(200 + nb)
    B, M = 4001, 61
    lut = torch.rand((B, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    lut[100:113] = lut[99]
    obs = (lut[torch.arange(M, device="cuda:0") * 7 % B] + 0.03 * torch.randn((M, nb), generator=g, device="cuda:0",
                                                                            dtype=torch.float64).to(td)).contiguous()
    w = (0.5 + 1.5 * torch.rand((nb,), generator=g, device="cuda:0", dtype=torch.float64)).to(td)
    W = w[None, :].repeat(M, 1).contiguous()
    keep = torch.ones(nb, dtype=torch.bool, device="cuda:0")
    keep[torch.arange(0, nb, 5, device="cuda:0")] = False          # S = every fifth band
    W2 = W.clone()
    W2[:, ~keep] = 0
    obs2 = obs.clone()
    obs2[:, ~keep] = float("nan")
    for k in (1, 10, 256):
        i1, c1 = eng.lut_topk(lut, obs, k, W, dtype)
        i0, c0 = eng.lut_topk(lut, obs, k, w, dtype)
        assert torch.equal(i1, i0) and torch.equal(c1, c0), ("I1", nb, k)
        i2, c2 = eng.lut_topk(lut, obs2, k, W2, dtype)
        iw, cw = wide(torch, eng, lut[:, keep].contiguous(), obs[:, keep].contiguous(), w[keep].contiguous(), k, dtype)
        assert torch.equal(i2, iw) and torch.equal(c2, cw), ("I2", nb, k)
    i, c = eng.lut_nearest(lut, obs, W, dtype)
    i0, c0 = eng.lut_nearest(lut, obs, w, dtype)
    assert torch.equal(i, i0) and torch.equal(c, c0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb", [13, 97])
def test_obs_weights_edges(torch_mod, eng, bf, nb, dtype):
    torch = torch_mod
    td = tdtype(torch, dtype)
    B, M = 2049, 40
    g = torch.Generator(device="cuda:0").manual_seed(5)
    lut = torch.rand((B, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    lut[17] = float("nan")                                  # a NaN row
    lut[30, 2] = float("nan")                               # a row with one NaN entry, in a band some observations mask
    lut[100:113] = lut[99]                                  # 13 equal rows: ties across k = 10
    obs = lut[torch.arange(M, device="cuda:0") * 37 % B].clone()
    w = (0.5 + 1.5 * torch.rand((M, nb), generator=g, device="cuda:0", dtype=torch.float64)).to(td)
    obs[0] = lut[99] + 1e-3
    obs[1] = lut[18]                                        # an exact member next to the NaN row
    obs[2] = lut[30]
    w[2, 2] = 0                                             # row 30's NaN band masked: row 30 still never appears
    w[3] = 0                                                # all weights zero: the first k accepted rows at cost 0
    w[4, 5] = -0.5                                          # negative / NaN / infinite weights: nothing
    w[5, 6] = float("nan")
    w[6, 7] = float("inf")
    obs[7, 3] = float("nan")                                # a non-finite value in an unmasked band: nothing
    obs[8, 4] = float("inf")
    obs[9, 1], w[9, 1] = float("nan"), 0                    # ... but masked it is fine
    w[10, 0] = -0.0                                         # negative zero is zero: a mask
    w = w.contiguous()
    for k in (1, 10, 256):
        rc, idx, cost, st = obsw(torch, eng, lut, obs, w, k, dtype)
        assert rc == 0
        check(torch, eng, bf, lut, obs, w, k, dtype)
        for m in (4, 5, 6, 7, 8):
            assert bool((idx[m] == -1).all()) and bool(torch.isinf(cost[m]).all()), (m, k)
        accepted = [r for r in range(B) if r not in (17, 30)][:k]
        assert idx[3].tolist() == accepted and bool((cost[3] == 0).all())
        assert int(idx[1, 0]) == 18 and float(cost[1, 0]) == 0.0
        assert 17 not in idx.tolist() and 30 not in idx[2].tolist()
        if k >= 10:
            assert idx[0, :10].tolist() == list(range(99, 109))
    # fewer rows than k, and M = 0
    st = check(torch, eng, bf, lut[:40].contiguous(), obs, w, 256, dtype)
    assert st["brute_force"] > 0
    rc, idx, cost, _ = obsw(torch, eng, lut, obs[:0], w[:0], 4, dtype)
    assert rc == 0 and idx.shape == (0, 4)
    i, c = eng.lut_topk(lut, obs[:0], 4, w[:0], dtype)
    assert i.shape == (0, 4)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_obs_weights_fallback_is_exercised(torch_mod, eng, bf, dtype):
    """all rows equal but one: every tile is a candidate, the lists overflow, the brute force decides (and is checked)"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    lut, obs = equal_rows_case(torch, g, td)
    w = masked_weights(torch, g, 9, lut.shape[1], td, obs)
    for k in (1, 10):
        st = check(torch, eng, bf, lut, obs, w, k, dtype)
        assert st["brute_force"] > 0, st


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_filter_settles_noisy_spectra(torch_mod, eng, bf, spectra, dtype):
    """211-band R_TOC spectra, observations = other rows x (1 + 0.02 N(0, 1)), weights noise_weights(rel_sigma = 0.02): the
    filter decides every observation (no brute force) and the answer is exact"""
    from spart_amd import noise_weights
    torch = torch_mod
    td = tdtype(torch, dtype)
    lut = spectra[:3900].to(td).contiguous()
    g = torch.Generator(device="cuda:0").manual_seed(8)
    o = spectra[3900:] * (1 + 0.02 * torch.randn(spectra[3900:].shape, generator=g, device="cuda:0", dtype=torch.float64))
    obs = o.to(td).contiguous()
    w = torch.as_tensor(noise_weights(obs.cpu().numpy(), rel_sigma=0.02), device="cuda:0").to(td).contiguous()
    for k in (1, 10):
        st = check(torch, eng, bf, lut, obs, w, k, dtype)
        assert st["brute_force"] == 0, st
        assert st["nbound"] > 0


def test_obs_weights_64bit_offsets(torch_mod, eng):
    """10.3M x 211 float32 LUT (B nb > 2^31): observations copied from rows past element offset 2^31 come back as those rows
    (the lowest duplicate index) at cost 0, with masked bands holding NaN"""
    torch = torch_mod
    B, nb = 10_300_000, 211
    g = torch.Generator(device="cuda:0").manual_seed(11)
    lut = torch.rand((B, nb), generator=g, device="cuda:0", dtype=torch.float32)
    rows = torch.tensor([10_200_001, 10_250_000, 10_299_998, 10_299_999, 10_260_000], device="cuda:0")
    lut[10_299_999] = lut[10_260_000]
    obs = lut[rows].clone()
    w = torch.ones((5, nb), device="cuda:0")
    w[:, 3] = 0
    obs[:, 3] = float("nan")
    want = torch.tensor([10_200_001, 10_250_000, 10_299_998, 10_260_000, 10_260_000], device="cuda:0")
    rc, idx, cost, st = obsw(torch, eng, lut, obs, w, 2)
    assert rc == 0
    assert torch.equal(idx[:, 0], want), (idx, st)
    assert bool((cost[:, 0] == 0).all())
    assert int(idx[3, 1]) == 10_299_999 and float(cost[3, 1]) == 0.0
    del lut
    torch.cuda.empty_cache()


def test_obs_weights_rejections(torch_mod, eng):
    torch = torch_mod
    lut = torch.rand((100, 2163), device="cuda:0")
    obs = lut[:3].clone()
    w = torch.ones((3, 2163), device="cuda:0")
    assert obsw(torch, eng, lut, obs, w, 1)[0] == -1                        # nb = 2163
    assert eng.lib.spart_lut_topk_obs_weights_workspace_bytes(0, 100, 2163, 3, 1) == 0
    z = torch.empty((100, 0), device="cuda:0")
    assert obsw(torch, eng, z, z[:3], z[:3], 1)[0] == -1                  # nb = 0
    assert eng.lib.spart_lut_topk_obs_weights_workspace_bytes(0, 100, 0, 3, 1) == 0
    lut2, obs2, w2 = lut[:, :2162].contiguous(), obs[:, :2162].contiguous(), w[:, :2162].contiguous()
    assert obsw(torch, eng, lut2, obs2, w2, 0)[0] == -1                    # k = 0
    assert obsw(torch, eng, lut2, obs2, w2, 257)[0] == -1                  # k = 257
    for k in (0, 257):
        assert eng.lib.spart_lut_topk_obs_weights_workspace_bytes(0, 100, 2162, 3, k) == 0
    assert obsw(torch, eng, lut2, obs2, None, 4)[0] == -1                  # NULL weights
    assert obsw(torch, eng, lut2, obs2, w2, 4, ws_bytes=64)[0] == -3       # short workspace
    assert obsw(torch, eng, lut2, obs2, w2, 4)[0] == 0
    with pytest.raises(ValueError, match="weights"):
        eng.lut_topk(lut2, obs2, 4, w2[:2])
    with pytest.raises(ValueError, match="weights"):
        eng.lut_nearest(lut2, obs2, w2[:, :5])


def test_engine_dispatch_and_stats(torch_mod, eng, bf, spectra):
    torch = torch_mod
    lut, obs = spectra[:4000].float().contiguous(), (spectra[4000:] * 1.01).float().contiguous()
    w = torch.rand(obs.shape, device="cuda:0") + 0.5
    before = eng.calls["spart_lut_topk_obs_weights"]
    i, c = eng.lut_nearest(lut, obs, w)
    ti, tc = bf.brute_force_topk_obs_weights_torch(lut, obs, 1, w)
    assert torch.equal(i, ti[:, 0]) and torch.equal(c, tc[:, 0])
    i, c, st = eng.lut_topk(lut, obs, 10, w, stats=True)
    ti, tc = bf.brute_force_topk_obs_weights_torch(lut, obs, 10, w)
    assert torch.equal(i, ti) and torch.equal(c, tc)
    assert set(st) == {"brute_force", "candidate_tiles", "max_candidate_tiles", "nbound"}
    assert eng.calls["spart_lut_topk_obs_weights"] == before + 2


def test_generate_invert_retrieve_end_to_end(torch_mod, bf, hyper_si, tmp_path):
    from spart_amd import noise_weights, workloads
    from spart_amd.lut import generate_lut, invert_lut, load_lut, retrieve, summarise_rows
    torch = torch_mod
    P = workloads.lhs_params(6000, "full", seed=4)
    path = str(tmp_path / "hyper211")
    generate_lut(P, "hyper211", path=path, sensor_info=hyper_si)
    meta, params, cols = load_lut(path)
    table = np.nan_to_num(np.asarray(cols["R_TOC"]), nan=0.5)
    rng = np.random.default_rng(1)
    obs = (table[rng.integers(0, 6000, 50)] * (1 + 0.02 * rng.standard_normal((50, 211)))).astype(np.float32)
    obs[rng.random(obs.shape) < 0.05] = np.nan                 # flagged bands
    W = noise_weights(obs, rel_sigma=0.02)
    L = torch.as_tensor(np.array(cols["R_TOC"]), device="cuda:0")
    O = torch.as_tensor(obs, device="cuda:0")
    Wt = torch.as_tensor(W, device="cuda:0").float()
    idx, cost = invert_lut(path, obs, weights=W, k=10)
    ti, tc = bf.brute_force_topk_obs_weights_torch(L, O, 10, Wt)
    assert np.array_equal(idx, ti.cpu().numpy()) and np.array_equal(cost, tc.cpu().numpy())
    i1, c1 = invert_lut(table, obs, weights=W)                 # in memory, nearest
    ti, tc = bf.brute_force_topk_obs_weights_torch(torch.as_tensor(table, device="cuda:0"), O, 1, Wt)
    assert np.array_equal(i1, ti[:, 0].cpu().numpy()) and np.array_equal(c1, tc[:, 0].cpu().numpy())
    r = retrieve(path, obs, 10, weights=W)
    assert np.array_equal(r["idx"], idx) and np.array_equal(r["cost"], cost)
    for a, b in zip((r["mean"], r["median"], r["std"]), summarise_rows(params, idx)):
        assert np.array_equal(a, b, equal_nan=True)
