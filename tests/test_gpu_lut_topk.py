"""spart_lut_topk / Engine.lut_topk / retrieve on the MI355X: the k nearest LUT rows, index AND cost bit-equal to a brute force
of the defined cost (tools/lut_brute_force.py; its numpy and torch forms agree: tests/test_lut_topk_host.py), ordered by
(cost, row), padded with (-1, +inf)."""
import numpy as np
import pytest

from helpers.lut_calls import bf, eng, lut_call, torch_mod  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KS = (1, 2, 10, 64, 256)


def _check(torch, eng, bf, lut, obs, k, w, dtype, nearest=True):
    L = torch.as_tensor(lut, device="cuda:0")
    O = torch.as_tensor(obs, device="cuda:0")
    W = None if w is None else torch.as_tensor(w, device="cuda:0")
    idx, cost, st = eng.lut_topk(L, O, k, W, dtype, stats=True)
    ti, tc = bf.brute_force_topk_torch(L, O, k, W)
    bad = int((idx != ti).any(dim=1).sum())
    assert torch.equal(idx, ti), (dtype, lut.shape, k, bad)
    assert torch.equal(cost, tc), (dtype, lut.shape, k)
    if nearest:                                        # column 0 is spart_lut_nearest's answer, bit for bit
        i1, c1 = eng.lut_nearest(L, O, W, dtype)
        assert torch.equal(idx[:, 0], i1) and torch.equal(cost[:, 0], c1)
    return idx, cost, st


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb", [1, 6, 13, 21, 31])
def test_topk_matches_brute_force(dtype, nb, torch_mod, eng, bf):
    """every nb class, k in {1, 2, 10, 64, 256}, unweighted and weighted (one zero weight); a NaN row, exact members, and a
    row repeated 12 times that the observations sit on, so that ties straddle the k-th place"""
    rng = np.random.default_rng(1000 + nb)
    B, M = 20_011, 301
    npdt = np.float32 if dtype == "float32" else np.float64
    lut = rng.uniform(0.0, 0.6, (B, nb)).astype(npdt)
    lut[17] = np.nan
    lut[[900, 901, 5000, 5001, 5002, 7000, 9001, 12000, 15000, 19999, 20010]] = lut[450]
    obs = (lut[rng.integers(18, B, M)] + rng.normal(0, 0.01, (M, nb))).astype(npdt)
    obs[:5] = lut[100:105]
    obs[5:10] = lut[450]
    obs[10:12] = lut[450] + npdt(1e-3)
    w = rng.uniform(0.5, 2.0, nb).astype(npdt)
    w[0] = 0.0
    for k in KS:
        for ww in (None, w):
            idx, cost, st = _check(torch_mod, eng, bf, lut, obs, k, ww, dtype)
            assert not (idx == 17).any()
            assert 0 <= st["brute_force"] <= M and np.isfinite(st["nmax"])
            if k == 1 or nb == 1:
                continue
            assert (idx >= 0).all()
            if ww is None and k >= 12:
                assert sorted(idx[5, :12].tolist()) == [450, 900, 901, 5000, 5001, 5002, 7000, 9001, 12000, 15000, 19999, 20010]


def test_topk_edge_cases(torch_mod, eng, bf):
    """an all-NaN LUT (nothing qualifies), B < k (padding), observations with NaN, M = 0, NaN rows everywhere"""
    torch = torch_mod
    rng = np.random.default_rng(5)
    for dtype, npdt in (("float32", np.float32), ("float64", np.float64)):
        lut = rng.uniform(0, 0.6, (3000, 13)).astype(npdt)
        obs = (lut[rng.integers(0, 3000, 50)] + rng.normal(0, 0.01, (50, 13))).astype(npdt)
        obs[3, 4] = np.nan
        obs[4, 0] = np.inf
        idx, cost, _ = _check(torch, eng, bf, np.full_like(lut, np.nan), obs, 10, None, dtype)
        assert (idx == -1).all() and torch.isinf(cost).all()
        idx, cost, _ = _check(torch, eng, bf, lut[:7], obs, 10, None, dtype)            # B < k
        assert (idx[:, 7:] == -1).all() and (idx[[0, 1, 2, 5], :7] >= 0).all()
        assert (idx[3] == -1).all() and (idx[4] == -1).all()
        holes = lut.copy()
        holes[rng.random(3000) < 0.3] = np.nan
        _check(torch, eng, bf, holes, obs, 64, None, dtype)
        _check(torch, eng, bf, holes[:100], obs, 256, None, dtype)                     # fewer rows than k qualify
        i0, c0 = eng.lut_topk(lut, obs[:0], 5, None, dtype)
        assert tuple(i0.shape) == (0, 5) and tuple(c0.shape) == (0, 5)


@pytest.mark.parametrize("dtype,nb", [("float32", 6), ("float32", 13), ("float64", 13)])
def test_topk_exact_on_a_correlated_lut(dtype, nb, torch_mod, eng, bf):
    """tools/lut_invert_rate.py's correlated LUT (4 latent parameters; neighbouring rows are close) with 2 % noise"""
    torch = torch_mod
    rng = np.random.default_rng(200 + nb)
    B, M = 400_000, 2000
    z = rng.uniform(0, 1, (B, 4))
    A, C = rng.normal(0, 1.5, (4, nb)), rng.normal(0, 1.0, (4, nb))
    npdt = np.float32 if dtype == "float32" else np.float64
    lut = (0.03 + 0.5 / (1.0 + np.exp(-(z @ A + (z * z) @ C - 1.0)))).astype(npdt)
    pick = rng.integers(0, B, M)
    obs = (lut[pick] * (1.0 + rng.normal(0, 0.02, (M, nb)))).astype(npdt)
    for k in (10, 64):
        _, _, st = _check(torch, eng, bf, lut, obs, k, None, dtype)
        assert st["brute_force"] <= 0.05 * M, st


@pytest.fixture(scope="module")
def s2_lut(tmp_path_factory, torch_mod):
    import spart_amd
    from spart_amd import workloads
    d = str(tmp_path_factory.mktemp("s2lut") / "lut")
    spart_amd.generate_lut(workloads.lhs_params(400_000, "full", seed=11), "Sentinel2A-MSI", path=d, dtype="float32")
    return d


def test_topk_on_a_sentinel2_lut(s2_lut, torch_mod, eng, bf):
    import spart_amd
    _, _, cols = spart_amd.load_lut(s2_lut)
    lut = np.asarray(cols["R_TOC"])
    rng = np.random.default_rng(3)
    obs = (lut[rng.integers(0, len(lut), 3000)] * (1 + 0.02 * rng.standard_normal((3000, lut.shape[1])))).astype(np.float32)
    for k in (1, 10, 64):
        _check(torch_mod, eng, bf, lut, obs, k, None, "float32")
    idx, cost = spart_amd.invert_lut(s2_lut, obs, k=10)
    i1, c1 = spart_amd.invert_lut(s2_lut, obs)
    assert idx.shape == (3000, 10) and np.array_equal(idx[:, 0], i1) and np.array_equal(cost[:, 0], c1)


def test_retrieve_statistics(s2_lut, torch_mod):
    import spart_amd
    from spart_amd import workloads
    _, params, cols = spart_amd.load_lut(s2_lut)
    lut = np.asarray(cols["R_TOC"])
    rng = np.random.default_rng(4)
    obs = (lut[rng.integers(0, len(lut), 200)] * (1 + 0.01 * rng.standard_normal((200, lut.shape[1])))).astype(np.float32)
    r = spart_amd.retrieve(s2_lut, obs, 16)
    assert r["names"] == list(workloads.PARAM_NAMES) and r["mean"].shape == (200, 27)
    idx, cost = spart_amd.invert_lut(s2_lut, obs, k=16)
    assert np.array_equal(r["idx"], idx) and np.array_equal(r["cost"], cost)
    P = np.asarray(params)
    for m in range(200):
        g = P[idx[m][idx[m] >= 0]]
        np.testing.assert_allclose(r["mean"][m], g.mean(axis=0), rtol=1e-13, atol=1e-13)
        np.testing.assert_array_equal(r["median"][m], np.median(g, axis=0))
        np.testing.assert_allclose(r["std"][m], g.std(axis=0), rtol=1e-11, atol=1e-13)


def test_k10_mean_retrieves_lai_better_than_k1(s2_lut, torch_mod):
    """the reason for top-k: on a held-out seeded Sentinel-2 set with 3 % noise the mean LAI of the 10 nearest rows has a
    smaller median absolute error than the single nearest row's LAI (deterministic: every step is exact)"""
    import spart_amd
    from spart_amd import workloads
    P = workloads.lhs_params(2000, "full", seed=12345)                 # held out: not the LUT's seed
    obs = spart_amd.generate_lut(P, "Sentinel2A-MSI", dtype="float32")["R_TOC"]
    rng = np.random.default_rng(6)
    obs = (obs * (1 + 0.03 * rng.standard_normal(obs.shape))).astype(np.float32)
    lai = workloads.PARAM_NAMES.index("LAI")
    r1 = spart_amd.retrieve(s2_lut, obs, 1)
    r10 = spart_amd.retrieve(s2_lut, obs, 10)
    e1 = np.median(np.abs(r1["mean"][:, lai] - P[:, lai]))
    e10 = np.median(np.abs(r10["mean"][:, lai] - P[:, lai]))
    assert e10 < e1, (e10, e1)


def test_topk_at_size(torch_mod, eng, bf):
    """1M rows x 4096 observations, k = 64, against the torch brute force"""
    torch = torch_mod
    g = torch.Generator("cuda:0").manual_seed(17)
    B, M, nb = 1_000_000, 4096, 13
    lut = torch.rand((B, nb), device="cuda:0", dtype=torch.float32, generator=g)
    pick = torch.randint(0, B, (M,), device="cuda:0", generator=g)
    obs = lut[pick] + 0.01 * torch.randn((M, nb), device="cuda:0", dtype=torch.float32, generator=g)
    idx, cost, st = eng.lut_topk(lut, obs, 64, stats=True)
    ti, tc = bf.brute_force_topk_torch(lut, obs, 64)
    assert torch.equal(idx, ti) and torch.equal(cost, tc), int((idx != ti).any(dim=1).sum())
    assert st["brute_force"] <= 0.01 * M, st


def test_topk_abi_refusals(torch_mod, eng):
    """k outside 1 ... 256, NULL outputs, a workspace that is too small: refused with the documented codes"""
    torch = torch_mod
    lib = eng.lib
    lut = torch.rand((1000, 13), device="cuda:0")
    obs = torch.rand((10, 13), device="cuda:0")
    n = int(lib.spart_lut_topk_workspace_bytes(0, 1000, 13, 10, 8))

    def call(k, **kw):
        return lut_call(torch, eng, "spart_lut_topk", lut, obs, k, **kw)[0]
    assert lib.spart_lut_topk_workspace_bytes(0, 1000, 13, 10, 0) == 0
    assert lib.spart_lut_topk_workspace_bytes(0, 1000, 13, 10, 257) == 0
    assert call(0) == -1 and call(257) == -1
    assert call(8, null=("idx",)) == -1 and call(8, null=("cost",)) == -1
    assert call(8, ws_bytes=n - 1) == -3
    assert call(8) == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        eng.lut_topk(lut, obs, 0)
    with pytest.raises(RuntimeError):
        eng.lut_topk(lut, obs, 257)
    # the workspace rule of the issue: B = 4M, M = 1M, k = 64, nb = 13, float32 within 1 GiB
    assert 0 < lib.spart_lut_topk_workspace_bytes(0, 4_000_000, 13, 1_000_000, 64) <= 1 << 30
