"""The three chunked top-k searches past their first observation chunk, on the MI355X: spart_lut_topk (chunks of 65 536
observations), spart_lut_topk_wide (16 384) and spart_lut_topk_obs_weights (16 384, cut to 7 168 at 2162 bands in float64).
Every case has M = 2 chunks + 37: the second loop iteration (obs + m0 nb, w + m0 nb, the select kernels' m0), a ragged last
chunk shorter than the per-chunk buffers it reuses, the call-wide list of flagged observations and the final brute-force pass
picking up observations flagged in a later chunk.  Index AND cost are compared for bit equality with the torch brute force of
the defined cost (tools/lut_brute_force.py) over ALL observations, and the rows around every chunk boundary with a separate
call on just that slice (position invariance).

Every search here goes through lut_call(guard=True): the workspace is filled with 0xFF bytes first, so a buffer a ragged chunk
under-fills holds NaN patterns rather than the previous chunk's plausible values, and the bytes behind the size the search
asked for must come back untouched.

Wall time on one MI355X: 17 s for the 28 tests of this module (the longest: per-observation weights at 211 bands in float64,
2.7 s; retrieve_stream 2.7 s).  What else was and was not measured: DESIGN.md section 13."""
import numpy as np
import pytest

from helpers.lut_calls import bf, eng, equal_rows_case, lut_call, tdtype, torch_mod  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B_ROWS = 20_011                                    # not a multiple of 32
TIED = [450, 900, 901, 5000, 5001, 5002, 7000, 9001, 12000, 15000, 19999, 20010]       # twelve equal rows
SEARCHES = [("spart_lut_topk", 13), ("spart_lut_topk_wide", 211), ("spart_lut_topk_obs_weights", 13),
            ("spart_lut_topk_obs_weights", 211)]
OBSW = "spart_lut_topk_obs_weights"


def chunk_of(entry, nb, dtype):
    """observations per pass: LUT_TOPK_CHUNK, LUTW_CHUNK, and for per-observation weights LUTW_CHUNK cut to a multiple of
    1024 such that the 2 nbp operand entries per observation (nbp = nb + 1 rounded up to 32) stay within 256 MiB"""
    if entry == "spart_lut_topk":
        return 65_536
    if entry == "spart_lut_topk_wide":
        return 16_384
    nbp = (nb + 1 + 31) // 32 * 32
    fit = (1 << 28) // (2 * nbp * (4 if dtype == "float32" else 8)) // 1024 * 1024
    return max(1024, min(fit, 16_384))


def test_chunk_rule():
    assert chunk_of(OBSW, 2162, "float32") == 15_360 and chunk_of(OBSW, 2162, "float64") == 7_168
    assert chunk_of(OBSW, 211, "float64") == 16_384 and chunk_of(OBSW, 13, "float32") == 16_384


def build(torch, entry, nb, dtype, seed, B=B_ROWS, M=None, hostile=True):
    """-> lut (B, nb), obs (M, nb), w (None, (nb,) or (M, nb)), chunk.  A LUT of uniform [0, 0.6] with a NaN row and twelve
    equal rows; observations = rows + 0.01 N(0, 1), some of them ON the equal rows in every chunk (ties across the k-th place).
    Shared weights (one of them zero) for float64, none for float32; per-observation weights in [0.5, 2] with 10 % masked
    bands, the observation NaN or inf there."""
    td = tdtype(torch, dtype)
    c = chunk_of(entry, nb, dtype)
    M = 2 * c + 37 if M is None else M
    g = torch.Generator(device=DEV).manual_seed(seed)
    lut = (0.6 * torch.rand((B, nb), generator=g, device=DEV, dtype=torch.float64)).to(td)
    if hostile:
        lut[17] = float("nan")
        lut[TIED[1:]] = lut[TIED[0]].clone()
    pick = torch.randint(18, B, (M,), generator=g, device=DEV)
    obs = (lut[pick] + (0.01 * torch.randn((M, nb), generator=g, device=DEV, dtype=torch.float64)).to(td)).contiguous()
    if hostile:
        for m in (0, 1, c - 1, c, c + 3, 2 * c - 1, 2 * c, M - 1):
            obs[m] = lut[TIED[0]]
        obs[2] = lut[TIED[0]] + 1e-3
        obs[M - 2] = lut[TIED[0]] + 1e-3
    w = None
    if entry == OBSW:
        w = (0.5 + 1.5 * torch.rand((M, nb), generator=g, device=DEV, dtype=torch.float64)).to(td)
        zero = torch.rand((M, nb), generator=g, device=DEV) < 0.1
        w[zero] = 0
        r = torch.rand((M, nb), generator=g, device=DEV)
        obs[zero & (r < 0.4)] = float("nan")
        obs[zero & (r > 0.7)] = float("inf")
        w = w.contiguous()
    elif dtype == "float64":
        w = (0.5 + 1.5 * torch.rand((nb,), generator=g, device=DEV, dtype=torch.float64)).to(td)
        w[0] = 0
    return lut, obs, w, c


def search(torch, eng, entry, lut, obs, w, k, dtype):
    rc, idx, cost, st = lut_call(torch, eng, entry, lut, obs, k, w, dtype, guard=True)
    assert rc == 0, (entry, dtype, k, eng.lib.spart_last_error(None))
    return idx, cost, st


def brute(bf, entry, lut, obs, w, k):
    if entry == OBSW:
        return bf.brute_force_topk_obs_weights_torch(lut, obs, k, w)
    return bf.brute_force_topk_torch(lut, obs, k, w)


def rows_of(w, sl):
    return w[sl].contiguous() if w is not None and w.dim() == 2 else w


def boundary_slices(c, M):
    """[c - 100, c + 100) around every chunk boundary, and the ragged tail"""
    n = (M - 1) // c
    return [slice(i * c - 100, i * c + 100) for i in range(1, n + 1)] + [slice(n * c, M)]


def assert_position_invariant(torch, eng, entry, lut, obs, w, k, dtype, c, idx, cost):
    for sl in boundary_slices(c, obs.shape[0]):
        i, co, _ = search(torch, eng, entry, lut, obs[sl].contiguous(), rows_of(w, sl), k, dtype)
        assert torch.equal(i, idx[sl]) and torch.equal(co, cost[sl]), (entry, dtype, k, sl)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("entry,nb", SEARCHES)
def test_two_chunks_and_a_ragged_one(torch_mod, eng, bf, entry, nb, dtype):
    torch = torch_mod
    lut, obs, w, c = build(torch, entry, nb, dtype, 7000 + nb)
    M = obs.shape[0]
    assert M == 2 * c + 37
    ti, tc = brute(bf, entry, lut, obs, w, 256)        # once: by the (cost, row) order its first k columns are the k nearest
    for k in (1, 10, 256):
        idx, cost, st = search(torch, eng, entry, lut, obs, w, k, dtype)
        bad = (idx != ti[:, :k]).any(dim=1) | (cost != tc[:, :k]).any(dim=1)
        where = torch.nonzero(bad).flatten()
        assert not bool(bad.any()), (entry, dtype, k, f"{int(bad.sum())} of {M} observations differ", "first / last",
                                     int(where[0]), int(where[-1]), "per chunk",
                                     [int(bad[i * c:(i + 1) * c].sum()) for i in range(3)], st)
        assert not bool((idx == 17).any()) and 0 <= st["brute_force"] <= M
        if k >= 12 and w is None:
            for m in (0, c, 2 * c, M - 1):
                assert sorted(idx[m, :12].tolist()) == TIED, m
        assert_position_invariant(torch, eng, entry, lut, obs, w, k, dtype, c, idx, cost)
    del ti, tc
    torch.cuda.empty_cache()


def test_position_invariance_against_a_million_rows(torch_mod, eng):
    """no brute force needed: the rows of the whole call around the boundaries equal a call on just those observations"""
    torch = torch_mod
    entry, nb, dtype = "spart_lut_topk", 13, "float32"
    lut, obs, w, c = build(torch, entry, nb, dtype, 99, B=1_000_000, hostile=False)
    for k in (1, 10):
        idx, cost, st = search(torch, eng, entry, lut, obs, w, k, dtype)
        assert bool((idx >= 0).all()) and st["brute_force"] <= 0.01 * obs.shape[0], st
        assert_position_invariant(torch, eng, entry, lut, obs, w, k, dtype, c, idx, cost)
    del lut
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("entry,nb", SEARCHES)
def test_fallback_from_the_last_chunk(torch_mod, eng, bf, entry, nb, dtype):
    """9 605 equal rows inside an ordinary LUT and the nine observations of equal_rows_case on them (every tile of the block
    a candidate: the lists overflow), placed only in the ragged last chunk: flagged there, settled by the brute force after
    the loop, exact -- and the observations of the earlier chunks are what they are without them"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    lut, obs, w, c = build(torch, entry, nb, dtype, 8000 + nb)
    M = obs.shape[0]
    g = torch.Generator(device=DEV).manual_seed(3)
    elut, eobs = equal_rows_case(torch, g, td, nb=nb)
    n, at = eobs.shape[0], 10_000
    lut[at:at + elut.shape[0]] = elut
    plain = obs.clone()
    plain[M - n:] = torch.nan_to_num(obs[100:100 + n], nan=0.3, posinf=0.3)      # the same call without them
    if entry == OBSW:
        w[M - n:] = 1.0                                # (every band of the nine counts)
    obs[M - n:] = eobs
    tail = slice(M - n, M)
    for k in (1, 10):
        idx, cost, st = search(torch, eng, entry, lut, obs, w, k, dtype)
        ti, tc = brute(bf, entry, lut, obs[tail].contiguous(), rows_of(w, tail), k)
        assert torch.equal(idx[tail], ti) and torch.equal(cost[tail], tc), (entry, dtype, k, st)
        assert st["brute_force"] >= n, st
        pidx, pcost, pst = search(torch, eng, entry, lut, plain, w, k, dtype)
        assert torch.equal(idx[:M - n], pidx[:M - n]) and torch.equal(cost[:M - n], pcost[:M - n]), (entry, dtype, k)
        assert st["brute_force"] >= pst["brute_force"]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("entry,nb", SEARCHES)
def test_observations_that_match_nothing_at_the_boundaries(torch_mod, eng, bf, entry, nb, dtype):
    """a non-finite observation, a negative weight row and an all-zero weight row at c - 1, c and M - 1 (each kind at each
    place; the two weight kinds exist with per-observation weights only), checked with their neighbours against the brute force"""
    torch = torch_mod
    lut, obs0, w0, c = build(torch, entry, nb, dtype, 9000 + nb)
    M = obs0.shape[0]
    places = (c - 1, c, M - 1)
    kinds = ("nonfinite", "negative", "zero") if entry == OBSW else ("nonfinite",)
    near = torch.tensor(sorted({m + d for m in places + (2 * c - 1, 2 * c) for d in (-2, -1, 0, 1, 2) if 0 <= m + d < M}), device=DEV)
    for turn in range(len(kinds)):
        obs, w = obs0.clone(), None if w0 is None else w0.clone()
        what = {}
        for i, m in enumerate(places):
            kind = kinds[(i + turn) % len(kinds)]
            what[m] = kind
            if kind == "nonfinite":
                if entry == OBSW:
                    w[m, 1] = 1.0                                          # (an unmasked band)
                obs[m, 1] = float("nan") if i % 2 == 0 else float("inf")
            elif kind == "negative":
                w[m, nb // 2] = -0.5
            else:
                w[m] = 0
        for k in (1, 10):
            idx, cost, st = search(torch, eng, entry, lut, obs, w, k, dtype)
            ti, tc = brute(bf, entry, lut, obs[near].contiguous(), rows_of(w, near), k)
            assert torch.equal(idx[near], ti) and torch.equal(cost[near], tc), (entry, dtype, k, what, st)
            for m, kind in what.items():
                if kind == "zero":                                         # every accepted row costs 0: the first k of them
                    assert idx[m].tolist() == list(range(k)) and bool((cost[m] == 0).all()), (m, kind)
                else:
                    assert bool((idx[m] == -1).all()) and bool(torch.isinf(cost[m]).all()), (m, kind)


def test_cut_chunks_at_2162_bands(torch_mod, eng, bf):
    """per-observation weights at 2162 bands in float64: three chunks of 7 168 / 7 168 / 2 085 observations"""
    torch = torch_mod
    nb, dtype = 2162, "float64"
    lut, obs, w, c = build(torch, OBSW, nb, dtype, 2162, B=1537, M=16_384 + 37, hostile=False)
    assert c == 7168 and obs.shape[0] == 2 * c + 2085
    lut[17] = float("nan")
    lut[100:112] = lut[99]
    for m in (0, c - 1, c, 2 * c - 1, 2 * c, obs.shape[0] - 1):
        obs[m] = lut[99]
        w[m] = 1.0
    k = 10
    idx, cost, st = search(torch, eng, OBSW, lut, obs, w, k, dtype)
    ti, tc = brute(bf, OBSW, lut, obs, w, k)
    bad = (idx != ti).any(dim=1) | (cost != tc).any(dim=1)
    assert not bool(bad.any()), (int(bad.sum()), [int(bad[i * c:(i + 1) * c].sum()) for i in range(3)], st)
    assert idx[c, :10].tolist() == list(range(99, 109))
    assert_position_invariant(torch, eng, OBSW, lut, obs, w, k, dtype, c, idx, cost)
    del lut, obs, w, ti, tc
    torch.cuda.empty_cache()


def test_retrieve_stream_default_chunk(torch_mod, tmp_path):
    """retrieve_stream with its DEFAULT outer chunk (65 536) on 65 536 + 4 097 pixels with per-pixel noise weights and
    NaN-masked bands -- four inner chunks of the obs-weights search per call -- equals retrieve(summary="device") on slices
    of 4 096"""
    import spart_amd
    from spart_amd import workloads
    d = str(tmp_path / "lut")
    spart_amd.generate_lut(workloads.lhs_params(400_000, "full", seed=11), "Sentinel2A-MSI", path=d, dtype="float32")
    _, _, cols = spart_amd.load_lut(d)
    lut = np.asarray(cols["R_TOC"])
    M, k = 65_536 + 4_097, 10
    rng = np.random.default_rng(61)
    obs = (lut[rng.integers(0, len(lut), M)] * (1 + 0.02 * rng.standard_normal((M, lut.shape[1])))).astype(np.float32)
    obs[rng.random(obs.shape) < 0.02] = np.nan                     # masked by the noise weights
    w = spart_amd.noise_weights(obs, abs_sigma=0.002, rel_sigma=0.02)
    for m in (16_383, 16_384, 65_535, 65_536, M - 1):
        w[m, 3] = -1.0                                             # pixels that match nothing, at inner and outer boundaries
    e = spart_amd.get_engine(None, None)
    before = e.calls.get("spart_lut_topk_obs_weights", 0)
    got = spart_amd.retrieve_stream(d, obs, k, weights=w)
    assert e.calls["spart_lut_topk_obs_weights"] - before == 2
    for m0 in range(0, M, 4096):
        sl = slice(m0, min(m0 + 4096, M))
        one = spart_amd.retrieve(d, obs[sl], k, weights=w[sl], summary="device")
        for name in ("mean", "median", "std", "count"):
            assert got[name][sl].dtype == one[name].dtype and np.array_equal(got[name][sl], one[name], equal_nan=True), (name, m0)
        assert np.array_equal(got["best_cost"][sl], one["cost"][:, 0]), m0
    assert (got["count"][[16_383, 16_384, 65_535, 65_536, M - 1]] == 0).all() and (got["count"] == k).sum() >= M - 5
