"""spart_lut_bayes_quantiles / Engine.lut_bayes(quantiles=...) / retrieve(bayes={"quantiles": ...}) on the MI355X: the base
outputs against spart_lut_bayes bit for bit, every quantile against its definition by the bracket property (the exactly rounded
sums of the same omegas, helpers.lut_bayes_quantile_calls.bracket_violations), the exact cases, the filter path against the
brute-force path, batch, chunk and level-order independence, the shapes at which the kernel takes another path, the refusals
and the Python calls."""
import json
import math
import os

import numpy as np
import pytest

from helpers.lut_bayes_calls import FILL, OUTS, bayes_call, defined, noisy_case, same, to_np
from helpers.lut_bayes_quantile_calls import QOUTS, bracket_violations, quant_call, quantiles_want
from helpers.lut_calls import bf, eng, torch_mod, tdtype  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DTYPES = ["float32", "float64"]
INVALID = -1
B0 = 32 * 300 + 5
LEVELS = (0.05, 0.5, 0.95, 0.0, 1.0)          # five: more than one group of levels in the kernel


def run(torch, eng, lut, params, obs, w, dtype, **kw):
    rc, res, st = quant_call(torch, eng, lut, params, obs, w, dtype=dtype, **kw)
    assert rc == 0, eng.lib.spart_last_error(None)
    return res, st


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def check_bracket(res, members, want, params, levels, cut=50.0, tau=1.0, label=""):
    """every (m, p, i) by the bracket property; prints (never asserts) the share equal to the numpy definition's value"""
    got = res["quant"].cpu().numpy()
    share = float(np.mean((got == want) | (np.isnan(got) & np.isnan(want))))
    print(f"{label}: {got.size} quantiles, {100.0 * share:.2f} % equal to the numpy definition's value")
    bad = bracket_violations(members, params, got, levels, cut, tau)
    assert bad == [], bad[:5]


_cases = {}


def case(torch, eng, dtype, nb):
    """test_gpu_lut_bayes' case (B0 rows, 257 observations, noise levels at which the sets within cut = 50 run from a few rows to
    thousands): the plain call, the quantile call on the filter path, the members and the definition, computed once"""
    if (dtype, nb) not in _cases:
        td = tdtype(torch, dtype)
        g = torch.Generator(device="cuda:0").manual_seed(1000 + nb)
        lut, params, obs, w = noisy_case(torch, g, B0, 257, nb, 5, td, rel=0.5, floor=0.55 if nb == 211 else 0.01)
        rc, plain, pst = bayes_call(torch, eng, lut, params, obs, w, dtype=dtype)
        assert rc == 0
        res, st = run(torch, eng, lut, params, obs, w, dtype, levels=LEVELS)
        members, want = quantiles_want(*host(lut, params, obs, w), LEVELS)
        _cases[(dtype, nb)] = (lut, params, obs, w, plain, pst, res, st, members, want)
    return _cases[(dtype, nb)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [13, 211])
def test_base_outputs_and_stats_are_the_plain_calls(torch_mod, eng, nb, dtype):
    _, _, _, _, plain, pst, res, st, _, _ = case(torch_mod, eng, dtype, nb)
    assert same(torch_mod, plain, res) is None
    assert st == pst and st["brute_force"] == 0 and st["candidate_tiles"] > 0, (st, pst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [13, 211])
def test_bracket_property(torch_mod, eng, nb, dtype):
    """every (m, p, i) of the 257 x 5 x 5; q = 0 and q = 1 are the minimum and maximum over the definition's rows; the sets
    include ones larger than the LDS cache holds (682 members) and ones of a few rows"""
    _, params, _, _, _, _, res, _, members, want = case(torch_mod, eng, dtype, nb)
    sizes = [r.size for r, _, _, _ in members]
    assert max(sizes) > 700 and min(sizes) < 64
    par = params.cpu().numpy()
    check_bracket(res, members, want, par, LEVELS, label=f"{dtype} nb={nb}")
    got = res["quant"].cpu().numpy()
    for m, (rows, _, _, _) in enumerate(members):
        assert np.array_equal(got[m, :, 3], par[rows].min(axis=0)) and np.array_equal(got[m, :, 4], par[rows].max(axis=0)), m
    assert (got[:, :, 3] <= got[:, :, 0]).all() and (got[:, :, 0] <= got[:, :, 1]).all() and (got[:, :, 1] <= got[:, :, 2]).all()
    assert (got[:, :, 2] <= got[:, :, 4]).all()                            # non-decreasing in q


@pytest.mark.parametrize("dtype", DTYPES)
def test_unique_minimum_gives_the_best_row(torch_mod, eng, dtype):
    """cut = 0 with a unique minimum (test_gpu_lut_bayes.test_boundary's nb = 1 LUT): every quantile is params[best_idx]"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    npdt = np.float32 if dtype == "float32" else np.float64
    two = npdt(2.0)
    rows = [npdt(0.0), two, np.nextafter(two, npdt(3.0)), npdt(2.5), npdt(3.0)] + [npdt(5.0 + i) for i in range(70)]
    lut = torch.as_tensor(np.array(rows, dtype=npdt)[:, None], device="cuda:0")
    params = torch.arange(1.0, lut.shape[0] + 1, dtype=torch.float64, device="cuda:0")[:, None].repeat(1, 3).contiguous()
    params[:, 1] = params[:, 0] * math.pi
    obs = torch.zeros((1, 1), dtype=td, device="cuda:0")
    w = torch.ones((1, 1), dtype=td, device="cuda:0")
    for bfc in (0, 1):
        res, _ = run(torch, eng, lut, params, obs, w, dtype, cut=0.0, brute_force=bfc, levels=(0.0, 0.3, 0.5, 1.0))
        assert res["count"].tolist() == [1] and res["best_idx"].tolist() == [0]
        assert torch.equal(res["quant"][0], params[0][:, None].expand(3, 4))
        # cut = 4: rows 0 and 1 (x = 1 and 2) with omega 1 and exp(-2): F(1) = 1 reaches half of 1.135 but not all of it
        res, _ = run(torch, eng, lut, params, obs, w, dtype, cut=4.0, brute_force=bfc, levels=(0.0, 0.5, 1.0))
        assert res["count"].tolist() == [2] and res["quant"][0, 0].tolist() == [1.0, 1.0, 2.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_unit_weights_give_the_sorted_rank(torch_mod, eng, dtype):
    """all-zero weights (omega = 1, every sum an exact integer) and dyadic levels: sort(x)[max(ceil(q n) - 1, 0)] over every
    accepted row, through the brute-force kernel (B = 40 005, one NaN LUT row: test_overflow_to_brute_force's case)"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    B, nb, M = 40_005, 5, 8
    g = torch.Generator(device="cuda:0").manual_seed(21)
    lut, params, obs, w = noisy_case(torch, g, B, M, nb, 3, td, rel=0.5)
    lut[777, 2] = float("nan")                                            # one row that is never accepted
    obs[0, 1] = float("nan")                                              # (masked: allowed)
    levels = (0.0, 0.25, 0.5, 0.75, 1.0)
    res, st = run(torch, eng, lut, params, obs, torch.zeros_like(w), dtype, cut=0.0, levels=levels)
    assert st["brute_force"] == M and res["count"].tolist() == [B - 1] * M
    x = np.sort(np.delete(params.cpu().numpy(), 777, axis=0), axis=0)
    n = B - 1
    want = np.stack([x[max(math.ceil(q * n) - 1, 0)] for q in levels], axis=1)
    got = res["quant"].cpu().numpy()
    for m in range(M):
        assert np.array_equal(got[m], want), m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [13, 211])
def test_path_batch_and_level_order_independence(torch_mod, eng, nb, dtype):
    torch = torch_mod
    lut, params, obs, w, _, _, res, _, _, _ = case(torch, eng, dtype, nb)
    sub = torch.arange(0, 257, 16, device="cuda:0")                       # (the brute force over 17 observations: seconds)
    o17, w17 = obs[sub].contiguous(), w[sub].contiguous()
    part, _ = run(torch, eng, lut, params, o17, w17, dtype, levels=LEVELS)
    assert same(torch, res, part, rows=sub, names=QOUTS) is None          # inside a batch of 257 or of 17
    brute, st = run(torch, eng, lut, params, o17, w17, dtype, levels=LEVELS, brute_force=1)
    assert st["brute_force"] == sub.numel() and st["candidate_tiles"] == 0
    assert same(torch, part, brute, names=QOUTS) is None
    one, _ = run(torch, eng, lut, params, obs[100:101].contiguous(), w[100:101].contiguous(), dtype, levels=LEVELS)       # M = 1
    assert same(torch, res, one, rows=slice(100, 101), names=QOUTS) is None
    # the same levels in another order, and one repeated
    perm, _ = run(torch, eng, lut, params, o17, w17, dtype, levels=(1.0, 0.95, 0.05, 0.5, 0.5, 0.0))
    assert torch.equal(perm["quant"][:, :, [2, 3, 1, 5, 0]], part["quant"]) and torch.equal(perm["quant"][:, :, 3], perm["quant"][:, :, 4])
    assert same(torch, part, perm) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks(torch_mod, eng, dtype):
    """M = chunk + 37 against its slices (test_gpu_lut_bayes.test_chunks' case): the observation's chunk does not matter"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    chunk, B, nb = 16_384, 4101, 5
    g = torch.Generator(device="cuda:0").manual_seed(77)
    lut, params, obs, w = noisy_case(torch, g, B, chunk + 37, nb, 3, td, rel=0.3)
    res, st = run(torch, eng, lut, params, obs, w, dtype, cut=12.0, levels=(0.05, 0.5, 0.95))
    assert st["brute_force"] == 0
    for lo, hi in ((0, 37), (chunk - 5, chunk + 37), (chunk, chunk + 37)):
        part, _ = run(torch, eng, lut, params, obs[lo:hi].contiguous(), w[lo:hi].contiguous(), dtype, cut=12.0, levels=(0.05, 0.5, 0.95))
        assert same(torch, res, part, rows=slice(lo, hi), names=QOUTS) is None, (lo, hi)
    assert int(res["count"].max()) > 1 and not bool(torch.isnan(res["quant"]).any())
    lo, hi = chunk - 5, chunk + 37                                        # ... and those rows against the definition
    members, want = quantiles_want(*host(lut, params, obs[lo:hi], w[lo:hi]), (0.05, 0.5, 0.95), cut=12.0)
    check_bracket({"quant": res["quant"][lo:hi]}, members, want, params.cpu().numpy(), (0.05, 0.5, 0.95), cut=12.0, label=f"{dtype} chunk edge")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,levels", [(1, (0.5,)), (27, (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 0.5)), (64, (0.05, 0.5, 0.95))])
def test_hostile_inputs_and_parameter_counts(torch_mod, eng, bf, P, levels, dtype):
    """test_gpu_lut_bayes.test_hostile_inputs' case -- a NaN row, a row whose norm overflows, invalid observations between valid
    ones, one observation with every band masked -- at P = 1 / 27 / 64 and nq = 1 / 8 / 3"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    B, nb, M = 32 * 40 + 7, 6, 11
    g = torch.Generator(device="cuda:0").manual_seed(40 + P)
    lut, params, obs, w = noisy_case(torch, g, B, M, nb, P, td, rel=0.5)
    lut[5, 3] = float("nan")
    lut[B - 1, 0] = 1e30 if dtype == "float32" else 1e200                 # its centred norm overflows: rejected
    clean_w, clean_obs = w.clone(), obs.clone()
    w[2, 1] = -1.0
    w[4] = 0                                                              # every band masked: every accepted row, omega = 1
    obs[4] = float("nan")
    obs[6, 0] = float("inf")
    w[8, 5] = float("nan")
    res, _ = run(torch, eng, lut, params, obs, w, dtype, levels=levels)
    rc, plain, _ = bayes_call(torch, eng, lut, params, obs, w, dtype=dtype)
    assert rc == 0 and same(torch, plain, res) is None
    got = res["quant"].cpu().numpy()
    assert got.shape == (M, P, len(levels))
    for m in (2, 6, 8):                                                   # invalid observations: NaN beside the empty outputs
        assert np.isnan(got[m]).all() and int(res["count"][m]) == 0
    par = params.cpu().numpy()
    rows = np.array([r for r in range(B) if r not in (5, B - 1)])
    assert np.array_equal(got[4], defined.quantiles_of_members(par[rows], np.ones(rows.size), levels))   # omega = 1: exact
    good = torch.tensor([0, 1, 3, 5, 7, 9, 10], device="cuda:0")
    row_ok = bf.norm_rule_numpy(lut.cpu().numpy(), np.full(nb, 0.5))
    members, want = quantiles_want(*host(lut, params, clean_obs[good], clean_w[good]), levels, row_ok=row_ok)
    check_bracket({"quant": res["quant"][good]}, members, want, par, levels, label=f"{dtype} P={P}")
    alone, _ = run(torch, eng, lut, params, clean_obs[good].contiguous(), clean_w[good].contiguous(), dtype, levels=levels)
    assert same(torch, res, alone, rows=good, names=QOUTS) is None        # no neighbour's output changed
    # quant = NULL with other outputs given: the plain call; only quant asked for: the others stay as they were
    rc, some, _ = quant_call(torch, eng, lut, params, obs, w, dtype=dtype, levels=levels, outs=("mean", "count"))
    assert rc == 0 and same(torch, res, some, names=("mean", "count")) is None
    assert all(bool((some[n] == FILL).all()) for n in QOUTS if n not in ("mean", "count"))
    rc, some, _ = quant_call(torch, eng, lut, params, obs, w, dtype=dtype, levels=levels, outs=("quant",))
    assert rc == 0 and same(torch, res, some, names=("quant",)) is None
    assert all(bool((some[n] == FILL).all()) for n in OUTS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sets_of_1_64_and_65_rows(torch_mod, eng, dtype):
    """nb = 1, obs 0, w 1, lut[b] = b / 8: the cost b^2 / 64 is exact, so cut = ((n - 1) / 8)^2 holds exactly n rows"""
    torch = torch_mod
    td = tdtype(torch, dtype)
    B = 200
    g = torch.Generator(device="cuda:0").manual_seed(9)
    lut = (torch.arange(B, device="cuda:0", dtype=torch.float64) / 8.0).to(td)[:, None].contiguous()
    params = (8.0 * torch.rand((B, 3), generator=g, device="cuda:0", dtype=torch.float64)).contiguous()
    obs = torch.zeros((1, 1), dtype=td, device="cuda:0")
    w = torch.ones((1, 1), dtype=td, device="cuda:0")
    for n in (1, 64, 65):
        cut = ((n - 1) / 8.0) ** 2
        members, want = quantiles_want(*host(lut, params, obs, w), LEVELS, cut=cut)
        assert members[0][0].tolist() == list(range(n))
        for bfc in (0, 1):
            res, _ = run(torch, eng, lut, params, obs, w, dtype, cut=cut, brute_force=bfc, levels=LEVELS)
            assert res["count"].tolist() == [n]
            check_bracket(res, members, want, params.cpu().numpy(), LEVELS, cut=cut, label=f"{dtype} n={n} brute_force={bfc}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_duplicate_infinite_and_nan_columns(torch_mod, eng, dtype):
    """columns: random / constant / few distinct values / +inf and -inf entries / one NaN inside S of observation 0 / random.
    The NaN makes exactly the (m, 4) whose set holds that row NaN; its neighbours are untouched."""
    torch = torch_mod
    td = tdtype(torch, dtype)
    g = torch.Generator(device="cuda:0").manual_seed(5)
    lut, params, obs, w = noisy_case(torch, g, 2053, 33, 6, 6, td, rel=0.5)
    members = defined.members_defined(*host(lut, obs, w), 50.0)
    params[:, 1] = 2.5
    params[:, 2] = torch.round(params[:, 2] / 2.0)                        # 0 ... 4
    params[::7, 3] = float("inf")
    params[3::11, 3] = float("-inf")
    nan_row = members[0][2]                                               # the best row of observation 0: in its set
    clean = params.clone()
    params[nan_row, 4] = float("nan")
    levels = (0.05, 0.5, 0.95)
    for bfc in (0, 1):
        res, _ = run(torch, eng, lut, params, obs, w, dtype, levels=levels, brute_force=bfc)
        want = defined.lut_bayes_quantiles_defined(*host(lut, params, obs, w), levels, members=members)
        check_bracket(res, members, want, params.cpu().numpy(), levels, label=f"{dtype} brute_force={bfc}")
        got = res["quant"].cpu().numpy()
        hit = np.array([nan_row in r for r, _, _, _ in members])
        assert hit[0] and np.isnan(got[hit, 4]).all() and not np.isnan(got[~hit, 4]).any()
        assert not np.isnan(got[:, [0, 1, 2, 3, 5]]).any() and (got[:, 1] == 2.5).all()
        assert np.isin(got[:, 2], [0.0, 1.0, 2.0, 3.0, 4.0]).all() and np.isinf(got[:, 3]).any()
        ref, _ = run(torch, eng, lut, clean, obs, w, dtype, levels=levels, brute_force=bfc)
        assert torch.equal(ref["quant"][:, [0, 1, 2, 3, 5]], res["quant"][:, [0, 1, 2, 3, 5]])
        assert torch.equal(ref["quant"][torch.as_tensor(~hit, device="cuda:0")], res["quant"][torch.as_tensor(~hit, device="cuda:0")])


def test_refusals(torch_mod, eng):
    """each new refusal leaves FILL in every output; the older ones are spart_lut_bayes' (spot-checked)"""
    torch = torch_mod
    g = torch.Generator(device="cuda:0").manual_seed(1)
    lut, params, obs, w = noisy_case(torch, g, 500, 4, 7, 3, torch.float32)
    nan = float("nan")
    bad = [dict(levels=(), nq=0), dict(levels=(0.5,) * 9), dict(levels=(0.5,), nq=9), dict(levels=(0.5,), nq=-1),
           dict(levels=None, nq=3), dict(levels=(0.5, -0.1, 2.0)), dict(levels=(0.5, 1.000001)), dict(levels=(0.5, nan)),
           dict(outs=()), dict(opt=False), dict(null=("out",)), dict(cut=-1.0), dict(temperature=nan), dict(brute_force=2),
           dict(P=65), dict(dt=2), dict(null=("lut",))]
    for kw in bad:
        rc, res, _ = quant_call(torch, eng, lut, params, obs, w, **kw)
        assert rc == INVALID, kw
        assert all(bool((t == FILL).all()) for t in res.values()), kw       # nothing was written
    rc, _, _ = quant_call(torch, eng, lut, params, obs, w, levels=(0.5, -0.1, 2.0))
    assert rc == INVALID and b"levels[1]" in eng.lib.spart_last_error(None)  # the first offending index
    rc, res, _ = quant_call(torch, eng, lut, params, obs, w, ws_bytes=1000)
    assert rc == -3 and all(bool((t == FILL).all()) for t in res.values())
    # quant = NULL with other outputs given is accepted: the plain call
    rc, res, st = quant_call(torch, eng, lut, params, obs, w, outs=OUTS)
    rc2, plain, pst = bayes_call(torch, eng, lut, params, obs, w)
    assert rc == 0 and rc2 == 0 and same(torch, plain, res) is None and st == pst and bool((res["quant"] == FILL).all())
    # levels at the ends of the range, unsorted, repeated: accepted
    rc, res, _ = quant_call(torch, eng, lut, params, obs, w, levels=(1.0, 0.0, 0.0, 1.0))
    assert rc == 0 and torch.equal(res["quant"][:, :, 0], res["quant"][:, :, 3]) and not bool(torch.isnan(res["quant"]).any())
    # M = 0 launches nothing; B = 0 writes NaN beside the empty-observation outputs
    rc, res, _ = quant_call(torch, eng, lut, params, obs[:0], w[:0])
    assert rc == 0
    rc, res, _ = quant_call(torch, eng, lut[:0], params[:0], obs, w)
    assert rc == 0 and bool(torch.isnan(res["quant"]).all()) and res["quant"].shape == (4, 3, 3)
    assert res["count"].tolist() == [0] * 4 and res["best_idx"].tolist() == [-1] * 4 and bool(torch.isnan(res["mean"]).all())


def test_engine_call(torch_mod, eng):
    """Engine.lut_bayes(quantiles=...) = the raw call; without it today's call, keys and counter; bad levels raise before any
    GPU work"""
    torch = torch_mod
    g = torch.Generator(device="cuda:0").manual_seed(2)
    lut, params, obs, w = noisy_case(torch, g, 1500, 9, 7, 3, torch.float32, rel=0.5)
    raw, _ = run(torch, eng, lut, params, obs, w, "float32", levels=(0.05, 0.5, 0.95))
    before = dict(eng.calls)
    a = eng.lut_bayes(lut, params, obs, weights=w, quantiles=[0.05, 0.5, 0.95])
    assert sorted(a) == sorted(OUTS + ("quantiles",)) and a["quantiles"].shape == (9, 3, 3) and a["quantiles"].dtype == torch.float64
    assert torch.equal(a["quantiles"], raw["quant"]) and same(torch, a, raw) is None
    assert eng.calls["spart_lut_bayes_quantiles"] == before.get("spart_lut_bayes_quantiles", 0) + 1
    assert eng.calls["spart_lut_bayes"] == before.get("spart_lut_bayes", 0)
    b, st = eng.lut_bayes(lut, params, obs, weights=w, quantiles=np.array([0.5]), brute_force=True, stats=True)
    assert torch.equal(b["quantiles"][:, :, 0], raw["quant"][:, :, 1]) and st["brute_force"] == 9
    plain = eng.lut_bayes(lut, params, obs, weights=w)
    assert sorted(plain) == sorted(OUTS) and same(torch, plain, raw) is None
    assert eng.calls["spart_lut_bayes"] == before.get("spart_lut_bayes", 0) + 1
    none = eng.lut_bayes(lut, params, obs[:0], quantiles=(0.5, 0.9))
    assert none["quantiles"].shape == (0, 3, 2)
    empty = eng.lut_bayes(lut[:0], params[:0], obs, quantiles=(0.5, 0.9))
    assert bool(torch.isnan(empty["quantiles"]).all()) and empty["quantiles"].shape == (9, 3, 2)
    calls = dict(eng.calls)
    for q in ([], [0.5] * 9, [1.5], [-0.01], [float("nan")], 0.5, "median", [None]):
        with pytest.raises(ValueError):
            eng.lut_bayes(lut, params, obs, quantiles=q)
    assert dict(eng.calls) == calls


def write_lut(path, lut, params, dtype):
    os.makedirs(path)
    np.save(os.path.join(path, "R_TOC.npy"), lut)
    np.save(os.path.join(path, "params.npy"), params)
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"sensor": "Sentinel2A-MSI", "dtype": dtype, "rows": int(lut.shape[0]), "columns": ["R_TOC"],
                   "band_model": "centre"}, f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_retrieve_and_retrieve_stream(torch_mod, eng, tmp_path, dtype):
    """bayes={"quantiles": ...}: bayes_quantiles = Engine.lut_bayes' on the same tensors, from retrieve and from retrieve_stream
    at two chunk sizes; every other key as without; without "quantiles" exactly today's keys"""
    import spart_amd
    from spart_amd import workloads
    torch = torch_mod
    npdt = np.float32 if dtype == "float32" else np.float64
    rng = np.random.default_rng(6)
    B, nb, M = 700, 13, 23
    lut = rng.uniform(0.0, 0.6, (B, nb)).astype(npdt)
    params = rng.uniform(0.0, 8.0, (B, workloads.NPARAM))
    obs = (lut[rng.integers(0, B, M)] * (1 + 0.2 * rng.standard_normal((M, nb)))).astype(npdt)
    obs[3, 4] = np.nan                                                    # a masked band
    wts = spart_amd.noise_weights(obs, abs_sigma=0.01, rel_sigma=0.3)
    path = str(tmp_path / "lut")
    write_lut(path, lut, params, dtype)
    cols = ["LAI", "Cab", "Cw"]
    ci = [workloads.PARAM_NAMES.index(n) for n in cols]
    opts = {"cut": 20.0, "temperature": 1.5}
    qopts = {**opts, "quantiles": [0.05, 0.5, 0.95]}
    today = {"bayes_mean", "bayes_std", "bayes_ess", "bayes_sum_w", "bayes_count"}
    want = eng.lut_bayes(lut, params[:, ci], obs, weights=torch.as_tensor(wts.astype(npdt)), dtype=dtype, **qopts)
    assert int(want["count"].max()) > 1 and not bool(torch.isnan(want["quantiles"]).any())
    base = spart_amd.retrieve(path, obs, 5, weights=wts, summary="device", params_cols=cols)
    plain = spart_amd.retrieve(path, obs, 5, weights=wts, summary="device", params_cols=cols, bayes=opts)
    got = spart_amd.retrieve(path, obs, 5, weights=wts, summary="device", params_cols=cols, bayes=qopts)
    assert set(plain) - set(base) == today and set(got) - set(plain) == {"bayes_quantiles"}
    for key, v in plain.items():
        assert key == "names" and got[key] == v or np.array_equal(got[key], v, equal_nan=True), key
    assert got["bayes_quantiles"].shape == (M, 3, 3) and got["bayes_quantiles"].dtype == np.float64
    assert np.array_equal(got["bayes_quantiles"], want["quantiles"].cpu().numpy())
    splain = spart_amd.retrieve_stream(path, obs, 5, weights=wts, params_cols=cols, bayes=opts)
    assert set(splain) - set(spart_amd.retrieve_stream(path, obs, 5, weights=wts, params_cols=cols)) == today
    for chunk in (7, M):
        s = spart_amd.retrieve_stream(path, obs, 5, weights=wts, params_cols=cols, chunk=chunk, bayes=qopts)
        assert set(s) - set(splain) == {"bayes_quantiles"}
        for key, v in splain.items():
            assert key == "names" and s[key] == v or np.array_equal(s[key], v, equal_nan=True), (chunk, key)
        assert np.array_equal(s["bayes_quantiles"], got["bayes_quantiles"]), chunk
