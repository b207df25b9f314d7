"""The k nearest LUT rows without a GPU: the merge rule of per-shard top-k lists (sharding.select_nearest_k), the sharded
search under gloo with a numpy brute force standing in for the device search, invert_lut(shard=False) under an initialised
process group (no collective), the two brute-force checkers, and the parameter summary of retrieve()."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
INF = float("inf")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _load(name):
    import importlib.util
    p = os.path.join(ROOT, "spart-python_amd", "spart_amd", name + ".py")
    spec = importlib.util.spec_from_file_location("_" + name, p)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bf():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lut_brute_force
    return lut_brute_force


def _reference_merge(costs, idxs, k):
    """the definition: the stable argsort by (cost, row) of the union of the finite entries"""
    W, M, _ = costs.shape
    out_i = np.full((M, k), -1, dtype=np.int64)
    out_c = np.full((M, k), np.inf, dtype=costs.dtype)
    for m in range(M):
        ent = sorted((float(c), int(i)) for c, i in zip(costs[:, m].ravel(), idxs[:, m].ravel()) if i >= 0 and np.isfinite(c))
        for p, (c, i) in enumerate(ent[:k]):
            out_i[m, p], out_c[m, p] = i, c
    return out_i, out_c


def test_select_nearest_k_rules():
    sh = _load("sharding")
    # obs 0: a tie inside shard 0 (rows 3, 9) and across shards (row 2 in shard 1 at the same cost): lowest rows first
    # obs 1: shard 1 empty (all padding), shard 2 ragged (one row);  obs 2: only shard 0 has rows
    # obs 3: +inf costs with real rows, padding elsewhere -> all padding
    costs = torch.tensor([[[1.0, 1.0, 4.0], [0.5, 2.0, INF], [0.1, 0.2, 0.3], [INF, INF, INF]],
                          [[1.0, 3.0, 3.0], [INF, INF, INF], [INF, INF, INF], [INF, INF, INF]],
                          [[0.0, 1.0, INF], [0.7, INF, INF], [INF, INF, INF], [INF, INF, INF]]], dtype=torch.float64)
    idxs = torch.tensor([[[3, 9, 1], [4, 5, -1], [7, 8, 6], [10, 11, 12]],
                         [[2, 20, 13], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]],
                         [[30, 31, -1], [40, -1, -1], [-1, -1, -1], [-1, -1, -1]]])
    for k in (1, 2, 3):
        i, c = sh.select_nearest_k(costs[:, :, :k], idxs[:, :, :k])
        ri, rc = _reference_merge(costs[:, :, :k].numpy(), idxs[:, :, :k].numpy(), k)
        assert i.tolist() == ri.tolist() and c.tolist() == rc.tolist(), k
    i, c = sh.select_nearest_k(costs, idxs)
    assert i[0].tolist() == [30, 2, 3] and c[0].tolist() == [0.0, 1.0, 1.0]       # tie at 1.0: row 2 (shard 1) before row 3
    assert i[1].tolist() == [4, 40, 5] and c[1].tolist() == [0.5, 0.7, 2.0]     # one shard empty, one ragged
    assert i[2].tolist() == [7, 8, 6] and c[2].tolist() == [0.1, 0.2, 0.3]
    assert i[3].tolist() == [-1, -1, -1] and all(v == INF for v in c[3].tolist())
    # float64 and a random cross-check against the definition (duplicated costs everywhere)
    rng = np.random.default_rng(3)
    for W, M, k in ((2, 7, 5), (3, 11, 4), (4, 5, 1)):
        cst = rng.integers(0, 4, (W, M, k)).astype(np.float64)
        idx = np.arange(W * M * k).reshape(W, M, k) % 17 + 100 * np.arange(W)[:, None, None]
        cst[rng.random((W, M, k)) < 0.2] = np.inf
        idx[rng.random((W, M, k)) < 0.1] = -1
        i, c = sh.select_nearest_k(torch.as_tensor(cst), torch.as_tensor(idx))
        ri, rc = _reference_merge(cst, idx, k)
        assert i.tolist() == ri.tolist() and c.tolist() == rc.tolist()


def test_brute_force_topk_numpy_and_torch_agree():
    bf = _bf()
    rng = np.random.default_rng(11)
    for dt in (np.float32, np.float64):
        lut = rng.uniform(0.0, 0.6, (300, 7)).astype(dt)
        lut[[40, 41, 250]] = lut[5]                  # ties
        lut[17] = np.nan
        obs = (lut[rng.integers(0, 300, 9)] + rng.normal(0, 0.01, (9, 7))).astype(dt)
        obs[0] = lut[5]
        obs[1, 2] = np.nan                           # nothing qualifies
        w = np.linspace(0.0, 2.0, 7).astype(dt)      # one zero weight
        for k, ww in ((1, None), (4, w), (300, None), (310, w)):
            ni, nc = bf.brute_force_topk_numpy(lut, obs, k, ww)
            ti, tc = bf.brute_force_topk_torch(torch.as_tensor(lut), torch.as_tensor(obs), k,
                                               None if ww is None else torch.as_tensor(ww))
            assert np.array_equal(ni, ti.numpy()) and np.array_equal(nc, tc.numpy()), (dt, k)
            assert (ni[1] == -1).all() and np.isinf(nc[1]).all()
            if k >= 4 and ww is None:
                assert ni[0, :4].tolist() == [5, 40, 41, 250]
            # column 0 is the k = 1 answer of the existing checker
            i1, c1 = bf.brute_force_numpy(lut, obs, ww)
            assert np.array_equal(ni[:, 0], i1) and np.array_equal(nc[:, 0], c1)
            assert (ni[:, 299:] == -1).all() if k > 299 else True          # row 17 (NaN) never appears: 299 rows qualify


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nb,seed", [(13, 0), (211, 1)])
def test_brute_forces_agree_on_hostile_magnitudes(nb, seed, dtype):
    """the numpy and the torch (CPU) brute forces give the same index and cost, bit for bit, on the cases of
    tests/test_gpu_lut_magnitudes.py: offsets, band scales and weights over many decades, subnormal and zero costs, one huge
    entry, rows ruled out by their norm (row_ok) -- and each case is what it claims to be (``holds``)"""
    from helpers import lut_hostile as H
    bf = _bf()
    for case in H.hostile_cases(bf, dtype, nb, seed):
        ni, nc = H.oracle(bf, case, 10)
        case.holds(ni, nc)
        t = [None if a is None else torch.as_tensor(a) for a in (case.lut, case.obs, case.w, case.row_ok)]
        f = bf.brute_force_topk_obs_weights_torch if case.per_observation else bf.brute_force_topk_torch
        ti, tc = f(t[0], t[1], 10, t[2], row_ok=t[3])
        assert np.array_equal(ni, ti.numpy()) and np.array_equal(nc, tc.numpy()), case.name
        if case.row_ok is not None and case.name.startswith("huge_entry"):       # the plain brute force leaves that row out too
            pi, pc = bf.brute_force_topk_numpy(case.lut, case.obs, 10, case.w)
            assert np.array_equal(pi, ni) and np.array_equal(pc, nc), case.name
        if not case.per_observation:                   # the obs-weights definition with every weight row equal: the same answer
            W = np.ones_like(case.obs) if case.w is None else np.repeat(case.w[None, :], len(case.obs), axis=0)
            oi, oc = bf.brute_force_topk_obs_weights_numpy(case.lut, case.obs, 10, W, row_ok=case.row_ok)
            assert np.array_equal(oi, ni) and np.array_equal(oc, nc), case.name


def test_norm_rule_numpy_is_the_kernels_norm():
    """norm_rule_numpy: finite entries and a finite centred (weighted) norm, the sum taken band by band in the dtype"""
    bf = _bf()
    lut = np.array([[1.0, 2.0], [1e20, 0.0], [np.nan, 0.0], [1.8e19, 1.8e19], [1.0, np.inf]], dtype=np.float32)
    assert bf.norm_rule_numpy(lut, np.zeros(2)).tolist() == [True, False, False, False, False]
    assert bf.norm_rule_numpy(lut, np.zeros(2), w=np.array([1e-4, 1.0])).tolist() == [True, True, False, True, False]
    assert bf.norm_rule_numpy(lut, np.zeros(2), w=np.array([-1e-4, 1e-4])).tolist() == [True, True, False, True, False]
    assert bf.norm_rule_numpy(lut.astype(np.float64), np.zeros(2)).tolist() == [True, True, False, True, False]
    assert bf.norm_rule_numpy(lut, np.array([-3e19, 0.0])).tolist() == [False] * 5      # a far centre rules out every row


def _case(B, nb, M, seed):
    rng = np.random.default_rng(seed)
    lut = rng.uniform(0.0, 0.6, (B, nb)).astype(np.float32)
    if B > 6:
        lut[B - 2] = lut[1]                          # the same spectrum in the first and the last shard
        lut[B // 2] = lut[B // 2 - 1]
        lut[3] = np.nan
    obs = (lut[rng.integers(0, B, M)] * (1 + 0.02 * rng.standard_normal((M, nb)))).astype(np.float32)
    if B > 6:
        obs[0] = lut[1]
        obs[1] = lut[B // 2]
    return lut, obs


def _topk_worker(rank, world, port, B, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lut_brute_force import brute_force_topk_numpy
    sh = _load("sharding")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lut, obs = _case(B, 13, 30, seed=7)
    w = np.linspace(0.5, 1.5, 13).astype(np.float32)
    ok = []
    lo, hi = sh.shard_bounds(B, world, rank)
    for k in (1, 3, 10):
        def topk(l, o, kk):
            i, c = brute_force_topk_numpy(l.numpy(), o.numpy(), kk, w)
            return torch.as_tensor(i), torch.as_tensor(c)
        idx, cost = sh.lut_topk_sharded(torch.as_tensor(lut[lo:hi]), lo, torch.as_tensor(obs), k, topk)
        ti, tc = brute_force_topk_numpy(lut, obs, k, w)
        ok.append(bool(np.array_equal(idx.numpy(), ti) and np.array_equal(cost.numpy(), tc)))
    # float64 bit patterns, an all-NaN LUT
    l64, o64 = lut.astype(np.float64), obs.astype(np.float64)
    i64, c64 = sh.lut_topk_sharded(torch.as_tensor(l64[lo:hi]), lo, torch.as_tensor(o64), 4,
                                   lambda l, o, kk: tuple(torch.as_tensor(x) for x in brute_force_topk_numpy(l.numpy(), o.numpy(), kk)))
    t64 = brute_force_topk_numpy(l64, o64, 4)
    ok.append(bool(np.array_equal(i64.numpy(), t64[0]) and np.array_equal(c64.numpy(), t64[1])))
    nan = np.full_like(lut, np.nan)
    ni, nc = sh.lut_topk_sharded(torch.as_tensor(nan[lo:hi]), lo, torch.as_tensor(obs), 3,
                                 lambda l, o, kk: tuple(torch.as_tensor(x) for x in brute_force_topk_numpy(l.numpy(), o.numpy(), kk)))
    ok.append(bool((ni == -1).all() and torch.isinf(nc).all()))
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


def _run(target, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=240) for _ in range(world)), key=lambda g: g[0])
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    assert [g[0] for g in got] == list(range(world))
    return got


@pytest.mark.parametrize("world,B", [(2, 101), (3, 50), (3, 2)])
def test_lut_rows_sharded_topk_matches_single_search(world, B):
    """ONE all_gather of (cost bits, global row) per observation and place, merged by (cost, row): the same k rows and
    costs as one search over the whole LUT, bit for bit, on every rank -- ties across shards, NaN rows, empty blocks."""
    for _, ok in _run(_topk_worker, world, B):
        assert all(ok), ok


class _HostEngine:
    """stands in for the HIP engine: the defined cost by brute force, on the host"""
    device = "cpu"

    def lut_nearest(self, l, o, weights=None, dtype="float32", stats=False):
        from lut_brute_force import brute_force_numpy
        return tuple(torch.as_tensor(x) for x in brute_force_numpy(l.numpy(), o.numpy(), weights))

    def lut_topk(self, l, o, k, weights=None, dtype="float32", stats=False):
        from lut_brute_force import brute_force_topk_numpy
        return tuple(torch.as_tensor(x) for x in brute_force_topk_numpy(l.numpy(), o.numpy(), k, weights))


def _unsharded_worker(rank, world, port, B, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    from lut_brute_force import brute_force_numpy, brute_force_topk_numpy
    import spart_amd.lut as L
    L.get_engine = lambda sensor, device: _HostEngine()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real = dist.all_gather

    def counting(*a, **kw):
        calls.append("all_gather")
        return real(*a, **kw)
    dist.all_gather = counting
    lut, _ = _case(B, 13, 2, seed=9)
    _, obs = _case(B, 13, 12, seed=100 + rank)      # every rank its own observations
    idx, cost = L.invert_lut(lut, obs)
    ti, tc = brute_force_numpy(lut, obs)
    same1 = bool(np.array_equal(idx, ti) and np.array_equal(cost, tc))
    idx, cost = L.invert_lut(lut, obs, k=5)
    ti, tc = brute_force_topk_numpy(lut, obs, 5)
    samek = bool(np.array_equal(idx, ti) and np.array_equal(cost, tc) and idx.shape == (12, 5))
    dist.barrier()
    q.put((rank, [same1, samek, not calls]))
    dist.destroy_process_group()


def test_invert_lut_unsharded_issues_no_collective():
    """invert_lut(shard=False) with a process group initialised: each rank searches the whole table for ITS observations,
    gets the single-process answer (k = None and integer k), and no collective is issued."""
    for _, ok in _run(_unsharded_worker, 2, 60):
        assert all(ok), ok


def test_summarise_rows_matches_numpy():
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    from spart_amd.lut import summarise_rows
    rng = np.random.default_rng(5)
    P = rng.normal(size=(1000, 27))
    idx = rng.integers(0, 1000, (37, 6))
    idx[3, 4:] = -1                                  # padding excluded
    idx[5] = -1                                      # no row at all -> NaN
    for block in (1 << 18, 7):
        mean, med, std = summarise_rows(P, idx, block_rows=block)
        for m in range(37):
            rows = idx[m][idx[m] >= 0]
            if len(rows) == 0:
                assert np.isnan(mean[m]).all() and np.isnan(med[m]).all() and np.isnan(std[m]).all()
                continue
            g = P[rows]
            np.testing.assert_allclose(mean[m], g.mean(axis=0), rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(med[m], np.median(g, axis=0), rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(std[m], g.std(axis=0), rtol=1e-12, atol=1e-14)
