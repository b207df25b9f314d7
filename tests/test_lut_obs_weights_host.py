"""Per-observation LUT weights without a GPU: the two brute-force checkers of spart_lut_topk_obs_weights agree (zero-skip with
NaN / inf in masked bands), noise_weights' values and mask, the weights-shape rule of Engine.lut_nearest / lut_topk, and
invert_lut(shard=True) with (M, nb) weights under gloo with a host stand-in engine."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, HERE)

import lut_brute_force as bf  # noqa: E402
from test_lut_topk_host import _run  # noqa: E402


def _masked_case(B, nb, M, dt, seed):
    rng = np.random.default_rng(seed)
    lut = rng.uniform(0.0, 0.6, (B, nb)).astype(dt)
    lut[[11, 12, 40]] = lut[5]                               # ties
    lut[17, 2] = np.nan                                      # a NaN row (masked or not, it never appears)
    obs = (lut[rng.integers(0, B, M)] + rng.normal(0, 0.01, (M, nb))).astype(dt)
    w = rng.uniform(0.5, 2.0, (M, nb)).astype(dt)
    zero = rng.random((M, nb)) < 0.15
    w[zero] = 0
    obs[zero & (rng.random((M, nb)) < 0.5)] = np.nan         # masked bands may hold NaN / inf
    obs[zero & (rng.random((M, nb)) < 0.3)] = np.inf
    obs[0] = lut[5]
    w[1] = 0                                                 # all masked: every accepted row costs 0
    w[2, 0] = -1.0                                           # a negative weight: nothing
    w[3, 1] = np.nan
    w[4, 1] = np.inf
    obs[5, 3], w[5, 3] = np.nan, 1.0                         # a non-finite unmasked value: nothing
    return lut, obs, w


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_obs_weights_brute_forces_agree(dt):
    B, nb, M = 300, 7, 12
    lut, obs, w = _masked_case(B, nb, M, dt, 11)
    for k in (1, 4, 299, 310):
        ni, nc = bf.brute_force_topk_obs_weights_numpy(lut, obs, k, w)
        ti, tc = bf.brute_force_topk_obs_weights_torch(torch.as_tensor(lut), torch.as_tensor(obs), k, torch.as_tensor(w))
        assert np.array_equal(ni, ti.numpy()) and np.array_equal(nc, tc.numpy()), k
        for m in (2, 3, 4, 5):
            assert (ni[m] == -1).all() and np.isinf(nc[m]).all(), (k, m)
        kk = min(k, B - 1)                                   # row 17 never appears
        assert ni[1, :kk].tolist() == [r for r in range(B) if r != 17][:kk] and (nc[1, :kk] == 0).all()
        assert 17 not in ni
        if k >= 4:
            assert ni[0, :4].tolist() == [5, 11, 12, 40]
    # the definition, literally, for a few observations (no vectorisation at all)
    ni, nc = bf.brute_force_topk_obs_weights_numpy(lut, obs, 3, w)
    for m in (0, 6, 9):
        c = []
        for b in range(B):
            s = dt(0)
            for j in range(nb):
                if w[m, j] == 0:
                    continue
                d = dt(lut[b, j] - obs[m, j])
                s = dt(s + dt(dt(w[m, j] * d) * d))
            c.append(s if np.isfinite(lut[b]).all() and np.isfinite(s) else dt(np.inf))
        o = sorted(range(B), key=lambda b: (c[b], b))[:3]
        assert ni[m].tolist() == o and nc[m].tolist() == [c[b] for b in o]


def test_obs_weights_shared_rows_equal_shared_weights():
    """identity (I1) of the checkers: every weight row equal to w, no masks -> brute_force_topk_numpy(w), bit for bit"""
    rng = np.random.default_rng(2)
    for dt in (np.float32, np.float64):
        lut = rng.uniform(0, 1, (200, 9)).astype(dt)
        obs = rng.uniform(0, 1, (8, 9)).astype(dt)
        w = rng.uniform(0.5, 2, 9).astype(dt)
        a = bf.brute_force_topk_obs_weights_numpy(lut, obs, 6, np.tile(w, (8, 1)))
        b = bf.brute_force_topk_numpy(lut, obs, 6, w)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_noise_weights_values_and_mask():
    from spart_amd import noise_weights
    obs = np.array([[0.1, 0.2, np.nan, 0.4], [0.5, np.inf, 0.0, -np.inf]])
    w = noise_weights(obs, abs_sigma=0.01, rel_sigma=0.02)
    assert w.dtype == np.float64 and w.shape == (2, 4)
    fin = np.isfinite(obs)
    assert (w[~fin] == 0).all()
    np.testing.assert_array_equal(w[fin], 1.0 / (0.01 ** 2 + (0.02 * obs[fin]) ** 2))
    a = np.array([0.01, 0.02, 0.03, 0.04])
    w2 = noise_weights(obs, abs_sigma=a)                     # per-band absolute sigma, no relative term
    np.testing.assert_array_equal(w2[fin], (1.0 / np.broadcast_to(a * a, obs.shape))[fin])
    w3 = noise_weights(obs, rel_sigma=0.02)
    assert w3[1, 2] == np.inf and w3[0, 0] == 1.0 / (0.02 * 0.1) ** 2
    with pytest.raises(ValueError):
        noise_weights(obs)
    with pytest.raises(ValueError):
        noise_weights(obs, abs_sigma=np.zeros(4))
    with pytest.raises(ValueError):
        noise_weights(obs, abs_sigma=np.ones(3))
    with pytest.raises(ValueError):
        noise_weights(obs[0], rel_sigma=0.02)


def test_engine_weights_shape_rule():
    from spart_amd.engine import lut_weights_kind
    assert lut_weights_kind(None, 5, 13) == "none"
    assert lut_weights_kind((13,), 5, 13) == "shared"
    assert lut_weights_kind((13,), 13, 13) == "shared"
    assert lut_weights_kind((5, 13), 5, 13) == "per_observation"
    assert lut_weights_kind((1, 13), 1, 13) == "per_observation"
    for bad in ((12,), (5, 12), (4, 13), (1, 13), (13, 1), (5, 13, 1), ()):
        with pytest.raises(ValueError, match="weights"):
            lut_weights_kind(bad, 5, 13)


class _HostEngine:
    """stands in for the HIP engine: the defined cost by brute force, on the host"""
    device = "cpu"

    def lut_nearest(self, l, o, weights=None, dtype="float32", stats=False):
        i, c = self.lut_topk(l, o, 1, weights, dtype, stats)
        return i[:, 0], c[:, 0]

    def lut_topk(self, l, o, k, weights=None, dtype="float32", stats=False):
        w = np.asarray(weights, dtype=l.numpy().dtype)
        assert w.shape == tuple(o.shape)
        return tuple(torch.as_tensor(x) for x in bf.brute_force_topk_obs_weights_numpy(l.numpy(), o.numpy(), k, w))


def _sharded_worker(rank, world, port, B, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import spart_amd.lut as L
    L.get_engine = lambda sensor, device: _HostEngine()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lut, obs, w = _masked_case(B, 13, 20, np.float32, 5)
    ok = []
    for k in (None, 1, 4, 10):
        idx, cost = L.invert_lut(lut, obs, weights=w, shard=True, k=k)
        ti, tc = bf.brute_force_topk_obs_weights_numpy(lut, obs, 1 if k is None else k, w)
        if k is None:
            ti, tc = ti[:, 0], tc[:, 0]
        ok.append(bool(np.array_equal(idx, ti) and np.array_equal(cost, tc)))
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,B", [(2, 101), (3, 50)])
def test_invert_lut_sharded_obs_weights_matches_single_search(world, B):
    """(M, nb) weights, the same on every rank: the merged per-shard results equal one search of the whole LUT bit for bit"""
    for _, ok in _run(_sharded_worker, world, B):
        assert all(ok), ok
