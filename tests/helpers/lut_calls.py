"""What the GPU tests of the LUT searches share: the raw C-ABI caller of all four searches (spart_lut_nearest, _topk,
_topk_wide, _topk_obs_weights), their fixtures (imported by name) and the data builders more than one file uses."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hyperspectral.npz")
DT = {"float32": 0, "float64": 1}
# search -> (prefix of its *_workspace_bytes / *_stats, the widest nb it takes, the key of its stats' float64 word)
ENTRIES = {"spart_lut_nearest": ("spart_lut", 31, "nmax"),
           "spart_lut_topk": ("spart_lut_topk", 31, "nmax"),
           "spart_lut_topk_wide": ("spart_lut_topk_wide", 2162, "nmax"),
           "spart_lut_topk_obs_weights": ("spart_lut_topk_obs_weights", 2162, "nbound")}
FILL = -7          # what lut_call writes into idx and cost before the call: a refused call leaves it there
GUARD = 4096       # lut_call(guard=True): bytes kept behind the workspace that the call must leave as they were


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def bf():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lut_brute_force
    return lut_brute_force


@pytest.fixture(scope="module")
def eng(torch_mod):
    from spart_amd import get_engine
    return get_engine(None, 0)


@pytest.fixture(scope="module")
def hyper_si():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_hyperspectral import sensorinfo_from_npz
    return sensorinfo_from_npz(dict(np.load(FIXTURE)))


@pytest.fixture(scope="module")
def spectra(torch_mod, hyper_si):
    """(4096, 211) float64 R_TOC spectra of the 211-band sensor on LHS parameters (NaN entries replaced by 0.5)"""
    from spart_amd import get_engine, workloads
    e = get_engine(None, 0, sensor_info=hyper_si)
    P = workloads.lhs_params(4096, "full", seed=321)
    r = e.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), "float64")["R_TOC"]
    return torch_mod.nan_to_num(r, nan=0.5)


def lut_call(torch, eng, entry, lut, obs, k, w=None, dtype="float32", ws_bytes=None, null=(), guard=False, **sizes):
    """One LUT search through ctypes -> (rc, idx, cost, stats dict).  ``k`` None goes with spart_lut_nearest: no k argument,
    (M,) outputs, two stats.  ``ws_bytes``: the workspace size handed in, in place of the search's *_workspace_bytes;
    ``null``: which of lut / obs / w / idx / cost to pass as NULL; ``sizes``: B / nb / M / dt (the dtype code) to pass in
    place of the tensors' own -- for the refusal cases, which return before anything is read.
    ``guard``: the workspace is allocated GUARD bytes longer than *_workspace_bytes says and filled with 0xFF bytes throughout
    (a buffer the call does not write then holds NaN patterns, not an earlier chunk's plausible values); the call is given the
    size it asked for, and afterwards the GUARD bytes behind it must still be 0xFF."""
    family, _, scale = ENTRIES[entry]
    B, nb, M = (sizes.get(n, v) for n, v in zip(("B", "nb", "M"), (*lut.shape, obs.shape[0])))
    dt = sizes.get("dt", DT[dtype])
    kk = () if k is None else (k,)
    shape = (obs.shape[0],) + tuple(max(x, 0) for x in kk)
    idx = torch.full(shape, FILL, dtype=torch.int64, device=lut.device)
    cost = torch.full(shape, FILL, dtype=lut.dtype, device=lut.device)
    need = int(getattr(eng.lib, family + "_workspace_bytes")(dt, B, nb, M, *kk))
    n = need if ws_bytes is None else ws_bytes
    if guard:
        assert ws_bytes is None and need > 0
        ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=lut.device)
    else:
        ws = torch.empty(max(n, 256), dtype=torch.uint8, device=lut.device)
    p = {"lut": lut, "obs": obs, "w": w, "idx": idx, "cost": cost}
    p = {name: None if t is None or name in null else t.data_ptr() for name, t in p.items()}
    rc = getattr(eng.lib, entry)(eng.ctx, dt, B, nb, p["lut"], M, p["obs"], p["w"], *kk, p["idx"], p["cost"], ws.data_ptr(),
                                 ctypes.c_size_t(n), None)
    st = {}
    if rc == 0 and M > 0:
        torch.cuda.synchronize()
        names = ("brute_force", "candidate_tiles", "max_candidate_tiles")[:1 if k is None else 3]
        counts, word = [ctypes.c_int64() for _ in names], ctypes.c_double()
        assert getattr(eng.lib, family + "_stats")(eng.ctx, dt, B, nb, M, *kk, ws.data_ptr(), *map(ctypes.byref, counts),
                                                   ctypes.byref(word)) == 0
        st = {**{name: c.value for name, c in zip(names, counts)}, scale: word.value}
    if guard:
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xFF).all()), (entry, dtype, "bytes behind the workspace were written")
    return rc, idx, cost, st


def tdtype(torch, dtype):
    return torch.float32 if dtype == "float32" else torch.float64


def near_rows_case(torch, g, B, M, nb, td):
    """a uniform (B, nb) LUT and M observations = every 13th row + 0.05 N(0, 1), from the generator ``g``"""
    lut = torch.rand((B, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    obs = (lut[torch.arange(M, device="cuda:0") * 13 % B] + 0.05 * torch.randn((M, nb), generator=g, device="cuda:0",
                                                                             dtype=torch.float64).to(td)).contiguous()
    return lut, obs


def equal_rows_case(torch, g, td, nb=211, B=32 * 300 + 5):
    """all rows equal but one, 9 observations within 0.1 % of them: every tile is a candidate, the lists overflow and the
    brute force decides"""
    base = torch.rand((1, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td)
    lut = base.repeat(B, 1).contiguous()
    lut[4000] = base[0] * 0.999
    obs = (base.repeat(9, 1) * (1 + 0.001 * torch.randn((9, nb), generator=g, device="cuda:0", dtype=torch.float64).to(td))).contiguous()
    return lut, obs
