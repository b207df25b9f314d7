"""What the GPU tests of spart_lut_bayes share: the raw C-ABI caller, the definition (tools/lut_bayes_defined.py) and the data
builders.  The fixtures are helpers.lut_calls' (imported by name)."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import DT, ROOT, near_rows_case

sys.path.insert(0, os.path.join(ROOT, "tools"))
import lut_bayes_defined as defined  # noqa: E402

OUTS = ("mean", "std", "sum_w", "ess", "count", "best_idx", "best_cost")
FILL = -7          # what bayes_call writes into every output before the call: a refused call leaves it there


def bayes_call(torch, eng, lut, params, obs, w, cut=50.0, temperature=1.0, brute_force=0, dtype="float32", ws_bytes=None,
               null=(), outs=OUTS, opt=True, **sizes):
    """One spart_lut_bayes through ctypes -> (rc, dict of the output tensors, stats dict).  ``null``: which of lut / params / obs /
    w / out to pass as NULL; ``outs``: the outputs that are not NULL; ``opt`` False: a NULL option struct; ``sizes``: B / nb / P /
    M / dt to pass in place of the tensors' own (the refusal cases, which return before anything is read)."""
    from spart_amd import _lib
    B, nb, P, M = (sizes.get(n, v) for n, v in zip(("B", "nb", "P", "M"), (*lut.shape, params.shape[1], obs.shape[0])))
    dt = sizes.get("dt", DT[dtype])
    m, p = obs.shape[0], params.shape[1]
    res = {"mean": torch.full((m, p), FILL, dtype=torch.float64, device=lut.device),
           "std": torch.full((m, p), FILL, dtype=torch.float64, device=lut.device),
           "sum_w": torch.full((m,), FILL, dtype=torch.float64, device=lut.device),
           "ess": torch.full((m,), FILL, dtype=torch.float64, device=lut.device),
           "count": torch.full((m,), FILL, dtype=torch.int64, device=lut.device),
           "best_idx": torch.full((m,), FILL, dtype=torch.int64, device=lut.device),
           "best_cost": torch.full((m,), FILL, dtype=lut.dtype, device=lut.device)}
    o = _lib.SpartLutBayesOpt(cut, temperature, brute_force)
    out = _lib.SpartLutBayesOut(*[res[n].data_ptr() if n in outs else None for n in OUTS])
    need = int(eng.lib.spart_lut_bayes_workspace_bytes(dt, B, nb, M))
    n = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=lut.device)
    a = {"lut": lut, "params": params, "obs": obs, "w": w}
    a = {name: None if t is None or name in null else t.data_ptr() for name, t in a.items()}
    rc = eng.lib.spart_lut_bayes(eng.ctx, dt, B, nb, a["lut"], P, a["params"], M, a["obs"], a["w"],
                                 ctypes.byref(o) if opt else None, None if "out" in null else ctypes.byref(out), ws.data_ptr(),
                                 ctypes.c_size_t(n), None)
    torch.cuda.synchronize()
    st = {}
    if rc == 0 and M > 0 and B > 0:
        names = ("brute_force", "candidate_tiles", "max_candidate_tiles")
        counts, word = [ctypes.c_int64() for _ in names], ctypes.c_double()
        assert eng.lib.spart_lut_bayes_stats(eng.ctx, dt, B, nb, M, ws.data_ptr(), *map(ctypes.byref, counts), ctypes.byref(word)) == 0
        st = {**{name: c.value for name, c in zip(names, counts)}, "nbound": word.value}
    return rc, res, st


def same(torch, a, b, rows=None, names=OUTS):
    """the outputs of two calls equal bit for bit (NaN == NaN), on ``rows`` of the first and all of the second"""
    for n in names:
        x = a[n] if rows is None else a[n][rows]
        if not torch.equal(torch.nan_to_num(x.double(), nan=-1.25e300), torch.nan_to_num(b[n].double(), nan=-1.25e300)):
            return n
    return None


def noisy_case(torch, g, B, M, nb, P, td, rel=0.05, floor=0.01):
    """near_rows_case's LUT and observations with relative-noise weights 1 / (rel |obs| + floor)^2, and a (B, P) parameter table.
    In a uniform random LUT the chi^2 of the other rows is narrow around nb / (6 sigma^2): rel and floor decide whether a cut of
    50 above the observation's own row holds one row, some, or all of them."""
    lut, obs = near_rows_case(torch, g, B, M, nb, td)
    w = (1.0 / (rel * obs.double().abs() + floor) ** 2).to(td).contiguous()
    params = (8.0 * torch.rand((B, P), generator=g, device="cuda:0", dtype=torch.float64)).contiguous()
    return lut, params, obs, w


def to_np(t):
    return {n: v.cpu().numpy() for n, v in t.items()}
