"""What the tests of spart_lut_bayes_quantiles share: the raw C-ABI caller beside helpers.lut_bayes_calls' (same outputs, same
FILL, plus quant), and the bracket property that ties a returned quantile to the exactly rounded sums of the same omegas."""
import ctypes
import math

import numpy as np

from helpers.lut_bayes_calls import FILL, OUTS, defined
from helpers.lut_calls import DT

QOUTS = OUTS + ("quant",)


def quant_call(torch, eng, lut, params, obs, w, levels=(0.05, 0.5, 0.95), cut=50.0, temperature=1.0, brute_force=0, dtype="float32",
               ws_bytes=None, null=(), outs=QOUTS, opt=True, nq=None, **sizes):
    """One spart_lut_bayes_quantiles through ctypes -> (rc, dict of the output tensors with "quant" (M, P, Q), stats dict).
    helpers.lut_bayes_calls.bayes_call's arguments; ``levels`` None: a NULL pointer; ``nq``: the count handed over in place of
    len(levels) (the buffer of "quant" is sized for max(len(levels), 1))."""
    from spart_amd import _lib
    B, nb, P, M = (sizes.get(n, v) for n, v in zip(("B", "nb", "P", "M"), (*lut.shape, params.shape[1], obs.shape[0])))
    dt = sizes.get("dt", DT[dtype])
    m, p = obs.shape[0], params.shape[1]
    Q = max(len(levels) if levels is not None else 1, 1)
    res = {"mean": torch.full((m, p), FILL, dtype=torch.float64, device=lut.device),
           "std": torch.full((m, p), FILL, dtype=torch.float64, device=lut.device),
           "sum_w": torch.full((m,), FILL, dtype=torch.float64, device=lut.device),
           "ess": torch.full((m,), FILL, dtype=torch.float64, device=lut.device),
           "count": torch.full((m,), FILL, dtype=torch.int64, device=lut.device),
           "best_idx": torch.full((m,), FILL, dtype=torch.int64, device=lut.device),
           "best_cost": torch.full((m,), FILL, dtype=lut.dtype, device=lut.device),
           "quant": torch.full((m, p, Q), FILL, dtype=torch.float64, device=lut.device)}
    lv = None if levels is None else (ctypes.c_double * max(len(levels), 1))(*levels)
    o = _lib.SpartLutBayesQOpt(_lib.SpartLutBayesOpt(cut, temperature, brute_force), len(levels or ()) if nq is None else nq, lv)
    out = _lib.SpartLutBayesQOut(_lib.SpartLutBayesOut(*[res[n].data_ptr() if n in outs else None for n in OUTS]),
                                 res["quant"].data_ptr() if "quant" in outs else None)
    need = int(eng.lib.spart_lut_bayes_workspace_bytes(dt, B, nb, M))
    n = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=lut.device)
    a = {"lut": lut, "params": params, "obs": obs, "w": w}
    a = {name: None if t is None or name in null else t.data_ptr() for name, t in a.items()}
    rc = eng.lib.spart_lut_bayes_quantiles(eng.ctx, dt, B, nb, a["lut"], P, a["params"], M, a["obs"], a["w"],
                                           ctypes.byref(o) if opt else None, None if "out" in null else ctypes.byref(out),
                                           ws.data_ptr(), ctypes.c_size_t(n), None)
    torch.cuda.synchronize()
    st = {}
    if rc == 0 and M > 0 and B > 0:
        names = ("brute_force", "candidate_tiles", "max_candidate_tiles")
        counts, word = [ctypes.c_int64() for _ in names], ctypes.c_double()
        assert eng.lib.spart_lut_bayes_stats(eng.ctx, dt, B, nb, M, ws.data_ptr(), *map(ctypes.byref, counts), ctypes.byref(word)) == 0
        st = {**{name: c.value for name, c in zip(names, counts)}, "nbound": word.value}
    return rc, res, st


def bracket_violations(members, params, quant, levels, cut, tau):
    """The bracket property of every (m, p, i), none left out.  ``members``: tools/lut_bayes_defined.members_defined's list;
    ``quant`` (M, P, Q).  With F_ex and W by math.fsum over long-double omegas (as lut_bayes_exact), a returned v must
      - be one of the x values of S,
      - satisfy F_ex(v) >= q W (1 - g),
      - and, for the next smaller data value u (if there is one and q > 0), F_ex(u) < q W (1 + g).
    g = 3 f with f = 4 ((4 + cut / tau) 2^-52 + n 2^-53), the bound test_gpu_lut_bayes.check_values derives for an ordered sum
    of n omegas against the exactly rounded one: counted once for F, once for sum_w and once for the product q * sum_w.
    An empty set wants NaN; a column with a NaN over S wants NaN.  -> list of (m, p, i, what) that fail."""
    params = np.asarray(params, dtype=np.float64)
    bad = []
    ltau = np.longdouble(1.0 if tau == 0 else tau)
    for m, (rows, e, _, _) in enumerate(members):
        if rows.size == 0:
            bad += [(m, p, i, "not NaN for an empty set") for p, i in zip(*np.nonzero(~np.isnan(quant[m])))]
            continue
        om = np.exp(-(e.astype(np.longdouble) / (2 * ltau))).astype(np.float64)
        n = rows.size
        g = 3.0 * 4.0 * ((4.0 + min(cut / float(ltau), 1500.0)) * 2.0 ** -52 + n * 2.0 ** -53)
        W = math.fsum(om)
        for p in range(params.shape[1]):
            x = params[rows, p]
            if np.isnan(x).any():
                bad += [(m, p, i, "not NaN for a column with a NaN") for i in np.nonzero(~np.isnan(quant[m, p]))[0]]
                continue
            order = np.argsort(x, kind="stable")
            xs = x[order]
            for i, q in enumerate(levels):
                v = quant[m, p, i]
                if not (v == xs).any() or np.isnan(v):
                    bad.append((m, p, i, f"{v!r} is not a value of the set"))
                    continue
                hi = int(np.searchsorted(xs, v, side="right"))             # rows with x <= v: xs[:hi]
                lo = int(np.searchsorted(xs, v, side="left"))              # rows with x < v = rows with x <= u: xs[:lo]
                F_v = math.fsum(om[order[:hi]])
                if not F_v >= q * W * (1.0 - g):
                    bad.append((m, p, i, f"F({v!r}) = {F_v!r} < q W (1 - g) = {q * W * (1.0 - g)!r}"))
                if lo > 0 and q > 0:
                    F_u = math.fsum(om[order[:lo]])
                    if not F_u < q * W * (1.0 + g):
                        bad.append((m, p, i, f"F({xs[lo - 1]!r}) = {F_u!r} >= q W (1 + g): {v!r} is not the smallest"))
    return bad


def quantiles_want(lut, params, obs, w, levels, cut=50.0, temperature=1.0, row_ok=None):
    """(members, the numpy definition's (M, P, Q)) of host arrays"""
    members = defined.members_defined(lut, obs, w, cut, row_ok)
    return members, defined.lut_bayes_quantiles_defined(lut, params, obs, w, levels, cut, temperature, row_ok, members=members)
