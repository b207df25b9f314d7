"""What the GPU tests of spart_refine_views share beside helpers/refine_calls.py: the raw C-ABI caller, the case builder --
refine_calls.make_case's recipe with a view axis -- and the comparison with the definition tools/refine_views_defined.py."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT
from helpers.refine_calls import COLUMNS, FILL, GUARD, OUTS, bounds_of, cols_of, forward_of, rd, same
from helpers.refine_srf_calls import srf_forward_of

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_views_defined as rvd  # noqa: E402

# distinct sun / view geometry and aerosol load per view
GEOMETRY = {"tts": lambda v: 15.0 + (11 * v) % 45, "tto": lambda v: 2.0 + (7 * v) % 28, "psi": lambda v: (37.0 * v) % 180,
            "aot550": lambda v: 0.08 + 0.03 * (v % 13)}


def views_call(torch, eng, base, shared, local, lo, hi, obs, w=None, mean=None, weight=None, column=0, n_iter=2, band_model=0,
               guard=False, null=(), ws_bytes=None, V=None, n_shared=None, F=None, M=None, ctx="own"):
    """One spart_refine_views through ctypes -> (rc, dict of numpy outputs), every output pre-filled with FILL.  base (V, M, 27);
    shared, local: column numbers; obs (M, V, nb); w None, (nb,) or (M, V, nb); mean / weight: the prior per unknown, (n,) or
    (M, n).  ``V`` / ``n_shared`` / ``F`` / ``M``: sizes to pass in place of the arrays' own; ``guard``: GUARD bytes of 0xFF
    behind a correctly sized workspace must survive."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    v, m, _ = base.shape
    nb, free = obs.shape[2], list(shared) + list(local)
    f, fs = len(free), len(shared)
    n = fs + v * (f - fs)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt = up(np.moveaxis(base, 2, 0))                                  # (27, V, M)
    ot, wt, mt, pt = up(obs), up(w), up(mean), up(weight)
    full = lambda shape, dt=torch.float64: torch.full(shape, int(FILL) if dt is torch.int32 else FILL, dtype=dt, device=dev)  # noqa: E731
    out = {"x": full((m, n)), "cost": full((m,)), "cost0": full((m,)), "std": full((m, n)), "n_accept": full((m,), torch.int32),
           "y": full((m, v, nb))}
    opt = _lib.SpartRefineViewsOpt(V=v if V is None else V, n_shared=fs if n_shared is None else n_shared, band_model=band_model)
    opt.fit = _lib.SpartRefineOpt(column=column, n_iter=n_iter, weights_per_obs=int(w is not None and np.ndim(w) == 3),
                                  prior_per_obs=int(mean is not None and np.ndim(mean) == 2),
                                  prior_mean=None if mt is None else mt.data_ptr(), prior_weight=None if pt is None else pt.data_ptr())
    need = int(eng.lib.spart_views_workspace_bytes(eng.ctx, m, v, f, fs))
    size = need if ws_bytes is None else ws_bytes
    if guard:
        assert ws_bytes is None and need > 0
        ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    else:
        ws = torch.empty(max(size, 256), dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    ptr = lambda name, val: None if name in null else val     # noqa: E731
    rc = eng.lib.spart_refine_views(eng.ctx if ctx == "own" else ctx, m if M is None else M,
                                    ptr("base", (_lib.vp * 27)(*[Bt[i].data_ptr() for i in range(27)])), f if F is None else F,
                                    ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), ptr("lo", lo.ctypes.data_as(_lib.c_dp)),
                                    ptr("hi", hi.ctypes.data_as(_lib.c_dp)), ptr("obs", ot.data_ptr()),
                                    None if wt is None else wt.data_ptr(), ptr("opt", ctypes.byref(opt)),
                                    *[ptr(k, out[k].data_ptr()) for k in OUTS], ptr("ws", ws.data_ptr()), ctypes.c_size_t(size),
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[need:] == 0xFF).all()), "bytes behind the workspace were written"
    return rc, {k: val.cpu().numpy() for k, val in out.items()}


def make_views_case(torch, eng, shared, local, M, V, column, kind, prior, seed, at=0, srf=False):
    """refine_calls.make_case with a view axis.  truth = LHS rows, the same for every view but for tts / tto / psi / aot550
    (GEOMETRY) and the local names (their own LHS draw per view); obs = the model at the truth, 1 % noise; starts moved up to
    10 % of the range.  ``kind``: "none" / "shared" ((nb,)) / "per_pixel" ((M, V, nb), 15 % zeros over NaN observations) weights;
    ``prior``: "none" / "shared" ((n,)) / "per_pixel" ((M, n), 20 % zero weights over NaN means).
    Special pixels from ``at`` (M >= at + 4; the fifth needs M > at + 4): +0 a start outside the bounds and a NaN in view 1's entry of a shared column
    (ignored); +1 a NaN fixed parameter in the last view only (dead); +2 a negative weight in view 0 (per-pixel weights; dead);
    +3 the last view fully masked over NaN observations (per-pixel weights); +4 a local start exactly on hi in the last view only.
    -> dict of views_call's / refine_views_defined's arguments (names -> column numbers) and ``truth`` (V, M, 27)"""
    from spart_amd import workloads
    rng = np.random.default_rng(seed)
    names = list(shared) + list(local)
    free, (lo, hi) = cols_of(names), bounds_of(names)
    Fs, Fl = len(shared), len(local)
    F, n = Fs + Fl, Fs + V * Fl
    truth = np.repeat(workloads.lhs_params(M, "full", seed=seed)[None], V, axis=0)
    for v in range(V):
        for name, f in GEOMETRY.items():
            if name not in shared:
                truth[v, :, workloads.PARAM_NAMES.index(name)] = f(v)
        if Fl and v:
            truth[v][:, free[Fs:]] = workloads.lhs_params(M, "full", seed=seed + 1000 * v)[:, free[Fs:]]
    fwd = (srf_forward_of if srf else forward_of)(torch, eng, column)
    with np.errstate(all="ignore"):
        obs = np.moveaxis(fwd(truth.reshape(V * M, 27)).reshape(V, M, -1), 0, 1)
    obs = np.where(np.isfinite(obs), obs, 0.3) * (1.0 + 0.01 * rng.normal(size=obs.shape))
    nb = obs.shape[2]
    base = truth.copy()
    move = rng.uniform(-0.1, 0.1, (V, M, F)) * (hi - lo)
    move[:, :, :Fs] = move[0][None][:, :, :Fs]                        # one start per shared name
    base[:, :, free] = rd.clip_defined(truth[:, :, free] + move, lo, hi)
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 2, nb)
        w[rng.random(nb) < 0.2] = 0.0
        w[0] = w[0] or 1.0
    elif kind == "per_pixel":
        w = 10.0 ** rng.uniform(-1, 2, (M, V, nb))
        w[rng.random((M, V, nb)) < 0.15] = 0.0
        w[:, :, 1] = np.where(w[:, :, 1] == 0.0, 1.0, w[:, :, 1])     # (at least one band counts in every view)
    if M >= at + 4:
        base[0, at, free[0]] = hi[0] + 0.5 * (hi[0] - lo[0])
        if V > 1 and Fs:
            base[1, at, free[0]] = np.nan
        base[V - 1, at + 1, 20 if 20 not in free else 26] = np.nan
        if kind == "per_pixel":
            w[at + 2, 0, nb // 2] = -1.0
            w[at + 3, V - 1] = 0.0
        if Fl and M > at + 4:
            base[V - 1, at + 4, free[-1]] = hi[-1]
    if kind == "per_pixel":
        obs[w == 0.0] = np.nan                                        # zero weights over NaN observations
    mean = weight = None
    if prior != "none":
        name_of = [rvd.name_of(a, Fs, Fl) for a in range(n)]
        t0 = np.stack([truth[max(rvd.view_of(a, Fs, Fl), 0), :, free[name_of[a]]] for a in range(n)], axis=1)      # (M, n)
        shape = (M, n) if prior == "per_pixel" else (n,)
        mean = (t0 if prior == "per_pixel" else t0[0]) + 0.1 * rng.normal(size=shape) * (hi - lo)[name_of]
        weight = np.array(np.broadcast_to(1.0 / (0.1 * (hi - lo)[name_of]) ** 2, shape))
        if prior == "per_pixel":
            zero = rng.random(shape) < 0.2
            mean, weight = np.where(zero, np.nan, mean), np.where(zero, 0.0, weight)
    return dict(base=base, shared=free[:Fs], local=free[Fs:], lo=lo, hi=hi, obs=obs, w=w, mean=mean, weight=weight, truth=truth)


def defined_views(torch, eng, case, column, n_iter, srf=False, history=None):
    fwd = (srf_forward_of if srf else forward_of)(torch, eng, COLUMNS[column])
    return rvd.refine_views_defined(case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], fwd,
                                    weights=case["w"], n_iter=n_iter, prior_mean=case["mean"], prior_weight=case["weight"],
                                    history=history)


def call_views(torch, eng, case, column, n_iter, **kw):
    rc, got = views_call(torch, eng, case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], case["w"],
                         case["mean"], case["weight"], column=column, n_iter=n_iter, **kw)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    return got


def not_vacuous(ref, n_iter, what):
    """the conditions on the DEFINITION's output that keep a random case from being vacuous"""
    live = ref["n_accept"] >= 0
    assert live.mean() >= 0.85, (what, float(live.mean()))
    assert n_iter == 0 or (ref["n_accept"] >= 1).mean() >= 0.5, (what, float((ref["n_accept"] >= 1).mean()))
    assert (ref["cost"][live] <= ref["cost0"][live]).all(), what


def check_views(torch, eng, case, column, n_iter, what, **kw):
    """the library against the definition, bit for bit -> (ref, got)"""
    ref = defined_views(torch, eng, case, column, n_iter, srf=kw.get("band_model", 0) == 1)
    got = call_views(torch, eng, case, column, n_iter, **kw)
    for k in OUTS:
        assert same(got[k], ref[k]), (what, k, int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()))
    not_vacuous(ref, n_iter, what)
    return ref, got
