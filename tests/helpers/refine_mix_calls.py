"""What the GPU tests of spart_refine_mix share beside helpers/refine_calls.py: the raw C-ABI caller, the case builder --
refine_calls.make_case's recipe with a component axis and fractions -- and the comparison with the definition
tools/refine_mix_defined.py, whose forward model is the engine's own forward call (refine_calls.forward_of)."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT
from helpers.refine_calls import COLUMNS, FILL, GUARD, bounds_of, cols_of, forward_of, rd
from helpers.refine_srf_calls import srf_forward_of

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_mix_defined as rmd  # noqa: E402

OUTS = ("x", "cost", "cost0", "std", "n_accept", "y", "frac", "y_comp")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def n_of(V, Fs, Fl, active, fit):
    return rmd.maps_defined(V, Fs, Fl, active, fit)[0].size


def mix_call(torch, eng, base, shared, local, lo, hi, obs, frac, active=None, fit=True, w=None, mean=None, weight=None, column=0,
             n_iter=2, lambda0=0.0, band_model=0, frac_lo=0.0, frac_hi=0.0, guard=False, null=(), ws_bytes=None, V=None, n_shared=None,
             F=None, M=None, ctx="own", only=None):
    """One spart_refine_mix through ctypes -> (rc, dict of numpy outputs), every output pre-filled with FILL.  base (V, M, 27);
    shared, local: column numbers; obs (M, nb); frac (M, V); active None or (V, Fl) 0 / 1; w None, (nb,) or (M, nb); mean /
    weight: the prior per unknown, (n,) or (M, n).  ``V`` / ``n_shared`` / ``F`` / ``M`` / ``fit``: values to pass in place of
    the arrays' own; ``only``: the outputs to ask for beside x and cost (the others are NULL); ``guard``: GUARD bytes of 0xFF
    behind a correctly sized workspace must survive."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    v, m, _ = base.shape
    nb, free = obs.shape[1], list(shared) + list(local)
    f, fs = len(free), len(shared)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    try:
        n = n_of(v, fs, f - fs, None if act is None else np.clip(act, 0, 1), fit in (1, True))
    except ValueError:
        n = f
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt = up(np.moveaxis(base, 2, 0))                                  # (27, V, M)
    ot, wt, mt, pt, ft = up(obs), up(w), up(mean), up(weight), up(frac)
    full = lambda shape, dt=torch.float64: torch.full(shape, int(FILL) if dt is torch.int32 else FILL, dtype=dt, device=dev)  # noqa: E731
    out = {"x": full((m, n)), "cost": full((m,)), "cost0": full((m,)), "std": full((m, n)), "n_accept": full((m,), torch.int32),
           "y": full((m, nb)), "frac": full((m, v)), "y_comp": full((m, v, nb))}
    opt = _lib.SpartRefineMixOpt(V=v if V is None else V, n_shared=fs if n_shared is None else n_shared, band_model=band_model,
                                 fit_fractions=int(fit), local_active=None if act is None else act.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 frac_lo=frac_lo, frac_hi=frac_hi)
    opt.fit = _lib.SpartRefineOpt(column=column, n_iter=n_iter, lambda0=lambda0, weights_per_obs=int(w is not None and np.ndim(w) == 2),
                                  prior_per_obs=int(mean is not None and np.ndim(mean) == 2),
                                  prior_mean=None if mt is None else mt.data_ptr(), prior_weight=None if pt is None else pt.data_ptr())
    need = int(eng.lib.spart_mix_workspace_bytes(eng.ctx, m, v, f, n))
    size = need if ws_bytes is None else ws_bytes
    if guard:
        assert ws_bytes is None and need > 0
        ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    else:
        ws = torch.empty(max(size, 256), dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    ptr = lambda name, val: None if name in null else val     # noqa: E731
    asked = lambda k: k in ("x", "cost") or only is None or k in only     # noqa: E731
    co = _lib.SpartRefineMixOut(**{k: ptr(k, out[k].data_ptr()) if asked(k) else None for k in OUTS})
    rc = eng.lib.spart_refine_mix(eng.ctx if ctx == "own" else ctx, m if M is None else M,
                                  ptr("base", (_lib.vp * 27)(*[Bt[i].data_ptr() for i in range(27)])), f if F is None else F,
                                  ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), ptr("lo", lo.ctypes.data_as(_lib.c_dp)),
                                  ptr("hi", hi.ctypes.data_as(_lib.c_dp)), ptr("obs", ot.data_ptr()),
                                  None if wt is None else wt.data_ptr(), ptr("frac", ft.data_ptr()), ptr("opt", ctypes.byref(opt)),
                                  ptr("out", ctypes.byref(co)), ptr("ws", ws.data_ptr()), ctypes.c_size_t(size),
                                  ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[need:] == 0xFF).all()), "bytes behind the workspace were written"
    return rc, {k: val.cpu().numpy() for k, val in out.items()}


def make_mix_case(torch, eng, V, shared, local, active, fit, M, column, kind, prior, seed, at=0, srf=False, move=0.1, lambda0=None,
                  noise=0.01, last_below=None, prior_sigma=0.1):
    """refine_calls.make_case with a component axis.  truth = one LHS draw per component, the shared names from component 0;
    true fractions a Dirichlet(3) draw (``last_below``: the last one uniform below that value); obs = the mixed model at the
    truth, ``noise`` relative noise; starts moved up to ``move`` of the range, fitted fractions start at 0.8 a + 0.2 / V.
    ``kind``: "none" / "shared" ((nb,)) / "per_pixel" ((M, nb), 15 % zeros over NaN observations) weights; ``prior``: "none" /
    "shared" ((n,)) / "per_pixel" ((M, n), 20 % zero weights over NaN means), sigma = ``prior_sigma`` of the range.
    Planted pixels from ``at`` (M >= at + 5): +0 a start outside its box, an unread NaN in component 1's entry of a shared
    column and (fitted) an unread NaN in frac[:, V - 1]; +1 a NaN fixed parameter in the last component (dead); +2 a negative
    weight (per-pixel weights; dead); +3 an infeasible start (fitted, V >= 3; dead, cost +inf); +4 a given fraction of -0.1
    (given; dead).  -> dict of mix_call's / refine_mix_defined's arguments, ``truth`` (V, M, 27), ``a`` (M, V), ``planted``"""
    from spart_amd import workloads
    rng = np.random.default_rng(seed)
    names = list(shared) + list(local)
    free, (lo, hi) = cols_of(names), bounds_of(names)
    Fs, Fl = len(shared), len(local)
    F = Fs + Fl
    act = None if active is None else np.asarray(active, dtype=np.int32).reshape(V, Fl)
    kindu, name, comp, _ = rmd.maps_defined(V, Fs, Fl, act, fit)
    n, nm = kindu.size, int((kindu != rmd.FRACTION).sum())
    truth = np.stack([workloads.lhs_params(M, "full", seed=seed + 1000 * v) for v in range(V)])
    truth[1:, :, free[:Fs]] = truth[0][None][:, :, free[:Fs]]
    a = rng.dirichlet(np.full(V, 3.0), M)
    if last_below is not None:
        a[:, V - 1] = rng.uniform(0.0, last_below, M)
        a[:, :V - 1] *= ((1.0 - a[:, V - 1]) / a[:, :V - 1].sum(axis=1))[:, None]
    fwd = (srf_forward_of if srf else forward_of)(torch, eng, column)
    with np.errstate(all="ignore"):
        Yt = fwd(truth.reshape(V * M, 27)).reshape(V, M, -1)
    Yt = np.where(np.isfinite(Yt), Yt, 0.3)
    obs = np.einsum("mv,vmj->mj", a, Yt) * (1.0 + noise * rng.normal(size=Yt.shape[1:]))
    nb = obs.shape[1]
    base = truth.copy()
    mv = rng.uniform(-move, move, (V, M, F)) * (hi - lo)
    mv[:, :, :Fs] = mv[0][None][:, :, :Fs]                            # one start per shared name
    base[:, :, free] = rd.clip_defined(truth[:, :, free] + mv, lo, hi)
    frac = 0.8 * a + 0.2 / V if fit else a.copy()
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 2, nb)
        w[rng.random(nb) < 0.2] = 0.0
        w[0] = w[0] or 1.0
    elif kind == "per_pixel":
        w = 10.0 ** rng.uniform(-1, 2, (M, nb))
        w[rng.random((M, nb)) < 0.15] = 0.0
        w[:, 1] = np.where(w[:, 1] == 0.0, 1.0, w[:, 1])
    planted = set()
    if M >= at + 5:
        base[0, at, free[0]] = hi[0] + 0.5 * (hi[0] - lo[0])
        if V > 1 and Fs:
            base[1, at, free[0]] = np.nan
        if fit:
            frac[at, V - 1] = np.nan
        base[V - 1, at + 1, 20 if 20 not in free else 26] = np.nan
        planted.add(at + 1)
        if kind == "per_pixel":
            w[at + 2, nb // 2] = -1.0
            planted.add(at + 2)
        if fit and V >= 3:
            frac[at + 3, :2] = 0.8
            planted.add(at + 3)
        if not fit:
            frac[at + 4, 0] = -0.1
            planted.add(at + 4)
    if kind == "per_pixel":
        obs[w == 0.0] = np.nan                                        # zero weights over NaN observations
    mean = weight = None
    if prior != "none":
        wid = np.concatenate([(hi - lo)[name[:nm]], np.ones(n - nm)])
        t0 = np.stack([a[:, comp[u]] if kindu[u] == rmd.FRACTION else truth[max(comp[u], 0), :, free[name[u]]] for u in range(n)], axis=1)
        shape = (M, n) if prior == "per_pixel" else (n,)
        mean = (t0 if prior == "per_pixel" else t0[0]) + 0.1 * rng.normal(size=shape) * wid
        weight = np.array(np.broadcast_to(1.0 / (prior_sigma * wid) ** 2, shape))
        if prior == "per_pixel":
            zero = rng.random(shape) < 0.2
            mean, weight = np.where(zero, np.nan, mean), np.where(zero, 0.0, weight)
    return dict(base=base, shared=free[:Fs], local=free[Fs:], lo=lo, hi=hi, obs=obs, frac=frac, active=act, fit=fit, w=w, mean=mean,
                weight=weight, lambda0=lambda0, truth=truth, a=a, planted=planted)


def defined_mix(torch, eng, case, column, n_iter, srf=False, history=None, **kw):
    fwd = (srf_forward_of if srf else forward_of)(torch, eng, COLUMNS[column])
    extra = {} if case.get("lambda0") is None else {"lambda0": case["lambda0"]}
    return rmd.refine_mix_defined(case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], fwd, case["frac"],
                                  active=case["active"], fit_fractions=case["fit"], weights=case["w"], n_iter=n_iter,
                                  prior_mean=case["mean"], prior_weight=case["weight"], history=history, **extra, **kw)


def call_mix(torch, eng, case, column, n_iter, **kw):
    rc, got = mix_call(torch, eng, case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["obs"], case["frac"],
                       case["active"], case["fit"], case["w"], case["mean"], case["weight"], column=column, n_iter=n_iter,
                       lambda0=case.get("lambda0") or 0.0, **kw)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    return got


def not_vacuous(ref, case, n_iter, what):
    """the conditions on the DEFINITION's output that keep a random case from being vacuous: of the pixels without a planted
    fault at least 85 % are live, and with n_iter >= 1 at least half accept a step and at least one rejects one"""
    clean = np.ones(ref["n_accept"].size, dtype=bool)
    clean[list(case["planted"])] = False
    na = ref["n_accept"][clean]
    live, acc, rej = float((na >= 0).mean()), float((na >= 1).mean()), int(((na >= 0) & (na < n_iter)).sum())
    print(f"[refine_mix] {what}: n_iter {n_iter}: live {live:.2f}, accepted {acc:.2f}, rejecting {rej} of {na.size}")
    assert live >= 0.85, (what, live)
    assert n_iter == 0 or (acc >= 0.5 and rej >= 1), (what, acc, rej)
    alive = ref["n_accept"] >= 0
    assert (ref["cost"][alive] <= ref["cost0"][alive]).all(), what
    assert all(ref["n_accept"][m] == -1 for m in case["planted"]), (what, ref["n_accept"][sorted(case["planted"])])


def check_mix(torch, eng, case, column, n_iter, what, **kw):
    """the definition's non-vacuity first, then the library against the definition, bit for bit -> (ref, got)"""
    ref = defined_mix(torch, eng, case, column, n_iter, srf=kw.get("band_model", 0) == 1)
    not_vacuous(ref, case, n_iter, what)
    got = call_mix(torch, eng, case, column, n_iter, **kw)
    for k in OUTS:
        assert same(got[k], ref[k]), (what, k, int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()))
    return ref, got
