"""What the GPU tests of spart_refine's Gaussian prior share beside helpers/refine_calls.py: the raw C-ABI caller with the
prior members of spart_refine_opt, the prior builder with its planted rows, and the comparison with the definition."""
import ctypes

import numpy as np

from helpers.refine_calls import COLUMNS, FILL, GUARD, OUTS, forward_of, rd, same


def prior_call(torch, eng, base, free, lo, hi, obs, w=None, mean=None, weight=None, per_obs=None, column=0, n_iter=3, guard=False):
    """refine_calls.refine_call with opt.prior_mean / prior_weight / prior_per_obs: ``mean`` / ``weight`` numpy arrays or None
    (a NULL pointer each); ``per_obs``: the value to pass in place of the arrays' own (ndim == 2) -> (rc, dict of outputs)"""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, f, nb = base.shape[0], len(free), obs.shape[1]
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt, ot, wt, mt, pt = up(base.T), up(obs), up(w), up(mean), up(weight)
    full = lambda shape, dt=torch.float64: torch.full(shape, int(FILL) if dt is torch.int32 else FILL, dtype=dt, device=dev)  # noqa: E731
    out = {"x": full((m, f)), "cost": full((m,)), "cost0": full((m,)), "std": full((m, f)), "n_accept": full((m,), torch.int32),
           "y": full((m, nb))}
    if per_obs is None:
        per_obs = int(any(a is not None and np.ndim(a) == 2 for a in (mean, weight)))
    opt = _lib.SpartRefineOpt(column=column, n_iter=n_iter, weights_per_obs=1 if (w is not None and np.ndim(w) == 2) else 0,
                              prior_per_obs=per_obs, prior_mean=None if mt is None else mt.data_ptr(),
                              prior_weight=None if pt is None else pt.data_ptr())
    need = int(eng.lib.spart_refine_workspace_bytes(eng.ctx, m, f))
    assert need > 0
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=dev) if guard else torch.empty(need, dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    rc = eng.lib.spart_refine(eng.ctx, m, (_lib.vp * 27)(*[Bt[i].data_ptr() for i in range(27)]), f,
                              fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), lo.ctypes.data_as(_lib.c_dp), hi.ctypes.data_as(_lib.c_dp),
                              ot.data_ptr(), None if wt is None else wt.data_ptr(), ctypes.byref(opt),
                              *[out[k].data_ptr() for k in OUTS], ws.data_ptr(), ctypes.c_size_t(need),
                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[need:] == 0xFF).all()), "bytes behind the workspace were written"
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def make_prior(M, free, lo, hi, seed, per_obs):
    """means = the truth of make_case(seed) + noise of 10 % of the range, sigma = 10 % of the range; per observation: (M, F)
    with about 20 % zero weights (NaN means under them); shared: (F,), the truth being row 0's"""
    from spart_amd import workloads
    rng = np.random.default_rng(seed + 4242)
    truth = workloads.lhs_params(M, "full", seed=seed)[:, free]
    shape = (M, len(free)) if per_obs else (len(free),)
    mean = (truth if per_obs else truth[0]) + 0.1 * rng.normal(size=shape) * (hi - lo)
    sigma = np.broadcast_to(0.1 * (hi - lo), shape)
    weight = 1.0 / (sigma * sigma)
    if per_obs:
        zero = rng.random(shape) < 0.2
        mean, weight = np.where(zero, np.nan, mean), np.where(zero, 0.0, weight)
    return np.array(mean), np.array(weight)


def check_prior_against_definition(torch, eng, case, mean, weight, column, n_iter, what, guard=False):
    base, free, lo, hi, obs, w = case
    ref = rd.refine_defined(base, free, lo, hi, obs, forward_of(torch, eng, COLUMNS[column]), weights=w, n_iter=n_iter,
                            prior_mean=mean, prior_weight=weight)
    rc, got = prior_call(torch, eng, base, free, lo, hi, obs, w, mean, weight, column=column, n_iter=n_iter, guard=guard)
    assert rc == 0, (what, eng.lib.spart_last_error(eng.ctx))
    for k in OUTS:
        assert same(got[k], ref[k]), (what, k, int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()))
    return ref, got
