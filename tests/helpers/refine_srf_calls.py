"""What the GPU tests of spart_refine_srf share beside helpers/refine_calls.py: the forward model the definition
tools/refine_defined.py is given (the engine's float64 pruned call with ONE *_srf output, configured like the fit), the raw
C-ABI caller of either entry point with every member of spart_refine_opt, the case builder and the comparison."""
import ctypes

import numpy as np

from helpers.refine_calls import COLUMNS, FILL, GUARD, OUTS, bounds_of, cols_of, rd, same

L8, S3 = "LANDSAT8-OLI", "Sentinel3A-OLCI"


def srf_forward_of(torch, eng, column, lidf="literal", nlayers=None):
    """rows (R, 27) -> (R, nb): ``column`` + "_srf" of Engine.run(float64, prune=True), the only SRF output asked for"""
    name = column + "_srf"

    def forward(rows):
        P = torch.as_tensor(np.ascontiguousarray(rows.T), device=eng.device)
        return eng.run(P, "float64", prune=True, lidf=lidf, nlayers=nlayers, materialize=[name])[name].cpu().numpy()
    return forward


def aligned_olci():
    """the packaged 21-band OLCI with its SRF columns put in the order of its band centres (align_srf): a sensor_info= dict"""
    import spart_amd
    from spart_amd import tables
    return spart_amd.align_srf(tables.load_sensor_info(S3))


def raw_refine(torch, eng, entry, base, free, lo, hi, obs, w=None, mean=None, weight=None, column=0, n_iter=2, lidf="literal",
               nlayers=None, guard=False):
    """One ``entry`` (spart_refine / spart_refine_srf) through ctypes -> (rc, dict of numpy outputs), every output pre-filled
    with FILL.  ``mean`` / ``weight``: the prior, (F,) or (M, F), or None; ``guard``: GUARD bytes of 0xFF behind the workspace
    must survive.  The workspace is sized by spart_refine_workspace_bytes for either entry."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, f, nb = base.shape[0], len(free), obs.shape[1]
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt, ot, wt, mt, pt = up(base.T), up(obs), up(w), up(mean), up(weight)
    full = lambda shape, dt=torch.float64: torch.full(shape, int(FILL) if dt is torch.int32 else FILL, dtype=dt, device=dev)  # noqa: E731
    out = {"x": full((m, f)), "cost": full((m,)), "cost0": full((m,)), "std": full((m, f)), "n_accept": full((m,), torch.int32),
           "y": full((m, nb))}
    opt = _lib.SpartRefineOpt(column=column, n_iter=n_iter, weights_per_obs=1 if (w is not None and np.ndim(w) == 2) else 0,
                              fast_prelude=1 if lidf == "newton" else 0, nlayers=0 if nlayers is None else nlayers,
                              prior_per_obs=int(mean is not None and np.ndim(mean) == 2),
                              prior_mean=None if mt is None else mt.data_ptr(), prior_weight=None if pt is None else pt.data_ptr())
    need = int(eng.lib.spart_refine_workspace_bytes(eng.ctx, m, f))
    assert need > 0
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=dev) if guard else torch.empty(need, dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    rc = getattr(eng.lib, entry)(eng.ctx, m, (_lib.vp * 27)(*[Bt[i].data_ptr() for i in range(27)]), f,
                                 fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), lo.ctypes.data_as(_lib.c_dp), hi.ctypes.data_as(_lib.c_dp),
                                 ot.data_ptr(), None if wt is None else wt.data_ptr(), ctypes.byref(opt),
                                 *[out[k].data_ptr() for k in OUTS], ws.data_ptr(), ctypes.c_size_t(need),
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[need:] == 0xFF).all()), "bytes behind the workspace were written"
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def make_srf_case(torch, eng, names, M, column, kind, prior, seed):
    """refine_calls.make_case with the SRF column as the observed quantity, and a prior: truth = LHS rows; obs = the SRF model at
    the truth, 1 % noise; starts moved up to 10 % of the range.  ``kind``: "none" / "shared" / "per_observation" band weights;
    ``prior``: "none" / "shared" ((F,)) / "per_observation" ((M, F), about 20 % zero weights over NaN means).
    Planted with per-observation weights and M >= 63: 3 an unmasked NaN observation (dead), 5 a negative weight (dead), 6 a NaN
    observation under a zero weight (alive).  -> (base, free, lo, hi, obs, w, mean, weight)"""
    from spart_amd import workloads
    rng = np.random.default_rng(seed)
    free, (lo, hi) = cols_of(names), bounds_of(names)
    F = len(free)
    truth = workloads.lhs_params(M, "full", seed=seed)
    with np.errstate(all="ignore"):
        obs = srf_forward_of(torch, eng, column)(truth)
    obs = np.where(np.isfinite(obs), obs, 0.3) * (1.0 + 0.01 * rng.normal(size=obs.shape))
    nb = obs.shape[1]
    base = truth.copy()
    base[:, free] = rd.clip_defined(truth[:, free] + rng.uniform(-0.1, 0.1, (M, F)) * (hi - lo), lo, hi)
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 2, nb)
        w[rng.random(nb) < 0.2] = 0.0
        w[0] = w[0] or 1.0                                           # (at least one band counts)
    elif kind == "per_observation":
        w = 10.0 ** rng.uniform(-1, 2, (M, nb))
        w[rng.random((M, nb)) < 0.15] = 0.0
        w[:, 1] = np.where(w[:, 1] == 0.0, 1.0, w[:, 1])             # (at least one band counts in every row)
        obs[w == 0.0] = np.nan                                       # zero weights over NaN observations
        if M >= 63:
            w[3, nb // 2], obs[3, nb // 2] = 1.0, np.nan
            w[5, 0] = -1.0
            w[6, nb - 1], obs[6, nb - 1] = 0.0, np.nan
    mean = weight = None
    if prior != "none":
        shape = (M, F) if prior == "per_observation" else (F,)
        mean = (truth[:, free] if prior == "per_observation" else truth[0, free]) + 0.1 * rng.normal(size=shape) * (hi - lo)
        weight = np.array(np.broadcast_to(1.0 / (0.1 * (hi - lo)) ** 2, shape))
        if prior == "per_observation":
            zero = rng.random(shape) < 0.2
            mean, weight = np.where(zero, np.nan, mean), np.where(zero, 0.0, weight)
    return base, free, lo, hi, obs, w, mean, weight


def defined_srf(torch, eng, case, column, n_iter, lidf="literal", nlayers=None):
    base, free, lo, hi, obs, w, mean, weight = case
    return rd.refine_defined(base, free, lo, hi, obs, srf_forward_of(torch, eng, COLUMNS[column], lidf, nlayers), weights=w, n_iter=n_iter,
                             prior_mean=mean, prior_weight=weight)


def mismatches(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return "shape" if a.shape != b.shape else int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def assert_same(got, ref, what, keys=OUTS):
    for k in keys:
        assert same(got[k], ref[k]), (what, k, mismatches(got[k], ref[k]))


def call_srf(torch, eng, case, column, n_iter, lidf="literal", nlayers=None, guard=False, entry="spart_refine_srf"):
    base, free, lo, hi, obs, w, mean, weight = case
    rc, got = raw_refine(torch, eng, entry, base, free, lo, hi, obs, w, mean, weight, column=column, n_iter=n_iter, lidf=lidf,
                         nlayers=nlayers, guard=guard)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    return got
