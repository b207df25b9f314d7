"""The DEFINITION of spart_refine_leaf (include/spart_hip.h): spart_refine's bounded Levenberg-Marquardt fit of a few of the
nine leaf parameters against measured leaf reflectance and / or transmittance on the 2001-band grid, in numpy, every sum and
solve in one pinned order.  It is refine_defined.py's text with two substitutions: the rows of an evaluation are leaves and Y is
their (refl, tran) spectra, and every sum over the bands is 64 lane partials plus a fixed join (partials_defined,
join_defined).  The forward model is a callable, so that the same text serves against the g++ build of the leaf model
(tests/test_refine_leaf_host.py: bit for bit), against the oracle and against Engine.prospect (tests/test_gpu_refine_leaf.py).

Band sums.  Partial p_l, l = 0 ... 63, starts at 0.0 and takes the bands i = l, l + 64, ... < 2001 in ascending order; at each
band the reflectance term first, then the transmittance term; a term is skipped if its array is absent or its weight is 0.
Join: for d = 32, 16, 8, 4, 2, 1: p_l = p_l + p_(l + d) for l < d; the sum is p_0.  The prior's terms come after the join.
"""
import numpy as np

import refine_defined as rd

NWL, NPAR, MAX_F, LANES = 2001, 9, 9, 64
PASSES = (NWL + LANES - 1) // LANES


def by_pass(a, fill):
    """(M, 2001, ...) -> (M, PASSES, 64, ...): band 64 k + l at [k, l]; the 47 places past band 2000 hold ``fill``"""
    a = np.asarray(a, dtype=np.float64)
    pad = np.full((a.shape[0], PASSES * LANES - NWL) + a.shape[2:], fill, dtype=np.float64)
    return np.concatenate([a, pad], axis=1).reshape((a.shape[0], PASSES, LANES) + a.shape[2:])


def join_defined(p):
    """(M, 64, ...) lane partials -> (M, ...): for d = 32 ... 1: p_l = p_l + p_(l + d) for l < d"""
    p = np.array(p, dtype=np.float64, copy=True)
    d = LANES // 2
    with np.errstate(all="ignore"):
        while d >= 1:
            p[:, :d] = p[:, :d] + p[:, d:2 * d]
            d //= 2
    return p[:, 0]


def leaf_weights_defined(weights, given, M):
    """the weights of one observation array: absent array -> all 0 (every term skipped); none -> 1; (2001,) or (M, 2001)"""
    if not given:
        if weights is not None:
            raise ValueError("weights for an observation array that is not given")
        return np.zeros((M, NWL))
    return rd.weights_defined(weights, M, NWL)


def cost_defined(Y0, obs, w):
    """the band part of the trial cost: Y0, obs, w are (refl, tran) pairs of (M, 2001).  Per lane, per band ascending, refl then
    tran: skip w == 0, else d = Y0 - obs, c = c + (w d) d.  -> (c (M,), (d_refl, d_tran))"""
    M = Y0[0].shape[0]
    p = np.zeros((M, LANES))
    with np.errstate(all="ignore"):
        ds = [Y0[s] - obs[s] for s in (0, 1)]
        wp = [by_pass(w[s], 0.0) for s in (0, 1)]
        dp = [by_pass(ds[s], 0.0) for s in (0, 1)]
        for k in range(PASSES):
            for s in (0, 1):
                p = np.where(wp[s][:, k] == 0.0, p, p + (wp[s][:, k] * dp[s][:, k]) * dp[s][:, k])
    return join_defined(p), ds


def normal_defined(J, r, w):
    """the band sums of the normal equations: J, r, w are (refl, tran) pairs, J (M, 2001, F), r and w (M, 2001) -> packed
    (M, F (F + 1) / 2 + F): the lower triangle of A (entry (a, b), a >= b: + (w J_a) J_b), then g (+ (w J_a) r)"""
    M, _, F = J[0].shape
    ia, ib = rd.packed_pairs(F)
    nt = ia.size
    p = np.zeros((M, LANES, nt + F))
    with np.errstate(all="ignore"):
        wp = [by_pass(w[s], 0.0) for s in (0, 1)]
        Jp = [by_pass(J[s], 0.0) for s in (0, 1)]
        rp = [by_pass(r[s], 0.0) for s in (0, 1)]
        for k in range(PASSES):
            for s in (0, 1):
                skip = (wp[s][:, k] == 0.0)[:, :, None]
                wj = wp[s][:, k, :, None] * Jp[s][:, k]                          # (M, 64, F): w J_a
                term = np.concatenate([wj[:, :, ia] * Jp[s][:, k][:, :, ib], wj * rp[s][:, k, :, None]], axis=2)
                p = np.where(skip, p, p + term)
    return join_defined(p)


def refine_leaf_defined(leaf, free, lo, hi, obs_refl, obs_tran, forward, w_refl=None, w_tran=None, n_iter=20, rel_step=1e-3,
                        lambda0=1e-2, history=None, prior_mean=None, prior_weight=None, spectra=True):
    """leaf (M, 9) start rows (Cab, Cdm, Cw, Cs, Cca, Cant, N, PROT, CBC); free: F distinct column numbers 0 ... 8; lo, hi (F,);
    obs_refl, obs_tran (M, 2001) or None (not both); w_refl, w_tran None, (2001,) or (M, 2001), only for a given array (a weight
    of exactly 0 skips the band, the observation may be NaN there); forward(rows (R, 9)) -> (refl, tran), each (R, 2001).
    prior_mean, prior_weight as for refine_defined.
    -> dict x (M, F), cost, cost0 (M,), std (M, F), n_accept (M,) int32 (-1: a dead leaf) and, with ``spectra``, y_refl, y_tran
    (M, 2001): the spectra at x from one closing call of ``forward``.
    ``history``: an optional list that receives (x, cost) after every decision (the prefix property)."""
    leaf = np.ascontiguousarray(leaf, dtype=np.float64)
    free = [int(f) for f in free]
    F, M = len(free), leaf.shape[0]
    if leaf.ndim != 2 or leaf.shape[1] != NPAR:
        raise ValueError(f"leaf has shape {leaf.shape}, expected (M, {NPAR})")
    if not 1 <= F <= MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= NPAR:
        raise ValueError("free: 1 ... 9 distinct column numbers of 0 ... 8")
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    if not 0 <= int(n_iter) <= rd.MAX_ITER:
        raise ValueError("n_iter: 0 ... 100")
    if obs_refl is None and obs_tran is None:
        raise ValueError("obs_refl and obs_tran are both None")
    given = [obs_refl is not None, obs_tran is not None]
    obs = [np.ascontiguousarray(o, dtype=np.float64) if g else np.zeros((M, NWL)) for o, g in zip((obs_refl, obs_tran), given)]
    for o in obs:
        if o.shape != (M, NWL):
            raise ValueError(f"an observation array has shape {o.shape}, expected ({M}, {NWL})")
    w = [leaf_weights_defined(ws, g, M) for ws, g in zip((w_refl, w_tran), given)]
    bad = rd.bad_weights_defined(w[0]) | rd.bad_weights_defined(w[1])
    mu, pw = rd.prior_defined(prior_mean, prior_weight, M, F)
    if pw is not None:
        bad = bad | rd.bad_weights_defined(pw)
    h = rel_step * (hi - lo)
    x = rd.clip_defined(leaf[:, free], lo, hi)
    t = x.copy()
    c = np.full(M, np.inf)
    cost0 = np.full(M, np.nan)
    lam = np.full(M, float(lambda0))
    n_accept = np.zeros(M, dtype=np.int32)
    dead = np.zeros(M, dtype=bool)
    packed = np.zeros((M, F * (F + 1) // 2 + F))

    def rows_of(point, sh):
        rows = np.repeat(leaf[None], F + 1 if sh is not None else 1, axis=0)        # p_0, p_1 ... p_F
        rows[:, :, free] = point[None]
        if sh is not None:
            with np.errstate(all="ignore"):
                for f in range(F):
                    rows[f + 1, :, free[f]] = point[:, f] + sh[:, f]
        return rows.reshape(-1, NPAR)

    def spectra_of(rows, n):
        Y = forward(rows)
        return [np.asarray(Y[s], dtype=np.float64).reshape(n, M, NWL) for s in (0, 1)]

    for it in range(int(n_iter) + 1):
        sh = rd.step_sign(t, h, hi) * h
        Y = spectra_of(rows_of(t, sh), F + 1)
        ct, d = cost_defined([Y[0][0], Y[1][0]], obs, w)
        if pw is not None:
            ct, e = rd.prior_cost_defined(ct, t, mu, pw)
        with np.errstate(all="ignore"):
            accept = (ct < c) & ~dead & ~bad
        if it == 0:
            cost0 = ct.copy()
            dead = ~accept
            c = np.where(dead, ct, c)
            n_accept[dead] = -1
        if accept.any():
            with np.errstate(all="ignore"):
                J = [np.moveaxis((Y[s][1:] - Y[s][0][None]) / sh.T[:, :, None], 0, 2) for s in (0, 1)]       # (M, 2001, F)
            new = normal_defined(J, d, w)
            if pw is not None:
                new = rd.prior_normal_defined(new, e, pw)
            packed = np.where(accept[:, None], new, packed)
        x = np.where(accept[:, None], t, x)
        c = np.where(accept, ct, c)
        if it > 0:
            lam = np.where(dead, lam, rd.lambda_defined(lam, accept))
            n_accept = n_accept + accept.astype(np.int32)
        if history is not None:
            history.append((x.copy(), c.copy()))
        if it == int(n_iter):
            break
        t = np.where(dead[:, None], t, rd.propose_defined(packed, lam, x, lo, hi))
    std = np.where(dead[:, None], np.nan, rd.std_defined(packed, F))
    res = {"x": x, "cost": c, "cost0": cost0, "std": std, "n_accept": n_accept}
    if spectra:
        Yx = spectra_of(rows_of(x, None), 1)
        res["y_refl"], res["y_tran"] = Yx[0][0], Yx[1][0]
    return res
