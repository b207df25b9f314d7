"""The DEFINITION of spart_sample (include/spart_hip.h) in numpy: the affine-invariant ensemble sampler (Goodman & Weare 2010;
the two-half-ensemble stretch move of emcee, Foreman-Mackey et al. 2013) of the posterior of a few of the 27 SPART parameters
per observation, with the forward model as the likelihood and a box as the support.  All arithmetic is float64, every written
operation is one rounded operation (numpy rounds every ufunc once and never fuses a multiply with an add), every sum in one
pinned order:

  numbers   Philox4x32-10 blocks, a pure function of (seed, global observation g, step s, walker k, draw d)   (philox4x32, block)
  start     x_kf = a_f + u (b_f - a_f) in the start box clipped to the bounds, or the given ensemble           (start_defined)
  step      per half h: partner j, t = (a - 1) u1 + 1, z = (t t) / a, y = x_j + z (x_k - x_j); inside the box or rejected;
            q = z^(F-1) exp(-((c' - c) / (2 T))); accept iff inside and u2 < q                      (propose_defined, accept_defined)
  best      first-seen strict minimum of the cost                                                             (best_defined)
  kept      chain rows and, with walkers ascending, S_f += e_f, Q_ab += e_a e_b (e = x - x0)                   (sums_defined)
  finish    mean = x0 + S / n, cov = Q / n - (S_a / n)(S_b / n), std = sqrt(cov_ff)                            (finish_defined)

``forward(rows (R, 27)) -> (R, nb)`` is the chosen sensor column, as in refine_defined.py, whose cost, prior and weight rules
are imported, not restated.  exp is numpy's: the one operation not pinned to the bit; every decision's margin |u2 - q| / q is
returned so that a test can require it to be large before it compares decisions."""
import numpy as np

from refine_defined import (MAX_F, bad_weights_defined, clip_defined, cost_defined, packed_pairs, prior_cost_defined, prior_defined,
                            weights_defined)

WALKERS = (8, 16, 32, 64)
MAX_STEPS = 1 << 20
FLOAT_OUTS = ("mean", "cov", "std", "best_x", "best_cost", "chain", "chain_cost", "last", "last_cost")
OUTS = ("mean", "cov", "std", "best_x", "best_cost", "n_accept", "status", "chain", "chain_cost", "last", "last_cost")

_M0, _M1, _W0, _W1, _MASK = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011): counter words and key words (arrays or scalars below 2^32) -> four uint64 arrays
    holding the 32-bit output words"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1)))
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
    return c0, c1, c2, c3


def u53(a, b):
    """((a >> 5) 2^26 + (b >> 6)) 2^-53: exact, in [0, 1)"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) * (2.0 ** -53)


def block(seed, g, s, k, d):
    """the block of (seed, observation g, step s, walker k, draw d): key (seed lo, seed hi), counter (g lo, g hi, s mod 2^32,
    (k << 8) | d)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.asarray(g, dtype=np.uint64)
    return philox4x32(g & _MASK, g >> _S32, np.uint64(int(s) & 0xFFFFFFFF), (np.asarray(k, dtype=np.uint64) << np.uint64(8)) | np.uint64(d),
                      seed & 0xFFFFFFFF, seed >> 32)


def start_defined(seed, g, s, W, x0, r, lo, hi):
    """x0, r (M, F), g (M,) -> the start ensemble (M, W, F): a = max(lo, x0 - r), b = min(hi, x0 + r), x = a + u (b - a)"""
    M, F = x0.shape
    k = np.arange(W)[None, :, None]
    w = block(seed, np.asarray(g)[:, None, None], s, k, np.arange(F, dtype=np.uint64)[None, None, :])
    u = u53(w[0], w[1])
    with np.errstate(all="ignore"):
        a = np.maximum(lo, x0 - r)[:, None, :]
        b = np.minimum(hi, x0 + r)[:, None, :]
        return a + u * (b - a)


def propose_defined(seed, g, s, h, W, x, a, lo, hi):
    """The half-step h of step s: x (M, W, F) -> y (M, W/2, F), z, zp, u2 (M, W/2), inside (M, W/2) bool, partner j"""
    M, _, F = x.shape
    H = W // 2
    k = h * H + np.arange(H)[None, :]
    gg = np.asarray(g)[:, None]
    w = block(seed, gg, s, k, 0)
    u1 = u53(w[0], w[1])
    j = (1 - h) * H + (w[2] % np.uint64(H)).astype(np.int64)
    w = block(seed, gg, s, k, 1)
    u2 = u53(w[0], w[1])
    with np.errstate(all="ignore"):
        t = (a - 1.0) * u1 + 1.0
        z = (t * t) / a
        xk = x[:, h * H:(h + 1) * H, :]
        xj = np.take_along_axis(x, j[:, :, None], axis=1)
        y = xj + z[:, :, None] * (xk - xj)
        inside = ((lo <= y) & (y <= hi)).all(axis=2)
        zp = np.ones_like(z)
        for _ in range(F - 1):
            zp = zp * z
    return y, z, zp, u2, inside, j


def accept_defined(inside, u2, zp, cnew, cold, temperature):
    """-> (accept, q): q = zp exp(-((c' - c) / (2 T))); accept iff inside and u2 < q (a NaN never accepts)"""
    with np.errstate(all="ignore"):
        q = zp * np.exp(-((cnew - cold) / (2.0 * temperature)))
        return inside & (u2 < q), q


def best_defined(best_x, best_cost, x, c, ks):
    """for k in ks ascending: c_k < best_cost, strictly, takes the walker (in place)"""
    for k in ks:
        with np.errstate(all="ignore"):
            better = c[:, k] < best_cost
        best_cost[better] = c[better, k]
        best_x[better] = x[better, k]


def sums_defined(S, Q, x, x0):
    """walkers ascending: e = x_k - x0, S_f += e_f, Q_ab += e_a e_b for a >= b (packed, a (a + 1) / 2 + b)  (in place)"""
    ia, ib = packed_pairs(x.shape[2])
    with np.errstate(all="ignore"):
        for k in range(x.shape[1]):
            e = x[:, k, :] - x0
            S += e
            Q += e[:, ia] * e[:, ib]


def finish_defined(S, Q, x0, n):
    """n = (double)(n_keep W) -> mean (M, F), cov (M, F, F), std (M, F); nothing is clamped"""
    M, F = S.shape
    ia, ib = packed_pairs(F)
    n = np.float64(n)
    with np.errstate(all="ignore"):
        sn = S / n
        mean = x0 + sn
        cp = Q / n - sn[:, ia] * sn[:, ib]
        cov = np.empty((M, F, F))
        cov[:, ia, ib] = cp
        cov[:, ib, ia] = cp
        std = np.sqrt(cov[:, np.arange(F), np.arange(F)])
    return mean, cov, std


def check_options(F, W, n_steps, burn, thin, a, temperature, rel_init, step0, obs_offset):
    """the option checks of the call, in its order -> (a, temperature, rel_init) with the defaults 0 stands for, n_keep"""
    if W not in WALKERS or W < 2 * F:
        raise ValueError(f"W = {W}: one of {WALKERS} with W >= 2 F = {2 * F}")
    if not 1 <= n_steps <= MAX_STEPS or not 0 <= burn <= n_steps - 1 or thin < 1 or (n_steps - burn) // thin < 1:
        raise ValueError("n_steps 1 ... 2^20, burn 0 ... n_steps - 1, thin >= 1, (n_steps - burn) / thin >= 1")
    a = 2.0 if a == 0 else float(a)
    if not (np.isfinite(a) and a > 1.0):
        raise ValueError("a: 0 (= 2.0) or finite and > 1")
    temperature = 1.0 if temperature == 0 else float(temperature)
    if not (np.isfinite(temperature) and temperature > 0.0):
        raise ValueError("temperature: 0 (= 1.0) or finite and > 0")
    rel_init = 0.01 if rel_init == 0 else float(rel_init)
    if not (np.isfinite(rel_init) and rel_init > 0.0):
        raise ValueError("rel_init: 0 (= 0.01) or finite and > 0")
    if step0 < 0 or obs_offset < 0:
        raise ValueError("step0 and obs_offset >= 0")
    return a, temperature, rel_init, (n_steps - burn) // thin


def sample_defined(base, free, lo, hi, obs, forward, weights=None, prior_mean=None, prior_weight=None, W=8, n_steps=100, burn=0,
                   thin=1, a=0.0, temperature=0.0, rel_init=0.0, init_radius=None, init=None, step0=0, obs_offset=0, seed=0):
    """base (M, 27); free: F distinct column numbers; lo, hi (F,); obs (M, nb); weights None, (nb,) or (M, nb); prior_mean,
    prior_weight None or both (F,) or (M, F); init_radius None or (M, F); init None or (M, W, F).
    -> dict of the eleven outputs (OUTS) and, for the tests: ``margin`` (the smallest |u2 - q| / q of the decisions of living
    observations on proposals inside the box), ``n_accepted``, ``n_rejected`` (by u2), ``n_outside`` (those decisions counted)."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    free = [int(f) for f in free]
    F, (M, nb) = len(free), obs.shape
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not 1 <= F <= MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[1]:
        raise ValueError("free: 1 ... 16 distinct column numbers")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    W, n_steps, burn, thin, step0 = int(W), int(n_steps), int(burn), int(thin), int(step0)
    a, temperature, rel_init, n_keep = check_options(F, W, n_steps, burn, thin, a, temperature, rel_init, step0, int(obs_offset))
    H = W // 2
    w = weights_defined(weights, M, nb)
    dead = bad_weights_defined(w)
    mu, pw = prior_defined(prior_mean, prior_weight, M, F)
    if pw is not None:
        dead = dead | bad_weights_defined(pw)
    g = int(obs_offset) + np.arange(M, dtype=np.uint64)
    x0 = clip_defined(base[:, free], lo, hi)
    with np.errstate(all="ignore"):
        r = np.broadcast_to(rel_init * (hi - lo), (M, F)) if init_radius is None else np.asarray(init_radius, dtype=np.float64).reshape(M, F)
        dead = dead | ~(np.isfinite(r) & (r > 0.0)).all(axis=1)
        if init is None:
            x = start_defined(seed, g, step0, W, x0, r, lo, hi)
        else:
            x = np.array(init, dtype=np.float64).reshape(M, W, F)
            dead = dead | ~((lo <= x) & (x <= hi)).all(axis=(1, 2))

    def cost_of(points, ks):
        """the cost, prior included, of points (M, len(ks), F)"""
        n = points.shape[1]
        rows = np.repeat(base[:, None, :], n, axis=1)
        rows[:, :, free] = points
        Y = np.asarray(forward(rows.reshape(M * n, base.shape[1])), dtype=np.float64).reshape(M, n, nb)
        out = np.empty((M, n))
        for i in range(n):
            c, _ = cost_defined(Y[:, i, :], obs, w)
            if pw is not None:
                c, _ = prior_cost_defined(c, points[:, i, :], mu, pw)
            out[:, i] = c
        return out

    # (an observation that is dead already walks from x0: its rows stay valid and nothing reads them)
    x = np.where(dead[:, None, None], x0[:, None, :], x)
    c = np.empty((M, W))
    best_x, best_cost = np.full((M, F), np.nan), np.full(M, np.inf)
    for h in (0, 1):
        ks = range(h * H, (h + 1) * H)
        c[:, h * H:(h + 1) * H] = cost_of(x[:, h * H:(h + 1) * H, :], ks)
        best_defined(best_x, best_cost, x, c, ks)
    dead = dead | ~np.isfinite(c).all(axis=1)
    live = ~dead
    n_accept = np.zeros(M, dtype=np.int64)
    S, Q = np.zeros((M, F)), np.zeros((M, F * (F + 1) // 2))
    chain, chain_cost = np.full((M, n_keep, W, F), np.nan), np.full((M, n_keep, W), np.nan)
    margin, counts = np.inf, [0, 0, 0]
    for s in range(step0 + 1, step0 + n_steps + 1):
        for h in (0, 1):
            sl = slice(h * H, (h + 1) * H)
            y, z, zp, u2, inside, _ = propose_defined(seed, g, s, h, W, x, a, lo, hi)
            rows_y = np.where(inside[:, :, None], y, x[:, sl, :])
            cnew = cost_of(rows_y, range(h * H, (h + 1) * H))
            acc, q = accept_defined(inside, u2, zp, cnew, c[:, sl], temperature)
            with np.errstate(all="ignore"):
                dec = inside & live[:, None]
                mg = np.abs(u2 - q) / q
                if dec.any():
                    margin = min(margin, float(np.nanmin(np.where(dec, mg, np.inf))))
            counts[0] += int((acc & live[:, None]).sum())
            counts[1] += int((dec & ~acc).sum())
            counts[2] += int((~inside & live[:, None]).sum())
            x[:, sl, :] = np.where(acc[:, :, None], y, x[:, sl, :])
            c[:, sl] = np.where(acc, cnew, c[:, sl])
            n_accept += acc.sum(axis=1)
            best_defined(best_x, best_cost, x, c, range(h * H, (h + 1) * H))
        rel = s - step0
        if rel > burn and (rel - burn) % thin == 0:
            t = (rel - burn) // thin - 1
            if t < n_keep:
                chain[:, t], chain_cost[:, t] = x, c
                sums_defined(S, Q, x, x0)
    mean, cov, std = finish_defined(S, Q, x0, n_keep * W)
    res = {"mean": mean, "cov": cov, "std": std, "best_x": best_x, "best_cost": best_cost, "n_accept": n_accept,
           "status": np.where(dead, -1, 0).astype(np.int32), "chain": chain, "chain_cost": chain_cost, "last": x.copy(),
           "last_cost": c.copy()}
    for k in FLOAT_OUTS:
        res[k] = np.where(dead.reshape((M,) + (1,) * (res[k].ndim - 1)), np.nan, res[k])
    res["n_accept"] = np.where(dead, -1, n_accept)
    res.update(margin=margin, n_accepted=counts[0], n_rejected=counts[1], n_outside=counts[2])
    return res
