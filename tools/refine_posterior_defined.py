"""The DEFINITION of spart_refine_posterior (include/spart_hip.h): what the optimal-estimation fit of spart_refine knows about
a point -- the Jacobian of the sensor column, the posterior covariance (J^T W J + S_a^-1)^-1, the averaging kernel and its
trace, the degrees of freedom for signal -- in numpy, vectorised over the observations, every sum in one pinned order.  It is
the oracle of csrc/spart_refine_posterior.h the way tools/refine_defined.py is the oracle of csrc/spart_refine.h: the g++ build
of the functions (tests/test_refine_posterior_host.py) and the kernel (tests/test_gpu_refine_posterior.py) reproduce it bit for
bit.  Everything the two definitions share is imported from refine_defined, so `std` here IS std_defined's number and `cost`
IS the fit's cost.

Index conventions are refine_defined's: packed lower triangles in the order a (a + 1) / 2 + b, a >= b.  Z = L^-1 is lower
triangular and packed the same way: Z_kf at tri(k, f), k >= f.
"""
import numpy as np

from refine_defined import (MAX_F, bad_weights_defined, cholesky_defined, clip_defined, cost_defined, normal_defined,
                            packed_pairs, prior_cost_defined, prior_defined, step_sign, tri, weights_defined)

OUTS = ("x", "y", "jac", "cov", "ak", "std", "dfs", "cost", "nband", "status")


def inverse_lower_defined(L, F):
    """Z = L^-1, column f by std_defined's recurrence: z_k = ((k == f) - sum_{f <= i < k} L_ki z_i) / L_kk, i ascending.
    L packed (M, F(F+1)/2) -> Z packed (M, F(F+1)/2)"""
    Z = np.zeros_like(L)
    with np.errstate(all="ignore"):
        for f in range(F):
            for k in range(f, F):
                s = np.full(L.shape[0], 1.0 if k == f else 0.0)
                for i in range(f, k):
                    s = s - L[:, tri(k, i)] * Z[:, tri(i, f)]
                Z[:, tri(k, f)] = s / L[:, tri(k, k)]
    return Z


def cov_defined(Z, F):
    """cov = Z^T Z, the packed lower triangle: cov_ab (a >= b) is v = 0; for k = a ... F-1: v = v + Z_ka Z_kb"""
    ia, ib = packed_pairs(F)
    C = np.zeros_like(Z)
    with np.errstate(all="ignore"):
        for e, (a, b) in enumerate(zip(ia, ib)):
            v = np.zeros(Z.shape[0])
            for k in range(a, F):
                v = v + Z[:, tri(k, a)] * Z[:, tri(k, b)]
            C[:, e] = v
    return C


def full_defined(P, F):
    """packed lower triangle (M, F(F+1)/2) -> (M, F, F), the value of (a, b) copied to (b, a)"""
    out = np.zeros((P.shape[0], F, F))
    for a in range(F):
        for b in range(a + 1):
            out[:, a, b] = out[:, b, a] = P[:, tri(a, b)]
    return out


def avk_defined(cov, K):
    """ak_ab = 0; for c = 0 ... F-1: ak_ab = ak_ab + cov_ac K_cb.  cov, K full (M, F, F)"""
    F = cov.shape[1]
    ak = np.zeros_like(cov)
    with np.errstate(all="ignore"):
        for c in range(F):
            ak = ak + cov[:, :, c, None] * K[:, None, c, :]
    return ak


def trace_defined(ak):
    """dfs = 0; for a ascending: dfs = dfs + ak_aa"""
    d = np.zeros(ak.shape[0])
    with np.errstate(all="ignore"):
        for a in range(ak.shape[1]):
            d = d + ak[:, a, a]
    return d


def posterior_of_normal(Kp, pw, F):
    """From the packed data part K (M, F(F+1)/2) and the prior weights pw ((M, F) or None):
    -> (A packed, ok (M,), cov (M, F, F), ak (M, F, F), std (M, F), dfs (M,)); rows whose factorisation fails are NaN"""
    A = np.array(Kp, dtype=np.float64, copy=True)
    with np.errstate(all="ignore"):
        if pw is not None:
            for a in range(F):
                A[:, tri(a, a)] = np.where(pw[:, a] == 0.0, A[:, tri(a, a)], A[:, tri(a, a)] + pw[:, a])
        L, ok = cholesky_defined(A, F)
        Z = inverse_lower_defined(L, F)
        Cp = cov_defined(Z, F)
        cov = full_defined(Cp, F)
        ak = avk_defined(cov, full_defined(Kp, F))
        std = np.sqrt(np.stack([Cp[:, tri(f, f)] for f in range(F)], axis=1))
        dfs = trace_defined(ak)
    nan = ~ok
    return (A, ok, np.where(nan[:, None, None], np.nan, cov), np.where(nan[:, None, None], np.nan, ak),
            np.where(nan[:, None], np.nan, std), np.where(nan, np.nan, dfs))


def posterior_defined(base, free, lo, hi, obs, forward, weights=None, rel_step=1e-3, prior_mean=None, prior_weight=None):
    """base (M, 27) rows; free: F distinct column numbers; lo, hi (F,); obs (M, nb) or None; weights None, (nb,) or (M, nb);
    forward(rows (R, 27)) -> (R, nb) float64, the chosen sensor column; prior as refine_defined's.
    -> dict x (M, F), y (M, nb), jac (M, nb, F), cov, ak (M, F, F), std (M, F), dfs, cost (M,), nband, status (M,) int32
    (status 0 ok, 1 A not positive definite, -1 dead)."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    free = [int(f) for f in free]
    F, M = len(free), base.shape[0]
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not 1 <= F <= MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[1]:
        raise ValueError("free: 1 ... 16 distinct column numbers")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    h = rel_step * (hi - lo)
    x = clip_defined(base[:, free], lo, hi)
    sh = step_sign(x, h, hi) * h
    rows = np.repeat(base[None], F + 1, axis=0)                     # (F + 1, M, 27): p_0, p_1 ... p_F
    rows[:, :, free] = x[None]
    with np.errstate(all="ignore"):
        for f in range(F):
            rows[f + 1, :, free[f]] = x[:, f] + sh[:, f]
    Y = np.asarray(forward(rows.reshape(-1, base.shape[1])), dtype=np.float64)
    nb = Y.shape[1]
    Y = Y.reshape(F + 1, M, nb)
    w = weights_defined(weights, M, nb)
    bad = bad_weights_defined(w)
    mu, pw = prior_defined(prior_mean, prior_weight, M, F)
    if obs is None:
        c = np.zeros(M)
    else:
        c, _ = cost_defined(Y[0], np.ascontiguousarray(obs, dtype=np.float64).reshape(M, nb), w)
    if pw is not None:
        bad = bad | bad_weights_defined(pw)
        c, _ = prior_cost_defined(c, x, mu, pw)
    with np.errstate(all="ignore"):
        dead = bad | ~(c < np.inf)
        J = np.moveaxis((Y[1:] - Y[0][None]) / sh.T[:, :, None], 0, 2)               # (M, nb, F), every band
    Kp = normal_defined(J, np.zeros((M, nb)), w)[:, :F * (F + 1) // 2]
    _, ok, cov, ak, std, dfs = posterior_of_normal(Kp, pw, F)
    status = np.where(dead, -1, np.where(ok, 0, 1)).astype(np.int32)
    d3, d2 = dead[:, None, None], dead[:, None]
    return {"x": x, "y": Y[0].copy(), "jac": np.where(d3, np.nan, J), "cov": np.where(d3, np.nan, cov),
            "ak": np.where(d3, np.nan, ak), "std": np.where(d2, np.nan, std), "dfs": np.where(dead, np.nan, dfs), "cost": c,
            "nband": (w != 0.0).sum(axis=1).astype(np.int32), "status": status}
