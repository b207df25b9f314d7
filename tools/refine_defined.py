"""The DEFINITION of spart_refine (include/spart_hip.h): bounded Levenberg-Marquardt refinement of a few of the 27 SPART
parameters per observation, in numpy, vectorised over the observations, with every sum and solve in one pinned order.  It is
the oracle of csrc/spart_refine.h in the way lut_brute_force.summarise_defined is the oracle of spart_lut_summarise: the g++
build of the step functions (tests/test_refine_host.py) and the kernels (tests/test_gpu_refine.py) must reproduce it bit for
bit.  numpy rounds every ufunc once and never fuses a multiply with an add, which is the arithmetic the definition asks for
(float64, no FMA contraction, IEEE division and square root).

The optional Gaussian prior on the free parameters (prior_mean, prior_weight = 1 / sigma^2; optimal estimation) adds its terms
after the band sums: prior_cost_defined to the trial cost, prior_normal_defined to the diagonal of A and to g.

Index conventions.  A is symmetric and only its LOWER triangle is ever formed: entry (a, b), a >= b, is
sum_j (w_j J_ja) J_jb -- the weight multiplies the factor with the LARGER column number.  PACKED(F) lists the pairs in the
order a(a + 1)/2 + b; the packed vector of an observation is those F(F + 1)/2 sums followed by g_0 ... g_{F-1}.
"""
import numpy as np

LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12
MAX_F, MAX_ITER = 16, 100


def packed_pairs(F):
    """(ia, ib): the column numbers a >= b of the packed lower triangle, in the order a(a + 1)/2 + b"""
    ia = np.array([a for a in range(F) for b in range(a + 1)], dtype=np.int64)
    ib = np.array([b for a in range(F) for b in range(a + 1)], dtype=np.int64)
    return ia, ib


def tri(a, b):
    return a * (a + 1) // 2 + b


def clip_defined(v, lo, hi):
    """t = v; if t < lo: t = lo; if t > hi: t = hi  (a NaN stays a NaN)"""
    t = np.array(v, dtype=np.float64, copy=True)
    t = np.where(t < lo, lo, t)
    return np.where(t > hi, hi, t)


def weights_defined(weights, M, nb):
    """none / (nb,) / (M, nb) -> (M, nb) float64"""
    if weights is None:
        return np.ones((M, nb))
    w = np.asarray(weights, dtype=np.float64)
    if w.shape not in ((nb,), (M, nb)):
        raise ValueError(f"weights has shape {w.shape}, expected ({nb},) or ({M}, {nb})")
    return np.ascontiguousarray(np.broadcast_to(w, (M, nb)))


def bad_weights_defined(w):
    """per observation: a negative, NaN or infinite weight"""
    return (~(w >= 0.0) | np.isinf(w)).any(axis=1)


def cost_defined(Y0, obs, w):
    """step 3: c = 0; for j ascending: skip w_j == 0, else d = Y0_j - obs_j, c = c + (w_j d) d.  -> (c (M,), d (M, nb))"""
    M, nb = Y0.shape
    c = np.zeros(M)
    with np.errstate(all="ignore"):
        d = Y0 - obs
        for j in range(nb):
            c = np.where(w[:, j] == 0.0, c, c + (w[:, j] * d[:, j]) * d[:, j])
    return c, d


def normal_defined(J, r, w):
    """step 6, the sums: J (M, nb, F), r (M, nb), w (M, nb) -> packed (M, F(F+1)/2 + F): the lower triangle of A, then g.
    Bands of weight 0 are skipped in every sum (J and r may hold anything there)."""
    M, nb, F = J.shape
    ia, ib = packed_pairs(F)
    A = np.zeros((M, ia.size))
    g = np.zeros((M, F))
    with np.errstate(all="ignore"):
        for j in range(nb):
            skip = (w[:, j] == 0.0)[:, None]
            wj = w[:, j, None] * J[:, j, :]                        # w_j J_ja, one product per column
            A = np.where(skip, A, A + wj[:, ia] * J[:, j, ib])
            g = np.where(skip, g, g + wj * r[:, j, None])
    return np.concatenate([A, g], axis=1)


def cholesky_defined(Bp, F):
    """packed lower triangle (M, F(F+1)/2) -> (L packed, ok (M,)): textbook row order, sums over k ascending; a pivot
    !(s > 0) fails the observation (its L is then meaningless)"""
    L = np.array(Bp, dtype=np.float64, copy=True)
    ok = np.ones(L.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(F):
            for j in range(i + 1):
                s = L[:, tri(i, j)].copy()
                for k in range(j):
                    s = s - L[:, tri(i, k)] * L[:, tri(j, k)]
                if i == j:
                    ok &= s > 0.0
                    L[:, tri(i, i)] = np.sqrt(s)
                else:
                    L[:, tri(i, j)] = s / L[:, tri(j, j)]
    return L, ok


def propose_defined(packed, lam, x, lo, hi):
    """step 6, the solve: packed (M, P), lam (M,), x (M, F) -> the next trial t (M, F) = clip(x + delta)"""
    M, F = x.shape
    nt = F * (F + 1) // 2
    B = np.array(packed[:, :nt], dtype=np.float64, copy=True)
    g = packed[:, nt:]
    with np.errstate(all="ignore"):
        for a in range(F):
            Aaa = B[:, tri(a, a)]
            D = np.where(Aaa > 0.0, Aaa, 1.0)
            B[:, tri(a, a)] = Aaa + lam * D
        L, ok = cholesky_defined(B, F)
        d = np.zeros((M, F))
        for i in range(F):                                         # L y = -g
            s = -g[:, i]
            for k in range(i):
                s = s - L[:, tri(i, k)] * d[:, k]
            d[:, i] = s / L[:, tri(i, i)]
        for i in range(F - 1, -1, -1):                             # L^T delta = y
            s = d[:, i].copy()
            for k in range(i + 1, F):
                s = s - L[:, tri(k, i)] * d[:, k]
            d[:, i] = s / L[:, tri(i, i)]
        ok = ok & np.isfinite(d).all(axis=1)
        d = np.where(ok[:, None], d, 0.0)
        return clip_defined(x + d, lo, hi)


def std_defined(packed, F):
    """the linearised 1-sigma of every free parameter from the undamped A: Cholesky A = L L^T; for each f solve L z = e_f
    (z_k = 0 for k < f, z_k = ((k == f) - sum_{f <= i < k} L_ki z_i) / L_kk, i ascending); var_f = sum_{k >= f} z_k^2 in
    ascending k, std_f = sqrt(var_f).  All NaN when the factorisation fails."""
    M = packed.shape[0]
    L, ok = cholesky_defined(packed[:, :F * (F + 1) // 2], F)
    out = np.full((M, F), np.nan)
    with np.errstate(all="ignore"):
        for f in range(F):
            z = np.zeros((M, F))
            var = np.zeros(M)
            for k in range(f, F):
                s = np.full(M, 1.0 if k == f else 0.0)
                for i in range(f, k):
                    s = s - L[:, tri(k, i)] * z[:, i]
                z[:, k] = s / L[:, tri(k, k)]
                var = var + z[:, k] * z[:, k]
            out[:, f] = np.sqrt(var)
    return np.where(ok[:, None], out, np.nan)


def lambda_defined(lam, accept):
    """accept: max(lam / 10, 1e-12); reject: min(lam * 10, 1e12)"""
    return np.where(accept, np.maximum(lam / 10.0, LAMBDA_MIN), np.minimum(lam * 10.0, LAMBDA_MAX))


def step_sign(t, h, hi):
    """s_f = +1 if t_f + h_f <= hi_f else -1 (a NaN t gives -1)"""
    with np.errstate(all="ignore"):
        return np.where(t + h <= hi, 1.0, -1.0)


def prior_defined(prior_mean, prior_weight, M, F):
    """none / (F,) / (M, F) -> (mu, p), both (M, F) float64, or (None, None) without a prior"""
    if prior_mean is None and prior_weight is None:
        return None, None
    if prior_mean is None or prior_weight is None:
        raise ValueError("prior_mean and prior_weight come together")
    mu, p = np.asarray(prior_mean, dtype=np.float64), np.asarray(prior_weight, dtype=np.float64)
    if mu.shape != p.shape or mu.shape not in ((F,), (M, F)):
        raise ValueError(f"prior_mean {mu.shape} and prior_weight {p.shape}: expected both ({F},) or both ({M}, {F})")
    return np.array(np.broadcast_to(mu, (M, F)), order="C"), np.array(np.broadcast_to(p, (M, F)), order="C")


def prior_cost_defined(c, t, mu, p):
    """the prior's part of step 3: for f ascending: skip p_f == 0 (mu_f may be NaN), else e_f = t_f - mu_f,
    c = c + (p_f e_f) e_f.  -> (c (M,), e (M, F))"""
    with np.errstate(all="ignore"):
        e = t - mu
        for f in range(t.shape[1]):
            c = np.where(p[:, f] == 0.0, c, c + (p[:, f] * e[:, f]) * e[:, f])
    return c, e


def prior_normal_defined(packed, e, p):
    """the prior's part of step 6, after the band sums: for a ascending with p_a != 0: A_aa = A_aa + p_a,
    g_a = g_a + p_a e_a.  -> a new packed (M, P)"""
    F = e.shape[1]
    nt = F * (F + 1) // 2
    out = np.array(packed, dtype=np.float64, copy=True)
    with np.errstate(all="ignore"):
        for a in range(F):
            skip = p[:, a] == 0.0
            out[:, tri(a, a)] = np.where(skip, out[:, tri(a, a)], out[:, tri(a, a)] + p[:, a])
            out[:, nt + a] = np.where(skip, out[:, nt + a], out[:, nt + a] + p[:, a] * e[:, a])
    return out


def refine_defined(base, free, lo, hi, obs, forward, weights=None, n_iter=10, rel_step=1e-3, lambda0=1e-2, history=None,
                   prior_mean=None, prior_weight=None):
    """base (M, 27) start rows; free: F distinct column numbers; lo, hi (F,); obs (M, nb); weights None, (nb,) or (M, nb) (a
    weight of exactly 0 skips the band); forward(rows (R, 27)) -> (R, nb) float64, the chosen sensor column of the model.
    prior_mean, prior_weight: None, or both (F,) or both (M, F): a Gaussian prior on the free parameters, weight = 1 / sigma^2
    (exactly 0: no prior on that parameter, the mean may then be NaN; negative, NaN or infinite: a dead observation).
    -> dict x (M, F), cost, cost0 (M,), std (M, F), n_accept (M,) int32 (-1: a dead observation), y (M, nb).
    ``history``: an optional list that receives (x, cost) after every decision (the prefix property)."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    free = [int(f) for f in free]
    F, (M, nb) = len(free), obs.shape
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not 1 <= F <= MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[1]:
        raise ValueError("free: 1 ... 16 distinct column numbers")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    if not 0 <= int(n_iter) <= MAX_ITER:
        raise ValueError("n_iter: 0 ... 100")
    w = weights_defined(weights, M, nb)
    bad = bad_weights_defined(w)
    mu, pw = prior_defined(prior_mean, prior_weight, M, F)
    if pw is not None:
        bad = bad | bad_weights_defined(pw)
    h = rel_step * (hi - lo)
    x = clip_defined(base[:, free], lo, hi)
    t = x.copy()
    c = np.full(M, np.inf)
    cost0 = np.full(M, np.nan)
    lam = np.full(M, float(lambda0))
    n_accept = np.zeros(M, dtype=np.int32)
    dead = np.zeros(M, dtype=bool)
    packed = np.zeros((M, F * (F + 1) // 2 + F))
    y = np.full((M, nb), np.nan)
    for it in range(int(n_iter) + 1):
        sh = step_sign(t, h, hi) * h
        rows = np.repeat(base[None], F + 1, axis=0)                 # (F + 1, M, 27): p_0, p_1 ... p_F
        rows[:, :, free] = t[None]
        with np.errstate(all="ignore"):
            for f in range(F):
                rows[f + 1, :, free[f]] = t[:, f] + sh[:, f]
        Y = np.asarray(forward(rows.reshape(-1, base.shape[1])), dtype=np.float64).reshape(F + 1, M, nb)
        ct, d = cost_defined(Y[0], obs, w)
        if pw is not None:
            ct, e = prior_cost_defined(ct, t, mu, pw)
        with np.errstate(all="ignore"):
            accept = (ct < c) & ~dead & ~bad
        if it == 0:
            cost0 = ct.copy()
            dead = ~accept
            c = np.where(dead, ct, c)
            y = np.where(dead[:, None], Y[0], y)
            n_accept[dead] = -1
        if accept.any():
            with np.errstate(all="ignore"):
                J = np.moveaxis((Y[1:] - Y[0][None]) / sh.T[:, :, None], 0, 2)       # (M, nb, F)
            new = normal_defined(J, d, w)
            if pw is not None:
                new = prior_normal_defined(new, e, pw)
            packed = np.where(accept[:, None], new, packed)
        x = np.where(accept[:, None], t, x)
        c = np.where(accept, ct, c)
        y = np.where(accept[:, None], Y[0], y)
        if it > 0:
            lam = np.where(dead, lam, lambda_defined(lam, accept))
            n_accept = n_accept + accept.astype(np.int32)
        if history is not None:
            history.append((x.copy(), c.copy()))
        if it == int(n_iter):
            break
        t = np.where(dead[:, None], t, propose_defined(packed, lam, x, lo, hi))
    std = np.where(dead[:, None], np.nan, std_defined(packed, F))
    return {"x": x, "cost": c, "cost0": cost0, "std": std, "n_accept": n_accept, "y": y}
