"""The DEFINITION of spart_refine_views (include/spart_hip.h): spart_refine's bounded Levenberg-Marquardt fit with ONE unknown
vector per pixel against V observations (views) of it -- Fs shared parameters, one value for all views, and Fl local ones, one
value per view -- in numpy, every sum and solve in one pinned order.  It is refine_defined.py's text with F read as
n = Fs + V Fl wherever the unknowns are meant; what is new is the index maps, the V (F + 1) forward rows of a trial and the
structurally absent entries of J.  csrc/spart_refine_views.h must reproduce it bit for bit.

Index conventions.  free = shared + local lists the F = Fs + Fl free columns by NAME; lo, hi are per name.  Unknown a < Fs is
shared name a; unknown Fs + v Fl + l is local name Fs + l in view v.  Virtual band u = v nb + j.  Unknown a is ACTIVE in view v
when it is shared or a local of view v.
"""
import numpy as np

import refine_defined as rd

MAX_V = 64


def unknown_of(v, f, Fs, Fl):
    """the unknown that free column f takes its value from in view v"""
    return f if f < Fs else Fs + v * Fl + (f - Fs)


def name_of(a, Fs, Fl):
    """the index into ``free`` of unknown a"""
    return a if a < Fs else Fs + (a - Fs) % Fl


def view_of(a, Fs, Fl):
    """the view of a local unknown; -1 for a shared one"""
    return -1 if a < Fs else (a - Fs) // Fl


def active_defined(V, Fs, Fl, nb):
    """(V nb, n) bool: unknown a is active at virtual band u"""
    n = Fs + V * Fl
    va = np.array([view_of(a, Fs, Fl) for a in range(n)])
    vu = np.repeat(np.arange(V), nb)
    return (va[None, :] < 0) | (va[None, :] == vu[:, None])


def weights_views_defined(weights, M, V, nb):
    """none / (nb,) for every view / (M, V, nb) -> (M, V nb) float64"""
    if weights is None:
        return np.ones((M, V * nb))
    w = np.asarray(weights, dtype=np.float64)
    if w.shape not in ((nb,), (M, V, nb)):
        raise ValueError(f"weights has shape {w.shape}, expected ({nb},) or ({M}, {V}, {nb})")
    return np.ascontiguousarray(np.broadcast_to(w, (M, V, nb))).reshape(M, V * nb)


def normal_views_defined(J, r, w, act):
    """rd.normal_defined over the virtual bands with the absent entries SKIPPED: J (M, U, n), r, w (M, U), act (U, n).  The
    sum of A_ab runs over the u where a and b are active and w_u != 0, that of g_a over the u where a is; J may hold anything
    where it is absent."""
    M, U, n = J.shape
    ia, ib = rd.packed_pairs(n)
    A = np.zeros((M, ia.size))
    g = np.zeros((M, n))
    with np.errstate(all="ignore"):
        for u in range(U):
            skip = (w[:, u] == 0.0)[:, None]
            wj = w[:, u, None] * J[:, u, :]
            A = np.where(skip | ~(act[u, ia] & act[u, ib])[None, :], A, A + wj[:, ia] * J[:, u, ib])
            g = np.where(skip | ~act[u][None, :], g, g + wj * r[:, u, None])
    return np.concatenate([A, g], axis=1)


def rows_defined(base, free, Fs, t, sh):
    """the V (F + 1) rows of a trial: base (V, M, 27), t, sh (M, n) -> (V, F + 1, M, 27).  p_(v,0) = view v's base with the
    free columns from the trial; p_(v,f) = p_(v,0) with column free[f-1] moved by s_a h_a of the unknown it belongs to"""
    V, F, Fl = base.shape[0], len(free), len(free) - Fs
    rows = np.repeat(base[:, None], F + 1, axis=1)
    with np.errstate(all="ignore"):
        for v in range(V):
            for f in range(F):
                a = unknown_of(v, f, Fs, Fl)
                rows[v, :, :, free[f]] = t[None, :, a]
                rows[v, f + 1, :, free[f]] = t[:, a] + sh[:, a]
    return rows


def refine_views_defined(base, shared, local, lo, hi, obs, forward, weights=None, n_iter=10, rel_step=1e-3, lambda0=1e-2,
                         history=None, prior_mean=None, prior_weight=None):
    """base (V, M, 27): every view's rows; shared, local: Fs + Fl = F distinct column numbers; lo, hi (F,) per name; obs
    (M, V, nb); weights None, (nb,) or (M, V, nb); forward(rows (R, 27)) -> (R, nb), row by row; prior_mean, prior_weight None,
    or both (n,) or both (M, n).  The shared columns of views 1 ... V-1 of ``base`` are never read.
    -> dict x (M, n), cost, cost0 (M,), std (M, n), n_accept (M,) int32 (-1: a dead pixel), y (M, V, nb)."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    shared, local = [int(f) for f in shared], [int(f) for f in local]
    free, Fs, Fl = shared + local, len(shared), len(local)
    F, (M, V, nb) = Fs + Fl, obs.shape
    n, U = Fs + V * Fl, V * nb
    if not 1 <= V <= MAX_V or base.shape[:2] != (V, M):
        raise ValueError("V: 1 ... 64 views, base (V, M, 27)")
    if not 1 <= F <= rd.MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[2]:
        raise ValueError("free: 1 ... 16 distinct column numbers")
    if not 1 <= n <= rd.MAX_F:
        raise ValueError("n = Fs + V Fl: 1 ... 16 unknowns")
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    if not 0 <= int(n_iter) <= rd.MAX_ITER:
        raise ValueError("n_iter: 0 ... 100")
    names = [name_of(a, Fs, Fl) for a in range(n)]
    lo_n, hi_n = lo[names], hi[names]
    h = (rel_step * (hi - lo))[names]
    act = active_defined(V, Fs, Fl, nb)
    w = weights_views_defined(weights, M, V, nb)
    bad = rd.bad_weights_defined(w)
    mu, pw = rd.prior_defined(prior_mean, prior_weight, M, n)
    if pw is not None:
        bad = bad | rd.bad_weights_defined(pw)
    start = np.empty((M, n))
    for a in range(n):
        start[:, a] = base[max(view_of(a, Fs, Fl), 0), :, free[names[a]]]
    x = rd.clip_defined(start, lo_n, hi_n)
    t = x.copy()
    obs_u = obs.reshape(M, U)
    c = np.full(M, np.inf)
    cost0 = np.full(M, np.nan)
    lam = np.full(M, float(lambda0))
    n_accept = np.zeros(M, dtype=np.int32)
    dead = np.zeros(M, dtype=bool)
    packed = np.zeros((M, n * (n + 1) // 2 + n))
    y = np.full((M, U), np.nan)
    for it in range(int(n_iter) + 1):
        sh = rd.step_sign(t, h, hi_n) * h
        rows = rows_defined(base, free, Fs, t, sh)
        Y = np.asarray(forward(rows.reshape(-1, base.shape[2])), dtype=np.float64).reshape(V, F + 1, M, nb)
        Y0 = np.ascontiguousarray(np.moveaxis(Y[:, 0], 0, 1)).reshape(M, U)
        ct, d = rd.cost_defined(Y0, obs_u, w)
        if pw is not None:
            ct, e = rd.prior_cost_defined(ct, t, mu, pw)
        with np.errstate(all="ignore"):
            accept = (ct < c) & ~dead & ~bad
        if it == 0:
            cost0 = ct.copy()
            dead = ~accept
            c = np.where(dead, ct, c)
            y = np.where(dead[:, None], Y0, y)
            n_accept[dead] = -1
        if accept.any():
            J = np.zeros((M, U, n))
            with np.errstate(all="ignore"):
                for a in range(n):
                    for v in (range(V) if a < Fs else [view_of(a, Fs, Fl)]):
                        J[:, v * nb:(v + 1) * nb, a] = (Y[v, names[a] + 1] - Y[v, 0]) / sh[:, a, None]
            new = normal_views_defined(J, d, w, act)
            if pw is not None:
                new = rd.prior_normal_defined(new, e, pw)
            packed = np.where(accept[:, None], new, packed)
        x = np.where(accept[:, None], t, x)
        c = np.where(accept, ct, c)
        y = np.where(accept[:, None], Y0, y)
        if it > 0:
            lam = np.where(dead, lam, rd.lambda_defined(lam, accept))
            n_accept = n_accept + accept.astype(np.int32)
        if history is not None:
            history.append((x.copy(), c.copy()))
        if it == int(n_iter):
            break
        t = np.where(dead[:, None], t, rd.propose_defined(packed, lam, x, lo_n, hi_n))
    std = np.where(dead[:, None], np.nan, rd.std_defined(packed, n))
    return {"x": x, "cost": c, "cost0": cost0, "std": std, "n_accept": n_accept, "y": y.reshape(M, V, nb)}
