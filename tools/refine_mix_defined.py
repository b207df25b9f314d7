"""The DEFINITION of spart_refine_mix (include/spart_hip.h): spart_refine's bounded Levenberg-Marquardt fit of ONE observed
column per pixel with a LINEAR MIXTURE of V canopies, y_j = sum_v a_v Y_v[j], in numpy, every sum and solve in one pinned order.
It is refine_defined.py's text with F read as n wherever the unknowns are meant; what is new is the unknown maps with the
activity mask of the locals, the fractions on the simplex, the mixed column and the Jacobian that is dense over the nb bands.
csrc/spart_refine_mix.h must reproduce it bit for bit.  The chosen column itself is mixed: for R_TOA / L_TOA that neglects the
coupling of neighbouring surfaces through the atmosphere.

Index conventions.  free = shared + local lists the F = Fs + Fl free columns by NAME; lo, hi are per name.  The unknowns are, in
this order: the Fs shared names; the ACTIVE locals, component v ascending and within a component l ascending (``active`` (V, Fl)
bool; an inactive local of a component stays at that component's base value and is no unknown); with fit_fractions
q_0 ... q_{V-2}.  nm counts the model unknowns, n = nm + (V - 1 if fit_fractions else 0), 1 <= n <= 16, 1 <= V <= 8.
"""
import numpy as np

import refine_defined as rd

MAX_V = 8
SHARED, LOCAL, FRACTION = 0, 1, 2


def maps_defined(V, Fs, Fl, active=None, fit_fractions=True):
    """-> (kind, name, comp, unknown): kind[a] SHARED / LOCAL / FRACTION, name[a] the index into ``free`` (-1 for a fraction),
    comp[a] the component (-1 for a shared unknown; v of q_v for a fraction); unknown[v, f] the unknown that free column f takes
    its value from in component v, -1 where that local is inactive.  ValueError for a local that is active nowhere."""
    act = np.ones((V, Fl), dtype=bool) if active is None else np.asarray(active)
    if act.shape != (V, Fl):
        raise ValueError(f"active has shape {act.shape}, expected (V, Fl) = ({V}, {Fl})")
    if not np.isin(act, (0, 1)).all():
        raise ValueError("active: entries 0 / 1")
    act = act.astype(bool)
    if Fl and not act.any(axis=0).all():
        raise ValueError("a local name is active in no component")
    kind, name, comp = [SHARED] * Fs, list(range(Fs)), [-1] * Fs
    unknown = np.full((V, Fs + Fl), -1, dtype=np.int64)
    unknown[:, :Fs] = np.arange(Fs)[None]
    for v in range(V):
        for l in range(Fl):
            if act[v, l]:
                unknown[v, Fs + l] = len(kind)
                kind.append(LOCAL), name.append(Fs + l), comp.append(v)
    if fit_fractions:
        for v in range(V - 1):
            kind.append(FRACTION), name.append(-1), comp.append(v)
    return np.array(kind, dtype=np.int64), np.array(name, dtype=np.int64), np.array(comp, dtype=np.int64), unknown


def rows_defined(base, free, unknown, t, sh):
    """the V (F + 1) rows of a trial, as rows_defined of the views definition: base (V, M, 27), t, sh (M, n) ->
    (V, F + 1, M, 27).  p_(v,0) = component v's base with the free columns that have an unknown from the trial; p_(v,f+1) =
    p_(v,0) with column free[f] moved by s_a h_a of that unknown.  Where the local is inactive in v the block is the unmoved
    trial row."""
    V, F = base.shape[0], len(free)
    rows = np.repeat(base[:, None], F + 1, axis=1)
    with np.errstate(all="ignore"):
        for v in range(V):
            for f in range(F):
                a = unknown[v, f]
                if a < 0:
                    continue
                rows[v, :, :, free[f]] = t[None, :, a]
                rows[v, f + 1, :, free[f]] = t[:, a] + sh[:, a]
    return rows


def fractions_defined(t, nm, V, frac, fit_fractions):
    """the fractions of a trial -> (a (M, V), feasible (M,), bad (M,)).  Fitted: s = 0; for v < V - 1 ascending a_v = t[nm + v],
    s = s + a_v; a_{V-1} = 1 - s; FEASIBLE iff a_{V-1} >= 0 (a NaN is not).  Given: a_v = frac[m, v] as it is, always feasible;
    a negative, NaN or infinite entry is the rule of a bad weight."""
    M = t.shape[0]
    if not fit_fractions:
        return frac.copy(), np.ones(M, dtype=bool), rd.bad_weights_defined(frac)
    a = np.empty((M, V))
    s = np.zeros(M)
    with np.errstate(all="ignore"):
        for v in range(V - 1):
            a[:, v] = t[:, nm + v]
            s = s + a[:, v]
        a[:, V - 1] = 1.0 - s
        return a, a[:, V - 1] >= 0.0, np.zeros(M, dtype=bool)


def mix_defined(a, Y0):
    """the mixed column: a (M, V), Y0 (V, M, nb) -> y_j = a_0 Y_(0,0)j; for v = 1 ... V - 1: y_j = y_j + a_v Y_(v,0)j"""
    with np.errstate(all="ignore"):
        y = a[:, 0, None] * Y0[0]
        for v in range(1, a.shape[1]):
            y = y + a[:, v, None] * Y0[v]
    return y


def jacobian_defined(Y, a, sh, kind, name, comp):
    """Y (V, F + 1, M, nb), a (M, V), sh (M, n) -> J (M, nb, n), dense over the bands.  Local unknown of component v, name f:
    a_v ((Y_(v,f+1) - Y_(v,0)) / (s h)); shared: that product for v = 0, then + a_v (...) for v ascending; fraction q_v:
    Y_(v,0) - Y_(V-1,0)."""
    V, _, M, nb = Y.shape
    J = np.zeros((M, nb, kind.size))
    with np.errstate(all="ignore"):
        for u in range(kind.size):
            if kind[u] == FRACTION:
                J[:, :, u] = Y[comp[u], 0] - Y[V - 1, 0]
                continue
            f = name[u]
            for v in (range(V) if kind[u] == SHARED else [comp[u]]):
                term = a[:, v, None] * ((Y[v, f + 1] - Y[v, 0]) / sh[:, u, None])
                J[:, :, u] = term if (kind[u] == LOCAL or v == 0) else J[:, :, u] + term
    return J


def refine_mix_defined(base, shared, local, lo, hi, obs, forward, frac, active=None, fit_fractions=True, frac_lo=0.0, frac_hi=1.0,
                       weights=None, n_iter=10, rel_step=1e-3, lambda0=1e-2, prior_mean=None, prior_weight=None, history=None):
    """base (V, M, 27): every component's rows; shared, local: Fs + Fl = F distinct column numbers; lo, hi (F,) per name; obs
    (M, nb); frac (M, V): the given fractions, or the start of the fitted ones (its last column is then never read); weights
    None, (nb,) or (M, nb); forward(rows (R, 27)) -> (R, nb), row by row; prior_mean, prior_weight None, or both (n,) or both
    (M, n); history: an optional list that receives (x, cost, feasible) after every decision.  The shared columns of
    components 1 ... V-1 of ``base`` are never read.
    -> dict x, std (M, n), cost, cost0 (M,), n_accept (M,) int32 (-1: a dead pixel), y (M, nb) the mixed column at x, frac (M, V)
    all V fractions at x, y_comp (M, V, nb) the components' own columns at x."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    frac = np.ascontiguousarray(frac, dtype=np.float64)
    shared, local = [int(f) for f in shared], [int(f) for f in local]
    free, Fs, Fl = shared + local, len(shared), len(local)
    F, (M, nb), V = Fs + Fl, obs.shape, base.shape[0]
    if not 1 <= V <= MAX_V or base.shape[:2] != (V, M) or frac.shape != (M, V):
        raise ValueError("V: 1 ... 8 components, base (V, M, 27), frac (M, V)")
    if not 1 <= F <= rd.MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[2]:
        raise ValueError("free: 1 ... 16 distinct column numbers")
    kind, name, comp, unknown = maps_defined(V, Fs, Fl, active, fit_fractions)
    n, nm = kind.size, int((kind != FRACTION).sum())
    if not 1 <= n <= rd.MAX_F:
        raise ValueError("n: 1 ... 16 unknowns")
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    if not 0.0 <= frac_lo < frac_hi <= 1.0:
        raise ValueError("fraction box: 0 <= lo < hi <= 1")
    if not 0 <= int(n_iter) <= rd.MAX_ITER:
        raise ValueError("n_iter: 0 ... 100")
    # bounds and step per unknown: those of its name; a fraction has the box [frac_lo, frac_hi] and no step
    lo_n = np.concatenate([lo[name[:nm]], np.full(n - nm, float(frac_lo))])
    hi_n = np.concatenate([hi[name[:nm]], np.full(n - nm, float(frac_hi))])
    h = np.concatenate([(rel_step * (hi - lo))[name[:nm]], np.zeros(n - nm)])
    w = rd.weights_defined(weights, M, nb)
    bad = rd.bad_weights_defined(w)
    mu, pw = rd.prior_defined(prior_mean, prior_weight, M, n)
    if pw is not None:
        bad = bad | rd.bad_weights_defined(pw)
    start = np.empty((M, n))
    for u in range(n):
        start[:, u] = frac[:, comp[u]] if kind[u] == FRACTION else base[max(comp[u], 0), :, free[name[u]]]
    x = rd.clip_defined(start, lo_n, hi_n)
    t = x.copy()
    c = np.full(M, np.inf)
    cost0 = np.full(M, np.nan)
    lam = np.full(M, float(lambda0))
    n_accept = np.zeros(M, dtype=np.int32)
    dead = np.zeros(M, dtype=bool)
    packed = np.zeros((M, n * (n + 1) // 2 + n))
    y = np.full((M, nb), np.nan)
    fr = np.full((M, V), np.nan)
    yc = np.full((M, V, nb), np.nan)
    for it in range(int(n_iter) + 1):
        sh = rd.step_sign(t, h, hi_n) * h
        rows = rows_defined(base, free, unknown, t, sh)
        Y = np.asarray(forward(rows.reshape(-1, base.shape[2])), dtype=np.float64).reshape(V, F + 1, M, nb)
        a, feasible, bad_a = fractions_defined(t, nm, V, frac, fit_fractions)
        ym = mix_defined(a, Y[:, 0])
        ct, d = rd.cost_defined(ym, obs, w)
        if pw is not None:
            ct, e = rd.prior_cost_defined(ct, t, mu, pw)
        ct = np.where(feasible, ct, np.inf)
        with np.errstate(all="ignore"):
            accept = (ct < c) & ~dead & ~bad & ~bad_a
        if it == 0:
            cost0 = ct.copy()
            dead = ~accept
            c = np.where(dead, ct, c)
            y = np.where(dead[:, None], ym, y)
            fr = np.where(dead[:, None], a, fr)
            yc = np.where(dead[:, None, None], np.moveaxis(Y[:, 0], 0, 1), yc)
            n_accept[dead] = -1
        if accept.any():
            J = jacobian_defined(Y, a, sh, kind, name, comp)
            new = rd.normal_defined(J, d, w)
            if pw is not None:
                new = rd.prior_normal_defined(new, e, pw)
            packed = np.where(accept[:, None], new, packed)
        x = np.where(accept[:, None], t, x)
        c = np.where(accept, ct, c)
        y = np.where(accept[:, None], ym, y)
        fr = np.where(accept[:, None], a, fr)
        yc = np.where(accept[:, None, None], np.moveaxis(Y[:, 0], 0, 1), yc)
        if it > 0:
            lam = np.where(dead, lam, rd.lambda_defined(lam, accept))
            n_accept = n_accept + accept.astype(np.int32)
        if history is not None:
            history.append((x.copy(), c.copy(), feasible.copy()))
        if it == int(n_iter):
            break
        t = np.where(dead[:, None], t, rd.propose_defined(packed, lam, x, lo_n, hi_n))
    std = np.where(dead[:, None], np.nan, rd.std_defined(packed, n))
    return {"x": x, "cost": c, "cost0": cost0, "std": std, "n_accept": n_accept, "y": y, "frac": fr, "y_comp": yc}
