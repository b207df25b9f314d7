"""The DEFINITION of spart_refine_tiles (include/spart_hip.h): bounded Levenberg-Marquardt refinement in which the first Fs free
parameters are shared by a TILE of pixels and the other Fl = F - Fs belong to one pixel each, in numpy, with every sum and
solve in one pinned order.  The per-entry arithmetic is tools/refine_defined.py's and is imported, not restated; what is new
is the order of the sums over the pixels of a tile and the block-arrowhead solve.

Index conventions.  ``free`` lists the F free columns by NAME, the shared ones first; lo / hi / h belong to a name.  Inside a
pixel the unknowns are taken in SOLVE ORDER, every local first and then the shared ones: solve index q = b for local name
Fs + b and q = Fl + a for shared name a.  The packed vector of a pixel, A_m then g_m, is refine_defined's in that order, so a
shared row of A_m holds (w J_shared) J_local: with one pixel per tile the call IS refine_defined with free = local names then
shared names.  The unknowns of a tile are ordered every live pixel's locals (pixels ascending), then the shared ones; entries
between locals of different pixels are structurally absent and skipped everywhere.
"""
import numpy as np

from refine_defined import (MAX_F, MAX_ITER, bad_weights_defined, clip_defined, cost_defined, lambda_defined, normal_defined,
                            packed_pairs, prior_cost_defined, prior_defined, prior_normal_defined, step_sign, tri, weights_defined)

MAX_TILE = 4096


def check_tile_start(tile_start, M):
    """(T + 1,) int64 with tile_start[0] = 0, strictly increasing, tile_start[T] = M, no tile above MAX_TILE pixels"""
    ts = np.asarray(tile_start, dtype=np.int64).reshape(-1)
    if ts.size < 1 or ts[0] != 0 or ts[-1] != M or (np.diff(ts) <= 0).any() or (np.diff(ts) > MAX_TILE).any():
        raise ValueError("tile_start: 0 = s_0 < s_1 < ... < s_T = M with at most 4096 pixels per tile")
    return ts


def eliminate_defined(Bp, F, Fl):
    """refine_defined.cholesky_defined over the columns j < Fl only: packed (M, F(F+1)/2) in solve order -> (L, ok).  The local
    block becomes R_m, the local part of a shared row W_m; the shared block is left as it came."""
    L = np.array(Bp, dtype=np.float64, copy=True)
    ok = np.ones(L.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(F):
            for j in range(min(i + 1, Fl)):
                s = L[:, tri(i, j)].copy()
                for k in range(j):
                    s = s - L[:, tri(i, k)] * L[:, tri(j, k)]
                if i == j:
                    ok &= s > 0.0
                    L[:, tri(i, i)] = np.sqrt(s)
                else:
                    L[:, tri(i, j)] = s / L[:, tri(j, j)]
    return L, ok


def local_forward_defined(L, g, Fl):
    """R_m d_m = -g_m[local], k ascending -> d (M, Fl)"""
    d = np.zeros((L.shape[0], Fl))
    with np.errstate(all="ignore"):
        for j in range(Fl):
            s = -g[:, j]
            for k in range(j):
                s = s - L[:, tri(j, k)] * d[:, k]
            d[:, j] = s / L[:, tri(j, j)]
    return d


def shared_factor_defined(L, Bs, Fs, Fl):
    """L (G, nt): the eliminated matrices of a tile's live pixels in order; Bs: the packed (damped) shared block.  Entry (a, b):
    s = B_ab; for m ascending, k = 0 .. Fl - 1: s = s - W_m[a, k] W_m[b, k]; for shared k < b: s = s - Ls[a, k] Ls[b, k].
    -> (Ls packed, ok)"""
    ia, ib = packed_pairs(Fs)
    acc = np.array(Bs, dtype=np.float64, copy=True)
    with np.errstate(all="ignore"):
        for m in range(L.shape[0]):
            for k in range(Fl):
                acc = acc - L[m, tri(Fl + ia, k)] * L[m, tri(Fl + ib, k)]
        ok = True
        for a in range(Fs):
            for b in range(a + 1):
                s = acc[tri(a, b)]
                for k in range(b):
                    s = s - acc[tri(a, k)] * acc[tri(b, k)]
                if a == b:
                    ok = ok and bool(s > 0.0)
                    acc[tri(a, a)] = np.sqrt(s)
                else:
                    acc[tri(a, b)] = s / acc[tri(b, b)]
    return acc, ok


def tile_solve_defined(L, d, Ls, gs, Fs, Fl):
    """The rest of B delta = -g for one tile: the shared forward substitution (s = -gs_a; for m ascending, k ascending:
    s = s - W_m[a, k] d_(m, k); for shared k < a: s = s - Ls[a, k] y_k), the shared back substitution from Fs - 1 down, then
    every local j from Fl - 1 down with k = j + 1 .. Fl - 1 first and the shared a ascending after.  -> (delta_s, delta_l)"""
    G = L.shape[0]
    sa = np.arange(Fs)
    ds = np.zeros(Fs)
    dl = np.zeros((G, Fl))
    with np.errstate(all="ignore"):
        acc = -np.array(gs, dtype=np.float64)
        for m in range(G):
            for k in range(Fl):
                acc = acc - L[m, tri(Fl + sa, k)] * d[m, k]
        for a in range(Fs):
            s = acc[a]
            for k in range(a):
                s = s - Ls[tri(a, k)] * ds[k]
            ds[a] = s / Ls[tri(a, a)]
        for a in range(Fs - 1, -1, -1):
            s = ds[a]
            for k in range(a + 1, Fs):
                s = s - Ls[tri(k, a)] * ds[k]
            ds[a] = s / Ls[tri(a, a)]
        for j in range(Fl - 1, -1, -1):
            s = d[:, j].copy()
            for k in range(j + 1, Fl):
                s = s - L[:, tri(k, j)] * dl[:, k]
            for a in range(Fs):
                s = s - L[:, tri(Fl + a, j)] * ds[a]
            dl[:, j] = s / L[:, tri(j, j)]
    return ds, dl


def tile_std_defined(L, Ls, Fs, Fl):
    """refine_defined.std_defined's recurrence in the tile's unknown order, from the UNDAMPED factors: for a shared f, k runs
    over the shared unknowns >= f; for a local (m, j), k runs over m's locals >= j and then over every shared unknown.
    -> (shared_std (Fs,), local_std (G, Fl))"""
    G = L.shape[0]
    ss, ls = np.zeros(Fs), np.zeros((G, Fl))
    with np.errstate(all="ignore"):
        for f in range(Fs):
            z = np.zeros(Fs)
            var = 0.0
            for k in range(f, Fs):
                s = 1.0 if k == f else 0.0
                for i in range(f, k):
                    s = s - Ls[tri(k, i)] * z[i]
                z[k] = s / Ls[tri(k, k)]
                var = var + z[k] * z[k]
            ss[f] = np.sqrt(var)
        for j in range(Fl):
            z = np.zeros((G, Fl + Fs))
            var = np.zeros(G)
            for k in range(j, Fl):
                s = np.full(G, 1.0 if k == j else 0.0)
                for i in range(j, k):
                    s = s - L[:, tri(k, i)] * z[:, i]
                z[:, k] = s / L[:, tri(k, k)]
                var = var + z[:, k] * z[:, k]
            for a in range(Fs):
                s = np.zeros(G)
                for i in range(j, Fl):
                    s = s - L[:, tri(Fl + a, i)] * z[:, i]
                for i in range(a):
                    s = s - Ls[tri(a, i)] * z[:, Fl + i]
                z[:, Fl + a] = s / Ls[tri(a, a)]
                var = var + z[:, Fl + a] * z[:, Fl + a]
            ls[:, j] = np.sqrt(var)
    return ss, ls


def shared_prior_defined(mean, weight, T, Fs):
    """none / (Fs,) / (T, Fs) -> (mu, p), both (T, Fs), or (None, None)"""
    return prior_defined(mean, weight, T, Fs)


def refine_tiles_defined(base, shared, local, lo, hi, tile_start, obs, forward, weights=None, n_iter=10, rel_step=1e-3,
                         lambda0=1e-2, prior_mean=None, prior_weight=None, shared_prior_mean=None, shared_prior_weight=None,
                         history=None):
    """base (M, 27) start rows; shared / local: the Fs + Fl distinct column numbers; lo, hi (F,) by name, shared first;
    tile_start (T + 1,); obs (M, nb); weights None, (nb,) or (M, nb); forward(rows (R, 27)) -> (R, nb).
    prior_*: the prior of the LOCAL unknowns, None or both (Fl,) or both (M, Fl); shared_prior_*: None or both (Fs,) or (T, Fs).
    -> dict shared, shared_std (T, Fs); local, local_std (M, Fl); cost, cost0 (T,); n_accept (T,) int32 (-1: dead tile);
    pixel_cost (M,); status (M,) int32 (0 live, -1 dead pixel, 1 live pixel of a dead tile); y (M, nb).
    ``history``: an optional list that receives (shared, local, cost) after every decision."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    shared, local = [int(f) for f in shared], [int(f) for f in local]
    free = shared + local
    Fs, Fl, F, (M, nb) = len(shared), len(local), len(free), obs.shape
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not 1 <= F <= MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[1]:
        raise ValueError("shared + local: 1 ... 16 distinct column numbers")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    if not 0 <= int(n_iter) <= MAX_ITER:
        raise ValueError("n_iter: 0 ... 100")
    ts = check_tile_start(tile_start, M)
    T = ts.size - 1
    tile_of = np.repeat(np.arange(T), np.diff(ts))
    # solve order: q -> name
    name = np.array(list(range(Fs, F)) + list(range(Fs)), dtype=np.int64)
    qlo, qhi = lo[name], hi[name]
    nt = F * (F + 1) // 2
    nts = Fs * (Fs + 1) // 2

    w = weights_defined(weights, M, nb)
    bad = bad_weights_defined(w)
    mu_l, pw_l = prior_defined(prior_mean, prior_weight, M, Fl) if Fl else (None, None)
    mu_s, pw_s = shared_prior_defined(shared_prior_mean, shared_prior_weight, T, Fs) if Fs else (None, None)
    if pw_l is not None:
        bad = bad | bad_weights_defined(pw_l)
        mu_q = np.concatenate([mu_l, np.zeros((M, Fs))], axis=1)           # the prior in solve order: no entry for the shared
        pw_q = np.concatenate([pw_l, np.zeros((M, Fs))], axis=1)
    bad_tile = bad_weights_defined(pw_s) if pw_s is not None else np.zeros(T, dtype=bool)

    h = rel_step * (hi - lo)
    qh = h[name]
    z = clip_defined(base[ts[:-1]][:, shared], lo[:Fs], hi[:Fs]) if Fs else np.zeros((T, 0))            # (T, Fs)
    l = clip_defined(base[:, local], lo[Fs:], hi[Fs:]) if Fl else np.zeros((M, 0))                     # (M, Fl)
    zt, lt = z.copy(), l.copy()
    C = np.full(T, np.inf)
    cost0 = np.full(T, np.nan)
    lam = np.full(T, float(lambda0))
    n_accept = np.zeros(T, dtype=np.int32)
    dead_tile = np.zeros(T, dtype=bool)
    status = np.zeros(M, dtype=np.int32)
    pixel_cost = np.full(M, np.nan)
    packed = np.zeros((M, nt + F))
    S = np.zeros((T, nts + Fs))
    y = np.full((M, nb), np.nan)
    live = np.ones(M, dtype=bool)
    for it in range(int(n_iter) + 1):
        tq = np.concatenate([lt, zt[tile_of]], axis=1)                      # (M, F) the trial in solve order
        sh = step_sign(tq, qh, qhi) * qh
        rows = np.repeat(base[None], F + 1, axis=0)
        rows[:, :, free] = tq[:, np.argsort(name)][None]
        with np.errstate(all="ignore"):
            for f in range(F):
                q = int(np.where(name == f)[0][0])
                rows[f + 1, :, free[f]] = tq[:, q] + sh[:, q]
        Y = np.asarray(forward(rows.reshape(-1, base.shape[1])), dtype=np.float64).reshape(F + 1, M, nb)
        ct, d = cost_defined(Y[0], obs, w)
        if pw_l is not None:
            ct, e = prior_cost_defined(ct, tq, mu_q, pw_q)
        if it == 0:
            with np.errstate(all="ignore"):
                live = (ct < np.inf) & ~bad
            status[~live] = -1
            pixel_cost = np.where(live, pixel_cost, ct)
            y = np.where(live[:, None], y, Y[0])
        # the tile cost and the decision
        Ct = np.zeros(T)
        accept = np.zeros(T, dtype=bool)
        with np.errstate(all="ignore"):
            for t in range(T):
                c = 0.0
                for m in range(ts[t], ts[t + 1]):
                    if live[m]:
                        c = c + ct[m]
                if pw_s is not None:
                    for a in range(Fs):
                        if pw_s[t, a] != 0.0:
                            ea = zt[t, a] - mu_s[t, a]
                            c = c + (pw_s[t, a] * ea) * ea
                Ct[t] = c
                accept[t] = bool(c < C[t]) and not dead_tile[t] and not bad_tile[t] and live[ts[t]:ts[t + 1]].any()
        if it == 0:
            cost0 = Ct.copy()
            dead_tile = ~accept
            C = np.where(dead_tile, Ct, C)
            n_accept[dead_tile] = -1
            orphan = dead_tile[tile_of] & live
            status[orphan] = 1
            pixel_cost = np.where(orphan, ct, pixel_cost)
            y = np.where(orphan[:, None], Y[0], y)
        acc_m = accept[tile_of] & live
        if acc_m.any():
            with np.errstate(all="ignore"):
                blocks = Y[1:][name]                                         # (F, M, nb) in solve order
                J = np.moveaxis((blocks - Y[0][None]) / sh.T[:, :, None], 0, 2)
            new = normal_defined(J, d, w)
            if pw_l is not None:
                new = prior_normal_defined(new, e, pw_q)
            packed = np.where(acc_m[:, None], new, packed)
            with np.errstate(all="ignore"):
                for t in np.flatnonzero(accept):
                    s = np.zeros(nts + Fs)
                    ia, ib = packed_pairs(Fs)
                    pick = np.concatenate([tri(Fl + ia, Fl + ib), nt + Fl + np.arange(Fs)]).astype(np.int64)
                    for m in range(ts[t], ts[t + 1]):
                        if live[m]:
                            s = s + packed[m, pick]
                    if pw_s is not None:
                        for a in range(Fs):
                            if pw_s[t, a] != 0.0:
                                s[tri(a, a)] = s[tri(a, a)] + pw_s[t, a]
                                s[nts + a] = s[nts + a] + pw_s[t, a] * (zt[t, a] - mu_s[t, a])
                    S[t] = s
        z = np.where(accept[:, None], zt, z)
        l = np.where(acc_m[:, None], lt, l)
        C = np.where(accept, Ct, C)
        pixel_cost = np.where(acc_m, ct, pixel_cost)
        y = np.where(acc_m[:, None], Y[0], y)
        if it > 0:
            lam = np.where(dead_tile, lam, lambda_defined(lam, accept))
            n_accept = n_accept + accept.astype(np.int32)
        if history is not None:
            history.append((z.copy(), l.copy(), C.copy()))
        if it == int(n_iter):
            break
        # propose
        lam_m = lam[tile_of]
        B = packed[:, :nt].copy()
        with np.errstate(all="ignore"):
            for j in range(Fl):
                Ajj = B[:, tri(j, j)]
                B[:, tri(j, j)] = Ajj + lam_m * np.where(Ajj > 0.0, Ajj, 1.0)
        L, okm = eliminate_defined(B, F, Fl)
        dloc = local_forward_defined(L, packed[:, nt:], Fl)
        for t in np.flatnonzero(~dead_tile):
            idx = np.arange(ts[t], ts[t + 1])
            idx = idx[live[idx]]
            Bs = S[t, :nts].copy()
            with np.errstate(all="ignore"):
                for a in range(Fs):
                    Saa = Bs[tri(a, a)]
                    Bs[tri(a, a)] = Saa + lam[t] * (Saa if Saa > 0.0 else 1.0)
            Ls, ok = shared_factor_defined(L[idx], Bs, Fs, Fl)
            ds, dl = tile_solve_defined(L[idx], dloc[idx], Ls, S[t, nts:], Fs, Fl)
            ok = ok and bool(okm[idx].all()) and bool(np.isfinite(ds).all()) and bool(np.isfinite(dl).all())
            if not ok:
                ds, dl = np.zeros(Fs), np.zeros((idx.size, Fl))
            with np.errstate(all="ignore"):
                zt[t] = clip_defined(z[t] + ds, lo[:Fs], hi[:Fs])
                lt[idx] = clip_defined(l[idx] + dl, lo[Fs:], hi[Fs:])
    # std from the undamped matrices
    shared_std = np.full((T, Fs), np.nan)
    local_std = np.full((M, Fl), np.nan)
    L, okm = eliminate_defined(packed[:, :nt], F, Fl)
    for t in np.flatnonzero(~dead_tile):
        idx = np.arange(ts[t], ts[t + 1])
        idx = idx[live[idx]]
        Ls, ok = shared_factor_defined(L[idx], S[t, :nts], Fs, Fl)
        if ok and okm[idx].all():
            shared_std[t], local_std[idx] = tile_std_defined(L[idx], Ls, Fs, Fl)
    return {"shared": z, "shared_std": shared_std, "local": l, "local_std": local_std, "cost": C, "cost0": cost0,
            "n_accept": n_accept, "pixel_cost": pixel_cost, "status": status, "y": y}
