"""The DEFINITION of spart_refine_series (include/spart_hip.h): spart_refine_tiles with the tile read as a TIME SERIES of one
pixel -- a row is one date -- and a first-difference penalty between consecutive rows of a series on every local unknown
(the temporal regulariser of EO-LDAS, the Whittaker smoother), in numpy / Python floats with every sum and solve in one
pinned order.  What it does not change is imported from tools/refine_defined.py and tools/refine_tiles_defined.py.

The additions.  kappa_(m,b) = gamma_b * link[m] ties local b of row m to local b of row m + 1 (0: no tie).  The cost gains
(kappa e) e with e = t_(m+1,b) - t_(m,b); the diagonal of both rows gains kappa, the entry between them is -kappa; the
damped system is block-tridiagonal (a row's own local block, the Fl x Fl block X between consecutive rows, present iff some
kappa of that pair is not 0) with a border (the shared unknowns).  Unknown order: row 0's locals, row 1's locals, ..., then
the shared.  Every sum runs over the structurally present k, ascending in that order; an absent entry is skipped, never
multiplied in as a zero.  A series dies as a whole: a chain cannot lose a link.
"""
import math

import numpy as np

from refine_defined import (MAX_F, MAX_ITER, bad_weights_defined, clip_defined, cost_defined, lambda_defined, normal_defined,
                            packed_pairs, prior_cost_defined, prior_defined, prior_normal_defined, step_sign, tri)
from refine_defined import weights_defined
from refine_tiles_defined import shared_prior_defined

MAX_SERIES = 256


def check_series_start(series_start, M):
    """(S + 1,) int64 with series_start[0] = 0, strictly increasing, series_start[S] = M, no series above MAX_SERIES rows"""
    ts = np.asarray(series_start, dtype=np.int64).reshape(-1)
    if ts.size < 1 or ts[0] != 0 or ts[-1] != M or (np.diff(ts) <= 0).any() or (np.diff(ts) > MAX_SERIES).any():
        raise ValueError("series_start: 0 = s_0 < s_1 < ... < s_S = M with at most 256 rows per series")
    return ts


def smooth_defined(smooth, Fl):
    """(Fl,) gamma_b >= 0 and finite, one per LOCAL name"""
    g = np.asarray(smooth, dtype=np.float64).reshape(-1)
    if g.shape != (Fl,) or not (np.isfinite(g).all() and (g >= 0.0).all()):
        raise ValueError("smooth: (Fl,) finite values >= 0")
    return g


def kappa_defined(gamma, link, ts):
    """-> (kappa (M, Fl), the tie of row m to row m + 1 (0.0 at a series' last row, whose link is never read), bad link (M,))"""
    M, Fl = int(ts[-1]), gamma.size
    has_next = np.ones(M, dtype=bool)
    has_next[ts[1:] - 1] = False
    ln = np.ones(M) if link is None else np.asarray(link, dtype=np.float64).reshape(M)
    with np.errstate(all="ignore"):
        kap = np.where(has_next[:, None], gamma[None, :] * ln[:, None], 0.0)
        bad = has_next & (~(ln >= 0.0) | np.isinf(ln))
    return kap, bad, has_next


def chain_cost_defined(C, kap, lt, b0, b1):
    """the chain term of one series on the trial locals: m ascending over rows with a successor, b ascending, kappa == 0 skipped"""
    for m in range(b0, b1 - 1):
        for b in range(kap.shape[1]):
            k = float(kap[m, b])
            if k != 0.0:
                e = float(lt[m + 1, b]) - float(lt[m, b])
                C = C + (k * e) * e
    return C


def augment_defined(packed, kap, l, ts, rows, Fl, nt):
    """the chain's part of A_m and g_m of the rows ``rows`` (bool (M,)) at the accepted locals l: predecessor first, then
    successor; in place"""
    first = np.zeros(packed.shape[0], dtype=bool)
    first[ts[:-1]] = True
    for m in np.flatnonzero(rows):
        for b in range(Fl):
            A, g = float(packed[m, tri(b, b)]), float(packed[m, nt + b])
            if not first[m] and kap[m - 1, b] != 0.0:
                k = float(kap[m - 1, b])
                e = float(l[m, b]) - float(l[m - 1, b])
                A, g = A + k, g + k * e
            if kap[m, b] != 0.0:                                           # (0.0 at a series' last row)
                k = float(kap[m, b])
                e = float(l[m + 1, b]) - float(l[m, b])
                A, g = A + k, g - k * e
            packed[m, tri(b, b)], packed[m, nt + b] = A, g


def series_factor_defined(A, kap, Bs, Fs, Fl):
    """One series.  A (G, nt): the rows' (damped) packed matrices in solve order; kap (G, Fl): kap[m] ties rows m and m + 1;
    Bs: the packed (damped) shared block.  refine_cholesky's text over the present entries:
      X_m[i, j] = ((-kappa_(m-1,j) if i == j else 0.0) - sum_{k < j} X_m[i, k] R_(m-1)[j, k]) / R_(m-1)[j, j]    (m ties to m - 1)
      R_m[i, j]: s = B_m[i, j]; for k = 0 .. Fl-1: s = s - X_m[i, k] X_m[j, k]; for k < j: s = s - R_m[i, k] R_m[j, k]
      W_m[a, j]: s = A_m[a, j]; for k = 0 .. Fl-1: s = s - W_(m-1)[a, k] X_m[j, k]; for k < j: s = s - W_m[a, k] R_m[j, k]
      Ls: tiles' Schur sums over m then k, then the shared k < b.
    -> (L list of G packed lists, X list of G (Fl x Fl lists or None), Ls list, ok); at a pivot !(s > 0) ok is False and the rest
    is meaningless"""
    G, F = len(A), Fs + Fl
    L = [[float(v) for v in row] for row in A]
    X = [None] * G
    ia, ib = packed_pairs(Fs)
    acc = [float(v) for v in Bs]
    for m in range(G):
        Lm = L[m]
        Xm = None
        if m > 0 and any(float(k) != 0.0 for k in kap[m - 1]):
            Lq = L[m - 1]
            Xm = [[0.0] * Fl for _ in range(Fl)]
            for i in range(Fl):
                for j in range(Fl):
                    s = -float(kap[m - 1, j]) if i == j else 0.0
                    for k in range(j):
                        s = s - Xm[i][k] * Lq[tri(j, k)]
                    Xm[i][j] = s / Lq[tri(j, j)]
            X[m] = Xm
        for i in range(F):
            for j in range(min(i + 1, Fl)):
                s = Lm[tri(i, j)]
                if Xm is not None:
                    if i < Fl:
                        for k in range(Fl):
                            s = s - Xm[i][k] * Xm[j][k]
                    else:
                        for k in range(Fl):
                            s = s - L[m - 1][tri(i, k)] * Xm[j][k]
                for k in range(j):
                    s = s - Lm[tri(i, k)] * Lm[tri(j, k)]
                if i == j:
                    if not s > 0.0:
                        return L, X, acc, False
                    Lm[tri(i, i)] = math.sqrt(s)
                else:
                    Lm[tri(i, j)] = s / Lm[tri(j, j)]
        for e in range(len(acc)):
            a, b = int(ia[e]), int(ib[e])
            for k in range(Fl):
                acc[e] = acc[e] - Lm[tri(Fl + a, k)] * Lm[tri(Fl + b, k)]
    for a in range(Fs):
        for b in range(a + 1):
            s = acc[tri(a, b)]
            for k in range(b):
                s = s - acc[tri(a, k)] * acc[tri(b, k)]
            if a == b:
                if not s > 0.0:
                    return L, X, acc, False
                acc[tri(a, a)] = math.sqrt(s)
            else:
                acc[tri(a, b)] = s / acc[tri(b, b)]
    return L, X, acc, True


def series_solve_defined(L, X, Ls, g, gs, Fs, Fl):
    """B delta = -g from the factors, forward and back in the unknown order.  Forward, local (m, j): s = -g_(m,j); for
    k = 0 .. Fl-1: s = s - X_m[j, k] d_(m-1,k); for k < j: s = s - R_m[j, k] d_(m,k).  Shared as in tiles.  Back, local (m, j)
    from the last row down, j from Fl - 1 down: k = j + 1 .. Fl-1 of the row, then the next row's i = 0 .. Fl-1 through
    X_(m+1)[i, j], then the shared a ascending.  -> (delta_s list, delta_l list of lists)"""
    G = len(L)
    d = [[0.0] * Fl for _ in range(G)]
    acc = [-float(v) for v in gs]
    for m in range(G):
        Lm, dm = L[m], d[m]
        for j in range(Fl):
            s = -float(g[m][j])
            if X[m] is not None:
                for k in range(Fl):
                    s = s - X[m][j][k] * d[m - 1][k]
            for k in range(j):
                s = s - Lm[tri(j, k)] * dm[k]
            dm[j] = s / Lm[tri(j, j)]
        for a in range(Fs):
            for k in range(Fl):
                acc[a] = acc[a] - Lm[tri(Fl + a, k)] * dm[k]
    ds = [0.0] * Fs
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
    for m in range(G - 1, -1, -1):
        Lm, dm = L[m], d[m]
        nxt = X[m + 1] if m + 1 < G else None
        for j in range(Fl - 1, -1, -1):
            s = dm[j]
            for k in range(j + 1, Fl):
                s = s - Lm[tri(k, j)] * dm[k]
            if nxt is not None:
                for i in range(Fl):
                    s = s - nxt[i][j] * d[m + 1][i]
            for a in range(Fs):
                s = s - Lm[tri(Fl + a, j)] * ds[a]
            dm[j] = s / Lm[tri(j, j)]
    return ds, d


def series_std_defined(L, X, Ls, Fs, Fl):
    """refine_std's recurrence in the series' unknown order from the UNDAMPED factors.  For a local (m, j): k runs over m's
    locals >= j, then every later row's locals (through X and R), then the shared; the shared right-hand sides are
    accumulated row by row, which is the same order (m ascending, i ascending) per shared unknown.  Vectorised over the
    unknowns of the series; every unknown sees exactly its own terms.  -> (shared_std (Fs,), local_std (G, Fl))"""
    G = len(L)
    ss = np.zeros(Fs)
    with np.errstate(all="ignore"):
        for f in range(Fs):
            z = [0.0] * Fs
            var = 0.0
            for k in range(f, Fs):
                s = 1.0 if k == f else 0.0
                for i in range(f, k):
                    s = s - Ls[tri(k, i)] * z[i]
                z[k] = s / Ls[tri(k, k)]
                var = var + z[k] * z[k]
            ss[f] = math.sqrt(var)
        um, uj = np.repeat(np.arange(G), Fl), np.tile(np.arange(Fl), G)
        U = G * Fl
        var = np.zeros(U)
        zs = np.zeros((U, Fs))
        zp = np.zeros((U, Fl))
        for mp in range(G):
            Lm = L[mp]
            own, before = um == mp, um < mp
            zc = np.zeros((U, Fl))
            for k in range(Fl):
                s = np.where(own & (uj == k), 1.0, 0.0)
                if X[mp] is not None:
                    for i in range(Fl):
                        use = (um < mp - 1) | ((um == mp - 1) & (uj <= i))
                        s = np.where(use, s - X[mp][k][i] * zp[:, i], s)
                for i in range(k):
                    use = before | (own & (uj <= i))
                    s = np.where(use, s - Lm[tri(k, i)] * zc[:, i], s)
                zk = s / Lm[tri(k, k)]
                part = before | (own & (uj <= k))
                zc[:, k] = np.where(part, zk, 0.0)
                var = np.where(part, var + zk * zk, var)
            for a in range(Fs):
                for i in range(Fl):
                    use = before | (own & (uj <= i))
                    zs[:, a] = np.where(use, zs[:, a] - Lm[tri(Fl + a, i)] * zc[:, i], zs[:, a])
            zp = zc
        for a in range(Fs):
            s = zs[:, a].copy()
            for i in range(a):
                s = s - Ls[tri(a, i)] * zs[:, i]
            zs[:, a] = s / Ls[tri(a, a)]
            var = var + zs[:, a] * zs[:, a]
        return ss, np.sqrt(var).reshape(G, Fl)


def refine_series_defined(base, shared, local, lo, hi, series_start, obs, forward, smooth, link=None, weights=None, n_iter=10,
                          rel_step=1e-3, lambda0=1e-2, prior_mean=None, prior_weight=None, shared_prior_mean=None,
                          shared_prior_weight=None, history=None, want_std=True, trace=None):
    """base (M, 27) start rows, one per date; shared / local: the Fs + Fl distinct column numbers, Fl >= 1; lo, hi (F,) by name,
    shared first; series_start (S + 1,); obs (M, nb); smooth (Fl,) gamma_b; link None (= 1) or (M,); weights None, (nb,) or
    (M, nb); forward(rows (R, 27)) -> (R, nb).  prior_*: the LOCAL prior, None or both (Fl,) or (M, Fl); shared_prior_*: None or
    both (Fs,) or (S, Fs).
    -> refine_tiles_defined's dict with "tile" read as series; status -1 a bad row, 1 another row of a dead series.
    ``history`` as in refine_tiles_defined; ``trace``: an optional list that receives, per series, the inputs and results of
    every cost sum, augmentation, proposal and std (tests/test_refine_series_host.py feeds them to the g++ build)."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    shared, local = [int(f) for f in shared], [int(f) for f in local]
    free = shared + local
    Fs, Fl, F, (M, nb) = len(shared), len(local), len(free), obs.shape
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(F), np.asarray(hi, dtype=np.float64).reshape(F)
    if not 1 <= F <= MAX_F or len(set(free)) != F or min(free) < 0 or max(free) >= base.shape[1]:
        raise ValueError("shared + local: 1 ... 16 distinct column numbers")
    if Fl < 1:
        raise ValueError("nothing to link: use refine_tiles_defined")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("bounds must be finite with lo < hi")
    if not 0 <= int(n_iter) <= MAX_ITER:
        raise ValueError("n_iter: 0 ... 100")
    ts = check_series_start(series_start, M)
    gamma = smooth_defined(smooth, Fl)
    T = ts.size - 1
    tile_of = np.repeat(np.arange(T), np.diff(ts))
    name = np.array(list(range(Fs, F)) + list(range(Fs)), dtype=np.int64)
    qhi = hi[name]
    nt = F * (F + 1) // 2
    nts = Fs * (Fs + 1) // 2
    ia, ib = packed_pairs(Fs)
    pick = np.concatenate([tri(Fl + ia, Fl + ib), nt + Fl + np.arange(Fs)]).astype(np.int64)

    w = weights_defined(weights, M, nb)
    bad = bad_weights_defined(w)
    mu_l, pw_l = prior_defined(prior_mean, prior_weight, M, Fl)
    mu_s, pw_s = shared_prior_defined(shared_prior_mean, shared_prior_weight, T, Fs) if Fs else (None, None)
    if pw_l is not None:
        bad = bad | bad_weights_defined(pw_l)
        mu_q = np.concatenate([mu_l, np.zeros((M, Fs))], axis=1)
        pw_q = np.concatenate([pw_l, np.zeros((M, Fs))], axis=1)
    bad_tile = bad_weights_defined(pw_s) if pw_s is not None else np.zeros(T, dtype=bool)
    kap, bad_link, _ = kappa_defined(gamma, link, ts)
    bad = bad | bad_link

    h = rel_step * (hi - lo)
    qh = h[name]
    z = clip_defined(base[ts[:-1]][:, shared], lo[:Fs], hi[:Fs]) if Fs else np.zeros((T, 0))
    l = clip_defined(base[:, local], lo[Fs:], hi[Fs:])
    zt, lt = z.copy(), l.copy()
    C = np.full(T, np.inf)
    cost0 = np.full(T, np.nan)
    lam = np.full(T, float(lambda0))
    n_accept = np.zeros(T, dtype=np.int32)
    dead = np.zeros(T, dtype=bool)
    status = np.zeros(M, dtype=np.int32)
    pixel_cost = np.full(M, np.nan)
    packed = np.zeros((M, nt + F))
    S = np.zeros((T, nts + Fs))
    y = np.full((M, nb), np.nan)
    for it in range(int(n_iter) + 1):
        tq = np.concatenate([lt, zt[tile_of]], axis=1)
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
                bad = bad | ~(ct < np.inf)
        Ct = np.zeros(T)
        accept = np.zeros(T, dtype=bool)
        with np.errstate(all="ignore"):
            for t in range(T):
                if dead[t]:
                    continue
                c = 0.0
                for m in range(ts[t], ts[t + 1]):
                    c = c + float(ct[m])
                c = chain_cost_defined(c, kap, lt, ts[t], ts[t + 1])
                if pw_s is not None:
                    for a in range(Fs):
                        if pw_s[t, a] != 0.0:
                            ea = zt[t, a] - mu_s[t, a]
                            c = c + (pw_s[t, a] * ea) * ea
                Ct[t] = c
                if trace is not None:
                    trace.append(("cost", t, ct[ts[t]:ts[t + 1]].copy(), lt[ts[t]:ts[t + 1]].copy(), zt[t].copy(), c))
                if it == 0:
                    accept[t] = bool(c < np.inf) and not bad_tile[t] and not bad[ts[t]:ts[t + 1]].any()
                else:
                    accept[t] = bool(c < C[t])
        if it == 0:
            cost0 = Ct.copy()
            dead = ~accept
            C = np.where(dead, Ct, C)
            n_accept[dead] = -1
            dm = dead[tile_of]
            status[dm] = np.where(bad[dm], -1, 1)
            pixel_cost = np.where(dm, ct, pixel_cost)
            y = np.where(dm[:, None], Y[0], y)
        acc_m = accept[tile_of]
        if acc_m.any():
            with np.errstate(all="ignore"):
                blocks = Y[1:][name]
                J = np.moveaxis((blocks - Y[0][None]) / sh.T[:, :, None], 0, 2)
                new = normal_defined(J, d, w)
                if pw_l is not None:
                    new = prior_normal_defined(new, e, pw_q)
                plain = new.copy()
                augment_defined(new, kap, lt, ts, acc_m, Fl, nt)
                if trace is not None:
                    for t in np.flatnonzero(accept):
                        sl = slice(ts[t], ts[t + 1])
                        trace.append(("augment", t, plain[sl], lt[sl].copy(), new[sl].copy()))
                packed = np.where(acc_m[:, None], new, packed)
                for t in np.flatnonzero(accept):
                    s = np.zeros(nts + Fs)
                    for m in range(ts[t], ts[t + 1]):
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
            lam = np.where(dead, lam, lambda_defined(lam, accept))
            n_accept = n_accept + accept.astype(np.int32)
        if history is not None:
            history.append((z.copy(), l.copy(), C.copy()))
        if it == int(n_iter):
            break
        with np.errstate(all="ignore"):
            for t in np.flatnonzero(~dead):
                b0, b1 = int(ts[t]), int(ts[t + 1])
                A = packed[b0:b1, :nt].copy()
                for j in range(Fl):
                    Ajj = A[:, tri(j, j)]
                    A[:, tri(j, j)] = Ajj + lam[t] * np.where(Ajj > 0.0, Ajj, 1.0)
                Bs = S[t, :nts].copy()
                for a in range(Fs):
                    Saa = Bs[tri(a, a)]
                    Bs[tri(a, a)] = Saa + lam[t] * (Saa if Saa > 0.0 else 1.0)
                L, X, Ls, ok = series_factor_defined(A, kap[b0:b1], Bs, Fs, Fl)
                if ok:
                    ds, dl = series_solve_defined(L, X, Ls, packed[b0:b1, nt:nt + Fl], S[t, nts:], Fs, Fl)
                    ds, dl = np.array(ds, dtype=np.float64).reshape(Fs), np.array(dl, dtype=np.float64).reshape(b1 - b0, Fl)
                    ok = bool(np.isfinite(ds).all()) and bool(np.isfinite(dl).all())
                if not ok:
                    ds, dl = np.zeros(Fs), np.zeros((b1 - b0, Fl))
                zt[t] = clip_defined(z[t] + ds, lo[:Fs], hi[:Fs])
                lt[b0:b1] = clip_defined(l[b0:b1] + dl, lo[Fs:], hi[Fs:])
                if trace is not None:
                    trace.append(("propose", t, packed[b0:b1].copy(), S[t].copy(), float(lam[t]), z[t].copy(), l[b0:b1].copy(),
                                  zt[t].copy(), lt[b0:b1].copy(), ok))
    shared_std = np.full((T, Fs), np.nan)
    local_std = np.full((M, Fl), np.nan)
    if want_std:
        for t in np.flatnonzero(~dead):
            b0, b1 = int(ts[t]), int(ts[t + 1])
            L, X, Ls, ok = series_factor_defined(packed[b0:b1, :nt], kap[b0:b1], S[t, :nts], Fs, Fl)
            if ok:
                shared_std[t], local_std[b0:b1] = series_std_defined(L, X, Ls, Fs, Fl)
            if trace is not None:
                trace.append(("std", t, packed[b0:b1].copy(), S[t].copy(), shared_std[t].copy(), local_std[b0:b1].copy()))
    return {"shared": z, "shared_std": shared_std, "local": l, "local_std": local_std, "cost": C, "cost0": cost0,
            "n_accept": n_accept, "pixel_cost": pixel_cost, "status": status, "y": y}
