"""The DEFINITION of spart_sobol (include/spart_hip.h) in numpy: Sobol' first-order and total indices of every band of a sensor
column to F free parameters over their ranges, with delete-one-block jackknife standard errors.  Every line below is one rounded
float64 operation per entry (numpy never contracts), every sum in one pinned order:

  points    x = lo + u * (hi - lo), the difference formed first                                       (points_defined)
  rows      A, B, then C^f = A with column free[f] from B: N (F + 2) rows per site                     (rows_defined)
  shift     c = yA[0];  a = yA - c,  b = yB - c,  d^f = (yC^f - c) - a                                 (terms_defined)
  blocks    the Q = 4 + 3 F quantities sa, sb, saa, sbb, (u_f, t_f, e_f) of 64 consecutive samples joined by the tree
            s = 32, 16, 8, 4, 2, 1: t_r = t_r + t_{r+s} for r < s                                      (tree_defined, blocks_defined)
  totals    over blocks ascending from 0.0                                                             (totals_defined)
  finish    mu, var, mean, S1_f, ST_f (Saltelli et al. 2010, Table 2 (b) and (f), on shifted outputs)  (finish_defined)
  jackknife delete one block, n' = n - 64; se = sqrt((v (G - 1)) / G)                                  (jackknife_defined)

``forward(table)`` maps a (R, 27) table of parameter rows to the (R, nb) column; the tests pass Engine.run (float64, pruned), the
CPU oracle or a toy.  sobol_of_outputs() is the part after the forward model, for outputs that come from elsewhere."""
import numpy as np

BLOCK = 64
MIN_N, MAX_N = 128, 1 << 20
OUTS = ("mean", "var", "S1", "ST", "S1_se", "ST_se")


def points_defined(u, lo, hi):
    u, lo, hi = (np.asarray(v, dtype=np.float64) for v in (u, lo, hi))
    w = hi - lo
    return lo + u * w


def rows_defined(base_row, free, xA, xB):
    """one site's table, (N (F + 2), 27): the rows of A, of B, then of C^0 ... C^(F-1)"""
    N, F = xA.shape
    T = np.repeat(np.asarray(base_row, dtype=np.float64)[None, :], N * (F + 2), axis=0)
    for f, col in enumerate(free):
        T[:, col] = np.tile(xA[:, f], F + 2)
        T[N:2 * N, col] = xB[:, f]
        T[(2 + f) * N:(3 + f) * N, col] = xB[:, f]
    return T


def terms_defined(yA, yB, yC):
    """yA, yB (N, nb), yC (F, N, nb) -> c (nb,) and the per-sample quantities (Q, N, nb) in the workspace's order"""
    c = yA[0].copy()
    a = yA - c
    b = yB - c
    q = [a, b, a * a, b * b]
    for f in range(yC.shape[0]):
        d = (yC[f] - c) - a
        q += [b * d, d * d, d]
    return c, np.stack(q)


def tree_defined(t):
    """t (..., 64, nb) -> (..., nb): the fixed tree over axis -2"""
    t = np.array(t, dtype=np.float64)
    s = BLOCK // 2
    while s >= 1:
        t[..., :s, :] = t[..., :s, :] + t[..., s:2 * s, :]
        s //= 2
    return t[..., 0, :]


def blocks_defined(q):
    """(Q, N, nb) -> block sums (Q, G, nb)"""
    Q, N, nb = q.shape
    return tree_defined(q.reshape(Q, N // BLOCK, BLOCK, nb))


def ordered_sum(x, axis):
    """the sum along ``axis`` in ascending order from 0.0 (np.cumsum adds one entry after the other)"""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    return np.cumsum(np.concatenate([np.zeros((1,) + x.shape[1:]), x]), axis=0)[-1]


def totals_defined(bs):
    return ordered_sum(bs, 1)


def finish_defined(X, n):
    """X (Q, ...) totals, n the sample count as float -> mu, var (...), S1, ST (F, ...)"""
    F = (X.shape[0] - 4) // 3
    n = np.float64(n)
    mu = (X[0] + X[1]) / (2.0 * n)
    m2 = (X[2] + X[3]) / (2.0 * n)
    var = m2 - mu * mu
    U, T, D = X[4::3], X[5::3], X[6::3]
    with np.errstate(all="ignore"):
        S1 = (U / n - mu * (D / n)) / var
        ST = (T / (2.0 * n)) / var
    assert S1.shape[0] == F
    return mu, var, S1, ST


def jackknife_defined(bs, X, N):
    """bs (Q, G, nb), X (Q, nb) -> S1_se, ST_se (F, nb)"""
    G = bs.shape[1]
    Xg = X[:, None, :] - bs                                   # (Q, G, nb): every total without block g
    _, _, S1g, STg = finish_defined(Xg, np.float64(N) - np.float64(BLOCK))        # (F, G, nb)
    out = []
    Gd = np.float64(G)
    with np.errstate(all="ignore"):
        for th in (S1g, STg):
            bar = ordered_sum(th, 1) / Gd
            e = th - bar[:, None, :]
            v = ordered_sum(e * e, 1)
            out.append(np.sqrt((v * (Gd - 1.0)) / Gd))
    return out


def sobol_of_outputs(yA, yB, yC, want_se=True):
    """The definition after the forward model: yA, yB (N, nb), yC (F, N, nb) -> dict mean, var (nb,), S1, ST, S1_se, ST_se (nb, F)"""
    yA, yB, yC = (np.asarray(v, dtype=np.float64) for v in (yA, yB, yC))
    N = yA.shape[0]
    if N % BLOCK or not MIN_N <= N <= MAX_N:
        raise ValueError(f"N = {N}, expected a multiple of {BLOCK} in {MIN_N} ... {MAX_N}")
    with np.errstate(all="ignore"):
        c, q = terms_defined(yA, yB, yC)
        bs = blocks_defined(q)
        X = totals_defined(bs)
        mu, var, S1, ST = finish_defined(X, N)
        res = {"mean": c + mu, "var": var, "S1": S1.T.copy(), "ST": ST.T.copy()}
        if want_se:
            s1, st = jackknife_defined(bs, X, N)
            res["S1_se"], res["ST_se"] = s1.T.copy(), st.T.copy()
    return res


def sobol_defined(base, free, lo, hi, uA, uB, forward, want_se=True):
    """base (M, 27), free (F,) column indices, lo, hi (F,), uA, uB (N, F), forward((R, 27)) -> (R, nb)
    -> dict mean, var (M, nb), S1, ST, S1_se, ST_se (M, nb, F)"""
    base = np.asarray(base, dtype=np.float64)
    uA, uB = np.asarray(uA, dtype=np.float64), np.asarray(uB, dtype=np.float64)
    N, F = uA.shape
    xA, xB = points_defined(uA, lo, hi), points_defined(uB, lo, hi)
    M, R = base.shape[0], N * (F + 2)
    if M == 0:
        return {}
    # (one forward call for all sites: a row's column is a function of the row alone)
    Y = np.asarray(forward(np.concatenate([rows_defined(base[m], free, xA, xB) for m in range(M)])), dtype=np.float64)
    sites = []
    for m in range(M):
        y = Y[m * R:(m + 1) * R]
        sites.append(sobol_of_outputs(y[:N], y[N:2 * N], y[2 * N:].reshape(F, N, -1), want_se))
    return {k: np.stack([s[k] for s in sites]) for k in sites[0]}
