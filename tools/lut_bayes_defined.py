"""spart_lut_bayes' definition (include/spart_hip.h), literally, in numpy: the likelihood-weighted LUT estimate.

    python tools/lut_bayes_defined.py          (a small self-check against the long-double evaluation, no GPU)

Per observation m, in the LUT's dtype T: the costs c_T(b, m), the row rule and the observation rule are those of
lut_brute_force.brute_force_topk_obs_weights_numpy (called with k = B: every row with a finite cost, ordered by (cost, row)).
    E        the accepted rows with a finite c_T; empty (or an invalid observation): count 0, best_idx -1, best_cost +inf,
             sum_w 0, ess / mean / std NaN
    c*       min c_T over E, best_idx the lowest row attaining it
    e_b      float64(c_T(b)) - float64(c*)
    S        {b in E: e_b <= cut} in ascending row order, count = |S|
    omega_b  exp(-(e_b / (2 tau)))                       (float64; 2 tau formed first)
    sums     float64, sequential over S ascending from 0 (np.add.accumulate: one rounded addition per row, in order):
             sum_w = sum omega;  s2 = sum omega omega;  ess = (sum_w sum_w) / s2
             mean_p = (sum (omega x_bp)) / sum_w;  var_p = (sum ((omega d) d)) / sum_w, d = x_bp - mean_p;  std_p = sqrt(var_p)
numpy rounds every elementwise operation to float64 on its own, so the expressions below ARE the definition; only exp is not
pinned to the bit (numpy's and the device's each keep their own error bound), which is why omega = 1 at e = 0 is the one
value both agree on exactly.

spart_lut_bayes_quantiles adds, per parameter p and level q, the smallest value v among the x_bp of S with F_p(v) >= q sum_w,
F_p(v) the same ordered sum of omega restricted to the rows with x_bp <= v: lut_bayes_quantiles_defined.  quantile_search is
the device kernel's search in numpy, which must give the same values and counts the passes over S it takes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lut_brute_force import brute_force_topk_obs_weights_numpy  # noqa: E402


def _ordered_sum(terms):
    """((0 + t_1) + t_2) + ... along axis 0, one rounded float64 addition per term"""
    zero = np.zeros((1,) + terms.shape[1:])
    return np.add.accumulate(np.concatenate([zero, terms], axis=0), axis=0)[-1]


def members_defined(lut, obs, w, cut=50.0, row_ok=None):
    """per observation: (rows of S ascending (int64), e_b of those rows (float64), best_idx, best_cost); rows is empty for an
    empty E.  ``row_ok`` as for brute_force_topk_obs_weights_numpy (the rows whose unweighted centred norm is finite)."""
    lut = np.ascontiguousarray(lut)
    B = lut.shape[0]
    if B == 0:
        none = np.zeros(0, dtype=np.int64), np.zeros(0), -1, lut.dtype.type(np.inf)
        return [none for _ in range(np.shape(obs)[0])]
    idx, cost = brute_force_topk_obs_weights_numpy(lut, obs, B, w, row_ok=row_ok)
    res = []
    for m in range(idx.shape[0]):
        ok = idx[m] >= 0
        rows, c = idx[m][ok], cost[m][ok]
        if rows.size == 0:
            res.append((rows, np.zeros(0), -1, lut.dtype.type(np.inf)))
            continue
        e = c.astype(np.float64) - np.float64(c[0])                    # (cost, row) order: c[0] = c*, rows[0] = best_idx
        take = e <= cut
        order = np.argsort(rows[take], kind="stable")
        res.append((rows[take][order], e[take][order], int(rows[0]), c[0]))
    return res


def lut_bayes_defined(lut, params, obs, w, cut=50.0, temperature=1.0, row_ok=None):
    """lut (B, nb), obs and w (M, nb) of one float dtype, params (B, P) -> dict: mean, std (M, P) float64, sum_w, ess (M,)
    float64, count, best_idx (M,) int64, best_cost (M,) in the LUT's dtype"""
    lut = np.ascontiguousarray(lut)
    params = np.asarray(params, dtype=np.float64)
    M, P = np.shape(obs)[0], params.shape[1]
    two_tau = np.float64(2.0) * np.float64(1.0 if temperature == 0 else temperature)
    out = {"mean": np.full((M, P), np.nan), "std": np.full((M, P), np.nan), "sum_w": np.zeros(M), "ess": np.full(M, np.nan),
           "count": np.zeros(M, dtype=np.int64), "best_idx": np.full(M, -1, dtype=np.int64),
           "best_cost": np.full(M, np.inf, dtype=lut.dtype)}
    with np.errstate(all="ignore"):
        for m, (rows, e, best, cstar) in enumerate(members_defined(lut, obs, w, cut, row_ok)):
            if rows.size == 0:
                continue
            om = np.exp(-(e / two_tau))
            x = params[rows]
            sw = _ordered_sum(om)
            s2 = _ordered_sum(om * om)
            mean = _ordered_sum(om[:, None] * x) / sw
            d = x - mean
            var = _ordered_sum((om[:, None] * d) * d) / sw
            out["mean"][m], out["std"][m], out["sum_w"][m], out["ess"][m] = mean, np.sqrt(var), sw, (sw * sw) / s2
            out["count"][m], out["best_idx"][m], out["best_cost"][m] = rows.size, best, cstar
    return out


def quantiles_of_members(x, om, levels):
    """spart_lut_bayes_quantiles' definition for ONE observation: x (n, P) the parameter rows of S in ascending row order, om
    (n,) their omega, levels (Q,) -> (P, Q): the smallest data value v with F_p(v) >= q * sum_w, NaN for a column with a NaN.
    F_p(v) is the ordered sum of om over the rows with x <= v; a row that does not qualify adds +0.0, which changes no sum
    >= 0 (the same bits as leaving it out).  F_p is non-decreasing in v, so the smallest qualifying value is found by a
    bisection over the column's sorted values (F_p(max) = sum_w >= q * sum_w: the last one always qualifies); of values that
    compare equal the one in the lowest row is returned."""
    x = np.asarray(x, dtype=np.float64)
    n, P = x.shape
    levels = np.asarray(levels, dtype=np.float64)
    out = np.full((P, levels.size), np.nan)
    if n == 0:
        return out
    Q = levels.size
    with np.errstate(all="ignore"):
        target = (levels * _ordered_sum(om))[None, :]                  # one float64 multiplication per level
        vals = np.sort(x, axis=0)                                      # per column, ascending (a NaN column is overwritten below)
        lo = np.zeros((P, Q), dtype=np.int64)                          # the answer's place in vals[:, p] lies in [lo, hi]
        hi = np.full((P, Q), n - 1, dtype=np.int64)
        cols = np.arange(P)[:, None]
        xx = np.repeat(x[:, :, None], Q, axis=2)
        while (lo < hi).any():
            mid = (lo + hi) // 2
            ok = _ordered_sum(np.where(xx <= vals[mid, cols][None], om[:, None, None], 0.0)) >= target
            hi = np.where(ok, mid, hi)
            lo = np.where(ok, lo, mid + 1)
        first = np.argmax(xx == vals[hi, cols][None], axis=0)          # the lowest row holding a value equal to the answer
        out = x[first, cols]
        out[np.isnan(x).any(axis=0)] = np.nan
    return out


def lut_bayes_quantiles_defined(lut, params, obs, w, levels, cut=50.0, temperature=1.0, row_ok=None, members=None):
    """lut_bayes_defined's arguments and ``levels`` (Q,) in [0, 1] -> (M, P, Q) float64: the weighted quantiles of the parameter
    rows over S (include/spart_hip.h: spart_lut_bayes_quantiles); NaN for an empty E or an invalid observation.  ``members``:
    members_defined's result for the same arguments, if the caller already has it"""
    params = np.asarray(params, dtype=np.float64)
    levels = np.asarray(levels, dtype=np.float64)
    M, P = np.shape(obs)[0], params.shape[1]
    two_tau = np.float64(2.0) * np.float64(1.0 if temperature == 0 else temperature)
    out = np.full((M, P, levels.size), np.nan)
    with np.errstate(all="ignore"):
        for m, (rows, e, _, _) in enumerate(members_defined(lut, obs, w, cut, row_ok) if members is None else members):
            if rows.size:
                out[m] = quantiles_of_members(params[rows], np.exp(-(e / two_tau)), levels)
    return out


def _key(x):
    """the order-preserving unsigned 64-bit image of non-NaN doubles, both zeros on the image of +0.0 (k_lut_posterior_quant's)"""
    b = (np.asarray(x, dtype=np.float64) + 0.0).view(np.uint64)        # (-0.0 + 0.0 = +0.0)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def quantile_search(x, om, levels):
    """k_lut_posterior_quant's search for one observation, step for step in numpy: per column and level an interval [lo, hi] of data
    values on the integer image, pivot = lo + (hi - lo) // 2, one pass over S per step giving F(pivot), the largest x <= pivot
    and the smallest x > pivot.  -> ((P, Q) quantiles, passes over S): what the kernel returns and how many passes it takes
    (the pass that gives sum_w and the ranges not counted).  Columns with a NaN give NaN and take no pass."""
    x = np.asarray(x, dtype=np.float64)
    n, P = x.shape
    levels = np.asarray(levels, dtype=np.float64)
    Q = levels.size
    out = np.full((P, Q), np.nan)
    with np.errstate(all="ignore"):
        good = ~np.isnan(x).any(axis=0)
        xs = x[:, good]
        if n == 0 or xs.shape[1] == 0:
            return out, 0
        k = _key(xs)                                                   # (n, P')
        kk = np.repeat(k[:, :, None], Q, axis=2)                       # (n, P', Q)
        target = (levels * _ordered_sum(om))[None, :]
        lo = np.repeat(k.min(axis=0)[:, None], Q, axis=1)
        hi = np.repeat(k.max(axis=0)[:, None], Q, axis=1)
        passes = 0
        while (lo < hi).any():
            passes += 1
            piv = lo + ((hi - lo) >> np.uint64(1))
            le = kk <= piv[None]
            F = _ordered_sum(np.where(le, om[:, None, None], 0.0))
            bel = np.where(le, kk, np.uint64(0)).max(axis=0)
            abv = np.where(le, ~np.uint64(0), kk).min(axis=0)
            opened = lo < hi
            up = F >= target
            hi = np.where(opened & up, bel, hi)
            lo = np.where(opened & ~up, abv, lo)
        cols = np.flatnonzero(good)
        for j, p in enumerate(cols):
            for i in range(Q):
                out[p, i] = xs[np.argmax(k[:, j] == hi[j, i]), j]
    return out, passes


def lut_bayes_exact(lut, params, obs, w, cut=50.0, temperature=1.0, row_ok=None):
    """the same quantities with the sums by math.fsum (exactly rounded) and omega through numpy.longdouble: what the ordered
    float64 sums are compared against.  -> dict of sum_w, ess, mean, var (float64) and abs_mean, abs_var: the sums of
    |omega x| / sum_w and of omega d^2 / sum_w that scale the rounding bounds of mean and var"""
    import math
    params = np.asarray(params, dtype=np.float64)
    M, P = np.shape(obs)[0], params.shape[1]
    tau = np.longdouble(1.0 if temperature == 0 else temperature)
    out = {k: np.full((M, P), np.nan) for k in ("mean", "var", "abs_mean", "abs_var")}
    out.update(sum_w=np.zeros(M), ess=np.full(M, np.nan))
    for m, (rows, e, _, _) in enumerate(members_defined(lut, obs, w, cut, row_ok)):
        if rows.size == 0:
            continue
        om = np.exp(-(e.astype(np.longdouble) / (2 * tau))).astype(np.float64)
        sw, s2 = math.fsum(om), math.fsum(om * om)
        out["sum_w"][m], out["ess"][m] = sw, sw * sw / s2
        for p in range(P):
            x = params[rows, p]
            mean = math.fsum(om * x) / sw
            d = x - mean
            out["mean"][m, p], out["abs_mean"][m, p] = mean, math.fsum(om * np.abs(x)) / sw
            out["var"][m, p] = out["abs_var"][m, p] = math.fsum(om * d * d) / sw
    return out


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    lut = rng.uniform(0.0, 0.6, (400, 7)).astype(np.float32)
    par = rng.uniform(0.0, 8.0, (400, 5))
    obs = (lut[rng.integers(0, 400, 9)] * (1 + 0.02 * rng.standard_normal((9, 7)))).astype(np.float32)
    w = (1.0 / (0.02 * obs) ** 2).astype(np.float32)
    a, b = lut_bayes_defined(lut, par, obs, w, cut=50.0), lut_bayes_exact(lut, par, obs, w, cut=50.0)
    print("count", a["count"].tolist())
    print("max |sum_w - exact| / exact", float(np.max(np.abs(a["sum_w"] - b["sum_w"]) / b["sum_w"])))
    print("max |mean - exact|", float(np.max(np.abs(a["mean"] - b["mean"]))))
