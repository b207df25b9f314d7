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
value both agree on exactly."""
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
