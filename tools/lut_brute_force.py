"""Brute-force checkers of spart_lut_nearest, spart_lut_topk, spart_lut_topk_obs_weights and spart_lut_summarise (tests/ and
bench.py; tooling, not product).

The cost is DEFINED (include/spart_hip.h) as the sequential evaluation, in the call's dtype and without fused multiply-adds,

    c = 0;  for j = 0 .. nb-1:  d = lut[b, j] - obs[m, j];  c = c + (w_j * d) * d        (w = None: c = c + d * d)

and the answer as the LOWEST row index attaining the minimum; rows whose cost is NaN / +inf never win (-1 / +inf).  This is the
reference's own nearest-index rule -- an exact np.argmin, first index on ties (/root/reference/src/SPART/SPART.py:381-387) --
applied to the weighted squared distance.  numpy / eager torch evaluate every elementwise operation on its own, rounded to the
array dtype, so the loops below ARE that definition.
"""
import numpy as np


def brute_force_numpy(lut, obs, w=None):
    """lut (B, nb), obs (M, nb), w (nb,) or None, all of ONE float dtype -> (idx (M,) int64, cost (M,) dtype)"""
    lut = np.ascontiguousarray(lut)
    dt = lut.dtype
    obs = np.ascontiguousarray(obs, dtype=dt)
    w = None if w is None else np.asarray(w, dtype=dt)
    B, nb = lut.shape
    M = obs.shape[0]
    idx = np.full(M, -1, dtype=np.int64)
    cost = np.full(M, np.inf, dtype=dt)
    cols = [np.ascontiguousarray(lut[:, j]) for j in range(nb)]
    with np.errstate(all="ignore"):
        for m in range(M):
            c = np.zeros(B, dtype=dt)
            for j in range(nb):
                d = cols[j] - obs[m, j]
                t = d if w is None else w[j] * d
                c = c + t * d
            c[~np.isfinite(c)] = np.inf
            i = int(np.argmin(c))                     # first index of the minimum
            if c[i] < np.inf:
                idx[m], cost[m] = i, c[i]
    return idx, cost


def brute_force_torch(lut, obs, w=None, max_elems=1 << 27):
    """the same on the GPU with eager torch ops (one kernel per operation: no contraction), in blocks of observations.
    lut (B, nb), obs (M, nb), w (nb,) or None: tensors of one dtype on one device -> (idx int64, cost)"""
    import torch
    B, nb = lut.shape
    M = obs.shape[0]
    inf = float("inf")
    cols = [lut[:, j].contiguous() for j in range(nb)]
    rows = torch.arange(B, device=lut.device, dtype=torch.int64)
    idx = torch.full((M,), -1, dtype=torch.int64, device=lut.device)
    cost = torch.full((M,), inf, dtype=lut.dtype, device=lut.device)
    mb = max(1, min(M, max_elems // max(B, 1)))
    for m0 in range(0, M, mb):
        o = obs[m0:m0 + mb]
        c = torch.zeros((o.shape[0], B), dtype=lut.dtype, device=lut.device)
        for j in range(nb):
            d = cols[j][None, :] - o[:, j][:, None]
            t = d if w is None else w[j] * d
            c = c + t * d
        c = torch.where(torch.isfinite(c), c, torch.full_like(c, inf))
        cmin = c.min(dim=1).values
        first = torch.where(c == cmin[:, None], rows[None, :], torch.full_like(rows, B)[None, :]).min(dim=1).values
        ok = cmin < inf
        idx[m0:m0 + mb] = torch.where(ok, first, torch.full_like(first, -1))
        cost[m0:m0 + mb] = cmin
    return idx, cost


def _topk_from_costs_numpy(c, k):
    """c (B,) costs -> the first k of the stable argsort with non-finite costs as +inf, padded with (-1, +inf)"""
    c = np.where(np.isfinite(c), c, np.inf)
    o = np.argsort(c, kind="stable")[:k]
    o = o[c[o] < np.inf]
    idx = np.full(k, -1, dtype=np.int64)
    cost = np.full(k, np.inf, dtype=c.dtype)
    idx[:len(o)], cost[:len(o)] = o, c[o]
    return idx, cost


def brute_force_topk_numpy(lut, obs, k, w=None, row_ok=None):
    """spart_lut_topk's definition: per observation the first k entries of np.argsort(c, kind="stable") after non-finite
    costs are set to +inf (rows of a non-finite cost never appear; (-1, +inf) pads) -> (idx (M, k) int64, cost (M, k)).
    ``row_ok`` (B,) bool: the rows that count at all (norm_rule_numpy: the overflowing-norm rule); None = every row."""
    lut = np.ascontiguousarray(lut)
    dt = lut.dtype
    obs = np.ascontiguousarray(obs, dtype=dt)
    w = None if w is None else np.asarray(w, dtype=dt)
    B, nb = lut.shape
    M = obs.shape[0]
    idx = np.full((M, k), -1, dtype=np.int64)
    cost = np.full((M, k), np.inf, dtype=dt)
    cols = [np.ascontiguousarray(lut[:, j]) for j in range(nb)]
    with np.errstate(all="ignore"):
        for m in range(M):
            c = np.zeros(B, dtype=dt)
            for j in range(nb):
                d = cols[j] - obs[m, j]
                t = d if w is None else w[j] * d
                c = c + t * d
            if row_ok is not None:
                c[~np.asarray(row_ok)] = np.inf
            idx[m], cost[m] = _topk_from_costs_numpy(c, k)
    return idx, cost


def brute_force_topk_torch(lut, obs, k, w=None, max_elems=1 << 27, row_ok=None):
    """the same with eager torch ops (one kernel per operation: no contraction), in blocks of observations: tensors of one
    dtype on one device -> (idx (M, k) int64, cost (M, k)).  The (cost, row) order is a stable sort by cost of the rows in
    ascending order, i.e. the lowest row first among equal costs.  ``row_ok`` (B,) bool tensor or None, as above."""
    import torch
    B, nb = lut.shape
    M = obs.shape[0]
    inf = float("inf")
    cols = [lut[:, j].contiguous() for j in range(nb)]
    idx = torch.full((M, k), -1, dtype=torch.int64, device=lut.device)
    cost = torch.full((M, k), inf, dtype=lut.dtype, device=lut.device)
    kk = min(k, B)
    mb = max(1, min(M, max_elems // max(B, 1)))
    for m0 in range(0, M, mb):
        o = obs[m0:m0 + mb]
        c = torch.zeros((o.shape[0], B), dtype=lut.dtype, device=lut.device)
        for j in range(nb):
            d = cols[j][None, :] - o[:, j][:, None]
            t = d if w is None else w[j] * d
            c = c + t * d
        fin = torch.isfinite(c) if row_ok is None else torch.isfinite(c) & row_ok[None, :]
        c = torch.where(fin, c, torch.full_like(c, inf))
        s, order = torch.sort(c, dim=1, stable=True)
        s, order = s[:, :kk], order[:, :kk]
        ok = s < inf
        idx[m0:m0 + mb, :kk] = torch.where(ok, order, torch.full_like(order, -1))
        cost[m0:m0 + mb, :kk] = s
    return idx, cost


def norm_rule_numpy(lut, centre, w=None):
    """The row rule of every search (include/spart_hip.h): a row counts only if all its entries are finite and its centred
    norm  n = 0; for j ascending: xc = lut[b, j] - centre[j]; n = n + (|w_j| * xc) * xc  is finite in the LUT's dtype.  The
    verdict depends on the centres only for entries near the square root of the largest finite number; ``centre`` (nb,) is
    the caller's stand-in for the device's column centres (any value between a column's moderate entries gives the same
    verdict on a LUT whose other entries are moderate).  The obs-weights search applies it without weights (w = None).
    -> row_ok (B,) bool, the ``row_ok`` argument of the brute forces below."""
    lut = np.ascontiguousarray(lut)
    dt = lut.dtype
    centre = np.asarray(centre, dtype=dt)
    n = np.zeros(lut.shape[0], dtype=dt)
    with np.errstate(all="ignore"):
        for j in range(lut.shape[1]):
            xc = lut[:, j] - centre[j]
            n = n + ((xc if w is None else abs(dt.type(w[j])) * xc) * xc)
    return np.isfinite(lut).all(axis=1) & np.isfinite(n)


def _obs_weights_checks(lut, obs, w):
    """the row and observation rules of spart_lut_topk_obs_weights: rows with a non-finite entry never appear; an observation
    with a negative or non-finite weight, or a non-finite value in a band of non-zero weight, matches nothing"""
    row_ok = np.isfinite(lut).all(axis=1)
    obs_ok = ((w >= 0) & np.isfinite(w) & ((w == 0) | np.isfinite(obs))).all(axis=1)
    return row_ok, obs_ok


def brute_force_topk_obs_weights_numpy(lut, obs, k, w, row_ok=None):
    """spart_lut_topk_obs_weights' definition, literally: per observation m
        c = 0;  for j: if w[m, j] == 0: skip;  d = lut[:, j] - obs[m, j];  c = c + (w[m, j] * d) * d
    then the first k of the stable argsort (non-finite costs as +inf), padded with (-1, +inf).  lut (B, nb), obs and w (M, nb)
    of one float dtype -> (idx (M, k) int64, cost (M, k)).  ``row_ok`` (B,) bool: the rows whose UNWEIGHTED centred norm is
    finite (norm_rule_numpy(lut, centre)): the search's row rule, which does not depend on the observation; it is applied on
    top of the finite-entries rule.  None = no norm near overflow."""
    lut = np.ascontiguousarray(lut)
    dt = lut.dtype
    obs = np.ascontiguousarray(obs, dtype=dt)
    w = np.ascontiguousarray(w, dtype=dt)
    B, nb = lut.shape
    M = obs.shape[0]
    idx = np.full((M, k), -1, dtype=np.int64)
    cost = np.full((M, k), np.inf, dtype=dt)
    fin_ok, obs_ok = _obs_weights_checks(lut, obs, w)
    row_ok = fin_ok if row_ok is None else fin_ok & np.asarray(row_ok)
    cols = [np.ascontiguousarray(lut[:, j]) for j in range(nb)]
    with np.errstate(all="ignore"):
        for m in range(M):
            if not obs_ok[m]:
                continue
            c = np.zeros(B, dtype=dt)
            for j in range(nb):
                if w[m, j] == 0:
                    continue
                d = cols[j] - obs[m, j]
                c = c + (w[m, j] * d) * d
            c[~row_ok] = np.inf
            idx[m], cost[m] = _topk_from_costs_numpy(c, k)
    return idx, cost


def brute_force_topk_obs_weights_torch(lut, obs, k, w, max_elems=1 << 27, row_ok=None):
    """the same with eager torch ops, in blocks of observations; a masked band keeps the running cost as it is
    (torch.where), which is the skip.  Tensors of one dtype on one device -> (idx (M, k) int64, cost (M, k))"""
    import torch
    B, nb = lut.shape
    M = obs.shape[0]
    inf = float("inf")
    cols = [lut[:, j].contiguous() for j in range(nb)]
    row_ok = torch.isfinite(lut).all(dim=1) if row_ok is None else torch.isfinite(lut).all(dim=1) & row_ok
    obs_ok = ((w >= 0) & torch.isfinite(w) & ((w == 0) | torch.isfinite(obs))).all(dim=1)
    idx = torch.full((M, k), -1, dtype=torch.int64, device=lut.device)
    cost = torch.full((M, k), inf, dtype=lut.dtype, device=lut.device)
    kk = min(k, B)
    mb = max(1, min(M, max_elems // max(B, 1)))
    for m0 in range(0, M, mb):
        o, ww = obs[m0:m0 + mb], w[m0:m0 + mb]
        c = torch.zeros((o.shape[0], B), dtype=lut.dtype, device=lut.device)
        for j in range(nb):
            wj = ww[:, j][:, None]
            d = cols[j][None, :] - o[:, j][:, None]
            c = torch.where(wj == 0, c, c + (wj * d) * d)
        ok = torch.isfinite(c) & row_ok[None, :] & obs_ok[m0:m0 + mb, None]
        c = torch.where(ok, c, torch.full_like(c, inf))
        s, order = torch.sort(c, dim=1, stable=True)
        s, order = s[:, :kk], order[:, :kk]
        fin = s < inf
        idx[m0:m0 + mb, :kk] = torch.where(fin, order, torch.full_like(order, -1))
        cost[m0:m0 + mb, :kk] = s
    return idx, cost


def summarise_defined(params, idx):
    """spart_lut_summarise's definition (include/spart_hip.h), literally, in float64.  For observation m the places j with
    0 <= idx[m, j] < B are taken in place order (every other value -- the -1 padding, anything out of range -- is skipped),
    x_i = params[idx[m, j_i]], and per parameter
        count = n;   mean = (((x_1 + x_2) + x_3) + ... + x_n) / n;   std = sqrt((((x_1 - mean)^2 + (x_2 - mean)^2) + ...) / n)
        median = NaN if any x_i is NaN, else s[(n-1)/2] (n odd) or (s[n/2 - 1] + s[n/2]) / 2 (n even), s the ascending sort
    and NaN for all three when n = 0.  The sums are plain loops over the places, all observations at once (no np.sum: its order is not
    promised); numpy rounds every elementwise operation to float64 on its own, so the loops ARE the definition.
    params (B, P), idx (M, k) -> (mean, median, std (M, P) float64, count (M,) int32)"""
    params = np.asarray(params, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    B, P = params.shape
    M, k = idx.shape
    ok = (idx >= 0) & (idx < B)                                       # the places that count
    safe = np.where(ok, idx, 0)
    rows = params if B > 0 else np.full((1, P), np.nan)               # (an empty table: nothing is in range)
    count = np.zeros(M, dtype=np.int32)
    s = np.zeros((M, P))
    with np.errstate(all="ignore"):
        for j in range(k):                                            # place by place, every observation at once
            x, take = rows[safe[:, j]], ok[:, j]
            first = take & (count == 0)
            s = np.where(first[:, None], x, np.where(take[:, None], s + x, s))
            count += take
        n = count.astype(np.float64)[:, None]
        mean = np.where(n > 0, s / n, np.nan)
        q, seen = np.zeros((M, P)), np.zeros(M, dtype=np.int32)
        for j in range(k):
            x, take = rows[safe[:, j]], ok[:, j]
            d = x - mean
            first = take & (seen == 0)
            q = np.where(first[:, None], d * d, np.where(take[:, None], q + d * d, q))
            seen += take
        std = np.where(n > 0, np.sqrt(q / n), np.nan)
        X = np.where(ok[:, :, None], rows[safe], np.nan)              # (M, k, P); skipped places sort last, as NaN
        has_nan = (np.isnan(X) & ok[:, :, None]).any(axis=1)
        srt = np.sort(X, axis=1)
        m = np.arange(M)
        a, b = srt[m, np.maximum(count - 1, 0) // 2], srt[m, np.minimum(count // 2, k - 1)]
        median = np.where((count % 2 == 1)[:, None], a, (a + b) / np.float64(2))
        median = np.where(has_nan | (count == 0)[:, None], np.nan, median)
    return mean, median, std, count
