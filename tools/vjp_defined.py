"""spart_vjp as include/spart_hip.h defines it, in numpy: the text of the header's comment, operation by operation.  numpy's
float64 +, -, *, / are single IEEE operations without contraction, so what this file computes is what the library must
return bit for bit, given the same forward model.

    vjp_defined(base, free, lo, hi, gy, forward, rel_step=1e-3) -> grad (M, F)

base (M, 27); free: F column numbers; lo, hi (F,); gy: three entries, each None or (M, nb), the loss's gradient with respect to
R_TOC, R_TOA, L_TOA; forward(rows (R, 27)) -> three (R, nb) arrays (an entry nobody reads may be None).  The tests hand in the
library's own float64 pruned column path, or a toy model.
"""
import numpy as np

REL_STEP, MAX_REL_STEP = 1e-3, 0.5
ROWS = 1 << 19           # rows of one forward call at most: observations go in chunks of ROWS // (2 F)


def chunk_of(F):
    return ROWS // (2 * F)


def clip_defined(v, lo, hi):
    """t = v; if t < lo: t = lo; if t > hi: t = hi (a NaN stays a NaN)"""
    with np.errstate(invalid="ignore"):
        t = np.where(v < lo, lo, v)
        return np.where(t > hi, hi, t)


def steps_defined(x, lo, hi, rel_step=REL_STEP):
    """x (M, F) clipped -> a, b (M, F): a = x + h, put back on hi where it passes it; b = x - h, put back on lo"""
    h = rel_step * (hi - lo)
    with np.errstate(invalid="ignore"):
        a = x + h
        a = np.where(a > hi, hi, a)
        b = x - h
        b = np.where(b < lo, lo, b)
    return a, b


def rows_defined(base, free, x, a, b):
    """-> (2 F, M, 27): row 2 f is base with every free column at x and column free[f] at a_f, row 2 f + 1 the same with b_f"""
    F = len(free)
    point = np.array(base, dtype=np.float64)
    point[:, free] = x
    T = np.repeat(point[None], 2 * F, axis=0)
    for f in range(F):
        T[2 * f, :, free[f]] = a[:, f]
        T[2 * f + 1, :, free[f]] = b[:, f]
    return T


def sum_defined(gy, Yp, Ym):
    """gy: three entries None or (M, nb); Yp, Ym: three entries None or (F, M, nb) -> s (M, F): c ascending over the entries that
    are there, j ascending, a band of g == 0 skipped, otherwise s = s + g * (Y+ - Y-)"""
    first = next(i for i in range(3) if gy[i] is not None)
    F, M, nb = Yp[first].shape
    s = np.zeros((M, F))
    with np.errstate(all="ignore"):
        for c in range(3):
            if gy[c] is None:
                continue
            for j in range(nb):
                g = np.asarray(gy[c], dtype=np.float64)[:, j][:, None]
                d = (Yp[c][:, :, j] - Ym[c][:, :, j]).T
                s = np.where(g == 0.0, s, s + g * d)
    return s


def vjp_defined(base, free, lo, hi, gy, forward, rel_step=REL_STEP):
    base = np.asarray(base, dtype=np.float64)
    free = list(free)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    M, F = base.shape[0], len(free)
    x = clip_defined(base[:, free], lo, hi)
    a, b = steps_defined(x, lo, hi, rel_step)
    T = rows_defined(base, free, x, a, b)
    Y = forward(T.reshape(2 * F * M, 27))
    Yp, Ym = [None] * 3, [None] * 3
    for c in range(3):
        if gy[c] is not None:
            y = np.asarray(Y[c], dtype=np.float64).reshape(F, 2, M, -1)
            Yp[c], Ym[c] = y[:, 0], y[:, 1]
    with np.errstate(all="ignore"):
        return sum_defined(gy, Yp, Ym) / (a - b)
