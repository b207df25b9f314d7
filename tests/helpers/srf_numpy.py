"""The SRF convolution of spectra on the model grid, restated in plain numpy (no GPU, no library).

calculate_spectral_convolution (SPART.py:358-396) maps every SRF sample wavelength to its nearest point of the spectrum's
wavelength axis -- np.argmin(np.abs(grid - w)): first minimum, so ties go to the lower index and a NaN wavelength gives
index 0 -- and returns sum(spectrum[idx] * p) / sum(p) per band.  Applied to the 2162-point grid wlS this file is the
definition include/spart_hip.h states for the *_srf outputs and for spart_srf_support.

For |w| >= 1e15 the float64 subtraction grid - w no longer tells the grid points apart and the literal argmin returns 0
whatever the sign of w, while the definition takes the nearest point in exact arithmetic: the last grid point for a huge
positive w.  nearest_index_literal is the argmin as it stands; nearest_index is the definition: the literal argmin for every
|w| < 1e15 and the end point on w's side beyond.  The packaged tables hold 20 such wavelengths, all in Sentinel-2B with
weights <= 7e-310: 19 negative ones (index 0 either way) and one of +9.1e306 in band 4, which the definition sends to the
thermal evaluation (one more support entry than the literal form, 963 instead of 962, carrying a weight of 6.9e-310).
"""
import numpy as np

NWL, NWLS = 2001, 2162


def wl_solar():
    """wlS (SPART.py:303-310): 400..2400 nm by 1, 2500..15000 by 100, 16000..50000 by 1000"""
    return np.concatenate([np.arange(400, 2401, 1), np.arange(2500, 15001, 100),
                           np.arange(16000, 50001, 1000)]).astype(np.float64)


def nearest_index_literal(wl_srf):
    """(nsrf, nb) int64: np.argmin(|wlS - w|) per SRF sample, literally (get_closest_index, SPART.py:381-387)"""
    w = np.asarray(wl_srf, dtype=np.float64)
    g = wl_solar()
    with np.errstate(invalid="ignore"):
        return np.argmin(np.abs(g[:, None] - w.reshape(1, -1)), axis=0).reshape(w.shape).astype(np.int64)


def nearest_index(wl_srf):
    """the definition: the literal argmin, and for |w| >= 1e15 -- where the subtraction above has lost the grid -- the
    nearest point in exact arithmetic, i.e. the first grid point for negative and the last for positive w"""
    w = np.asarray(wl_srf, dtype=np.float64)
    idx = nearest_index_literal(w)
    with np.errstate(invalid="ignore"):
        idx[w >= 1e15] = NWLS - 1
        idx[w <= -1e15] = 0
    return idx


def evaluation_index(wl_srf):
    """the model evaluation a grid point stands for: 0..2000 = 400..2400 nm, 2001 = the one thermal evaluation (all 161
    thermal pad bands hold the same value, SPART.py:427-470)"""
    return np.minimum(nearest_index(wl_srf), NWL)


def support(wl_srf, p_srf):
    """The compressed support of every band, with plain Python sums in SRF-sample order:
    -> (start (nb + 1,) int32, ev (n,) int32, q (n,) float64, Q (nb,) float64); band j owns entries start[j]:start[j + 1],
    ev ascending and distinct, q[e] = sum of p_srf[i, j] over the samples i that map to ev[e], Q[j] = sum_i p_srf[i, j]."""
    p = np.asarray(p_srf, dtype=np.float64)
    idx = evaluation_index(wl_srf)
    nsrf, nb = p.shape
    start, ev, q, Q = [0], [], [], []
    for j in range(nb):
        acc, tot = {}, 0.0
        for i in range(nsrf):
            pij = float(p[i, j])
            e = int(idx[i, j])
            acc[e] = acc.get(e, 0.0) + pij
            tot = tot + pij
        for e in sorted(acc):
            ev.append(e)
            q.append(acc[e])
        start.append(len(ev))
        Q.append(tot)
    return np.array(start, np.int32), np.array(ev, np.int32), np.array(q, np.float64), np.array(Q, np.float64)


def convolve_literal(spectrum, wl_srf, p_srf):
    """calculate_spectral_convolution(wlS[:, None], spectrum, sensorinfo) for (B, 2162) spectra -> (B, nb), in the
    reference's own form: gather, multiply, sum over the SRF samples, divide"""
    x = np.asarray(spectrum, dtype=np.float64)
    p = np.asarray(p_srf, dtype=np.float64)
    idx = nearest_index_literal(wl_srf)
    with np.errstate(all="ignore"):
        return np.sum(x[:, idx] * p[None], axis=1) / np.sum(p, axis=0)[None]


def convolve(spectrum, wl_srf, p_srf, lists=None):
    """The same convolution through the compressed support, in the order the library defines:
    x_srf[s, j] = (sum over e in E_j ascending of q_e x[s, e]) / Q_j.  Differs from convolve_literal by the rounding of a
    re-ordered sum only.  ``lists``: (start, ev, q, Q) to use in place of support(wl_srf, p_srf), e.g. spart_srf_support's."""
    x = np.asarray(spectrum, dtype=np.float64)
    start, ev, q, Q = support(wl_srf, p_srf) if lists is None else lists
    grid_of = np.where(ev < NWL, ev, NWL)             # evaluation 2001 = any thermal pad band: take the first
    out = np.empty((x.shape[0], len(Q)))
    with np.errstate(all="ignore"):
        for j in range(len(Q)):
            acc = np.zeros(x.shape[0])
            for e in range(start[j], start[j + 1]):
                acc = acc + q[e] * x[:, grid_of[e]]
            out[:, j] = acc / Q[j]
    return out


def toc_to_toa(at, rso, rdo, rsd, rdd, La):
    """SPART.py:243-252 on (B, nb) arrays; ``at``: the nine SMAC outputs by name -> R_TOC, R_TOA, L_TOA"""
    with np.errstate(all="ignore"):
        den = 1 - rdd * at["Ra_dd"]
        rtoa0 = at["Ra_so"] + at["Ta_ss"] * rso * at["Ta_oo"]
        rtoa1 = (at["Ta_sd"] * rdo + at["Ta_ss"] * rsd * at["Ra_dd"] * rdo) * at["Ta_oo"] / den
        rtoa2 = (at["Ta_ss"] * rsd + at["Ta_sd"] * rdd) * at["Ta_do"] / den
        R_TOC = (at["Ta_ss"] * rso + at["Ta_sd"] * rdo) / (at["Ta_ss"] + at["Ta_sd"])
        R_TOA = at["Tg"] * (rtoa0 + rtoa1 + rtoa2)
        return R_TOC, R_TOA, La * R_TOA


def rel_err(x, ref):
    """max |x - ref| / max(|ref|, 1e-6), NaN-aware: a NaN must sit where the reference has one, and only there"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.array_equal(np.isnan(x), np.isnan(ref)):
        return np.inf
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(x[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-6)
    d = np.where(x[ok] == ref[ok], 0.0, d)            # (equal infinities)
    return float(np.max(d))
