"""Does a sensor's SRF column j belong to its band centre j?

The SRF-convolved columns (band_model="srf"; include/spart_hip.h: spart_materialize.R_TOC_srf ...) convolve band j's canopy
spectra with column j of wl_srf_smac / p_srf_smac and take the result through the SMAC coefficients of band j.  The reference
only ever uses the SRF columns for the extraterrestrial irradiance, and two of its packaged tables carry them in another band
order than wl_smac / SMAC_coef: MODIS (12 of 20 centres lie inside their own column's wavelength extent) and OLCI-A / -B
(0 of 21).  The engine and the C ABI do what the tables say; these two functions let a caller see and mend the pairing.
Pure numpy, no GPU.
"""
import numpy as np

# A sample counts as weighted when |p| exceeds this fraction of its column's largest |p|: half a unit in the last place of
# the column's weight sum, so a sample below it cannot change the convolved value's leading digits.  Without the floor the
# packaged Sentinel-2B table, whose padding holds wavelengths of +-9e306 nm with weights of 6.9e-310, would have bands whose
# "extent" is the whole real line and the test below would say nothing about them.
WEIGHT_FLOOR = 2.0 ** -53


def _srf(sensorinfo):
    wl = np.asarray(sensorinfo["wl_smac"], dtype=np.float64).reshape(-1)
    w = np.asarray(sensorinfo["wl_srf_smac"], dtype=np.float64)
    p = np.asarray(sensorinfo["p_srf_smac"], dtype=np.float64)
    if w.ndim != 2 or w.shape != p.shape or w.shape[1] != wl.size:
        raise ValueError(f"wl_srf_smac {w.shape} / p_srf_smac {p.shape} must both be (nsrf, {wl.size})")
    ok = np.isfinite(w) & np.isfinite(p)
    pmax = np.where(ok, np.abs(p), 0.0).max(axis=0)
    return wl, w, p, ok & (p != 0) & (np.abs(p) > WEIGHT_FLOOR * pmax)      # the weighted, finite samples


def _inside(wl, w, used):
    lo = np.where(used, w, np.inf).min(axis=0)
    hi = np.where(used, w, -np.inf).max(axis=0)
    return (lo <= wl) & (wl <= hi)                                     # (a band without a weighted sample: False)


def check_srf(sensorinfo):
    """(nb,) bool: band j's centre wl_smac[j] lies inside the wavelength extent of the weighted (|p| above WEIGHT_FLOOR of the
    column's largest), finite samples of ITS SRF column.  All true for Landsat 4 / 5 / 7 / 8 and Sentinel-2A / 2B as packaged; 12 of 20 for MODIS, none of 21 for
    OLCI-A / -B."""
    wl, w, _, used = _srf(sensorinfo)
    return _inside(wl, w, used)


def align_srf(sensorinfo):
    """A copy of ``sensorinfo`` whose SRF columns (wl_srf_smac, p_srf_smac) are permuted to the order of the band centres:
    the column with the k-th smallest centroid (weighted mean wavelength of its weighted, finite samples) goes to the band
    with the k-th smallest centre.  wl_smac, SMAC_coef and band_id_smac keep their order, and so does everything the centre
    columns are made of -- except the convolved irradiance La, which is the SRF's.  The identity on the six aligned packaged
    sensors; 20 of 20 / 21 of 21 centres inside their extent for MODIS / OLCI.  ValueError if a centre still falls outside
    the extent of the column it is paired with (the tables then do not describe the same bands)."""
    wl, w, p, used = _srf(sensorinfo)
    if not used.any(axis=0).all():
        raise ValueError("align_srf: a band's SRF column has no weighted, finite sample")
    with np.errstate(all="ignore"):
        centroid = np.where(used, w * p, 0.0).sum(axis=0) / np.where(used, p, 0.0).sum(axis=0)
    if not np.isfinite(centroid).all():
        raise ValueError("align_srf: a band's SRF column has no finite centroid (its weights sum to zero)")
    perm = np.empty(wl.size, dtype=np.int64)
    perm[np.argsort(wl, kind="stable")] = np.argsort(centroid, kind="stable")     # band j takes column perm[j]
    out = dict(sensorinfo)
    out["wl_srf_smac"] = np.ascontiguousarray(w[:, perm])
    out["p_srf_smac"] = np.ascontiguousarray(p[:, perm])
    bad = np.flatnonzero(~_inside(wl, out["wl_srf_smac"], used[:, perm]))
    if bad.size:
        raise ValueError(f"align_srf: after pairing by rank the centres of bands {bad.tolist()} still lie outside their SRF's extent")
    return out
