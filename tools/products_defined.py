"""The definition of spart_products (include/spart_hip.h) in numpy, float64: fAPAR and albedo, black- and white-sky, and
fCover of a parameter row.  Test infrastructure: it takes the CPU oracle (oracle/spart_oracle.py) as an argument for the leaf,
the soil, the leaf-angle distribution and volscatt, and restates the canopy flux terms operation for operation from the
oracle's sailh (the lines cited there as sailh.py:142-152, 154-210, 222-233), so that the rsd / rdd rebuilt here are the
oracle's bit for bit.  The order of the band sums is numpy's; the kernel's fixed order is compared within a tolerance.

The model as it is: sailh.py:189 has denom = 1 - rinf2 ** 2 where SAIL has 1 - rinf^2 e2.  The isolated canopy therefore does
not conserve energy, fAPAR does not go to 0 with LAI, and a_s / a_d go slightly negative outside the PAR range.  No physical
limit holds for these numbers; they are defined on the model the reflectances come from.
"""
import numpy as np

PRODUCT_NAMES = ("fAPAR_bs", "fAPAR_ws", "albedo_bs", "albedo_ws", "fCover")
NWL = 2001
PAR = slice(0, 301)                          # 400 ... 700 nm
LITAB = np.array([*range(5, 80, 10), *range(81, 91, 2)], dtype=np.float64)       # sailh.py:49


def sun_geometry(oracle, P):
    """k (B, 1), bf (B, 1), lidf (B, 13) of sailh.py:93, 95, 348: functions of LIDFa, LIDFb and tts alone (chi_s of volscatt
    reads no view angle; it is evaluated at tto = 0, psi = 0)"""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    lidf = oracle.calculate_leafangles(P[:, 16], P[:, 17])
    deg2rad = np.pi / 180
    tts = P[:, 19:20]
    zero = np.zeros_like(tts)
    sin_tts, cos_tts = np.sin(tts * deg2rad), np.cos(tts * deg2rad)
    sin_ttli, cos_ttli = np.sin(LITAB[None, :] * deg2rad), np.cos(LITAB[None, :] * deg2rad)
    with np.errstate(all="ignore"):
        chi_s, _, _, _ = oracle.volscatt(sin_tts, cos_tts, np.sin(zero), np.cos(zero), zero, sin_ttli, cos_ttli)
        ksli = chi_s / cos_tts
        bfli = cos_ttli ** 2
        dot = lambda m: np.sum(m * lidf, axis=1, keepdims=True)
        k, bf = dot(ksli), dot(bfli * np.ones_like(ksli))
    return k, bf, lidf


def flux_terms(rho, tau, k, bf, LAI):
    """rho_dd, tau_dd, tau_sd, rho_sd (sailh.py:205-209) and tau_ss (:200) from leaf spectra (B, n) and the sample scalars
    (B, 1); the oracle's operations in the oracle's order"""
    with np.errstate(all="ignore"):
        sdb, sdf = 0.5 * (k + bf), 0.5 * (k - bf)
        ddb, ddf = 0.5 * (1 + bf), 0.5 * (1 - bf)
        sigb = ddb * rho + ddf * tau
        sigf = ddf * rho + ddb * tau
        sb = sdb * rho + sdf * tau
        sf = sdf * rho + sdb * tau
        a = 1 - sigf
        m = np.sqrt(a ** 2 - sigb ** 2)
        rinf = (a - m) / sigb
        rinf2 = rinf * rinf
        x = -1
        sing = np.abs((m - k) * LAI) < 1e-6                                    # calcJ1, :154-170
        normal = (np.exp(m * LAI * x) - np.exp(k * LAI * x)) / (k - m)
        singular = (-0.5 * (np.exp(m * LAI * x) + np.exp(k * LAI * x)) * LAI * x
                    * (1 - 1 / 12 * (k - m) ** 2 * LAI ** 2))
        J1k = np.where(sing, singular, normal)
        x = 0
        J2k = (np.exp(k * LAI * x) - np.exp(-k * LAI) * np.exp(-m * LAI * (1 + x))) / (k + m)   # calcJ2, :172-177
        e1 = np.exp(-m * LAI)
        e2 = e1 ** 2
        re = rinf * e1
        denom = 1 - rinf2 ** 2                                                 # sic, :189
        s1 = sf + rinf * sb
        s2 = sf * rinf + sb
        Pss = s1 * J1k
        Qss = s2 * J2k
        tau_ss = np.exp(-k * LAI)
        tau_dd = (1 - rinf2) * e1 / denom
        rho_dd = rinf * (1 - e2) / denom
        tau_sd = (Pss - re * Qss) / denom
        rho_sd = (Qss - re * Pss) / denom
    return dict(rho_dd=rho_dd, tau_dd=tau_dd, tau_sd=tau_sd, rho_sd=rho_sd, tau_ss=tau_ss)


def band_terms(f, rs):
    """rsd, rdd (sailh.py:232-233, the oracle's expressions) and the two canopy absorptances"""
    with np.errstate(all="ignore"):
        tau_ss, tau_sd, tau_dd, rho_sd, rho_dd = f["tau_ss"], f["tau_sd"], f["tau_dd"], f["rho_sd"], f["rho_dd"]
        denom = 1 - rs * rho_dd
        rsd = rho_sd + (tau_ss + tau_sd) * rs * tau_dd / denom
        rdd = rho_dd + tau_dd * rs * tau_dd / denom
        a_s = 1 - rsd - (1 - rs) * (tau_ss + tau_sd) / denom
        a_d = 1 - rdd - (1 - rs) * tau_dd / denom
    return dict(rsd=rsd, rdd=rdd, a_s=a_s, a_d=a_d)


def fcover_exponent(lidf):
    """sum_j lidf_j cos(litab_j pi / 180), (B,): volscatt's chi_o at tto = 0 summed over the classes"""
    return np.sum(lidf * np.cos(LITAB[None, :] * (np.pi / 180)), axis=1)


def spectra(oracle, tables, P):
    """the per-band terms of the definition on the 2001 model bands: dict rsd, rdd, a_s, a_d, rho_dd, ... (B, 2001), lidf"""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    with np.errstate(all="ignore"):
        refl, tran, _ = oracle.prospect_5d(P[:, 0:9], tables)
        rwet, _ = oracle.bsm(P[:, 9:15], tables)
    k, bf, lidf = sun_geometry(oracle, P)
    f = flux_terms(refl, tran, k, bf, P[:, 15:16])
    out = dict(f)
    out.update(band_terms(f, rwet))
    out.update(lidf=lidf, rs=rwet)
    return out


def products_defined(oracle, tables, P):
    """{name: (B,) float64} for PRODUCT_NAMES"""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    t = spectra(oracle, tables, P)
    Ea = np.asarray(tables["Ea"], dtype=np.float64).reshape(-1)[:NWL]
    with np.errstate(all="ignore"):
        out = {
            "fAPAR_bs": np.sum(Ea[PAR] * t["a_s"][:, PAR], axis=1) / np.sum(Ea[PAR]),
            "fAPAR_ws": np.sum(Ea[PAR] * t["a_d"][:, PAR], axis=1) / np.sum(Ea[PAR]),
            "albedo_bs": np.sum(Ea * t["rsd"], axis=1) / np.sum(Ea),
            "albedo_ws": np.sum(Ea * t["rdd"], axis=1) / np.sum(Ea),
            "fCover": 1 - np.exp(-P[:, 15] * fcover_exponent(t["lidf"])),
        }
    return out
