"""ctypes binding of libspart_hip.so (include/spart_hip.h).  There is no CPU path: if the
library or a GPU is missing every compute entry point raises."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(HERE, "..", "libspart_hip.so"))

SPART_F32, SPART_F64 = 0, 1
NPARAM, NCOEF, NWL, NWLS, NLINCL = 27, 48, 2001, 2162, 13
NLAYERS = 60            # SPART_NLAYERS: CanopyStructure's default (sailh.py:345)
ABI_VERSION = 14        # SPART_ABI_VERSION of include/spart_hip.h this binding was written against

c_dp = ctypes.POINTER(ctypes.c_double)
vp = ctypes.c_void_p


class SpartTables(ctypes.Structure):
    _fields_ = [(n, c_dp) for n in ("nr", "Kab", "Kca", "Kdm", "Kw", "Ks", "Kant", "cbc", "prot", "GSV", "nw", "Ea")] + [
        ("nb", ctypes.c_int32), ("wl_smac", c_dp), ("coef", c_dp), ("nsrf", ctypes.c_int32), ("wl_srf", c_dp),
        ("p_srf", c_dp)]


class SpartMaterialize(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("leaf_refl", "leaf_tran", "leaf_kchl", "soil_refl", "soil_refl_dry", "rso", "rdo",
                                  "rsd", "rdd", "rsoil", "La", "rdry_in", "band_mean")] + [("prune_unused_bands", ctypes.c_int32),
                                                                                          ("f32_columns", ctypes.c_int32),
                                                                                          ("f32_bands", ctypes.c_int32),
                                                                                          ("fast_prelude", ctypes.c_int32),
                                                                                          ("lidf_in", vp),
                                                                                          ("nlayers", ctypes.c_int32)] + [
        (n, vp) for n in ("R_TOC_srf", "R_TOA_srf", "L_TOA_srf", "rso_srf", "rdo_srf", "rsd_srf", "rdd_srf")]


class SpartRefineOpt(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("column", "n_iter", "weights_per_obs", "fast_prelude", "nlayers")] + [
        ("rel_step", ctypes.c_double), ("lambda0", ctypes.c_double), ("prior_per_obs", ctypes.c_int32), ("prior_mean", vp),
        ("prior_weight", vp)]


class SpartRefineViewsOpt(ctypes.Structure):
    _fields_ = [("fit", SpartRefineOpt), ("V", ctypes.c_int32), ("n_shared", ctypes.c_int32), ("band_model", ctypes.c_int32)]


class SpartRefineMixOpt(ctypes.Structure):
    _fields_ = [("fit", SpartRefineOpt), ("V", ctypes.c_int32), ("n_shared", ctypes.c_int32), ("band_model", ctypes.c_int32),
                ("fit_fractions", ctypes.c_int32), ("local_active", ctypes.POINTER(ctypes.c_int32)),      # local_active: HOST (V, Fl)
                ("frac_lo", ctypes.c_double), ("frac_hi", ctypes.c_double)]


class SpartRefineMixOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("x", "cost", "cost0", "std", "n_accept", "y", "frac", "y_comp")]


class SpartRefineTilesOpt(ctypes.Structure):
    _fields_ = [("fit", SpartRefineOpt), ("n_shared", ctypes.c_int32), ("band_model", ctypes.c_int32),
                ("shared_prior_per_tile", ctypes.c_int32), ("shared_prior_mean", vp), ("shared_prior_weight", vp)]


class SpartRefineSeriesOpt(ctypes.Structure):
    _fields_ = [("tiles", SpartRefineTilesOpt), ("smooth", c_dp), ("link", vp)]        # smooth: HOST (Fl,); link: device (M,) or NULL


class SpartTilesOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("shared", "shared_std", "local", "local_std", "cost", "cost0", "n_accept", "pixel_cost", "status",
                                  "y")]


class SpartPosteriorOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("x", "y", "jac", "cov", "ak", "std", "dfs", "cost", "nband", "status")]


class SpartLutBayesOpt(ctypes.Structure):
    _fields_ = [("cut", ctypes.c_double), ("temperature", ctypes.c_double), ("brute_force", ctypes.c_int32)]


class SpartLutBayesOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("mean", "std", "sum_w", "ess", "count", "best_idx", "best_cost")]


class SpartLutBayesQOpt(ctypes.Structure):
    _fields_ = [("base", SpartLutBayesOpt), ("nq", ctypes.c_int32), ("levels", c_dp)]      # levels: HOST (nq,)


class SpartLutBayesQOut(ctypes.Structure):
    _fields_ = [("base", SpartLutBayesOut), ("quant", vp)]


class SpartProductsOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("fapar_bs", "fapar_ws", "albedo_bs", "albedo_ws", "fcover")]


class SpartSobolOpt(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("column", "band_model", "fast_prelude", "nlayers")]


class SpartSobolOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("mean", "var", "S1", "ST", "S1_se", "ST_se")]


class SpartVjpOpt(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("band_model", "fast_prelude", "nlayers")] + [("rel_step", ctypes.c_double)]


class SpartLeafFitOpt(ctypes.Structure):
    _fields_ = [("n_iter", ctypes.c_int32), ("weights_per_obs", ctypes.c_int32), ("rel_step", ctypes.c_double),
                ("lambda0", ctypes.c_double), ("prior_per_obs", ctypes.c_int32), ("prior_mean", vp), ("prior_weight", vp)]


class SpartLeafFitOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("x", "cost", "cost0", "std", "n_accept", "y_refl", "y_tran")]


class SpartSampleOpt(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("column", "band_model", "fast_prelude", "nlayers", "weights_per_obs", "prior_per_obs")] + [
        ("prior_mean", vp), ("prior_weight", vp), ("W", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_steps", ctypes.c_int64),
        ("burn", ctypes.c_int64), ("thin", ctypes.c_int64), ("a", ctypes.c_double), ("temperature", ctypes.c_double),
        ("rel_init", ctypes.c_double), ("init_radius", vp), ("init", vp), ("step0", ctypes.c_int64), ("obs_offset", ctypes.c_int64),
        ("seed", ctypes.c_uint64)]


class SpartSampleOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("mean", "cov", "std", "best_x", "best_cost", "n_accept", "status", "chain", "chain_cost", "last",
                                  "last_cost")]


PRODUCT_NAMES = ("fAPAR_bs", "fAPAR_ws", "albedo_bs", "albedo_ws", "fCover")      # spart_products_out, in its order
PRODUCTS_NREAD = 22                                 # spart_products reads params[0 ... 21]
LUT_BAYES_OUTS = tuple(n for n, _ in SpartLutBayesOut._fields_)      # spart_lut_bayes_out, in its order
LUT_BAYES_MAXP = 64
LUT_BAYES_MAXQ = 8                                  # spart_lut_bayes_q_opt.nq
POSTERIOR_OUTS = tuple(n for n, _ in SpartPosteriorOut._fields_)     # spart_posterior_out, in its order
REFINE_COLUMNS = ("R_TOC", "R_TOA", "L_TOA")       # spart_refine_opt.column
REFINE_MAXF, REFINE_MAX_ITER = 16, 100
REFINE_MAXV = 64                                    # spart_refine_views_opt.V
MIX_MAXV = 8                                        # spart_refine_mix_opt.V
MIX_OUTS = tuple(n for n, _ in SpartRefineMixOut._fields_)           # spart_refine_mix_out, in its order
TILES_OUTS = tuple(n for n, _ in SpartTilesOut._fields_)             # spart_tiles_out, in its order
TILES_MAXG = 4096                                   # pixels per tile of spart_refine_tiles
SERIES_MAXT = 256                                   # rows per series of spart_refine_series
SOBOL_OUTS = tuple(n for n, _ in SpartSobolOut._fields_)             # spart_sobol_out, in its order
SOBOL_BLOCK, SOBOL_MIN_N, SOBOL_MAX_N = 64, 128, 1 << 20             # spart_sobol: N a multiple of 64 in 128 ... 2^20
VJP_MAX_REL_STEP = 0.5                              # spart_vjp_opt.rel_step
LEAF_NPAR, LEAF_MAXF = 9, 9                          # spart_refine_leaf: leaf[9], 1 <= F <= 9
LEAF_FIT_OUTS = tuple(n for n, _ in SpartLeafFitOut._fields_)        # spart_leaf_fit_out, in its order
SAMPLE_OUTS = tuple(n for n, _ in SpartSampleOut._fields_)           # spart_sample_out, in its order
SAMPLE_WALKERS, SAMPLE_MAX_STEPS = (8, 16, 32, 64), 1 << 20          # spart_sample_opt.W (and W >= 2 F), n_steps

# the LUT searches: (dtype, B, nb, M) of every call; the three top-k searches share one argument list per function
c_i64p = ctypes.POINTER(ctypes.c_int64)
_LUT_SIZES = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
_LUT_TOPK_CALL = [vp] + _LUT_SIZES[:3] + [vp, ctypes.c_int64, vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]
_LUT_TOPK_STATS = [vp] + _LUT_SIZES + [ctypes.c_int, vp, c_i64p, c_i64p, c_i64p, c_dp]

# spart_refine and spart_refine_srf: one argument list
_REFINE_CALL = [vp, ctypes.c_int64, ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), c_dp, c_dp,
                vp, vp, ctypes.POINTER(SpartRefineOpt), vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]

# name -> (restype, argtypes): every symbol include/spart_hip.h declares
SIGNATURES = {
    "spart_ctx_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(SpartTables)]),
    "spart_ctx_destroy": (ctypes.c_int, [vp]),
    "spart_last_error": (ctypes.c_char_p, [vp]),
    "spart_build_id": (ctypes.c_char_p, []),
    "spart_abi_version": (ctypes.c_int, []),
    "spart_ctx_nb": (ctypes.c_int, [vp]),
    "spart_ctx_econv": (ctypes.c_int, [vp, c_dp]),
    "spart_ctx_set_row_pitch": (ctypes.c_int, [vp, ctypes.c_int64, ctypes.c_int64]),
    "spart_calculate_tav": (ctypes.c_int, [ctypes.c_double, c_dp, ctypes.c_int64, c_dp]),
    "spart_srf_support": (ctypes.c_int, [c_dp, c_dp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_int32), c_dp, c_dp]),
    "spart_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int, ctypes.c_int64]),
    "spart_workspace_bandsum": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t),
                                               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]),
    "spart_prospect_batch": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(vp), vp, vp, vp, vp,
                                            ctypes.c_size_t, vp]),
    "spart_bsm_batch": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(vp), vp, vp, vp, vp,
                                       ctypes.c_size_t, vp]),
    "spart_lidf_batch": (ctypes.c_int, [vp, ctypes.c_int64, vp, vp, vp, vp]),
    "spart_sailh_batch": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int64, vp, vp, vp, ctypes.POINTER(vp),
                                         ctypes.POINTER(vp), vp, ctypes.c_int32, ctypes.POINTER(vp), vp, ctypes.c_size_t, vp]),
    "spart_smac_batch": (ctypes.c_int, [vp, ctypes.c_int64, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                        vp, ctypes.c_size_t, vp]),
    "spart_run_batch": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(vp), vp, vp, vp, vp, vp,
                                       ctypes.POINTER(SpartMaterialize), vp, ctypes.c_size_t, vp]),
    "spart_lut_workspace_bytes": (ctypes.c_size_t, _LUT_SIZES),
    "spart_lut_nearest": (ctypes.c_int, [vp] + _LUT_SIZES[:3] + [vp, ctypes.c_int64, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]),
    "spart_lut_stats": (ctypes.c_int, [vp] + _LUT_SIZES + [vp, c_i64p, c_dp]),
    **{name + suffix: sig for name in ("spart_lut_topk", "spart_lut_topk_wide", "spart_lut_topk_obs_weights")
       for suffix, sig in (("_workspace_bytes", (ctypes.c_size_t, _LUT_SIZES + [ctypes.c_int])),
                           ("", (ctypes.c_int, _LUT_TOPK_CALL)),
                           ("_stats", (ctypes.c_int, _LUT_TOPK_STATS)))},
    "spart_lut_summarise": (ctypes.c_int, [vp, ctypes.c_int64, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_int, vp, vp, vp, vp, vp, vp]),
    "spart_lut_bayes_workspace_bytes": (ctypes.c_size_t, _LUT_SIZES),
    "spart_lut_bayes": (ctypes.c_int, [vp] + _LUT_SIZES[:3] + [vp, ctypes.c_int, vp, ctypes.c_int64, vp, vp,
                                                              ctypes.POINTER(SpartLutBayesOpt), ctypes.POINTER(SpartLutBayesOut),
                                                              vp, ctypes.c_size_t, vp]),
    "spart_lut_bayes_stats": (ctypes.c_int, [vp] + _LUT_SIZES + [vp, c_i64p, c_i64p, c_i64p, c_dp]),
    "spart_lut_bayes_quantiles": (ctypes.c_int, [vp] + _LUT_SIZES[:3] + [vp, ctypes.c_int, vp, ctypes.c_int64, vp, vp,
                                                                        ctypes.POINTER(SpartLutBayesQOpt),
                                                                        ctypes.POINTER(SpartLutBayesQOut), vp, ctypes.c_size_t, vp]),
    "spart_refine_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int]),
    "spart_refine": (ctypes.c_int, _REFINE_CALL),
    "spart_refine_srf": (ctypes.c_int, _REFINE_CALL),
    "spart_views_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "spart_refine_views": (ctypes.c_int, _REFINE_CALL[:9] + [ctypes.POINTER(SpartRefineViewsOpt)] + _REFINE_CALL[10:]),
    "spart_mix_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "spart_refine_mix": (ctypes.c_int, _REFINE_CALL[:9] + [vp, ctypes.POINTER(SpartRefineMixOpt), ctypes.POINTER(SpartRefineMixOut)] +
                         _REFINE_CALL[16:]),
    "spart_tiles_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "spart_refine_tiles": (ctypes.c_int, _REFINE_CALL[:7] + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)] + _REFINE_CALL[7:9] +
                           [ctypes.POINTER(SpartRefineTilesOpt), ctypes.POINTER(SpartTilesOut)] + _REFINE_CALL[16:]),
    "spart_series_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "spart_refine_series": (ctypes.c_int, _REFINE_CALL[:7] + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)] + _REFINE_CALL[7:9] +
                            [ctypes.POINTER(SpartRefineSeriesOpt), ctypes.POINTER(SpartTilesOut)] + _REFINE_CALL[16:]),
    "spart_refine_posterior": (ctypes.c_int, _REFINE_CALL[:10] + [ctypes.c_int, ctypes.POINTER(SpartPosteriorOut)] + _REFINE_CALL[16:]),
    "spart_products": (ctypes.c_int, [vp, ctypes.c_int64, ctypes.POINTER(vp), ctypes.POINTER(SpartProductsOut), vp, ctypes.c_size_t, vp]),
    "spart_sobol_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "spart_sobol": (ctypes.c_int, _REFINE_CALL[:7] + [ctypes.c_int64, vp, vp, ctypes.POINTER(SpartSobolOpt),
                                                     ctypes.POINTER(SpartSobolOut)] + _REFINE_CALL[16:]),
    "spart_sample_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "spart_sample": (ctypes.c_int, _REFINE_CALL[:9] + [ctypes.POINTER(SpartSampleOpt), ctypes.POINTER(SpartSampleOut)] + _REFINE_CALL[16:]),
    "spart_vjp_workspace_bytes": (ctypes.c_size_t, [vp, ctypes.c_int64, ctypes.c_int]),
    "spart_vjp": (ctypes.c_int, _REFINE_CALL[:7] + [ctypes.POINTER(vp), ctypes.POINTER(SpartVjpOpt), vp] + _REFINE_CALL[16:]),
    "spart_refine_leaf": (ctypes.c_int, [vp, ctypes.c_int64, ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), c_dp, c_dp,
                                         vp, vp, vp, vp, ctypes.POINTER(SpartLeafFitOpt), ctypes.POINTER(SpartLeafFitOut), vp]),
    "spart_profile_enable": (ctypes.c_int, [vp, ctypes.c_int]),
    "spart_profile_read": (ctypes.c_int, [vp, c_dp, ctypes.POINTER(ctypes.c_int)]),
    "spart_profile_read_stages": (ctypes.c_int, [vp, c_dp, ctypes.POINTER(ctypes.c_int)]),
}
STAGES = ("prelude", "bands", "columns")        # spart_profile_read_stages

_libs = {}


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_spart_build", os.path.join(HERE, "..", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def expected_build_id():
    """id of the sources next to this package (build.py: source_id) -- what the in-tree library must report"""
    return _build_module().source_id(os.environ.get("SPART_FAST_MATH", "1") == "1")


def build_id(lib=None):
    """spart_build_id() of the loaded library"""
    return (lib or load()).spart_build_id().decode()


def load(path=None):
    """dlopen the library (torch is imported first so that its HIP runtime, soname
    libamdhip64.so.7, is the one both sides use).  ``path`` selects another build of the same
    ABI (tools/ab_bench.py compares kernel variants in one process).  The in-tree library must have been built from
    the sources next to it (content hash embedded at build time): a stale one is rebuilt when hipcc is there, and
    refused otherwise -- never loaded silently."""
    path = os.path.abspath(path or os.environ.get("SPART_HIP_LIB") or LIB_PATH)
    if path in _libs:
        return _libs[path]
    import torch  # noqa: F401

    in_tree = path == os.path.abspath(LIB_PATH)
    want = None
    if in_tree:
        try:
            b = _build_module()
            want = expected_build_id()
        except OSError:
            # a deployment that ships the prebuilt library without csrc/: nothing to compare the binary with
            b, want = None, None
            if not os.path.exists(path):
                raise RuntimeError(f"{path} is missing and the kernel sources to build it from are not installed. "
                                   "spart_amd has no CPU fallback.") from None
        have = b.binary_id(path) if b is not None else None
        if want is not None and have != want:
            # the .so is a build artefact (git-ignored): compile it when it is missing or stale and hipcc is around.  Several
            # ranks may get here at once: one compiles (file lock), the others wait and find the library current.
            try:
                import fcntl
                with open(path + ".lock", "w") as lock:
                    fcntl.flock(lock, fcntl.LOCK_EX)
                    try:
                        if b.binary_id(path) != want:
                            b.build(verbose=True)
                    finally:
                        fcntl.flock(lock, fcntl.LOCK_UN)
            except Exception as e:      # noqa: BLE001
                if os.path.exists(path):
                    raise RuntimeError(f"{path} was built from other sources (build id {have}, sources {want}) and could "
                                       f"not be rebuilt ({e}); run `python spart-python_amd/build.py`") from e
                raise RuntimeError(f"{path} is missing and could not be built ({e}); run `python spart-python_amd/build.py` "
                                   "(hipcc, gfx950). spart_amd has no CPU fallback.") from e
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python spart-python_amd/build.py` "
            "(hipcc, gfx950). spart_amd has no CPU fallback.")
    lib = ctypes.CDLL(path)
    # the interface version first: a library built from another round's header (SPART_HIP_LIB=, lib_path=) would otherwise be
    # called with shifted arguments / a shorter spart_materialize
    try:
        lib.spart_abi_version.restype = ctypes.c_int
        have_abi = int(lib.spart_abi_version())
    except AttributeError:
        have_abi = None
    if have_abi != ABI_VERSION:
        raise RuntimeError(f"{path} implements interface version {have_abi if have_abi is not None else '< 6 (no spart_abi_version)'}"
                           f", this binding needs {ABI_VERSION} (include/spart_hip.h: SPART_ABI_VERSION); rebuild it with "
                           "`python spart-python_amd/build.py`")
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # symbols can be added without a new interface version (include/spart_hip.h: spart_refine_srf), so the number
            # alone does not say that a foreign library has them all
            raise RuntimeError(f"{path} implements interface version {have_abi} but does not export {name}, which this binding "
                               "needs (include/spart_hip.h); rebuild it with `python spart-python_amd/build.py`") from None
        fn.restype = res
        fn.argtypes = args
    if in_tree and want is not None and lib.spart_build_id().decode() != want:      # (what the loaded code says, not what the file's bytes said)
        raise RuntimeError(f"{path} reports build id {lib.spart_build_id().decode()}, the sources next to it are {want}")
    _libs[path] = lib
    return lib


def check(lib, ctx, rc):
    if rc != 0:
        msg = lib.spart_last_error(ctx)
        raise RuntimeError(f"libspart_hip error {rc}: {msg.decode() if msg else '?'}")
