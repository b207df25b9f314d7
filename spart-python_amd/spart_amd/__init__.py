"""spart_amd: MI355X-native batched SPART evaluator (HIP kernels behind libspart_hip.so).

Public names mirror wirrell/SPART-python's ``SPART`` package (src/SPART/__init__.py:1-5).
"""
from .api import (BSM, PROSPECT_5D, SAILH, SMAC, SPART, Angles, AtmosphericOptics, AtmosphericProperties,  # noqa: F401
                  BatchResult, CanopyReflectances, CanopyStructure, LeafBiology, LeafOptics, SoilOptics,
                  SoilParameters, SoilParametersFromFile, SpectralBands, calculate_ET_radiance,
                  calculate_leafangles, calculate_spectral_convolution, calculate_tav, soilwat, load_ET_parameters,
                  load_optical_parameters, load_sensor_info, set_leaf_refl_trans_assumptions,
                  set_soil_refl_trans_assumptions)
from .engine import PRODUCT_NAMES, Engine, get_engine, knn_prior  # noqa: F401
from .srf import align_srf, check_srf  # noqa: F401
from .tables import SENSORS  # noqa: F401
from . import workloads  # noqa: F401
from .lut import (date_links, generate_lut, invert_lut, jacobian, load_lut, lut_products, lut_to_parquet, noise_weights, posterior,  # noqa: F401
                  products, refine, refine_leaf, refine_mix, refine_series, refine_views, refine_tiles, retrieve, retrieve_stream, chain_summary, sample, sobol,
                  sobol_design,
                  tiles_from_labels, vjp, window_tiles)

__version__ = "0.1.0"


def __getattr__(name):
    # spart_amd.SpartLayer is a torch.nn.Module: torch is imported when it is first asked for, not with the package
    if name == "SpartLayer":
        from .autograd import SpartLayer
        return SpartLayer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
