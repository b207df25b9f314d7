"""The forward model as a differentiable torch layer: SpartLayer runs the float64 pruned column path forward and ONE spart_vjp
call backward (include/spart_hip.h: spart_vjp; Engine.vjp), so that SPART can end a network -- a physics decoder behind an
encoder -- or sit under torch.optim with a loss of the caller's."""
import torch

from . import _lib, workloads
from .engine import Engine, _band_model, get_engine, refine_plan, vjp_columns, vjp_rel_step


class _SpartFunction(torch.autograd.Function):
    """(x, table, layer) -> one (M, nb) tensor per column of the layer, in x's dtype.  ``table`` (27, M) float64 already holds
    the clamped x in its free rows; the gradient goes to x alone."""

    @staticmethod
    def forward(ctx, x, table, layer):
        ctx.set_materialize_grads(False)
        ctx.layer = layer
        ctx.save_for_backward(table)
        return tuple(y.to(x.dtype) for y in layer._run(table))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        layer = ctx.layer
        given = {c: g.to(torch.float64) for c, g in zip(layer.columns, grads) if g is not None}
        if not given:
            return None, None, None
        table, = ctx.saved_tensors
        res = layer.engine.vjp(table, given, layer.names, bounds=layer.bounds, rel_step=layer.rel_step, lidf=layer.lidf,
                               nlayers=layer.nlayers, band_model=layer.band_model)
        return res["grad"].to(next(g.dtype for g in grads if g is not None)), None, None      # (the outputs' dtype is x's)


class SpartLayer(torch.nn.Module):
    """SPART's sensor columns as a function of ``free`` parameters, with a gradient.

    sensor / sensor_info, device : as for spart_amd.get_engine (the engine is made at the first forward call)
    free, bounds : as for refine(): 1 ... 16 names from workloads.PARAM_NAMES and {name: (lo, hi)}, workloads.RANGES otherwise
    columns : names from R_TOC / R_TOA / L_TOA; one column returns its (M, nb) tensor, several a dict by name
    rel_step : the central-difference step of the backward pass, rel_step (hi - lo) to either side, cut at the bounds
    lidf, nlayers, band_model : as for refine(); "srf" returns the SRF-convolved column and takes one column

    forward(x, base): x (M, F) in physical units, float32 or float64; base the fixed parameters, a (27, M) tensor or a list of
    27 entries of 1 or M values whose free entries are ignored (and may be None).  x is clamped to the bounds, the columns are
    the float64 ones rounded once to x's dtype.  Backward is ONE spart_vjp call whatever the number of columns; the gradient
    goes to x only, straight through the clamp (a parameter outside its bounds gets the one-sided slope at the bound).  Second
    derivatives are not defined: a double backward raises."""

    def __init__(self, sensor, free, bounds=None, columns=("R_TOC",), rel_step=1e-3, lidf="literal", nlayers=None, band_model="centre",
                 device=None, sensor_info=None):
        super().__init__()
        plan = refine_plan(free, bounds, 0, "R_TOC", 1e-3, 1e-2)
        self.columns = vjp_columns(columns, band_model)
        self.single = isinstance(columns, str) or len(self.columns) == 1
        self.rel_step = vjp_rel_step(rel_step)
        if lidf not in ("literal", "newton"):
            raise ValueError("lidf must be 'literal' or 'newton'")
        Engine._nlayers(nlayers)
        self.names, self.bounds = list(plan["names"]), dict(bounds or {})
        self.free_cols = [int(c) for c in plan["cols"]]
        self.register_buffer("lo", torch.as_tensor(plan["lo"].copy()), persistent=False)
        self.register_buffer("hi", torch.as_tensor(plan["hi"].copy()), persistent=False)
        self.sensor, self.sensor_info, self.device = sensor, sensor_info, device
        self.lidf, self.nlayers, self.band_model = lidf, nlayers, band_model
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            eng = get_engine(self.sensor, self.device, sensor_info=self.sensor_info)
            _band_model(self.band_model, eng)
            self._engine = eng
        return self._engine

    def from_unit(self, u):
        """[0, 1] -> physical units, lo + u (hi - lo) per free parameter, in plain torch (for a sigmoid-headed encoder)"""
        lo, hi = (b.to(device=u.device, dtype=u.dtype) for b in (self.lo, self.hi))
        return lo + u * (hi - lo)

    def _run(self, table):
        """the layer's columns of a (27, M) float64 device table, float64, in the order of self.columns"""
        srf = self.band_model == "srf"
        keys = [c + "_srf" if srf else c for c in self.columns]
        res = self.engine.run(table, "float64", prune=True, lidf=self.lidf, nlayers=self.nlayers, **({"materialize": keys} if srf else {}))
        return [res[k] for k in keys]

    def _table(self, x, base):
        eng, F = self.engine, len(self.names)
        if x.dim() != 2 or x.shape[1] != F:
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (M, {F})")
        if x.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"x is {x.dtype}, expected float32 or float64")
        M = int(x.shape[0])
        if torch.is_tensor(base):
            if base.dim() != 2 or base.shape[0] != _lib.NPARAM or base.shape[1] not in (1, M):
                raise ValueError(f"base has shape {tuple(base.shape)}, expected (27, {M})")
            table = base.detach().to(device=eng.device, dtype=torch.float64).expand(_lib.NPARAM, M).clone()
        else:
            if len(base) != _lib.NPARAM:
                raise ValueError(f"base must have {_lib.NPARAM} entries, got {len(base)}")
            rows = [0.0 if i in self.free_cols else (v.detach() if torch.is_tensor(v) else v) for i, v in enumerate(base)]
            missing = [workloads.PARAM_NAMES[i] for i, v in enumerate(rows) if v is None]
            if missing:
                raise ValueError(f"base: {missing} are None and not free")
            table = torch.stack(eng.columns(rows, M)[0])
        lo, hi = (b.to(device=eng.device, dtype=torch.float64) for b in (self.lo, self.hi))
        xc = x.detach().to(device=eng.device, dtype=torch.float64)
        xc = torch.where(xc < lo, lo, xc)                  # spart_refine's clip: a NaN stays a NaN
        xc = torch.where(xc > hi, hi, xc)
        table[self.free_cols] = xc.T
        return table

    def forward(self, x, base):
        table = self._table(x, base)
        if torch.is_grad_enabled() and x.requires_grad:
            ys = _SpartFunction.apply(x.to(table.device), table, self)
        else:
            ys = tuple(y.to(x.dtype) for y in self._run(table))
        ys = [y.to(x.device) for y in ys]
        return ys[0] if self.single else dict(zip(self.columns, ys))
