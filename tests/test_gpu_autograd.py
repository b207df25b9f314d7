"""spart_amd.SpartLayer on the GPU: forward and backward against Engine.run and Engine.vjp bit for bit (float64) and rounded
once (float32), the chain rule through from_unit, the number of spart_vjp calls a backward pass makes, repeated and double
backward, a descent step that must lower the cost of every pixel, and the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, torch_mod  # noqa: F401 (fixture)
from helpers.vjp_calls import S2, bounds_of, cols_of

pytestmark = pytest.mark.gpu
NAMES = ["LAI", "Cab", "Cw"]


def bits(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def setup(torch_mod):
    """M = 9 LHS rows; x is their free columns with row 0 pushed above hi and row 1 below lo -> (layer of two columns, eng, base
    (27, M) device tensor, x (M, 3) float64 device tensor, clamped x)"""
    import spart_amd
    from spart_amd import workloads
    layer = spart_amd.SpartLayer(S2, NAMES, columns=("R_TOC", "L_TOA"))
    eng = layer.engine
    base = torch_mod.as_tensor(workloads.lhs_params(9, "full", seed=21).T.copy(), device=eng.device)
    lo, hi = (torch_mod.as_tensor(v, device=eng.device) for v in bounds_of(NAMES))
    x = base[cols_of(NAMES)].T.clone()
    x[0] = hi + 0.25 * (hi - lo)
    x[1] = lo - 1.0
    return layer, eng, base, x, torch_mod.minimum(torch_mod.maximum(x, lo), hi)


def run_at(torch, eng, base, xc, **kw):
    table = base.clone()
    table[cols_of(NAMES)] = xc.T
    return eng.run(table, "float64", prune=True, **kw), table


def test_float64_forward_and_backward_are_run_and_vjp(torch_mod, setup):
    layer, eng, base, x, xc = setup
    x = x.clone().requires_grad_(True)
    poison = base.clone()
    poison[cols_of(NAMES)] = float("nan")                                    # the free rows of base are ignored
    out = layer(x, poison)
    want, table = run_at(torch_mod, eng, base, xc)
    assert set(out) == {"R_TOC", "L_TOA"} and all(out[k].dtype == torch_mod.float64 and bits(out[k], want[k]) for k in out)
    g = {k: torch_mod.randn_like(out[k]) for k in out}
    loss = sum((out[k] * g[k]).sum() for k in out)
    loss.backward()
    ref = eng.vjp(table, g, NAMES)["grad"]
    assert x.grad.dtype == torch_mod.float64 and bits(x.grad, ref) and bool(torch_mod.isfinite(ref).all()) and bool((ref != 0).all())
    # a list of rows with None in the free places is the same base
    rows = [None if i in cols_of(NAMES) else base[i] for i in range(27)]
    again = layer(x.detach(), rows)
    assert all(bits(again[k], want[k]) for k in again)
    with pytest.raises(ValueError, match="not free"):
        layer(x.detach(), [None] * 27)
    with pytest.raises(ValueError, match="expected \\(M, 3\\)"):
        layer(x.detach()[:, :2], base)


def test_float32_is_the_float64_result_rounded_once(torch_mod, setup):
    layer, eng, base, x, xc = setup
    x32 = x.float().requires_grad_(True)
    out = layer(x32, base)
    xc32 = torch_mod.minimum(torch_mod.maximum(x32.detach().double(), layer.lo.to(eng.device)), layer.hi.to(eng.device))
    want, table = run_at(torch_mod, eng, base, xc32)
    assert all(out[k].dtype == torch_mod.float32 and bits(out[k], want[k].float()) for k in out)
    g = {k: torch_mod.randn_like(out[k]) for k in out}
    sum((out[k] * g[k]).sum() for k in out).backward()
    ref = eng.vjp(table, {k: v.double() for k, v in g.items()}, NAMES)["grad"]
    assert x32.grad.dtype == torch_mod.float32 and bits(x32.grad, ref.float())


def test_the_chain_rule_through_from_unit(torch_mod, setup):
    layer, eng, base, x, xc = setup
    u = torch_mod.rand(9, 3, dtype=torch_mod.float64, device=eng.device).requires_grad_(True)
    xu = layer.from_unit(u)
    xu.retain_grad()
    out = layer(xu, base)
    (out["R_TOC"].sum() + 0.01 * out["L_TOA"].sum()).backward()
    want = xu.grad * (layer.hi - layer.lo).to(eng.device)
    err = ((u.grad - want).abs() / want.abs()).max().item()
    print(f"from_unit chain rule: worst relative difference {err:.3e} (4 eps = {4 * 2.0 ** -52:.3e})")
    assert bool((want != 0).all()) and err <= 4 * 2.0 ** -52


def test_one_vjp_call_per_backward_and_none_without_grad(torch_mod, setup):
    layer, eng, base, x, xc = setup
    n0 = eng.calls["spart_vjp"]
    with torch_mod.no_grad():
        out = layer(x.clone().requires_grad_(True), base)
    assert not out["R_TOC"].requires_grad
    out = layer(x, base)
    assert not x.requires_grad and not out["R_TOC"].requires_grad and eng.calls["spart_vjp"] == n0
    xg = x.clone().requires_grad_(True)
    out = layer(xg, base)
    assert eng.calls["spart_vjp"] == n0                                      # (forward makes none)
    (out["R_TOC"].sum() + out["L_TOA"].mean()).backward()
    assert eng.calls["spart_vjp"] == n0 + 1                                  # two columns, one call
    both = xg.grad.clone()
    xg.grad = None
    layer(xg, base)["L_TOA"].mean().backward()                               # R_TOC's gradient is None: NULL for it
    assert eng.calls["spart_vjp"] == n0 + 2
    nb = eng.nb
    ref = eng.vjp(run_at(torch_mod, eng, base, xc)[1], {"L_TOA": torch_mod.full((9, nb), 1.0 / (9 * nb), dtype=torch_mod.float64)}, NAMES)["grad"]
    assert bits(xg.grad, ref) and not bits(xg.grad, both)


def test_repeated_backward_gives_the_same_bits_and_double_backward_raises(torch_mod, setup):
    import spart_amd
    layer, eng, base, x, xc = setup
    single = spart_amd.SpartLayer(S2, NAMES, columns="R_TOA", band_model="srf", lidf="newton", nlayers=30, rel_step=0.01)
    xg = x.clone().requires_grad_(True)
    y = single(xg, base)
    want = run_at(torch_mod, eng, base, xc, lidf="newton", nlayers=30, materialize=["R_TOA_srf"])[0]["R_TOA_srf"]
    assert torch_mod.is_tensor(y) and bits(y, want)                          # one column: the tensor itself
    loss = (y ** 2).sum()
    loss.backward(retain_graph=True)
    first = xg.grad.clone()
    xg.grad = None
    loss.backward()
    assert bits(xg.grad, first) and bool((first != 0).all())
    ref = single.engine.vjp(run_at(torch_mod, eng, base, xc)[1], {"R_TOA": 2.0 * want}, NAMES, rel_step=0.01, lidf="newton", nlayers=30,
                            band_model="srf")["grad"]
    assert bits(first, ref)
    xg.grad = None
    y = single(xg, base)
    grad, = torch_mod.autograd.grad(y.sum(), xg, create_graph=True)
    assert not grad.requires_grad                                            # once_differentiable: the gradient has no graph of its own
    with pytest.raises(RuntimeError):
        grad.sum().backward()


def test_one_step_along_the_negative_gradient_lowers_every_pixels_cost(torch_mod):
    """Sentinel-2A, M = 32, F = 2 (LAI, Cab): observations from the model at known parameters, starts at interior LHS rows that
    differ from the truth; one step along -grad with step halving (at most 20 halvings) must strictly lower sum (y - obs)^2 of
    EVERY pixel.  A sign error, an f-permutation or a wrong denominator fails this."""
    import spart_amd
    from spart_amd import workloads
    names = ["LAI", "Cab"]
    free, (lo, hi) = cols_of(names), bounds_of(names)
    M = 32
    truth = workloads.lhs_params(M, "full", seed=31)
    start = workloads.lhs_params(M, "full", seed=32)[:, free]
    rng = (hi - lo)
    inside = ((start > lo + 0.05 * rng) & (start < hi - 0.05 * rng)).all(axis=1)
    start[~inside] = (lo + 0.5 * rng)
    near = (np.abs(start - truth[:, free]) < 0.1 * rng).any(axis=1)              # chosen on the CPU to differ from the truth
    start[near] = np.where(truth[near][:, free] > lo + 0.5 * rng, lo + 0.25 * rng, lo + 0.75 * rng)
    assert (np.abs(start - truth[:, free]) >= 0.1 * rng).all() and ((start > lo) & (start < hi)).all()
    layer = spart_amd.SpartLayer(S2, names)
    dev = layer.engine.device
    base = torch_mod.as_tensor(truth.T.copy(), device=dev)
    obs = layer(torch_mod.as_tensor(truth[:, free].copy(), device=dev), base)
    assert bool(torch_mod.isfinite(obs).all())
    x = torch_mod.as_tensor(start, device=dev).requires_grad_(True)
    cost = lambda xx: ((layer(xx, base) - obs) ** 2).sum(dim=1)                 # noqa: E731
    c0 = cost(x)
    c0.sum().backward()
    g = x.grad
    assert bool((c0 > 0).all()) and bool(torch_mod.isfinite(g).all()) and bool((g != 0).any(dim=1).all())
    # the first step moves the parameter that moves most by a quarter of its range
    step = 0.25 / (g.abs() / torch_mod.as_tensor(rng, device=dev)).max(dim=1, keepdim=True).values
    done = torch_mod.zeros(M, dtype=torch_mod.bool, device=dev)
    with torch_mod.no_grad():
        for halving in range(21):
            c1 = cost(x - step * g)
            done |= c1 < c0
            if bool(done.all()):
                break
            step = torch_mod.where(done[:, None], step, step * 0.5)
    print(f"descent: every pixel lower after {halving} halvings; cost {c0.sum().item():.4e} -> {c1.sum().item():.4e}")
    assert bool(done.all()), (c0[~done], c1[~done])


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "autograd.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    first, last = (float(re.search(rf"{k} loss ([0-9.e+-]+)", r.stdout).group(1)) for k in ("first", "last"))
    print(r.stdout)
    assert last < first and "30 spart_vjp calls" in r.stdout
