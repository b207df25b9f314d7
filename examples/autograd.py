"""SPART as the decoder of an auto-encoder: a small MLP reads a pixel's 13 Sentinel-2A reflectances and proposes LAI, Cab, Cw
and Cdm; spart_amd.SpartLayer turns them back into reflectances, and Adam trains the MLP on the reconstruction loss alone --
the gradient comes through the radiative-transfer model (one spart_vjp call per step).  Needs an MI355X.

    python examples/autograd.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import SpartLayer, workloads  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
free = ["LAI", "Cab", "Cw", "Cdm"]
torch.manual_seed(0)
layer = SpartLayer("Sentinel2A-MSI", free)
eng = layer.engine
dev = eng.device

# 256 synthetic pixels: the model at Latin-hypercube parameters
truth = torch.as_tensor(workloads.lhs_params(256, "full", seed=1).T.copy(), device=dev)
obs = eng.run(truth, "float64", prune=True)["R_TOC"].float()
assert bool(torch.isfinite(obs).all())

net =torch.nn.Sequential(torch.nn.Linear(eng.nb, 32), torch.nn.Tanh(), torch.nn.Linear(32, len(free)), torch.nn.Sigmoid()).to(dev)
adam = torch.optim.Adam(net.parameters(), lr=1e-2)
losses = []
for step in range(steps):
    adam.zero_grad()
    x = layer.from_unit(net(obs))                 # (256, 4) in physical units
    loss = ((layer(x, truth) - obs) ** 2).mean()  # the free rows of `truth` are ignored: the layer puts x there
    loss.backward()
    adam.step()
    losses.append(float(loss))
print(f"{steps} Adam steps on {obs.shape[0]} pixels, free = {free}, {eng.calls['spart_vjp']} spart_vjp calls")
print(f"first loss {losses[0]:.6e}")
print(f"last loss {losses[-1]:.6e}")
