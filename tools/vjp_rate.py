"""Rate of the backward pass (spart_vjp) against what it is made of and against what a user had before it.

    python tools/vjp_rate.py [--reps 20] [--out profiles/vjp_rate.txt] [--timeout 300]

Workload: Sentinel-2A (nb = 13), M = 262 144 observations, F = 6 free parameters, one column (R_TOC), float64, everything already
on the device.  Three steps, each in a fresh child process under a time limit of its own, device events, medians after two
warm-up calls:
  vjp       Engine.vjp: 2 F M forward rows in chunks of 2^19 and the ordered sums;
  forward   ONE Engine.run(float64, prune=True) of a table of the same 2 F M rows: what the call cannot go below;
  jacobian  the path of a user without the call: Engine.jacobian ((F + 1) M rows, one-sided, an (M, nb, F) Jacobian stored)
            followed by torch.einsum("mj,mjf->mf", g, jac).
Then the two ratios vjp / forward and jacobian / vjp.  Every figure in the report is measured in this run.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from refine_rate import SENSOR, event_ms, stats  # noqa: E402

FREE = ["LAI", "Cab", "Cw", "Cdm", "N", "B"]
M = 262144
STEPS = ("vjp", "forward", "jacobian")


def child(a):
    """one step -> a JSON line {step, ms: [...], note}"""
    import torch
    from spart_amd import get_engine, workloads
    eng = get_engine(SENSOR, 0)
    F = len(FREE)
    base = workloads.lhs_params(M, "full", seed=77)
    P = torch.as_tensor(np.ascontiguousarray(base.T), device=eng.device)
    g = torch.randn(M, eng.nb, dtype=torch.float64, device=eng.device, generator=torch.Generator(eng.device).manual_seed(1))
    note = ""
    if a.child == "vjp":
        kept = {}
        ts = event_ms(torch, lambda: kept.update(eng.vjp(P, {"R_TOC": g}, FREE)), a.reps)
        grad = kept["grad"]
        jac = eng.jacobian(P, FREE)["jac"]
        other = torch.einsum("mj,mjf->mf", g, jac)
        fine = torch.isfinite(grad).all(dim=1) & torch.isfinite(other).all(dim=1)
        rel = ((grad - other).abs() / grad.abs().clamp_min(1e-300))[fine]
        note = (f"workspace {int(eng.lib.spart_vjp_workspace_bytes(eng.ctx, M, F)) / 2 ** 20:.1f} MiB; {int(fine.sum())} of {M} rows finite; "
                f"median |central - one-sided| / |central| over them {rel.median().item():.2e}")
    elif a.child == "forward":
        import vjp_defined as vd
        cols = [workloads.PARAM_NAMES.index(n) for n in FREE]
        lo, hi = (np.array([workloads.RANGES[n][i] for n in FREE], dtype=np.float64) for i in (0, 1))
        x = vd.clip_defined(base[:, cols], lo, hi)
        rows = vd.rows_defined(base, cols, x, *vd.steps_defined(x, lo, hi)).reshape(2 * F * M, 27)
        table = torch.as_tensor(np.ascontiguousarray(rows.T), device=eng.device)
        ts = event_ms(torch, lambda: eng.run(table, "float64", prune=True), a.reps)
        note = f"{table.shape[1]} rows in one call"
    else:
        ts = event_ms(torch, lambda: torch.einsum("mj,mjf->mf", g, eng.jacobian(P, FREE)["jac"]), a.reps)
        note = f"the stored Jacobian is {M * eng.nb * F * 8 / 1e6:.0f} MB"
    torch.cuda.synchronize()
    print(json.dumps({"step": a.child, "ms": ts, "note": note}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds one step may take")
    ap.add_argument("--child", default=None, choices=STEPS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"spart_vjp on MI355X (one GCD), tools/vjp_rate.py: {SENSOR}, nb = 13, M = {M}, F = {len(FREE)} free parameters {FREE}, one "
        f"column (R_TOC), float64; device events, medians of {a.reps} after 2 warm-up calls, each step in a process of its own.")
    med = {}
    for step in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps)], capture_output=True,
                               text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            say(f"  {step:9s} (killed after {a.timeout} s)")
            break                                           # nothing more is started after a step that did not end
        if r.returncode != 0:
            say(f"  {step:9s} (failed: exit status {r.returncode}) {r.stderr[-400:]}")
            break
        res = json.loads(r.stdout.strip().splitlines()[-1])
        med[step] = float(np.median(res["ms"]))
        say(f"  {step:9s} {stats(res['ms'])}  {res['note']}")
    if len(med) == len(STEPS):
        say(f"  vjp / forward = {med['vjp'] / med['forward']:.3f}  (the call's own part: {med['vjp'] - med['forward']:.3f} ms)")
        say(f"  jacobian + einsum / vjp = {med['jacobian'] / med['vjp']:.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(med) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
