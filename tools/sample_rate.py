"""Rate of the ensemble sampler (spart_sample) against the forward model it is built around: the same number of forward rows
through Engine.run (float64, pruned) in calls of the same size, already on the device, with nothing done to their output.

    python tools/sample_rate.py [--reps 5] [--out profiles/sample_rate.txt] [--no-trace]

Workload: Sentinel-2A (nb = 13), R_TOA, M = 16 384 observations, F = 4 free parameters (LAI, Cab, Cw, Cdm), W = 16 walkers,
n_steps = 200: 2 (n_steps + 1) = 402 forward calls of M W / 2 = 131 072 rows each.
  a  the whole call (Engine.sample) and 402 Engine.run calls of 131 072 rows, device events, medians after one warm-up call, and
     their ratio;
then, from a separate run of the call in a child process under `rocprofv3 --kernel-trace --stats` with no counters, the time of
every kernel per call and its share.  Every figure in the report is measured in this run.
"""
import argparse
import csv
import glob
import os
import signal
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from refine_rate import SENSOR, event_ms, stats  # noqa: E402

FREE = ["LAI", "Cab", "Cw", "Cdm"]
M, W, N_STEPS, COLUMN = 16384, 16, 200, "R_TOA"
NEW = ("k_sample_init", "k_sample_table", "k_sample_step")
FORWARD = ("k_prelude", "k_columns", "k_bands")


def workload(torch, eng):
    """truth from the benchmark's Latin hypercube, 2 % noise, the start at the truth -> (P (27, M) on the device, obs, weights)"""
    from spart_amd import workloads
    truth = workloads.lhs_params(M, "full", seed=77)
    P = torch.as_tensor(np.ascontiguousarray(truth.T), device=eng.device)
    clean = eng.run(P, "float64", prune=True)[COLUMN]
    clean = torch.where(torch.isfinite(clean), clean, torch.full_like(clean, 0.3))
    sigma = 0.02 * clean.clamp_min(0.01)
    g = torch.Generator(device=eng.device).manual_seed(1)
    obs = clean + sigma * torch.randn(clean.shape, generator=g, device=eng.device, dtype=torch.float64)
    return P, obs, 1.0 / sigma ** 2


def call(eng, P, obs, w):
    return eng.sample(P, obs, FREE, weights=w, walkers=W, n_steps=N_STEPS, column=COLUMN, seed=1)


def child(a):
    """the program rocprofv3 is pointed at: two calls"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    P, obs, w = workload(torch, eng)
    torch.cuda.synchronize()
    for _ in range(2):
        call(eng, P, obs, w)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=180, help="seconds one rocprofv3 run may take")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    from spart_amd import get_engine
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = get_engine(SENSOR, 0)
    F, rows, calls = len(FREE), M * W // 2, 2 * (N_STEPS + 1)
    say(f"spart_sample on MI355X (one GCD), tools/sample_rate.py: {SENSOR}, nb = {eng.nb}, {COLUMN}, M = {M}, F = {F} {FREE}, W = {W}, "
        f"n_steps = {N_STEPS}, float64; device events, medians of {a.reps} after 1 warm-up call.  forward: {calls} calls of "
        f"Engine.run(float64, prune=True) on {rows} rows already on the device -- the same {calls * rows} forward rows in calls of the "
        "same size, nothing done to their output.")
    say(f"workspace {int(eng.lib.spart_sample_workspace_bytes(eng.ctx, M, F, W)) / 2 ** 20:.1f} MiB")
    P, obs, w = workload(torch, eng)
    res = {}
    ts = event_ms(torch, lambda: res.update(call(eng, P, obs, w)), a.reps, warm=1)
    table = P.repeat_interleave(W // 2, dim=1).contiguous()

    def forward():
        for _ in range(calls):
            eng.run(table, "float64", prune=True)
    tf = event_ms(torch, forward, a.reps, warm=1)
    say(f"  a  spart_sample {stats(ts)}")
    say(f"     forward      {stats(tf)}")
    say(f"     spart_sample / forward = {np.median(ts) / np.median(tf):.3f}; the call's own part {np.median(ts) - np.median(tf):.3f} ms; "
        f"{calls * rows / np.median(ts) * 1e3:.3g} forward rows/s through the call")
    acc, status = res["accept_fraction"].cpu().numpy(), res["status"].cpu().numpy()
    say(f"     status 0 for {int((status == 0).sum())} of {M}; acceptance fraction median {np.nanmedian(acc):.3f} "
        f"(5 % {np.nanquantile(acc, 0.05):.3f}, 95 % {np.nanquantile(acc, 0.95):.3f})")
    ok = True
    if a.no_trace:
        say("  rocprofv3 --kernel-trace --stats: (not collected: --no-trace)")
    else:
        krows, note = kernel_rows(a)
        ok = not note
        total = sum(krows.values())
        say(f"  rocprofv3 --kernel-trace --stats (a separate run, 2 calls in a fresh process; ms of ONE call): {note}")
        for k, ms in sorted(krows.items(), key=lambda kv: -kv[1]):
            say(f"    {k:16s} {ms:9.3f} ms  {100 * ms / total:5.1f} %")
        if krows:
            new, fwd = sum(krows.get(k, 0.0) for k in NEW), sum(krows.get(k, 0.0) for k in FORWARD)
            say(f"    the three new kernels {new:.3f} ms ({100 * new / total:.1f} %), forward kernels {fwd:.3f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


def kernel_rows(a):
    """--child under rocprofv3 --kernel-trace --stats in a fresh process group -> ({kernel: total ms of one call}, note)"""
    d = tempfile.mkdtemp(prefix="sample_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", "1"]
    try:
        proc = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
    except OSError as e:
        return {}, f"(rocprofv3 could not be started: {e})"
    try:
        rc = proc.wait(timeout=a.trace_timeout)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        return {}, f"(rocprofv3 run killed after {a.trace_timeout} s)"
    if rc != 0:
        return {}, f"(rocprofv3 run failed: exit status {rc})"
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            hit = [k for k in NEW + FORWARD if k in row["Name"]]
            if hit:
                k = max(hit, key=len)
                rows[k] = rows.get(k, 0.0) + int(row["Calls"]) * float(row["AverageNs"]) / 1e6 / 2       # (two calls in the child)
    return rows, "" if rows else "(no kernel rows in the kernel stats)"


if __name__ == "__main__":
    sys.exit(main())
