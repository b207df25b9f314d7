"""Rates of the Sobol' sensitivity call (spart_sobol) against the floor a user reaches without it: one Engine.run (float64,
pruned) of the same N (F + 2) M table rows, already on the device, forward only, no reduction at all.

    python tools/sobol_rate.py [--reps 10] [--out profiles/sobol_rate.txt] [--no-trace]

Workload: Sentinel-2A (nb = 13), R_TOC, F = 8 free parameters, 655 360 forward rows as ONE site of N = 65 536 base samples and
as 64 sites of N = 1024, float64, the designs of spart_amd.sobol_design on the device.
  a  the whole call (Engine.sobol) and the forward call of the same rows (Engine.run), device events, medians after two warm-up
     calls, and their ratio;
  b  the count of words in which the call's six outputs differ from tools/sobol_defined.py given Engine.run as its forward model;
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
import sobol_defined as sd  # noqa: E402
from refine_rate import SENSOR, event_ms, stats  # noqa: E402

FREE = ["LAI", "Cab", "Cw", "Cdm", "N", "LIDFa", "B", "SMp"]
SHAPES = {"one": (1, 65536), "many": (64, 1024)}               # label -> (M sites, N base samples)
NEW = ("k_sobol_rows", "k_sobol_blocks", "k_sobol_finish")
FORWARD = ("k_prelude", "k_columns", "k_bands")
KERNELS = NEW + FORWARD


def workload(M, N):
    from spart_amd import sobol_design, workloads
    cols = [workloads.PARAM_NAMES.index(n) for n in FREE]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in FREE], dtype=np.float64) for i in (0, 1))
    sites = workloads.lhs_params(max(M, 2), "full", seed=77)[:M]
    uA, uB = sobol_design(N, len(FREE), seed=1)
    return sites, cols, lo, hi, uA, uB


def child(a):
    """the program rocprofv3 is pointed at: two calls of one shape"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    M, N = SHAPES[a.child]
    sites, _, _, _, uA, uB = workload(M, N)
    P = torch.as_tensor(np.ascontiguousarray(sites.T), device=eng.device)
    design = tuple(torch.as_tensor(u, device=eng.device) for u in (uA, uB))
    for _ in range(2):
        eng.sobol(P, FREE, design=design)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
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
    F = len(FREE)
    say(f"spart_sobol on MI355X (one GCD), tools/sobol_rate.py: {SENSOR}, nb = {eng.nb}, R_TOC, F = {F} free parameters {FREE}, "
        f"float64; device events, medians of {a.reps} after 2 warm-up calls.  forward: Engine.run(float64, prune=True) of the same "
        "table rows already on the device, no reduction -- the floor of a user without the call.")
    ok = True
    for label, (M, N) in SHAPES.items():
        sites, cols, lo, hi, uA, uB = workload(M, N)
        rows = M * N * (F + 2)
        say()
        say(f"{label}: M = {M} site(s), N = {N} base samples, {rows} forward rows in chunks of {((1 << 19) // (64 * (F + 2))) * 64 * (F + 2)}, "
            f"workspace {int(eng.lib.spart_sobol_workspace_bytes(eng.ctx, M, N, F)) / 2 ** 20:.1f} MiB")
        P = torch.as_tensor(np.ascontiguousarray(sites.T), device=eng.device)
        design = tuple(torch.as_tensor(u, device=eng.device) for u in (uA, uB))
        res = {}
        ts = event_ms(torch, lambda: res.update(eng.sobol(P, FREE, design=design)), a.reps)
        xA, xB = sd.points_defined(uA, lo, hi), sd.points_defined(uB, lo, hi)
        table = torch.as_tensor(np.ascontiguousarray(np.concatenate([sd.rows_defined(s, cols, xA, xB) for s in sites]).T), device=eng.device)
        kept = {}
        tf = event_ms(torch, lambda: kept.update(eng.run(table, "float64", prune=True)), a.reps)
        say(f"  a  spart_sobol {stats(ts)}")
        say(f"     forward     {stats(tf)}")
        say(f"     spart_sobol / forward = {np.median(ts) / np.median(tf):.3f}; the call's own part {np.median(ts) - np.median(tf):.3f} ms")
        Y = kept["R_TOC"].cpu().numpy()
        ref = sd.sobol_defined(sites, cols, lo, hi, uA, uB, lambda t: Y)
        got = {k: res[k].cpu().numpy() for k in sd.OUTS}
        bad = {k: int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()) for k in sd.OUTS}
        big = max(float(np.nanmax(np.abs(got[k] - ref[k]))) for k in sd.OUTS)
        ok = ok and not any(bad.values())
        say(f"  b  words differing from the definition: {sum(bad.values())} of {sum(v.size for v in ref.values())} "
            f"(largest |kernel - definition| = {big:g}); largest ST {np.nanmax(got['ST']):.3f}, largest ST_se {np.nanmax(got['ST_se']):.4f}")
        if a.no_trace:
            say("  rocprofv3 --kernel-trace --stats: (not collected: --no-trace)")
            continue
        krows, note = kernel_rows(a, label)
        ok = ok and not note
        total = sum(krows.values())
        say(f"  rocprofv3 --kernel-trace --stats (a separate run, 2 calls in a fresh process; ms of ONE call): {note}")
        for k, ms in sorted(krows.items(), key=lambda kv: -kv[1]):
            say(f"    {k:16s} {ms:9.3f} ms  {100 * ms / total:5.1f} %")
        if krows:
            new, fwd = sum(krows.get(k, 0.0) for k in NEW), sum(krows.get(k, 0.0) for k in FORWARD)
            say(f"    the three new kernels {new:.3f} ms ({100 * new / total:.1f} %), forward kernels {fwd:.3f} ms" +
                ("  -- the new kernels take MORE than the forward call" if new > fwd else ""))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


def kernel_rows(a, label):
    """--child under rocprofv3 --kernel-trace --stats in a fresh process group -> ({kernel: total ms of one call}, note)"""
    d = tempfile.mkdtemp(prefix="sobol_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", label]
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
            hit = [k for k in KERNELS if k in row["Name"]]
            if hit:
                k = max(hit, key=len)
                rows[k] = rows.get(k, 0.0) + int(row["Calls"]) * float(row["AverageNs"]) / 1e6 / 2       # (two calls in the child)
    return rows, "" if rows else "(no kernel rows in the kernel stats)"


if __name__ == "__main__":
    sys.exit(main())
