"""Rates of the joint refinement over views (spart_refine_views) against spart_refine on the same number of forward rows.

    python tools/refine_views_rate.py [--pixels 65536] [--views 4] [--iters 10] [--reps 20] [--out profiles/refine_views_rate.txt]

Workload: Sentinel-2A (nb = 13), M LHS rows as the truth of the pixels, V views with their own tts / tto / psi, Fs = 4 shared
parameters (LAI, Cab, Cw, Cdm) and Fl = 1 local one (aot550), started 10 % of their range away, float64.
  a  the whole spart_refine_views call (Engine.refine_views);
  b  the same n_iter + 1 forward calls alone, eng.run(..., "float64", prune=True) on V (F + 1) M rows;
  c  (a - b) / (n_iter + 1): init, step kernel and chunking per iteration, by device events;
and the yardstick beside it: a, b, c of spart_refine with F = 5 (the same names, all free per observation) on V M
observations -- the same number of forward rows.  Then the kernels' own rows of `rocprofv3 --kernel-trace --stats` from a
separate run of both calls in a child process, the ratio of the two step kernels, and the W and LDS bytes refine_group picks.
Device events, medians after two warm-up calls; every figure in the report is measured in this run.
"""
import argparse
import csv
import glob
import os
import re
import signal
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from refine_rate import SENSOR, event_ms, stats  # noqa: E402

SHARED, LOCAL = ["LAI", "Cab", "Cw", "Cdm"], ["aot550"]
GEOMETRY = [dict(tts=30.0, tto=0.0, psi=0.0), dict(tts=45.0, tto=25.0, psi=20.0), dict(tts=55.0, tto=28.0, psi=160.0),
            dict(tts=20.0, tto=10.0, psi=90.0)]


def group(F, n):
    """refine_group / refine_lds_bytes of refine_lds_rows(F + 1, n, 0), from the constants of csrc/spart_refine.h -> (W, LDS bytes)"""
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine.h")).read()
    c = {k: int(v) for k, v in re.findall(r"(REFINE_[A-Z_]+) = (\d+)", src)}
    nt = n * (n + 1) // 2
    rows = (F + 1) * c["REFINE_JT"] + 2 * c["REFINE_JT"] + (nt + n) + nt + 3 * n + 1
    W = c["REFINE_MAX_GROUP"]
    while W > c["REFINE_MIN_GROUP"] and rows * (W + 1) * 8 > c["REFINE_LDS_BUDGET"]:
        W >>= 1
    return W, rows * (W + 1) * 8


def workload(torch, eng, M, V):
    """(start (27, V, M), obs (M, V, nb)) device tensors"""
    from spart_amd import workloads
    names = SHARED + LOCAL
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
    truth = np.repeat(workloads.lhs_params(M, "full", seed=77)[None], V, axis=0)
    for v in range(V):
        for k, val in GEOMETRY[v % len(GEOMETRY)].items():
            truth[v, :, workloads.PARAM_NAMES.index(k)] = val + v // len(GEOMETRY)
    rows = torch.as_tensor(np.ascontiguousarray(truth.reshape(V * M, 27).T), device=eng.device)
    obs = eng.run(rows, "float64", prune=True)["R_TOC"].reshape(V, M, -1).permute(1, 0, 2).contiguous()
    start = truth.copy()
    start[:, :, cols] = truth[:, :, cols] + 0.1 * (hi - lo) * np.sign(0.5 * (lo + hi) - truth[:, :, cols])
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(start, 2, 0)), device=eng.device), obs


def child(a):
    """the program rocprofv3 is pointed at: three calls of each refinement"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    start, obs = workload(torch, eng, a.pixels, a.views)
    flat, fobs = start.reshape(27, -1).contiguous(), obs.permute(1, 0, 2).reshape(-1, eng.nb).contiguous()
    for _ in range(3):
        eng.refine_views(start, obs, SHARED, LOCAL, n_iter=a.iters)
        eng.refine(flat, fobs, SHARED + LOCAL, n_iter=a.iters)
    torch.cuda.synchronize()


KERNELS = ("k_refine_views_step", "k_refine_views_init", "k_refine_step", "k_columns", "k_prelude")


def kernel_lines(a):
    """--child under rocprofv3 --kernel-trace --stats in a fresh process group -> ({kernel: (calls, average ms, min, max)}, note)"""
    d = tempfile.mkdtemp(prefix="refine_views_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", "--pixels", str(a.pixels), "--views", str(a.views), "--iters", str(a.iters)]
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
                n, avg = int(row["Calls"]), float(row["AverageNs"]) / 1e6
                n0, avg0, lo0, hi0 = rows.get(k, (0, 0.0, np.inf, 0.0))          # (the instantiations of a template add up)
                rows[k] = (n0 + n, (n0 * avg0 + n * avg) / (n0 + n), min(lo0, float(row["MinNs"]) / 1e6), max(hi0, float(row["MaxNs"]) / 1e6))
    return rows, "" if "k_refine_views_step" in rows and "k_refine_step" in rows else "(no step kernel rows in the kernel stats)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=65536)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=240, help="seconds the rocprofv3 run may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    Fs, Fl = len(SHARED), len(LOCAL)
    if not 1 <= a.views <= (16 - Fs) // Fl:
        ap.error(f"--views: 1 ... {(16 - Fs) // Fl}")
    if a.child:
        return child(a)
    import torch
    from spart_amd import get_engine
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = get_engine(SENSOR, 0)
    M, V, nb, calls = a.pixels, a.views, eng.nb, a.iters + 1
    F, n = Fs + Fl, Fs + V * Fl
    rows = V * (F + 1) * M
    chunk = max(1, (1 << 19) // ((F + 1) * V))
    W, lds = group(F, n)
    W0, lds0 = group(F, F)
    say(f"spart_refine_views on MI355X (one GCD), tools/refine_views_rate.py: {SENSOR}, nb = {nb}, M = {M} pixels, V = {V} views, "
        f"shared {SHARED}, local {LOCAL} (n = {n} unknowns), n_iter = {a.iters} ({calls} forward calls of {rows} rows, in chunks of "
        f"{chunk} pixels), float64; device events, medians of {a.reps} after 2 warm-up calls.")
    say(f"k_refine_views_step: groups of W = {W} pixels, {lds} B of LDS per workgroup;  k_refine_step at F = {F}: W = {W0}, {lds0} B.")
    say()
    start, obs = workload(torch, eng, M, V)
    flat, fobs = start.reshape(27, -1).contiguous(), obs.permute(1, 0, 2).reshape(-1, nb).contiguous()
    res = {}
    Pf = torch.as_tensor(np.ascontiguousarray(np.tile(flat.cpu().numpy(), (1, F + 1))), device=eng.device)
    out = {k: torch.empty((rows, nb), dtype=torch.float64, device=eng.device) for k in ("R_TOC", "R_TOA", "L_TOA")}

    def forward():
        for _ in range(calls):
            eng.run(Pf, "float64", out=out, prune=True)
    tb = event_ms(torch, forward, a.reps)
    mb = float(np.median(tb))
    say(f"  b  {calls} forward calls alone (V (F + 1) M = {rows} rows each)        {stats(tb)}   = {mb / calls:.3f} ms per call, "
        f"{mb * 1e6 / (calls * rows):.2f} ns per row")
    share = {}
    for name, what, call in (("views", "the whole spart_refine_views call", lambda: res.update(eng.refine_views(start, obs, SHARED, LOCAL, n_iter=a.iters))),
                             ("plain", f"spart_refine, F = {F}, on V M = {V * M} observations", lambda: res.update(eng.refine(flat, fobs, SHARED + LOCAL, n_iter=a.iters)))):
        ta = event_ms(torch, call, a.reps)
        ma = float(np.median(ta))
        share[name] = (ma - mb) / calls
        say(f"  a  {what:58s}{stats(ta)}   a / b = {ma / mb:.3f}")
        say(f"  c  (a - b) / {calls}: init, step kernel and chunking per iteration   {share[name]:9.3f} ms   = {(ma - mb) / mb:.3f} of the forward "
            "time of its iteration")
        cost, cost0, na = (res[k].cpu().numpy() for k in ("cost", "cost0", "n_accept"))
        alive = na >= 0
        say(f"     the fit: {int(alive.sum())} of {na.size} alive, median cost / cost0 = {np.median(cost[alive] / cost0[alive]):.3e}, median "
            f"accepted steps = {np.median(na[alive]):.0f}")
    say(f"  c of spart_refine_views / c of spart_refine = {share['views'] / share['plain']:.3f}")
    say()
    ok = True
    if a.no_trace:
        say("rocprofv3 --kernel-trace --stats: (not collected: --no-trace)")
    else:
        rows_, note = kernel_lines(a)
        ok = not note
        say(f"rocprofv3 --kernel-trace --stats (a separate run, 3 calls of each in a fresh process): {note}")
        for k, (cnt, avg, lo_, hi_) in sorted(rows_.items()):
            say(f"  {k:20s} {cnt:5d} calls, average {avg:.3f} ms (min {lo_:.3f}, max {hi_:.3f})")
        if ok:
            # all launches of the three calls together (the last chunk of a call is short), per observation and iteration
            per_v = rows_["k_refine_views_step"][0] * rows_["k_refine_views_step"][1] / (3 * calls * M * V)
            per_p = rows_["k_refine_step"][0] * rows_["k_refine_step"][1] / (3 * calls * M * V)
            say(f"  step kernel per observation and iteration: views {per_v * 1e6:.2f} ns, spart_refine {per_p * 1e6:.2f} ns, ratio {per_v / per_p:.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
