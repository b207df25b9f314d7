"""Rates of the mixture refinement (spart_refine_mix) against spart_refine_views with the same V, Fs and Fl -- the same
(F + 1) V M forward rows, so the difference is the step kernel.

    python tools/refine_mix_rate.py [--pixels 65536] [--iters 10] [--reps 20] [--out profiles/refine_mix_rate.txt]

Workload: Sentinel-2A (nb = 13), float64, two setups: V = 2 crop / soil (B shared; LAI, Cab local to component 0 only; the
fraction fitted: n = 4) and V = 4 (B shared; LAI, Cab, Cw local everywhere; fractions fitted: n = 16).  Truth = one LHS draw per
component, equal true fractions, starts 10 % of the range away.  Per setup:
  a  the whole spart_refine_mix call (Engine.refine_mix);
  b  the same n_iter + 1 forward calls alone, eng.run(..., "float64", prune=True) on V (F + 1) M rows;
  c  (a - b) / (n_iter + 1): init, step kernel and chunking per iteration, by device events;
  and a, c of spart_refine_views with the same names shared / local (every local in every view) on the components' own columns.
Then the kernels' own rows of `rocprofv3 --kernel-trace --stats` from a separate run of the calls in a child process.
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
import refine_views_rate as rvr  # noqa: E402
from refine_rate import SENSOR, event_ms, stats  # noqa: E402

SETUPS = {"crop / soil": (2, ["B"], ["LAI", "Cab"], {"LAI": [0], "Cab": [0]}),
          "four components": (4, ["B"], ["LAI", "Cab", "Cw"], None)}
KERNELS = ("k_refine_mix_step", "k_refine_mix_init", "k_refine_views_step", "k_refine_views_init", "k_columns", "k_prelude")


def group(n):
    """refine_group / refine_lds_bytes of refine_lds_rows(n, n, MIX_MAXV), from the constants of csrc/spart_refine.h -> (W, LDS bytes)"""
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_refine.h")).read()
    c = {k: int(v) for k, v in re.findall(r"(REFINE_[A-Z_]+) = (\d+)", src)}
    nt = n * (n + 1) // 2
    rows = n * c["REFINE_JT"] + 2 * c["REFINE_JT"] + (nt + n) + nt + 3 * n + 1 + 8
    W = c["REFINE_MAX_GROUP"]
    while W > c["REFINE_MIN_GROUP"] and rows * (W + 1) * 8 > c["REFINE_LDS_BUDGET"]:
        W >>= 1
    return W, rows * (W + 1) * 8


def workload(torch, eng, M, V, shared, local):
    """(start (27, V, M), obs of the mixture (M, nb), obs of the views (M, V, nb)) device tensors"""
    from spart_amd import workloads
    names = shared + local
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
    truth = np.stack([workloads.lhs_params(M, "full", seed=77 + v) for v in range(V)])
    truth[1:, :, cols[:len(shared)]] = truth[0][None][:, :, cols[:len(shared)]]
    rows = torch.as_tensor(np.ascontiguousarray(truth.reshape(V * M, 27).T), device=eng.device)
    comp = eng.run(rows, "float64", prune=True)["R_TOC"].reshape(V, M, -1).permute(1, 0, 2).contiguous()
    start = truth.copy()
    start[:, :, cols] = truth[:, :, cols] + 0.1 * (hi - lo) * np.sign(0.5 * (lo + hi) - truth[:, :, cols])
    start[1:, :, cols[:len(shared)]] = start[0][None][:, :, cols[:len(shared)]]
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(start, 2, 0)), device=eng.device), comp.mean(dim=1).contiguous(), comp


def child(a):
    """the program rocprofv3 is pointed at: three calls of each refinement of each setup"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    for V, shared, local, active in SETUPS.values():
        start, obs, comp = workload(torch, eng, a.pixels, V, shared, local)
        for _ in range(3):
            eng.refine_mix(start, obs, shared, local, active=active, n_iter=a.iters)
            eng.refine_views(start, comp, shared, local, n_iter=a.iters)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=240, help="seconds the rocprofv3 run may take")
    ap.add_argument("--child", action="store_true")
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
    M, nb, calls = a.pixels, eng.nb, a.iters + 1
    say(f"spart_refine_mix on MI355X (one GCD), tools/refine_mix_rate.py: {SENSOR}, nb = {nb}, M = {M} pixels, n_iter = {a.iters} "
        f"({calls} forward calls), float64; device events, medians of {a.reps} after 2 warm-up calls.")
    for title, (V, shared, local, active) in SETUPS.items():
        Fs, Fl = len(shared), len(local)
        F = Fs + Fl
        nloc = V * Fl if active is None else sum(len(v) for v in active.values())
        n, nv = Fs + nloc + V - 1, Fs + V * Fl
        rows = V * (F + 1) * M
        W, lds = group(n)
        Wv, ldsv = rvr.group(F, nv)
        say()
        say(f"{title}: V = {V}, shared {shared}, local {local}" + ("" if active is None else f" active {active}") +
            f", fractions fitted: n = {n} unknowns ({rows} forward rows per call, chunks of {max(1, (1 << 19) // ((F + 1) * V))} pixels).")
        say(f"  k_refine_mix_step: W = {W} pixels, {lds} B of LDS per workgroup;  k_refine_views_step at n = {nv}: W = {Wv}, {ldsv} B.")
        start, obs, comp = workload(torch, eng, M, V, shared, local)
        Pf = torch.as_tensor(np.ascontiguousarray(np.tile(start.reshape(27, -1).cpu().numpy(), (1, F + 1))), device=eng.device)
        out = {k: torch.empty((rows, nb), dtype=torch.float64, device=eng.device) for k in ("R_TOC", "R_TOA", "L_TOA")}

        def forward():
            for _ in range(calls):
                eng.run(Pf, "float64", out=out, prune=True)
        tb = event_ms(torch, forward, a.reps)
        mb = float(np.median(tb))
        say(f"  b  {calls} forward calls alone                               {stats(tb)}   = {mb / calls:.3f} ms per call, "
            f"{mb * 1e6 / (calls * rows):.2f} ns per row")
        res, share = {}, {}
        for name, what, call in (("mix", "the whole spart_refine_mix call", lambda: res.update(eng.refine_mix(start, obs, shared, local, active=active, n_iter=a.iters))),
                                 ("views", f"spart_refine_views, n = {nv}, on the components' columns", lambda: res.update(eng.refine_views(start, comp, shared, local, n_iter=a.iters)))):
            ta = event_ms(torch, call, a.reps)
            ma = float(np.median(ta))
            share[name] = (ma - mb) / calls
            say(f"  a  {what:58s}{stats(ta)}   a / b = {ma / mb:.3f}")
            say(f"  c  (a - b) / {calls}: init, step kernel and chunking per iteration   {share[name]:9.3f} ms   = {(ma - mb) / mb:.3f} of the "
                "forward time of its iteration")
            cost, cost0, na = (res[k].cpu().numpy() for k in ("cost", "cost0", "n_accept"))
            alive = na >= 0
            say(f"     the fit: {int(alive.sum())} of {na.size} alive, median cost / cost0 = {np.median(cost[alive] / cost0[alive]):.3e}, "
                f"median accepted steps = {np.median(na[alive]):.0f}")
        say(f"  c of spart_refine_mix / c of spart_refine_views = {share['mix'] / share['views']:.3f}")
    say()
    ok = True
    if a.no_trace:
        say("rocprofv3 --kernel-trace --stats: (not collected: --no-trace)")
    else:
        d = tempfile.mkdtemp(prefix="refine_mix_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--pixels", str(a.pixels), "--iters", str(a.iters)]
        rows_, note = {}, ""
        try:
            proc = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = proc.wait(timeout=a.trace_timeout)
                note = "" if rc == 0 else f"(rocprofv3 run failed: exit status {rc})"
            except subprocess.TimeoutExpired:
                os.killpg(proc.pid, signal.SIGKILL)
                proc.wait()
                note = f"(rocprofv3 run killed after {a.trace_timeout} s)"
        except OSError as e:
            note = f"(rocprofv3 could not be started: {e})"
        if not note:
            for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    hit = [k for k in KERNELS if k in row["Name"]]
                    if hit:
                        k = max(hit, key=len)
                        cnt, avg = int(row["Calls"]), float(row["AverageNs"]) / 1e6
                        n0, avg0, lo0, hi0 = rows_.get(k, (0, 0.0, np.inf, 0.0))      # (the instantiations of a template add up)
                        rows_[k] = (n0 + cnt, (n0 * avg0 + cnt * avg) / (n0 + cnt), min(lo0, float(row["MinNs"]) / 1e6),
                                    max(hi0, float(row["MaxNs"]) / 1e6))
            if "k_refine_mix_step" not in rows_ or "k_refine_views_step" not in rows_:
                note = "(no step kernel rows in the kernel stats)"
        ok = not note
        say(f"rocprofv3 --kernel-trace --stats (a separate run, 3 calls of each refinement of both setups in a fresh process): {note}")
        for k, (cnt, avg, lo_, hi_) in sorted(rows_.items()):
            say(f"  {k:20s} {cnt:5d} calls, average {avg:.3f} ms (min {lo_:.3f}, max {hi_:.3f})")
        if ok:
            # all launches of both setups together (the last chunk of a call is short), per pixel and iteration
            px = 3 * calls * M * len(SETUPS)
            per_m = rows_["k_refine_mix_step"][0] * rows_["k_refine_mix_step"][1] / px
            per_v = rows_["k_refine_views_step"][0] * rows_["k_refine_views_step"][1] / px
            say(f"  step kernel per pixel and iteration, both setups together: mixture {per_m * 1e6:.2f} ns, views {per_v * 1e6:.2f} ns, "
                f"ratio {per_m / per_v:.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
