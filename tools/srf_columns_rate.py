"""Rate of the SRF-convolved sensor columns (spart_materialize.R_TOC_srf ... rdd_srf, kernel k_columns_srf).

    python tools/srf_columns_rate.py [--rows 262144] [--reps 20] [--sensor Sentinel2A-MSI] [--out profiles/srf_columns_rate.txt]
                                     [--trace-dir DIR | --no-trace]

Workload: Latin-hypercube parameters on one sensor (Sentinel-2A by default), float64, every buffer resident and preallocated.
Timed with device events on the current stream, medians of --reps calls after two warm-up calls:
  a  a pruned call without the *_srf outputs                      (prelude + k_columns: what the new path adds to)
  b  a pruned call with the seven *_srf outputs                   (a + k_columns_srf)
  c  the only route to the same numbers without the kernel: a pruned call that materialises rso, rdo, rsd, rdd in float64
     (B x 2162 each) followed by the same convolution with torch on the device -- four matrix products of the (B, 2162)
     spectra with the (2162, nb) matrix of q_e / Q_j -- then the division is done; SMAC and TOC -> TOA are NOT redone, so c is
     a lower bound of that route
and the ratio c / b, which must be at least 2.  The seven outputs of b are compared with c's four canopy columns.
The kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of this script's --child mode in a fresh process,
started LAST, after the timings: its k_columns_srf line is copied into the report.  If that run fails or exceeds its time
limit the report is still written, with the failure in place of the line, and the tool exits with status 1.
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
CANOPY = ("rso", "rdo", "rsd", "rdd")
SRF7 = ["R_TOC_srf", "R_TOA_srf", "L_TOA_srf", "rso_srf", "rdo_srf", "rsd_srf", "rdd_srf"]


def stats(ts):
    return f"{np.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, n = {len(ts)})"


def event_ms(torch, f, reps, warm=2):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def support_matrix(eng):
    """(2162, nb) float64: column j holds q_e / 1 at the grid row of every entry of band j (the thermal evaluation at row 2001),
    and Q (nb,): the library's own support (spart_srf_support)"""
    import ctypes
    from spart_amd import _lib
    w, p = eng._keep["wsrf"], eng._keep["psrf"]
    nsrf, nb = w.shape
    ip = ctypes.POINTER(ctypes.c_int32)
    start = np.zeros(nb + 1, np.int32)
    _lib.check(eng.lib, None, eng.lib.spart_srf_support(w.ctypes.data_as(_lib.c_dp), p.ctypes.data_as(_lib.c_dp), nsrf, nb,
                                                        start.ctypes.data_as(ip), None, None, None))
    ev, q, Q = np.zeros(start[nb], np.int32), np.zeros(start[nb]), np.zeros(nb)
    _lib.check(eng.lib, None, eng.lib.spart_srf_support(w.ctypes.data_as(_lib.c_dp), p.ctypes.data_as(_lib.c_dp), nsrf, nb,
                                                        start.ctypes.data_as(ip), ev.ctypes.data_as(ip), q.ctypes.data_as(_lib.c_dp),
                                                        Q.ctypes.data_as(_lib.c_dp)))
    W = np.zeros((_lib.NWLS, nb))
    for j in range(nb):
        W[ev[start[j]:start[j + 1]], j] = q[start[j]:start[j + 1]]
    return W, Q, int(start[nb])


def child(a):
    """the program rocprofv3 is pointed at: a few pruned calls with the *_srf outputs"""
    import torch
    from spart_amd import get_engine, workloads
    eng = get_engine(a.sensor, 0)
    P = torch.as_tensor(workloads.lhs_params(a.rows, "full", seed=77).T.copy(), device=eng.device)
    for _ in range(5):
        eng.run(P, "float64", materialize=SRF7, prune=True)
    torch.cuda.synchronize()


def kernel_line(a):
    """run --child under rocprofv3 --kernel-trace --stats in a fresh process group -> (the k_columns_srf row of its kernel
    stats, ok).  A child that fails or runs into the time limit (the whole group is then killed) gives ok = False."""
    d = a.trace_dir or tempfile.mkdtemp(prefix="srf_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", "--rows", str(a.rows), "--sensor", a.sensor]
    try:
        proc = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
    except OSError as e:
        return f"(rocprofv3 could not be started: {e})", False
    try:
        rc = proc.wait(timeout=a.trace_timeout)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        return f"(rocprofv3 run killed after {a.trace_timeout} s)", False
    if rc != 0:
        return f"(rocprofv3 run failed: exit status {rc})", False
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_columns_srf" in row["Name"]:
                return (f"k_columns_srf: {row['Calls']} calls, average {float(row['AverageNs']) / 1e6:.3f} ms, min "
                        f"{float(row['MinNs']) / 1e6:.3f}, max {float(row['MaxNs']) / 1e6:.3f}, {row['Percentage']} % of the "
                        f"kernel time of the run   [{row['Name'][:60]}...]"), True
    return "(no k_columns_srf row in the kernel stats)", False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sensor", default="Sentinel2A-MSI")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=240, help="seconds the rocprofv3 run may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    from spart_amd import _lib, get_engine, workloads
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = get_engine(a.sensor, 0)
    B, nb = a.rows, eng.nb
    P = torch.as_tensor(workloads.lhs_params(B, "full", seed=77).T.copy(), device=eng.device)
    cols = lambda: {k: torch.empty((B, nb), dtype=torch.float64, device=eng.device) for k in ("R_TOC", "R_TOA", "L_TOA")}
    out_a, out_b, out_c = cols(), cols(), cols()
    out_b.update({k: torch.empty((B, nb), dtype=torch.float64, device=eng.device) for k in SRF7})
    out_c.update({k: eng._alloc_spec(B, _lib.NWLS, torch.float64) for k in CANOPY})
    W, Q, nsup = support_matrix(eng)
    Wd, Qd = torch.as_tensor(W, device=eng.device), torch.as_tensor(Q, device=eng.device)
    conv = {k: torch.empty((B, nb), dtype=torch.float64, device=eng.device) for k in CANOPY}
    say(f"SRF-convolved sensor columns on MI355X (one GCD), tools/srf_columns_rate.py: {a.sensor}, nb = {nb}, sum_j |E_j| = {nsup} "
        f"band evaluations per sample, float64, B = {B}; device events, medians of {a.reps} after 2 warm-up calls.")
    say()

    def call_a():
        eng.run(P, "float64", out=out_a, prune=True)

    def call_b():
        eng.run(P, "float64", out=out_b, materialize=SRF7, prune=True)

    def call_c():
        eng.run(P, "float64", out=out_c, materialize=CANOPY, prune=True)
        for k in CANOPY:
            torch.matmul(out_c[k], Wd, out=conv[k])
            conv[k].div_(Qd)

    def call_c_spectra():
        eng.run(P, "float64", out=out_c, materialize=CANOPY, prune=True)
    ta = event_ms(torch, call_a, a.reps)
    tb = event_ms(torch, call_b, a.reps)
    tc = event_ms(torch, call_c, a.reps)
    tcs = event_ms(torch, call_c_spectra, a.reps)
    ma, mb, mc = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
    say(f"  a  pruned call, no *_srf outputs                              {stats(ta)}")
    say(f"  b  pruned call + the seven *_srf outputs                      {stats(tb)}   = {mb * 1e6 / B:.2f} ms per 1M samples")
    say(f"     b - a (the SRF kernel's share of the call)                 {mb - ma:9.3f} ms   = {(mb - ma) * 1e6 / B:.2f} ms per 1M samples, "
        f"{(mb - ma) * 1e9 / (B * nsup):.1f} ps per band evaluation")
    say(f"  c  pruned call materialising rso, rdo, rsd, rdd + torch       {stats(tc)}")
    say(f"     of which the materialising call alone                      {stats(tcs)}   ({4 * B * _lib.NWLS * 8 / 1e9:.1f} GB of spectra stored)")
    ratio = mc / mb
    say(f"  c / b = {ratio:.2f}   requirement (at least 2): {'met' if ratio >= 2 else 'MISSED'}")
    torch.cuda.synchronize()
    worst = max(float(((out_b[k + "_srf"] - conv[k]).abs() / conv[k].abs().clamp_min(1e-6)).max()) for k in CANOPY)
    say(f"  rso_srf ... rdd_srf of b against c's convolution of the materialised spectra: worst |d| / max(|ref|, 1e-6) = {worst:.2e}")
    say()
    del out_a, out_b, out_c, conv                      # the traced process gets the device memory back
    torch.cuda.empty_cache()
    trace, ok = ("(not collected: --no-trace)", True) if a.no_trace else kernel_line(a)
    say(f"rocprofv3 --kernel-trace --stats (a separate run, 5 calls of b in a fresh process): {trace}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
