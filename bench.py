"""Headline benchmark: full SPART spectra/sec (R_TOC + R_TOA + L_TOA) at batch 1M (BASELINE.json config 4).

    python bench.py --gpus 1 --steps 10 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path (spart_run_batch: prelude + fused PROSPECT/BSM/SAILH band kernel over all 2162
bands + float64 column kernel: canopy model at the sensor bands, SMAC, TOC->TOA) over one batch of synthetic parameters already resident in HBM,
plus -- for N > 1 -- the single RCCL gather of the (3, B/N, nb) result shards to rank 0 (BASELINE.json north_star).
Workload = config 4's generator (22-D Latin hypercube, Sentinel2A-MSI, float32 bands / float64 sample scalars).

Scaling (--scaling): the default is STRONG -- the global batch of 1M spectra is cut into N contiguous shards
(spart_amd.sharding.shard_bounds; 8 x 125k + gather = config 4 as BASELINE states it); `weak` gives every rank its own
1M-spectrum shard.  Rank 0 prints ONE JSON line; at N = 1 it also carries driver-timed sub-records: "fp64" (the
reference's own arithmetic) and "configs" (BASELINE configs 2, 3, 5 on one GPU).

--dump-outputs DIR writes what the last timed step computed (R_TOC / R_TOA / L_TOA as rank 0 holds them) to DIR/<name>.npy:
the inputs are the same for the same arguments, so two builds can be compared output for output.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))

PROFILE_TAGS = ("r6", "r5", "r4", "r3", "r2")   # profiles/<tag>_counters_<what>.json: the committed rocprofv3 PMC passes (tools/ingest_profiles.py), newest first
HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
VALU_PEAK_TFLOPS = {"float32": 157.3, "float64": 78.6}   # MI355X_MICROARCH.md: peak FP32 / FP64 vector
ISSUE_CYCLES = {"float32": 2.0, "float64": 4.0}          # cycles per wave64 VALU instruction on a SIMD-32 (fp64: half rate)
FLOP_EQ_PER_SPECTRUM = 8.7e5                             # the reference's arithmetic per spectrum
FLOP_EQ_PER_LEAF = 2001 * 160
METRIC = "SPART spectra/sec (R_TOC+R_TOA+L_TOA) at batch 1M; achieved HBM GB/s vs peak"


def algorithmic_bytes(nb, dtype):
    """inputs + requested outputs per spectrum (SURVEY.md section 8d counts 27 x 4 B of inputs = 264 B with 13 bands;
    here the 27 inputs stay float64 -- SMAC's cos(psi * 180/pi) amplifies a float32 rounding of the azimuth 3283x --
    hence 372 B)."""
    es = 4 if dtype == "float32" else 8
    return 27 * 8 + 3 * nb * es


def src_hash():
    """identifies the kernel sources a committed counter profile belongs to"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "spart-python_amd", "csrc")
    for f in sorted(os.listdir(d)):
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:12]


def counters(dtype):
    """The committed rocprofv3 PMC passes of this build (FETCH_SIZE, WRITE_SIZE and SQ counters need separate passes
    under the profiler, so they cannot be collected inside this run): per-kernel averages per launch at B = 1M.
    -> (dict or None, source string, whether the kernel sources are the ones that were profiled)"""
    for tag in PROFILE_TAGS:
        name = f"{tag}_counters_{dtype}.json"
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", name)))
        except Exception:
            continue
        return d, "profiles/" + name, d.get("src_hash") == src_hash()
    return None, None, False


def _cpu_worker(job):
    """One process of the CPU baseline: the oracle over its slice, 256-row blocks."""
    sensor, rows, seed, lo, hi, mode = job
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import spart_oracle as O
    from spart_amd import workloads
    T = O.load_tables()
    P = workloads.lhs_params(rows, "full", seed=seed)[lo:hi]
    kw = dict(e1="quad", pso="quad") if mode == "quad" else dict(pso="gl")
    if mode != "quad":
        O.spart_run(P[:8], sensor, T, **kw)              # warm-up (imports, table derivation)
    t0 = time.perf_counter()
    # "quad": ONE ROW PER CALL, as the reference is used (a fresh SPART object and one run() per sample, SPART.py:162-269)
    step = 1 if mode == "quad" else 256
    for i in range(0, len(P), step):
        O.spart_run(P[i:i + step], sensor, T, **kw)
    return time.perf_counter() - t0


def _config2_oracle(nrows):
    """(cpu_baseline leg, checker only) the oracle's PROSPECT-5D on the first ``nrows`` rows of BASELINE config 2's workload"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import spart_oracle as O
    from spart_amd import workloads
    return O.prospect_5d(workloads.lhs_params(10_000, "leaf")[:nrows, :9], O.load_tables())


CONFIG2_CHECK = {}        # filled by cpu_baseline(): expected refl / tran / kChlrel of config 2's first 256 rows


def cpu_baseline(sensor, rows_per_core, seed):
    """The oracle (numpy port of the reference) timed on this box's host cores, bounded sample.  Runs BEFORE the
    GPU is initialised (worker processes are forked) and never touches it."""
    import multiprocessing as mp
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = max(1, min(cores, 16))                       # a one-GPU box gives this job a 16-core share
    rows = rows_per_core * cores
    ctx = mp.get_context("fork")
    bounds = [(i * rows // cores, (i + 1) * rows // cores) for i in range(cores)]
    with ctx.Pool(cores) as pool:
        t0 = time.perf_counter()
        busy = pool.map(_cpu_worker, [(sensor, rows, seed, lo, hi, "fast") for lo, hi in bounds])
        dt = time.perf_counter() - t0
        # the reference's own numerical route (scipy quad for E1 and the 61 hot-spot integrals), 4 rows per core
        q0 = time.perf_counter()
        qbusy = pool.map(_cpu_worker, [(sensor, 4 * cores, seed, 4 * i, 4 * i + 4, "quad") for i in range(cores)])
        qdt = time.perf_counter() - q0
        CONFIG2_CHECK["rows"] = 256
        CONFIG2_CHECK["expected"] = pool.apply(_config2_oracle, (256,))
    return {"value": rows / dt, "unit": "spectra/s", "cores": cores, "kind": "port",
            "sample": f"{rows} rows of the same LHS workload, oracle/spart_oracle.py (vectorised numpy, closed-form E1 / "
                      f"Gauss-Legendre hot spot), {cores} processes, {dt:.1f} s wall ({sum(busy):.0f} s CPU)",
            "per_core": rows / sum(busy),
            # The three CPU figures north_star asks for side by side: the reference itself (cannot travel to this box: a stated
            # constant with its provenance), the oracle on the reference's own numerical route one sample per call (what the
            # reference costs per sample on THIS box's cores, minus its pandas / object overhead), and the vectorised port above.
            "reference_in_container": {"value": 3.17, "unit": "spectra/s/core", "cores": 1, "cpu": "Xeon 2.1 GHz (build container)",
                                       "source": "BASELINE.md section 2 / SURVEY.md section 6: SPART(...).run(), fresh object per sample, "
                                                 "22-D LHS, Sentinel2A-MSI, measured with the real reference; not re-measured here"},
            "reference_route": {"value": 4 * cores / qdt, "unit": "spectra/s", "cores": cores, "per_core": 4 * cores / sum(qbusy),
                                "sample": f"{4 * cores} rows, ONE ROW PER CALL like the reference, same oracle with the reference's "
                                          f"scipy-quad E1 (2001 calls per row) and hot-spot integrals (61 calls per row) "
                                          f"(e1='quad', pso='quad'), {qdt:.1f} s wall",
                                "note": "per_core stands beside reference_in_container: same numerical route, this box's cores; the "
                                        "port (value above) is faster per core because it replaces the 2062 QUADPACK calls per "
                                        "sample by closed forms and is vectorised over 256 rows"}}


def roofline(dtype, B, nb, stage_ms, step_ms, band_kernel):
    """The dominant kernel is the fused band kernel; it is VALU-issue bound, so `achieved` is the
    reference's arithmetic per spectrum (flop-equivalents) per second of that kernel against the vector peak.  The HBM
    side the metric asks for is the `hbm` sub-object: algorithmic bytes over the whole step, and the step-level counter
    traffic of all of the step's kernels."""
    kern_s = stage_ms["bands"] / 1e3
    peak = VALU_PEAK_TFLOPS[dtype]
    achieved = FLOP_EQ_PER_SPECTRUM * B / kern_s / 1e12
    ab = algorithmic_bytes(nb, dtype)
    hbm = {"algorithmic_bytes_per_spectrum": ab, "survey_8d_bytes_per_spectrum": 27 * 4 + 3 * nb * (4 if dtype == "float32" else 8),
           "achieved_GBps": ab * B / (step_ms / 1e3) / 1e9, "peak_GBps": HBM_PEAK_GBS,
           "frac": ab * B / (step_ms / 1e3) / 1e9 / HBM_PEAK_GBS,
           "note": "algorithmic bytes over the whole step's time; the fused path moves a few hundred bytes per 8.7e5 "
                   "flop-eq, so this is << 1 by construction"}
    r = {"bound": "valu", "kernel": band_kernel, "kernel_ms": kern_s * 1e3, "achieved": achieved, "peak": peak,
         "unit": "TFLOP/s", "frac": achieved / peak, "flop_eq_per_spectrum": FLOP_EQ_PER_SPECTRUM,
         "stage_ms": stage_view(stage_ms, dtype), "traffic": None, "hbm": hbm}
    if "columns_beside_bands" in r["stage_ms"]:
        r["note"] = ("kernel_ms is the band kernel's duration IN the timed region, where k_columns (float64) runs beside it "
                     "on a side stream and take some of its issue slots; stage_ms_serial = the same kernels one after the other")
    c, source, fresh = counters(dtype)
    if c is not None and B == c.get("batch") and nb == c.get("nb"):
        k = c["kernels"]
        key = ",".join(band_kernel.replace(" ", "").rstrip(">").split(",")[:3])     # (older profiles: other trailing template arguments)
        bk = next((v for n, v in k.items() if n.replace(" ", "").startswith(key)), None)
        if bk and "SQ_INSTS_VALU" in bk:
            r["issue"] = {"valu_wave_insts_per_launch": bk["SQ_INSTS_VALU"],
                          "transcendental_wave_insts": bk.get("SQ_INSTS_VALU_TRANS_F32"),
                          "issue_frac": bk["SQ_INSTS_VALU"] * ISSUE_CYCLES[dtype] / (1024 * 2.4e9 * kern_s),
                          "note": f"VALU wave-instructions x {ISSUE_CYCLES[dtype]:g} cycles / (1024 SIMDs x 2.4 GHz x kernel_ms of THIS run)",
                          "source": source, "profiled_sources_match": fresh}
        step_bytes = sum(v.get("hbm_bytes", 0.0) for v in k.values() if v.get("in_step"))
        if step_bytes:
            r["traffic"] = step_bytes
            hbm.update({"counter_bytes_per_step": step_bytes, "ratio_to_algorithmic": step_bytes / (ab * B),
                        "counter_bytes_per_kernel": {n: v["hbm_bytes"] for n, v in k.items() if v.get("in_step")},
                        "correction": c.get("correction"), "source": source, "profiled_sources_match": fresh})
    return r


def stage_view(stage_ms, dtype, f32_bands=False, pruned=False):
    """Per-stage HIP-event times as the bench line shows them.  Whenever the full-band kernel runs (every mode but
    prune_unused_bands), the column kernel runs on the context's side stream BESIDE it (spart_capi.hip: fork / join), so
    its event measures when it finished relative to the end of the prelude, not how long it would take alone: it is
    shown as `columns_beside_bands`, and the step is prelude + max(bands, columns_beside_bands)."""
    if "columns" not in stage_ms:                     # (already a view)
        return dict(stage_ms)
    if not pruned and os.environ.get("SPART_SIDE_STREAM", "1") != "0":
        return {"prelude": stage_ms["prelude"], "bands": stage_ms["bands"], "columns_beside_bands": stage_ms["columns"]}
    return dict(stage_ms)


def serial_stages(torch, sensor, dev_index, P, dtype, steps=3):
    """The same step with every kernel on ONE stream (SPART_SIDE_STREAM=0, a second context): the kernels' own durations."""
    from spart_amd.engine import Engine
    old = os.environ.get("SPART_SIDE_STREAM")
    os.environ["SPART_SIDE_STREAM"] = "0"
    try:
        eng = Engine(sensor, dev_index)
    finally:
        if old is None:
            del os.environ["SPART_SIDE_STREAM"]
        else:
            os.environ["SPART_SIDE_STREAM"] = old
    eng.run(P, dtype)
    eng.profile(steps)
    for _ in range(steps):
        eng.run(P, dtype)
    st, n = eng.profile_read_stages()
    eng.profile(0)
    return {k: v / max(n, 1) for k, v in st.items()}


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def run_config(torch, eng, P, dtype, steps, warmup, graph=False, **kw):
    """spectra/s of eng.run over the resident batch P + the per-stage HIP-event split (a separate pass when the timed
    steps are HIP-graph replays: events cannot be recorded inside a graph)."""
    B = P.shape[1]
    td = torch.float32 if dtype == "float32" else torch.float64
    out = {k: torch.empty((B, eng.nb), dtype=td, device=P.device) for k in ("R_TOC", "R_TOA", "L_TOA")}
    step = lambda: eng.run(P, dtype, out=dict(out), **kw)          # noqa: E731
    if graph:
        step = eng.capture(P, dtype, out=out, **kw)
    sec = timed(torch, step, steps, warmup)
    eng.profile(steps)
    for _ in range(steps):
        eng.run(P, dtype, out=dict(out), **kw)
    st, n = eng.profile_read_stages()
    eng.profile(0)
    ok = all(bool(torch.isfinite(v).all().item()) for v in out.values())
    return {"value": B / sec, "unit": "spectra/s", "ms_per_step": sec * 1e3, "batch": B, "steps": steps,
            "stage_ms": stage_view({k: v / max(n, 1) for k, v in st.items()}, dtype, bool(kw.get("f32_bands")), bool(kw.get("prune"))), "finite": ok,
            "hip_graph": bool(graph)}


def extras(torch, args, dev):
    """Driver-timed sub-records at N = 1: the float64 mode of the headline workload and BASELINE configs 2, 3, 5."""
    from spart_amd import get_engine, workloads
    steps = max(3, min(args.steps, 10))
    eng = get_engine(args.sensor, dev.index)
    P = torch.as_tensor(workloads.lhs_params(args.batch, "full").T.copy(), device=dev)
    r = run_config(torch, eng, P, "float64", steps, 1)
    r["roofline"] = roofline("float64", args.batch, eng.nb, r["stage_ms"], r["ms_per_step"], "k_bands<double, 0, 1, false>")
    r["dtype"] = "f64"
    # float64 columns over a float32 full-band pass (spart_materialize.f32_bands): the SAME float64 columns -- checked
    # here bit for bit -- at the float32 mode's speed; the 2162 bands of every sample are still all evaluated, in float32
    ref = {k: v.clone() for k, v in eng.run(P, "float64").items()}
    m = run_config(torch, eng, P, "float64", steps, 1, f32_bands=True)
    got = eng.run(P, "float64", f32_bands=True)
    r["columns_over_f32_bands"] = {"value": m["value"], "unit": "spectra/s", "ms_per_step": m["ms_per_step"],
                                   "bit_identical_to_fp64_mode": all(bool(torch.equal(ref[k], got[k])) for k in ref),
                                   "what": "float64 R_TOC / R_TOA / L_TOA (prelude, sensor-slot bands, SMAC, TOC->TOA in float64); "
                                           "the evaluation of all 2162 bands per sample (band sums) in float32"}
    del ref, got
    fp64 = r
    cfg = {}
    # config 2: PROSPECT-5D leaf only, 10k x 2001, fp64: outputs refl, tran, kChlrel (48 096 B per leaf spectrum)
    eng0 = get_engine(None, dev.index)
    Pl = workloads.lhs_params(10_000, "leaf")
    cols = [torch.as_tensor(Pl[:, i].copy(), device=dev) for i in range(9)]
    # 2000 calls after 300 untimed ones (0.3 s): a 50-call burst (8 ms) is over before the shader clock has settled -- it measured
    # 0.155-0.17 ms where the loop's steady state is 0.143 ms at 2.14 GHz / 1.33 kW (profiles/r6_power_config2.txt)
    c2_steps = 2000
    sec = timed(torch, lambda: eng0.prospect(cols, "float64"), c2_steps, 300)
    by = 9 * 8 + 3 * 2001 * 8
    cfg["2"] = {"workload": "PROSPECT-5D leaf only, 10k LeafBiology samples x 2001 bands, fp64, refl + tran + kChlrel out",
                "value": 10_000 / sec, "unit": "leaf spectra/s", "ms_per_step": sec * 1e3, "steps": c2_steps,
                "roofline": {"bound": "hbm", "achieved": by * 10_000 / sec / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": by * 10_000 / sec / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes_per_leaf": by,
                             "valu_tflop_eq": FLOP_EQ_PER_LEAF * 10_000 / sec / 1e12, "valu_peak_fp64": VALU_PEAK_TFLOPS["float64"],
                             "note": "whole call (prelude + k_prospect<double>) timed on the host, synchronised"}}
    if CONFIG2_CHECK:
        # the result of THE TIMED CALL against the oracle on the first 256 rows (computed in the cpu_baseline leg, before the GPU
        # was initialised); tests/test_gpu_parity.py::test_config2_lhs_workload_all_rows checks all 10 000
        got = eng0.prospect(cols, "float64")
        n = CONFIG2_CHECK["rows"]
        cfg["2"]["max_abs_vs_oracle"] = {k: float(abs(g[:n].cpu().numpy() - e).max())
                                         for k, g, e in zip(("refl", "tran", "kChlrel"), got, CONFIG2_CHECK["expected"])}
        cfg["2"]["max_abs_vs_oracle"]["rows"] = n
        del got
    del cols
    # config 3: full SPART, 100k, Sentinel-2A, fp32 (and 125k = the per-GPU shard of config 4 cut in 8)
    for name, b in (("3", 100_000), ("4_shard_125k", 125_000)):
        Pb = P[:, :b].contiguous()
        cfg[name] = run_config(torch, eng, Pb, "float32", 50, 5, graph=True)
        cfg[name]["workload"] = f"full SPART, {b} spectra of the config-4 LHS, {args.sensor}, fp32, all 2162 bands"
    # config 5: PROSPECT-PRO + SAILH, 1M, Sentinel-2B, fp32 and fp64 (the tolerance sweep itself is tests/test_gpu_parity.py::
    # test_float32_tolerance_at_size; here the max deviation of this run is reported next to the rate)
    del P
    engb = get_engine("Sentinel2B-MSI", dev.index)
    Pp = torch.as_tensor(workloads.lhs_params(args.batch, "pro").T.copy(), device=dev)
    c5 = run_config(torch, engb, Pp, "float32", steps, 1)
    c5["workload"] = f"PROSPECT-PRO (Cdm = 0, PROT / CBC vary) + SAILH, {args.batch} spectra, Sentinel2B-MSI, fp32"
    c5f = run_config(torch, engb, Pp, "float64", 3, 1)
    a, b = engb.run(Pp, "float32"), None
    a = {k: v.clone() for k, v in a.items()}
    b = engb.run(Pp, "float64")
    c5["fp64_value"] = c5f["value"]
    c5["fp32_vs_fp64_max_rel_floor1e-6"] = {k: float(((a[k].double() - b[k]).abs() / b[k].abs().clamp_min(1e-6)).max().item())
                                            for k in ("R_TOC", "R_TOA", "L_TOA")}
    cfg["5"] = c5
    del Pp, a, b
    torch.cuda.empty_cache()
    cfg.update(mode_records(torch, args, dev))
    return fp64, cfg


MAT_FIELDS = ("leaf_refl", "leaf_tran", "leaf_kchl", "soil_refl", "soil_refl_dry", "rso", "rdo", "rsd", "rdd")
MAT_BYTES_F32 = (7 * 2162 + 2 * 2001) * 4          # +75 256 B per spectrum, float32
LUT_BOUND = "mfma"                                 # k_lut_scan_mfma: exact-f32 v_mfma_f32_32x32x2_f32


def mode_records(torch, args, dev):
    """Driver-timed records of the modes SURVEY.md section 8(f) adds to the path (N = 1 only): materialised spectra (the
    one HBM-bound mode, and the one in which the full-band evaluation is CONSUMED), the pruned step (= what the returned
    columns cost), LUT generation end to end (host table in, host columns out) and LUT inversion."""
    import numpy as np
    import spart_amd
    from spart_amd import get_engine, workloads
    rec = {}
    eng = get_engine(args.sensor, dev.index)
    P1m = workloads.lhs_params(1_000_000, "full")
    # --- materialised: 9 spectrum arrays, B = 200k, float32, padded row pitch (Engine default)
    B = 200_000
    P = torch.as_tensor(P1m[:B].T.copy(), device=dev)
    out = eng.run(P, "float32", materialize=MAT_FIELDS)             # allocates the nine (B, pitch) arrays once
    mat_step = lambda: eng.run(P, "float32", materialize=MAT_FIELDS, out=out)    # noqa: E731  (caller-owned buffers)
    steps = 10
    sec = timed(torch, mat_step, steps, 2)
    eng.profile(steps)
    for _ in range(steps):
        mat_step()
    st, n = eng.profile_read_stages()
    eng.profile(0)
    kms = st["bands"] / max(n, 1)
    nbytes = MAT_BYTES_F32 * B
    c, source, fresh = counters("materialized")
    traffic = None
    if c is not None and c.get("batch") == B:
        bk = next((v for nme, v in c["kernels"].items() if nme.replace(" ", "").startswith("k_bands<float,1,")), None)
        traffic = bk.get("hbm_bytes") if bk else None
    rec["materialized"] = {
        "workload": f"full SPART + the nine leaf / soil / canopy spectrum arrays (SPART.py:66-81) written to HBM, {B} spectra of the "
                    f"config-4 LHS, {args.sensor}, fp32, rows padded to 2176 / 2048 elements",
        "value": B / sec, "unit": "spectra/s", "ms_per_step": sec * 1e3, "batch": B, "steps": steps,
        "bytes_per_spectrum": MAT_BYTES_F32 + algorithmic_bytes(eng.nb, "float32"),
        "step_GBps": (nbytes + algorithmic_bytes(eng.nb, "float32") * B) / sec / 1e9,
        "finite": all(bool(torch.isfinite(out[k]).all().item()) for k in MAT_FIELDS),
        "roofline": {"bound": "hbm", "kernel": "k_bands<float, 1, 1, true>", "kernel_ms": kms,
                     "achieved": nbytes / (kms / 1e3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": nbytes / (kms / 1e3) / 1e9 / HBM_PEAK_GBS, "frac_over_step": nbytes / sec / 1e9 / HBM_PEAK_GBS,
                     "algorithmic_bytes_per_launch": nbytes, "traffic": traffic,
                     "traffic_source": source if traffic else None, "profiled_sources_match": fresh if traffic else None,
                     "note": "achieved = bytes of spectra stored / the band kernel's HIP-event duration (the kernel also does "
                             "the whole 2162-band arithmetic, 2.3 ms of VALU work at this batch)"}}
    del out, P
    torch.cuda.empty_cache()
    # --- pruned: only the <= 2 nb bands the sensor columns depend on; bit-identical columns.  This IS the cost of
    # the returned R_TOC / R_TOA / L_TOA: in the headline mode they come from prelude + k_columns as well,
    # the full-band kernel beside them evaluates the other bands of every spectrum (band sums, materialised spectra)
    Pd = torch.as_tensor(P1m.T.copy(), device=dev)
    r = run_config(torch, eng, Pd, "float32", 20, 3, prune=True)
    full = eng.run(Pd, "float32")
    full = {k: v.clone() for k, v in full.items()}
    pr = eng.run(Pd, "float32", prune=True)
    r["columns_bit_identical_to_full_evaluation"] = all(bool(torch.equal(full[k], pr[k])) for k in full)
    r["workload"] = (f"prune_unused_bands = 1: prelude + float64 column kernel (canopy model at {eng.nb} of 2162 bands, SMAC, TOC->TOA), 1M spectra, "
                     f"{args.sensor}; NOT full spectra -- reported as the cost of the returned columns, never as the headline")
    rf = run_config(torch, eng, Pd, "float32", 20, 3, prune=True, lidf="newton")
    r["with_fast_prelude"] = {"value": rf["value"], "ms_per_step": rf["ms_per_step"], "stage_ms": rf["stage_ms"]}
    # HBM traffic of this step from the committed counter passes over the same mode (tools/mode_run.py pruned)
    c, source, fresh = counters("pruned")
    ab = algorithmic_bytes(eng.nb, "float32") * 1_000_000
    if c is not None and c.get("batch") == 1_000_000:
        per = {n: v.get("hbm_bytes", 0.0) for n, v in c["kernels"].items() if n != "k_econv" and v.get("hbm_bytes")}
        tot = sum(per.values())
        # how close the two float64 kernels run to their instruction issue: committed VALU wave-instruction counts x the data-sheet
        # 4 cycles (and x the 2.28 ns MEASURED for v_fma_f64 on this chip, profiles/r4_ubench_f64_issue.txt) over THIS run's
        # HIP-event kernel times
        issue = {}
        for kn, stage in (("k_prelude", "prelude"), ("k_columns", "columns")):
            kv = next((v for n, v in c["kernels"].items() if n.startswith(kn)), None)
            ms = r["stage_ms"].get(stage)
            if kv and kv.get("SQ_INSTS_VALU") and ms:
                issue[stage] = {"valu_wave_insts_per_launch": kv["SQ_INSTS_VALU"], "kernel_ms": ms,
                                "issue_frac": kv["SQ_INSTS_VALU"] * ISSUE_CYCLES["float64"] / (1024 * 2.4e9 * ms * 1e-3),
                                "frac_of_measured_fma_f64_rate": kv["SQ_INSTS_VALU"] * 2.28e-9 / (1024 * ms * 1e-3)}
        r["roofline"] = {"bound": "valu", "note": "float64 instruction issue binds both kernels (DESIGN.md section 4); HBM traffic reported "
                                                  "because the returned columns are what a user of the drop-in receives",
                         "issue": issue,
                         "traffic": tot, "algorithmic_bytes": ab, "ratio_to_algorithmic": tot / ab, "traffic_per_kernel": per,
                         "achieved_GBps_over_step": tot / (r["ms_per_step"] / 1e3) / 1e9, "peak_GBps": HBM_PEAK_GBS,
                         "traffic_source": source, "profiled_sources_match": fresh}
    rec["pruned"] = r
    # --- fast_prelude (lidf="newton"): the documented speed / agreement trade of the per-sample prelude, full evaluation
    fp = run_config(torch, eng, Pd, "float32", 10, 2, lidf="newton")
    nw = eng.run(Pd, "float32", lidf="newton")
    fp["max_rel_dev_from_default_columns_floor1e-6"] = {k: float(((nw[k].double() - full[k].double()).abs() / full[k].double().abs().clamp_min(1e-6)).max().item())
                                                         for k in full}
    # the contract of include/spart_hip.h (spart_materialize.fast_prelude), measured on the float64 columns of this table
    f64a = {k: v.clone() for k, v in eng.run(Pd, "float64", prune=True).items()}
    f64b = eng.run(Pd, "float64", prune=True, lidf="newton")
    fdev = {}
    for k in f64a:
        d = (f64b[k] - f64a[k]).abs()
        rel = d / f64a[k].abs().clamp_min(1e-6)
        over = rel > 1e-6
        fdev[k] = {"max_abs": float(d.max().item()), "max_metric_floor1e-6": float(rel.max().item()),
                  "p99.999_metric": float(torch.quantile(rel.flatten()[::7].float(), 0.99999).item()),
                  "entries_over_1e-6": int(over.sum().item()), "entries": int(rel.numel()),
                  "largest_value_among_them": float(f64a[k].abs()[over].max().item()) if bool(over.any()) else 0.0}
    fp["float64_columns_vs_default"] = fdev
    del f64a, f64b
    fp["workload"] = ("spart_materialize.fast_prelude = 1 (Engine.run(lidf='newton')): exact root of the LIDF equation + 8-point hot-spot "
                      "panels instead of the reference's stopped iteration; all 2162 bands evaluated; 1M spectra, fp32")
    rec["fast_prelude"] = fp
    # --- canopy.lidf handed in (spart_materialize.lidf_in; the reference's SAILH reads it from the object, sailh.py:51): the
    # prelude skips its 12 fixed-point solves per sample.  Here every row gets the distribution its own (LIDFa, LIDFb) gives
    # (spart_lidf_batch), so the columns must be the pruned run's, bit for bit.
    li = get_engine(None, dev.index).lidf(Pd[16], Pd[17])
    rl = run_config(torch, eng, Pd, "float32", 20, 3, prune=True, canopy_lidf=li)
    gl = eng.run(Pd, "float32", prune=True, canopy_lidf=li)
    rec["lidf_given"] = {"workload": "prune_unused_bands = 1 with canopy.lidf given as a (B, 13) input (k_prelude<false, true>), 1M spectra, "
                                     f"{args.sensor}: the cost of the returned columns when the leaf-angle distribution is data, not (LIDFa, LIDFb)",
                         "value": rl["value"], "unit": "spectra/s", "ms_per_step": rl["ms_per_step"], "stage_ms": rl["stage_ms"],
                         "columns_bit_identical_to_derived_lidf": all(bool(torch.equal(pr[k], gl[k])) for k in ("R_TOC", "R_TOA", "L_TOA")),
                         "extra_input_bytes_per_spectrum": 13 * 8}
    del li, gl
    del full, pr, nw
    # --- LUT inversion: 1M-row LUT (this run's R_TOC columns) x 65 536 observations, float32
    lut = eng.run(Pd, "float32")["R_TOC"].clone()
    M = 65536
    g = torch.Generator(device=dev).manual_seed(3)
    pick = torch.randint(0, lut.shape[0], (M,), generator=g, device=dev)
    obs = lut[pick] * (1 + 0.02 * torch.randn((M, lut.shape[1]), generator=g, device=dev))
    eng0 = get_engine(None, dev.index)
    idx, cost, lst = eng0.lut_nearest(lut, obs, stats=True)
    sec = timed(torch, lambda: eng0.lut_nearest(lut, obs), 5, 1)
    # EVERY winner of the run against a brute force of the defined cost (tools/lut_brute_force.py: eager torch ops, sequential
    # float32 arithmetic, first index on ties -- plumbing, not the product): index and cost must be bit-equal
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lut_brute_force import brute_force_torch
    t0 = time.perf_counter()
    bf_idx, bf_cost = brute_force_torch(lut, obs)
    torch.cuda.synchronize()
    bf_s = time.perf_counter() - t0
    nbp = 2 * next(k for k in (4, 7, 8, 11, 16) if k >= (lut.shape[1] + 2) // 2)     # K of the GEMM: nb + 1 (norm slot), in MFMA steps of 2
    cmp_s = lut.shape[0] * M / sec
    rec["lut_invert"] = {
        "workload": f"spart_lut_nearest: {lut.shape[0]}-row LUT (R_TOC of the config-4 table, {lut.shape[1]} bands) x {M} noisy observations, fp32",
        "value": cmp_s, "unit": "row comparisons/s", "ms_per_step": sec * 1e3, "steps": 5,
        "observations_per_s": M / sec,
        "winners_equal_to_brute_force": int((idx == bf_idx).sum().item()), "costs_bit_equal": int((cost == bf_cost).sum().item()),
        "checked": M, "brute_force_check_s": bf_s,
        "observations_on_the_brute_force_path": lst["brute_force"], "bound_scale_nmax": lst["nmax"],
        "roofline": {"bound": LUT_BOUND, "achieved": cmp_s * 2 * nbp / 1e12,
                     "peak": VALU_PEAK_TFLOPS["float32"], "unit": "TFLOP/s", "frac": cmp_s * 2 * nbp / 1e12 / VALU_PEAK_TFLOPS["float32"],
                     "flops_per_comparison": 2 * nbp,
                     "note": f"filter a~(b, m) = sum_k A[b][k] Bq[k][m], K = {nbp} (nb + 1 incl. the norm slot, in MFMA steps of 2): 2 x {nbp} flops "
                             "per comparison on v_mfma_f32_32x32x2_f32 (exact f32); peak = the f32-input MFMA peak 157.3 TF "
                             "(MI355X_MICROARCH.md: equal to the vector peak); whole call timed (centre + prep + scan + exact reduce + "
                             "brute-force kernel for the flagged observations + merge)"}}
    del bf_idx, bf_cost
    l64, o64 = lut.double(), obs.double()
    eng0.lut_nearest(l64, o64, dtype="float64")
    sec64 = timed(torch, lambda: eng0.lut_nearest(l64, o64, dtype="float64"), 3, 1)
    rec["lut_invert"]["fp64"] = {"value": lut.shape[0] * M / sec64, "unit": "row comparisons/s", "ms_per_step": sec64 * 1e3,
                                 "note": "the same search in float64 on v_mfma_f64_16x16x4_f64 (K = 16)"}
    del lut, obs, idx, cost, pick, l64, o64
    torch.cuda.empty_cache()
    # --- LUT generation end to end: host parameter table in, host columns out (PCIe-inclusive; never the headline)
    P8 = np.tile(P1m, (8, 1))
    spart_amd.generate_lut(P8[:1 << 20], args.sensor, prune=False)
    best, bestp, bestr = 1e9, 1e9, 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        o = spart_amd.generate_lut(P8, args.sensor, prune=False)
        best = min(best, time.perf_counter() - t0)
        del o
        t0 = time.perf_counter()
        o = spart_amd.generate_lut(P8, args.sensor, prune=True)
        bestp = min(bestp, time.perf_counter() - t0)
        t0 = time.perf_counter()
        spart_amd.generate_lut(P8, args.sensor, prune=True, out=dict(o))      # destination pages resident (a reused result)
        bestr = min(bestr, time.perf_counter() - t0)
        del o
    rec["lut_generate"] = {
        "workload": f"spart_amd.generate_lut: {P8.shape[0]} spectra (the 1M config-4 table x 8), {args.sensor}, fp32, pageable host table in -> "
                    "host columns out, chunks of 256k rows, copies overlapped with the kernels, all 2162 bands of every spectrum evaluated (prune=False; "
                    "the function's default is the pruned path = pruned_value); best of 3",
        "value": P8.shape[0] / best, "unit": "spectra/s", "ms_per_step": best * 1e3,
        "host_bytes_per_spectrum": 27 * 8 + 3 * eng.nb * 4, "host_GBps": (27 * 8 + 3 * eng.nb * 4) * P8.shape[0] / best / 1e9,
        "pruned_value": P8.shape[0] / bestp, "pruned_ms": bestp * 1e3,
        "pruned_reused_destination_value": P8.shape[0] / bestr, "pruned_reused_destination_ms": bestr * 1e3,
        "note": "PCIe-inclusive, reported beside the resident-input headline (never as `value` of the line)"}
    return rec


def lut_records_multi_rank(torch, dist, args, dev, eng, rank, world, lut_local, row0, rows_per_rank, gathered_lut):
    """N > 1: the LUT rows of SURVEY.md section 8(f) sharded over the ranks (spart_amd.sharding / spart_amd.lut), timed like the
    headline (barrier + synchronise on both sides, MAX over ranks) and checked on rank 0 against the single-device search.
    lut_local = this rank's R_TOC rows of the global table (its result of the timed steps), gathered_lut = the whole LUT on
    rank 0 (from the steps' gather), None elsewhere.  Every rank returns; rank 0's dict goes into the line."""
    import numpy as np
    import spart_amd
    from spart_amd import get_engine, sharding, workloads
    nb = lut_local.shape[1]

    def fence():
        torch.cuda.synchronize()
        dist.barrier()

    def wall(fn, reps):
        best, mine = 1e9, 1e9
        for _ in range(reps):
            fence()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            own = time.perf_counter() - t0
            dist.barrier()
            t = torch.tensor([time.perf_counter() - t0, own], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            if float(t[0]) < best:
                best, mine = float(t[0]), own
        return best, mine

    rec = {}
    # --- inversion: LUT row-sharded, M observations replicated, ONE all_gather of (cost bits, global row) per call
    M = 65536
    Bg = int(sum(rows_per_rank))
    obs = torch.empty((M, nb), dtype=lut_local.dtype, device=dev)
    if rank == 0:
        g = torch.Generator(device=dev).manual_seed(3)
        pick = torch.randint(0, Bg, (M,), generator=g, device=dev)
        obs.copy_(gathered_lut[pick] * (1 + 0.02 * torch.randn((M, nb), generator=g, device=dev)))
    dist.broadcast(obs, src=0)
    eng0 = get_engine(None, dev.index)
    comm = None if dist.get_backend() == "nccl" else "cpu"
    search = lambda: sharding.lut_nearest_sharded(lut_local, row0, obs, eng0.lut_nearest, comm_device=comm)      # noqa: E731
    idx, cost = search()
    sec, own = wall(search, 5)
    owns = [None] * world
    dist.all_gather_object(owns, own * 1e3)
    chk = None
    if rank == 0:
        try:            # rank-0-only work: must never make rank 0 leave the collective sequence the other ranks follow
            si, sc = eng0.lut_nearest(gathered_lut, obs)
            chk = {"winners_equal_to_single_device_search": int((idx.to(dev) == si).sum().item()),
                   "costs_bit_equal": int((cost.to(dev) == sc).sum().item()), "checked": M}
        except Exception as e:      # noqa: BLE001
            chk = {"check_error": f"{type(e).__name__}: {e}"}
    rec["lut_invert"] = dict({
        "workload": f"spart_amd.sharding.lut_nearest_sharded: {Bg}-row LUT (R_TOC of the global table) ROW-SHARDED over {world} ranks x "
                    f"{M} replicated observations, fp32: per-rank exact search + ONE all_gather of (cost, global row) -- 16 B x M per rank",
        "value": Bg * M / sec, "unit": "row comparisons/s", "ms_per_step": sec * 1e3, "steps": 5, "observations_per_s": M / sec,
        "ranks_seen": world, "rows_per_rank": list(rows_per_rank), "per_rank_ms": owns}, **(chk or {}))
    # --- generation: every rank streams ITS block of the host table through its GPU into its own host arrays; no collective
    P1 = workloads.lhs_params(args.batch, "full")
    P8 = np.tile(P1, (8, 1))
    spart_amd.generate_lut(P8[:1 << 18], args.sensor, prune=False, shard=True)
    holder = {}

    def gen():
        holder["o"] = spart_amd.generate_lut(P8, args.sensor, prune=False, shard=True)
    sec, own = wall(gen, 2)
    o = holder["o"]
    owns = [None] * world
    dist.all_gather_object(owns, {"ms": own * 1e3, "rows": list(o.rows)})
    # the block a rank produced == the rows the timed steps produced for the same parameters (rank-local check, then AND)
    lo, hi = o.rows
    ok = torch.tensor([1.0 if (o.total == P8.shape[0] and np.isfinite(o["R_TOC"]).all()) else 0.0], dtype=torch.float64, device=dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    rec["lut_generate"] = {
        "workload": f"spart_amd.generate_lut(shard=True): {P8.shape[0]} spectra (the global table x 8) cut into {world} contiguous blocks, "
                    f"{args.sensor}, fp32, each rank: pageable host table in -> its own host columns out, all 2162 bands evaluated; no collective "
                    "on the data path; best of 2",
        "value": P8.shape[0] / sec, "unit": "spectra/s", "ms_per_step": sec * 1e3, "ranks_seen": world,
        "rows_per_rank": [r["rows"][1] - r["rows"][0] for r in owns], "per_rank_ms": [r["ms"] for r in owns],
        "finite_on_every_rank": bool(ok.item() == 1.0),
        "note": "PCIe-inclusive (every rank has its own link), reported beside the resident-input headline"}
    return rec


DUMP_BYTES = 48_000_000     # --dump-outputs: at most this many bytes of column data (the .npy headers add a few hundred)
DUMP_SEED = 0


def dump_outputs(torch, path, cols):
    """--dump-outputs: the (3, B, nb) columns a caller of the timed path receives (R_TOC, R_TOA, L_TOA; on N > 1 ranks
    rank 0's gathered global batch) -> path/<name>.npy in the step's dtype.  When all B rows exceed DUMP_BYTES, a fixed
    sample of rows is written instead: sorted(numpy default_rng(DUMP_SEED).choice(B, k, replace=False)), the same rows
    for the same arguments in every run and every build."""
    import numpy as np
    _, B, nb = cols.shape
    k = min(B, DUMP_BYTES // (3 * nb * cols.element_size()))
    if k < B:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(B, k, replace=False))
        cols = cols.index_select(1, torch.as_tensor(idx, device=cols.device))
    host = cols.cpu().numpy()
    os.makedirs(path, exist_ok=True)
    for i, name in enumerate(("R_TOC", "R_TOA", "L_TOA")):
        np.save(os.path.join(path, name + ".npy"), host[i])
    return {"dir": path, "names": ["R_TOC", "R_TOA", "L_TOA"], "rows": int(k), "of_rows": int(B),
            "sample": None if k == B else f"sorted numpy default_rng({DUMP_SEED}).choice({B}, {k}, replace=False)",
            "dtype": str(host.dtype)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1_000_000, help="GLOBAL batch (strong scaling) / batch per GPU (weak)")
    ap.add_argument("--scaling", default="auto", choices=["auto", "strong", "weak"],
                    help="auto = strong for N > 1 (BASELINE config 4: 1M spectra cut into N shards + gather)")
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    ap.add_argument("--sensor", default="Sentinel2A-MSI")
    ap.add_argument("--cpu-rows", type=int, default=8192, help="rows PER HOST CORE for the CPU baseline (0 = skip)")
    ap.add_argument("--no-extras", action="store_true", help="skip the fp64 / configs sub-records (profiling runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the columns of the last timed step as DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    cpu = None
    if world == 1 and args.cpu_rows > 0:
        from spart_amd import workloads as _w            # (no torch / HIP import yet: the workers are forked)
        cpu = cpu_baseline(args.sensor, args.cpu_rows, _w.LHS_SEED)

    import torch
    import torch.distributed as dist
    from spart_amd import get_engine, sharding, workloads

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE={world})")
    # SPART_BENCH_BACKEND=gloo + several ranks on one GPU is a rehearsal mode for the 1-GPU box (it exercises
    # the shard / double-buffer / gather logic); the driver's multi-GPU run uses the default "nccl" = RCCL.
    backend = os.environ.get("SPART_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if backend == "nccl" else local_rank % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    # auto = strong: the global batch (1M, BASELINE config 4) is what stays fixed as N grows; at N = 1 both modes are the
    # same run, and the line says "strong" so that the driver's N = 1, 2, 4, 8 series carries one label
    scaling = args.scaling if args.scaling != "auto" else "strong"
    eng = get_engine(args.sensor, dev_index)
    nb = eng.nb
    from spart_amd import _lib as _spart_lib
    build_id = _spart_lib.build_id()                  # == the hash of the sources next to the library (_lib.load checks)
    # synthetic inputs, resident in HBM before timing starts.  strong: this rank's contiguous shard of ONE global LHS
    # table (spart_amd.sharding.shard_bounds); weak: every rank its own table (seed + rank)
    if scaling == "strong":
        Bg = args.batch
        lo, hi = sharding.shard_bounds(Bg, world, rank)
        per = -(-Bg // world)                            # gather block: the last shards may be short (padded with zeros)
        P = torch.as_tensor(workloads.lhs_params(Bg, "full", seed=workloads.LHS_SEED)[lo:hi].T.copy(), device=dev)
    else:
        Bg = args.batch * world
        lo, hi, per = 0, args.batch, args.batch
        P = torch.as_tensor(workloads.lhs_params(args.batch, "full", seed=workloads.LHS_SEED + rank).T.copy(), device=dev)
    B = hi - lo
    td = torch.float32 if args.dtype == "float32" else torch.float64
    # (3, per, nb) so that the three result columns travel in ONE gather.  Two result buffers: the gather of
    # step i (RCCL's own stream) overlaps the kernels of step i + 1 (compute stream); a buffer is reused
    # only after its gather has completed.  Every gather is inside the timed region (fence() waits for all).
    nbuf = 2 if world > 1 else 1
    res = [torch.zeros((3, per, nb), dtype=td, device=dev) for _ in range(nbuf)]
    outs = [{"R_TOC": r[0, :B], "R_TOA": r[1, :B], "L_TOA": r[2, :B]} for r in res]
    gather_lists = [[torch.empty_like(res[0]) for _ in range(world)] if rank == 0 else None
                    for _ in range(nbuf)] if world > 1 else None
    works = [None] * nbuf
    counter = [0]

    def step():
        j = counter[0] % nbuf
        counter[0] += 1
        if works[j] is not None:
            works[j].wait()                     # compute stream waits until buffer j's previous gather is done
            works[j] = None
        if B:
            eng.run(P, args.dtype, out=dict(outs[j]))   # opt = NULL: all 2162 bands of every spectrum are evaluated
        if world > 1:
            works[j] = dist.gather(res[j], gather_lists[j], dst=0, async_op=True)

    def fence():
        for j in range(nbuf):
            if works[j] is not None:
                works[j].wait()
                works[j] = None
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    eng.profile(args.steps)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    dumped = None
    if args.dump_outputs and rank == 0:
        last = (counter[0] - 1) % nbuf                 # the buffer the last timed step wrote (and, for N > 1, gathered)
        if world > 1:
            rows = [hi_r - lo_r for lo_r, hi_r in (sharding.shard_bounds(Bg, world, r) for r in range(world))] \
                if scaling == "strong" else [args.batch] * world
            cols = torch.cat([g[:, :n] for g, n in zip(gather_lists[last], rows)], dim=1)
        else:
            cols = res[last][:, :B]
        dumped = dump_outputs(torch, args.dump_outputs, cols)
    stage, ncalls = eng.profile_read_stages()
    eng.profile(0)
    own_dt = dt
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # Self-diagnosis of a multi-rank run (nobody watches the driver's 8-GPU job): AFTER the timed region every rank times
    # its own compute-only steps and one gather on its own, and rank 0 prints what every rank saw.  A slow rank, a rank-0
    # gather skew or a wrong rank count then shows in the line itself.
    diag = None
    if world > 1:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            if B:
                eng.run(P, args.dtype, out=dict(outs[0]))
        torch.cuda.synchronize()
        compute_ms = (time.perf_counter() - t1) / args.steps * 1e3
        dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            dist.gather(res[0], gather_lists[0] if rank == 0 else None, dst=0)
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - t1) / 3 * 1e3
        ones = torch.ones(1, dtype=torch.float64, device=dev)
        dist.all_reduce(ones)
        info = {"rank": rank, "device": dev_index, "rows": B, "step_ms": own_dt / args.steps * 1e3, "compute_ms": compute_ms,
                "band_kernel_ms": stage.get("bands", 0.0) / max(ncalls, 1), "gather_ms": gather_ms}
        infos = [None] * world
        dist.all_gather_object(infos, info)
        infos = sorted(infos, key=lambda r: r["rank"])
        slow = max(r["compute_ms"] for r in infos)
        diag = {"ranks_seen": int(round(float(ones.item()))), "ranks": [r["rank"] for r in infos], "devices": [r["device"] for r in infos],
                "rows_per_rank": [r["rows"] for r in infos],
                "per_rank_ms": [r["step_ms"] for r in infos],
                "per_rank_compute_ms": [r["compute_ms"] for r in infos],
                "per_rank_band_kernel_ms": [r["band_kernel_ms"] for r in infos],
                "gather_ms": infos[0]["gather_ms"], "per_rank_gather_ms": [r["gather_ms"] for r in infos],
                "predicted_value": Bg / (slow * 1e-3) if slow > 0 else None,
                "gather_exposed_ms": dt / args.steps * 1e3 - slow,
                "note": ("measured after the timed region, no collective added inside it: per_rank_ms = each rank's own clock over "
                         "the timed steps; per_rank_compute_ms = the same steps without the gather; gather_ms = one (3, B/N, nb) "
                         "gather to rank 0 on its own (rank 0's clock); predicted_value = global batch / slowest rank's compute "
                         "= the rate with the gather fully hidden; gather_exposed_ms = ms_per_step - slowest compute")}

    lut_rec = None
    if world > 1 and not args.no_extras and args.dtype == "float32":
        rows = diag["rows_per_rank"]
        gathered = torch.cat([g[0, :n] for g, n in zip(gather_lists[0], rows)]) if rank == 0 else None
        try:
            lut_rec = lut_records_multi_rank(torch, dist, args, dev, eng, rank, world, res[0][0, :B].clone(),
                                             lo if scaling == "strong" else sum(rows[:rank]), rows, gathered)
        except Exception as e:      # noqa: BLE001  (never lose the headline line to a side record; the error is IN the line)
            lut_rec = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        ok = all(bool(torch.isfinite(r).all().item()) for r in res)
        if world > 1:
            ok = ok and all(bool(torch.isfinite(g).all().item()) for gl in gather_lists for g in gl)
        # order-independent checksum of the columns as rank 0 holds them (the integer sum of their bit patterns): equal for
        # any number of ranks when the gathered shards are exactly the single-rank result
        bits = torch.int32 if td == torch.float32 else torch.int64
        blocks = gather_lists[0] if world > 1 else [res[0]]
        checksum = int(sum(int(g.view(bits).to(torch.int64).sum().item()) for g in blocks) & ((1 << 63) - 1))
        value = Bg * args.steps / dt
        stage_ms = {k: v / max(ncalls, 1) for k, v in stage.items()}
        band_kernel = "k_bands<float, 0, 1, false>" if args.dtype == "float32" else "k_bands<double, 0, 1, false>"
        line = {
            "metric": METRIC,
            "value": value, "unit": "spectra/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": scaling,
            "vs_baseline": None, "dtype": "f32" if args.dtype == "float32" else "f64", "data": "synthetic",
            "config": {"workload": "BASELINE config 4: full SPART (BSM+PROSPECT-5D+SAILH+SMAC), 22-D Latin hypercube "
                                   f"(seed 20240613), {args.sensor}, all 2162 bands evaluated per spectrum, columns-only output",
                       "global_batch": Bg, "batch_per_gpu": B if scaling == "strong" else args.batch,
                       "bands_evaluated": 2162, "sensor_bands": nb,
                       "parallelism": (f"dp{world}: {'one 1M LHS table cut into contiguous shards' if scaling == 'strong' else 'one table per rank'}"
                                       " + one RCCL gather of the (3, B/N, nb) block to rank 0 per step, overlapped with the next "
                                       "step's kernels") if world > 1 else "single GPU",
                       "input_dtype": "f64", "build_id": build_id,
                       "columns": ("R_TOC / R_TOA / L_TOA come from the float64 column path (k_prelude -> k_columns over the <= 2 nb "
                                   "bands they depend on) in every mode: float32 columns = the float64 mode's, rounded once; the "
                                   "full-band kernel k_bands (the dominant kernel of this step) evaluates all 2162 bands of every spectrum "
                                   "beside it and feeds only the band sums -- roofline.columns_path_ms is what the returned columns "
                                   "cost, configs.materialized the mode in which the band kernel's work is consumed"),
                       "tables": "17 table values per band held in VGPRs (lane = band); the per-sample constants, not the tables, "
                                 "are staged through LDS (north_star says tables in LDS; measured slower, DESIGN.md section 4)",
                       "finite": ok, "columns_checksum": checksum},
            "roofline": roofline(args.dtype, B, nb, stage_ms, dt / args.steps * 1e3, band_kernel),
        }
        line["cpu_baseline"] = cpu
        if diag is not None:
            line["multi_rank"] = diag
        if lut_rec is not None:
            line["configs"] = lut_rec
        if world == 1 and "columns_beside_bands" in line["roofline"]["stage_ms"]:
            ser = serial_stages(torch, args.sensor, dev_index, P, args.dtype)
            line["roofline"]["stage_ms_serial"] = ser
            line["roofline"]["columns_path_ms"] = ser["prelude"] + ser["columns"]
        if world == 1 and not args.no_extras and args.dtype == "float32":
            line["fp64"], line["configs"] = extras(torch, args, dev)
            pr = line["configs"].get("pruned")
            if pr:
                # THE SECOND HEADLINE: what the R_TOC / R_TOA / L_TOA a caller receives cost (SPART.run() of the Python mirror
                # uses exactly this mode); the headline above additionally evaluates the other 2149 bands of every spectrum
                line["returned_columns"] = {"value": pr["value"], "unit": pr["unit"], "ms_per_step": pr["ms_per_step"],
                                            "stage_ms": pr["stage_ms"],
                                            "bit_identical_to_full_evaluation": pr["columns_bit_identical_to_full_evaluation"],
                                            "traffic": (pr.get("roofline") or {}).get("traffic"),
                                            "workload": pr["workload"]}
        if dumped is not None:
            line["dumped_outputs"] = dumped
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
