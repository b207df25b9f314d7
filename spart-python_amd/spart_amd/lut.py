"""Look-up-table generation: stream a large parameter table through the GPU in chunks and land the sensor
columns in host memory / on disk.  The host<->device copies of chunk i+1 / i run on their
own HIP streams beside the kernels (double-buffered device buffers, no host staging copy), so the PCIe traffic
(216 B in + 3*nb*4 B out per spectrum) hides behind the evaluation whenever the link keeps up.

On-disk layout (a directory):
    meta.json                  sensor, band ids, band centres, dtype, parameter names, number of rows, band model
    params.npy   (B, 27) f64   the parameter table (workloads.PARAM_NAMES order)
    R_TOC.npy / R_TOA.npy / L_TOA.npy   (B, nb) in the chosen dtype
    products.npy (B, 5) f64    optional, written by lut_products: fAPAR_bs, fAPAR_ws, albedo_bs, albedo_ws, fCover of every row
All .npy files are plain numpy arrays (np.load(..., mmap_mode="r") works for tables larger than RAM).
"""
import ctypes
import json
import os
import warnings

import numpy as np

from . import _lib, workloads
from .engine import (BAND_MODELS, DTYPES, PRODUCT_NAMES, _SRF_COLUMNS, Engine, _band_model, chain_summary, get_engine, knn_prior,  # noqa: F401
                     lut_weights_kind, sample_args,
                     params_rows, prior_arrays, product_names, products_columns, quantile_levels, refine_args, refine_plan,
                     refine_leaf_args, refine_mix_args, refine_series_args, refine_tiles_args, refine_views_args, sobol_args, sobol_design, vjp_args)

COLUMNS = ("R_TOC", "R_TOA", "L_TOA")
LUT_MAX_K = 256                    # the k of spart_lut_topk / spart_lut_summarise: 1 ... 256


def _np_dtype(name):
    """the numpy dtype of a LUT's columns (meta.json "dtype", one of engine.DTYPES' names), which is the dtype its searches run in"""
    return np.float32 if DTYPES.get(name, _lib.SPART_F64) == _lib.SPART_F32 else np.float64


def _torch_dtype(npdt):
    import torch
    return getattr(torch, np.dtype(npdt).name)


def _host_tensor(a):
    """the numpy array ``a`` as a CPU tensor over the same memory"""
    import torch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # read-only inputs (memmaps opened "r") are only read
        return torch.from_numpy(a)


def _check_out(out, shapes):
    """out= of generate_lut / retrieve_stream: ``shapes`` {name: (shape, dtype)} -> {name: out[name]}, each checked"""
    for n, (s, d) in shapes.items():
        a = out.get(n)
        if not isinstance(a, np.ndarray) or a.shape != s or a.dtype != d or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError(f"out[{n!r}] must be a writable C-contiguous {s} {np.dtype(d).name} array")
    return {n: out[n] for n in shapes}


def _check_k(k):
    if not 1 <= int(k) <= LUT_MAX_K:
        raise ValueError(f"k = {k}, expected 1 <= k <= {LUT_MAX_K}")
    return int(k)


_MADV_POPULATE_WRITE = 23          # linux/mman.h (Linux >= 5.14): fault the range in, writable, inside ONE system call
_libc = None


def _prefault(a):
    """Make the pages under the C-contiguous numpy view ``a`` resident and writable without touching their contents.
    The destination of a LUT is fresh memory (1.25 GB per 8M Sentinel-2 spectra): left to the download copies, its
    first-touch page faults -- zero-filling 4 KB at a time on the copying thread -- cost more than the kernels that
    produce the data.  Several threads call this on disjoint slices ahead of the pipeline (ctypes releases the GIL).
    Returns False where the kernel does not know MADV_POPULATE_WRITE (then the copies fault the pages in as before)."""
    global _libc
    if a.nbytes == 0:
        return True
    if _libc is None:
        _libc = ctypes.CDLL(None, use_errno=True)
        _libc.madvise.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page = os.sysconf("SC_PAGE_SIZE")
    lo = a.ctypes.data & ~(page - 1)
    try:
        return _libc.madvise(lo, a.ctypes.data + a.nbytes - lo, _MADV_POPULATE_WRITE) == 0
    except Exception:               # noqa: BLE001  (pre-faulting is an optimisation: never let it fail the LUT)
        return False


class LutBlock(dict):
    """Result of generate_lut: the column arrays, with ``rows = (lo, hi)`` = the rows THIS process evaluated (the whole
    table unless ``shard=True`` under a process group) and ``total`` = the table's row count.  Without ``path`` a sharded call
    returns arrays holding only the rows lo..hi; with ``path`` the arrays are memmaps of the whole files."""
    rows = (0, 0)
    total = 0


def _group_info(shard, group):
    """(world, rank) of the process group a sharded call runs under; (1, 0) for a plain call"""
    if not shard:
        return 1, 0
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1, 0
    return dist.get_world_size(group), dist.get_rank(group)


def open_lut_files(path, files, world=1, rank=0, group=None):
    """The .npy files of a LUT directory as writable memmaps shared by the ranks of a sharded generate_lut.
    files: [(name, dtype, shape)].  Rank 0 creates them at their final size (and removes a manifest left over from an earlier
    table: meta.json is what says "complete"); after ONE barrier the other ranks open the same files read-write; every rank
    then writes only its own rows (single node: one page cache; on a network file system every rank must flush before the
    closing barrier, which generate_lut does)."""
    whole = None
    if rank == 0:
        os.makedirs(path, exist_ok=True)
        stale = os.path.join(path, "meta.json")
        if os.path.exists(stale):
            os.remove(stale)
        whole = {k: np.lib.format.open_memmap(os.path.join(path, k + ".npy"), mode="w+", dtype=dt_, shape=shp)
                 for k, dt_, shp in files}
    if world > 1:
        import torch.distributed as dist
        dist.barrier(group)                        # the files exist with their final size
    if rank != 0:
        whole = {k: np.lib.format.open_memmap(os.path.join(path, k + ".npy"), mode="r+") for k, _, _ in files}
        for k, dt_, shp in files:
            if whole[k].shape != tuple(shp) or whole[k].dtype != np.dtype(dt_):
                raise RuntimeError(f"{path}/{k}.npy is {whole[k].shape} {whole[k].dtype}, expected {tuple(shp)} {np.dtype(dt_)}")
    return whole


def _run_pipeline(nchunks, upload, launch, download, ahead=None):
    """The double-buffered schedule generate_lut and retrieve_stream share.  Chunk i lives in buffer i % 2; ``upload(i)`` and
    ``launch(i)`` are called on this thread, ``download(i)`` on ONE helper thread (so that it overlaps the next upload; torch
    releases the GIL inside the copies) and must return only when buffer i % 2 may be overwritten; ``ahead(i)`` is called
    before chunk i + 1 is touched (generate_lut pre-faults its destination pages there).  The order per chunk i:
    upload(i + 1) beside the kernels of chunk i, the download of chunk i - 1 awaited, launch(i + 1), download(i) submitted."""
    from concurrent.futures import ThreadPoolExecutor
    fut = [None, None]
    with ThreadPoolExecutor(1) as pool:
        if nchunks:
            upload(0)
            launch(0)
        for i in range(nchunks):
            if ahead is not None:
                ahead(i)
            if i + 1 < nchunks:
                upload(i + 1)                                  # overlaps the kernels of chunk i
                if fut[(i + 1) % 2] is not None:
                    fut[(i + 1) % 2].result()                  # the output buffer (i+1) % 2 has been drained (chunk i-1)
                launch(i + 1)
            fut[i % 2] = pool.submit(download, i)              # overlaps the kernels of chunk i+1
        for f in fut:
            if f is not None:
                f.result()


def generate_lut(params, sensor, path=None, dtype="float32", chunk=1 << 18, device=None, prune=True, fault_threads=8,
                 f32_bands=False, shard=False, group=None, out=None, sensor_info=None, band_model="centre"):
    """params: (B, 27) array-like on the HOST (numpy / memmap).  Returns dict of host arrays (np.memmap when
    ``path`` is given).

    ``shard=True`` under an initialised torch.distributed process group (one process per GPU): the table is cut into
    contiguous blocks of ceil(B / world) rows (sharding.shard_bounds) and every rank evaluates ITS block on its own device
    and writes it at its own rows -- with ``path``, straight into the directory's R_TOC.npy / R_TOA.npy / L_TOA.npy /
    params.npy (rank 0 creates the files, the other ranks open them read-write after ONE barrier; a second barrier, then rank
    0 writes meta.json).  No result ever crosses ranks: there is no collective on the data path, and the directory is
    byte-identical to a single-process run.  Without ``path`` every rank gets the arrays of its own block (LutBlock.rows).

    ``prune=True`` (default: a LUT holds the sensor columns only) evaluates just the <= 2 nb bands those columns
    depend on -- bit-identical columns; ``prune=False`` also evaluates the other bands of every spectrum (band sums);
    ``dtype="float64", f32_bands=True`` gives float64 columns identical to the float64 mode's at the float32 mode's speed.
    ``sensor_info``: a reference-style sensorinfo dict (wl_smac, SMAC_coef, wl_srf_smac, p_srf_smac, optional band_id_smac;
    up to 2162 bands, e.g. a hyperspectral imager) instead of a packaged sensor: the engine is then
    get_engine(sensor, device, sensor_info=sensor_info), and meta.json records ``sensor`` as given with that dict's bands and
    centres.
    ``band_model``: "centre" (default: the canopy spectra sampled at the band centre, like the reference) or "srf": the
    columns R_TOC / R_TOA / L_TOA hold the SRF-convolved values (Engine.run's R_TOC_srf ...; the band's spectral response
    function applied to the canopy spectra); meta.json records it.  ValueError for a sensor whose SRF columns are not in the
    order of its band centres (packaged MODIS, OLCI): pass ``sensor_info=spart_amd.align_srf(load_sensor_info(sensor))``.
    The C ABI always writes the centre columns, so "srf" costs one more (3, chunk, nb) device block that receives them and is
    never downloaded: their kernel time and stores are spent for nothing in this mode.
    ``out``: optional dict of caller-owned host arrays for the three columns (this rank's rows), e.g. a previous call's result:
    their pages are already resident.  Fresh arrays cost 1.25 GB of first-touch page faults per 8M spectra even with the helper
    threads -- 8M pruned: 57 ms fresh, 40 ms reused (2.0e8 spectra/s; the two PCIe directions alone need 33 ms);
    transparent huge pages made it worse on the test box (madvise mode with direct compaction: 71 ms), so the arrays are ordinary.

    Pipeline per chunk i (three HIP streams; the host never holds a private staging copy):
        upload(i+1)   H2D of the next (n, 27) rows straight from the caller's table + on-device transpose to the
                      structure-of-arrays layout the kernels read          -- overlaps the kernels of chunk i
        launch(i+1)   queued behind chunk i on the compute stream
        download(i)   D2H of the three (n, nb) column blocks straight into the destination arrays / memmaps
                                                                            -- overlaps the kernels of chunk i+1
        prefault(i+2) ``fault_threads`` helper threads make the destination pages of chunk i+2 resident (see _prefault)
    ``chunk`` = 262 144 rows by default: the pipeline's fill (first upload) and drain (last download) are not overlapped
    with anything, so smaller chunks waste less (8M spectra, all bands: 112 ms with 1M-row chunks, 105 ms with 256k; below
    that the per-chunk launch / copy overheads win).
    The copies block the HOST thread (pageable memory) but not the GPU, which stays busy as long as the two copies
    of a chunk (372 B per spectrum, ~7 ms per 1M at PCIe Gen5 rates) take less than its kernels (12 ms per 1M)."""
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from .sharding import shard_bounds
    P = np.asarray(params) if not isinstance(params, np.memmap) else params
    if P.ndim != 2 or P.shape[1] != workloads.NPARAM:
        raise ValueError("params must be (B, 27)")
    Btot = P.shape[0]
    world, rank = _group_info(shard, group)
    lo0, hi0 = shard_bounds(Btot, world, rank)
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    nb = eng.nb
    srf = _band_model(band_model, eng)
    npdt = _np_dtype(dtype)
    tdt = _torch_dtype(npdt)
    if path is not None and out is not None:
        raise ValueError("generate_lut: give `path` (results land in the directory's .npy files) or `out` (caller-owned arrays), not both")
    if path is not None:
        whole = open_lut_files(path, [(k, npdt, (Btot, nb)) for k in COLUMNS] + [("params", np.float64, tuple(P.shape))],
                               world, rank, group)
        full_out = {k: whole[k] for k in COLUMNS}
        out = {k: whole[k][lo0:hi0] for k in COLUMNS}          # this rank's rows of the shared files
        pm = whole["params"][lo0:hi0]
    else:
        full_out = None
        if out is not None:                                    # caller-owned destination (reused between tables: its pages are resident)
            out = _check_out(out, {k: ((int(hi0 - lo0), int(nb)), npdt) for k in COLUMNS})
        else:
            out = {k: np.empty((hi0 - lo0, nb), dtype=npdt) for k in COLUMNS}
        pm = None
    P = P[lo0:hi0]
    B = hi0 - lo0
    chunk = int(max(1, min(chunk, max(B, 1))))
    dev = eng.device
    compute = torch.cuda.current_stream(dev)
    h2d, d2h = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    drow = [torch.empty((chunk, workloads.NPARAM), dtype=torch.float64, device=dev) for _ in range(2)]   # as on the host
    dsoa = [torch.empty((workloads.NPARAM, chunk), dtype=torch.float64, device=dev) for _ in range(2)]   # kernel layout
    dout = [torch.empty((3, chunk, nb), dtype=tdt, device=dev) for _ in range(2)]
    dctr = torch.empty((3, chunk, nb), dtype=tdt, device=dev) if srf else None     # band_model="srf": the centre columns, not kept
    ev_in = [torch.cuda.Event() for _ in range(2)]
    ev_done = [torch.cuda.Event() for _ in range(2)]
    nchunks = (B + chunk - 1) // chunk
    keep = [None, None]         # host source of the upload in flight on buffer j (a temporary when P needed converting)

    def bounds(i):
        lo = i * chunk
        return lo, min(chunk, B - lo)

    def upload(i):
        j = i % 2
        lo, n = bounds(i)
        src = P[lo:lo + n]
        if src.dtype != np.float64 or not src.flags.c_contiguous:
            src = np.ascontiguousarray(src, dtype=np.float64)
        with torch.cuda.stream(h2d):
            if i >= 2:
                h2d.wait_event(ev_done[j])                         # dsoa[j] is free once chunk i-2's kernels ran
            keep[j] = src
            drow[j][:n].copy_(_host_tensor(src), non_blocking=True)
            dsoa[j][:, :n].copy_(drow[j][:n].t())                  # -> structure of arrays (27, n)
            ev_in[j].record(h2d)
        if pm is not None:
            pm[lo:lo + n] = src

    def launch(i):
        j = i % 2
        lo, n = bounds(i)
        compute.wait_event(ev_in[j])
        res = dout[j][:, :n]
        Pd = dsoa[j] if n == chunk else dsoa[j][:, :n].contiguous()
        if srf:
            eng.run(Pd, dtype, out={**{k: dctr[q, :n] for q, k in enumerate(COLUMNS)}, **{k: res[q] for q, k in enumerate(_SRF_COLUMNS)}},
                    materialize=_SRF_COLUMNS, prune=prune, f32_bands=f32_bands)
        else:
            eng.run(Pd, dtype, out={"R_TOC": res[0], "R_TOA": res[1], "L_TOA": res[2]}, prune=prune, f32_bands=f32_bands)
        ev_done[j].record(compute)

    fault_threads = max(0, int(fault_threads))
    fpool = ThreadPoolExecutor(fault_threads) if fault_threads else None
    faults = {}                                                    # chunk -> futures of its prefault tasks

    def prefault(i):
        if fpool is None or i >= nchunks or i in faults:
            return
        lo, n = bounds(i)
        dests = [out[k][lo:lo + n] for k in COLUMNS] + ([pm[lo:lo + n]] if pm is not None else [])
        per = max(1, -(-n // max(1, fault_threads // len(dests))))
        faults[i] = [fpool.submit(_prefault, d[r:r + per]) for d in dests for r in range(0, n, per)]

    def download(i):                                               # runs on the helper thread
        j = i % 2
        lo, n = bounds(i)
        for f in faults.pop(i, ()):
            try:
                f.result()                                         # the destination pages of this chunk are resident
            except Exception:       # noqa: BLE001  ("not pre-faulted": the copy below faults the pages in itself)
                pass
        with torch.cuda.device(dev), torch.cuda.stream(d2h):
            d2h.wait_event(ev_done[j])
            for q, k in enumerate(COLUMNS):
                _host_tensor(out[k][lo:lo + n]).copy_(dout[j][q, :n], non_blocking=True)
            d2h.synchronize()                                      # dout[j] may be overwritten by chunk i+2

    # downloads (which also take the first-touch page faults of the destination) run on the pipeline's helper thread so
    # that they overlap the uploads issued by this thread
    try:
        prefault(0)
        prefault(1)
        _run_pipeline(nchunks, upload, launch, download, ahead=lambda i: prefault(i + 2))
    finally:                                                       # also on an exception in upload / launch / download
        if fpool is not None:
            fpool.shutdown(wait=True, cancel_futures=True)
    if path is not None:
        for a in whole.values():
            a.flush()
        if world > 1:
            import torch.distributed as dist
            dist.barrier(group)                    # every rank's rows are in the files
        if rank == 0:
            meta = {"sensor": sensor, "bands": [str(b) for b in eng.band_id], "wavelengths": [float(w) for w in eng.wl_smac],
                    "dtype": np.dtype(npdt).name, "rows": int(Btot), "param_names": workloads.PARAM_NAMES,
                    "columns": list(COLUMNS), "pruned": bool(prune), "band_model": band_model}
            with open(os.path.join(path, "meta.json"), "w") as f:
                json.dump(meta, f, indent=1)
    res = LutBlock(full_out if full_out is not None else out)
    res.rows, res.total = (int(lo0), int(hi0)), int(Btot)
    return res


def load_lut(path, mmap=True):
    """-> (meta dict, params, dict of columns), memory-mapped by default."""
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    mode = "r" if mmap else None
    cols = {k: np.load(os.path.join(path, k + ".npy"), mmap_mode=mode) for k in meta["columns"]}
    return meta, np.load(os.path.join(path, "params.npy"), mmap_mode=mode), cols


def invert_lut(lut, obs, column="R_TOC", weights=None, dtype=None, shard=False, group=None, device=None, stats=False, k=None):
    """Nearest LUT row per observed spectrum (spart_lut_nearest: exact argmin of the weighted squared distance, lowest index
    on ties) over a LUT directory written by generate_lut (``lut`` = its path) or an in-memory (B, nb) array.
    ``k`` = None: (idx (M,) int64 numpy, cost (M,) numpy).  An integer ``k`` (1 ... 256): the k nearest rows per observation
    (spart_lut_topk: ordered by cost, then row index; padded with (-1, +inf)) as (idx (M, k), cost (M, k)).

    ``shard=True`` under a process group: every rank searches ITS contiguous block of rows (read from the directory's memmap:
    only those rows are ever touched) and ONE all_gather of (cost, global row) per observation (and place) settles the
    result (sharding.lut_nearest_sharded / lut_topk_sharded); every rank returns the same arrays, equal bit for bit to the
    single-process search.  ``obs`` must then be the same on every rank.  ``shard=False`` never issues a collective, whether
    or not a process group is initialised: each process searches the whole table for its own ``obs``.

    ``weights``: None, (nb,) (one weight per band) or (M, nb): one weight row per observation (spart_lut_topk_obs_weights;
    a band of weight zero is skipped, so the observation may be NaN there -- noise_weights() builds such rows).  Under
    ``shard=True`` (M, nb) weights must, like ``obs``, be the same on every rank."""
    import torch
    from .sharding import lut_nearest_sharded, lut_topk_sharded, shard_bounds
    if isinstance(lut, (str, os.PathLike)):
        meta, _, cols = load_lut(lut)
        table = cols[column]
        dtype = dtype or meta["dtype"]
    else:
        table = lut
        dtype = dtype or ("float64" if np.asarray(lut[:1]).dtype == np.float64 else "float32")
    world, rank = _group_info(shard, group)
    lo, hi = shard_bounds(table.shape[0], world, rank)
    eng = get_engine(None, device)
    td = _torch_dtype(_np_dtype(dtype))
    local = torch.as_tensor(np.array(table[lo:hi])).to(device=eng.device, dtype=td)      # (a copy: memmaps opened read-only)
    o = torch.as_tensor(np.asarray(obs)).to(device=eng.device, dtype=td)
    info = {}

    def nearest(l, ob):
        r = eng.lut_nearest(l, ob, weights=weights, dtype=dtype, stats=stats)
        if stats:
            info.update(r[2])
        return r[0], r[1]

    def topk(l, ob, kk):
        r = eng.lut_topk(l, ob, kk, weights=weights, dtype=dtype, stats=stats)
        if stats:
            info.update(r[2])
        return r[0], r[1]
    if world > 1:
        import torch.distributed as dist
        comm = "cpu" if dist.get_backend(group) != "nccl" else None   # gloo moves host tensors: the winners travel through the host
        if k is None:
            idx, cost = lut_nearest_sharded(local, lo, o, nearest, group, comm_device=comm)
        else:
            idx, cost = lut_topk_sharded(local, lo, o, int(k), topk, group, comm_device=comm)
    else:                                              # one process, the whole table: no collective, whatever is initialised
        M = o.shape[0]
        shape = (M,) if k is None else (M, int(k))
        if local.shape[0] > 0 and M > 0:
            idx, cost = nearest(local, o) if k is None else topk(local, o, int(k))
        else:
            if k is not None:
                _check_k(k)
            idx = torch.full(shape, -1, dtype=torch.int64)
            cost = torch.full(shape, float("inf"), dtype=td)
    out = (idx.cpu().numpy(), cost.cpu().numpy())
    return out + (dict(info, rows=(lo, hi)),) if stats else out


def noise_weights(obs, abs_sigma=0.0, rel_sigma=0.0):
    """Per-observation weights of the usual noise model for invert_lut / retrieve / Engine.lut_topk: sigma_mj^2 =
    abs_sigma_j^2 + (rel_sigma * obs_mj)^2, weight 1 / sigma_mj^2, and weight 0 -- a masked band -- wherever obs is not finite
    (saturated, flagged or missing bands marked with NaN).  ``abs_sigma`` is a scalar or (nb,); ``rel_sigma`` a scalar.
    -> (M, nb) float64.  A band whose sigma is exactly 0 gets weight +inf, which the search refuses: give abs_sigma > 0
    when an observation can be exactly 0."""
    o = np.asarray(obs, dtype=np.float64)
    if o.ndim != 2:
        raise ValueError(f"obs must be (M, nb), got shape {o.shape}")
    a = np.asarray(abs_sigma, dtype=np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != o.shape[1]):
        raise ValueError(f"abs_sigma must be a scalar or ({o.shape[1]},), got shape {a.shape}")
    r = float(rel_sigma)
    if not (np.all(a >= 0) and r >= 0):
        raise ValueError("abs_sigma and rel_sigma must be >= 0")
    if not (np.any(a > 0) or r > 0):
        raise ValueError("noise_weights needs abs_sigma or rel_sigma > 0")
    ok = np.isfinite(o)
    with np.errstate(divide="ignore"):
        w = 1.0 / (a * a + (r * np.where(ok, o, 0.0)) ** 2)
    return np.where(ok, w, 0.0)


def summarise_rows(params, idx, block_rows=1 << 18):
    """mean / median / std (numpy's, ddof = 0) of the parameter rows ``params[idx[m]]`` per observation, padding (-1)
    excluded: params (B, P) array or memmap, idx (M, k) int64 -> three (M, P) float64 arrays (NaN where an observation has no
    row).  Works in blocks of observations of about ``block_rows`` gathered rows, reading only the rows it needs, so that the
    host never holds an (M * k, P) copy."""
    idx = np.asarray(idx)
    M, k = idx.shape
    P = params.shape[1]
    res = [np.full((M, P), np.nan) for _ in range(3)]
    mb = max(1, int(block_rows) // max(k, 1))
    for m0 in range(0, M, mb):
        ii = idx[m0:m0 + mb]
        ok = ii >= 0
        if not ok.any():
            continue
        rows, inv = np.unique(ii[ok], return_inverse=True)
        vals = np.asarray(params[rows], dtype=np.float64)            # sorted unique rows: a memmap reads only those
        g = np.full(ii.shape + (P,), np.nan)
        g[ok] = vals[inv]
        full = ok.all(axis=1)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # all-padding observations stay NaN
            for r, f in zip(res, (np.nanmean, np.nanmedian, np.nanstd)):
                r[m0:m0 + mb] = f(g, axis=1)
            if full.any():                                          # the common case: numpy's own mean / median / std
                gf = g[full]
                for r, f in zip(res, (np.mean, np.median, np.std)):
                    r[m0:m0 + mb][full] = f(gf, axis=1)
    return res


SUMMARIES = ("host", "device")
STREAM_MAPS = ("mean", "median", "std")            # the (M, P) float64 arrays of retrieve_stream, then count and best_cost


def _param_columns(params_cols):
    """params_cols (None = every parameter, or a list of names from workloads.PARAM_NAMES and PRODUCT_NAMES) -> (names, column
    numbers): the parameter names in the order given, then the product names in the order given; a product's column number
    is NPARAM + its place in PRODUCT_NAMES, its column of the stacked table (_summary_table)"""
    if params_cols is None:
        return list(workloads.PARAM_NAMES), list(range(workloads.NPARAM))
    given = list(params_cols)
    unknown = [n for n in given if n not in workloads.PARAM_NAMES and n not in PRODUCT_NAMES]
    if unknown or not given:
        raise ValueError(f"params_cols: unknown parameter name(s) {unknown}; expected names from {list(workloads.PARAM_NAMES)} "
                         f"or, for a LUT with products.npy (lut_products), {list(PRODUCT_NAMES)}")
    names = [n for n in given if n in workloads.PARAM_NAMES] + [n for n in given if n in PRODUCT_NAMES]
    return names, [workloads.PARAM_NAMES.index(n) if n in workloads.PARAM_NAMES else workloads.NPARAM + PRODUCT_NAMES.index(n)
                   for n in names]


class _Stacked:
    """params.npy (B, 27) and products.npy (B, 5) read as ONE (B, 32) table, the parameter columns first: rows are gathered
    from both files (memmaps read only the rows asked for), np.asarray gives the whole table"""

    def __init__(self, params, products):
        if products.shape != (params.shape[0], len(PRODUCT_NAMES)):
            raise ValueError(f"products.npy is {products.shape}, params.npy {params.shape}: run lut_products again")
        self.params, self.products = params, products
        self.shape = (params.shape[0], params.shape[1] + products.shape[1])

    def __getitem__(self, rows):
        return np.concatenate([np.asarray(self.params[rows], dtype=np.float64), np.asarray(self.products[rows], dtype=np.float64)], axis=1)

    def __array__(self, dtype=None, copy=None):
        return self[slice(None)]


def _needs_products(lut_dir, cols):
    """ValueError when ``cols`` names a product column and the LUT directory has no products.npy; before any search"""
    if max(cols, default=0) >= workloads.NPARAM and not os.path.exists(os.path.join(lut_dir, "products.npy")):
        raise ValueError(f"params_cols names a product ({list(PRODUCT_NAMES)}) but {lut_dir} has no products.npy: "
                         "run spart_amd.lut_products(lut_dir) first")


def _summary_table(lut_dir, params, cols):
    """the table ``cols`` index: params.npy itself while only parameters are chosen, else params.npy | products.npy"""
    if max(cols, default=0) < workloads.NPARAM:
        return params
    _needs_products(lut_dir, cols)
    return _Stacked(params, np.load(os.path.join(lut_dir, "products.npy"), mmap_mode="r"))


def products(params_host, names=None, device=None):
    """The host form of Engine.products: numpy in and out.  ``params_host``: a (27, B) array or a list of 27 scalars / arrays
    (workloads.PARAM_NAMES order; the atmosphere and DOY entries are not read and may be None); ``names``: some of
    PRODUCT_NAMES in the order wanted (None = all five).  -> dict {name: (B,) float64 array}.  No sensor is involved.
    Every argument check that needs no device runs before one is asked for."""
    names = product_names(names)
    cols = products_columns(params_host if isinstance(params_host, (list, tuple)) else np.asarray(params_host, dtype=np.float64))
    eng = get_engine(None, device)
    padded = cols + [None] * (workloads.NPARAM - len(cols)) if isinstance(cols, list) else cols
    return {n: v.cpu().numpy() for n, v in eng.products(padded, names).items()}


def lut_products(lut_dir, chunk=1 << 18, device=None, shard=False, group=None):
    """Give an existing generate_lut directory its product columns: params.npy is read in chunks of ``chunk`` rows, every row
    goes through Engine.products (spart_products), and the directory gains products.npy (rows, 5) float64 in PRODUCT_NAMES
    order; meta.json gains ``"product_names"`` and keeps every other key.  retrieve / retrieve_stream then take product names
    in ``params_cols``: the k nearest rows, or the posterior weights, average the product itself.  The values do not depend
    on ``chunk`` (a row's products are the same bits in any batch).  No sensor engine is needed.  ``shard=True`` under a
    process group of more than one rank is a ValueError (sharded products are not built).  -> the (rows, 5) array."""
    if _group_info(shard, group)[0] > 1:
        raise ValueError("lut_products does not take shard=True under a process group of more than one rank: "
                         "run it on one rank after generate_lut")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk}, expected >= 1")
    with open(os.path.join(lut_dir, "meta.json")) as f:
        meta = json.load(f)
    params = np.load(os.path.join(lut_dir, "params.npy"), mmap_mode="r")
    B = params.shape[0]
    out = np.empty((B, len(PRODUCT_NAMES)), dtype=np.float64)
    if B > 0:
        import torch
        eng = get_engine(None, device)
        for lo in range(0, B, chunk):
            block = torch.as_tensor(np.ascontiguousarray(np.array(params[lo:lo + chunk], dtype=np.float64).T))    # (a copy: the memmap is read-only)
            res = eng.products(block)
            for j, n in enumerate(PRODUCT_NAMES):
                out[lo:lo + chunk, j] = res[n].cpu().numpy()
    tmp = os.path.join(lut_dir, f"products.npy.tmp.{os.getpid()}")
    with open(tmp, "wb") as f:
        np.save(f, out)
    os.replace(tmp, os.path.join(lut_dir, "products.npy"))
    meta["product_names"] = list(PRODUCT_NAMES)
    with open(os.path.join(lut_dir, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return out


def refine(params, obs, sensor, free, bounds=None, weights=None, column="R_TOC", n_iter=10, rel_step=1e-3, lambda0=1e-2,
           lidf="literal", nlayers=None, sensor_info=None, device=None, prior=None, prior_mean=None, prior_weight=None,
           band_model="centre"):
    """The host form of Engine.refine: numpy in and out.  ``params`` (27, M) or a list of 27 scalars / arrays (run()'s
    conventions), ``obs`` (M, nb), ``sensor`` a packaged sensor name (or None with ``sensor_info``, a sensorinfo dict);
    ``prior`` or ``prior_mean`` / ``prior_weight`` and ``band_model`` as for Engine.refine.
    -> dict of numpy arrays x, cost, cost0, std, n_accept, y and the list ``names``.  Every argument check that needs no
    device runs before one is asked for."""
    plan, params = refine_args(params, obs, free, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior, prior_mean,
                               prior_weight, band_model)[:2]
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.refine(params, np.asarray(obs, dtype=np.float64), free, weights=weights, lidf=lidf, nlayers=nlayers,
                     prior_mean=prior_mean, prior_weight=prior_weight, band_model=band_model, _plan=plan)
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def refine_leaf(leaf, refl=None, tran=None, free=("Cab", "Cw", "Cdm", "N"), bounds=None, weights_refl=None, weights_tran=None,
                n_iter=20, rel_step=1e-3, lambda0=1e-2, prior=None, prior_mean=None, prior_weight=None, spectra=False, device=None):
    """The host form of Engine.refine_leaf (PROSPECT inversion of measured leaf spectra): numpy in and out.  ``leaf``: the
    start rows, a (9, M) array, a list of nine scalars / arrays, or a LeafBiology whose fields are scalars or arrays; ``refl``,
    ``tran`` (M, 2001), either may be None; everything else as for Engine.refine_leaf.  No sensor is involved.
    -> dict of numpy arrays x, std, cost, cost0, n_accept (and y_refl, y_tran with ``spectra``) and the list ``names``.  Every
    argument check that needs no device runs before one is asked for."""
    if hasattr(leaf, "columns") and callable(leaf.columns):
        leaf = [np.asarray(c, dtype=np.float64) for c in leaf.columns()]
    plan, leaf = refine_leaf_args(leaf, refl, tran, free, bounds, weights_refl, weights_tran, n_iter, rel_step, lambda0, prior,
                                  prior_mean, prior_weight)[:2]
    eng = get_engine(None, device)
    host = lambda v: None if v is None else np.asarray(v, dtype=np.float64)      # noqa: E731
    res = eng.refine_leaf(leaf, host(refl), host(tran), free, bounds=bounds, weights_refl=weights_refl, weights_tran=weights_tran,
                          n_iter=n_iter, rel_step=rel_step, lambda0=lambda0, prior=prior, prior_mean=prior_mean,
                          prior_weight=prior_weight, spectra=spectra)
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def posterior(params, obs, sensor, free, bounds=None, weights=None, column="R_TOC", rel_step=1e-3, lidf="literal", nlayers=None,
              sensor_info=None, device=None, prior=None, prior_mean=None, prior_weight=None, band_model="centre"):
    """The host form of Engine.posterior: numpy in and out.  ``params``, ``sensor`` / ``sensor_info`` as for refine(); ``obs``
    (M, nb) or None.  -> dict of numpy arrays x, y, jac, cov, ak, std, dfs, cost, nband, status, corr and the list ``names``.
    Every argument check that needs no device runs before one is asked for."""
    shape_of = obs
    if obs is None:
        nb = 1 if weights is None else int(np.shape(weights)[-1]) if np.ndim(weights) else 1
        shape_of = np.broadcast_to(np.float64(0.0), (params_rows(params), nb))
    plan, params = refine_args(params, shape_of, free, bounds, weights, column, 0, rel_step, 1e-2, lidf, prior, prior_mean,
                               prior_weight, band_model)[:2]
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.posterior(params, None if obs is None else np.asarray(obs, dtype=np.float64), free, weights=weights, lidf=lidf,
                        nlayers=nlayers, prior_mean=prior_mean, prior_weight=prior_weight, band_model=band_model, _plan=plan)
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def sobol(params, sensor, free, N=4096, bounds=None, design=None, seed=0, column="R_TOC", band_model="centre", lidf="literal",
          nlayers=None, sensor_info=None, device=None):
    """The host form of Engine.sobol: numpy in and out.  ``params`` (27, M) or a list of 27 scalars / arrays, one column per
    site, ``sensor`` / ``sensor_info`` as for refine(); everything else as for Engine.sobol.  -> dict of numpy arrays mean, var
    (M, nb), S1, ST, S1_se, ST_se (M, nb, F) and the list ``names``.  Every argument check that needs no device runs before
    one is asked for."""
    params, _, N, uA, uB = sobol_args(params, free, N, bounds, design, seed, column, band_model, lidf)[1:]
    Engine._nlayers(nlayers)
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.sobol(params, free, N=N, bounds=bounds, design=(uA, uB), column=column, band_model=band_model, lidf=lidf, nlayers=nlayers)
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def sample(params, obs, sensor, free, bounds=None, weights=None, prior=None, walkers=None, n_steps=1000, burn=None, thin=1, seed=0,
           init=None, init_radius=None, step0=0, obs_offset=0, column="R_TOC", band_model="centre", chain=False, a=2.0,
           temperature=1.0, rel_init=0.01, prior_mean=None, prior_weight=None, lidf="literal", nlayers=None, sensor_info=None,
           device=None):
    """The host form of Engine.sample: numpy in and out.  ``params`` (27, M) or a list of 27 scalars / arrays, ``obs`` (M, nb),
    ``sensor`` / ``sensor_info`` as for refine(); everything else as for Engine.sample.  -> dict of numpy arrays mean, std, cov,
    best, best_cost, accept_fraction, status, last, last_cost (chain, chain_cost with chain=True) and the list ``names``.  Every
    argument check that needs no device runs before one is asked for."""
    init, init_radius = (None if v is None else np.asarray(v, dtype=np.float64) for v in (init, init_radius))
    sample_args(params, obs, free, bounds, weights, prior, prior_mean, prior_weight, walkers, n_steps, burn, thin, a, temperature,
                rel_init, init, init_radius, step0, obs_offset, seed, column, band_model, lidf)
    Engine._nlayers(nlayers)
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.sample(params, obs, free, bounds=bounds, weights=weights, prior=prior, walkers=walkers, n_steps=n_steps, burn=burn,
                     thin=thin, seed=seed, init=init, init_radius=init_radius, step0=step0, obs_offset=obs_offset, column=column,
                     band_model=band_model, chain=chain, a=a, temperature=temperature, rel_init=rel_init, prior_mean=prior_mean,
                     prior_weight=prior_weight, lidf=lidf, nlayers=nlayers)
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def jacobian(params, sensor, free, bounds=None, column="R_TOC", rel_step=1e-3, lidf="literal", nlayers=None, sensor_info=None,
             device=None, band_model="centre"):
    """The host form of Engine.jacobian: -> dict of numpy arrays y (M, nb), jac (M, nb, F) and the list ``names``"""
    plan, params = refine_args(params, np.broadcast_to(np.float64(0.0), (params_rows(params), 1)), free, bounds, None, column, 0,
                               rel_step, 1e-2, lidf, None, None, None, band_model)[:2]
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.posterior(params, None, free, lidf=lidf, nlayers=nlayers, band_model=band_model, _plan=plan, _outputs=("y", "jac"))
    return {"y": res["y"].cpu().numpy(), "jac": res["jac"].cpu().numpy(), "names": res["names"]}


def vjp(params, grad_outputs, sensor, free, bounds=None, rel_step=1e-3, lidf="literal", nlayers=None, sensor_info=None, device=None,
        band_model="centre"):
    """The host form of Engine.vjp: ``grad_outputs`` {column name: (M, nb) array} -> {"grad": (M, F) numpy array, "names"}.
    Every argument check that needs no device runs before one is asked for."""
    params = vjp_args(params, grad_outputs, free, bounds, rel_step, lidf, band_model)[1]
    Engine._nlayers(nlayers)
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.vjp(params, grad_outputs, free, bounds=bounds, rel_step=rel_step, lidf=lidf, nlayers=nlayers, band_model=band_model)
    return {"grad": res["grad"].cpu().numpy(), "names": res["names"]}


def refine_views(params, obs, sensor, shared, local=(), bounds=None, weights=None, column="R_TOC", n_iter=10, rel_step=1e-3,
                 lambda0=1e-2, lidf="literal", nlayers=None, sensor_info=None, device=None, prior=None, prior_mean=None,
                 prior_weight=None, band_model="centre"):
    """The host form of Engine.refine_views: numpy in and out.  ``params`` (27, V, M) or 27 entries each broadcastable to (V, M),
    ``obs`` (M, V, nb), ``sensor`` a packaged sensor name (or None with ``sensor_info``); everything else as for
    Engine.refine_views.  -> dict of numpy arrays x, std, cost, cost0, n_accept, y, shared, shared_std, local, local_std and the
    list ``names``.  Every argument check that needs no device runs before one is asked for.  A LUT search across views is
    another feature: retrieve / retrieve_stream do not call this."""
    params = refine_views_args(params, obs, shared, local, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior,
                               prior_mean, prior_weight, band_model)[1]
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.refine_views(params if isinstance(params, list) else eng.torch.as_tensor(params), np.asarray(obs, dtype=np.float64),
                           shared, local, bounds=bounds, weights=weights, column=column, n_iter=n_iter, rel_step=rel_step,
                           lambda0=lambda0, lidf=lidf, nlayers=nlayers, prior=prior, prior_mean=prior_mean,
                           prior_weight=prior_weight, band_model=band_model)
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def refine_mix(params, obs, sensor, shared=(), local=(), active=None, fractions=None, fit_fractions=True, fraction_bounds=(0, 1),
               bounds=None, weights=None, column="R_TOC", n_iter=10, rel_step=1e-3, lambda0=1e-2, lidf="literal", nlayers=None,
               prior=None, band_model="centre", sensor_info=None, device=None):
    """The host form of Engine.refine_mix: numpy in and out.  ``params`` (27, V, M) or 27 entries each broadcastable to (V, M),
    ``obs`` (M, nb), ``sensor`` a packaged sensor name (or None with ``sensor_info``); everything else as for Engine.refine_mix.
    -> dict of numpy arrays x, std, cost, cost0, n_accept, y, y_comp, fractions, fractions_std, shared, shared_std, local,
    local_std and the list ``names``.  Every argument check that needs no device runs before one is asked for."""
    params = refine_mix_args(params, obs, shared, local, active, fractions, fit_fractions, fraction_bounds, bounds, weights, column,
                             n_iter, rel_step, lambda0, lidf, prior, band_model)[1]
    Engine._nlayers(nlayers)
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.refine_mix(params if isinstance(params, list) else eng.torch.as_tensor(params), np.asarray(obs, dtype=np.float64),
                         shared, local, active=active, fractions=fractions, fit_fractions=fit_fractions,
                         fraction_bounds=fraction_bounds, bounds=bounds, weights=weights, column=column, n_iter=n_iter,
                         rel_step=rel_step, lambda0=lambda0, lidf=lidf, nlayers=nlayers, prior=prior, band_model=band_model)
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def refine_tiles(params, obs, sensor, shared, local=(), tile_size=None, tile_start=None, bounds=None, weights=None, column="R_TOC",
                 n_iter=10, rel_step=1e-3, lambda0=1e-2, lidf="literal", nlayers=None, sensor_info=None, device=None, prior=None,
                 band_model="centre"):
    """The host form of Engine.refine_tiles: numpy in and out.  ``params`` (27, M) or a list of 27 scalars / arrays, ``obs``
    (M, nb), ``sensor`` a packaged sensor name (or None with ``sensor_info``); everything else as for Engine.refine_tiles.
    -> dict of numpy arrays shared, shared_std, local, local_std, cost, cost0, n_accept, pixel_cost, status, y, tile_start and
    the list ``names``.  Every argument check that needs no device runs before one is asked for."""
    params = refine_tiles_args(params, obs, shared, local, tile_size, tile_start, bounds, weights, column, n_iter, rel_step, lambda0,
                               lidf, prior, band_model)[1]
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.refine_tiles(params, np.asarray(obs, dtype=np.float64), shared, local, tile_size=tile_size, tile_start=tile_start,
                           bounds=bounds, weights=weights, column=column, n_iter=n_iter, rel_step=rel_step, lambda0=lambda0,
                           lidf=lidf, nlayers=nlayers, prior=prior, band_model=band_model)
    return {k: (v if k in ("names", "tile_start") else v.cpu().numpy()) for k, v in res.items()}


def refine_series(params, obs, sensor, shared=(), local=(), n_dates=None, series_start=None, smooth=None, link=None, bounds=None,
                  weights=None, column="R_TOC", n_iter=10, rel_step=1e-3, lambda0=1e-2, lidf="literal", nlayers=None, sensor_info=None,
                  device=None, prior=None, band_model="centre"):
    """The host form of Engine.refine_series: numpy in and out.  ``params`` (27, M) or a list of 27 scalars / arrays, one column
    per date, ``obs`` (M, nb), ``sensor`` a packaged sensor name (or None with ``sensor_info``); everything else as for
    Engine.refine_series.  -> dict of numpy arrays (refine_tiles' keys, ``series_start`` in place of ``tile_start``) and the list
    ``names``.  Every argument check that needs no device runs before one is asked for."""
    params = refine_series_args(params, obs, shared, local, n_dates, series_start, smooth, link, bounds, weights, column, n_iter,
                                rel_step, lambda0, lidf, prior, band_model)[1]
    eng = get_engine(sensor, device, sensor_info=sensor_info)
    res = eng.refine_series(params, np.asarray(obs, dtype=np.float64), shared, local, n_dates=n_dates, series_start=series_start,
                            smooth=smooth, link=link, bounds=bounds, weights=weights, column=column, n_iter=n_iter, rel_step=rel_step,
                            lambda0=lambda0, lidf=lidf, nlayers=nlayers, prior=prior, band_model=band_model)
    return {k: (v if k in ("names", "series_start") else v.cpu().numpy()) for k, v in res.items()}


def date_links(days, series_start, power=1):
    """The ``link`` of refine_series from acquisition days: ``days`` (M,) increasing within every series, ``series_start``
    (S + 1,) -> (M,) float64 with 1 / dt^power at row m for dt = days[m + 1] - days[m], and 0 at each series' last row.
    Days that do not increase within a series are a ValueError."""
    days = np.asarray(days, dtype=np.float64)
    ts = np.asarray(series_start, dtype=np.int64)
    if days.ndim != 1 or ts.ndim != 1 or ts.size < 1 or ts[0] != 0 or ts[-1] != days.size or (np.diff(ts) < 1).any():
        raise ValueError(f"days {days.shape} and series_start {ts.tolist() if ts.ndim == 1 else ts.shape}: (M,) and 0 = s_0 < ... < s_S = M expected")
    link = np.zeros(days.size)
    if days.size:
        inner = np.ones(days.size, dtype=bool)
        inner[ts[1:] - 1] = False
        dt = np.diff(days, append=days[-1])
        if not (dt[inner] > 0.0).all():
            m = int(np.flatnonzero(inner & ~(dt > 0.0))[0])
            raise ValueError(f"days must increase within a series: days[{m + 1}] = {days[m + 1]} after {days[m]}")
        link[inner] = 1.0 / dt[inner] ** power
    return link


def tiles_from_labels(labels):
    """Tiles for an object-based inversion: ``labels`` (M,), one label per pixel (a field, a segment) -> (order, tile_start):
    ``order`` (M,) int64 sorts the pixels by label, stably, so that pixels of one label are contiguous and keep their order;
    tile t is order[tile_start[t]:tile_start[t + 1]].  Pass params[:, order], obs[order] to refine_tiles and scatter the pixel
    outputs back with out[order] = res[...].  A label of more than 4096 pixels is for the caller to split."""
    labels = np.asarray(labels)
    if labels.ndim != 1:
        raise ValueError(f"labels has shape {labels.shape}, expected (M,)")
    order = np.argsort(labels, kind="stable").astype(np.int64)
    srt = labels[order]
    cut = np.flatnonzero(srt[1:] != srt[:-1]) + 1 if labels.size else np.zeros(0, dtype=np.int64)
    return order, np.concatenate([[0], cut, [labels.size]]).astype(np.int64) if labels.size else np.zeros(1, dtype=np.int64)


def window_tiles(height, width, win):
    """Tiles for one atmosphere per window: square windows of ``win`` x ``win`` pixels over a (height, width) raster in
    row-major pixel order, the windows at the right and bottom edges smaller -> (order, tile_start) as tiles_from_labels gives
    them (windows in row-major order, the pixels of a window in row-major order)."""
    for what, v in (("height", height), ("width", width), ("win", win)):
        if isinstance(v, bool) or int(v) != v or int(v) < (1 if what == "win" else 0):
            raise ValueError(f"{what} = {v!r}, expected an integer >= {1 if what == 'win' else 0}")
    height, width, win = int(height), int(width), int(win)
    if win * win > _lib.TILES_MAXG:
        raise ValueError(f"win = {win}: a window of {win * win} pixels, at most {_lib.TILES_MAXG} fit a tile")
    r, c = np.divmod(np.arange(height * width, dtype=np.int64), max(width, 1))
    return tiles_from_labels((r // win) * ((width + win - 1) // win) + c // win)


REFINE_OPTS = ("bounds", "n_iter", "rel_step", "lambda0", "lidf", "nlayers", "prior", "prior_floor", "band_model",
               "posterior")
REFINE_KEYS = {"refined": "x", "refined_std": "std", "refined_cost": "cost", "refined_cost0": "cost0", "refined_accepts": "n_accept"}
POSTERIOR_KEYS = {"refined_cov": "cov", "refined_ak": "ak", "refined_dfs": "dfs"}      # refine_opts={"posterior": True}


def _refine_setup(lut_dir, refine, refine_opts, shard, group, sensor_info):
    """retrieve(refine=...): everything that can be refused from the LUT directory alone -> (plan, options, sensor, sensor_info).
    options["band_model"] is then set: the fit's band model, which must be the LUT's.  It is never taken from meta.json
    silently: an SRF iteration evaluates the whole SRF support of every band (968 model bands per row for Sentinel-2A, 13 for
    the centre model), so the caller says so."""
    opts = dict(refine_opts or {})
    stray = [n for n in opts if n not in REFINE_OPTS]
    if stray:
        raise ValueError(f"refine_opts: unknown option(s) {stray}; expected some of {REFINE_OPTS}")
    if refine is None:
        if opts:
            raise ValueError("refine_opts without refine=[names]")
        return None
    meta, params, _ = load_lut(lut_dir)
    have, want = meta.get("band_model", "centre"), opts.setdefault("band_model", "centre")
    if want not in BAND_MODELS:
        raise ValueError(f'refine_opts["band_model"] = {want!r}, expected "centre" or "srf"')
    if want != have:
        raise ValueError(f'retrieve(refine=...): the LUT holds band_model="{have}" columns and the fit was asked for "{want}"; the '
                         f'fit uses the band model the LUT was generated with: pass refine_opts={{"band_model": "{have}"}}'
                         + (" (an srf iteration evaluates the whole SRF support of every band)" if have == "srf" else ""))
    if _group_info(shard, group)[0] > 1:
        raise ValueError("retrieve(refine=...) does not take shard=True under a process group of more than one rank "
                         "(sharded refinement is not built yet)")
    if sensor_info is None and not isinstance(meta.get("sensor"), str):
        raise ValueError("retrieve(refine=...): meta.json names no packaged sensor; pass the LUT's sensor_info=")
    names, cols = _param_columns(list(refine))
    if not isinstance(opts.get("posterior", False), (bool, np.bool_)):
        raise ValueError(f'refine_opts["posterior"] = {opts["posterior"]!r}, expected True or False')
    prior = opts.get("prior")
    if not (prior is None or isinstance(prior, dict) or (isinstance(prior, str) and prior == "knn")):
        raise ValueError(f'refine_opts["prior"] = {prior!r}, expected a dict {{name: (mean, sigma)}} or "knn"')
    if "prior_floor" in opts:
        if not (isinstance(prior, str) and prior == "knn"):
            raise ValueError('refine_opts["prior_floor"] goes with "prior": "knn"')
        knn_prior(np.zeros((0, 1)), np.zeros((0, 1)), [0.0], [1.0], floor=opts["prior_floor"])      # (its own check of floor)
    P = np.asarray(params)
    ranges = {}
    for n, c in zip(names, cols):                     # the LUT's own extent of every free column
        lo, hi = (float(P[:, c].min()), float(P[:, c].max())) if P.shape[0] else (np.nan, np.nan)
        if lo < hi:
            ranges[n] = (lo, hi)
        elif n not in (opts.get("bounds") or {}):
            raise ValueError(f"retrieve(refine=...): column {n!r} is constant in the LUT ({lo}); give refine_opts="
                             f"{{'bounds': {{{n!r}: (lo, hi)}}}} or leave it out")
    plan = refine_plan(names, opts.get("bounds"), opts.get("n_iter", 10), "R_TOC", opts.get("rel_step", 1e-3),
                       opts.get("lambda0", 1e-2), default_ranges=ranges, prior=prior if isinstance(prior, dict) else None)
    return plan, opts, meta.get("sensor"), sensor_info


BAYES_OPTS = ("cut", "temperature", "quantiles")
BAYES_KEYS = {"bayes_mean": "mean", "bayes_std": "std", "bayes_ess": "ess", "bayes_sum_w": "sum_w", "bayes_count": "count"}


def _bayes_setup(bayes, shard=False, group=None):
    """retrieve(bayes=...): None, or a dict with some of BAYES_OPTS -> None or Engine.lut_bayes' keyword arguments, checked"""
    if bayes is None:
        return None
    if not isinstance(bayes, dict):
        raise ValueError(f"bayes = {bayes!r}, expected a dict with some of {BAYES_OPTS}")
    stray = [n for n in bayes if n not in BAYES_OPTS]
    if stray:
        raise ValueError(f"bayes: unknown option(s) {stray}; expected some of {BAYES_OPTS}")
    opts = {"cut": float(bayes.get("cut", 50.0)), "temperature": float(bayes.get("temperature", 1.0))}
    if not opts["cut"] >= 0:
        raise ValueError(f'bayes["cut"] = {opts["cut"]}, expected >= 0 (inf: every accepted row)')
    if not (0 < opts["temperature"] < np.inf):
        raise ValueError(f'bayes["temperature"] = {opts["temperature"]}, expected finite and > 0')
    if bayes.get("quantiles") is not None:                         # (the key is there only when asked for)
        opts["quantiles"] = quantile_levels(bayes["quantiles"])
    if _group_info(shard, group)[0] > 1:
        raise ValueError("retrieve(bayes=...) does not take shard=True under a process group of more than one rank: every rank "
                         "holds only its own rows (the sharded posterior is not built yet)")
    return opts


def _bayes_shapes(M, P, opts=None):
    """the bayes_* outputs of M observations and P parameter columns; ``opts`` (_bayes_setup's) with levels: bayes_quantiles too"""
    nq = len((opts or {}).get("quantiles") or ())
    return {"bayes_mean": ((M, P), np.float64), "bayes_std": ((M, P), np.float64), "bayes_ess": ((M,), np.float64),
            "bayes_sum_w": ((M,), np.float64), "bayes_count": ((M,), np.int64),
            **({"bayes_quantiles": ((M, P, nq), np.float64)} if nq else {})}


def _bayes_maps(eng, lut_t, par_t, obs_t, weights, dtype, opts):
    """Engine.lut_bayes -> its BAYES_KEYS tensors"""
    r = eng.lut_bayes(lut_t, par_t, obs_t, weights=weights, dtype=dtype, **opts)
    return {**{key: r[name] for key, name in BAYES_KEYS.items()}, **({"bayes_quantiles": r["quantiles"]} if "quantiles" in r else {})}


def _retrieve_bayes(lut_dir, obs, column, weights, device, cols, opts):
    """the bayes_* arrays of retrieve(): the column and the chosen parameter columns go up as _upload_lut does, one
    Engine.lut_bayes for all M observations; an empty table or M = 0 gets the empty-observation values"""
    import torch
    meta, params, tabs = load_lut(lut_dir)
    table = tabs[column]
    npdt = _np_dtype(meta["dtype"])
    M, B = np.shape(obs)[0], table.shape[0]
    if B == 0 or M == 0:
        return _unmatched(_bayes_shapes(M, len(cols), opts))
    eng = get_engine(None, device)
    o = torch.as_tensor(np.asarray(obs)).to(device=eng.device, dtype=_torch_dtype(npdt))
    w = None if weights is None else _host_tensor(np.ascontiguousarray(weights, dtype=npdt)).to(eng.device)
    up = _upload_lut(eng, table, _summary_table(lut_dir, params, cols), cols, npdt)
    return {n: v.cpu().numpy() for n, v in _bayes_maps(eng, *up, o, w, meta["dtype"], opts).items()}


# what an observation that matches nothing gets, by output name (retrieve, retrieve_stream and the fit)
_EMPTY = {"idx": -1, "cost": np.inf, "best_cost": np.inf, "mean": np.nan, "median": np.nan, "std": np.nan, "count": 0,
          "bayes_mean": np.nan, "bayes_std": np.nan, "bayes_ess": np.nan, "bayes_sum_w": 0.0, "bayes_count": 0,
          "bayes_quantiles": np.nan,
          "refined": np.nan, "refined_std": np.nan, "refined_cost": np.nan, "refined_cost0": np.nan, "refined_accepts": -1,
          "refined_cov": np.nan, "refined_ak": np.nan, "refined_dfs": np.nan}


def _summary_shapes(M, P):
    return {**{n: ((M, P), np.float64) for n in STREAM_MAPS}, "count": ((M,), np.int32)}


def _refined_shapes(M, F, posterior=False):
    more = {"refined_cov": ((M, F, F), np.float64), "refined_ak": ((M, F, F), np.float64), "refined_dfs": ((M,), np.float64)}
    return {"refined": ((M, F), np.float64), "refined_std": ((M, F), np.float64), "refined_cost": ((M,), np.float64),
            "refined_cost0": ((M,), np.float64), "refined_accepts": ((M,), np.int32), **(more if posterior else {})}


def _unmatched(shapes):
    """host arrays {name: (shape, dtype)} in which nothing matched"""
    return {n: np.full(s, _EMPTY[n], dtype=d) for n, (s, d) in shapes.items()}


def _dict_prior(setup, M):
    """the (mean, weight) arrays of refine_opts["prior"] = {name: (mean, sigma)} for M observations, else None"""
    return None if setup is None or setup[0]["prior"] is None else prior_arrays(setup[0]["prior"], M)


def _f64_tensor(a, device):
    return _host_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)


class _Fit:
    """The join of search, summary, prior and fit, built once per call of retrieve / retrieve_stream from _refine_setup's
    result: the sensor's engine (the searches run on one that needs no sensor); the plan with ``column`` re-indexed and its
    prior taken out; a dict prior (_dict_prior) as device (mean, weight), with the row offset of the next run(); for the "knn"
    prior the free columns of the parameter table on the device; the shared (nb,) weights as float64."""

    def __init__(self, setup, params, column, shared, dict_prior, device):
        plan, self.opts, sensor, sensor_info = setup
        self.eng = get_engine(sensor, device, sensor_info=sensor_info)
        dev = self.eng.device
        self.plan = dict(plan, column=COLUMNS.index(column), prior=None)
        self.prior = None if dict_prior is None else tuple(_f64_tensor(a, dev) for a in dict_prior)
        self.lo = 0                                                                      # first observation of the next run()
        self.free = _f64_tensor(np.asarray(params)[:, plan["cols"]], dev) if self.opts.get("prior") == "knn" else None
        self.shared = None if shared is None else _f64_tensor(shared, dev)

    def run(self, start, idx, obs64, w64):
        """Engine.refine of the next n observations, all on the engine's device and its current stream: ``start`` (27, n) the
        rows the fit starts from, ``idx`` (n, k) lut_topk's (the "knn" prior is knn_prior of Engine.lut_summarise of the free
        columns of those rows), ``obs64`` (n, nb) float64, ``w64`` (n, nb) float64 or None (then the shared weights, if any).
        -> the REFINE_KEYS tensors (with refine_opts["posterior"] the POSTERIOR_KEYS too: Engine.refine(posterior=True), one more
        forward call at the fitted rows); an observation without a row (idx[:, 0] < 0) is fitted like the others and overwritten."""
        import torch
        n, plan, opts = idx.shape[0], self.plan, self.opts
        pm = pw = None
        if self.prior is not None:
            pm, pw = (a[self.lo:self.lo + n] if a.dim() == 2 else a for a in self.prior)
        elif self.free is not None:
            near = self.eng.lut_summarise(self.free, idx)
            pm, pw = knn_prior(near["mean"], near["std"], plan["lo"], plan["hi"], floor=opts.get("prior_floor", 0.05))
        self.lo += n
        r = self.eng.refine(start, obs64, plan["names"], weights=self.shared if w64 is None else w64, lidf=opts.get("lidf", "literal"),
                            nlayers=opts.get("nlayers"), prior_mean=pm, prior_weight=pw, band_model=opts["band_model"], _plan=plan,
                            posterior=bool(opts.get("posterior", False)))
        none = idx[:, 0] < 0
        out = {}
        for key, name in {**REFINE_KEYS, **(POSTERIOR_KEYS if opts.get("posterior", False) else {})}.items():
            v = r[name]
            out[key] = torch.where(none.reshape((-1,) + (1,) * (v.dim() - 1)), torch.full((), _EMPTY[key], dtype=v.dtype, device=v.device), v)
        return out


def _refine_best(setup, dict_prior, lut_dir, obs, idx, column, weights, device):
    """the refinement of retrieve(): start = params.npy[idx[:, 0]], gathered on the host (a memmap reads only the rows it needs),
    one _Fit.run for all M observations; no engine is asked for when no observation has a row"""
    plan = setup[0]
    out = _unmatched(_refined_shapes(idx.shape[0], len(plan["names"]), bool(setup[1].get("posterior", False))))
    if (idx[:, :1] >= 0).any():
        _, params, _ = load_lut(lut_dir)
        shared = weights if weights is not None and np.ndim(weights) == 1 else None
        fit = _Fit(setup, params, column, shared, dict_prior, device)
        dev = fit.eng.device
        rows, inv = np.unique(np.maximum(idx[:, 0], 0), return_inverse=True)
        start = np.asarray(params[rows], dtype=np.float64)[inv]           # (sorted unique rows: a memmap reads only those)
        w64 = None if weights is None or shared is not None else _f64_tensor(weights, dev)
        r = fit.run(_f64_tensor(start.T, dev), _host_tensor(np.ascontiguousarray(idx)).to(dev), _f64_tensor(obs, dev), w64)
        out = {key: v.cpu().numpy() for key, v in r.items()}
    out["refined_names"] = list(plan["names"])
    return out


def retrieve(lut_dir, obs, k, column="R_TOC", weights=None, shard=False, group=None, device=None, summary="host",
             params_cols=None, refine=None, refine_opts=None, sensor_info=None, bayes=None):
    """LUT retrieval: the k nearest rows of a generate_lut directory per observed spectrum (invert_lut(k=k)) and the
    mean, median and standard deviation of their parameters (params.npy, workloads.PARAM_NAMES order; padded rows excluded).
    ``weights`` as for invert_lut: (nb,) or (M, nb), e.g. noise_weights(obs, rel_sigma=0.02).
    ``params_cols``: a list of names from workloads.PARAM_NAMES, to summarise only those columns (``names`` follows it).  Once
    lut_products has written products.npy it may also name products (PRODUCT_NAMES): the summarised table is then the chosen
    parameter columns followed by the chosen product columns, ``names`` in that order, and mean / median / std, the bayes_*
    outputs and their quantiles cover the products like any other column (the k nearest rows or the posterior weights average
    the product itself).  A product name without products.npy is a ValueError that says to run lut_products.
    ``summary="host"`` (default): summarise_rows on the host, in numpy.  ``summary="device"``: params.npy (or the chosen columns)
    is uploaded once, the indices stay on the device between the search and Engine.lut_summarise (spart_lut_summarise), and
    the result gains ``count`` (M,) int32, the rows found per observation.  The search is the same, so idx and cost are equal
    bit for bit; median too; mean and std differ from the host's by the rounding of another summation order at most.  One
    known difference: for an observation WITH padding summarise_rows goes through numpy's nan* forms, which also drop NaN
    parameter VALUES; the device definition propagates them.  LUT parameter tables hold no NaN, so the two agree on every real
    table.  ``summary="device"`` with ``shard=True`` under a process group of more than one rank raises ValueError: each rank
    holds only its own rows (the sharded summary is not built yet).
    -> dict: idx (M, k) int64, cost (M, k), mean / median / std (M, P) float64, names (the P parameter names).

    ``refine``: a list of names from workloads.PARAM_NAMES.  The best row of every observation (params.npy[idx[:, 0]]) then
    starts a bounded Levenberg-Marquardt fit of those parameters against the observation, the others held at the row's values
    (Engine.refine / spart_refine); the keys above are unchanged, bit for bit, and the result gains ``refined`` (M, F),
    ``refined_cost``, ``refined_cost0`` (the cost at the start: cost[:, 0] of a float64 LUT bit for bit), ``refined_std``
    (M, F), ``refined_accepts`` (M,) int32 and ``refined_names``; observations without a row (idx -1) get NaN and -1.
    ``refine_opts``: bounds / n_iter / rel_step / lambda0 / lidf / nlayers / band_model of Engine.refine; the default bounds are the
    LUT's own minimum and maximum of every free column (a constant column without a bound is a ValueError).  ``"band_model"``
    (default "centre") must be the LUT's own (meta.json): a generate_lut(band_model="srf") LUT is refined with
    refine_opts={"band_model": "srf"} (spart_refine_srf: the SRF-convolved column is the fitted quantity), and only so.
    ``"prior"``: a dict
    {name: (mean, sigma)} as for Engine.refine, or ``"knn"``: knn_prior of the mean and std of the free columns of the k rows
    found (Engine.lut_summarise, whatever ``summary`` says: that summary is one defined number), with the plan's bounds and
    ``"prior_floor"`` (default 0.05); ``refined_std`` is then the linearised posterior 1-sigma.  ``"posterior": True`` adds
    ``refined_cov`` (M, F, F), the full posterior covariance, ``refined_ak`` (M, F, F), the averaging kernel, and ``refined_dfs``
    (M,), its trace, the degrees of freedom for signal (Engine.posterior at the fitted rows; NaN without a row).  The sensor is
    meta.json's ``sensor``, or ``sensor_info=`` for a LUT of a custom sensor.  ValueError for a band model other than the
    LUT's and for ``shard=True`` under a process group of more than one rank (sharded refinement is not built yet).

    ``bayes``: a dict with some of ``cut`` (default 50.0), ``temperature`` (default 1.0) and ``quantiles`` (1 ... 8 levels in
    [0, 1]); unknown keys are a ValueError.
    The likelihood-weighted estimate over EVERY accepted row whose cost lies within ``cut`` of the best one
    (Engine.lut_bayes / spart_lut_bayes; weight exp(-(c - c*) / (2 temperature))), not just the k nearest: the result gains
    ``bayes_mean``, ``bayes_std`` (M, P over ``params_cols``), ``bayes_ess`` (the effective sample size: is the LUT dense enough
    for this noise?), ``bayes_sum_w`` and ``bayes_count`` (M,) int64; every other key stays bit for bit.  It goes with either
    ``summary`` and uploads the column and the parameter columns once more; a pixel that matches nothing gets NaN, sum_w 0 and
    count 0.  ``shard=True`` under a process group of more than one rank: ValueError (the sharded posterior is not built yet).
    With ``"quantiles": [0.05, 0.5, 0.95]`` the result also gains ``bayes_quantiles`` (M, P, Q over ``params_cols``): the
    weighted quantiles of each parameter over the same rows (spart_lut_bayes_quantiles: inverted CDF, always a table value;
    NaN where nothing matched), a median and a credible interval where mean and std mislead."""
    if summary not in SUMMARIES:
        raise ValueError(f"summary = {summary!r}, expected one of {SUMMARIES}")
    names, cols = _param_columns(params_cols)
    _needs_products(lut_dir, cols)
    bayes = _bayes_setup(bayes, shard, group)
    setup = _refine_setup(lut_dir, refine, refine_opts, shard, group, sensor_info)
    dict_prior = _dict_prior(setup, np.shape(obs)[0])                    # (an array that is not (M,): refused before the search)
    out = _retrieve_summary(lut_dir, obs, k, column, weights, shard, group, device, summary, params_cols, names, cols)
    if bayes is not None:
        out.update(_retrieve_bayes(lut_dir, obs, column, weights, device, cols, bayes))
    if setup is not None:
        out.update(_refine_best(setup, dict_prior, lut_dir, obs, out["idx"], column, weights, device))
    return out


def _retrieve_summary(lut_dir, obs, k, column, weights, shard, group, device, summary, params_cols, names, cols):
    """retrieve() without the refinement"""
    if summary == "host":
        idx, cost = invert_lut(lut_dir, obs, column=column, weights=weights, shard=shard, group=group, device=device, k=k)
        _, params, _ = load_lut(lut_dir)
        mean, median, std = summarise_rows(_summary_table(lut_dir, params, cols), idx)
        if params_cols is not None:
            mean, median, std = (np.ascontiguousarray(a[:, cols]) for a in (mean, median, std))
        return {"idx": idx, "cost": cost, "mean": mean, "median": median, "std": std, "names": names}
    if _group_info(shard, group)[0] > 1:
        raise ValueError('retrieve(summary="device") does not take shard=True under a process group of more than one rank: '
                         'every rank holds only its own rows; use summary="host"')
    import torch
    meta, params, tabs = load_lut(lut_dir)
    table = tabs[column]
    npdt = _np_dtype(meta["dtype"])
    k = _check_k(int(k))
    eng = get_engine(None, device)
    o = torch.as_tensor(np.asarray(obs)).to(device=eng.device, dtype=_torch_dtype(npdt))
    M, B = o.shape[0], table.shape[0]
    if B > 0 and M > 0:
        idx, cost, res = _topk_summary(eng, *_upload_lut(eng, table, _summary_table(lut_dir, params, cols), cols, npdt), o, k, weights,
                                       meta["dtype"])
        out = {n: v.cpu().numpy() for n, v in {"idx": idx, "cost": cost, **res}.items()}
    else:
        out = _unmatched({"idx": ((M, k), np.int64), "cost": ((M, k), npdt), **_summary_shapes(M, len(cols))})
    out["names"] = names
    return out


def _upload_lut(eng, table, params, cols, npdt):
    """the LUT column in its own dtype and the chosen parameter columns as float64, on the engine's device"""
    import torch
    lut_t = torch.as_tensor(np.array(table)).to(device=eng.device, dtype=_torch_dtype(npdt))     # (a copy: memmaps opened read-only)
    return lut_t, _f64_tensor(np.asarray(params)[:, cols], eng.device)


def _topk_summary(eng, lut_t, par_t, obs_t, k, weights, dtype):
    """Engine.lut_topk, then Engine.lut_summarise of the rows found: the indices never leave the device
    -> (idx (n, k), cost (n, k), {mean, median, std, count})"""
    idx, cost = eng.lut_topk(lut_t, obs_t, k, weights=weights, dtype=dtype)
    return idx, cost, eng.lut_summarise(par_t, idx)


class _DeviceStage:
    """The device side of retrieve_stream: the LUT column and the parameter columns, uploaded once; two sets of chunk
    buffers; three streams.  upload / launch / download are what _run_pipeline calls for buffer j = chunk number % 2."""

    def __init__(self, eng, lut_t, par_t, k, dtype, chunk, per_obs_weights, shared_weights, fit=None, params=None, bayes=None):
        import torch
        self.torch, self.eng, self.lut, self.par, self.k, self.dtype = torch, eng, lut_t, par_t, k, dtype
        self.bayes = bayes              # retrieve_stream(bayes=...): Engine.lut_bayes' keyword arguments, or None
        dev = self.dev = eng.device
        nb = lut_t.shape[1]
        self.compute = torch.cuda.current_stream(dev)
        self.h2d, self.d2h = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        self.obs = [torch.empty((chunk, nb), dtype=lut_t.dtype, device=dev) for _ in range(2)]
        self.w = [torch.empty((chunk, nb), dtype=lut_t.dtype, device=dev) for _ in range(2)] if per_obs_weights else None
        self.shared = shared_weights
        self.ev_in = [torch.cuda.Event() for _ in range(2)]
        self.ev_done = [torch.cuda.Event() for _ in range(2)]
        self.used = [False, False]
        self.keep = [None, None]        # host sources of the upload in flight on buffer j
        self.res = [None, None]         # device results of the chunk in buffer j, until its download is done
        # retrieve_stream(refine=...): a _Fit and the WHOLE parameter table, (B, 27): 216 B per row, which the start rows are
        # gathered from.  The fit runs in float64: a float32 LUT's chunks go up a second time, as float64 (obs64 / w64), so that
        # it sees the numbers retrieve() hands to it
        self.fit = fit
        self.table = None if fit is None else _f64_tensor(np.asarray(params), dev)
        self.wide = fit is not None and lut_t.dtype != torch.float64
        if self.wide:
            self.obs64 = [torch.empty((chunk, nb), dtype=torch.float64, device=dev) for _ in range(2)]
            self.w64 = [torch.empty((chunk, nb), dtype=torch.float64, device=dev) for _ in range(2)] if per_obs_weights else None

    def upload(self, j, obs, w, obs64=None, w64=None):
        n = obs.shape[0]
        with self.torch.cuda.stream(self.h2d):
            if self.used[j]:
                self.h2d.wait_event(self.ev_done[j])               # the kernels that read buffer j last have run
            self.keep[j] = (obs, w, obs64, w64)
            self.obs[j][:n].copy_(_host_tensor(obs), non_blocking=True)
            if w is not None:
                self.w[j][:n].copy_(_host_tensor(w), non_blocking=True)
            if self.wide:
                self.obs64[j][:n].copy_(_host_tensor(obs64), non_blocking=True)
                if w64 is not None:
                    self.w64[j][:n].copy_(_host_tensor(w64), non_blocking=True)
            self.ev_in[j].record(self.h2d)
        self.used[j] = True

    def launch(self, j, n):
        self.compute.wait_event(self.ev_in[j])
        w = self.w[j][:n] if self.w is not None else self.shared
        idx, cost, res = _topk_summary(self.eng, self.lut, self.par, self.obs[j][:n], self.k, w, self.dtype)
        res["best_cost"] = cost[:, 0].contiguous()
        if self.bayes is not None:
            res.update(_bayes_maps(self.eng, self.lut, self.par, self.obs[j][:n], w, self.dtype, self.bayes))
        if self.fit is not None:
            start = self.table.index_select(0, idx[:, 0].clamp(min=0)).t().contiguous()      # (27, n)
            o64 = self.obs64[j][:n] if self.wide else self.obs[j][:n]
            w64 = None if self.w is None else (self.w64[j][:n] if self.wide else w)
            res.update(self.fit.run(start, idx, o64, w64))
        self.res[j] = res
        self.ev_done[j].record(self.compute)

    def download(self, j, n, dest):                                # runs on the pipeline's helper thread
        with self.torch.cuda.device(self.dev), self.torch.cuda.stream(self.d2h):
            self.d2h.wait_event(self.ev_done[j])
            for name, a in dest.items():
                _host_tensor(a).copy_(self.res[j][name], non_blocking=True)
            self.d2h.synchronize()                                 # res[j] may be replaced by chunk i + 2


def _stream_chunks(obs, weights, chunk, out, stage, npdt, wide=False):
    """retrieve_stream's chunk arithmetic: observations lo ... lo + n of chunk i go up as C-contiguous ``npdt`` arrays (with
    their own rows of (M, nb) ``weights``; None otherwise), and the stage's results land in rows lo ... lo + n of every array
    of ``out``.  ``stage``: upload(j, obs, w), launch(j, n), download(j, n, dest) for buffer j = i % 2 (_DeviceStage)."""
    M = obs.shape[0]
    chunk = int(max(1, min(int(chunk), max(M, 1))))
    nchunks = (M + chunk - 1) // chunk

    def bounds(i):
        lo = i * chunk
        return lo, min(chunk, M - lo)

    def upload(i):
        lo, n = bounds(i)
        o, w = obs[lo:lo + n], None if weights is None else weights[lo:lo + n]
        more = (np.ascontiguousarray(o, dtype=np.float64), None if w is None else np.ascontiguousarray(w, dtype=np.float64)) if wide else ()
        stage.upload(i % 2, np.ascontiguousarray(o, dtype=npdt), None if w is None else np.ascontiguousarray(w, dtype=npdt), *more)

    def launch(i):
        stage.launch(i % 2, bounds(i)[1])

    def download(i):
        lo, n = bounds(i)
        stage.download(i % 2, n, {name: a[lo:lo + n] for name, a in out.items()})
    _run_pipeline(nchunks, upload, launch, download)
    return nchunks


def retrieve_stream(lut_dir, obs, k, column="R_TOC", weights=None, params_cols=None, chunk=1 << 16, device=None, out=None,
                    refine=None, refine_opts=None, sensor_info=None, bayes=None, _stage=None):
    """A scene in, parameter maps out: retrieve(summary="device") for any number of observations, in chunks.
    ``obs`` (M, nb) on the HOST (array or memmap; any M, also 0); ``weights`` None, (nb,) or (M, nb) (sliced with the chunks),
    as for invert_lut; ``params_cols`` as for retrieve.  The LUT column and the chosen parameter columns are uploaded ONCE;
    chunks of ``chunk`` observations then run through Engine.lut_topk + Engine.lut_summarise with the upload of chunk i + 1 and
    the download of chunk i - 1 on their own streams beside the kernels of chunk i (generate_lut's schedule, _run_pipeline).
    -> dict of host arrays: mean, median, std (M, P) float64, count (M,) int32, best_cost (M,) in the LUT's dtype (the cost of
    the nearest row, the usual quality flag), and names.  The (M, k) indices are not returned: at scene size they are the bulk
    of the download and the summary replaces them.  A pixel that matches nothing (a NaN observation without a mask, a negative
    weight) comes back with count 0 and NaN maps (best_cost +inf).  Every array equals retrieve(summary="device")'s bit for
    bit, whatever the chunk size.  ``out``: caller-owned arrays of those shapes and dtypes (e.g. a previous call's result).

    ``refine`` / ``refine_opts`` / ``sensor_info`` as for retrieve (the same refusals): refined maps.  The WHOLE 27-column
    parameter table is then uploaded once as well (216 B per row), and per chunk everything after the top-k stays on the
    device and on the compute stream: the start rows are gathered from it by idx[:, 0], the "knn" prior comes from the chunk's
    own summary of the free columns, Engine.refine takes both as device tensors.  The result (and ``out``) gains ``refined``,
    ``refined_std`` (M, F), ``refined_cost``, ``refined_cost0`` (M,), ``refined_accepts`` (M,) int32 and ``refined_names``, each
    equal to retrieve(summary="device", refine=...)'s bit for bit whatever the chunk size; a pixel without a row gets NaN
    and -1; with refine_opts={"posterior": True} ``refined_cov``, ``refined_ak`` and ``refined_dfs`` as maps too.  A
    per-observation prior dict goes up once too, as its (M, F) float64 mean and weight.

    ``bayes`` as for retrieve: one more call per chunk (Engine.lut_bayes on the chunk's own buffers, the LUT and the parameter
    columns already on the device); the result (and ``out``) gains ``bayes_mean``, ``bayes_std``, ``bayes_ess``,
    ``bayes_sum_w`` and ``bayes_count`` as maps (and ``bayes_quantiles`` (M, P, Q) with ``"quantiles"``), each equal to
    retrieve(bayes=...)'s bit for bit whatever the chunk size."""
    bayes = _bayes_setup(bayes)
    setup = _refine_setup(lut_dir, refine, refine_opts, False, None, sensor_info)
    meta, params, tabs = load_lut(lut_dir)
    table = tabs[column]
    names, cols = _param_columns(params_cols)
    _needs_products(lut_dir, cols)
    k = _check_k(int(k))
    B, nb = table.shape
    npdt = _np_dtype(meta["dtype"])
    obs = obs if isinstance(obs, np.memmap) else np.asarray(obs)
    if obs.ndim != 2 or obs.shape[1] != nb:
        raise ValueError(f"obs must be (M, {nb}), got shape {obs.shape}")
    M = obs.shape[0]
    if weights is not None and not isinstance(weights, np.memmap):
        weights = np.asarray(weights)
    kind = lut_weights_kind(None if weights is None else weights.shape, M, nb)
    shapes = {**_summary_shapes(M, len(cols)), "best_cost": ((M,), npdt), **({} if bayes is None else _bayes_shapes(M, len(cols), bayes))}
    if setup is not None:
        shapes.update(_refined_shapes(M, len(setup[0]["names"]), bool(setup[1].get("posterior", False))))
    dict_prior = _dict_prior(setup, M)
    res = {n: np.empty(s, dtype=d) for n, (s, d) in shapes.items()} if out is None else _check_out(out, shapes)
    if B == 0:                                                     # an empty table matches nothing
        for n, a in res.items():
            a[...] = _EMPTY[n]
    elif M > 0:
        stage = _stage
        if stage is None:
            eng = get_engine(None, device)
            shared = weights if kind == "shared" else None
            fit = None if setup is None else _Fit(setup, params, column, shared, dict_prior, device)
            if shared is not None:
                shared = _host_tensor(np.ascontiguousarray(shared, dtype=npdt)).to(eng.device)
            up = _upload_lut(eng, table, _summary_table(lut_dir, params, cols), cols, npdt)
            stage = _DeviceStage(eng, *up, k, meta["dtype"], max(1, min(int(chunk), M)),
                                 kind == "per_observation", shared, fit=fit, params=params, bayes=bayes)
        _stream_chunks(obs, weights if kind == "per_observation" else None, chunk, res, stage, npdt,
                       wide=bool(getattr(stage, "wide", False)))
    res["names"] = names
    if setup is not None:
        res["refined_names"] = list(setup[0]["names"])
    return res


def lut_to_parquet(path, parquet_path, compression="gzip"):
    """One wide table (parameters + <column>_<band centre>) like the reference's golden files
    (tests/unit/test_PROSPECT/build_PROSPECT_tests.py:35); for LUTs that fit in memory."""
    import pandas as pd
    meta, params, cols = load_lut(path)
    df = pd.DataFrame(np.asarray(params), columns=meta["param_names"])
    for k in meta["columns"]:
        for j, w in enumerate(meta["wavelengths"]):
            df[f"{k}_{w:g}"] = np.asarray(cols[k][:, j])
    df.to_parquet(parquet_path, compression=compression)
    return parquet_path
