"""Per-kernel resource metadata of libspart_hip's device code (hipcc -S of every translation unit with ITS flags,
build.device_asm; no GPU needed).  Memoised: one process compiles the device code once per set of extra flags."""
import functools
import os
import re
import sys
import tempfile

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
FIELDS = "vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size"


@functools.lru_cache(maxsize=None)
def kernel_meta(extra=()):
    """{mangled kernel name: {field of FIELDS: value}} for every kernel; ``extra``: a tuple of further hipcc flags"""
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    meta, cur = {}, None
    with tempfile.TemporaryDirectory() as d:
        for line in (l for f in build.device_asm(d, extra) for l in open(f)):
            m = re.match(r"\s+\.name:\s+(\S+)", line)
            if m:
                cur = m.group(1)
                meta[cur] = {}
                continue
            m = re.match(r"\s+\.(" + FIELDS + r"):\s+(\d+)", line)
            if m and cur:
                meta[cur][m.group(1)] = int(m.group(2))
    return {k: v for k, v in meta.items() if "vgpr_count" in v}
