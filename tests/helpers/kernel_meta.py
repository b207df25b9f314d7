"""Per-kernel resource metadata of libspart_hip's device code (hipcc -S of every translation unit with ITS flags,
build.device_asm; no GPU needed): the one reader behind every static guard and tools/kernel_meta.py.  Memoised: one process
compiles the device code once per set of extra flags."""
import functools
import os
import re
import sys
import tempfile

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
FIELDS = "vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size"


@functools.lru_cache(maxsize=None)
def device_asm(extra=()):
    """{file name of the translation unit: its device assembly}; ``extra``: a tuple of further hipcc flags"""
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    with tempfile.TemporaryDirectory() as d:
        return {os.path.basename(f)[:-len(".s")]: open(f).read() for f in build.device_asm(d, extra)}


def read_kernels(asm):
    """{mangled kernel name: {field of FIELDS: value}} of one translation unit's assembly.  A record of `amdhsa.kernels` is
    one list item (its fields are sorted, so some precede `.name`) and is read whole; the LDS size is checked against the
    kernel's own descriptor block (.amdhsa_kernel NAME ... .end_amdhsa_kernel), a second source in the same file."""
    meta = {}
    records = re.search(r"^amdhsa\.kernels:\n(.*?)^(?=\S)", asm, flags=re.M | re.S).group(1)      # up to the next top-level key
    for rec in re.split(r"^  - ", records, flags=re.M)[1:]:
        rec = "    " + rec                              # (the item's first field now sits at the indent of the others)
        name = re.search(r"^    \.name:\s+(\S+)", rec, flags=re.M).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"^    \.(" + FIELDS + r"):\s+(\d+)", rec, flags=re.M)}
    blocks = dict(re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S))
    if set(blocks) != set(meta):
        raise ValueError(f"kernels with a record but no descriptor block, or the reverse: {sorted(set(blocks) ^ set(meta))}")
    for name, body in blocks.items():
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        if meta[name]["group_segment_fixed_size"] != lds:
            raise ValueError(f"{name}: group_segment_fixed_size {meta[name]['group_segment_fixed_size']} in its record, {lds} in its descriptor")
    return meta


@functools.lru_cache(maxsize=None)
def kernel_meta(extra=()):
    """{mangled kernel name: {field of FIELDS: value}} for every kernel; ``extra``: a tuple of further hipcc flags"""
    return {k: v for asm in device_asm(extra).values() for k, v in read_kernels(asm).items()}
