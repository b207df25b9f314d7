"""Static LDS bytes per kernel of libspart_hip's device code, from each kernel's descriptor block in the device assembly
(.amdhsa_kernel NAME ... .amdhsa_group_segment_fixed_size N; build.device_asm, no GPU needed).  Memoised: one device
compile per process."""
import functools
import os
import re
import sys
import tempfile

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


@functools.lru_cache(maxsize=None)
def kernel_lds():
    """{mangled kernel name: bytes of static LDS}"""
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for f in build.device_asm(d):
            for name, body in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", open(f).read(), flags=re.S):
                out[name] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
    return out
