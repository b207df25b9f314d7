"""The compiled kernel metadata for the static guards (tests/test_*_resources.py, tests/test_isa_budget.py): a test module
imports the `kernel_meta` fixture from here; where there is no hipcc the test is skipped."""
import os
import shutil

import pytest

from helpers.kernel_meta import kernel_meta


def compiled(extra=()):
    """kernel_meta(extra) (memoised: one device compile per pytest process and flag set), or skip the calling test"""
    if not any(c and os.path.exists(c) for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc"))):
        pytest.skip("hipcc not available")
    return kernel_meta(extra)


@pytest.fixture(scope="module", name="kernel_meta")
def kernel_meta_fixture():
    return compiled()
