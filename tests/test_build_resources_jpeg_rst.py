"""CPU: the restart-interval kernels (csrc/jpeg_huff.hip) in the build's resource report.  A workgroup of 1024 leaves a lane 128 registers;
the lane's description of its subsequence (pointer, bits, index, first lane, blocks) is scalars, and anything hipcc demotes to scratch
would sit behind every symbol of a serial chain: each kernel once, zero scratch, zero spills."""
import json

import pytest


@pytest.fixture(scope="module")
def resources():
    from mv_ldm_amd import _build
    _build.build()
    if not _build.RES.exists():
        _build.build(force=True)
    return json.loads(_build.RES.read_text())


def test_restart_kernels_use_no_scratch(resources):
    mine = {k: v for k, v in resources.items() if "jpeg_rst_scan_kernel" in k or "jpeg_rst_dc_kernel" in k}
    assert sum("jpeg_rst_scan_kernel" in k for k in mine) == 1 and sum("jpeg_rst_dc_kernel" in k for k in mine) == 1, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0, (k, v)
        assert v["vgpr"] + v.get("agpr", 0) <= 128, (k, v)         # 1024 lanes = 4 waves per SIMD
