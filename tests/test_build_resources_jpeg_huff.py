"""CPU: the device entropy decoder's kernels (csrc/jpeg_huff.hip) in the build's resource report.  Their state is a handful of scalars per
lane -- bit position, block and zigzag index, three words of the bit window -- and a per-lane array (a window buffer, a local copy of a
table) would land in scratch behind every symbol of a serial chain: zero scratch, zero spills, and if hipcc gives any the kernel changes."""
import json

import pytest


@pytest.fixture(scope="module")
def resources():
    from mv_ldm_amd import _build
    _build.build()
    if not _build.RES.exists():
        _build.build(force=True)
    return json.loads(_build.RES.read_text())


def test_huffman_kernels_use_no_scratch(resources):
    mine = {k: v for k, v in resources.items() if "jpeg_huff_kernel" in k or "jpeg_huff_dc_kernel" in k}
    assert sum("jpeg_huff_kernel" in k for k in mine) == 1 and sum("jpeg_huff_dc_kernel" in k for k in mine) == 1, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0, (k, v)
        assert v["vgpr"] + v.get("agpr", 0) <= 128, (k, v)         # 1024 lanes = 4 waves per SIMD
