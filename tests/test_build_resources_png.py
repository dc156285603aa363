"""CPU: the PNG kernel (csrc/png.hip) in the build's resource report.  Its state is a handful of scalars per lane and two blocks of eight
prefetched words; an array the unrolling left indexed at run time would land in scratch behind every step of a serial chain: zero scratch,
zero spills, and registers for at least four waves per SIMD (the kernel runs one wave per frame, a batch is many frames)."""
import json

import pytest


@pytest.fixture(scope="module")
def resources():
    from mv_ldm_amd import _build
    _build.build()
    if not _build.RES.exists():
        _build.build(force=True)
    return json.loads(_build.RES.read_text())


def test_png_kernel_uses_no_scratch(resources):
    mine = {k: v for k, v in resources.items() if "png_unfilter_kernel" in k}
    assert len(mine) == 1, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0, (k, v)
        assert v["vgpr"] + v.get("agpr", 0) <= 128, (k, v)
