"""CPU: the inflate kernel (csrc/inflate.hip) in the build's resource report.  Its state is the decoding lane's bit buffer and a few
scalars; the tables, the window and the queue live in LDS.  An unrolled cold loop (the fixed code's lengths, the code-length order)
hoists its constants into registers for the whole kernel, and an array indexed at run time would land in scratch behind every symbol:
zero scratch, zero spills, and registers for at least four waves per SIMD -- the bound the PNG kernel's test uses; the kernel runs one
wave per frame and a batch is many frames."""
import json

import pytest


@pytest.fixture(scope="module")
def resources():
    from mv_ldm_amd import _build
    _build.build()
    if not _build.RES.exists():
        _build.build(force=True)
    return json.loads(_build.RES.read_text())


def test_inflate_kernel_uses_no_scratch(resources):
    mine = {k: v for k, v in resources.items() if "png_inflate_kernel" in k}
    assert len(mine) == 1, sorted(mine)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0, (k, v)
        assert v["vgpr"] + v.get("agpr", 0) <= 128, (k, v)
