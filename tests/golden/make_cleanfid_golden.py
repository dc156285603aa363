"""Writes tests/golden/cleanfid_resize.npz: PIL's own outputs of the resize clean-fid's "clean" mode calls -- every channel through
`Image.fromarray(x.astype(float32), mode="F").resize((ow, oh), resample=BICUBIC)` -- on seeded uint8 inputs and the pattern of
tests/test_hip_fid.py.  The only real pin this metric has: run on the CPU, with PIL; the GPU tests read the file and never import PIL.

    python tests/golden/make_cleanfid_golden.py

Cases (h x w -> oh x ow): 13 x 17 -> 29 x 23 (up both ways), 64 x 48 -> 29 x 23 (down: support > 2, taps clipped at both edges),
31 x 16 -> 16 x 31 (one down, one up), 16 x 16 -> 16 x 16 (both passes skipped)."""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import cleanfid_ref as R      # noqa: E402

if __name__ == "__main__":
    import PIL
    out = {"pil_version": np.array(PIL.__version__)}
    for h, w, oh, ow in R.RESIZE_CASES:
        src = R.resize_inputs(h, w)
        got = R.resize_pil(R.to_255(src), oh, ow)
        assert got.dtype == np.float32 and got.shape == (4, 3, oh, ow)
        if (h, w) == (oh, ow):
            assert np.array_equal(got, src.numpy().astype(np.float32))
        out[f"src_{h}x{w}_{oh}x{ow}"] = src.numpy()
        out[f"out_{h}x{w}_{oh}x{ow}"] = got
    path = HERE / "cleanfid_resize.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < 256 * 1024, path.stat().st_size
    print(path, path.stat().st_size, "bytes; PIL", PIL.__version__)
