"""Writes tests/golden/cropshim.npz: the crop shim's expectation from PIL itself (run where Pillow is installed; the tests need only the file).

Per case of tests/cropshim_ref.py the reference's three steps, literally (src/dataset/shims/crop_shim.py:11-75):
`Image.fromarray(image).resize((w_scaled, h_scaled), Image.LANCZOS)`, the centre crop, `/ 255` (the division is left to the tests: the
file keeps the cropped bytes), and `center_crop`'s intrinsics through torch.  Small cases store input, output and intrinsics; the
360 x 640 one only its seed's name and the SHA-256 of the expected bytes.

    python tests/golden/make_cropshim_golden.py"""
import sys
from pathlib import Path

import numpy as np
import torch
from PIL import Image

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import cropshim_ref as R  # noqa: E402


def reference_bytes(images: np.ndarray, shape) -> np.ndarray:
    """uint8 [n, h, w, 3] -> uint8 [n, h_out, w_out, 3] through PIL"""
    n, h, w, _ = images.shape
    h_out, w_out = shape
    scale_factor = max(h_out / h, w_out / w)
    h_scaled, w_scaled = round(h * scale_factor), round(w * scale_factor)
    assert h_scaled == h_out or w_scaled == w_out
    out = np.stack([np.array(Image.fromarray(im).resize((w_scaled, h_scaled), Image.LANCZOS)) for im in images])
    row, col = (h_scaled - h_out) // 2, (w_scaled - w_out) // 2
    return out[:, row:row + h_out, col:col + w_out], (h_scaled, w_scaled)


def reference_intrinsics(intrinsics: torch.Tensor, scaled, shape) -> torch.Tensor:
    intrinsics = intrinsics.clone()
    intrinsics[..., 0, 0] *= scaled[1] / shape[1]  # fx
    intrinsics[..., 1, 1] *= scaled[0] / shape[0]  # fy
    return intrinsics


def main():
    import PIL
    rec = {"pil_version": np.array(PIL.__version__)}
    g = torch.Generator().manual_seed(0)
    for name, h, w, shape, content in R.CASES:
        src = R.make_images(name, h, w, content)
        out, scaled = reference_bytes(src, shape)
        k = torch.eye(3).repeat(R.N_IMG, 1, 1)
        k[:, 0, 0], k[:, 1, 1] = 0.4 + torch.rand(R.N_IMG, generator=g), 0.4 + torch.rand(R.N_IMG, generator=g)
        k[:, 0, 2] = k[:, 1, 2] = 0.5
        rec[f"{name}_src"], rec[f"{name}_out"] = src, np.ascontiguousarray(out)
        rec[f"{name}_scaled"] = np.array(scaled, np.int32)
        rec[f"{name}_k_in"], rec[f"{name}_k_out"] = k.numpy(), reference_intrinsics(k, scaled, shape).numpy()
    name, h, w, shape, content = R.FULL
    out, scaled = reference_bytes(R.make_images(name, h, w, content), shape)
    rec["full_sha256"], rec["full_scaled"] = np.array(R.digest(out)), np.array(scaled, np.int32)
    path = HERE / "cropshim.npz"
    np.savez_compressed(path, **rec)
    print(f"{path}: {path.stat().st_size} bytes, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()
