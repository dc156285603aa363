"""CPU: the crop shim's expectation and host side.  tests/cropshim_ref.py (numpy integers) against PIL's own output
(tests/golden/cropshim.npz, and Pillow directly where it is installed); the geometry and camera helpers; the library's host-built
tables, workspace size and refusals (no launch happens: every call here returns before the device is touched)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import cropshim_ref as R

ALL = R.CASES + (R.FULL,)


@pytest.fixture(scope="module")
def gold(golden):
    return golden("cropshim")


@pytest.fixture(scope="module")
def lib():
    from mv_ldm_amd import _build, _lib
    _build.build()
    return _lib.load()


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_equals_every_golden_byte(gold, case):
    name, h, w, shape, content = case
    src = R.make_images(name, h, w, content)
    assert np.array_equal(src, gold[f"{name}_src"])                 # the generator the GPU tests share
    got = R.resize_crop_u8(src, shape)
    assert got.shape == (R.N_IMG, *shape, 3) and np.array_equal(got, gold[f"{name}_out"])
    if content == "checker":                                        # the case is there for the clips: both must occur
        assert (got == 0).any() and (got == 255).any()


def test_restatement_full_size_digest(gold):
    name, h, w, shape, content = R.FULL
    assert R.digest(R.resize_crop_u8(R.make_images(name, h, w, content), shape)) == str(gold["full_sha256"])


@pytest.mark.parametrize("h,w,shape", [(31, 47, (16, 24)), (64, 48, (24, 17)), (50, 50, (50, 50)), (29, 90, (9, 9)), (48, 64, (48, 60))])
def test_restatement_equals_pil(h, w, shape):
    Image = pytest.importorskip("PIL.Image")
    src = np.random.default_rng(h * 1000 + w).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    h_s, w_s, row, col = R.geometry(h, w, shape)
    want = np.stack([np.array(Image.fromarray(im).resize((w_s, h_s), Image.LANCZOS)) for im in src])[:, row:row + shape[0], col:col + shape[1]]
    assert np.array_equal(R.resize_crop_u8(src, shape), want)


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_geometry_and_intrinsics(gold, case):
    from mv_ldm_amd import dataset, ops
    name, h, w, shape, _ = case
    h_s, w_s, row, col = ops.crop_geometry(h, w, shape)
    assert (h_s, w_s) == tuple(gold[f"{name}_scaled"]) and (h_s, w_s, row, col) == R.geometry(h, w, shape)
    assert (row, col) == ((h_s - shape[0]) // 2, (w_s - shape[1]) // 2) and (h_s == shape[0] or w_s == shape[1])
    if name != "full":
        k_in = torch.from_numpy(gold[f"{name}_k_in"])
        keep = k_in.clone()
        got = dataset.crop_intrinsics(k_in, (h_s, w_s), shape)
        assert torch.equal(got, torch.from_numpy(gold[f"{name}_k_out"])) and torch.equal(k_in, keep)       # a clone is changed
        assert np.array_equal(R.scale_intrinsics(keep.numpy(), h_s, w_s, shape), gold[f"{name}_k_out"])


def test_geometry_known_values():
    from mv_ldm_amd import ops
    assert ops.crop_geometry(360, 640, (256, 256)) == (256, 455, 0, 99)
    assert ops.crop_geometry(45, 80, (32, 32)) == (32, 57, 0, 12)
    assert ops.crop_geometry(80, 45, (32, 32)) == (57, 32, 12, 0)
    assert ops.crop_geometry(37, 53, (16, 16)) == (16, 23, 0, 3)
    assert ops.crop_geometry(40, 72, (32, 32)) == (32, 58, 0, 13)
    assert ops.crop_geometry(23, 200, (8, 8)) == (8, 70, 0, 31)
    with pytest.raises(AssertionError):
        ops.crop_geometry(32, 32, (33, 32))


def _tables(lib, n_in, n_out, off, count):
    bounds = np.zeros((count, 2), np.int32)
    ks = lib.mvldm_crop_shim_axis(n_in, n_out, off, count, bounds.ctypes.data_as(C.POINTER(C.c_int32)), None, 0)
    assert ks > 0, lib.mvldm_last_error()
    coefs = np.full((count, ks), -1, np.int32)
    assert lib.mvldm_crop_shim_axis(n_in, n_out, off, count, None, coefs.ctypes.data_as(C.POINTER(C.c_int32)), coefs.size) == ks
    return ks, bounds, coefs


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_library_tables_equal_the_restatement(lib, case):
    """the host half of the kernel: bounds and 22-bit coefficients as the library uploads them, for the windows the op uses"""
    _, h, w, shape, _ = case
    h_s, w_s, row, col = R.geometry(h, w, shape)
    for n_in, n_out, off, count in ((w, w_s, col, shape[1]), (h, h_s, row, shape[0])):
        ks, bounds, coefs = _tables(lib, n_in, n_out, off, count)
        rks, rb, rc = R.axis_tables(n_in, n_out, off, count)
        assert ks == rks and np.array_equal(bounds, rb) and np.array_equal(coefs, rc)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ks).all()
        # the int32 sum cannot overflow: 255 sum |k| + 2^21 < 2^31
        assert 255 * int(np.abs(coefs.astype(np.int64)).sum(1).max()) + (1 << 21) < (1 << 31)


def test_workspace_bytes_and_refusals(lib):
    from mv_ldm_amd import ops
    ws = lib.mvldm_crop_shim_workspace_bytes
    _, by, _ = R.axis_tables(360, 256, 0, 256)
    rows = int((by[:, 0] + by[:, 1]).max() - by[:, 0].min())
    assert ws(5, 360, 640, 256, 256) == 5 * 3 * rows * 256 == ops.crop_shim_workspace_bytes(5, 360, 640, (256, 256))
    assert ws(2, 37, 53, 16, 16) == 2 * 3 * 37 * 16                  # every source row is under some tap
    assert ws(2, 32, 57, 32, 30) == 2 * 3 * 32 * 32                  # rows of the workspace are whole dwords
    assert ws(0, 45, 80, 32, 32) == 0 and ws(2, 32, 32, 33, 32) == 0 and ws(2, 0, 32, 0, 32) == 0 and ws(2, 32, 32768, 32, 32) == 0
    err = lambda: lib.mvldm_last_error()
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    p = buf.data_ptr()
    assert p % 16 == 0
    call = lambda src=p, u8=1, dst=p, n=2, h=45, w=80, ho=32, wo=32, wsp=p, wsb=1 << 16: lib.mvldm_crop_shim(src, u8, dst, n, h, w, ho, wo, wsp, wsb, None, None)
    assert call(u8=2) == -1 and b"src_u8" in err()                   # -1: MVLDM_ERR_ARG, -3: MVLDM_ERR_UNSUPPORTED
    assert call(n=-1) == -1 and b"n_img" in err()
    assert call(ho=0) == -1 and b"edge below 1" in err()
    assert call(ho=46) == -1 and b"only shrinks" in err()
    assert call(w=32768) == -3 and b"supported" in err()
    assert call(wsb=ws(2, 45, 80, 32, 32) - 1) == -1 and b"workspace" in err()
    assert call(src=None) == -1 and b"null" in err()
    assert call(dst=p + 2) == -1 and b"unaligned" in err()
    got = (C.c_int * 2)()
    assert lib.mvldm_crop_shim(None, 1, None, 0, 45, 80, 32, 32, None, 0, got, None) == 0 and tuple(got) == (32, 57)       # nothing to do
    assert lib.mvldm_crop_shim_axis(8, 9, 0, 9, None, None, 0) == -1 and lib.mvldm_crop_shim_axis(9, 8, 4, 5, None, None, 0) == -1


def test_new_kernels_use_no_scratch(lib):
    from mv_ldm_amd import _build
    if not _build.RES.exists():
        _build.build(force=True)
    res = {k: v for k, v in json.loads(_build.RES.read_text()).items() if "crop_h_kernel" in k or "crop_v_kernel" in k}
    assert len(res) == 4, sorted(res)
    assert all(v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0 for v in res.values()), res
