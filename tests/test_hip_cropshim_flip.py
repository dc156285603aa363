"""GPU: the crop shim's per-image mirrored read (`ops.crop_shim(flip=)`, `mvldm_crop_shim_flip`, csrc/cropshim.hip) against the numpy
restatement of PIL (tests/cropshim_ref.py, pinned to PIL's own output by tests/test_cropshim_cpu.py) applied to the source with the
flagged images reversed along w -- the augmentation shim's `image.flip(-1)` before `rescale_and_crop`.  Integer arithmetic: every
comparison is `torch.equal`, tolerance zero.

The small cases matter as follows: `odd`, `col_crop` and `pure_crop` have odd crop margins (the mirrored window is not the window), `even`
an even one, `wide` reads to both row ends.  `odd`'s byte buffer is 2 x 37 x 53 x 3 = 11766 bytes, no multiple of 4, but neither its
window (columns 1...48) nor the mirrored one (4...51) reaches the last column, so `whole_rows` below -- the same buffer cropped to
16 x 23, every column and the last row read -- is the case that fetches the buffer's last, partial dword on both paths."""
import numpy as np
import pytest
import torch

import cropshim_ref as R

pytestmark = pytest.mark.gpu
FLAGS = ((1, 0), (0, 1), (1, 1))


def _mirrored(src: np.ndarray, flags, axis: int) -> np.ndarray:
    out = src.copy()
    for i, f in enumerate(flags):
        if f:
            out[i] = np.flip(src[i], axis=axis - 1)
    return out


@pytest.fixture(scope="module")
def sources():
    """per case: the uint8 source and its expectation per flag pair, computed once"""
    out = {}
    for name, h, w, shape, content in R.CASES:
        src = R.make_images(name, h, w, content)
        out[name] = src, {flags: torch.from_numpy(R.crop_shim(_mirrored(src, flags, 2), shape)) for flags in FLAGS + ((0, 0),)}
    return out


@pytest.mark.parametrize("flags", FLAGS, ids=["first", "second", "both"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_flagged_images_are_mirrored_before_the_resize(sources, case, u8, flags):
    from mv_ldm_amd import ops
    name, h, w, shape, _ = case
    src, want = sources[name]
    images = torch.from_numpy(src if u8 else R.to_float(src)).cuda()           # k / 255 quantises back to k: the float path sees the same bytes
    flip = torch.tensor(flags, dtype=torch.uint8 if u8 else torch.bool, device="cuda")
    out, scaled = ops.crop_shim(images, shape, flip=flip)
    assert out.dtype == torch.float32 and tuple(out.shape) == (R.N_IMG, 3, *shape) and scaled == R.geometry(h, w, shape)[:2]
    assert torch.equal(out.cpu(), want[flags])
    assert not torch.equal(want[flags], want[(0, 0)])                           # (noise is not mirror-symmetric: the flag did something)


def test_the_mirrored_window_is_not_the_window_and_resize_then_flip_is_not_exact(sources):
    """why the flip sits at the source read: with an odd crop margin (col_crop, pure_crop: 25 columns, odd: 7) flipping the unflagged
    result is not the reference's image; with an even one (even: 26) it happens to be"""
    differs = {}
    for name in ("odd", "pure_crop", "col_crop", "even"):
        src, want = sources[name]
        differs[name] = not torch.equal(want[(1, 1)], want[(0, 0)].flip(-1))
    assert differs == {"odd": True, "pure_crop": True, "col_crop": True, "even": False}


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
def test_null_and_zero_flags_are_the_unflagged_shim(sources, u8):
    from mv_ldm_amd import _lib as L, ops
    for name, h, w, shape, _ in R.CASES:
        src, want = sources[name]
        images = torch.from_numpy(src if u8 else R.to_float(src)).cuda()
        need = ops.crop_shim_workspace_bytes(R.N_IMG, h, w, shape)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        base = torch.empty(R.N_IMG, 3, *shape, dtype=torch.float32, device="cuda")
        L.check(L.load().mvldm_crop_shim(images.data_ptr(), int(u8), base.data_ptr(), R.N_IMG, h, w, shape[0], shape[1], ws.data_ptr(), need, None, ops.stream()))
        zero = ops.crop_shim(images, shape, flip=torch.zeros(R.N_IMG, dtype=torch.uint8, device="cuda"))[0]
        null = ops.crop_shim(images, shape)[0]
        assert torch.equal(zero, base) and torch.equal(null, base) and torch.equal(base.cpu(), want[(0, 0)]), name


@pytest.mark.parametrize("flags", FLAGS + ((0, 0),), ids=["first", "second", "both", "none"])
def test_the_buffers_last_partial_dword(flags):
    """37 x 53 -> 16 x 23: scaled 16 x 23, nothing cropped, so the horizontal pass stages whole rows, the last row of the last image
    included: bytes 11764 and 11765 come from the partial dword, mirrored (slot 0) or not (the last slot).  The source is exactly sized."""
    from mv_ldm_amd import ops
    h, w, shape = 37, 53, (16, 23)
    assert R.geometry(h, w, shape) == (16, 23, 0, 0) and (R.N_IMG * h * w * 3) % 4 == 2
    assert R.axis_tables(w, 23)[1][0, 0] == 0 and R.axis_tables(w, 23)[1][-1].sum() == w and R.axis_tables(h, 16)[1][-1].sum() == h
    src = R.make_images("whole_rows", h, w, "noise")
    out = ops.crop_shim(torch.from_numpy(src).cuda(), shape, flip=torch.tensor(flags, dtype=torch.uint8, device="cuda"))[0]
    assert torch.equal(out.cpu(), torch.from_numpy(R.crop_shim(_mirrored(src, flags, 2), shape)))


def test_full_size_mirrored_by_digest():
    """360 x 640 -> 256 x 256, the first image mirrored: the bytes behind the floats hash to the restatement's"""
    from mv_ldm_amd import ops
    name, h, w, shape, content = R.FULL
    src = R.make_images(name, h, w, content)
    out = ops.crop_shim(torch.from_numpy(src).cuda(), shape, flip=torch.tensor([1, 0], dtype=torch.uint8, device="cuda"))[0].cpu()
    pixels = (out * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    assert torch.equal(out, torch.from_numpy(R.to_float(pixels)))
    want = R.resize_crop_u8(_mirrored(src, (1, 0), 2), shape)
    assert R.digest(pixels) == R.digest(want) != R.digest(R.resize_crop_u8(src, shape))


@pytest.mark.parametrize("name,h,w,shape,pad", [("col_crop", 45, 80, (32, 32), 64), ("ragged", 37, 53, (16, 15), 64), ("offset", 37, 53, (16, 16), 68)],
                         ids=["wide_stores", "ragged_width", "unaligned_rows"])
def test_writes_stay_inside_dst_and_workspace(name, h, w, shape, pad):
    """dst and an exactly sized workspace in the middle of canary-filled buffers, the source exactly sized too, the second image mirrored"""
    from mv_ldm_amd import _lib as L, ops
    src_np = R.make_images(name, h, w, "noise")
    src = torch.from_numpy(src_np).cuda()
    flip = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
    n_out = R.N_IMG * 3 * shape[0] * shape[1]
    need = ops.crop_shim_workspace_bytes(R.N_IMG, h, w, shape)
    dst = torch.full((pad // 4 + n_out + 64,), -7.0, dtype=torch.float32, device="cuda")
    ws = torch.full((64 + need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = dst[pad // 4:pad // 4 + n_out]
    L.check(L.load().mvldm_crop_shim_flip(src.data_ptr(), 1, mid.data_ptr(), R.N_IMG, h, w, shape[0], shape[1], flip.data_ptr(), ws[64:].data_ptr(), need,
                                          None, ops.stream()))
    torch.cuda.synchronize()
    dst, ws = dst.cpu(), ws.cpu()
    assert (dst[:pad // 4] == -7.0).all() and (dst[pad // 4 + n_out:] == -7.0).all()
    assert (ws[:64] == 0xA5).all() and (ws[64 + need:] == 0xA5).all()
    assert torch.equal(dst[pad // 4:pad // 4 + n_out].reshape(R.N_IMG, 3, *shape), torch.from_numpy(R.crop_shim(_mirrored(src_np, (0, 1), 2), shape)))


def test_bad_arguments_are_refused():
    from mv_ldm_amd import _lib as L, ops
    lib = L.load()
    src = torch.zeros(2, 45, 80, 3, dtype=torch.uint8, device="cuda")
    flip = torch.ones(2, dtype=torch.uint8, device="cuda")
    need = ops.crop_shim_workspace_bytes(2, 45, 80, (32, 32))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dst = torch.empty(2, 3, 32, 32, dtype=torch.float32, device="cuda")
    call = lambda s=src.data_ptr(), u8=1, d=dst.data_ptr(), h=45, w=80, ho=32, wo=32, nbytes=need: lib.mvldm_crop_shim_flip(
        s, u8, d, 2, h, w, ho, wo, flip.data_ptr(), ws.data_ptr(), nbytes, None, ops.stream())
    OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3                                    # include/mvldm.h
    assert call() == OK
    for bad in (call(nbytes=need - 1), call(u8=2), call(ho=64), call(wo=0), call(s=None), call(d=dst.data_ptr() + 2)):
        assert bad == ERR_ARG, bad
    assert call(w=16385) == ERR_UNSUPPORTED
    with pytest.raises(L.MvldmError, match="workspace"):
        ops.crop_shim(src, (32, 32), ws[:-1], flip=flip)
    for wrong in (flip.cpu(), flip[:1], flip.int()):
        with pytest.raises(AssertionError):
            ops.crop_shim(src, (32, 32), flip=wrong)
    out, scaled = ops.crop_shim(src[:0], (32, 32), flip=flip[:0])
    assert tuple(out.shape) == (0, 3, 32, 32) and scaled == (32, 57)
