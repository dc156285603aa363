"""GPU: `ops.crop_shim` (csrc/cropshim.hip) against PIL's own output (tests/golden/cropshim.npz).  The arithmetic is integer and the
numpy restatement reproduces PIL with zero mismatching bytes (tests/test_cropshim_cpu.py), so every comparison is `torch.equal` on
every pixel of every image: tolerance zero."""
import numpy as np
import pytest
import torch

import cropshim_ref as R

pytestmark = pytest.mark.gpu
BY_NAME = {c[0]: c for c in R.CASES}


@pytest.fixture(scope="module")
def gold(golden):
    return golden("cropshim")


def _want(gold, name) -> torch.Tensor:
    return torch.from_numpy(R.to_float(gold[f"{name}_out"]))


def _src(gold, name) -> torch.Tensor:
    return torch.from_numpy(gold[f"{name}_src"]).cuda()


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_small_cases_equal_pil(gold, case):
    from mv_ldm_amd import ops
    name, h, w, shape, _ = case
    out, scaled = ops.crop_shim(_src(gold, name), shape)
    assert out.dtype == torch.float32 and tuple(out.shape) == (R.N_IMG, 3, *shape) and scaled == tuple(gold[f"{name}_scaled"])
    assert torch.equal(out.cpu(), _want(gold, name))


def test_full_size_by_digest(gold):
    """360 x 640 -> 256 x 256: the bytes behind the floats hash to PIL's, and the floats are exactly those bytes / 255"""
    from mv_ldm_amd import ops
    name, h, w, shape, content = R.FULL
    out, scaled = ops.crop_shim(torch.from_numpy(R.make_images(name, h, w, content)).cuda(), shape)
    assert scaled == tuple(gold["full_scaled"]) == (256, 455)
    out = out.cpu()
    pixels = (out * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    assert torch.equal(out, torch.from_numpy(R.to_float(pixels)))
    assert R.digest(pixels) == str(gold["full_sha256"])


def test_float_input_is_quantised_as_the_reference_does():
    """the 256 values k / 255 and the edges of the clamp, tiled into 45 x 80 float images: the same result as feeding the reference's own
    quantisation -- (image * 255).clip(0, 255).type(uint8), by torch on the CPU -- as bytes.  Truncation, not rounding: 0.999999 is 254."""
    from mv_ldm_amd import ops
    vals = torch.cat([torch.arange(256, dtype=torch.float32) / 255, torch.tensor([-0.1, 0.0, 0.5 / 255, 0.999999, 1.0, 1.5])])
    n, h, w, shape = 2, 45, 80, (32, 32)
    perm = torch.randperm(n * 3 * h * w, generator=torch.Generator().manual_seed(5))
    image = vals.repeat(-(-n * 3 * h * w // len(vals)))[:n * 3 * h * w][perm].reshape(n, 3, h, w).contiguous()
    q = (image * 255).clip(min=0, max=255).type(torch.uint8)
    assert np.array_equal(q.permute(0, 2, 3, 1).numpy(), R.quantise(image.numpy()))
    assert q.min() == 0 and q.max() == 255 and (q == 254).any()          # -0.1 and 1.5 are clamped, 0.999999 is truncated to 254
    from_bytes, _ = ops.crop_shim(q.permute(0, 2, 3, 1).contiguous().cuda(), shape)
    from_float, scaled = ops.crop_shim(image.cuda(), shape)
    assert scaled == (32, 57) and torch.equal(from_float, from_bytes)
    assert torch.equal(from_float.cpu(), torch.from_numpy(R.crop_shim(image.numpy(), shape)))


def test_calls_of_different_shapes_share_a_workspace(gold):
    """the table cache is keyed by the geometry: a call is unaffected by the one before it"""
    from mv_ldm_amd import ops
    names = ("col_crop", "odd", "row_crop", "col_crop", "wide", "odd")
    need = max(ops.crop_shim_workspace_bytes(R.N_IMG, BY_NAME[n][1], BY_NAME[n][2], BY_NAME[n][3]) for n in names)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = [ops.crop_shim(_src(gold, n), BY_NAME[n][3], ws)[0] for n in names]          # back to back on one stream
    for n, out in zip(names, outs):
        assert torch.equal(out.cpu(), _want(gold, n)), n


def test_a_captured_call_replays_to_the_same_bytes(gold):
    from mv_ldm_amd import ops
    name, h, w, shape, _ = BY_NAME["even"]
    src = _src(gold, name)
    ws = torch.empty(ops.crop_shim_workspace_bytes(R.N_IMG, h, w, shape), dtype=torch.uint8, device="cuda")
    buf = torch.zeros_like(src)                                                         # captured on other contents
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = ops.crop_shim(src, shape, ws)[0].clone()                                # warm-up: the tables of this geometry are uploaded
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                       # one stream: a single-branch graph
        out = ops.crop_shim(buf, shape, ws)[0]
    buf.copy_(src)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out.cpu(), _want(gold, name))


@pytest.mark.parametrize("name,h,w,shape,pad", [("col_crop", 45, 80, (32, 32), 64), ("ragged", 37, 53, (16, 15), 64), ("offset", 37, 53, (16, 16), 68)],
                         ids=["wide_stores", "ragged_width", "unaligned_rows"])
def test_writes_stay_inside_dst_and_workspace(name, h, w, shape, pad):
    """dst and an exactly sized workspace in the middle of canary-filled buffers: 16-byte stores (aligned dst, width a multiple of 4), a
    width that is no multiple of 4 (the workspace's rows are padded to dwords, dst's are not) and a dst that is only 4-byte aligned"""
    from mv_ldm_amd import _lib as L, ops
    src_np = R.make_images(name, h, w, "noise")
    src = torch.from_numpy(src_np).cuda()
    n_out = R.N_IMG * 3 * shape[0] * shape[1]
    need = ops.crop_shim_workspace_bytes(R.N_IMG, h, w, shape)
    dst = torch.full((pad // 4 + n_out + 64,), -7.0, dtype=torch.float32, device="cuda")
    ws = torch.full((64 + need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = dst[pad // 4:pad // 4 + n_out]
    L.check(L.load().mvldm_crop_shim(src.data_ptr(), 1, mid.data_ptr(), R.N_IMG, h, w, shape[0], shape[1], ws[64:].data_ptr(), need, None, ops.stream()))
    torch.cuda.synchronize()
    dst, ws = dst.cpu(), ws.cpu()
    assert (dst[:pad // 4] == -7.0).all() and (dst[pad // 4 + n_out:] == -7.0).all()
    assert (ws[:64] == 0xA5).all() and (ws[64 + need:] == 0xA5).all()
    assert torch.equal(dst[pad // 4:pad // 4 + n_out].reshape(R.N_IMG, 3, *shape), torch.from_numpy(R.crop_shim(src_np, shape)))


def test_a_short_workspace_and_an_empty_batch():
    from mv_ldm_amd import _lib as L, ops
    src = torch.zeros(2, 45, 80, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.MvldmError, match="workspace"):
        ops.crop_shim(src, (32, 32), torch.empty(ops.crop_shim_workspace_bytes(2, 45, 80, (32, 32)) - 1, dtype=torch.uint8, device="cuda"))
    out, scaled = ops.crop_shim(src[:0], (32, 32))
    assert tuple(out.shape) == (0, 3, 32, 32) and scaled == (32, 57)
