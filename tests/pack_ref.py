"""The expectation of the weight-packer tests: the layouts of `mvldm_pack_weight` and `mvldm_pack_skinny` as include/mvldm.h states them,
written out as index arithmetic over the `[n_pad, k_pad]` grid of the packed tensor -- one gather and one conversion, no permute / reshape
of the weight (those cannot say "70 channels in a 128-channel pad" or "rows 3 .. 23 of 40").  A helper module like tests/cropshim_ref.py:
imported by tests/test_hip_pack_edges.py.  Works on CPU and on device tensors alike (the two grid-stride cases are too large to bring back).

Comparisons are on BITS (`same_bits`): -0.0 is not 0.0 and a conversion that rounds the wrong way is a different value; only NaN is
compared by position, since the payload of a converted NaN is the converter's business."""
import torch

GUARD_ROWS = 64           # rows of k_pad elements in front of and behind every destination
GUARD_BYTE = 0xAB


def block_k(dtype):
    return 32 if dtype == torch.float32 else 64


def geglu_row(np_, n_out):
    """source row of packed row np_ (< n_out) under the GEGLU interleave: 32 value rows (n), then their 32 gate rows (n + n_out/2)"""
    blk, wi = np_ // 32, np_ % 32
    return torch.where(blk % 2 == 1, n_out // 2 + (blk // 2) * 32 + wi, (blk // 2) * 32 + wi)


def pack_ref(w, dtype, *, c_pad, n_pad, k_pad, geglu=False, k_order=0, transpose=False, c_off=0, n_rows=None):
    """w fp32 `[n_out, c_in, k, k]` or `[n_out, c_in]` -> `[n_pad, k_pad]` in `dtype`: every element, the zero padding included"""
    n_out, c_in = w.shape[0], w.shape[1]
    ksize = w.shape[2] if w.ndim == 4 else 1
    taps, bk = ksize * ksize, block_k(dtype)
    n_rows = n_out if n_rows is None else n_rows
    w3 = w.reshape(n_out, c_in, taps)
    np_ = torch.arange(n_pad, device=w.device)[:, None]
    k = torch.arange(k_pad, device=w.device)[None, :]
    if k_order:
        kt = k // bk
        cb, tap = kt // taps, kt % taps
        c = cb * bk + k % bk
    else:
        tap, c = k // c_pad, k % c_pad
    if transpose:
        ok = (np_ < n_rows) & (c < n_out) & (tap < taps)
        val = w3[c.clamp(max=n_out - 1), (c_off + np_).clamp(max=c_in - 1), (taps - 1 - tap).clamp(0, taps - 1)]
    else:
        n = geglu_row(np_, n_out) if geglu else np_
        ok = (np_ < n_out) & (n < n_out) & (c < c_in) & (tap < taps)
        val = w3[n.clamp(max=n_out - 1), c.clamp(max=c_in - 1), tap.clamp(max=taps - 1)]
    return torch.where(ok, val, torch.zeros((), device=w.device)).to(dtype)


def skinny_ref(packed, geglu=False):
    """the fragment-order copy of a 16-bit k_order-1 pack `[n_pad, k_pad]`: 16-byte unit ((nt * (k_pad/32) + kg) * 64 + lane) =
    packed[row(nt, lane & 15)][32 kg + 8 (lane >> 4) .. + 7]"""
    n_pad, k_pad = packed.shape
    assert packed.element_size() == 2 and n_pad % 64 == 0 and k_pad % 64 == 0
    units = packed.contiguous().view(torch.int16).reshape(n_pad, k_pad // 8, 8)
    nt = torch.arange(n_pad // 16, device=packed.device)[:, None, None]
    kg = torch.arange(k_pad // 32, device=packed.device)[None, :, None]
    lane = torch.arange(64, device=packed.device)[None, None, :]
    r = lane & 15
    if geglu:           # tiles (2q, 2q + 1): the value / gate rows of output columns o = 16 q + r; a column's value row is 64 (o / 32) + o % 32
        o = 16 * (nt // 2) + r
        row = 64 * (o // 32) + 32 * (nt % 2) + o % 32
    else:
        row = 16 * nt + r
    return units[row, 4 * kg + lane // 16].reshape(n_pad, k_pad).view(packed.dtype)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(got, want, what=""):
    """`got` equals `want` bit for bit; where `want` is NaN, `got` is some NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    nan = torch.isnan(want)
    bad = torch.where(nan, ~torch.isnan(got), bits(got) != bits(want))
    if bool(bad.any()):
        at = bad.nonzero()[0].tolist()
        g, x = got[tuple(at)], want[tuple(at)]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} packed elements differ, first at {at}: "
                             f"{float(g)!r} ({int(bits(g)) & 0xFFFFFFFF:#x}) for {float(x)!r} ({int(bits(x)) & 0xFFFFFFFF:#x})")


def _row_bytes(k_pad, dtype):
    return k_pad * torch.empty((), dtype=dtype).element_size()


def guarded(n_pad, k_pad, dtype, device):
    """a uint8 buffer of GUARD_BYTE: GUARD_ROWS rows of k_pad elements, the `[n_pad, k_pad]` destination (`interior`), GUARD_ROWS rows"""
    return torch.full(((n_pad + 2 * GUARD_ROWS) * _row_bytes(k_pad, dtype),), GUARD_BYTE, dtype=torch.uint8, device=device)


def interior(buf, n_pad, k_pad, dtype):
    row = _row_bytes(k_pad, dtype)
    assert buf.numel() == (n_pad + 2 * GUARD_ROWS) * row
    return buf[GUARD_ROWS * row:(GUARD_ROWS + n_pad) * row].view(dtype).view(n_pad, k_pad)


def check_packed(buf, want, what=""):
    """the guards of `buf` still hold GUARD_BYTE, and every element of its interior has the bits of `want` (`[n_pad, k_pad]`)"""
    g = GUARD_ROWS * _row_bytes(want.shape[1], want.dtype)
    for side, part in (("front", buf[:g]), ("back", buf[buf.numel() - g:])):
        hit = part != GUARD_BYTE
        if bool(hit.any()):
            raise AssertionError(f"{what}: {int(hit.sum())} guard bytes written in the {side} guard, first at byte {int(hit.nonzero()[0])} of {g}")
    same_bits(interior(buf, want.shape[0], want.shape[1], want.dtype), want, what)
