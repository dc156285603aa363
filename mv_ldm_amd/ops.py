"""Tensor-level wrappers over the C ABI (include/mvldm.h).  torch is plumbing here: device memory,
the current HIP stream and dtype tags.  Every function enqueues hand-written HIP kernels from
libmvldm_hip.so on `torch.cuda.current_stream()`; nothing falls back to torch math.

Conventions: activations are NHWC tensors `[n_img, h, w, c]` (or token matrices `[rows, c]`) in the
activation dtype; biases / norm parameters / statistics are fp32.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import struct
import zlib
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import math

import numpy as np
import torch

from . import _lib as L

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}


def dt(t) -> int:
    return _DT[t if isinstance(t, torch.dtype) else t.dtype]


def epc(dtype: torch.dtype) -> int:
    """elements per 16-byte chunk: channel counts must be multiples of this"""
    return 4 if dtype == torch.float32 else 8


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _roundup(a: int, b: int) -> int:
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------ workspaces
_WS: dict = {}


def workspace(nbytes: int, device, key: str = "splitk") -> torch.Tensor:
    """grow-only scratch buffer per (device, key); eager ops share it (stream-ordered reuse)."""
    k = (str(device), key)
    cur = _WS.get(k)
    if cur is None or cur.numel() < nbytes:
        cur = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[k] = cur
    return cur


# ------------------------------------------------------------------------------------------ weights
@dataclass
class PackedWeight:
    """K-major [n_pad][k_pad] weight in the activation dtype + what the kernel needs to know."""
    data: torch.Tensor
    n_out: int
    n_pad: int
    k_pad: int
    c_pad: int      # channels per tap as seen by the kernel (sum of source channels)
    ksize: int
    geglu: bool = False
    k_order: int = 0    # 1: K stored as (channel block, tap, channel) -- needs every source's channels % BK == 0
    _skinny: Optional[torch.Tensor] = None
    _skinny_pinned: bool = False     # an op of some plan points at the fragment-order copy: it stays with the pack (drop_skinny is a no-op)

    def can_skinny(self) -> bool:
        """does igemm tile 15 (csrc/skinny.hip) read this weight?  16-bit block-major packs whose channel count is a multiple of 64"""
        return self.k_order == 1 and self.data.dtype != torch.float32 and self.c_pad % 64 == 0 and self.k_pad == self.ksize * self.ksize * self.c_pad \
            and self.ksize in (1, 2, 3) and self.n_out % 4 == 0

    def skinny(self) -> torch.Tensor:
        """the same weight in MFMA-fragment order (`mvldm_pack_skinny`), made on first use from the K-major pack and kept with it: the
        operand of igemm tile 15.  A re-pack produces a new PackedWeight (modules._PackMixin), so the copy cannot go stale."""
        if self._skinny is None:
            assert self.can_skinny(), "tile 15 needs a 16-bit block-major pack with channels in multiples of 64"
            out = torch.empty_like(self.data)
            L.check(L.load().mvldm_pack_skinny(self.data.data_ptr(), out.data_ptr(), self.n_pad, self.k_pad, int(self.geglu), dt(self.data), stream()))
            self._skinny = out
        return self._skinny

    def drop_skinny(self):
        if not self._skinny_pinned:
            self._skinny = None


def block_k(dtype: torch.dtype) -> int:
    return 32 if dtype == torch.float32 else 64


def pack_weight_t(w: torch.Tensor, dtype: torch.dtype, c_off: int = 0, n_rows: Optional[int] = None,
                  out: Optional[torch.Tensor] = None) -> PackedWeight:
    """the weight of the DATA-GRADIENT convolution of `w` (fp32 `[n_out, c_in, k, k]` / `[n_out, c_in]`): rows = input
    channels [c_off, c_off + n_rows), K = (flipped tap, output channel).  Fed to the forward implicit GEMM with the
    upstream gradient as its source, it yields dL/dx (stride-1 convs and Linears).  `out`: repack in place."""
    assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    n_out, c_in = w.shape[0], w.shape[1]
    ksize = w.shape[2] if w.ndim == 4 else 1
    n_rows = c_in - c_off if n_rows is None else n_rows
    c_pad = _roundup(n_out, epc(dtype))
    bk = block_k(dtype)
    k_pad = _roundup(ksize * ksize * c_pad, bk)
    n_pad = _roundup(n_rows, 64)
    k_order = int(c_pad % bk == 0)
    data = torch.zeros(n_pad, k_pad, dtype=dtype, device=w.device) if out is None else out
    L.check(L.load().mvldm_pack_weight(w.data_ptr(), data.data_ptr(), n_out, c_in, ksize, c_pad, n_pad, k_pad, 0, k_order, dt(dtype),
                                       1, c_off, n_rows, stream()))
    return PackedWeight(data, n_rows, n_pad, k_pad, c_pad, ksize, False, k_order)


def pack_weight(w: torch.Tensor, dtype: torch.dtype, c_pad: Optional[int] = None, geglu: bool = False,
                c_split: Optional[int] = None, out: Optional[torch.Tensor] = None) -> PackedWeight:
    """w: fp32 `[n_out, c_in, k, k]` (conv) or `[n_out, c_in]` (linear), on the GPU.  `c_split`: channel
    count of the first of two concatenated sources (decides whether the block-major K order applies)."""
    assert w.is_cuda, "pack_weight needs a device tensor (no CPU path)"
    w = w.detach().to(torch.float32).contiguous()
    n_out, c_in = w.shape[0], w.shape[1]
    ksize = w.shape[2] if w.ndim == 4 else 1
    e = epc(dtype)
    c_pad = _roundup(c_in, e) if c_pad is None else c_pad
    bk = block_k(dtype)
    k_pad = _roundup(ksize * ksize * c_pad, bk)
    n_pad = _roundup(n_out, 64)
    k_order = int(c_pad % bk == 0 and (c_split is None or c_split % bk == 0))
    out = torch.empty(n_pad, k_pad, dtype=dtype, device=w.device) if out is None else out
    L.check(L.load().mvldm_pack_weight(w.data_ptr(), out.data_ptr(), n_out, c_in, ksize, c_pad, n_pad, k_pad,
                                       int(geglu), k_order, dt(dtype), 0, 0, n_out, stream()))
    return PackedWeight(out, n_out, n_pad, k_pad, c_pad, ksize, geglu, k_order)


def pack_job(w: torch.Tensor, pw: PackedWeight, *, transpose: bool = False, c_off: int = 0) -> "L.PackJob":
    """the re-pack of `pw` (made by `pack_weight` / `pack_weight_t` from the fp32 weight `w`) as one job of `PackBatch`"""
    assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    j = L.PackJob()
    j.src, j.dst = w.data_ptr(), pw.data.data_ptr()
    j.n_out, j.c_in, j.ksize = w.shape[0], w.shape[1], pw.ksize
    j.c_pad, j.n_pad, j.k_pad, j.geglu, j.k_order = pw.c_pad, pw.n_pad, pw.k_pad, int(pw.geglu), pw.k_order
    j.transpose, j.c_off, j.n_rows = int(transpose), c_off, (pw.n_out if transpose else w.shape[0])
    L.check(L.load().mvldm_pack_job_prepare(C.byref(j), dt(pw.data.dtype)))
    return j


class PackBatch:
    """many weight re-packs as ONE launch (`mvldm_pack_weight_batch`): the job list lives on the device, a workgroup finds its
    job by its first-workgroup index.  Same bytes out as one `pack_weight(..., out=)` call per job."""

    def __init__(self, jobs: Sequence["L.PackJob"], dtype: torch.dtype, device):
        self.n, self.dtype = len(jobs), dtype
        arr = (L.PackJob * max(len(jobs), 1))()
        b0 = 0
        for i, j in enumerate(jobs):
            C.memmove(C.byref(arr[i]), C.byref(j), C.sizeof(L.PackJob))
            arr[i].block0 = b0
            b0 += j.blocks
        self.total_blocks = b0
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
        self.table = raw.to(device)
        # workgroup -> job table (without it the kernel searches the job list: measured slower, HISTORY 3.2)
        self.block_job = None
        if jobs:
            self.block_job = torch.repeat_interleave(torch.arange(len(jobs), dtype=torch.int32), torch.tensor([j.blocks for j in jobs])).to(device)
            assert self.block_job.numel() == b0

    def run(self):
        L.check(L.load().mvldm_pack_weight_batch(self.table.data_ptr(), self.n, None if self.block_job is None else self.block_job.data_ptr(),
                                                 self.total_blocks, dt(self.dtype), stream()))


# ------------------------------------------------------------------------------------------ igemm
def conv_out_hw(h: int, w: int, ksize: int, stride: int, pad: int, upsample) -> tuple:
    """output size of a forward conv; `upsample`: 0 / 1 (nearest-2x in front), or 2 + phase (one phase conv: the low-resolution size)"""
    if int(upsample) >= 2:
        return h, w
    hs, ws = (2 * h, 2 * w) if upsample else (h, w)
    if ksize == 3 and stride == 2 and pad == 0:       # VAE encoder: F.pad(0,1,0,1) then stride-2 conv
        return (hs + 1 - 3) // 2 + 1, (ws + 1 - 3) // 2 + 1
    return (hs + 2 * pad - ksize) // stride + 1, (ws + 2 * pad - ksize) // stride + 1


def use_skinny(d, pw: PackedWeight) -> torch.Tensor:
    """point igemm descriptor `d` at the fragment-order copy of `pw` (what tile 15, csrc/skinny.hip, reads); returns the copy"""
    t = pw.skinny()
    d.weight, d.k_order = ptr(t), 2
    return t


def igemm_desc(src0, src1, pw: PackedWeight, dst, *, n_img, h_in, w_in, h_out, w_out, stride=1, pad=None, upsample=False,
               bias=None, row_bias=None, residual=None, epilogue=L.EPI_NONE, out_scale=1.0, ws=None, splitk=0,
               tile=0, into=None) -> L.IgemmDesc:
    """the one place an implicit-GEMM descriptor is filled: eager calls get a fresh one, a plan passes `into=op.u.igemm`.
    `upsample`: 0 / 1, or 2 + phase (see upsample_phase_weights); `ws`: split-K workspace (None: one K pass)."""
    d = L.IgemmDesc() if into is None else into
    c0 = src0.shape[-1]
    c1 = 0 if src1 is None else src1.shape[-1]
    assert c0 + c1 == pw.c_pad, f"weight packed for {pw.c_pad} channels, sources give {c0}+{c1}"
    assert not pw.k_order or c0 % block_k(src0.dtype) == 0, "weight packed block-major but the source split is unaligned"
    d.src0, d.src1, d.weight = ptr(src0), ptr(src1), ptr(pw.data)
    d.bias, d.row_bias, d.residual, d.dst = ptr(bias), ptr(row_bias), ptr(residual), ptr(dst)
    d.c0, d.c1 = c0, c1
    d.n_img, d.h_in, d.w_in, d.h_out, d.w_out = n_img, h_in, w_in, h_out, w_out
    d.ksize, d.stride, d.upsample = pw.ksize, stride, int(upsample)
    d.pad = (pw.ksize // 2) if pad is None else pad
    d.n_out, d.n_pad, d.k_pad = pw.n_out, pw.n_pad, pw.k_pad
    d.row_bias_ld = 0 if row_bias is None else row_bias.stride(0)
    d.epilogue, d.act_dtype, d.dst_dtype = epilogue, dt(src0), dt(dst)
    d.splitk, d.tile, d.out_scale = splitk, tile, out_scale
    n_dst = pw.n_out // 2 if epilogue == L.EPI_GEGLU else pw.n_out
    d.dst_ld = 0 if dst.shape[-1] == n_dst else dst.shape[-1]      # rows of a wider buffer
    d.k_order = pw.k_order
    if (tile & 63) == 15:       # the skinny weight-streaming kernel reads the fragment-order copy of the pack
        use_skinny(d, pw)
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    else:
        d.workspace, d.workspace_bytes = None, 0
        if splitk == 0:
            d.splitk = 1
    return d


def conv2d(x: torch.Tensor, pw: PackedWeight, bias=None, *, x2=None, stride=1, pad=None, upsample=False, row_bias=None,
           residual=None, epilogue=L.EPI_NONE, out_dtype=None, out_scale=1.0, splitk=0, tile=0, out=None, dst=None) -> torch.Tensor:
    """x: NHWC `[n, h, w, c]`; x2: optional second source concatenated along c.  Returns NHWC.  `out`: write into this tensor
    (it may be the residual: x += f(x)).  `dst`: rows of a WIDER buffer instead -- a contiguous `[n, ho, wo, dst_ld]` tensor with
    dst_ld > n_dst whose columns [0, n_dst) are written (`[n, 2 ho, 2 wo, dst_ld]` for a phase conv, which scatters); returned as is."""
    assert x.is_cuda and x.is_contiguous() and (x2 is None or x2.is_contiguous())
    n, h, w, _ = x.shape
    pad = (pw.ksize // 2) if pad is None else pad
    ho, wo = conv_out_hw(h, w, pw.ksize, stride, pad, upsample)
    n_dst = pw.n_out // 2 if epilogue == L.EPI_GEGLU else pw.n_out
    if dst is not None:
        up = 2 if int(upsample) >= 2 else 1
        assert out is None and dst.is_contiguous() and dst.dtype == (out_dtype or x.dtype) and dst.shape[-1] > n_dst
        assert dst.numel() == n * up * ho * up * wo * dst.shape[-1]
        out = dst
    elif out is None:
        out = torch.empty(n, ho, wo, n_dst, dtype=out_dtype or x.dtype, device=x.device)
    else:
        assert out.is_contiguous() and out.numel() == n * ho * wo * n_dst and out.dtype == (out_dtype or x.dtype)
        out = out.view(n, ho, wo, n_dst)
    scratch = None
    if splitk != 1:
        # split-K only pays when M*N is small: the C side lowers the split count to what fits
        scratch = workspace(min(16 * n * ho * wo * pw.n_pad * 4, 256 << 20), x.device)
    d = igemm_desc(x, x2, pw, out, n_img=n, h_in=h, w_in=w, h_out=ho, w_out=wo, stride=stride, pad=pad,
                   upsample=upsample, bias=bias, row_bias=row_bias, residual=residual, epilogue=epilogue,
                   out_scale=out_scale, ws=scratch, splitk=splitk, tile=tile)
    L.check(L.load().mvldm_igemm_fwd(C.byref(d), stream()))
    return out


def upsample_phase_weights(w: torch.Tensor) -> list:
    """nearest-2x upsampling followed by a 3x3 / pad-1 conv equals four 2x2 convs on the LOW-resolution image, one per
    output parity (py, px): output (2i+py, 2j+px) reads input rows {i-1+py, i+py} and columns {j-1+px, j+px} with the 3x3
    taps that land on the same source pixel pre-summed (rows: py=0 -> [w0, w1+w2], py=1 -> [w0+w1, w2]; columns alike).
    4/9 of the multiply-adds, exact up to the rounding of the summed weights.  Returns the fp32 `[n, c, 2, 2]` weights of
    phases 0..3 (phase = 2*py + px)."""
    assert w.ndim == 4 and w.shape[2:] == (3, 3)
    w = w.detach().to(torch.float32)
    rows = {0: (w[:, :, 0], w[:, :, 1] + w[:, :, 2]), 1: (w[:, :, 0] + w[:, :, 1], w[:, :, 2])}     # [n, c, 3(kx)] each
    out = []
    for py in (0, 1):
        for px in (0, 1):
            taps = []
            for r in rows[py]:
                cols = (r[:, :, 0], r[:, :, 1] + r[:, :, 2]) if px == 0 else (r[:, :, 0] + r[:, :, 1], r[:, :, 2])
                taps.append(torch.stack(cols, dim=-1))
            out.append(torch.stack(taps, dim=-2).contiguous())       # [n, c, 2(ky), 2(kx)]
    return out


def conv2d_upsample_phases(x: torch.Tensor, pws, bias=None, tile=0, splitk=0) -> torch.Tensor:
    """x NHWC `[n, h, w, c]` (16-bit); `pws`: the 4 packed phase weights -> NHWC `[n, 2h, 2w, n_out]`"""
    n, h, w, _ = x.shape
    out = torch.empty(n, 2 * h, 2 * w, pws[0].n_out, dtype=x.dtype, device=x.device)
    scratch = workspace(min(16 * n * h * w * pws[0].n_pad * 4, 256 << 20), x.device)
    for phase, pw in enumerate(pws):
        d = igemm_desc(x, None, pw, out, n_img=n, h_in=h, w_in=w, h_out=h, w_out=w, stride=1, pad=0, upsample=2 + phase,
                       bias=bias, splitk=splitk, tile=tile, ws=scratch)
        L.check(L.load().mvldm_igemm_fwd(C.byref(d), stream()))
    return out


def linear(x: torch.Tensor, pw: PackedWeight, bias=None, *, residual=None, epilogue=L.EPI_NONE, out_dtype=None,
           splitk=0, tile=0, out=None, dst=None) -> torch.Tensor:
    """x: `[rows, c]` token matrix.  `dst`: a contiguous `[rows, dst_ld]` buffer wider than the output (see conv2d)."""
    rows, c = x.shape
    y = conv2d(x.view(rows, 1, 1, c), pw, bias, residual=None if residual is None else residual.view(rows, 1, 1, -1),
               epilogue=epilogue, out_dtype=out_dtype, splitk=splitk, tile=tile, out=out, dst=None if dst is None else dst.view(rows, 1, 1, -1))
    return y.view(rows, -1)


# ------------------------------------------------------------------------------------------ norms
def groupnorm(x: torch.Tensor, gamma, beta, groups: int, eps: float, silu: bool, x2=None, stats_out=None, out=None) -> torch.Tensor:
    """x NHWC `[n, h, w, c]` (or `[n, hw, c]`); x2: optional second source concatenated along c.
    stats_out: optional fp32 `[n, groups, 2]` receiving (mean, rstd) for the backward pass.  `out`: write into this contiguous tensor."""
    assert x.is_cuda and x.is_contiguous() and (x2 is None or x2.is_contiguous())
    n, c0 = x.shape[0], x.shape[-1]
    c1 = 0 if x2 is None else x2.shape[-1]
    hw = math.prod(x.shape[1:-1])
    if out is None:
        y = torch.empty(*x.shape[:-1], c0 + c1, dtype=x.dtype, device=x.device)
    else:
        assert out.is_contiguous() and out.dtype == x.dtype and out.numel() == n * hw * (c0 + c1)
        y = out.view(*x.shape[:-1], c0 + c1)
    ws = workspace(max(n, 1) * L.GN_MAX_CHUNKS * groups * 2 * 8, x.device, "gn")
    L.check(L.load().mvldm_groupnorm_fwd(x.data_ptr(), ptr(x2), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), n, hw, c0, c1,
                                         groups, eps, int(silu), dt(x), ws.data_ptr(), ptr(stats_out), stream()))
    return y


def layernorm(x: torch.Tensor, gamma, beta, eps: float = 1e-5, out=None) -> torch.Tensor:
    assert x.is_cuda and x.is_contiguous()
    c = x.shape[-1]
    rows = x.numel() // c
    if out is None:
        y = torch.empty_like(x)
    else:
        assert out.is_contiguous() and out.dtype == x.dtype and out.numel() == x.numel()
        y = out.view(x.shape)
    L.check(L.load().mvldm_layernorm_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, c, eps,
                                         dt(x), stream()))
    return y


# ------------------------------------------------------------------------------------------ attention
def make_segments(q_lens, kv_lens=None, device="cuda") -> torch.Tensor:
    """contiguous segments -> int32 [n_seg, 4] = {q_row0, q_len, kv_row0, kv_len}"""
    kv_lens = q_lens if kv_lens is None else kv_lens
    rows, q0, k0 = [], 0, 0
    for ql, kl in zip(q_lens, kv_lens):
        rows.append([q0, ql, k0, kl])
        q0, k0 = q0 + ql, k0 + kl
    return torch.tensor(rows, dtype=torch.int32, device=device)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, head_dim: int, seg: torch.Tensor,
              max_q_len: int, scale: Optional[float] = None, lse: Optional[torch.Tensor] = None, out=None) -> torch.Tensor:
    """q/k/v: 2-D row-major views `[tokens, >= heads*head_dim]` (may be column slices of one fused
    projection: only the row stride is used).  Returns `[q_tokens, heads*head_dim]`.  `out`: write into this 2-D view (unit column
    stride, any row stride); `lse`: fp32 `[heads, >= q_tokens]` receiving the log2-domain log-sum-exp."""
    assert q.is_cuda and q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1
    if out is None:
        out = torch.empty(q.shape[0], heads * head_dim, dtype=q.dtype, device=q.device)
    assert out.stride(1) == 1 and out.dtype == q.dtype and out.shape[1] == heads * head_dim
    scale = head_dim ** -0.5 if scale is None else scale
    L.check(L.load().mvldm_attention_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), q.stride(0), k.stride(0),
                                         v.stride(0), out.stride(0), heads, head_dim, seg.data_ptr(), seg.shape[0],
                                         max_q_len, scale, dt(q), ptr(lse), 0 if lse is None else lse.stride(0), stream()))
    return out


def attention_merge(oa, lse_a, ob, lse_b, a_img, b_img, out_img, tokens: int, heads: int, head_dim: int, out=None) -> torch.Tensor:
    """combine two attention results of the same queries over disjoint key sets (`mvldm_attention_merge`).  oa / ob / out: 2-D views
    `[rows, >= heads*head_dim]` with unit column stride; lse_a / lse_b: fp32 `[heads, lse_ld]` (log2 domain, from `attention(lse=)`);
    a_img / b_img / out_img: int32 `[n_img]` image maps over images of `tokens` rows.  `out` may be oa or ob."""
    assert oa.is_cuda and oa.dtype == ob.dtype and oa.stride(1) == 1 and ob.stride(1) == 1
    assert all(t.dtype == torch.int32 and t.numel() == a_img.numel() for t in (a_img, b_img, out_img))
    if out is None:
        out = torch.empty(int(out_img.numel()) * tokens, heads * head_dim, dtype=oa.dtype, device=oa.device)
    assert out.stride(1) == 1 and out.dtype == oa.dtype
    L.check(L.load().mvldm_attention_merge(oa.data_ptr(), lse_a.data_ptr(), ob.data_ptr(), lse_b.data_ptr(), out.data_ptr(), a_img.data_ptr(),
                                           b_img.data_ptr(), out_img.data_ptr(), a_img.numel(), tokens, heads, head_dim, oa.stride(0), ob.stride(0),
                                           out.stride(0), lse_a.stride(0), lse_b.stride(0), dt(oa), stream()))
    return out


# ------------------------------------------------------------------------------------------ small ops
def gather_rows(src: torch.Tensor, dst: torch.Tensor, src_index=None, dst_index=None, n_rows: Optional[int] = None) -> torch.Tensor:
    """dst row (dst_index[k] or k) = src row (src_index[k] or k), k < n_rows (`mvldm_gather_rows`).  src / dst: contiguous 2-D
    tensors of equal row size (a multiple of 16 bytes); the index vectors are int32 device tensors.  src may be dst when no
    destination row is also a source row."""
    assert src.is_cuda and src.is_contiguous() and dst.is_contiguous() and src.dim() == 2 and dst.dim() == 2
    row_bytes = src.shape[1] * src.element_size()
    assert row_bytes == dst.shape[1] * dst.element_size()
    for t in (src_index, dst_index):
        assert t is None or (t.dtype == torch.int32 and t.is_cuda and t.is_contiguous())
    if n_rows is None:
        n_rows = src_index.numel() if src_index is not None else dst_index.numel() if dst_index is not None else min(src.shape[0], dst.shape[0])
    L.check(L.load().mvldm_gather_rows(src.data_ptr(), dst.data_ptr(), ptr(src_index), ptr(dst_index), n_rows, row_bytes, stream()))
    return dst


def timestep_embed(timesteps: torch.Tensor, freqs: torch.Tensor, dim: int, flip_sin_to_cos: bool,
                   dtype=torch.float32) -> torch.Tensor:
    assert timesteps.dtype == torch.int64 and timesteps.is_cuda
    out = torch.empty(timesteps.numel(), dim, dtype=dtype, device=timesteps.device)
    L.check(L.load().mvldm_timestep_embed_fwd(timesteps.data_ptr(), freqs.data_ptr(), out.data_ptr(), timesteps.numel(),
                                              dim, int(flip_sin_to_cos), dt(dtype), stream()))
    return out


def eltwise(x: torch.Tensor, op: int, out_dtype=None) -> torch.Tensor:
    assert x.is_cuda and x.is_contiguous()
    y = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    L.check(L.load().mvldm_eltwise_fwd(x.data_ptr(), y.data_ptr(), x.numel(), op, dt(x), dt(y), stream()))
    return y


def silu(x, out_dtype=None):
    return eltwise(x, L.ELT_SILU, out_dtype)


def convert(x, out_dtype):
    return eltwise(x, L.ELT_COPY, out_dtype)


def nchw_to_nhwc(src: torch.Tensor, dtype, dst: Optional[torch.Tensor] = None, c_off: int = 0,
                 dst_c: Optional[int] = None, scale: float = 1.0, shift: float = 0.0,
                 img_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 NCHW `[n, c, h, w]` -> NHWC `[n, h, w, dst_c]` (channels [c_off, c_off+c) written), `* scale + shift`;
    `img_map` (int32 `[n]`): source image i lands in destination image img_map[i]."""
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous()
    n, c, h, w = src.shape
    if dst is None:
        dst_c = c if dst_c is None else dst_c
        dst = torch.zeros(n, h, w, dst_c, dtype=dtype, device=src.device)
    L.check(L.load().mvldm_nchw_to_nhwc(src.data_ptr(), dst.data_ptr(), n, c, h * w, dst.shape[-1], c_off, dt(dst), scale, shift,
                                        ptr(img_map), stream()))
    return dst


def ray_channels(mode: int = 0, n_origin_octaves: int = 0, n_dir_octaves: int = 0) -> int:
    return int(L.load(required=False).mvldm_ray_channels(mode, n_origin_octaves, n_dir_octaves)) if L.load(required=False) is not None else \
        {0: 6, 1: (6 * n_origin_octaves or 3) + (6 * n_dir_octaves or 3), 2: 6 * (n_origin_octaves + n_dir_octaves)}[mode]


def ray_encode(extrinsics: torch.Tensor, intrinsics: torch.Tensor, h: int, w: int, out_nchw: Optional[torch.Tensor] = None,
               out_nhwc: Optional[torch.Tensor] = None, c_off: int = 0, img_map: Optional[torch.Tensor] = None,
               mode: int = 0, n_origin_octaves: int = 0, n_dir_octaves: int = 0, plucker: bool = False):
    """extrinsics fp32 `[n, 4, 4]` (camera-to-world), intrinsics fp32 `[n, 3, 3]` on the device -> per-pixel
    [origin | direction] of the `h x w` latent grid: fp32 `[n, 6, h, w]` and/or channels [c_off, c_off+6) of an NHWC
    buffer `[.., h, w, C]` (camera i -> image img_map[i])."""
    n = extrinsics.shape[0]
    assert extrinsics.is_cuda and extrinsics.dtype == torch.float32 and extrinsics.is_contiguous() and extrinsics.shape[1:] == (4, 4)
    assert intrinsics.dtype == torch.float32 and intrinsics.is_contiguous() and intrinsics.shape == (n, 3, 3)
    if out_nchw is None and out_nhwc is None:
        out_nchw = torch.empty(n, ray_channels(mode, n_origin_octaves, n_dir_octaves), h, w, dtype=torch.float32, device=extrinsics.device)
    L.check(L.load().mvldm_ray_encode(extrinsics.data_ptr(), intrinsics.data_ptr(), n, h, w, ptr(out_nchw), ptr(out_nhwc),
                                      0 if out_nhwc is None else out_nhwc.shape[-1], c_off,
                                      L.F32 if out_nhwc is None else dt(out_nhwc), ptr(img_map), mode, n_origin_octaves, n_dir_octaves,
                                      int(plucker), stream()))
    return out_nchw if out_nchw is not None else out_nhwc


def posterior_sample(moments: torch.Tensor, noise: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """moments fp32 NCHW `[n, 2c, h, w]` = [mean | logvar]; `(mean + exp(0.5 clamp(logvar, -30, 20)) * noise) * scale`"""
    n, c2, h, w = moments.shape
    assert moments.is_cuda and moments.dtype == torch.float32 and moments.is_contiguous()
    assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.numel() == n * (c2 // 2) * h * w
    out = torch.empty(n, c2 // 2, h, w, dtype=torch.float32, device=moments.device)
    L.check(L.load().mvldm_posterior_sample(moments.data_ptr(), noise.data_ptr(), out.data_ptr(), n, c2 // 2, h * w, scale, stream()))
    return out


def nhwc_to_nchw(src: torch.Tensor, c: Optional[int] = None, c_off: int = 0, scale=1.0, shift=0.0,
                 clamp01=False) -> torch.Tensor:
    assert src.is_cuda and src.is_contiguous()
    n, h, w, sc = src.shape
    c = sc if c is None else c
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=src.device)
    L.check(L.load().mvldm_nhwc_to_nchw(src.data_ptr(), out.data_ptr(), n, c, h * w, sc, c_off, dt(src), scale, shift,
                                        int(clamp01), stream()))
    return out


def ddim_cfg_step(eps, x_t, cond_img, uncond_img, cfg_scale, coef, step_ptr, unet_in=None, clip_range: float = 0.0) -> torch.Tensor:
    """eps: fp32 NHWC `[n_img, h, w, c]`; x_t: fp32 NHWC `[n_tgt, h, w, c]` -> x_{t-1} (same shape).
    coef: fp32 `[n_steps, 4]`; `clip_range` > 0 clamps the predicted x0 (diffusers `clip_sample`)."""
    n_tgt, h, w, c = x_t.shape
    out = torch.empty_like(x_t)
    L.check(L.load().mvldm_ddim_cfg_step(eps.data_ptr(), x_t.data_ptr(), out.data_ptr(), cond_img.data_ptr(), ptr(uncond_img),
                                         n_tgt, h * w, c, cfg_scale, coef.data_ptr(), step_ptr.data_ptr(), ptr(unet_in),
                                         0 if unet_in is None else unet_in.shape[-1],
                                         dt(unet_in) if unet_in is not None else L.F32, coef.shape[0], clip_range, stream()))
    return out


def ddpm_cfg_step(eps_c, eps_u, x_t, noise, cfg_scale, coef, clip_range: float = 0.0) -> torch.Tensor:
    """diffusers `DDPMScheduler.step` (epsilon, fixed_small) behind the optional CFG compose, on flat fp32 tensors of equal size.
    coef: device fp32 [5] = {sqrt(1-a_t), sqrt(a_t), c_x0, c_xt, sigma}; `noise` None when sigma = 0 (t = 0)."""
    for t in (eps_c, eps_u, x_t, noise):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == x_t.numel())
    out = torch.empty_like(x_t)
    L.check(L.load().mvldm_ddpm_cfg_step(eps_c.data_ptr(), ptr(eps_u), x_t.data_ptr(), ptr(noise), out.data_ptr(), x_t.numel(),
                                         cfg_scale, coef.data_ptr(), clip_range, stream()))
    return out


# ------------------------------------------------------------------------------------------ training kernels
def wgrad_desc(x, x2, dy, grad, ws, *, h_out, w_out, ksize, stride, pad, upsample, n_out, c_in=None, accumulate=False, form: int = 0,
               target: int = 0, into=None) -> L.WgradDesc:
    """the one place a weight-gradient descriptor is filled (`into=op.u.wgrad` for a plan).  `ws`: uint8 slab workspace;
    form: 0 = the library's rule, 1 = register-staged small tile, 2 = wide LDS-DMA tile (bits 8-9 of `accumulate`);
    target: workgroup target of the pixel split, 0 = the library's, else 64 << target (bits 10-12, as plan.autotune_wgrad writes them)"""
    assert 0 <= int(form) <= 3 and 0 <= int(target) <= 7, (form, target)
    d = L.WgradDesc() if into is None else into
    n, h, w, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[-1]
    d.src0, d.src1, d.dy, d.grad = ptr(x), ptr(x2), ptr(dy), ptr(grad)
    d.workspace, d.workspace_bytes = ptr(ws), ws.numel()
    d.c0, d.c1, d.c_in = c0, c1, (c0 + c1) if c_in is None else c_in
    d.n_img, d.h_in, d.w_in, d.h_out, d.w_out = n, h, w, h_out, w_out
    d.ksize, d.stride, d.pad, d.upsample = ksize, stride, pad, int(upsample)
    d.n_out, d.dy_ld, d.act_dtype, d.accumulate = n_out, dy.stride(-2), dt(x), int(accumulate) | (int(form) << 8) | (int(target) << 10)
    return d


def conv_wgrad(x, dy, grad, *, ksize, stride=1, pad=None, upsample=False, x2=None, c_in=None, accumulate=False, n_out=None, form: int = 0,
               target: int = 0, ws=None) -> torch.Tensor:
    """x (x2): NHWC forward input(s); dy: NHWC / `[m, ld]` upstream gradient (columns [0, n_out)); grad: fp32 PyTorch-layout
    weight gradient `[n_out, c_in, k, k]` / `[n_out, c_in]`, written or accumulated in place.  `ws`: a caller-owned uint8 slab
    workspace (its size caps the split count); default: the shared one, 8 slabs."""
    n, h, w, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[-1]
    pad = ksize // 2 if pad is None else pad
    hs, ws_ = (2 * h, 2 * w) if upsample else (h, w)
    ho, wo = (hs + 2 * pad - ksize) // stride + 1, (ws_ + 2 * pad - ksize) // stride + 1
    n_out = grad.shape[0] if n_out is None else n_out
    need = n_out * ksize * ksize * (c0 + c1) * 4
    if ws is None:
        scratch = workspace(min(max(need * 8, 1 << 20), max(need, 512 << 20)), x.device, "wgrad")
    else:
        assert ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.data_ptr() % 16 == 0
        scratch = ws
    d = wgrad_desc(x, x2, dy, grad, scratch, h_out=ho, w_out=wo, ksize=ksize, stride=stride, pad=pad, upsample=upsample, n_out=n_out,
                   c_in=c_in, accumulate=accumulate, form=form, target=target)
    L.check(L.load().mvldm_igemm_wgrad(C.byref(d), stream()))
    return grad


def colsum(x2d, dst, rows_per_seg=None, per_seg=False, accumulate=False, n=None) -> torch.Tensor:
    rows = x2d.shape[0]
    n = x2d.shape[1] if n is None else n
    rows_per_seg = rows if rows_per_seg is None else rows_per_seg
    n_seg = rows // rows_per_seg
    ws = workspace(max((1024 + n_seg) * ((n + 7) // 8 * 8) * 4, 1 << 16), x2d.device, "colsum")
    L.check(L.load().mvldm_colsum(x2d.data_ptr(), dst.data_ptr(), ws.data_ptr(), ws.numel(), n_seg, rows_per_seg, n, x2d.stride(0),
                                  dst.stride(0) if dst.ndim == 2 else n, int(per_seg), int(accumulate), dt(x2d), stream()))
    return dst


def groupnorm_bwd(x, dy, gamma, beta, stats, dgamma, dbeta, groups, silu, x2=None):
    n, c0 = x.shape[0], x.shape[-1]
    c1 = 0 if x2 is None else x2.shape[-1]
    hw = math.prod(x.shape[1:-1])
    dx, dx2 = torch.empty_like(x), (None if x2 is None else torch.empty_like(x2))
    ws = workspace(n * (L.GN_MAX_CHUNKS * (c0 + c1) + groups) * 2 * 4, x.device, "gnb")
    L.check(L.load().mvldm_groupnorm_bwd(x.data_ptr(), ptr(x2), dy.data_ptr(), dx.data_ptr(), ptr(dx2), gamma.data_ptr(), beta.data_ptr(),
                                         stats.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, hw, c0, c1, groups, int(silu), dt(x),
                                         ws.data_ptr(), ws.numel(), stream()))
    return dx, dx2


def layernorm_bwd(x, dy, gamma, dgamma, dbeta, eps=1e-5):
    c = x.shape[-1]
    rows = x.numel() // c
    dx = torch.empty_like(x)
    ws = workspace(512 * c * 2 * 4, x.device, "lnb")
    L.check(L.load().mvldm_layernorm_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), gamma.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                         rows, c, eps, dt(x), ws.data_ptr(), ws.numel(), stream()))
    return dx


def attn_bwd_desc(q, k, v, out, dout, dq, dk, dv, lse, delta, seg, *, heads, head_dim, max_q_len, max_kv_len, scale=None,
                  into=None) -> L.AttnBwdDesc:
    """the one place an attention-backward descriptor is filled (`into=op.u.attention_bwd` for a plan).  q / k / v and their
    gradients are 2-D views with unit column stride (column slices of a fused projection: only the row strides are used)."""
    d = L.AttnBwdDesc() if into is None else into
    d.q, d.k, d.v, d.out, d.dout, d.dq, d.dk, d.dv = (t.data_ptr() for t in (q, k, v, out, dout, dq, dk, dv))
    d.lse, d.delta, d.seg = lse.data_ptr(), delta.data_ptr(), seg.data_ptr()
    d.ld_q, d.ld_k, d.ld_v, d.ld_o, d.ld_do, d.ld_dq, d.ld_dk, d.ld_dv = (t.stride(0) for t in (q, k, v, out, dout, dq, dk, dv))
    d.heads, d.head_dim, d.n_seg, d.max_q_len, d.max_kv_len = heads, head_dim, seg.shape[0], max_q_len, max_kv_len
    d.total_q_rows, d.stat_ld, d.dtype = q.shape[0], lse.stride(0), dt(q)
    d.scale = head_dim ** -0.5 if scale is None else scale
    return d


def attention_bwd(q, k, v, out, dout, lse, heads, head_dim, seg, max_q_len, max_kv_len, scale=None, dqkv=None):
    """returns (dq, dk, dv) `[tokens, heads*head_dim]` (views of `dqkv` `[tokens, 3C]` when given)"""
    C_ = heads * head_dim
    if dqkv is None:
        dq, dk, dv = (torch.empty(t.shape[0], C_, dtype=q.dtype, device=q.device) for t in (q, k, v))
    else:
        dq, dk, dv = dqkv[:, :C_], dqkv[:, C_:2 * C_], dqkv[:, 2 * C_:]
    delta = torch.empty_like(lse)
    d = attn_bwd_desc(q, k, v, out, dout, dq, dk, dv, lse, delta, seg, heads=heads, head_dim=head_dim, max_q_len=max_q_len,
                      max_kv_len=max_kv_len, scale=scale)
    L.check(L.load().mvldm_attention_bwd(C.byref(d), stream()))
    return dq, dk, dv


def train_eltwise(op: int, a, b, out, rows: int, d: int):
    L.check(L.load().mvldm_train_eltwise(op, a.data_ptr(), ptr(b), out.data_ptr(), rows, d, dt(a), dt(out), stream()))
    return out


def silu_bwd(x, dy):
    return train_eltwise(L.TE_SILU_BWD, x, dy, torch.empty_like(dy), 1, x.numel())


def geglu_fwd(ag):
    rows, d2 = ag.shape
    return train_eltwise(L.TE_GEGLU_FWD, ag, None, torch.empty(rows, d2 // 2, dtype=ag.dtype, device=ag.device), rows, d2 // 2)


def geglu_bwd(ag, dh):
    rows, d2 = ag.shape
    return train_eltwise(L.TE_GEGLU_BWD, ag, dh, torch.empty_like(ag), rows, d2 // 2)


def pool2x2_sum(du):
    n, h2, w2, c = du.shape
    dx = torch.empty(n, h2 // 2, w2 // 2, c, dtype=du.dtype, device=du.device)
    L.check(L.load().mvldm_pool2x2_sum(du.data_ptr(), dx.data_ptr(), n, h2 // 2, w2 // 2, c, dt(du), stream()))
    return dx


def zero_insert2x(x):
    n, h, w, c = x.shape
    out = torch.empty(n, 2 * h, 2 * w, c, dtype=x.dtype, device=x.device)
    L.check(L.load().mvldm_zero_insert2x(x.data_ptr(), out.data_ptr(), n, h, w, c, dt(x), stream()))
    return out


def _grad_norm(g, n: int, max_norm: float, norm_out, sumsq_in, amp_state):
    ws = workspace(1024 * 8, g.device, "norm")
    args = (g.data_ptr(), n, ptr(sumsq_in), max_norm, norm_out.data_ptr())
    if amp_state is None:
        L.check(L.load().mvldm_grad_norm(*args, ws.data_ptr(), stream()))
    else:
        L.check(L.load().mvldm_grad_norm_amp(*args, amp_state.data_ptr(), ws.data_ptr(), stream()))
    return norm_out


def grad_norm(flat_grad, max_norm: float, norm_out=None, sumsq_in=None, amp_state=None):
    """norm_out fp32 [4]: [total norm, clip coefficient, this buffer's sum of squares, -].  `amp_state` (mvldm_amp_state, int32 [8] device
    tensor): the gradients carry that record's loss scale -- norm, coefficient and sum of squares are those of the UNSCALED gradients,
    and the record's found_inf is set when the total is not finite"""
    norm_out = torch.zeros(4, dtype=torch.float32, device=flat_grad.device) if norm_out is None else norm_out
    return _grad_norm(flat_grad, flat_grad.numel(), max_norm, norm_out, sumsq_in, amp_state)


def clip_from_sumsq(sumsq, max_norm: float, norm_out, amp_state=None):
    """total norm + clip coefficient (+ found_inf under `amp_state`) from an already all-reduced, unscaled sum of squares (fp32 [1]):
    the same kernels on an empty buffer"""
    return _grad_norm(sumsq, 0, max_norm, norm_out, sumsq, amp_state)


def adamw_step(p, g, m, v, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step=1, grad_scale=1.0, clip=None, amp_state=None):
    """`amp_state`: the step count (`step` is not used), 1/S and the skip decision are read from the loss scaler's device record"""
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel() for t in (p, g, m, v))
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, betas[0], betas[1], eps, weight_decay)
    if amp_state is None:
        L.check(L.load().mvldm_adamw_step(*args, step, grad_scale, ptr(clip), stream()))
    else:
        L.check(L.load().mvldm_adamw_step_amp(*args, grad_scale, ptr(clip), amp_state.data_ptr(), stream()))


def amp_update(amp_state, growth_factor: float, backoff_factor: float, growth_interval: int):
    """torch._amp_update_scale_ on the record (one launch); also advances AdamW's step count on a taken step and clears found_inf"""
    L.check(L.load().mvldm_amp_update(amp_state.data_ptr(), float(growth_factor), float(backoff_factor), int(growth_interval), stream()))


def ema_update(avg, p, weight: float):
    """avg.lerp_(p, weight) on flat fp32 buffers (torch.optim.swa_utils EMA: weight = 1 - decay)"""
    assert avg.dtype == p.dtype == torch.float32 and avg.is_contiguous() and p.is_contiguous() and avg.numel() == p.numel()
    L.check(L.load().mvldm_ema_update(avg.data_ptr(), p.data_ptr(), avg.numel(), float(weight), stream()))


# ------------------------------------------------------------------------------------------ image metrics
IMAGE_METRICS_TILE = 32          # csrc/metrics.hip kTile: the output tile edge of one workgroup (the tests pick shapes around it)
IMAGE_METRICS_WINDOW = 11


def image_metrics_workspace_bytes(n_img: int, c: int, h: int, w: int) -> int:
    return int(L.load().mvldm_image_metrics_workspace_bytes(n_img, c, h, w))


def image_metrics(pred: torch.Tensor, gt: torch.Tensor, use_sample_covariance: bool = True, out=None, ws: Optional[torch.Tensor] = None):
    """(psnr, ssim), fp32 `[n_img]` each, of the image pairs `pred`, `gt` `[n_img, c, h, w]` (compute_psnr / compute_ssim,
    src/evaluation/metrics.py:17-24, 58-73; csrc/metrics.hip).  fp32 contiguous inputs are read in place; bf16 / f16 go through the
    elementwise convert first; anything else (uint8, strided views) is refused.  `out` = (psnr, ssim) and `ws` (uint8, at least
    `image_metrics_workspace_bytes`) let a captured graph own its buffers; by default the shared grow-only workspace is used."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not t.is_cuda:
            raise RuntimeError("mv_ldm_amd modules run only on a HIP device (no CPU fallback): move the module and its inputs to 'cuda'")
        if t.dim() != 4:
            raise ValueError(f"image_metrics: {name} must be [n_img, c, h, w], got {tuple(t.shape)}")
        if t.dtype not in _DT:
            raise TypeError(f"image_metrics: {name} is {t.dtype}; float32, bfloat16 or float16 images in [0, 1] are scored")
        if not t.is_contiguous():
            raise ValueError(f"image_metrics: {name} must be contiguous NCHW (got strides {t.stride()}); call .contiguous() first")
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError(f"image_metrics: pred {tuple(pred.shape)} on {pred.device} against gt {tuple(gt.shape)} on {gt.device}")
    pred = pred if pred.dtype == torch.float32 else convert(pred, torch.float32)
    gt = gt if gt.dtype == torch.float32 else convert(gt, torch.float32)
    n, c, h, w = pred.shape
    psnr, ssim = out if out is not None else (torch.empty(n, dtype=torch.float32, device=pred.device) for _ in range(2))
    assert psnr.dtype == ssim.dtype == torch.float32 and psnr.numel() == ssim.numel() == n and psnr.is_contiguous() and ssim.is_contiguous()
    need = image_metrics_workspace_bytes(n, c, h, w)
    if ws is None:
        ws = workspace(need, pred.device, "metrics")
    L.check(L.load().mvldm_image_metrics(pred.data_ptr(), gt.data_ptr(), n, c, h, w, int(bool(use_sample_covariance)), psnr.data_ptr(),
                                         ssim.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), stream()))
    return psnr, ssim


# ------------------------------------------------------------------------------------------ LPIPS glue (csrc/lpips.hip)
LPIPS_CHANNELS = (64, 128, 256, 512, 512)      # the five taps of LPIPS(net="vgg"): relu1_2, 2_2, 3_3, 4_3, 5_3
LPIPS_MIN_EDGE = 16                            # four 2x2 pools must leave one pixel


def lpips_workspace_bytes(n_img: int, h: int, w: int) -> int:
    """bytes of fp64 partials `lpips_tap` x 5 + `lpips_fold` need for `n_img` pairs of h x w images; 0 for a refused shape"""
    return int(L.load().mvldm_lpips_workspace_bytes(n_img, h, w))


def lpips_tap_slots(h: int, w: int, c: int) -> int:
    """partials (workgroups) per image of one tap over an h x w map of c channels; 0 for a refused map"""
    return int(L.load().mvldm_lpips_tap_slots(h, w, c))


def lpips_prep(in0: torch.Tensor, in1: torch.Tensor, dtype: torch.dtype, normalize: bool) -> torch.Tensor:
    """two fp32 NCHW `[n, 3, h, w]` -> NHWC `[2n, h, w, c_pad]` in `dtype` (rows [0, n): in0), through the package's ScalingLayer"""
    n, _, h, w = in0.shape
    dst = torch.empty(2 * n, h, w, epc(dtype), dtype=dtype, device=in0.device)
    L.check(L.load().mvldm_lpips_prep(in0.data_ptr(), in1.data_ptr(), dst.data_ptr(), n, h, w, dst.shape[-1], dt(dtype), int(bool(normalize)), stream()))
    return dst


def relu_(x: torch.Tensor) -> torch.Tensor:
    """in-place ReLU of a contiguous conv output (the C entry keeps the name of its first user, LPIPS)"""
    assert x.is_cuda and x.is_contiguous()
    L.check(L.load().mvldm_lpips_relu(x.data_ptr(), x.numel(), dt(x), stream()))
    return x


lpips_relu = relu_


def lpips_tap(feat: torch.Tensor, weight: torch.Tensor, ws: torch.Tensor, slot0: int, slots: int, pool: bool = True) -> Optional[torch.Tensor]:
    """feat: the pre-activation NHWC `[2n, h, w, c]` output of a stage's last conv; weight: fp32 `[c]`.  Writes the stage's distance
    partials of the n pairs to slots [slot0, slot0 + lpips_tap_slots) of `ws` (uint8, `slots` fp64 per image) and returns the 2x2
    max-pooled ReLU map `[2n, h // 2, w // 2, c]` (None when `pool` is False: the last tap)"""
    assert feat.is_cuda and feat.is_contiguous() and feat.dim() == 4 and feat.shape[0] % 2 == 0
    assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == feat.shape[-1]
    n2, h, w, c = feat.shape
    pooled = torch.empty(n2, h // 2, w // 2, c, dtype=feat.dtype, device=feat.device) if pool else None
    L.check(L.load().mvldm_lpips_tap(feat.data_ptr(), weight.data_ptr(), ptr(pooled), n2 // 2, h, w, c, dt(feat), ws.data_ptr(),
                                     ws.numel() * ws.element_size(), slot0, slots, stream()))
    return pooled


def lpips_fold(ws: torch.Tensor, n_img: int, h: int, w: int, out: torch.Tensor) -> torch.Tensor:
    """out fp32 `[n_img]` (any shape of n_img elements) = the five layer means of the partials in `ws`, summed"""
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n_img
    L.check(L.load().mvldm_lpips_fold(ws.data_ptr(), ws.numel() * ws.element_size(), n_img, h, w, out.data_ptr(), stream()))
    return out


# ------------------------------------------------------------------------------------------ DISTS glue (csrc/dists.hip)
DISTS_CHANNELS = (3, 64, 128, 256, 512, 512)   # the six taps of DISTS: the raw image, relu1_2, 2_2, 3_3, 4_3, 5_3 (1475 channels)
DISTS_SUMS = 5                                 # sum a, sum b, sum a^2, sum b^2, sum a b


def dists_workspace_bytes(n_img: int, h: int, w: int) -> int:
    """bytes of fp64 partials `dists_stats` x 6 + `dists_fold` need for `n_img` pairs of h x w images; 0 for a refused shape"""
    return int(L.load().mvldm_dists_workspace_bytes(n_img, h, w))


def dists_stat_slots(h: int, w: int, c: int) -> int:
    """partials (workgroups) per pair of one tap over an h x w map of c channels; 0 for a refused map"""
    return int(L.load().mvldm_dists_stat_slots(h, w, c))


def dists_layout(h: int, w: int):
    """([(h_k, w_k, c_k, offset_k)] of the six taps, doubles per pair): the workspace layout `dists_fold` reads"""
    taps, off, hk, wk = [], 0, h, w
    for k, c in enumerate(DISTS_CHANNELS):
        if k >= 2:
            hk, wk = (hk + 1) // 2, (wk + 1) // 2
        taps.append((hk, wk, c, off))
        off += dists_stat_slots(hk, wk, c) * DISTS_SUMS * c
    return taps, off


def dists_prep(in0: torch.Tensor, in1: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """two fp32 NCHW `[n, 3, h, w]` in [0, 1] -> NHWC `[2n, h, w, c_pad]` in `dtype` (rows [0, n): in0), (x - mean) / std"""
    n, _, h, w = in0.shape
    dst = torch.empty(2 * n, h, w, epc(dtype), dtype=dtype, device=in0.device)
    L.check(L.load().mvldm_dists_prep(in0.data_ptr(), in1.data_ptr(), dst.data_ptr(), n, h, w, dst.shape[-1], dt(dtype), stream()))
    return dst


def dists_stats(feat: torch.Tensor, ws: torch.Tensor, offset: int, stride: int, feat_b: Optional[torch.Tensor] = None) -> None:
    """feat: the pre-activation NHWC `[2n, h, w, c]` output of a stage's last conv -- or, with `feat_b`, the two raw fp32 NCHW
    `[n, 3, h, w]` inputs (tap 0).  Writes the five fp64 sums per (pair, workgroup, channel) to doubles [offset, offset +
    dists_stat_slots * 5 * c) of each pair's `stride` doubles in `ws` (uint8)"""
    assert feat.is_cuda and feat.is_contiguous() and feat.dim() == 4
    if feat_b is None:
        assert feat.shape[0] % 2 == 0
        n2, h, w, c = feat.shape
        n = n2 // 2
    else:
        assert feat_b.is_contiguous() and feat_b.shape == feat.shape and feat.dtype == feat_b.dtype == torch.float32
        n, c, h, w = feat.shape
    L.check(L.load().mvldm_dists_stats(feat.data_ptr(), ptr(feat_b), n, h, w, c, dt(feat), ws.data_ptr(), ws.numel() * ws.element_size(),
                                       offset, stride, stream()))


def dists_l2pool(feat: torch.Tensor) -> torch.Tensor:
    """the pre-activation NHWC `[2n, h, w, c]` -> `[2n, ceil(h / 2), ceil(w / 2), c]`: sqrt(3x3 Hann-weighted mean of relu(feat)^2 + 1e-12), stride 2"""
    assert feat.is_cuda and feat.is_contiguous() and feat.dim() == 4 and feat.shape[0] % 2 == 0
    n2, h, w, c = feat.shape
    out = torch.empty(n2, (h + 1) // 2, (w + 1) // 2, c, dtype=feat.dtype, device=feat.device)
    L.check(L.load().mvldm_dists_l2pool(feat.data_ptr(), out.data_ptr(), n2 // 2, h, w, c, dt(feat), stream()))
    return out


def dists_fold(ws: torch.Tensor, n_img: int, h: int, w: int, alpha: torch.Tensor, beta: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out fp32 `[n_img]` = the DISTS score of each pair from the partials in `ws`; alpha, beta: fp32, 1475 elements each, in tap order"""
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n_img
    for t in (alpha, beta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == sum(DISTS_CHANNELS)
    L.check(L.load().mvldm_dists_fold(ws.data_ptr(), ws.numel() * ws.element_size(), n_img, h, w, alpha.data_ptr(), beta.data_ptr(),
                                      out.data_ptr(), stream()))
    return out


# ------------------------------------------------------------------------------------------ FID glue (csrc/fid.hip)
FID_FEATURES = 64                              # feature=64: Inception-v3 after its first max-pool
FID_STATE = 1 + FID_FEATURES + FID_FEATURES * FID_FEATURES      # doubles of one side's running state: count, sum f, sum f^T f
FID_INFO = 8                                   # doubles of `fid_compute`'s record


def fid_workspace_bytes(n_img: int, h: int, w: int, c: int = FID_FEATURES) -> int:
    """bytes of fp64 `fid_pool` + `fid_accumulate` need for `n_img` pre-pool maps of h x w x c: the partials, then the features; 0 for
    a refused shape"""
    return int(L.load().mvldm_fid_workspace_bytes(n_img, h, w, c))


def fid_pool_slots(h: int, w: int, c: int) -> int:
    """partials (workgroups) per image of the pool over an h x w map of c channels; 0 for a refused map"""
    return int(L.load().mvldm_fid_pool_slots(h, w, c))


def fid_prep(imgs: torch.Tensor, dtype: torch.dtype, oh: int = 299, ow: int = 299) -> torch.Tensor:
    """fp32 in [0, 1] or uint8 NCHW `[n, 3, h, w]` -> NHWC `[n, oh, ow, c_pad]` in `dtype`: the package's byte quantisation, the
    TensorFlow-1 bilinear resize, (x - 128) / 128"""
    assert imgs.is_cuda and imgs.is_contiguous() and imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.dtype in (torch.float32, torch.uint8)
    n, _, h, w = imgs.shape
    dst = torch.empty(n, oh, ow, epc(dtype), dtype=dtype, device=imgs.device)
    L.check(L.load().mvldm_fid_prep(imgs.data_ptr(), int(imgs.dtype == torch.uint8), dst.data_ptr(), n, h, w, oh, ow, dst.shape[-1], dt(dtype), stream()))
    return dst


def fid_pool(feat: torch.Tensor, ws: torch.Tensor) -> None:
    """feat: the pre-activation NHWC `[n, h, w, c]`.  ReLU, max-pool 3x3 / 2, and the fp64 sum of the pooled map per channel: doubles
    `[n, fid_pool_slots, c]` at the start of `ws` (uint8)"""
    assert feat.is_cuda and feat.is_contiguous() and feat.dim() == 4
    n, h, w, c = feat.shape
    L.check(L.load().mvldm_fid_pool(feat.data_ptr(), n, h, w, c, dt(feat), ws.data_ptr(), ws.numel() * ws.element_size(), stream()))


def fid_accumulate(ws: torch.Tensor, n_img: int, h: int, w: int, c: int, state: Optional[torch.Tensor],
                   features: Optional[torch.Tensor] = None) -> None:
    """folds `fid_pool`'s partials in `ws` to the fp64 features `[n_img, c]` (written to `features` if given) and adds them to `state`
    (fp64, 1 + c + c c: count, sum f, sum f^T f; None: the features only)"""
    for t, numel in ((state, 1 + c + c * c), (features, n_img * c)):
        assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.numel() == numel)
    L.check(L.load().mvldm_fid_accumulate(ws.data_ptr(), ws.numel() * ws.element_size(), n_img, h, w, c, ptr(features), ptr(state), stream()))


def fid_compute(state1: torch.Tensor, state2: torch.Tensor, out: torch.Tensor, info: torch.Tensor) -> torch.Tensor:
    """out (fp32, one element) = the Frechet distance of two states of 64 features; info (fp64 `[FID_INFO]`): sweeps and final relative
    off-diagonal norm of the first solve, of the second, solves that stopped at the sweep cap (then `out` is NaN), the score in fp64,
    sum sqrt(lambda), |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2"""
    for t in (state1, state2):
        assert t.dtype == torch.float64 and t.is_contiguous()
    c = int(round((-1 + (1 + 4 * (state1.numel() - 1)) ** 0.5) / 2))
    assert state1.numel() == state2.numel() == 1 + c + c * c
    assert out.dtype == torch.float32 and out.numel() == 1 and info.dtype == torch.float64 and info.is_contiguous() and info.numel() == FID_INFO
    L.check(L.load().mvldm_fid_compute(state1.data_ptr(), state2.data_ptr(), c, out.data_ptr(), info.data_ptr(), stream()))
    return out


# ------------------------------------------------------------------------------------------ Clean-FID glue (csrc/inception.hip)
FRECHET_MAX_D = 2048                           # the widest feature vector `frechet_compute` takes (Inception-v3's pool3)


def frechet_state_size(d: int) -> int:
    """doubles of one side's running state at width d: count, sum f, sum f^T f"""
    return 1 + d + d * d


def inception_workspace_bytes(n_img: int, h: int, ow: int) -> int:
    """bytes `inception_prep` needs for n_img images of height h resized to width ow: the horizontal pass's float32 output"""
    return int(L.load().mvldm_inception_workspace_bytes(n_img, h, ow))


def inception_prep(imgs: torch.Tensor, dtype: torch.dtype, oh: int = 299, ow: int = 299, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 or fp32-in-[0, 1] NCHW `[n, 3, h, w]` -> NHWC `[n, oh, ow, c_pad]` in `dtype`: PIL's bicubic on float32 planes as clean-fid's
    "clean" mode calls it, clip to [0, 255], (x - 128) / 128.  A float image is multiplied by 255 and not quantised."""
    assert imgs.is_cuda and imgs.is_contiguous() and imgs.dim() == 4 and imgs.shape[1] == 3 and imgs.dtype in (torch.float32, torch.uint8)
    n, _, h, w = imgs.shape
    dst = torch.empty(n, oh, ow, epc(dtype), dtype=dtype, device=imgs.device)
    if ws is None:
        ws = workspace(inception_workspace_bytes(n, h, ow), imgs.device, "cleanfid")
    L.check(L.load().mvldm_inception_prep(imgs.data_ptr(), int(imgs.dtype == torch.uint8), dst.data_ptr(), n, h, w, oh, ow, dst.shape[-1], dt(dtype),
                                          ws.data_ptr(), ws.numel() * ws.element_size(), stream()))
    return dst


def inception_unfold(x: torch.Tensor, kh: int, kw: int) -> torch.Tensor:
    """NHWC `[n, h, w, c]` -> `[n, h, w, kh kw c]`: the kh x kw window around each pixel (padding kh // 2, kw // 2), tap-major then
    channel, zero outside the map"""
    assert x.is_cuda and x.is_contiguous() and x.dim() == 4
    n, h, w, c = x.shape
    out = torch.empty(n, h, w, kh * kw * c, dtype=x.dtype, device=x.device)
    L.check(L.load().mvldm_inception_unfold(x.data_ptr(), out.data_ptr(), n, h, w, c, kh, kw, kh // 2, kw // 2, dt(x), stream()))
    return out


def _slice_of(dst: Optional[torch.Tensor], c_off: int, n: int, oh: int, ow: int, c: int, like: torch.Tensor):
    if dst is None:
        assert c_off == 0
        return torch.empty(n, oh, ow, c, dtype=like.dtype, device=like.device)
    assert dst.is_cuda and dst.is_contiguous() and dst.dtype == like.dtype and tuple(dst.shape[:3]) == (n, oh, ow) and c_off + c <= dst.shape[-1]
    return dst


def inception_maxpool(x: torch.Tensor, stride: int, pad: int, dst: Optional[torch.Tensor] = None, c_off: int = 0) -> torch.Tensor:
    """3 x 3 max-pool of NHWC `[n, h, w, c]` (padding as -inf, floored size) into channels [c_off, c_off + c) of `dst` (a new map if None)"""
    assert x.is_cuda and x.is_contiguous() and x.dim() == 4
    n, h, w, c = x.shape
    out = _slice_of(dst, c_off, n, (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1, c, x)
    L.check(L.load().mvldm_inception_maxpool(x.data_ptr(), out.data_ptr(), n, h, w, c, stride, pad, out.shape[-1], c_off, dt(x), stream()))
    return out


def inception_avgpool(x: torch.Tensor, dst: Optional[torch.Tensor] = None, c_off: int = 0) -> torch.Tensor:
    """3 x 3 / stride 1 / padding 1 average of NHWC `[n, h, w, c]`, divided by the taps inside the map, into a channel slice of `dst`"""
    assert x.is_cuda and x.is_contiguous() and x.dim() == 4
    n, h, w, c = x.shape
    out = _slice_of(dst, c_off, n, h, w, c, x)
    L.check(L.load().mvldm_inception_avgpool(x.data_ptr(), out.data_ptr(), n, h, w, c, out.shape[-1], c_off, dt(x), stream()))
    return out


def inception_concat(x: torch.Tensor, dst: torch.Tensor, c_off: int, relu: bool = False) -> torch.Tensor:
    """the contiguous NHWC `x` (ReLU applied if asked) into channels [c_off, c_off + c) of the wider NHWC `dst`"""
    assert x.is_cuda and x.is_contiguous() and dst.is_contiguous() and dst.dtype == x.dtype and dst.shape[:-1] == x.shape[:-1]
    c = x.shape[-1]
    assert c_off + c <= dst.shape[-1]
    L.check(L.load().mvldm_inception_concat(x.data_ptr(), dst.data_ptr(), x.numel() // c, c, dst.shape[-1], c_off, int(bool(relu)), dt(x), stream()))
    return dst


def inception_features(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """NHWC `[n, h, w, c]` -> out fp64 `[n, c]`: the mean over the map, fp64 from the first add"""
    assert x.is_cuda and x.is_contiguous() and x.dim() == 4
    n, h, w, c = x.shape
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == n * c
    L.check(L.load().mvldm_inception_features(x.data_ptr(), n, h, w, c, dt(x), out.data_ptr(), stream()))
    return out


def frechet_accumulate(features: torch.Tensor, state: torch.Tensor) -> None:
    """state (fp64, 1 + d + d d: count, sum f, sum f^T f) += the rows of `features` (fp64 `[n, d]`), in order"""
    assert features.dtype == torch.float64 and features.is_contiguous() and features.dim() == 2
    n, d = features.shape
    assert state.dtype == torch.float64 and state.is_contiguous() and state.numel() == frechet_state_size(d)
    L.check(L.load().mvldm_frechet_accumulate(features.data_ptr(), n, d, state.data_ptr(), stream()))


def frechet_workspace_bytes(d: int) -> int:
    """bytes `frechet_compute` needs at width d (four d x d fp64 matrices and a little more); 0 for a refused width"""
    return int(L.load().mvldm_frechet_workspace_bytes(d))


def frechet_compute(state1: torch.Tensor, state2: torch.Tensor, out: torch.Tensor, info: torch.Tensor, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (fp32, one element) = the Frechet distance of two states of d features, d a multiple of 64 up to 2048; info (fp64 `[FID_INFO]`):
    sweeps and last residual of the first solve, of the second, solves still rotating at the sweep cap (then `out` is NaN), the score in
    fp64, sum sqrt(lambda), |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2"""
    for t in (state1, state2):
        assert t.dtype == torch.float64 and t.is_contiguous()
    d = int(round((-1 + (1 + 4 * (state1.numel() - 1)) ** 0.5) / 2))
    assert state1.numel() == state2.numel() == frechet_state_size(d)
    assert out.dtype == torch.float32 and out.numel() == 1 and info.dtype == torch.float64 and info.is_contiguous() and info.numel() == FID_INFO
    if ws is None:
        ws = workspace(frechet_workspace_bytes(d), state1.device, "frechet")
    L.check(L.load().mvldm_frechet_compute(state1.data_ptr(), state2.data_ptr(), d, ws.data_ptr(), ws.numel() * ws.element_size(), out.data_ptr(),
                                           info.data_ptr(), stream()))
    return out


# ------------------------------------------------------------------------------------------ Clean-KID (csrc/kid.hip)
KID_INFO = 4                                   # doubles of `kid_compute`'s record


def kid_workspace_bytes(m: int, num_subsets: int) -> int:
    """bytes `kid_compute` needs for `num_subsets` subsets of `m` rows a side: one double per Gram tile, two per subset; 0 for a refused
    size"""
    return int(L.load().mvldm_kid_workspace_bytes(m, num_subsets))


def kid_compute(f1: torch.Tensor, f2: torch.Tensor, idx1: torch.Tensor, idx2: torch.Tensor, out: torch.Tensor, info: torch.Tensor,
                per_subset: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (fp32, one element) = cleanfid's kernel_distance of the fp64 features f1 `[n1, d]`, f2 `[n2, d]` over the subsets idx1 (rows of
    f1), idx2 (rows of f2), int32 `[S, m]` on the same device; per_subset (fp64 `[S]`, optional): each subset's value; info (fp64
    `[KID_INFO]`): the score in fp64, the mean of the subsets' scales / m, m, the subsets with an index out of range (then `out` is NaN)"""
    for t in (f1, f2):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 2
    (n1, d), n2 = f1.shape, f2.shape[0]
    assert f2.shape[1] == d and f2.device == f1.device
    for t in (idx1, idx2):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 2 and t.device == f1.device
    s, m = idx1.shape
    assert tuple(idx2.shape) == (s, m)
    assert out.dtype == torch.float32 and out.numel() == 1 and info.dtype == torch.float64 and info.is_contiguous() and info.numel() == KID_INFO
    assert per_subset is None or (per_subset.dtype == torch.float64 and per_subset.is_contiguous() and per_subset.numel() == s)
    if ws is None:
        ws = workspace(kid_workspace_bytes(m, s), f1.device, "kid")
    L.check(L.load().mvldm_kid_compute(f1.data_ptr(), n1, f2.data_ptr(), n2, d, idx1.data_ptr(), idx2.data_ptr(), s, m, ws.data_ptr(),
                                       ws.numel() * ws.element_size(), out.data_ptr(), ptr(per_subset), info.data_ptr(), stream()))
    return out


# ------------------------------------------------------------------------------------------ crop shim (csrc/cropshim.hip)
def crop_geometry(h: int, w: int, shape) -> tuple:
    """(h_scaled, w_scaled, row, col) of `rescale_and_crop` (src/dataset/shims/crop_shim.py:51-75) and its `center_crop`: the one scale
    that makes both edges reach `shape`, Python's round, the floored centre offsets"""
    h_out, w_out = (int(v) for v in shape)
    assert h_out <= h and w_out <= w, f"crop shim only shrinks: {h} x {w} -> {h_out} x {w_out}"
    scale_factor = max(h_out / h, w_out / w)
    h_scaled, w_scaled = round(h * scale_factor), round(w * scale_factor)
    assert h_scaled == h_out or w_scaled == w_out
    return h_scaled, w_scaled, (h_scaled - h_out) // 2, (w_scaled - w_out) // 2


def _crop_src(images: torch.Tensor):
    assert images.is_cuda and images.is_contiguous() and images.dim() == 4, "crop_shim: a contiguous 4-d device tensor"
    if images.dtype == torch.uint8:
        assert images.shape[3] == 3, "crop_shim: uint8 images are [n, h, w, 3]"
        return images.shape[0], images.shape[1], images.shape[2]
    assert images.dtype == torch.float32 and images.shape[1] == 3, "crop_shim: float images are fp32 [n, 3, h, w]"
    return images.shape[0], images.shape[2], images.shape[3]


def crop_shim_workspace_bytes(n_img: int, h: int, w: int, shape) -> int:
    """bytes `crop_shim` needs for n_img images of h x w cropped to `shape`: the uint8 image between the two passes; 0 for a refused shape"""
    return int(L.load().mvldm_crop_shim_workspace_bytes(n_img, h, w, int(shape[0]), int(shape[1])))


def crop_shim(images: torch.Tensor, shape, ws: Optional[torch.Tensor] = None, flip: Optional[torch.Tensor] = None):
    """uint8 `[n, h, w, 3]` (decoded images) or fp32 `[n, 3, h, w]` in [0, 1] -> (fp32 `[n, 3, h_out, w_out]`, (h_scaled, w_scaled)): the
    reference's crop shim for the images -- quantise (float input: x 255, clamp, truncate), PIL's 8-bit LANCZOS resize to h_scaled x
    w_scaled bit for bit, centre crop, / 255 -- of which only the cropped window is computed.  The first call with a new geometry uploads
    its tables; later ones are two launches and can be captured.  `flip`: a device uint8 / bool tensor `[n]`; image i with flip[i] set is
    mirrored along w BEFORE the resize (the augmentation shim's `image.flip(-1)`), at the source read of the same two launches."""
    n, h, w = _crop_src(images)
    if flip is not None:
        assert flip.is_cuda and flip.device == images.device and flip.is_contiguous() and flip.dtype in (torch.uint8, torch.bool) \
            and tuple(flip.shape) == (n,), "crop_shim: flip is a contiguous device uint8 / bool tensor [n]"
    h_out, w_out = (int(v) for v in shape)
    h_scaled, w_scaled, _, _ = crop_geometry(h, w, (h_out, w_out))
    dst = torch.empty(n, 3, h_out, w_out, dtype=torch.float32, device=images.device)
    if ws is None:
        ws = workspace(crop_shim_workspace_bytes(n, h, w, (h_out, w_out)), images.device, "cropshim")
    got = (C.c_int * 2)()
    L.check(L.load().mvldm_crop_shim_flip(images.data_ptr(), int(images.dtype == torch.uint8), dst.data_ptr(), n, h, w, h_out, w_out,
                                          None if flip is None or n == 0 else flip.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), got, stream()))
    assert (got[0], got[1]) == (h_scaled, w_scaled), (tuple(got), h_scaled, w_scaled)
    return dst, (h_scaled, w_scaled)


# ------------------------------------------------------------------------------------------ JPEG frames (csrc/jpeg_host.cpp, csrc/jpeg.hip)
class JpegInfo(NamedTuple):
    """`mvldm_jpeg_probe` of an encoded frame.  `reason` 0: the library decodes it (`sampling`: `_lib.JPEG_GRAY` / `_444` / `_422` / `_420`);
    otherwise an index into `_lib.JPEG_REASONS`, `sampling` is -1, and h, w are the frame header's if one was read (else 0)."""
    h: int
    w: int
    sampling: int
    reason: int
    luma_blocks: int
    chroma_blocks: int
    mcu_cols: int
    mcu_rows: int

    @property
    def supported(self) -> bool:
        return self.reason == 0


def jpeg_probe(blob: bytes) -> JpegInfo:
    """size, sampling layout and block counts of an encoded frame from its markers, without decoding it (host only)"""
    info = (C.c_int32 * 8)()
    rc = L.load().mvldm_jpeg_probe(blob, len(blob), info)
    if rc < 0:
        L.check(rc)
    return JpegInfo(*info)


def jpeg_coef_count(h: int, w: int, sampling: int) -> int:
    """int16 coefficients of one h x w frame in a sampling layout (64 per block of every component's MCU-padded grid); 0 for a refused shape"""
    return int(L.load().mvldm_jpeg_coef_count(h, w, sampling))


def jpeg_workspace_bytes(n_img: int, h: int, w: int, sampling: int) -> int:
    """bytes `jpeg_decode_coefs` needs for n_img frames: the components' uint8 planes between the two kernels"""
    return int(L.load().mvldm_jpeg_workspace_bytes(n_img, h, w, sampling))


def jpeg_entropy(blob: bytes, coef: np.ndarray, qt: np.ndarray):
    """the host's entropy decoder: the frame's quantised coefficients into `coef` (a contiguous int16 array with room for
    `jpeg_coef_count` values) and its tables into `qt` (uint16 or int16, 192 values) -> (reason, largest S of a block).  Releases the GIL;
    keeps no state."""
    assert coef.dtype == np.int16 and coef.flags.c_contiguous and qt.dtype.itemsize == 2 and qt.flags.c_contiguous and qt.size >= 192
    max_s = C.c_int32(0)
    rc = L.load().mvldm_jpeg_entropy(blob, len(blob), coef.ctypes.data, coef.size, qt.ctypes.data, C.byref(max_s))
    if rc < 0:
        L.check(rc)
    return rc, max_s.value


def jpeg_idct_host(coef: np.ndarray, qt: np.ndarray, h: int, w: int, sampling: int) -> np.ndarray:
    """the device half of the decoder in plain C++ on the host (same arithmetic) -> uint8 `[h, w, 3]`: tests and tools"""
    assert coef.dtype == np.int16 and coef.flags.c_contiguous and coef.size >= jpeg_coef_count(h, w, sampling) > 0
    assert qt.dtype.itemsize == 2 and qt.flags.c_contiguous and qt.size >= 192
    out = np.empty((h, w, 3), dtype=np.uint8)
    L.check(L.load().mvldm_jpeg_idct_host(coef.ctypes.data, qt.ctypes.data, out.ctypes.data, h, w, sampling))
    return out


def jpeg_decode_coefs(coef: torch.Tensor, qt: torch.Tensor, h: int, w: int, sampling: int, dst: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`mvldm_jpeg_decode`: coefficients int16 `[n, jpeg_coef_count]` and tables int16 `[n, 192]` (uint16 bit patterns) on the device ->
    uint8 `[n, h, w, 3]`.  Two launches; nothing is allocated when `dst` and `ws` are given, so the call can be captured."""
    n = coef.shape[0]
    assert coef.is_cuda and coef.is_contiguous() and coef.dtype == torch.int16 and tuple(coef.shape) == (n, jpeg_coef_count(h, w, sampling))
    assert qt.is_cuda and qt.is_contiguous() and qt.dtype == torch.int16 and tuple(qt.shape) == (n, 192)
    if dst is None:
        dst = torch.empty(n, h, w, 3, dtype=torch.uint8, device=coef.device)
    assert dst.is_cuda and dst.is_contiguous() and dst.dtype == torch.uint8 and tuple(dst.shape) == (n, h, w, 3)
    if ws is None:
        ws = workspace(jpeg_workspace_bytes(n, h, w, sampling), coef.device, "jpeg")
    L.check(L.load().mvldm_jpeg_decode(coef.data_ptr(), qt.data_ptr(), dst.data_ptr(), n, h, w, sampling, ws.data_ptr(), ws.numel() * ws.element_size(),
                                       stream()))
    return dst


class JpegScan(NamedTuple):
    """`jpeg_scan_prepare` of one frame: `reason` 0 and the frame's part of `scan`, its `desc` and `tables` are what `jpeg_entropy_device`
    takes; `_lib.JPEG_RESTART`: the frame has restart intervals and its scan is `jpeg_entropy`'s; any other reason as `jpeg_probe`."""
    reason: int
    info: JpegInfo
    scan: np.ndarray
    desc: np.ndarray
    tables: np.ndarray


def jpeg_scan_room(n: int) -> int:
    """bytes of the packed scan buffer a frame of n encoded bytes (or a destuffed scan of n bytes) can take: padding included, a multiple of 16"""
    return int(L.load().mvldm_jpeg_scan_room(n))


def jpeg_entropy_chunk_subseqs() -> int:
    """subsequences (one per thread) of a chunk of the device entropy decoder"""
    return int(L.load().mvldm_jpeg_entropy_chunk_subseqs())


def _jpeg_prepare(c_name, room, blob, scan, scan_off, desc, tables) -> JpegScan:
    """the two prepares: `room()` bytes behind the offset when `scan` is left out, then the C function `c_name`"""
    if scan is None:
        scan = np.zeros(scan_off + room(), dtype=np.uint8)
    if desc is None:
        desc = np.zeros(4, dtype=np.int32)
    if tables is None:
        tables = np.zeros(L.JPEG_TABLE_BYTES, dtype=np.uint8)
    assert scan.dtype == np.uint8 and scan.flags.c_contiguous and scan.ndim == 1
    assert desc.dtype == np.int32 and desc.flags.c_contiguous and desc.size == 4
    assert tables.dtype == np.uint8 and tables.flags.c_contiguous and tables.size == L.JPEG_TABLE_BYTES
    info = (C.c_int32 * 8)()
    rc = getattr(L.load(), c_name)(blob, len(blob), scan.ctypes.data, scan_off, scan.size, desc.ctypes.data, tables.ctypes.data, info)
    if rc < 0:
        L.check(rc)
    return JpegScan(rc, JpegInfo(*info), scan, desc, tables)


def jpeg_scan_prepare(blob: bytes, scan: Optional[np.ndarray] = None, scan_off: int = 0, desc: Optional[np.ndarray] = None,
                      tables: Optional[np.ndarray] = None) -> JpegScan:
    """what the host still does for the device entropy decoder (`mvldm_jpeg_scan_prepare`): the markers, the destuffed scan into
    `scan[scan_off:]` (uint8, room for `jpeg_scan_room(len(blob))` bytes behind the offset, a multiple of 16), the descriptor into `desc`
    (int32 `[4]`) and the Huffman and quantisation tables into `tables` (uint8 `[_lib.JPEG_TABLE_BYTES]`).  Buffers left out are made.
    Releases the GIL; keeps no state."""
    return _jpeg_prepare("mvldm_jpeg_scan_prepare", lambda: jpeg_scan_room(len(blob)), blob, scan, scan_off, desc, tables)


def _jpeg_entropy_emul(c_name, scan, desc, tables, h, w, sampling, coef, qt, status, subseq_bits, chunk_subseqs):
    """the two emulations: the C function `c_name` over the frames of `desc`; outputs left out are made"""
    desc, tables = desc.reshape(-1, 4), tables.reshape(-1, L.JPEG_TABLE_BYTES)
    n, count = desc.shape[0], jpeg_coef_count(h, w, sampling)
    assert scan.dtype == np.uint8 and scan.flags.c_contiguous and desc.dtype == np.int32 and desc.flags.c_contiguous
    assert tables.dtype == np.uint8 and tables.flags.c_contiguous and tables.shape[0] == n and count > 0
    coef = np.empty((n, count), dtype=np.int16) if coef is None else coef
    qt = np.empty((n, 192), dtype=np.uint16) if qt is None else qt
    status = np.empty((n, 4), dtype=np.int32) if status is None else status
    assert coef.dtype == np.int16 and coef.flags.c_contiguous and coef.size == n * count and qt.dtype.itemsize == 2 and qt.flags.c_contiguous and qt.size == n * 192
    assert status.dtype == np.int32 and status.flags.c_contiguous and status.size == n * 4
    L.check(getattr(L.load(), c_name)(scan.ctypes.data, scan.size, desc.ctypes.data, tables.ctypes.data, n, h, w, sampling, coef.ctypes.data, qt.ctypes.data,
                                      status.ctypes.data, subseq_bits, chunk_subseqs))
    return coef, qt, status


def jpeg_entropy_emul(scan: np.ndarray, desc: np.ndarray, tables: np.ndarray, h: int, w: int, sampling: int, coef: Optional[np.ndarray] = None,
                      qt: Optional[np.ndarray] = None, status: Optional[np.ndarray] = None, subseq_bits: int = 0, chunk_subseqs: int = 0):
    """the device entropy decoder on the host (`mvldm_jpeg_entropy_emul_host`: the same step function, loops for threads) over the
    frames of `desc` int32 `[n, 4]` -> (coef int16 `[n, jpeg_coef_count]`, qt uint16 `[n, 192]`, status int32 `[n, 4]`): tests and tools"""
    return _jpeg_entropy_emul("mvldm_jpeg_entropy_emul_host", scan, desc, tables, h, w, sampling, coef, qt, status, subseq_bits, chunk_subseqs)


def _jpeg_entropy_device(c_name, scan, desc, tables, h, w, sampling, coef, qt, status, subseq_bits):
    """the two device entropy calls: the C function `c_name` over the frames of `desc`; outputs left out are made"""
    n, count = desc.shape[0], jpeg_coef_count(h, w, sampling)
    assert scan.is_cuda and scan.is_contiguous() and scan.dtype == torch.uint8 and scan.dim() == 1
    assert desc.is_cuda and desc.is_contiguous() and desc.dtype == torch.int32 and tuple(desc.shape) == (n, 4)
    assert tables.is_cuda and tables.is_contiguous() and tables.dtype == torch.uint8 and tuple(tables.shape) == (n, L.JPEG_TABLE_BYTES) and count > 0
    coef = torch.empty(n, count, dtype=torch.int16, device=scan.device) if coef is None else coef
    qt = torch.empty(n, 192, dtype=torch.int16, device=scan.device) if qt is None else qt
    status = torch.empty(n, 4, dtype=torch.int32, device=scan.device) if status is None else status
    assert coef.is_cuda and coef.is_contiguous() and coef.dtype == torch.int16 and tuple(coef.shape) == (n, count)
    assert qt.is_cuda and qt.is_contiguous() and qt.dtype == torch.int16 and tuple(qt.shape) == (n, 192)
    assert status.is_cuda and status.is_contiguous() and status.dtype == torch.int32 and tuple(status.shape) == (n, 4)
    L.check(getattr(L.load(), c_name)(scan.data_ptr(), scan.numel(), desc.data_ptr(), tables.data_ptr(), n, h, w, sampling, coef.data_ptr(), qt.data_ptr(),
                                      status.data_ptr(), subseq_bits, stream()))
    return coef, qt, status


def jpeg_entropy_device(scan: torch.Tensor, desc: torch.Tensor, tables: torch.Tensor, h: int, w: int, sampling: int, coef: Optional[torch.Tensor] = None,
                        qt: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, subseq_bits: int = 0):
    """`mvldm_jpeg_entropy_device`: the prepared frames of `desc` int32 `[n, 4]` (packed scans uint8, tables uint8 `[n, JPEG_TABLE_BYTES]`, all
    on the device) -> (coef int16 `[n, jpeg_coef_count]`, qt int16 `[n, 192]`, status int32 `[n, 4]` = reason, largest S, rounds, 0): what
    `jpeg_decode_coefs` takes.  A memset and two launches; nothing is allocated when the three outputs are given, and nothing is read
    back, so the call can be captured."""
    return _jpeg_entropy_device("mvldm_jpeg_entropy_device", scan, desc, tables, h, w, sampling, coef, qt, status, subseq_bits)


def jpeg_status_download(status: torch.Tensor) -> np.ndarray:
    """the status words of a `jpeg_entropy_device` call on the host: the one read-back (and synchronisation) of `jpeg_decode(entropy="device")`"""
    return status.cpu().numpy()


def jpeg_rst_room(n: int) -> int:
    """bytes of the packed buffer ANY frame of n encoded bytes can take on the restart path (`mvldm_jpeg_rst_room`): a multiple of 16"""
    return int(L.load().mvldm_jpeg_rst_room(n))


def jpeg_rst_need(blob: bytes) -> int:
    """bytes of the packed buffer THIS frame can take (`mvldm_jpeg_rst_need`, from its header: interval table, scan, alignment, padding);
    0 for a frame the parser refuses.  At most `jpeg_rst_room(len(blob))`; what `jpeg_rst_prepare` asks for behind its offset."""
    return int(L.load().mvldm_jpeg_rst_need(blob, len(blob)))


def jpeg_rst_prepare(blob: bytes, scan: Optional[np.ndarray] = None, scan_off: int = 0, desc: Optional[np.ndarray] = None,
                     tables: Optional[np.ndarray] = None) -> JpegScan:
    """`jpeg_scan_prepare` for frames with and without restart intervals (`mvldm_jpeg_rst_prepare`): the frame's region -- interval table
    and destuffed intervals -- into `scan[scan_off:]` (room for `jpeg_rst_need(blob)` bytes behind the offset, a multiple of 16), the
    descriptor (offset, intervals, bytes, MCUs per interval) into `desc` and the tables into `tables`: what `jpeg_rst_entropy_device`
    takes.  Never answers `_lib.JPEG_RESTART`.  Buffers left out are made.  Releases the GIL; keeps no state."""
    return _jpeg_prepare("mvldm_jpeg_rst_prepare", lambda: jpeg_rst_need(blob), blob, scan, scan_off, desc, tables)


def jpeg_rst_entropy_emul(scan: np.ndarray, desc: np.ndarray, tables: np.ndarray, h: int, w: int, sampling: int, coef: Optional[np.ndarray] = None,
                          qt: Optional[np.ndarray] = None, status: Optional[np.ndarray] = None, subseq_bits: int = 0, chunk_subseqs: int = 0):
    """`jpeg_entropy_emul` of the restart path (`mvldm_jpeg_rst_entropy_emul_host`) over the frames `jpeg_rst_prepare` laid down ->
    (coef, qt, status int32 `[n, 4]` = reason, largest S, rounds, intervals): tests and tools"""
    return _jpeg_entropy_emul("mvldm_jpeg_rst_entropy_emul_host", scan, desc, tables, h, w, sampling, coef, qt, status, subseq_bits, chunk_subseqs)


def jpeg_rst_entropy_device(scan: torch.Tensor, desc: torch.Tensor, tables: torch.Tensor, h: int, w: int, sampling: int, coef: Optional[torch.Tensor] = None,
                            qt: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, subseq_bits: int = 0):
    """`mvldm_jpeg_rst_entropy_device`: `jpeg_entropy_device` for the frames `jpeg_rst_prepare` laid down, with and without restart
    intervals -> (coef, qt, status int32 `[n, 4]` = reason, largest S, rounds, intervals).  A memset and two launches; nothing is
    allocated when the three outputs are given, and nothing is read back, so the call can be captured."""
    return _jpeg_entropy_device("mvldm_jpeg_rst_entropy_device", scan, desc, tables, h, w, sampling, coef, qt, status, subseq_bits)


def _map(pool, f, xs) -> list:
    """`[f(x) for x in xs]`, on `pool` when one is given and there is more than one job (results in the order of `xs`)"""
    return list(pool.map(f, xs)) if pool is not None and len(xs) > 1 else [f(x) for x in xs]


# What `jpeg_decode` stages for the `members` (frame numbers) of one sampling layout, `info` the probe of one of them -> (the pinned buffer
# that goes up in one copy, one host job `(function, *arguments)` per member that fills its part and returns its reason first, a function
# from the uploaded buffer to (coef, qt, status or None): what `jpeg_decode_coefs` takes)
def _jpeg_stage_host(blobs, members, info):
    """[coefficients | tables], filled by `jpeg_entropy`"""
    m, count = len(members), jpeg_coef_count(info.h, info.w, info.sampling)
    buf = torch.empty(m * (count + 192), dtype=torch.int16, pin_memory=True)
    host = buf.numpy()
    jobs = [(jpeg_entropy, blobs[i], host[j * count:(j + 1) * count], host[m * count + j * 192:m * count + (j + 1) * 192]) for j, i in enumerate(members)]
    return buf, jobs, lambda on_dev: (on_dev[:m * count].view(m, count), on_dev[m * count:].view(m, 192), None)


def _jpeg_stage_scans(room, prepare, entropy, blobs, members, info):
    """[scans or regions | tables | descriptors]: `room(blob)` bytes a frame (a multiple of 16), filled by `prepare`; the coefficients are
    `entropy`'s"""
    m, tb = len(members), L.JPEG_TABLE_BYTES
    offs = [0]
    for i in members:
        offs.append(offs[-1] + room(blobs[i]))
    end = offs[-1]
    buf = torch.empty(end + m * (tb + 16), dtype=torch.uint8, pin_memory=True)
    host = buf.numpy()
    tables, desc = host[end:end + m * tb].reshape(m, tb), host[end + m * tb:].view(np.int32).reshape(m, 4)
    jobs = [(prepare, blobs[i], host[:offs[j + 1]], offs[j], desc[j], tables[j]) for j, i in enumerate(members)]
    return buf, jobs, lambda on_dev: entropy(on_dev[:end], on_dev[end + m * tb:].view(torch.int32).view(m, 4), on_dev[end:end + m * tb].view(m, tb),
                                             info.h, info.w, info.sampling)


def jpeg_decode(blobs: Sequence[bytes], pool=None, device=None, entropy: str = "host", restarts: str = "host") -> torch.Tensor:
    """encoded frames of ONE size -> uint8 `[n, h, w, 3]` on the current device, the bytes `Image.open(...).convert("RGB")` gives.

    Per frame the host parses the markers and decodes the Huffman scan (`mvldm_jpeg_entropy`: no Pillow, no GIL; on `pool`, a
    `concurrent.futures` executor, when one is given) straight into one pinned staging tensor per sampling layout; each layout is one
    upload and one `mvldm_jpeg_decode` call.  A frame the library refuses -- progressive, CMYK, outside the range guard, PNG, ... -- is
    decoded by `dataset.decode_image` (Pillow) on the host and uploaded into its slot: the result never depends on which path ran.

    `entropy="device"`: the host only parses the markers and removes the byte stuffing (`mvldm_jpeg_scan_prepare`, on `pool`) into one
    pinned tensor per layout -- scans, tables, descriptors: about a twelfth of the coefficients -- and each layout is one upload, one
    `mvldm_jpeg_entropy_device`, one `mvldm_jpeg_decode` and then ONE small download of the frames' status words: a synchronisation
    with the device that the host path does not have.  A frame with restart intervals takes the host's entropy pass into the same device
    call; a frame whose status is not 0, or that prepare refused, goes through `decode_image` as above.  The same bytes either way.

    `restarts="device"` (needs `entropy="device"`): every frame of a layout, with or without restart intervals, goes through
    `mvldm_jpeg_rst_prepare` and ONE `mvldm_jpeg_rst_entropy_device` per layout -- the intervals are independent streams with known start
    states -- and `mvldm_jpeg_entropy` is never called.  The same bytes again."""
    from .dataset import decode_image
    n = len(blobs)
    if n == 0:
        raise ValueError("jpeg_decode: no frames")
    if entropy not in ("host", "device"):
        raise ValueError(f"jpeg_decode: entropy {entropy!r} (host or device)")
    if restarts not in ("host", "device") or (restarts == "device" and entropy != "device"):
        raise ValueError(f"jpeg_decode: restarts {restarts!r} with entropy {entropy!r} (host or device; device needs entropy=\"device\")")
    if entropy == "host":
        stage = _jpeg_stage_host
    elif restarts == "device":      # the room from the frame's header, not the bound for any frame
        stage = functools.partial(_jpeg_stage_scans, jpeg_rst_need, jpeg_rst_prepare, jpeg_rst_entropy_device)
    else:
        stage = functools.partial(_jpeg_stage_scans, lambda blob: jpeg_scan_room(len(blob)), jpeg_scan_prepare, jpeg_entropy_device)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    infos = [jpeg_probe(b) for b in blobs]
    groups: dict = {}
    for i, info in enumerate(infos):
        if info.supported:
            groups.setdefault(info.sampling, []).append(i)
    sizes = {(info.h, info.w) for info in infos if info.supported}

    def one_size():
        if len(sizes) > 1:
            raise ValueError(f"jpeg_decode: frames of one size, got {sorted(sizes)}")
    one_size()
    refused = [i for i, info in enumerate(infos) if not info.supported]
    run = lambda job: job[0](*job[1:])[0]       # the reason: first in `jpeg_entropy`'s pair and in `JpegScan`
    staged = [(members, *stage(blobs, members, infos[members[0]])) for members in groups.values()]
    order = [i for members, *_ in staged for i in members]
    reasons = dict(zip(order, _map(pool, run, [job for _, _, jobs, _ in staged for job in jobs])))
    refused += [i for i in order if reasons[i] not in (0, L.JPEG_RESTART)]      # the scan itself: corrupt, or outside the guard
    dst, pending = None, []
    with torch.cuda.device(dev):
        for members, buf, _, coefs in staged:
            info, m = infos[members[0]], len(members)
            coef, qt, status = coefs(buf.to(dev, non_blocking=True))
            at = [j for j, i in enumerate(members) if reasons[i] == L.JPEG_RESTART]
            if at:      # restart intervals (prepare's answer: device entropy only): the host's entropy pass, into the same device call
                rbuf, rjobs, rcoefs = _jpeg_stage_host(blobs, [members[j] for j in at], info)
                refused += [members[j] for j, reason in zip(at, _map(pool, run, rjobs)) if reason != 0]
                at = torch.tensor(at, device=dev)
                coef[at], qt[at], _ = rcoefs(rbuf.to(dev, non_blocking=True))     # after the kernels: their slots hold a refused frame's leftovers
            if dst is None:
                dst = torch.empty(n, info.h, info.w, 3, dtype=torch.uint8, device=dev)
            whole = m == n                      # the common case: every frame in one layout, decoded in place
            out = jpeg_decode_coefs(coef, qt, info.h, info.w, info.sampling, dst if whole else None)
            if not whole:
                dst[torch.tensor(members, device=dev)] = out
            if status is not None:
                pending.append((members, status))
        for members, status in pending:         # one small read-back per layout, after every launch; the host path has none
            st = jpeg_status_download(status)
            refused += [i for j, i in enumerate(members) if reasons[i] == 0 and st[j, 0] != 0]
        late = _map(pool, decode_image, [blobs[i] for i in sorted(refused)])
        sizes |= {f.shape[:2] for f in late}
        one_size()
        (h, w), = sizes
        if dst is None:
            dst = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
        if late:
            host = torch.empty(len(late), h, w, 3, dtype=torch.uint8, pin_memory=True)
            for j, f in enumerate(late):
                host.numpy()[j] = f
            dst[torch.tensor(sorted(refused), device=dev)] = host.to(dev, non_blocking=True)         # after the kernels: a refused scan's slot is overwritten
    return dst


# ------------------------------------------------------------------------------------------ PNG frames (csrc/png.hip, csrc/png_host.cpp)
_PNG_SIG = b"\x89PNG\r\n\x1a\n"
_PNG_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}        # the PNG specification's colour type -> bit depths
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_PNG_NO_FRAME = (0, -1, 0, 0, 0, 0, 0, 0)       # the descriptor of a frame the host refused: no format, so the kernel reads and writes nothing for it


class PngInfo(NamedTuple):
    """`png_probe` of an encoded frame.  `reason` 0: the library unfilters it on the device; otherwise an index into `_lib.PNG_REASONS`.
    h, w, color_type, depth and interlace are IHDR's where one was read (else 0)."""
    h: int
    w: int
    color_type: int
    depth: int
    interlace: int
    reason: int

    @property
    def supported(self) -> bool:
        return self.reason == 0

    @property
    def stride(self) -> int:
        """bytes of a row behind its filter byte"""
        return (self.w * _PNG_CHANNELS[self.color_type] * self.depth + 7) // 8

    @property
    def stream_bytes(self) -> int:
        """what IDAT has to inflate to"""
        return self.h * (1 + self.stride)


def png_probe(blob: bytes) -> PngInfo:
    """size, colour type, bit depth, interlace flag and reason of an encoded frame from its IHDR: nothing is inflated (host only, no library call)"""
    if len(blob) < 8 or bytes(blob[:8]) != _PNG_SIG:
        return PngInfo(0, 0, 0, 0, 0, L.PNG_NOT_PNG)
    if len(blob) < 33:
        return PngInfo(0, 0, 0, 0, 0, L.PNG_TRUNCATED)
    if bytes(blob[8:16]) != b"\x00\x00\x00\rIHDR":
        return PngInfo(0, 0, 0, 0, 0, L.PNG_NOT_PNG)
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", blob[16:29])
    why = lambda reason: PngInfo(h, w, ctype, depth, lace, reason)
    if struct.unpack(">I", blob[29:33])[0] != (zlib.crc32(blob[12:29]) & 0xFFFFFFFF):
        return why(L.PNG_CRC)
    if depth not in _PNG_DEPTHS.get(ctype, ()) or comp != 0 or filt != 0 or lace > 1:
        return why(L.PNG_FORMAT)
    if not (1 <= h <= L.PNG_MAX_DIM and 1 <= w <= L.PNG_MAX_DIM):
        return why(L.PNG_SIZE)
    if lace:
        return why(L.PNG_INTERLACE)
    if depth == 16:
        return why(L.PNG_DEPTH16)
    if ctype == 0 and depth < 8:
        return why(L.PNG_GREY_BITS)
    return why(0)


def _png_chunks(blob: bytes):
    """(reason, IDAT bodies, PLTE body or None) of a frame whose IHDR `png_probe` accepted: every chunk's CRC is checked (Pillow raises on
    a bad one, so such a frame is Pillow's to judge), the walk ends at IEND"""
    pos, idat, plte, n = 33, [], None, len(blob)
    view = memoryview(blob)
    while True:
        if pos + 12 > n:
            return L.PNG_TRUNCATED, idat, plte
        size, tag = struct.unpack(">I", view[pos:pos + 4])[0], bytes(view[pos + 4:pos + 8])
        if pos + 12 + size > n:
            return L.PNG_TRUNCATED, idat, plte
        body = view[pos + 8:pos + 8 + size]
        if struct.unpack(">I", view[pos + 8 + size:pos + 12 + size])[0] != (zlib.crc32(body, zlib.crc32(tag)) & 0xFFFFFFFF):
            return L.PNG_CRC, idat, plte
        if tag == b"IDAT":
            idat.append(body)
        elif tag == b"PLTE":
            if plte is not None or idat:
                return L.PNG_FORMAT, idat, plte
            plte = body
        elif tag == b"IEND":
            return (0 if idat else L.PNG_TRUNCATED), idat, plte
        elif tag == b"IHDR" or not (tag[0] & 0x20):     # a second header, or a critical chunk this reader does not know
            return L.PNG_FORMAT, idat, plte
        pos += 12 + size


def _png_stage(blob: bytes, info: PngInfo, host: np.ndarray, off: int, pal0: int, pal_off: int, desc: np.ndarray) -> int:
    """what the host does for one frame `png_probe` accepted: the chunks and their CRCs, IDAT inflated (`zlib`, which releases the GIL) into
    `host[off : off + info.stream_bytes]`, the palette to byte `pal_off` of the palettes, which start at `host[pal0]`, the descriptor into `desc` (int32 `[8]`).
    Returns the reason; after a refusal the descriptor is the no-frame one, and nothing reaches the kernel."""
    desc[:] = _PNG_NO_FRAME
    reason, idat, plte = _png_chunks(blob)
    if reason:
        return reason
    count = 0
    if info.color_type == 3:
        if plte is None or len(plte) == 0 or len(plte) % 3 or len(plte) > 768:
            return L.PNG_NO_PLTE
        count = len(plte) // 3
    need = info.stream_bytes
    inflater = zlib.decompressobj()
    try:
        raw = inflater.decompress(idat[0] if len(idat) == 1 else b"".join(idat), need + 1)
    except zlib.error:
        return L.PNG_INFLATE
    if len(raw) != need:
        return L.PNG_LENGTH                             # short, or bytes behind the last row
    if not inflater.eof or inflater.unused_data:
        return L.PNG_INFLATE                            # a stream without its end or with bytes behind it: Pillow's to judge
    rows = np.frombuffer(raw, dtype=np.uint8)
    if int(rows[::1 + info.stride].max()) > 4:
        return L.PNG_FILTER
    host[off:off + need] = rows
    if count:
        host[pal0 + pal_off:pal0 + pal_off + 3 * count] = np.frombuffer(plte, dtype=np.uint8)
    desc[:] = (off, info.color_type, info.depth, pal_off, count, 0, 0, 0)
    return 0


def _png_layout(infos) -> tuple:
    """(stream offsets of the supported frames {i: offset}, end of the streams = start of the palettes, start of the descriptors, bytes):
    one staging buffer [streams | 768 bytes of palette per frame | int32 [n, 8] descriptors]"""
    offs, end = {}, 0
    for i, info in enumerate(infos):
        if info.supported:
            offs[i] = end
            end += info.stream_bytes
    desc0 = (end + 768 * len(infos) + 3) & ~3
    return offs, end, desc0, desc0 + 4 * L.PNG_DESC_INTS * len(infos)


def png_unfilter_host(streams: np.ndarray, desc: np.ndarray, palettes: np.ndarray, h: int, w: int, dst: np.ndarray) -> np.ndarray:
    """`mvldm_png_unfilter_host`: the kernel's arithmetic in plain C++ over the frames of `desc` int32 `[n, 8]` into `dst` -- uint8
    `[n, h, w, 3]` or float32 `[n, 3, h, w]` -> status int32 `[n]`: tests and tools"""
    desc = desc.reshape(-1, L.PNG_DESC_INTS)
    n = desc.shape[0]
    assert streams.dtype == np.uint8 and streams.flags.c_contiguous and palettes.dtype == np.uint8 and palettes.flags.c_contiguous
    assert desc.dtype == np.int32 and desc.flags.c_contiguous and dst.flags.c_contiguous
    assert (dst.dtype == np.uint8 and dst.shape == (n, h, w, 3)) or (dst.dtype == np.float32 and dst.shape == (n, 3, h, w)), (dst.dtype, dst.shape)
    status = np.full(n, -1, dtype=np.int32)
    L.check(L.load().mvldm_png_unfilter_host(streams.ctypes.data, streams.size, desc.ctypes.data, palettes.ctypes.data if palettes.size else None, palettes.size,
                                             dst.ctypes.data, L.PNG_DST_U8 if dst.dtype == np.uint8 else L.PNG_DST_F32, n, h, w, status.ctypes.data))
    return status


def png_decode_host(blob: bytes, dst: Optional[np.ndarray] = None, out: str = "uint8"):
    """one encoded frame through the host twin -> (reason, pixels): uint8 `[h, w, 3]` or float32 `[3, h, w]` (`dst`, when given, is that
    array and is written in place).  A refused frame comes back with its reason and `None`, and `dst` is not touched; reason
    `_lib.PNG_PALETTE_INDEX` comes with the pixels the kernel would write (black where the index has no entry).  Tests and tools."""
    info = png_probe(blob)
    if not info.supported:
        return info.reason, None
    (offs, end, desc0, total), (h, w) = _png_layout([info]), (info.h, info.w)
    host = np.zeros(total, dtype=np.uint8)
    desc = host[desc0:].view(np.int32)
    reason = _png_stage(blob, info, host, 0, end, 0, desc)
    if reason:
        return reason, None
    shape = (h, w, 3) if out == "uint8" else (3, h, w)
    if dst is None:
        dst = np.empty(shape, dtype=np.uint8 if out == "uint8" else np.float32)
    assert dst.shape == shape and dst.flags.c_contiguous, (dst.shape, shape)
    status = png_unfilter_host(host[:end], desc, host[end:desc0], h, w, dst.reshape(1, *shape))
    return int(status[0]), dst


def png_unfilter(staged: torch.Tensor, stream_bytes: int, desc0: int, n: int, h: int, w: int, dst: torch.Tensor, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`mvldm_png_unfilter` over one uploaded staging buffer of `_png_layout` -> status int32 `[n]` on the device.  One launch; nothing is
    allocated when `status` is given, and nothing is read back, so the call can be captured."""
    assert staged.is_cuda and staged.is_contiguous() and staged.dtype == torch.uint8 and staged.dim() == 1 and desc0 % 4 == 0
    assert staged.numel() >= desc0 + 4 * L.PNG_DESC_INTS * n and stream_bytes + 768 * n <= desc0
    assert dst.is_cuda and dst.is_contiguous() and dst.device == staged.device
    assert (dst.dtype == torch.uint8 and tuple(dst.shape) == (n, h, w, 3)) or (dst.dtype == torch.float32 and tuple(dst.shape) == (n, 3, h, w)), (dst.dtype, tuple(dst.shape))
    status = torch.empty(n, dtype=torch.int32, device=staged.device) if status is None else status
    assert status.is_cuda and status.is_contiguous() and status.dtype == torch.int32 and tuple(status.shape) == (n,)
    base = staged.data_ptr()
    L.check(L.load().mvldm_png_unfilter(base, stream_bytes, base + desc0, base + stream_bytes, 768 * n, dst.data_ptr(),
                                        L.PNG_DST_U8 if dst.dtype == torch.uint8 else L.PNG_DST_F32, n, h, w, status.data_ptr(), stream()))
    return status


def png_inflate_host(z: np.ndarray, zdesc: np.ndarray, streams: np.ndarray, desc: np.ndarray, h: int, w: int) -> np.ndarray:
    """`mvldm_png_inflate_host`: the zlib streams of `zdesc` int32 `[n, 4]` (offset in `z`, a multiple of 16; bytes; zeros behind each up
    to `mvldm_png_inflate_room`) inflated into the slots of `desc` int32 `[n, 8]` in `streams`, by the kernel's step functions in plain C++
    -> status int32 `[n]`: tests, tools and `png_decode(device="cpu", inflate="device")`"""
    zdesc, desc = zdesc.reshape(-1, L.PNG_ZDESC_INTS), desc.reshape(-1, L.PNG_DESC_INTS)
    n = desc.shape[0]
    assert zdesc.shape[0] == n and zdesc.dtype == np.int32 and zdesc.flags.c_contiguous and desc.dtype == np.int32 and desc.flags.c_contiguous
    assert z.dtype == np.uint8 and z.flags.c_contiguous and streams.dtype == np.uint8 and streams.flags.c_contiguous and streams.flags.writeable
    status = np.full(n, -1, dtype=np.int32)
    L.check(L.load().mvldm_png_inflate_host(z.ctypes.data, z.size, zdesc.ctypes.data, streams.ctypes.data, streams.size, desc.ctypes.data, n, h, w, status.ctypes.data))
    return status


def png_inflate(z: torch.Tensor, zdesc: torch.Tensor, streams: torch.Tensor, desc: torch.Tensor, h: int, w: int, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`mvldm_png_inflate`: as `png_inflate_host` on device tensors (`z`, `streams` uint8, 1-D; `zdesc` int32 `[n, 4]`, `desc` int32
    `[n, 8]`) -> status int32 `[n]` on the device.  One launch; nothing is allocated when `status` is given, and nothing is read back, so
    the call can be captured."""
    n = desc.shape[0]
    assert z.is_cuda and z.is_contiguous() and z.dtype == torch.uint8 and z.dim() == 1 and z.data_ptr() % 16 == 0
    assert streams.is_cuda and streams.is_contiguous() and streams.dtype == torch.uint8 and streams.dim() == 1 and streams.device == z.device
    assert zdesc.is_cuda and zdesc.is_contiguous() and zdesc.dtype == torch.int32 and tuple(zdesc.shape) == (n, L.PNG_ZDESC_INTS)
    assert desc.is_cuda and desc.is_contiguous() and desc.dtype == torch.int32 and tuple(desc.shape) == (n, L.PNG_DESC_INTS)
    status = torch.empty(n, dtype=torch.int32, device=z.device) if status is None else status
    assert status.is_cuda and status.is_contiguous() and status.dtype == torch.int32 and tuple(status.shape) == (n,)
    L.check(L.load().mvldm_png_inflate(z.data_ptr(), z.numel(), zdesc.data_ptr(), streams.data_ptr(), streams.numel(), desc.data_ptr(), n, h, w, status.data_ptr(), stream()))
    return status


def _png_zstage(blobs, infos, pool, refused: dict, pin: bool):
    """the host's share of `png_decode(inflate="device")` for the frames `png_probe` accepted: the chunk walk with every CRC (on `pool`),
    then each frame's IDAT bodies copied back to back into ONE staging tensor [z streams, each at a multiple of 16 with zeros up to
    `mvldm_png_inflate_room` | 768 bytes of palette per frame | int32 [n, 8] descriptors | int32 [n, 4] z descriptors].  Adds what it
    refuses to `refused`; returns None when nothing is left, else (staging tensor, frames kept, end of the z streams = start of the
    palettes, bytes of the inflated streams, start of the descriptors, start of the z descriptors)."""
    n, lib = len(blobs), L.load()
    order = [i for i, p in enumerate(infos) if p.supported]
    keep, zend, send = [], 0, 0
    for i, (reason, idat, plte) in zip(order, _map(pool, lambda i: _png_chunks(blobs[i]), order)):
        if not reason and infos[i].color_type == 3 and (plte is None or len(plte) == 0 or len(plte) % 3 or len(plte) > 768):
            reason = L.PNG_NO_PLTE
        if reason:
            refused[i] = reason
            continue
        zbytes = sum(len(b) for b in idat)
        keep.append((i, idat, plte, zend, zbytes, send))
        zend += lib.mvldm_png_inflate_room(zbytes)
        send += infos[i].stream_bytes
    if not keep:
        return None
    desc0 = (zend + 768 * n + 3) & ~3
    zdesc0 = desc0 + 4 * L.PNG_DESC_INTS * n
    buf = torch.empty(zdesc0 + 4 * L.PNG_ZDESC_INTS * n, dtype=torch.uint8, pin_memory=pin)
    host = buf.numpy()
    desc = host[desc0:zdesc0].view(np.int32).reshape(n, L.PNG_DESC_INTS)
    zdesc = host[zdesc0:].view(np.int32).reshape(n, L.PNG_ZDESC_INTS)
    desc[:] = _PNG_NO_FRAME
    zdesc[:] = 0
    for i, idat, plte, zoff, zbytes, soff in keep:
        host[zoff:zoff + zbytes] = np.frombuffer(idat[0] if len(idat) == 1 else b"".join(idat), dtype=np.uint8)
        host[zoff + zbytes:zoff + lib.mvldm_png_inflate_room(zbytes)] = 0
        count = 0
        if infos[i].color_type == 3:
            count = len(plte) // 3
            host[zend + 768 * i:zend + 768 * i + 3 * count] = np.frombuffer(plte, dtype=np.uint8)
        desc[i] = (soff, infos[i].color_type, infos[i].depth, 768 * i, count, 0, 0, 0)
        zdesc[i] = (zoff, zbytes, 0, 0)
    return buf, [k[0] for k in keep], zend, send, desc0, zdesc0


def _png_decode_zdevice(blobs, infos, pool, dev, dst: torch.Tensor, h: int, w: int, refused: dict, info: Optional[dict]) -> None:
    """`png_decode(inflate="device")` behind `png_probe`: `_png_zstage` on the host, ONE upload, `mvldm_png_inflate` into a device tensor
    that is never uploaded, `mvldm_png_unfilter` out of it, and ONE download that carries both status vectors.  `dev` cpu: the two host
    twins.  Adds the frames either status refuses to `refused`, the inflate's reason first."""
    n, lib, on_host = len(blobs), L.load(), dev.type == "cpu"
    staged = _png_zstage(blobs, infos, pool, refused, pin=not on_host)
    if staged is None:
        return
    buf, keep, zend, send, desc0, zdesc0 = staged
    if on_host:
        host = buf.numpy()
        desc, zdesc = host[desc0:zdesc0].view(np.int32), host[zdesc0:].view(np.int32)
        streams = np.empty(send, dtype=np.uint8)
        status = np.stack([png_inflate_host(host[:zend], zdesc, streams, desc, h, w), png_unfilter_host(streams, desc, host[zend:zend + 768 * n], h, w, dst.numpy())])
    else:
        on_dev = buf.to(dev, non_blocking=True)
        streams = torch.empty(send, dtype=torch.uint8, device=dev)
        both = torch.empty(2, n, dtype=torch.int32, device=dev)
        base = on_dev.data_ptr()
        L.check(lib.mvldm_png_inflate(base, zend, base + zdesc0, streams.data_ptr(), send, base + desc0, n, h, w, both[0].data_ptr(), stream()))
        L.check(lib.mvldm_png_unfilter(streams.data_ptr(), send, base + desc0, base + zend, 768 * n, dst.data_ptr(),
                                       L.PNG_DST_U8 if dst.dtype == torch.uint8 else L.PNG_DST_F32, n, h, w, both[1].data_ptr(), stream()))
        status = both.cpu().numpy()                        # the one read-back: both status vectors
    for i in keep:
        if status[0][i] != 0 or status[1][i] != 0:         # a frame the inflate refused names that reason: its slot held nothing to unfilter
            refused[i] = int(status[0][i]) or int(status[1][i])
    if info is not None:
        info["upload_bytes"] = buf.numel()


def _pillow_rgb(blob: bytes) -> np.ndarray:
    """the expression the PNG path has to reproduce, and its fallback: an error Pillow raises for a broken file is the caller's"""
    from io import BytesIO
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(BytesIO(blob)).convert("RGB")))


def png_decode(blobs: Sequence[bytes], pool=None, device=None, out: str = "uint8", info: Optional[dict] = None, inflate: str = "host") -> torch.Tensor:
    """encoded PNG frames of ONE size -> uint8 `[n, h, w, 3]` (`out="uint8"`: what `jpeg_decode` returns and `crop_shim` takes) or fp32
    `[n, 3, h, w]` holding k / 255 (`out="float"`: what the metrics consume), the pixels `Image.open(...).convert("RGB")` gives.

    Per frame the host parses the chunks, checks their CRCs and inflates IDAT (`zlib`, no GIL; on `pool`, a `concurrent.futures`
    executor, when one is given) into one pinned staging tensor; then one upload, one `mvldm_png_unfilter` launch -- the five row filters,
    the expansion of grey, grey + alpha, RGBA and palette frames to RGB, the write into the layout asked for -- and ONE small download of
    the frames' status words.  A frame the library refuses (16-bit, grey below 8 bits, interlaced, a filter byte above 4, an inflated
    length other than h * (1 + stride), a bad CRC, no PLTE, not a PNG at all, ...) or that the kernel flags (a palette index beyond the PLTE
    entries) is decoded by Pillow on the host and uploaded into its slot: the result never depends on which path ran.
    `info`: a dict that receives `"fallback"`, the list of (frame number, reason) that took Pillow.
    `device="cpu"` (tests and tools on a machine without a device): the same staging, then the kernel's host twin
    (`mvldm_png_unfilter_host`: the same arithmetic in C++) into a host tensor.
    `inflate="device"` (opt-in; the default `"host"` is the path above): the host still walks the chunks and checks every CRC, but uploads
    the IDAT bytes as they are, and `mvldm_png_inflate` inflates them on the device in front of the unfilter launch (`_png_decode_zdevice`):
    the same pixels, the same fallbacks with the same reasons, and `info["upload_bytes"]`."""
    n = len(blobs)
    if n == 0:
        raise ValueError("png_decode: no frames")
    if inflate not in ("host", "device"):
        raise ValueError(f"png_decode: inflate {inflate!r} (host or device)")
    if out not in ("uint8", "float"):
        raise ValueError(f"png_decode: out {out!r} (uint8 or float)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    on_host = dev.type == "cpu"
    infos = [png_probe(b) for b in blobs]
    sizes = {(p.h, p.w) for p in infos if p.supported}

    def one_size():
        if len(sizes) > 1:
            raise ValueError(f"png_decode: frames of one size, got {sorted(sizes)}")
    one_size()
    refused = {i: p.reason for i, p in enumerate(infos) if not p.supported}
    dst = None
    with (contextlib.nullcontext() if on_host else torch.cuda.device(dev)):
        if len(refused) < n and inflate == "device":
            (h, w), = sizes
            dst = torch.empty((n, h, w, 3) if out == "uint8" else (n, 3, h, w), dtype=torch.uint8 if out == "uint8" else torch.float32, device=dev)
            _png_decode_zdevice(blobs, infos, pool, dev, dst, h, w, refused, info)
        elif len(refused) < n:
            (h, w), = sizes
            offs, end, desc0, total = _png_layout(infos)
            buf = torch.empty(total, dtype=torch.uint8, pin_memory=not on_host)
            host = buf.numpy()
            desc = host[desc0:].view(np.int32).reshape(n, L.PNG_DESC_INTS)
            desc[:] = _PNG_NO_FRAME
            order = sorted(offs)
            reasons = _map(pool, lambda i: _png_stage(blobs[i], infos[i], host, offs[i], end, 768 * i, desc[i]), order)
            refused.update({i: r for i, r in zip(order, reasons) if r})
            dst = torch.empty((n, h, w, 3) if out == "uint8" else (n, 3, h, w), dtype=torch.uint8 if out == "uint8" else torch.float32, device=dev)
            if len(refused) < n and on_host:
                status = png_unfilter_host(host[:end], desc, host[end:end + 768 * n], h, w, dst.numpy())
            elif len(refused) < n:
                status = png_unfilter(buf.to(dev, non_blocking=True), end, desc0, n, h, w, dst).cpu().numpy()       # the one read-back
                refused.update({i: int(status[i]) for i in order if i not in refused and status[i] != 0})
        at = sorted(refused)
        late = _map(pool, _pillow_rgb, [blobs[i] for i in at])
        sizes |= {f.shape[:2] for f in late}
        one_size()
        (h, w), = sizes
        if dst is None:
            dst = torch.empty((n, h, w, 3) if out == "uint8" else (n, 3, h, w), dtype=torch.uint8 if out == "uint8" else torch.float32, device=dev)
        if late:
            host = torch.empty(len(late), h, w, 3, dtype=torch.uint8, pin_memory=not on_host)
            for j, f in enumerate(late):
                host.numpy()[j] = f
            if out == "float":      # k / 255 divided on the host, where torch divides (the device multiplies by a reciprocal: other bits)
                host = (host.permute(0, 3, 1, 2).float() / 255).contiguous()
                host = host if on_host else host.pin_memory()
            dst[torch.tensor(at, device=dev)] = host.to(dev, non_blocking=True)       # after the kernel: a flagged frame's slot is overwritten
    if info is not None:
        info["fallback"] = [(i, L.PNG_REASONS[refused[i]]) for i in at]
    return dst
