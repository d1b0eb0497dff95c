"""MXFP4 (OCP MX: e2m1 elements, one E8M0 scale per 32) weight-only decode (``model.fp4_decode``).

Format of a bf16 weight ``W [N, K]``, ``K % 32 == 0`` (row-major, public):

* blocks of 32 consecutive k of one row; scale byte ``s = e + 127`` with
  ``e = floor(log2(amax)) - 2`` (2 = e2m1 emax) read from the float's exponent field, clamped to
  [-127, 127]; an all-zero block has ``e = 0``;
* elements ``x / 2^e`` (exact), magnitude saturated at 6 and rounded to nearest-even on the e2m1
  grid {0, .5, 1, 1.5, 2, 3, 4, 6}; the sign bit is the input's, also when the magnitude rounds
  to 0;
* ``codes [N, K / 2]`` uint8, element ``2 i`` in the low nibble of byte ``i``;
  ``scales [N, K / 32]`` uint8.

A widened MXFP4 weight is exactly a bf16 number, so the decode kernel (``gemv16_kernel<ImgFp4>``,
M <= 16) widens in registers with the hardware e2m1 -> bf16 conversion and runs the bf16 MFMA: a
quarter of the bf16 weight bytes per token. Round-to-nearest MXFP4 carries ~11 % relative rms
weight error on Gaussian weights: an opt-in latency / quality trade (docs/DESIGN.md).

Weights must be finite: a NaN or infinity in a block has no defined scale here (the GPU quantiser's
``fmaxf`` drops a NaN that ``torch.amax`` propagates), so the bitwise contract covers finite
inputs only.

CPU tensors run the eager implementation below, which is also the oracle of the GPU quantiser
(bitwise: the scale is a power of two and the rounding is a chain of threshold compares).
"""
from __future__ import annotations

import torch

from ._ext import native, on_gpu

E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32


def fp4_supported(w: torch.Tensor, act: int = 0) -> bool:
    """Shapes the decode image serves: 2-D, N % 16 == 0 (the [gate; up] pair of SwiGLU, act 5:
    N % 64 == 0) and K % 256 == 0 (one 2-KiB chunk of a 16-row group)."""
    return w.dim() == 2 and w.shape[0] > 0 and w.shape[0] % (64 if act == 5 else 16) == 0 and w.shape[1] > 0 \
        and w.shape[1] % 256 == 0


def _quantize_eager(w: torch.Tensor):
    N, K = w.shape
    x = w.detach().float().reshape(N, K // BLOCK, BLOCK)
    amax = x.abs().amax(-1)
    field = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    e = torch.where(amax == 0, torch.zeros_like(field), (field - 127 - 2).clamp(-127, 127))
    a = torch.ldexp(x.abs(), (-e)[..., None])
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
            + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = (code | (torch.signbit(x).to(torch.uint8) << 3)).reshape(N, K // 2, 2)
    codes = code[..., 0] | (code[..., 1] << 4)
    return codes.contiguous(), (e + 127).to(torch.uint8).contiguous()


def quantize_mxfp4(w: torch.Tensor):
    """bf16 ``[N, K]`` (K % 32 == 0) -> (codes uint8 [N, K / 2], scales uint8 [N, K / 32])."""
    if w.dim() != 2 or w.shape[1] % BLOCK != 0 or w.numel() == 0:
        raise ValueError(f"quantize_mxfp4: [N, K] with K % 32 == 0 expected, got {tuple(w.shape)}")
    if w.dtype != torch.bfloat16:
        raise ValueError(f"quantize_mxfp4: bfloat16 weight expected, got {w.dtype}")
    if on_gpu(w):
        q, s = native().quant_mxfp4(w.detach().contiguous())
        return q, s
    return _quantize_eager(w)


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(codes [N, K / 2], scales [N, K / 32]) -> fp32 ``[N, K]`` (every value is a bf16 number)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or tuple(scales.shape) != (N, K // BLOCK):
        raise ValueError("dequantize_mxfp4: uint8 codes [N, K / 2] and scales [N, K / 32] expected")
    nib = torch.stack((codes & 0xF, codes >> 4), -1).reshape(N, K // BLOCK, BLOCK).long()
    grid = torch.tensor(E2M1_GRID, dtype=torch.float32, device=codes.device)
    mag = grid[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag)
    return torch.ldexp(val, (scales.to(torch.int32) - 127)[..., None]).reshape(N, K)


# row-major staging buffers of the GPU refresh, one pair per (device, shape), shared by every cache:
# only the tile-ordered image of a weight stays resident (a second, row-major copy per weight would
# double the footprint: ~3.5 GB for a 7B model)
_STAGE = {}


def _stage(w: torch.Tensor):
    key = (w.device, w.shape[0], w.shape[1])
    buf = _STAGE.get(key)
    if buf is None:
        N, K = w.shape
        buf = _STAGE[key] = (torch.empty(N, K // 2, dtype=torch.uint8, device=w.device),
                             torch.empty(N, K // BLOCK, dtype=torch.uint8, device=w.device))
    return buf


class Fp4Cache(dict):
    """MXFP4 image of one weight (sibling of ``Fp8Cache`` / ``ShufCache``). On the GPU it holds the
    tile-ordered decode image of the 16-row W4A16 kernel (``image``), quantised through a shared
    row-major staging buffer; on the CPU the row-major codes and scales (``get``). Rebuilt in
    place when the source's data pointer or version changes (graph-safe addresses)."""

    def get_key(self):
        return dict.get(self, "key")

    @torch.no_grad()
    def get(self, w: torch.Tensor):
        """(codes, scales), row-major. CPU: the cached pair. GPU: a fresh quantisation (the cache
        keeps only the image there)."""
        if on_gpu(w):
            return quantize_mxfp4(w)
        key = (w.data_ptr(), w._version)
        if self.get_key() != key:
            q, s = quantize_mxfp4(w)
            old = dict.get(self, "q")
            if old is not None and old.shape == q.shape and old.device == q.device:
                self["q"].copy_(q)
                self["s"].copy_(s)
            else:
                self["q"], self["s"] = q, s
            self["key"] = key
        return self["q"], self["s"]

    @torch.no_grad()
    def image(self, w: torch.Tensor):
        """(code image, scale image) of the 16-row kernel (GPU, ``fp4_supported(w)``)."""
        key = (w.data_ptr(), w._version)
        if self.get_key() != key:
            q, s = _stage(w)
            native().quant_mxfp4(w.detach().contiguous(), q, s)
            img = dict.get(self, "img")
            if img is None or img.shape != q.shape or img.device != q.device:
                self["img"], self["simg"] = native().shuffle_decode_weight_fp4(q, s)
            else:
                native().shuffle_decode_weight_fp4(q, s, img, self["simg"])
            self["key"] = key
        return self["img"], self["simg"]
