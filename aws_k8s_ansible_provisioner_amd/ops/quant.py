"""FP8 (OCP e4m3fn) weight-only quantization, W8A16.

A quantized projection weight is ``Fp8Weight(q, scale)``: ``q`` uint8 [N, K] holding e4m3fn
codes (never the NaN codes 0x7F / 0xFF), ``scale`` fp32 [N], one value per output channel.

    y = x @ w.T   means   Y[m, n] = bf16(scale[n] * sum_k float(X[m, k]) * float(q[n, k]))

accumulated in fp32.  Activations stay bf16: every e4m3 value is exact in bf16, so the GPU
kernel (csrc/kernels/qgemm.hip) streams 1-byte weights, widens them in registers and runs the
bf16 MFMA; the scale multiplies the fp32 accumulators.
"""
from __future__ import annotations

from typing import Optional

import torch

from .._runtime_loader import contract as _contract

FP8_MAX = 448.0


def __getattr__(name: str):
    if name == "QGEMM_MAX_M":  # rows one qgemm launch covers; above: dequantize + bf16 GEMM
        return _contract().QGEMM_MAX_M
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class Fp8Weight:
    """Per-output-channel scaled e4m3fn weight [N, K]; stands where a bf16 weight tensor did."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dtype == torch.float8_e4m3fn:
            q = q.view(torch.uint8)
        if q.dtype != torch.uint8 or q.dim() != 2:
            raise ValueError("Fp8Weight: q must be a 2-D uint8 / float8_e4m3fn tensor")
        if scale.dtype != torch.float32 or scale.shape != (q.shape[0],):
            raise ValueError("Fp8Weight: scale must be fp32 [N]")
        self.q = q.contiguous()
        self.scale = scale.contiguous()

    @property
    def shape(self) -> torch.Size:
        return self.q.shape

    @property
    def device(self) -> torch.device:
        return self.q.device

    @property
    def is_cuda(self) -> bool:
        return self.q.is_cuda

    @property
    def dtype(self) -> torch.dtype:
        return torch.float8_e4m3fn

    def dim(self) -> int:
        return 2

    def numel(self) -> int:
        return self.q.numel()

    @property
    def nbytes(self) -> int:
        """N * K code bytes + 4 * N scale bytes."""
        return self.q.numel() + 4 * self.scale.numel()

    def float(self) -> torch.Tensor:
        """The dequantized fp32 matrix float(q) * scale[:, None] (exact)."""
        return self.q.view(torch.float8_e4m3fn).float() * self.scale[:, None]

    def __getitem__(self, idx) -> "Fp8Weight":
        """Row / column slices (tensor-parallel sharding): w[a:b] slices codes and scales,
        w[:, a:b] slices the codes of every channel and keeps its scale."""
        rows, cols = idx if isinstance(idx, tuple) else (idx, slice(None))
        if not (isinstance(rows, slice) and isinstance(cols, slice)):
            raise TypeError("Fp8Weight supports slices only")
        return Fp8Weight(self.q[rows, cols], self.scale[rows])

    def to(self, device) -> "Fp8Weight":
        return Fp8Weight(self.q.to(device), self.scale.to(device))

    def __repr__(self) -> str:
        return f"Fp8Weight(shape={tuple(self.shape)}, device={self.device})"


@torch.no_grad()
def quantize_fp8(w: torch.Tensor) -> Fp8Weight:
    """scale[n] = absmax(w[n, :]) / 448 (1.0 for an all-zero row); q = RNE(w / scale), clamped
    to +-448 before the cast (torch's float8 cast does not saturate)."""
    if w.dim() != 2:
        raise ValueError("quantize_fp8: 2-D weight")
    w32 = w.float()
    amax = w32.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (w32 / scale[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return Fp8Weight(q.view(torch.uint8), scale)


# ------------------------------------------------------------------ dequantization scratch
# One bf16 buffer per device, as large as the largest quantized weight: the prefill / mixed
# step path dequantizes a weight into it and runs the bf16 GEMM on it.  The NEXT call reuses
# the same bytes.  That is correct because every launch that writes or reads the scratch runs
# in stream order on the engine's one compute stream: the dequantize of call i+1 is queued
# behind the GEMM of call i.  It is allocated when a model is quantized (reserve_scratch),
# never inside a captured region.
_scratch: dict = {}


def reserve_scratch(numel: int, device) -> None:
    device = torch.device(device)
    if device.type != "cuda":
        return
    cur = _scratch.get(device)
    if cur is not None and cur.numel() >= numel:
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("fp8 dequantization scratch must be reserved before graph capture")
    _scratch[device] = None  # drop the old one first
    _scratch[device] = torch.empty(numel, dtype=torch.bfloat16, device=device)


def _dequant_to_scratch(w: Fp8Weight) -> torch.Tensor:
    reserve_scratch(w.numel(), w.device)
    out = _scratch[w.device][: w.numel()].view(w.shape)
    torch.ops.akap.dequant_fp8(out, w.q, w.scale)
    return out


def dequant_fp8(w: Fp8Weight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16(float(q) * scale[:, None]) as a new (or given) bf16 tensor; GPU: the HIP kernel."""
    if out is None:
        out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
    if w.is_cuda:
        from . import load_native

        load_native(required=True)
        torch.ops.akap.dequant_fp8(out, w.q, w.scale)
    else:
        out.copy_(w.float().to(torch.bfloat16))
    return out


def qgemm_supported(x: torch.Tensor, w: Fp8Weight, out: Optional[torch.Tensor] = None) -> bool:
    """Whether torch.ops.akap.qgemm takes the launch: the kernel's shape predicate and the
    tensor properties ops.cpp checks (out=None: a fresh dense [M, N] output)."""
    N, K = w.shape
    return (x.dim() == 2 and x.dtype == torch.bfloat16 and x.stride(-1) == 1
            and x.data_ptr() % 16 == 0
            and (out is None or (out.dim() == 2 and out.stride(-1) == 1
                                 and out.data_ptr() % 16 == 0))
            and _contract().qgemm_supported(x.shape[0], N, K, x.stride(0),
                                            N if out is None else out.stride(0)))


def linear_fp8(x: torch.Tensor, w: Fp8Weight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T for an Fp8Weight (the contract at the top of this file)."""
    if not x.is_cuda:
        y = (x.float() @ w.float().t()).to(x.dtype)
        if out is not None:
            out.copy_(y)
            return out
        return y
    from . import linear, load_native

    load_native(required=True)
    if x.shape[0] == 0:
        return out if out is not None else x.new_empty(0, w.shape[0])
    if qgemm_supported(x, w, out):
        if out is None:
            out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        torch.ops.akap.qgemm(out, x, w.q, w.scale)
        return out
    if w.shape[1] % 16:
        raise ValueError(f"fp8 weight {tuple(w.shape)}: K must be a multiple of 16")
    # prefill and mixed steps: dequantize into the shared scratch, then the bf16 GEMM
    return linear(x, _dequant_to_scratch(w), out=out)
