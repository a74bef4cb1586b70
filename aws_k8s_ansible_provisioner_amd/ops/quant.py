"""Weight-only quantization: FP8 (OCP e4m3fn, W8A16) and MXFP4 (OCP e2m1 + e8m0, W4A16).

A quantized projection weight is ``Fp8Weight(q, scale)``: ``q`` uint8 [N, K] holding e4m3fn
codes (never the NaN codes 0x7F / 0xFF), ``scale`` fp32 [N], one value per output channel.

    y = x @ w.T   means   Y[m, n] = bf16(scale[n] * sum_k float(X[m, k]) * float(q[n, k]))

accumulated in fp32.  Activations stay bf16: every e4m3 value is exact in bf16, so the GPU
kernel (csrc/kernels/qgemm.hip) streams 1-byte weights, widens them in registers and runs the
bf16 MFMA; the scale multiplies the fp32 accumulators.

``Fp8Experts(q, scale)`` is the same for the experts of an MoE layer: ``q`` uint8 [E, N, K],
``scale`` fp32 [E, N]; expert e follows the contract above with scale[e] (the grouped kernel is
csrc/kernels/moe_qgemm.hip).

``Mxfp4Weight(q, scale)``: ``q`` uint8 [N, K/2] holding two e2m1 codes per byte (element 2j in
the low nibble of byte j, element 2j+1 in the high nibble: torch.float4_e2m1fn_x2's packing),
``scale`` uint8 [N, K/32], one e8m0 code s (value 2^(s-127), 2 <= s <= 252) per 32 elements
along K.

    Y[m, n] = bf16(sum_k float(X[m, k]) * e2m1(q[n, k]) * 2^(scale[n, k/32] - 127))

accumulated in fp32.  An e2m1 value times such a power of two is exact in bf16, so the GPU
kernel (csrc/kernels/q4gemm.hip) streams half-byte weights and widens them, block scale
included, in registers.

``Mxfp4Experts(q, scale)`` is the same for the experts of an MoE layer: ``q`` uint8
[E, N, K/2], ``scale`` uint8 [E, N, K/32]; expert e follows the contract above with q[e] and
scale[e] (the grouped kernel is csrc/kernels/moe_q4gemm.hip, which needs K % 128 == 0).
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


class Fp8Experts:
    """The FP8 weights of a group of MoE experts, [E, N, K]: ``q`` uint8 e4m3fn codes (never a
    NaN code), ``scale`` fp32 [E, N], one value per expert and output channel.  Per expert e

        Y[r, n] = bf16(scale[e, n] * sum_k float(X[r, k]) * float(q[e, n, k]))

    accumulated in fp32 (csrc/kernels/moe_qgemm.hip).  ``w[e]`` is expert e's Fp8Weight, so
    code written for a bf16 [E, N, K] tensor that reads ``w[e].float()`` works unchanged."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dtype == torch.float8_e4m3fn:
            q = q.view(torch.uint8)
        if q.dtype != torch.uint8 or q.dim() != 3:
            raise ValueError("Fp8Experts: q must be a 3-D uint8 / float8_e4m3fn tensor [E, N, K]")
        if scale.dtype != torch.float32 or tuple(scale.shape) != tuple(q.shape[:2]):
            raise ValueError("Fp8Experts: scale must be fp32 [E, N]")
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
        return 3

    def numel(self) -> int:
        return self.q.numel()

    @property
    def nbytes(self) -> int:
        """E * N * K code bytes + 4 * E * N scale bytes."""
        return self.q.numel() + 4 * self.scale.numel()

    def float(self) -> torch.Tensor:
        """The dequantized fp32 tensor float(q) * scale[:, :, None] (exact)."""
        return self.q.view(torch.float8_e4m3fn).float() * self.scale[:, :, None]

    def flat(self) -> Fp8Weight:
        """All experts' channels as one [E * N, K] Fp8Weight (a view: the dequantizer's input)."""
        E, N, K = self.q.shape
        return Fp8Weight(self.q.view(E * N, K), self.scale.view(E * N))

    def __getitem__(self, idx):
        """w[e] -> expert e's Fp8Weight; w[a:b] -> the experts a..b (expert parallelism);
        w[:, :, a:b] / w[:, a:b] -> column / channel slices of every expert (tensor
        parallelism; a column slice keeps the scales, as Fp8Weight does)."""
        idx = idx if isinstance(idx, tuple) else (idx,)
        if len(idx) > 3:
            raise IndexError("Fp8Experts: at most 3 indices")
        ex, rows, cols = tuple(idx) + (slice(None),) * (3 - len(idx))
        if not (isinstance(rows, slice) and isinstance(cols, slice)):
            raise TypeError("Fp8Experts supports channel and column slices only")
        if isinstance(ex, int):
            return Fp8Weight(self.q[ex, rows, cols], self.scale[ex, rows])
        if not isinstance(ex, slice):
            raise TypeError("Fp8Experts: the expert index is an int or a slice")
        return Fp8Experts(self.q[ex, rows, cols], self.scale[ex, rows])

    def to(self, device) -> "Fp8Experts":
        return Fp8Experts(self.q.to(device), self.scale.to(device))

    def __repr__(self) -> str:
        return f"Fp8Experts(shape={tuple(self.shape)}, device={self.device})"


@torch.no_grad()
def quantize_fp8_experts(w: torch.Tensor) -> Fp8Experts:
    """quantize_fp8's rule per expert and output channel of w [E, N, K]."""
    if w.dim() != 3:
        raise ValueError("quantize_fp8_experts: 3-D weight [E, N, K]")
    E, N, K = w.shape
    q = torch.empty(E, N, K, dtype=torch.uint8, device=w.device)
    scale = torch.empty(E, N, dtype=torch.float32, device=w.device)
    for e in range(E):  # one expert's fp32 temporaries at a time
        f = quantize_fp8(w[e])
        q[e].copy_(f.q)
        scale[e].copy_(f.scale)
    return Fp8Experts(q, scale)


def dequant_fp8_experts(w: Fp8Experts) -> torch.Tensor:
    """bf16(float(q) * scale) of all experts as a [E, N, K] view of the shared scratch (GPU:
    the dequant_fp8 kernel, bit-exact; stream-ordered like every other use of the scratch,
    never inside a captured region) or a new tensor (CPU)."""
    if not w.is_cuda:
        return w.float().to(torch.bfloat16)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("fp8 experts are not dequantized inside a captured region")
    from . import load_native

    load_native(required=True)
    if w.shape[2] % 16:
        raise ValueError(f"fp8 experts {tuple(w.shape)}: K must be a multiple of 16")
    return _dequant_to_scratch(w.flat()).view(w.shape)


# ------------------------------------------------------------------ MXFP4
MX_BLOCK = 32                     # elements along K that share one e8m0 scale
MX_SCALE_MIN, MX_SCALE_MAX = 2, 252  # accepted e8m0 codes: 0.5 * 2^e and 6 * 2^e normal in bf16
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


class Mxfp4Weight:
    """MXFP4 weight [N, K]: packed e2m1 codes uint8 [N, K/2] and e8m0 block scales uint8
    [N, K/32]; stands where a bf16 weight tensor did."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor, check: bool = True):
        fp4 = getattr(torch, "float4_e2m1fn_x2", None)
        if fp4 is not None and q.dtype == fp4:
            q = q.view(torch.uint8)
        e8m0 = getattr(torch, "float8_e8m0fnu", None)
        if e8m0 is not None and scale.dtype == e8m0:
            scale = scale.view(torch.uint8)
        if q.dtype != torch.uint8 or q.dim() != 2:
            raise ValueError("Mxfp4Weight: q must be a 2-D uint8 tensor [N, K/2]")
        if q.shape[1] % (MX_BLOCK // 2):
            raise ValueError(f"Mxfp4Weight: K = {2 * q.shape[1]} must be a multiple of {MX_BLOCK}")
        if (scale.dtype != torch.uint8 or scale.dim() != 2
                or tuple(scale.shape) != (q.shape[0], q.shape[1] // (MX_BLOCK // 2))):
            raise ValueError("Mxfp4Weight: scale must be uint8 [N, K/32] (e8m0 codes)")
        # check=False: slices and copies of a weight that was checked when it was built
        bad = (scale < MX_SCALE_MIN) | (scale > MX_SCALE_MAX)
        if check and scale.numel() and bool(bad.any()):
            raise ValueError(f"Mxfp4Weight: e8m0 scale codes must lie in [{MX_SCALE_MIN}, "
                             f"{MX_SCALE_MAX}] (255 is NaN; outside, a dequantized value is not "
                             f"a normal bf16 number)")
        self.q = q.contiguous()
        self.scale = scale.contiguous()

    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.q.shape[0], 2 * self.q.shape[1]))

    @property
    def device(self) -> torch.device:
        return self.q.device

    @property
    def is_cuda(self) -> bool:
        return self.q.is_cuda

    @property
    def dtype(self) -> torch.dtype:
        return getattr(torch, "float4_e2m1fn_x2", torch.uint8)

    def dim(self) -> int:
        return 2

    def numel(self) -> int:
        return 2 * self.q.numel()

    @property
    def nbytes(self) -> int:
        """N * K / 2 code bytes + N * K / 32 scale bytes."""
        return self.q.numel() + self.scale.numel()

    def float(self) -> torch.Tensor:
        """The dequantized fp32 matrix e2m1(q) * 2^(scale - 127) (exact)."""
        lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32,
                           device=self.device)
        q = self.q.long()
        v = torch.stack((lut[q & 15], lut[q >> 4]), dim=-1).reshape(self.shape)
        s = torch.ldexp(torch.ones((), device=self.device), self.scale.to(torch.int32) - 127)
        return v * s.repeat_interleave(MX_BLOCK, dim=1)

    def __getitem__(self, idx) -> "Mxfp4Weight":
        """Row / column slices (tensor-parallel sharding): w[a:b] slices codes and scales by
        rows, w[:, a:b] by columns, where a and b must be multiples of 32 (whole scale blocks)."""
        rows, cols = idx if isinstance(idx, tuple) else (idx, slice(None))
        if not (isinstance(rows, slice) and isinstance(cols, slice)):
            raise TypeError("Mxfp4Weight supports slices only")
        a, b, step = cols.indices(self.shape[1])
        if step != 1 or a % MX_BLOCK or b % MX_BLOCK:
            raise ValueError(f"Mxfp4Weight: column slice [{a}:{b}] must start and end on "
                             f"multiples of {MX_BLOCK}")
        return Mxfp4Weight(self.q[rows, a // 2:b // 2],
                           self.scale[rows, a // MX_BLOCK:b // MX_BLOCK], check=False)

    def to(self, device) -> "Mxfp4Weight":
        return Mxfp4Weight(self.q.to(device), self.scale.to(device), check=False)

    def __repr__(self) -> str:
        return f"Mxfp4Weight(shape={tuple(self.shape)}, device={self.device})"


# what ops.linear / linear_silu, the loader and the byte accounting test a weight against
QuantWeight = (Fp8Weight, Mxfp4Weight)


@torch.no_grad()
def quantize_mxfp4(w: torch.Tensor) -> Mxfp4Weight:
    """The OCP MX rule per block of 32 along K: e = floor(log2(amax)) - 2 (scale code e + 127,
    clamped to 2..252; 127 for an all-zero block), code = RNE(w / 2^e) onto the e2m1 grid
    {0, .5, 1, 1.5, 2, 3, 4, 6}, saturated at +-6."""
    if w.dim() != 2 or w.shape[1] % MX_BLOCK:
        raise ValueError(f"quantize_mxfp4: 2-D weight with K a multiple of {MX_BLOCK}")
    N, K = w.shape
    w32 = w.float().reshape(N, K // MX_BLOCK, MX_BLOCK)
    amax = w32.abs().amax(dim=2)
    ex = torch.frexp(amax)[1] - 1  # floor(log2(amax)), exact (amax = m * 2^(ex + 1), m in [.5, 1))
    code = torch.where(amax > 0, ex - 2 + 127, torch.full_like(ex, 127))
    code = code.clamp_(MX_SCALE_MIN, MX_SCALE_MAX)
    a = torch.ldexp(w32.abs(), (127 - code)[:, :, None])  # |w| / 2^e, exact
    # RNE onto the grid: steps of 0.5 below 2, of 1 below 4, of 2 above (torch.round is
    # round-half-to-even, and the even neighbour is the even e2m1 mantissa at every tie)
    r = torch.where(a < 2, torch.round(a * 2) / 2,
                    torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2)).clamp_(max=6.0)
    grid = torch.tensor(_E2M1, dtype=torch.float32, device=w.device)
    c = torch.bucketize(r, grid)
    c = torch.where((w32 < 0) & (c > 0), c + 8, c).to(torch.uint8).reshape(N, K)
    return Mxfp4Weight(c[:, 0::2] | (c[:, 1::2] << 4), code.to(torch.uint8), check=False)


class Mxfp4Experts:
    """The MXFP4 weights of a group of MoE experts, [E, N, K]: ``q`` uint8 [E, N, K/2] (two e2m1
    codes per byte, element 2j in the low nibble: Mxfp4Weight's packing), ``scale`` uint8
    [E, N, K/32] of e8m0 codes in 2..252.  Per expert e

        Y[r, n] = bf16(sum_k float(X[r, k]) * e2m1(q[e, n, k]) * 2^(scale[e, n, k/32] - 127))

    accumulated in fp32 (csrc/kernels/moe_q4gemm.hip).  ``w[e]`` is expert e's Mxfp4Weight, so
    code written for a bf16 [E, N, K] tensor that reads ``w[e].float()`` works unchanged."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor, check: bool = True):
        fp4 = getattr(torch, "float4_e2m1fn_x2", None)
        if fp4 is not None and q.dtype == fp4:
            q = q.view(torch.uint8)
        e8m0 = getattr(torch, "float8_e8m0fnu", None)
        if e8m0 is not None and scale.dtype == e8m0:
            scale = scale.view(torch.uint8)
        if q.dtype != torch.uint8 or q.dim() != 3:
            raise ValueError("Mxfp4Experts: q must be a 3-D uint8 tensor [E, N, K/2]")
        if q.shape[2] % (MX_BLOCK // 2):
            raise ValueError(f"Mxfp4Experts: K = {2 * q.shape[2]} must be a multiple of {MX_BLOCK}")
        if (scale.dtype != torch.uint8 or scale.dim() != 3
                or tuple(scale.shape) != (q.shape[0], q.shape[1], q.shape[2] // (MX_BLOCK // 2))):
            raise ValueError("Mxfp4Experts: scale must be uint8 [E, N, K/32] (e8m0 codes)")
        # check=False: slices and copies of a weight that was checked when it was built
        if check and scale.numel() and bool(((scale < MX_SCALE_MIN) | (scale > MX_SCALE_MAX)).any()):
            raise ValueError(f"Mxfp4Experts: e8m0 scale codes must lie in [{MX_SCALE_MIN}, "
                             f"{MX_SCALE_MAX}] (255 is NaN; outside, a dequantized value is not "
                             f"a normal bf16 number)")
        self.q = q.contiguous()
        self.scale = scale.contiguous()

    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.q.shape[0], self.q.shape[1], 2 * self.q.shape[2]))

    @property
    def device(self) -> torch.device:
        return self.q.device

    @property
    def is_cuda(self) -> bool:
        return self.q.is_cuda

    @property
    def dtype(self) -> torch.dtype:
        return getattr(torch, "float4_e2m1fn_x2", torch.uint8)

    def dim(self) -> int:
        return 3

    def numel(self) -> int:
        return 2 * self.q.numel()

    @property
    def nbytes(self) -> int:
        """E * N * K / 2 code bytes + E * N * K / 32 scale bytes."""
        return self.q.numel() + self.scale.numel()

    def flat(self) -> Mxfp4Weight:
        """All experts' channels as one [E * N, K] Mxfp4Weight (a view: the dequantizer's
        input)."""
        E, N, K2 = self.q.shape
        return Mxfp4Weight(self.q.view(E * N, K2), self.scale.view(E * N, -1), check=False)

    def float(self) -> torch.Tensor:
        """The dequantized fp32 tensor e2m1(q) * 2^(scale - 127) (exact)."""
        return self.flat().float().view(self.shape)

    def __getitem__(self, idx):
        """w[e] -> expert e's Mxfp4Weight; w[a:b] -> the experts a..b (expert parallelism);
        w[:, :, a:b] / w[:, a:b] -> column / channel slices of every expert (tensor
        parallelism; column bounds must be multiples of 32, whole scale blocks)."""
        idx = idx if isinstance(idx, tuple) else (idx,)
        if len(idx) > 3:
            raise IndexError("Mxfp4Experts: at most 3 indices")
        ex, rows, cols = tuple(idx) + (slice(None),) * (3 - len(idx))
        if not (isinstance(rows, slice) and isinstance(cols, slice)):
            raise TypeError("Mxfp4Experts supports channel and column slices only")
        a, b, step = cols.indices(self.shape[2])
        if step != 1 or a % MX_BLOCK or b % MX_BLOCK:
            raise ValueError(f"Mxfp4Experts: column slice [{a}:{b}] must start and end on "
                             f"multiples of {MX_BLOCK}")
        qc, sc = slice(a // 2, b // 2), slice(a // MX_BLOCK, b // MX_BLOCK)
        if isinstance(ex, int):
            return Mxfp4Weight(self.q[ex, rows, qc], self.scale[ex, rows, sc], check=False)
        if not isinstance(ex, slice):
            raise TypeError("Mxfp4Experts: the expert index is an int or a slice")
        return Mxfp4Experts(self.q[ex, rows, qc], self.scale[ex, rows, sc], check=False)

    def to(self, device) -> "Mxfp4Experts":
        return Mxfp4Experts(self.q.to(device), self.scale.to(device), check=False)

    def __repr__(self) -> str:
        return f"Mxfp4Experts(shape={tuple(self.shape)}, device={self.device})"


# what ops.fused_moe, MoEBlock and the byte accounting test an expert weight against
QuantExperts = (Fp8Experts, Mxfp4Experts)


@torch.no_grad()
def quantize_mxfp4_experts(w: torch.Tensor) -> Mxfp4Experts:
    """quantize_mxfp4's rule per expert of w [E, N, K]."""
    if w.dim() != 3 or w.shape[2] % MX_BLOCK:
        raise ValueError(f"quantize_mxfp4_experts: 3-D weight [E, N, K], K a multiple of {MX_BLOCK}")
    E, N, K = w.shape
    q = torch.empty(E, N, K // 2, dtype=torch.uint8, device=w.device)
    scale = torch.empty(E, N, K // MX_BLOCK, dtype=torch.uint8, device=w.device)
    for e in range(E):  # one expert's fp32 temporaries at a time
        f = quantize_mxfp4(w[e])
        q[e].copy_(f.q)
        scale[e].copy_(f.scale)
    return Mxfp4Experts(q, scale, check=False)


def dequant_mxfp4_experts(w: Mxfp4Experts) -> torch.Tensor:
    """bf16(e2m1(q) * 2^(scale - 127)) of all experts as a [E, N, K] view of the shared scratch
    (GPU: the dequant_mxfp4 kernel, bit-exact; stream-ordered like every other use of the
    scratch, never inside a captured region) or a new tensor (CPU)."""
    if not w.is_cuda:
        return w.float().to(torch.bfloat16)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("mxfp4 experts are not dequantized inside a captured region")
    from . import load_native

    load_native(required=True)
    f = w.flat()
    reserve_scratch(f.numel(), f.device)
    out = _scratch[f.device][: f.numel()].view(f.shape)
    torch.ops.akap.dequant_mxfp4(out, f.q, f.scale)
    return out.view(w.shape)


def dequant_experts(w) -> torch.Tensor:
    """dequant_fp8_experts / dequant_mxfp4_experts by container."""
    if isinstance(w, Mxfp4Experts):
        return dequant_mxfp4_experts(w)
    return dequant_fp8_experts(w)


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


# ------------------------------------------------------------------ MXFP4 on the GPU
def dequant_mxfp4(w: Mxfp4Weight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16(e2m1(q) * 2^(scale - 127)) as a new (or given) bf16 tensor; GPU: the HIP kernel."""
    if out is None:
        out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
    if w.is_cuda:
        from . import load_native

        load_native(required=True)
        torch.ops.akap.dequant_mxfp4(out, w.q, w.scale)
    else:
        out.copy_(w.float().to(torch.bfloat16))
    return out


def q4gemm_supported(x: torch.Tensor, w: Mxfp4Weight, out: Optional[torch.Tensor] = None) -> bool:
    """Whether torch.ops.akap.q4gemm takes the launch: the kernel's shape predicate and the
    tensor properties ops.cpp checks (out=None: a fresh dense [M, N] output)."""
    N, K = w.shape
    return (x.dim() == 2 and x.dtype == torch.bfloat16 and x.stride(-1) == 1
            and x.data_ptr() % 16 == 0
            and (out is None or (out.dim() == 2 and out.stride(-1) == 1
                                 and out.data_ptr() % 16 == 0))
            and _contract().q4gemm_supported(x.shape[0], N, K, x.stride(0),
                                             N if out is None else out.stride(0)))


def linear_mxfp4(x: torch.Tensor, w: Mxfp4Weight,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T for an Mxfp4Weight (the contract at the top of this file)."""
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
    if q4gemm_supported(x, w, out):
        if out is None:
            out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        torch.ops.akap.q4gemm(out, x, w.q, w.scale)
        return out
    # prefill and mixed steps: dequantize into the shared scratch, then the bf16 GEMM
    reserve_scratch(w.numel(), w.device)
    wd = _scratch[w.device][: w.numel()].view(w.shape)
    torch.ops.akap.dequant_mxfp4(wd, w.q, w.scale)
    return linear(x, wd, out=out)


def linear_quant(x: torch.Tensor, w, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T for any QuantWeight."""
    if isinstance(w, Mxfp4Weight):
        return linear_mxfp4(x, w, out=out)
    return linear_fp8(x, w, out=out)
