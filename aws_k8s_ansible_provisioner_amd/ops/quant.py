"""Weight-only quantization: FP8 (OCP e4m3fn, W8A16) and MXFP4 (OCP e2m1 + e8m0, W4A16).

Each format is one ``QuantFormat`` in ``FORMATS`` (below): its packing, scale layout, checks,
quantizer, checkpoint form and GPU ops.  The containers and functions of this file are written
once on that description; ``Fp8Weight`` / ``Mxfp4Weight`` ([N, K]) and ``Fp8Experts`` /
``Mxfp4Experts`` ([E, N, K], the experts of an MoE layer) only bind a format to a container.

fp8: ``q`` uint8 [N, K] holding e4m3fn codes (never the NaN codes 0x7F / 0xFF), ``scale`` fp32
[N], one value per output channel.

    y = x @ w.T   means   Y[m, n] = bf16(scale[n] * sum_k float(X[m, k]) * float(q[n, k]))

accumulated in fp32.  Activations stay bf16: every e4m3 value is exact in bf16, so the GPU
kernel (csrc/kernels/qgemm.hip) streams 1-byte weights, widens them in registers and runs the
bf16 MFMA; the scale multiplies the fp32 accumulators.

mxfp4: ``q`` uint8 [N, K/2] holding two e2m1 codes per byte (element 2j in the low nibble of
byte j, element 2j+1 in the high nibble: torch.float4_e2m1fn_x2's packing), ``scale`` uint8
[N, K/32], one e8m0 code s (value 2^(s-127), 2 <= s <= 252) per 32 elements along K.

    Y[m, n] = bf16(sum_k float(X[m, k]) * e2m1(q[n, k]) * 2^(scale[n, k/32] - 127))

accumulated in fp32.  An e2m1 value times such a power of two is exact in bf16, so the GPU
kernel (csrc/kernels/q4gemm.hip) streams half-byte weights and widens them, block scale
included, in registers.

Experts carry one more leading dimension on ``q`` and ``scale``; expert e follows its format's
contract with q[e] and scale[e] (the grouped kernels are csrc/kernels/moe_qgemm.hip and
moe_q4gemm.hip, which needs K % 128 == 0).
"""
from __future__ import annotations

from typing import Optional

import torch

from .._runtime_loader import contract as _contract

FP8_MAX = 448.0
MX_BLOCK = 32                     # elements along K that share one e8m0 scale
MX_SCALE_MIN, MX_SCALE_MAX = 2, 252  # accepted e8m0 codes: 0.5 * 2^e and 6 * 2^e normal in bf16
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def __getattr__(name: str):
    if name == "QGEMM_MAX_M":  # rows one qgemm launch covers; above: dequantize + bf16 GEMM
        return _contract().QGEMM_MAX_M
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _dtypes(*names: str) -> tuple:
    """The torch dtypes of these names that this torch has."""
    return tuple(getattr(torch, n) for n in names if hasattr(torch, n))


class QuantFormat:
    """Everything that differs between the weight formats; FORMATS holds one per format.

    name         "fp8" | "mxfp4": the --quantization / --expert-quantization value
    per_byte     code elements per byte of ``q``
    block        elements along K that share a scale (0: one scale per output channel)
    scale_dtype  of the container's ``scale``; scale_codes: its accepted (min, max) or None
    code_view / scale_view   torch dtypes a constructor takes in place of uint8 (viewed)
    ckpt_dtypes / ckpt_scale_dtypes   what a checkpoint's `weight` / `weight_scale` of this
                 format may be (an fp8 scale is whatever is no other format's)
    quantize     2-D tensor -> this format's 2-D container (the rounding rule)
    to_float     (q, scale) of a 2-D weight -> the exact fp32 matrix
    export       (q, scale) of a 2-D weight -> the HF `weight`, `weight_scale` tensors
    gemm / dequant / moe_gemm   names of the torch.ops.akap ops; supported: the host predicate
    dequant_k    the multiple of K the dequantize op needs
    q_text / scale_text   the layouts, for error messages ({n}: the leading dimensions)
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.Weight = self.Experts = None  # the containers, bound below

    @property
    def dtype(self) -> torch.dtype:
        return getattr(torch, self.code_view, torch.uint8)

    def scale_shape(self, lead, K: int) -> tuple:
        """The scale's shape for codes of leading dimensions `lead` ((N,) or (E, N)) and K."""
        return tuple(lead) + ((K // self.block,) if self.block else ())

    def check(self, who: str, q: torch.Tensor, scale: torch.Tensor, nd: int, check: bool):
        """The constructor's views and refusals; returns (q, scale) as uint8 / scale_dtype."""
        n = "N" if nd == 2 else "E, N"
        if q.dtype in _dtypes(self.code_view):
            q = q.view(torch.uint8)
        if self.scale_view and scale.dtype in _dtypes(self.scale_view):
            scale = scale.view(torch.uint8)
        if q.dtype != torch.uint8 or q.dim() != nd:
            raise ValueError(f"{who}: q must be a {nd}-D {self.q_text.format(n=n)} tensor")
        K = q.shape[-1] * self.per_byte
        if self.block and K % self.block:
            raise ValueError(f"{who}: K = {K} must be a multiple of {self.block}")
        if scale.dtype != self.scale_dtype or tuple(scale.shape) != self.scale_shape(q.shape[:-1], K):
            raise ValueError(f"{who}: scale must be {self.scale_text.format(n=n)}")
        # check=False: slices and copies of a weight that was checked when it was built
        if check and self.scale_codes and scale.numel():
            lo, hi = self.scale_codes
            if bool(((scale < lo) | (scale > hi)).any()):
                raise ValueError(f"{who}: e8m0 scale codes must lie in [{lo}, {hi}] (255 is NaN; "
                                 f"outside, a dequantized value is not a normal bf16 number)")
        return q, scale

    def col_slices(self, who: str, cols: slice, K: int) -> tuple:
        """A column slice as (slice of q's last dimension, index tuple of scale's block
        dimension): any slice with per-channel scales, whole scale blocks otherwise."""
        if not self.block:
            return cols, ()
        a, b, step = cols.indices(K)
        if step != 1 or a % self.block or b % self.block:
            raise ValueError(f"{who}: column slice [{a}:{b}] must start and end on "
                             f"multiples of {self.block}")
        return (slice(a // self.per_byte, b // self.per_byte),
                (slice(a // self.block, b // self.block),))


class _Quant:
    """What a 2-D weight and a 3-D expert container share; stands where a bf16 tensor did."""

    __slots__ = ()
    fmt: QuantFormat
    _nd: int

    def __init__(self, q: torch.Tensor, scale: torch.Tensor, check: bool = True):
        q, scale = self.fmt.check(type(self).__name__, q, scale, self._nd, check)
        self.q = q.contiguous()
        self.scale = scale.contiguous()

    @property
    def shape(self) -> torch.Size:
        return torch.Size((*self.q.shape[:-1], self.q.shape[-1] * self.fmt.per_byte))

    @property
    def device(self) -> torch.device:
        return self.q.device

    @property
    def is_cuda(self) -> bool:
        return self.q.is_cuda

    @property
    def dtype(self) -> torch.dtype:
        return self.fmt.dtype

    def dim(self) -> int:
        return self._nd

    def numel(self) -> int:
        return self.fmt.per_byte * self.q.numel()

    @property
    def nbytes(self) -> int:
        """Code bytes + scale bytes."""
        return self.q.numel() + self.scale.element_size() * self.scale.numel()

    def to(self, device):
        return type(self)(self.q.to(device), self.scale.to(device), check=False)

    def __repr__(self) -> str:
        return f"{type(self).__name__}(shape={tuple(self.shape)}, device={self.device})"


class _QuantWeight(_Quant):
    """A quantized projection weight [N, K]."""

    __slots__ = ()
    _nd = 2

    def float(self) -> torch.Tensor:
        """The dequantized fp32 matrix (exact)."""
        return self.fmt.to_float(self.q, self.scale)

    def __getitem__(self, idx):
        """Row / column slices (tensor-parallel sharding): w[a:b] slices codes and scales by
        rows, w[:, a:b] by columns under the format's rule (fp8: any slice, the scales stay;
        mxfp4: a and b multiples of 32, whole scale blocks)."""
        rows, cols = idx if isinstance(idx, tuple) else (idx, slice(None))
        if not (isinstance(rows, slice) and isinstance(cols, slice)):
            raise TypeError(f"{type(self).__name__} supports slices only")
        qc, sc = self.fmt.col_slices(type(self).__name__, cols, self.shape[1])
        return type(self)(self.q[rows, qc], self.scale[(rows,) + sc], check=False)

    def hf_export(self) -> tuple:
        """(`weight`, `weight_scale`) as an HF checkpoint of this format holds them (copies)."""
        return self.fmt.export(self.q.clone(), self.scale.clone())

    @classmethod
    def cat(cls, parts: list):
        """Same-format weights concatenated along the output channels, bit for bit."""
        return cls(torch.cat([p.q for p in parts], 0), torch.cat([p.scale for p in parts], 0),
                   check=False)


class _QuantExperts(_Quant):
    """The quantized weights of a group of MoE experts, [E, N, K]: the 2-D format's ``q`` and
    ``scale`` with a leading expert dimension.  ``w[e]`` is expert e's 2-D weight, so code
    written for a bf16 [E, N, K] tensor that reads ``w[e].float()`` works unchanged."""

    __slots__ = ()
    _nd = 3

    def flat(self):
        """All experts' channels as one [E * N, K] weight (a view: the dequantizer's input)."""
        EN = self.q.shape[0] * self.q.shape[1]
        return self.fmt.Weight(self.q.view(EN, -1), self.scale.view(EN, *self.scale.shape[2:]),
                               check=False)

    def float(self) -> torch.Tensor:
        """The dequantized fp32 tensor (exact)."""
        return self.flat().float().view(self.shape)

    def __getitem__(self, idx):
        """w[e] -> expert e's 2-D weight; w[a:b] -> the experts a..b (expert parallelism);
        w[:, :, a:b] / w[:, a:b] -> column / channel slices of every expert (tensor
        parallelism; columns under the format's rule, as the 2-D weight)."""
        who = type(self).__name__
        idx = idx if isinstance(idx, tuple) else (idx,)
        if len(idx) > 3:
            raise IndexError(f"{who}: at most 3 indices")
        ex, rows, cols = tuple(idx) + (slice(None),) * (3 - len(idx))
        if not (isinstance(rows, slice) and isinstance(cols, slice)):
            raise TypeError(f"{who} supports channel and column slices only")
        qc, sc = self.fmt.col_slices(who, cols, self.shape[2])
        if isinstance(ex, int):
            cls = self.fmt.Weight
        elif isinstance(ex, slice):
            cls = type(self)
        else:
            raise TypeError(f"{who}: the expert index is an int or a slice")
        return cls(self.q[ex, rows, qc], self.scale[(ex, rows) + sc], check=False)


class Fp8Weight(_QuantWeight):
    """Per-output-channel scaled e4m3fn weight [N, K]."""
    __slots__ = ("q", "scale")


class Fp8Experts(_QuantExperts):
    """FP8 experts: ``q`` uint8 [E, N, K], ``scale`` fp32 [E, N] (csrc/kernels/moe_qgemm.hip)."""
    __slots__ = ("q", "scale")


class Mxfp4Weight(_QuantWeight):
    """MXFP4 weight [N, K]: packed e2m1 codes uint8 [N, K/2] and e8m0 block scales uint8
    [N, K/32]."""
    __slots__ = ("q", "scale")


class Mxfp4Experts(_QuantExperts):
    """MXFP4 experts: ``q`` uint8 [E, N, K/2], ``scale`` uint8 [E, N, K/32] of e8m0 codes in
    2..252 (csrc/kernels/moe_q4gemm.hip)."""
    __slots__ = ("q", "scale")


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


def _fp8_to_float(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """float(q) * scale[:, None]"""
    return q.view(torch.float8_e4m3fn).float() * scale[:, None]


def _mxfp4_to_float(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """e2m1(q) * 2^(scale - 127)"""
    lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=q.device)
    ql = q.long()
    v = torch.stack((lut[ql & 15], lut[ql >> 4]), dim=-1).reshape(q.shape[0], 2 * q.shape[1])
    s = torch.ldexp(torch.ones((), device=q.device), scale.to(torch.int32) - 127)
    return v * s.repeat_interleave(MX_BLOCK, dim=1)


FORMATS = {
    "fp8": QuantFormat(
        name="fp8", per_byte=1, block=0, scale_dtype=torch.float32, scale_codes=None,
        code_view="float8_e4m3fn", scale_view=None,
        ckpt_dtypes=_dtypes("float8_e4m3fn"), ckpt_scale_dtypes=(),
        quantize=quantize_fp8, to_float=_fp8_to_float,
        # a float8_e4m3fn view with an [N, 1] fp32 scale
        export=lambda q, s: (q.view(torch.float8_e4m3fn), s.reshape(-1, 1)),
        gemm="qgemm", dequant="dequant_fp8", moe_gemm="moe_qgemm", supported="qgemm_supported",
        dequant_k=16, q_text="uint8 / float8_e4m3fn [{n}, K]", scale_text="fp32 [{n}]"),
    "mxfp4": QuantFormat(
        name="mxfp4", per_byte=2, block=MX_BLOCK, scale_dtype=torch.uint8,
        scale_codes=(MX_SCALE_MIN, MX_SCALE_MAX),
        code_view="float4_e2m1fn_x2", scale_view="float8_e8m0fnu",
        ckpt_dtypes=_dtypes("uint8", "float4_e2m1fn_x2"),
        ckpt_scale_dtypes=_dtypes("uint8", "float8_e8m0fnu"),
        quantize=quantize_mxfp4, to_float=_mxfp4_to_float,
        export=lambda q, s: (q, s),  # uint8 codes with uint8 [N, K/32] e8m0 codes
        gemm="q4gemm", dequant="dequant_mxfp4", moe_gemm="moe_q4gemm",
        supported="q4gemm_supported", dequant_k=MX_BLOCK,
        q_text="uint8 [{n}, K/2]", scale_text="uint8 [{n}, K/32] (e8m0 codes)"),
}
for _f, _w, _e in ((FORMATS["fp8"], Fp8Weight, Fp8Experts),
                   (FORMATS["mxfp4"], Mxfp4Weight, Mxfp4Experts)):
    _f.Weight, _f.Experts = _w, _e
    _w.fmt = _e.fmt = _f

# what ops.linear / linear_silu, the loader and the byte accounting test a weight against
QuantWeight = (Fp8Weight, Mxfp4Weight)
# what ops.fused_moe, MoEBlock and the byte accounting test an expert weight against
QuantExperts = (Fp8Experts, Mxfp4Experts)


@torch.no_grad()
def quantize_experts(w: torch.Tensor, fmt: QuantFormat):
    """The format's 2-D rule per expert of w [E, N, K]."""
    if w.dim() != 3 or w.shape[2] % (fmt.block or 1):
        raise ValueError(f"quantize_{fmt.name}_experts: 3-D weight [E, N, K]"
                         + (f", K a multiple of {fmt.block}" if fmt.block else ""))
    E, N, K = w.shape
    q = torch.empty(E, N, K // fmt.per_byte, dtype=torch.uint8, device=w.device)
    scale = torch.empty(fmt.scale_shape((E, N), K), dtype=fmt.scale_dtype, device=w.device)
    for e in range(E):  # one expert's fp32 temporaries at a time
        f = fmt.quantize(w[e])
        q[e].copy_(f.q)
        scale[e].copy_(f.scale)
    return fmt.Experts(q, scale, check=False)


def quantize_fp8_experts(w): return quantize_experts(w, FORMATS["fp8"])  # noqa: E704
def quantize_mxfp4_experts(w): return quantize_experts(w, FORMATS["mxfp4"])  # noqa: E704


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
        raise RuntimeError("dequantization scratch must be reserved before graph capture")
    _scratch[device] = None  # drop the old one first
    _scratch[device] = torch.empty(numel, dtype=torch.bfloat16, device=device)


def _dequant_to_scratch(w: _QuantWeight, what: str = "weight", shape=None) -> torch.Tensor:
    """The 2-D weight w dequantized by its format's kernel into the shared scratch; `what`
    and `shape` name it in the refusal of a K the kernel does not take."""
    if w.shape[1] % w.fmt.dequant_k:
        raise ValueError(f"{w.fmt.name} {what} {tuple(shape or w.shape)}: K must be a multiple "
                         f"of {w.fmt.dequant_k}")
    reserve_scratch(w.numel(), w.device)
    out = _scratch[w.device][: w.numel()].view(w.shape)
    getattr(torch.ops.akap, w.fmt.dequant)(out, w.q, w.scale)
    return out


def dequant(w: _QuantWeight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The dequantized weight, rounded to bf16, as a new (or given) bf16 tensor; GPU: the
    format's HIP kernel."""
    if out is None:
        out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
    if w.is_cuda:
        from . import load_native

        load_native(required=True)
        getattr(torch.ops.akap, w.fmt.dequant)(out, w.q, w.scale)
    else:
        out.copy_(w.float().to(torch.bfloat16))
    return out


dequant_fp8 = dequant_mxfp4 = dequant


def dequant_experts(w: _QuantExperts) -> torch.Tensor:
    """The dequantized bf16 weights of all experts as a [E, N, K] view of the shared scratch
    (GPU: the format's dequantize kernel, bit-exact; stream-ordered like every other use of the
    scratch, never inside a captured region) or a new tensor (CPU)."""
    if not w.is_cuda:
        return w.float().to(torch.bfloat16)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{w.fmt.name} experts are not dequantized inside a captured region")
    from . import load_native

    load_native(required=True)
    return _dequant_to_scratch(w.flat(), "experts", w.shape).view(w.shape)


dequant_fp8_experts = dequant_mxfp4_experts = dequant_experts


def gemm_supported(x: torch.Tensor, w: _QuantWeight,
                   out: Optional[torch.Tensor] = None) -> bool:
    """Whether the format's decode GEMM op (qgemm / q4gemm) takes the launch: the kernel's
    shape predicate and the tensor properties ops.cpp checks (out=None: a fresh dense [M, N]
    output)."""
    N, K = w.shape
    return (x.dim() == 2 and x.dtype == torch.bfloat16 and x.stride(-1) == 1
            and x.data_ptr() % 16 == 0
            and (out is None or (out.dim() == 2 and out.stride(-1) == 1
                                 and out.data_ptr() % 16 == 0))
            and getattr(_contract(), w.fmt.supported)(
                x.shape[0], N, K, x.stride(0), N if out is None else out.stride(0)))


qgemm_supported = q4gemm_supported = gemm_supported


def linear_quant(x: torch.Tensor, w: _QuantWeight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w.T for any QuantWeight (its format's contract at the top of this file)."""
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
    if gemm_supported(x, w, out):
        if out is None:
            out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        getattr(torch.ops.akap, w.fmt.gemm)(out, x, w.q, w.scale)
        return out
    # prefill and mixed steps: dequantize into the shared scratch, then the bf16 GEMM
    return linear(x, _dequant_to_scratch(w), out=out)


linear_fp8 = linear_mxfp4 = linear_quant
