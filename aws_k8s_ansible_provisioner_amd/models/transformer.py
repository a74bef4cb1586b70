"""Decoder-only transformer (Qwen3 / Llama-3 / Mixtral) on the gfx950 kernels.

MI355X-first structure (not a module-per-op port):
  * fused weights: one QKV projection [ (Hq+2Hkv)*D, d ] and one gate|up projection
    [2F, d] per layer, so each layer is 4 large hipBLASLt GEMMs + 5 hand-written kernels
    (fused add+RMSNorm x2, QK-norm+RoPE+KV-write, paged attention, SiLU*mul);
  * the residual stream is updated in place by the fused add+norm kernel;
  * tensor parallel: QKV / gate_up column-split by heads / ffn rows, O / down row-split
    with one RCCL all-reduce each, vocab-parallel embedding + LM head;
  * everything in forward() is allocation-stable and sync-free on the decode path, so
    the engine captures it in a hipGraph per batch-size bucket.
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops
from ..ops import reference as ref
from ..ops.quant import FORMATS, Fp8Weight, Mxfp4Weight, QuantWeight, reserve_scratch
from ..parallel import comm
from ..parallel.state import ParallelState, get_state
from .config import ModelConfig
from .moe import MoEBlock

FUSED_DECODE = os.environ.get("AKAP_FUSED_DECODE", "1") != "0"
PREFETCH_WEIGHTS = os.environ.get("AKAP_PREFETCH_WEIGHTS", "0") == "1"
FUSED_GEMM = os.environ.get("AKAP_FUSED_GEMM", "1") != "0"
# prefill attention applies the q norm + RoPE itself from the QKV rows (AKAP_PREFILL_QPREP=0:
# the standalone pass writes every q row, the kernel reads q)
PREFILL_QPREP = os.environ.get("AKAP_PREFILL_QPREP", "1") != "0"
# fused decode chain: the new token's K/V rows are written by rider workgroups of the gate|up
# GEMM launch instead of by the attention kernel, when that launch has resident room for them
# (ops.kv_rider_blocks; AKAP_DECODE_KV_RIDER=0: always by the attention kernel)
DECODE_KV_RIDER = os.environ.get("AKAP_DECODE_KV_RIDER", "1") != "0"


@dataclasses.dataclass
class AttnBatch:
    """Flattened batch description consumed by the attention kernels."""
    is_prefill: bool
    positions: torch.Tensor      # [T] int64
    slots: torch.Tensor          # [T] int64 (-1 = padding)
    block_tables: torch.Tensor   # [B, max_blocks] int32
    seq_lens: torch.Tensor       # [B] int32
    q_start: torch.Tensor        # [B+1] int32
    tile_seq: Optional[torch.Tensor] = None  # prefill tile map
    tile_row: Optional[torch.Tensor] = None
    num_parts: int = 1           # decode split-KV partitions
    part_size: int = 512
    workspace: Optional[tuple] = None
    tile_rows: int = 64          # q rows per prefill tile of the map (128: flash-style kernel)
    num_decode: int = 0          # mixed step: leading single-token decode rows [0, num_decode)
    # V tail (GPU, bf16 cache): per-layer [slots, Hkv, 8, D] partial-group buffers and the
    # per-token (= per decode row) tail slot; None = the plain V cache write path
    v_tails: Optional[list] = None
    tail_slot: Optional[torch.Tensor] = None


@dataclasses.dataclass
class LayerWeights:
    ln1: torch.Tensor
    ln2: torch.Tensor
    w_qkv: torch.Tensor
    w_o: torch.Tensor
    q_norm: Optional[torch.Tensor]
    k_norm: Optional[torch.Tensor]
    w_gate_up: Optional[torch.Tensor]
    w_down: Optional[torch.Tensor]
    moe: Optional[MoEBlock] = None


def _shard_rows(w, rank: int, size: int):
    n = w.shape[0] // size
    return w[rank * n:(rank + 1) * n]


def _shard_cols(w, rank: int, size: int):
    n = w.shape[1] // size
    return w[:, rank * n:(rank + 1) * n]


PROJECTIONS = ("w_qkv", "w_o", "w_gate_up", "w_down")
QUANTIZATIONS = (None, "fp8", "mxfp4")
EXPERT_QUANTIZATIONS = (None, "fp8", "mxfp4")  # MoE expert weights only (ops.quant.QuantExperts)
_FP8_BLOCK = 128  # block-scaled checkpoints: one weight_scale_inv per 128 x 128 block


def _scale_kind(t: torch.Tensor) -> str:
    """Which quantization a checkpoint's `weight_scale` tensor belongs to: e8m0 codes (uint8)
    are MXFP4 block scales, anything else an FP8 scale."""
    return "mxfp4" if t.dtype in FORMATS["mxfp4"].ckpt_scale_dtypes else "fp8"


def _checkpoint_proj(sd: dict, key: str, quantization: Optional[str]):
    """The projection `key`.weight of a checkpoint: a plain tensor, an Mxfp4Weight for packed
    e2m1 codes (uint8 [N, K/2]) with e8m0 `weight_scale` codes (uint8 [N, K/32]), or an Fp8Weight
    for a
    pre-quantized float8_e4m3fn weight with a per-channel ([N, 1] / [N]) or per-tensor (scalar,
    expanded) `weight_scale`.  A block-scaled weight (`weight_scale_inv`, 128 x 128 blocks) is
    dequantized to fp32 here and re-quantized per channel by the caller.  `input_scale`
    (activation scales of W8A8 checkpoints) is not used: activations stay bf16."""
    w = sd[key + ".weight"]
    if w.dtype in FORMATS["mxfp4"].ckpt_dtypes:
        if quantization != "mxfp4":
            raise ValueError(f"{key}.weight holds packed 4-bit codes: this is an MXFP4 "
                             f"checkpoint, load it with --quantization mxfp4")
        if key + ".weight_scale" not in sd:
            raise ValueError(f"{key}.weight is MXFP4 but the checkpoint has no "
                             f"{key}.weight_scale")
        return Mxfp4Weight(w, sd[key + ".weight_scale"])  # refuses e8m0 codes outside 2..252
    if w.dtype not in FORMATS["fp8"].ckpt_dtypes:
        return w
    if quantization != "fp8":
        raise ValueError(f"{key}.weight is float8_e4m3fn: this is an FP8 checkpoint, load it "
                         f"with --quantization fp8")
    N, K = w.shape
    if key + ".weight_scale_inv" in sd:
        s = sd[key + ".weight_scale_inv"].float()
        s = s.repeat_interleave(_FP8_BLOCK, 0)[:N].repeat_interleave(_FP8_BLOCK, 1)[:, :K]
        return w.float() * s
    if key + ".weight_scale" not in sd:
        raise ValueError(f"{key}.weight is float8_e4m3fn but the checkpoint has no "
                         f"{key}.weight_scale")
    s = sd[key + ".weight_scale"].float().reshape(-1)
    if s.numel() == 1:
        s = s.expand(N)
    elif s.numel() != N:
        raise ValueError(f"{key}.weight_scale has {s.numel()} values for {N} output channels")
    return Fp8Weight(w.view(torch.uint8), s.contiguous())


def _fuse_rows(parts: list):
    """Concatenate projections along the output channels: bit-exact for pre-quantized parts
    (codes and per-channel scales are concatenated), fp32 otherwise."""
    if isinstance(parts[0], QuantWeight) and all(type(p) is type(parts[0]) for p in parts):
        return type(parts[0]).cat(parts)
    if any(isinstance(p, QuantWeight) or p.dtype == torch.float32 for p in parts):
        return torch.cat([p.float() for p in parts], 0)
    return torch.cat(parts, 0)


def ipc_safe_alloc_bytes(nbytes: int) -> int:
    """Bytes to allocate for an `nbytes` buffer that a peer process will hipIpc-open: the
    caching allocator's 2 MiB rounding, then, if bit 31 of the size is set (size mod 4 GiB >=
    2 GiB -- hipIpcOpenMemHandle of such an allocation hangs on the ROCm 7.0.2 runtime that
    PyTorch bundles), the next multiple of 4 GiB."""
    r = -(-int(nbytes) // (2 << 20)) * (2 << 20)
    if r & (1 << 31):
        r = ((r >> 32) + 1) << 32
    return r


def kv_segment_layers(L: int, per_layer: int, max_segment_bytes: int,
                      ipc_safe: bool = True) -> int:
    """Layers per KV segment: as many as fit `max_segment_bytes`; with ipc_safe, the count in
    [max/2, max] whose segments need the fewest ipc_safe_alloc_bytes padding bytes (ties: the
    fewest segments)."""
    lps_max = max(1, min(L, max_segment_bytes // max(1, per_layer)))
    if not ipc_safe:
        return lps_max

    def pad_total(lps: int) -> int:
        return sum(ipc_safe_alloc_bytes(min(lps, L - l0) * per_layer) -
                   min(lps, L - l0) * per_layer for l0 in range(0, L, lps))

    return min(range(lps_max, lps_max // 2, -1), key=pad_total)


class DecoderLM:
    """Weights + forward for one tensor-parallel rank."""

    def __init__(self, cfg: ModelConfig, device: torch.device | str = "cpu",
                 dtype: torch.dtype = torch.bfloat16, seed: int = 0,
                 pstate: Optional[ParallelState] = None, max_model_len: int = 4096,
                 full_then_shard: bool = False, init_std: float = 0.02,
                 quantization: Optional[str] = None,
                 expert_quantization: Optional[str] = None):
        if quantization == "none":
            quantization = None
        if quantization not in QUANTIZATIONS:
            raise ValueError(f"unknown quantization {quantization!r} (none | fp8 | mxfp4)")
        if quantization is not None and cfg.is_moe:
            raise ValueError(f"{cfg.name}: {quantization} weight quantization covers dense models only "
                             f"(MoE experts are not quantized by --quantization; see "
                             f"--expert-quantization)")
        if expert_quantization == "none":
            expert_quantization = None
        if expert_quantization not in EXPERT_QUANTIZATIONS:
            raise ValueError(f"unknown expert quantization {expert_quantization!r} "
                             f"(none | fp8 | mxfp4)")
        if expert_quantization is not None and not cfg.is_moe:
            raise ValueError(f"{cfg.name}: expert quantization set on a dense model (no experts); "
                             f"use --quantization")
        # "fp8" / "mxfp4": load_state_dict loads the experts as Fp8Experts / Mxfp4Experts
        # (pre-quantized kept bit for bit, plain ones quantized); a model built from random
        # weights is quantized by quantize_experts_fp8 / quantize_mxfp4_experts.  Everything but
        # the experts stays bf16.
        self.expert_quantization = expert_quantization
        self.experts_quantized = False  # the MoE blocks hold Fp8Experts or Mxfp4Experts
        # "fp8" / "mxfp4": load_state_dict accepts checkpoints of that kind and quantizes plain
        # ones; a model built from random weights is quantized by quantize_fp8 / quantize_mxfp4
        self.quantization = quantization
        self.quantized = False  # some layer projection is a QuantWeight
        self.cfg = cfg
        self.init_std = init_std
        self.device = torch.device(device)
        self.dtype = dtype
        self.ps = pstate or get_state()
        tp, r = self.ps.tp_size, self.ps.tp_rank
        if cfg.num_heads % tp:
            raise ValueError("num_heads must divide by tp")
        self.hq = cfg.num_heads // tp
        self.hkv = max(1, cfg.num_kv_heads // tp)
        self.kv_replicas = max(1, tp // cfg.num_kv_heads)
        self.D = cfg.head_dim
        self.ffn = cfg.intermediate_size // tp
        self.vocab_per = math.ceil(cfg.vocab_size / tp)
        self.vocab_start = r * self.vocab_per
        self.vocab_end = min(cfg.vocab_size, self.vocab_start + self.vocab_per)
        self.scale = 1.0 / math.sqrt(self.D)
        if max_model_len > cfg.max_position:
            # the rotary table (and the kernels that index it by position) end there
            raise ValueError(f"max_model_len {max_model_len} exceeds {cfg.name}'s "
                             f"max_position_embeddings {cfg.max_position}")
        self._init_weights(seed, full_then_shard)
        self.cos_sin = ref.rope_cos_sin(min(cfg.max_position, max(max_model_len, 16)), self.D,
                                        cfg.rope_theta, cfg.rope_scaling, device=self.device)

    # ------------------------------------------------------------------ weights
    def _rand(self, g: torch.Generator, *shape, std: Optional[float] = None) -> torch.Tensor:
        t = torch.empty(*shape, dtype=torch.float32, device=g.device)
        t.normal_(0.0, self.init_std if std is None else std, generator=g)
        return t.to(self.dtype)

    def _init_weights(self, seed: int, full_then_shard: bool) -> None:
        cfg, tp, r = self.cfg, self.ps.tp_size, self.ps.tp_rank
        d, D = cfg.hidden_size, self.D
        gdev = self.device if self.device.type == "cuda" else torch.device("cpu")
        # Full-then-shard (tests): identical logical weights for any tp.  Otherwise each
        # rank draws only its shard (70B at TP=8 never materialises the full model).
        g = torch.Generator(device=gdev)
        g.manual_seed(seed if full_then_shard else seed * 1000 + r)
        to = dict(device=self.device)
        one = lambda n: torch.ones(n, dtype=self.dtype, **to)  # noqa: E731

        vp = self.vocab_per
        if full_then_shard:
            emb_full = self._rand(g, vp * tp, d)
            emb_full[cfg.vocab_size:] = 0
            self.embed = emb_full[r * vp:(r + 1) * vp].contiguous().to(**to)
        else:
            self.embed = self._rand(g, vp, d).to(**to)
            self.embed[self.vocab_end - self.vocab_start:] = 0
        self.layers: list[LayerWeights] = []
        for _ in range(cfg.num_layers):
            if full_then_shard:
                wq = self._rand(g, cfg.q_size, d)
                wk = self._rand(g, cfg.kv_size, d)
                wv = self._rand(g, cfg.kv_size, d)
                wo = self._rand(g, d, cfg.q_size)
                q_sh = _shard_rows(wq, r, tp)
                k0, k1 = self._kv_head_range()
                k_sh, v_sh = wk[k0 * D:k1 * D], wv[k0 * D:k1 * D]
                w_qkv = torch.cat([q_sh, k_sh, v_sh], 0).contiguous().to(**to)
                w_o = _shard_cols(wo, r, tp).contiguous().to(**to)
            else:
                w_qkv = self._rand(g, (self.hq + 2 * self.hkv) * D, d).to(**to)
                w_o = self._rand(g, d, self.hq * D).to(**to)
            qn = one(D) if cfg.qk_norm else None
            kn = one(D) if cfg.qk_norm else None
            if cfg.is_moe:
                moe = MoEBlock(cfg, self.ps, self.device, self.dtype, g, full_then_shard,
                               std=self.init_std)
                lw = LayerWeights(one(d), one(d), w_qkv, w_o, qn, kn, None, None, moe)
            else:
                if full_then_shard:
                    wg = self._rand(g, cfg.intermediate_size, d)
                    wu = self._rand(g, cfg.intermediate_size, d)
                    wd = self._rand(g, d, cfg.intermediate_size)
                    w_gu = torch.cat([_shard_rows(wg, r, tp), _shard_rows(wu, r, tp)], 0).contiguous().to(**to)
                    w_d = _shard_cols(wd, r, tp).contiguous().to(**to)
                else:
                    w_gu = self._rand(g, 2 * self.ffn, d).to(**to)
                    w_d = self._rand(g, d, self.ffn).to(**to)
                lw = LayerWeights(one(d), one(d), w_qkv, w_o, qn, kn, w_gu, w_d)
            self.layers.append(lw)
        self.final_norm = one(d)
        if cfg.tie_embeddings:
            self.lm_head = self.embed
        elif full_then_shard:
            lm = self._rand(g, vp * tp, d)
            lm[cfg.vocab_size:] = 0
            self.lm_head = lm[r * vp:(r + 1) * vp].contiguous().to(**to)
        else:
            self.lm_head = self._rand(g, vp, d).to(**to)
            self.lm_head[self.vocab_end - self.vocab_start:] = 0

    def _kv_head_range(self) -> tuple[int, int]:
        """kv heads owned by this TP rank (replicated when tp > num_kv_heads)."""
        tp, r, H = self.ps.tp_size, self.ps.tp_rank, self.cfg.num_kv_heads
        if H >= tp:
            return r * H // tp, (r + 1) * H // tp
        h = r // (tp // H)
        return h, h + 1

    @property
    def graph_safe(self) -> bool:
        """Decode step free of host syncs (capturable in a hipGraph)."""
        return all(l.moe is None or l.moe.graph_safe for l in self.layers)

    def weight_bytes(self, as_bf16: bool = False) -> int:
        """bf16 tensors at 2 bytes per element; a quantized projection [N, K] counts
        N * K + 4 * N (fp8 codes + fp32 scales) or N * K / 2 + N * K / 32 (MXFP4 codes + block
        scales), or what it would take in bf16 with as_bf16."""
        n = self.embed.numel() + self.final_norm.numel()
        q = 0
        if self.lm_head is not self.embed:
            n += self.lm_head.numel()
        for lw in self.layers:
            for t in (lw.ln1, lw.ln2, lw.w_qkv, lw.w_o, lw.q_norm, lw.k_norm, lw.w_gate_up,
                      lw.w_down):
                if isinstance(t, QuantWeight):
                    q += 2 * t.numel() if as_bf16 else t.nbytes
                elif t is not None:
                    n += t.numel()
            # quantized experts [E, N, K]: E N K + 4 E N (fp8) or E N K / 2 + E N K / 32 (mxfp4)
            if lw.moe is not None:
                q += lw.moe.weight_bytes(as_bf16)
        return n * 2 + q

    @torch.no_grad()
    def quantize_experts_fp8(self) -> None:
        """Replace every MoE layer's expert weights by per-(expert, channel) e4m3fn Fp8Experts,
        one tensor at a time.  Router, attention projections, embedding, LM head and norms stay
        bf16 (`quantized` stays false: the dense-layer logic is untouched).  Also reserves the
        dequantization scratch the prefill path uses, sized to the largest expert tensor
        (E_local * 2F * d elements)."""
        self._quantize_experts(FORMATS["fp8"])

    @torch.no_grad()
    def quantize_mxfp4_experts(self) -> None:
        """The same for MXFP4: every MoE layer's expert weights become Mxfp4Experts (e2m1 codes
        with one e8m0 scale per 32 elements along K), on each rank's local experts or F shard,
        which must be a multiple of 128 (MoEBlock.check_mxfp4_shapes).  The scratch is the same
        size: it holds the dequantized bf16 tensor."""
        self._quantize_experts(FORMATS["mxfp4"])

    def _quantize_experts(self, fmt) -> None:
        if not self.cfg.is_moe:
            raise ValueError(f"{self.cfg.name}: a dense model has no experts to quantize")
        largest = 0
        for lw in self.layers:
            if lw.moe is not None:
                lw.moe.quantize(fmt)
                largest = max(largest, lw.moe.w13.numel(), lw.moe.w2.numel())
        self.expert_quantization = fmt.name
        self.experts_quantized = True
        reserve_scratch(largest, self.device)

    @torch.no_grad()
    def quantize_fp8(self) -> None:
        """Replace every dense layer's projections by per-channel e4m3fn Fp8Weights, one layer
        at a time, dropping each bf16 tensor as it goes.  Embedding, LM head and norms stay
        bf16, as in published FP8 checkpoints.  Also reserves the dequantization scratch the
        prefill path uses (ops.quant), sized to the largest quantized weight."""
        self._quantize("fp8")

    @torch.no_grad()
    def quantize_mxfp4(self) -> None:
        """The same for MXFP4: e2m1 codes with one e8m0 scale per 32 elements along K
        (Mxfp4Weight), after the bf16 weights are resident."""
        self._quantize("mxfp4")

    def _quantize(self, kind: str) -> None:
        if any(lw.moe is not None for lw in self.layers):
            raise ValueError(f"{self.cfg.name}: {kind} weight quantization covers dense models "
                             f"only (MoE experts are not quantized by it; see "
                             f"quantize_experts_fp8 / quantize_mxfp4_experts / "
                             f"--expert-quantization)")
        largest = 0
        for lw in self.layers:
            for name in PROJECTIONS:
                w = getattr(lw, name)
                if not isinstance(w, QuantWeight):
                    setattr(lw, name, None)
                    w = FORMATS[kind].quantize(w)
                    setattr(lw, name, w)
                largest = max(largest, w.numel())
        self.quantization = kind
        self.quantized = True
        reserve_scratch(largest, self.device)

    def hf_state_dict(self) -> dict:
        """This (unsharded, tp=1) model's weights under HF names, un-fusing QKV and gate|up
        and the Mixtral experts -- the inverse of load_state_dict (checkpoint export and the
        loader's round-trip tests)."""
        if self.ps.tp_size != 1:
            raise ValueError("hf_state_dict needs the unsharded (tp=1) model")
        cfg, D = self.cfg, self.D
        n = self.vocab_end - self.vocab_start
        sd = {"model.embed_tokens.weight": self.embed[:n].clone(),
              "model.norm.weight": self.final_norm.clone()}
        if not cfg.tie_embeddings:
            sd["lm_head.weight"] = self.lm_head[:n].clone()
        q, kv = self.hq * D, self.hkv * D

        def put(key: str, w, a: int = 0, b: Optional[int] = None) -> None:
            # rows [a, b) of a projection; quantized: its format's checkpoint form
            # (QuantFormat.export)
            if isinstance(w, QuantWeight):
                sd[key + ".weight"], sd[key + ".weight_scale"] = w[a:b].hf_export()
            else:
                sd[key + ".weight"] = w[a:b].clone()

        for i, lw in enumerate(self.layers):
            p = f"model.layers.{i}."
            sd[p + "input_layernorm.weight"] = lw.ln1.clone()
            sd[p + "post_attention_layernorm.weight"] = lw.ln2.clone()
            put(p + "self_attn.q_proj", lw.w_qkv, 0, q)
            put(p + "self_attn.k_proj", lw.w_qkv, q, q + kv)
            put(p + "self_attn.v_proj", lw.w_qkv, q + kv)
            put(p + "self_attn.o_proj", lw.w_o)
            if lw.q_norm is not None:
                sd[p + "self_attn.q_norm.weight"] = lw.q_norm.clone()
                sd[p + "self_attn.k_norm.weight"] = lw.k_norm.clone()
            if lw.moe is not None:
                sd.update(lw.moe.hf_state_dict(p))
            else:
                F_ = lw.w_gate_up.shape[0] // 2
                put(p + "mlp.gate_proj", lw.w_gate_up, 0, F_)
                put(p + "mlp.up_proj", lw.w_gate_up, F_)
                put(p + "mlp.down_proj", lw.w_down)
        return sd

    def _set_proj(self, lw: LayerWeights, name: str, src) -> None:
        """Store one (fused, sharded) projection.  bf16 model: copy into the existing tensor.
        Quantized model: a pre-quantized source is kept bit for bit (no bf16 detour); any other
        source is quantized from its own precision."""
        cur = getattr(lw, name)
        if tuple(src.shape) != tuple(cur.shape):
            raise ValueError(f"{name}: checkpoint shape {tuple(src.shape)} != model "
                             f"{tuple(cur.shape)}")
        if self.quantization is None:
            cur.copy_(src.to(cur.dtype))
            return
        setattr(lw, name, None)  # drop the old weight before the new one is resident
        if not isinstance(src, QuantWeight):
            src = FORMATS[self.quantization].quantize(src.to(self.device))
        setattr(lw, name, src.to(self.device))
        self.quantized = True
        reserve_scratch(src.numel(), self.device)

    def load_state_dict(self, sd: dict) -> None:
        """Load HF-named tensors (safetensors from the model PVC) into the fused layout.
        With quantization "fp8" the projections may be plain (quantized here), pre-quantized
        float8_e4m3fn + `weight_scale`, or block-scaled (`weight_scale_inv`); with "mxfp4",
        plain or pre-quantized uint8 [N, K/2] + uint8 `weight_scale` [N, K/32]."""
        cfg, tp, r = self.cfg, self.ps.tp_size, self.ps.tp_rank
        eq = self.expert_quantization
        for k in sd:
            if k.endswith((".weight_scale", ".weight_scale_inv")):
                kind = _scale_kind(sd[k])
                if eq is not None and ".experts." in k:
                    # expert tensors are judged against the expert knob
                    if kind != eq:
                        raise ValueError(f"checkpoint key {k}: these are {kind.upper()} experts, "
                                         f"load them with --expert-quantization {kind}")
                elif eq is not None and kind == "fp8":
                    pass  # an fp8 attention projection next to quantized experts: dequantized below
                elif kind != self.quantization:
                    raise ValueError(f"checkpoint key {k}: this is an {kind.upper()} checkpoint, "
                                     f"load it with --quantization {kind}")
        proj = lambda key: _checkpoint_proj(sd, key, self.quantization)  # noqa: E731
        if eq is not None:
            # only the experts are quantized: a pre-quantized attention projection becomes bf16
            noted = []

            def proj(key):  # noqa: F811
                fp8 = sd[key + ".weight"].dtype == torch.float8_e4m3fn
                w = _checkpoint_proj(sd, key, "fp8" if fp8 else eq)
                if isinstance(w, Fp8Weight):
                    if not noted:
                        noted.append(key)
                        print(f"[weights] {cfg.name}: fp8 attention projections ({key}, ...) are "
                              f"dequantized to bf16 at load: only the experts are quantized",
                              flush=True)
                    w = w.float()
                return w
        eproj = None if eq is None else (lambda key: _checkpoint_proj(sd, key, eq))
        cp = lambda dst, src: dst.copy_(src.to(dst.dtype))  # noqa: E731
        emb = sd["model.embed_tokens.weight"]
        n = self.vocab_end - self.vocab_start
        cp(self.embed[:n], emb[self.vocab_start:self.vocab_end])
        for i, lw in enumerate(self.layers):
            p = f"model.layers.{i}."
            cp(lw.ln1, sd[p + "input_layernorm.weight"])
            cp(lw.ln2, sd[p + "post_attention_layernorm.weight"])
            q = _shard_rows(proj(p + "self_attn.q_proj"), r, tp)
            k0, k1 = self._kv_head_range()
            D = self.D
            k = proj(p + "self_attn.k_proj")[k0 * D:k1 * D]
            v = proj(p + "self_attn.v_proj")[k0 * D:k1 * D]
            self._set_proj(lw, "w_qkv", _fuse_rows([q, k, v]))
            self._set_proj(lw, "w_o", _shard_cols(proj(p + "self_attn.o_proj"), r, tp))
            if lw.q_norm is not None:
                cp(lw.q_norm, sd[p + "self_attn.q_norm.weight"])
                cp(lw.k_norm, sd[p + "self_attn.k_norm.weight"])
            if lw.moe is not None:
                lw.moe.load_state_dict(sd, p, proj=eproj, fmt=FORMATS.get(eq))
                if eproj is not None:
                    self.experts_quantized = True
                    reserve_scratch(max(lw.moe.w13.numel(), lw.moe.w2.numel()), self.device)
            else:
                g_ = _shard_rows(proj(p + "mlp.gate_proj"), r, tp)
                u_ = _shard_rows(proj(p + "mlp.up_proj"), r, tp)
                self._set_proj(lw, "w_gate_up", _fuse_rows([g_, u_]))
                self._set_proj(lw, "w_down", _shard_cols(proj(p + "mlp.down_proj"), r, tp))
        cp(self.final_norm, sd["model.norm.weight"])
        if not cfg.tie_embeddings:
            cp(self.lm_head[:n], sd["lm_head.weight"][self.vocab_start:self.vocab_end])

    # ------------------------------------------------------------------ kv cache
    def allocate_kv_cache(self, num_blocks: int, block_size: int,
                          kv_dtype: str = "auto") -> torch.Tensor:
        """The whole cache as ONE allocation [L, 2, NB, Hkv*BS*D] (micro-benchmarks, tests)."""
        return self.allocate_kv_segments(num_blocks, block_size, kv_dtype,
                                         max_segment_bytes=1 << 62)[0]

    def allocate_kv_segments(self, num_blocks: int, block_size: int, kv_dtype: str = "auto",
                             max_segment_bytes: Optional[int] = None) -> list:
        """Layer-range segments [Ls, 2, NB, Hkv*BS*D] (K block = [Hkv,BS,D], V block =
        [Hkv,BS/8,D,8]) of at most `max_segment_bytes` each (AKAP_KV_SEGMENT_GIB, default 32),
        zero-filled so never-written slots read as finite zeros.  kv_dtype "fp8": uint8
        storage of OCP e4m3fn values (half the bytes of bf16).  Each segment is its own
        allocation, exported by hipIpc on its own (P/D pull).

        On the GPU every allocation's size is kept hipIpc-safe (`ipc_safe_alloc_bytes`): the
        HIP runtime PyTorch bundles (ROCm 7.0.2) hangs in hipIpcOpenMemHandle when bit 31 of
        the allocation size is set (size mod 4 GiB >= 2 GiB; 1.5 / 5 / 8 / 9.5 / 36 GiB map,
        2 / 2.5 / 6.6 GiB hang, at any occupancy -- bench/ipc_import_repro.cpp,
        profiles/r6_ipc_import_sweep.md; ROCm 7.2's runtime maps them all).  That was the
        round-4/5 "hang once the device is mostly allocated": big caches made such sizes.
        The layers per segment are chosen to avoid padding where possible; otherwise the
        allocation is padded to the next 4 GiB multiple (the tail is never addressed)."""
        per_block = self.hkv * block_size * self.D
        dt = torch.uint8 if kv_dtype.startswith("fp8") else self.dtype
        if max_segment_bytes is None:
            max_segment_bytes = int(float(os.environ.get("AKAP_KV_SEGMENT_GIB", "32")) * 2**30)
        L = self.cfg.num_layers
        es = torch.empty(0, dtype=dt).element_size()
        per_layer = 2 * num_blocks * per_block * es
        gpu = torch.device(self.device).type == "cuda"
        lps = kv_segment_layers(L, per_layer, max_segment_bytes, ipc_safe=gpu)
        segs = []
        for l0 in range(0, L, lps):
            n = min(lps, L - l0)
            elems = n * 2 * num_blocks * per_block
            alloc = ipc_safe_alloc_bytes(elems * es) // es if gpu else elems
            buf = torch.zeros(alloc, dtype=dt, device=self.device)
            segs.append(buf[:elems].view(n, 2, num_blocks, per_block))
        return segs

    def cache_views(self, kv, block_size: int):
        """Per-layer K / V views of the cache (one tensor or its list of layer segments)."""
        segs = list(kv) if isinstance(kv, (list, tuple)) else [kv]
        ks, vs = [], []
        for seg in segs:
            NB = seg.shape[2]
            ks += [seg[l, 0].view(NB, self.hkv, block_size, self.D) for l in range(seg.shape[0])]
            vs += [seg[l, 1].view(NB, self.hkv, block_size // ops.KV_GROUP, self.D, ops.KV_GROUP)
                   for l in range(seg.shape[0])]
        return ks, vs

    # ------------------------------------------------------------------ forward
    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        x = ops.embedding(ids, self.embed, vocab_start=self.vocab_start, vocab_end=self.vocab_end)
        return comm.tp_all_reduce(x)

    def _attention(self, q, batch: AttnBatch, kc, vc, out, vt=None, qprep=None):
        if batch.is_prefill:
            nd = batch.num_decode
            if nd and q.is_cuda:
                # mixed step: the decode rows lead the batch and run the split-KV decode
                # kernel; the prefill tile map covers only the prefill rows after them
                # (on CPU the reference attention handles every row at once)
                ops.paged_attention_decode(out[:nd], q[:nd], kc, vc, batch.block_tables[:nd],
                                           batch.seq_lens[:nd], self.hq // self.hkv,
                                           self.scale, workspace=batch.workspace,
                                           num_parts=batch.num_parts,
                                           part_size=batch.part_size, v_tail=vt,
                                           tail_slot=batch.tail_slot)
            ops.paged_attention_prefill(out, q, kc, vc, batch.block_tables, batch.seq_lens,
                                        batch.q_start, batch.tile_seq, batch.tile_row,
                                        self.hq // self.hkv, self.scale,
                                        tile_rows=batch.tile_rows, qprep=qprep)
        else:
            ops.paged_attention_decode(out, q, kc, vc, batch.block_tables, batch.seq_lens,
                                       self.hq // self.hkv, self.scale, workspace=batch.workspace,
                                       num_parts=batch.num_parts, part_size=batch.part_size,
                                       v_tail=vt, tail_slot=batch.tail_slot)
        return out

    def forward(self, input_ids: torch.Tensor, batch: AttnBatch, k_caches, v_caches
                ) -> torch.Tensor:
        cfg = self.cfg
        T = input_ids.shape[0]
        eps = cfg.rms_eps
        # (the fused dgemm chain is bf16-only: a quantized model takes the unfused path below)
        if (not batch.is_prefill and FUSED_DECODE and FUSED_GEMM and self.device.type == "cuda"
                and not self.quantized and all(l.moe is None for l in self.layers)):
            from ..ops import gemm_tuner

            plan = gemm_tuner.fused_plan(T)
            if plan is not None:
                return self._forward_fused_decode(input_ids, batch, k_caches, v_caches, plan)
        x = self.embed_tokens(input_ids)
        residual = x
        h = ops.rms_norm(x, self.layers[0].ln1, eps)
        x = None
        for li, lw in enumerate(self.layers):
            if li > 0:
                h, residual = ops.fused_add_rms_norm(x, residual, lw.ln1, eps)
            qkv = ops.linear(h, lw.w_qkv)
            attn = torch.empty(T, self.hq, self.D, dtype=self.dtype, device=self.device)
            if not batch.is_prefill and PREFETCH_WEIGHTS and not self.quantized:
                # warm this layer's remaining GEMM weights (+ the next QKV) in MALL before
                # the HBM-bound attention stream; the latency-bound GEMMs then hit cache
                nxt = self.layers[li + 1].w_qkv if li + 1 < len(self.layers) else None
                ops.l2_prefetch([lw.w_o, lw.w_gate_up, lw.w_down, nxt])
            vt = batch.v_tails[li] if batch.v_tails is not None else None
            if not batch.is_prefill and FUSED_DECODE:
                # q/k-norm + RoPE + KV-cache write fused into the decode attention kernel
                ops.paged_attention_decode_fused(
                    attn, qkv, k_caches[li], v_caches[li], batch.block_tables, batch.seq_lens,
                    batch.positions, batch.slots, self.cos_sin, lw.q_norm, lw.k_norm,
                    self.hq // self.hkv, self.scale, eps, workspace=batch.workspace,
                    num_parts=batch.num_parts, part_size=batch.part_size, v_tail=vt,
                    tail_slot=batch.tail_slot)
            else:
                q = torch.empty_like(attn)
                # prefill on the GPU: the attention kernel norms + rotates its own q rows from
                # the QKV projection, so the standalone pass writes q only for the decode rows
                qp = batch.is_prefill and PREFILL_QPREP and qkv.is_cuda
                ops.qk_norm_rope_cache(qkv, q, k_caches[li], v_caches[li], batch.positions,
                                       batch.slots, self.cos_sin, lw.q_norm, lw.k_norm, self.hq,
                                       self.hkv, eps, True, decode=not batch.is_prefill,
                                       v_tail=vt, tail_slot=batch.tail_slot,
                                       num_decode=batch.num_decode if batch.is_prefill else 0,
                                       q_rows=batch.num_decode if qp else -1)
                self._attention(q, batch, k_caches[li], v_caches[li], attn, vt,
                                qprep=(qkv, batch.positions, self.cos_sin, lw.q_norm, eps)
                                if qp else None)
            o = comm.tp_all_reduce(ops.linear(attn.view(T, self.hq * self.D), lw.w_o))
            h, residual = ops.fused_add_rms_norm(o, residual, lw.ln2, eps)
            if lw.moe is not None:
                x = lw.moe.forward(h)
            else:
                x = comm.tp_all_reduce(ops.linear(ops.linear_silu(h, lw.w_gate_up), lw.w_down))
        h, _ = ops.fused_add_rms_norm(x, residual, self.final_norm, eps)
        return h

    def _forward_fused_decode(self, input_ids, batch: AttnBatch, k_caches, v_caches, plan: dict
                              ) -> torch.Tensor:
        """Dense decode step as 4 fused GEMM launches + 1 attention launch per layer
        (csrc/kernels/dgemm.hip): the residual add and the elementwise half of the next
        RMSNorm run in the O / down projections' epilogues (which also accumulate the
        per-row sum of squares), the norm's row scale in the consumer GEMM's epilogue, and
        SwiGLU in the gate|up projection's epilogue -- no separate norm / activation kernels.
        Tensor parallel: the row-parallel O / down projections store their partial sums and
        the residual epilogue moves into the all-reduce (comm.tp_all_reduce_resnorm: the
        custom xGMI kernel applies it in its store pass), so a TP layer is still 4 GEMM
        launches + 2 all-reduce launches + attention.  Plan from gemm_tuner.fused_plan:
        projection -> the ops.gemm_variant.Variant its GEMM runs (or that record's fields as
        a sequence, trailing ones defaulted)."""
        T = input_ids.shape[0]
        eps = self.cfg.rms_eps
        L = len(self.layers)
        tp = self.ps.tp_size
        if tp == 1:
            # one launch (ops.embedding_prep): the embedding rows, the first layer's
            # un-normalised input and its row sums of squares (the first projection applies
            # the rsqrt, like every later one), and the zeroed per-layer accumulators
            ssb = torch.empty(2 * L + 1, T, dtype=torch.float32, device=self.device)
            ss, ss_in = ssb[:2 * L], ssb[2 * L]
            residual = torch.empty(T, self.cfg.hidden_size, dtype=self.dtype, device=self.device)
            a1 = torch.empty_like(residual)
            ops.embedding_prep(input_ids, self.embed, self.layers[0].ln1, residual, a1, ss_in,
                               ss, self.vocab_start, self.vocab_end)
        else:
            residual = self.embed_tokens(input_ids)
            ss = torch.zeros(2 * L, T, dtype=torch.float32, device=self.device)
            a1 = ops.rms_norm(residual, self.layers[0].ln1, eps)
            ss_in = None
        # K/V riders: bf16 cache with a V tail, tp = 1 (this path is dense and unquantized), and
        # the planned gate|up variant has resident room behind its tiles
        rider = (DECODE_KV_RIDER and tp == 1 and batch.v_tails is not None
                 and batch.tail_slot is not None and k_caches[0].dtype == torch.bfloat16
                 and ops.kv_rider_blocks(T, self.layers[0].w_gate_up.shape[0],
                                         plan["w_gate_up"], T, self.hkv) > 0)
        for li, lw in enumerate(self.layers):
            nxt = self.layers[li + 1].w_qkv if li + 1 < L else None
            qkv = ops.dgemm(a1, lw.w_qkv, eps=eps, ss_in=ss_in, variant=plan["w_qkv"])
            attn = torch.empty(T, self.hq, self.D, dtype=self.dtype, device=self.device)
            if PREFETCH_WEIGHTS:  # A/B knob: warm the layer's remaining weights in MALL
                ops.l2_prefetch([lw.w_o, lw.w_gate_up, lw.w_down, nxt])
            ops.paged_attention_decode_fused(
                attn, qkv, k_caches[li], v_caches[li], batch.block_tables, batch.seq_lens,
                batch.positions, batch.slots, self.cos_sin, lw.q_norm, lw.k_norm,
                self.hq // self.hkv, self.scale, eps, workspace=batch.workspace,
                num_parts=batch.num_parts, part_size=batch.part_size,
                v_tail=batch.v_tails[li] if batch.v_tails is not None else None,
                tail_slot=batch.tail_slot, write_kv=not rider)
            a2 = torch.empty_like(residual)
            if tp > 1:
                part = ops.dgemm(attn.view(T, self.hq * self.D), lw.w_o, eps=eps,
                                 variant=plan["w_o"])
                comm.tp_all_reduce_resnorm(part, residual, lw.ln2, a2, ss[2 * li])
            else:
                ops.dgemm(attn.view(T, self.hq * self.D), lw.w_o, eps=eps, out=residual,
                          epi=ops.EPI_RESNORM, ss_out=ss[2 * li], a_out=a2, ln_out=lw.ln2,
                          variant=plan["w_o"])
            kvw = ops.KvWrite(qkv, batch.positions, batch.slots, self.cos_sin, lw.k_norm,
                              k_caches[li], v_caches[li], batch.v_tails[li], batch.tail_slot,
                              self.hq, eps) if rider else None
            act = ops.dgemm(a2, lw.w_gate_up, eps=eps, ss_in=ss[2 * li], epi=ops.EPI_SILU,
                            variant=plan["w_gate_up"], kv_write=kvw)
            if li + 1 < L:
                a1 = torch.empty_like(residual)
                if tp > 1:
                    part = ops.dgemm(act, lw.w_down, eps=eps, variant=plan["w_down"])
                    comm.tp_all_reduce_resnorm(part, residual, self.layers[li + 1].ln1, a1,
                                               ss[2 * li + 1])
                else:
                    ops.dgemm(act, lw.w_down, eps=eps, out=residual, epi=ops.EPI_RESNORM,
                              ss_out=ss[2 * li + 1], a_out=a1, ln_out=self.layers[li + 1].ln1,
                              variant=plan["w_down"])
                ss_in = ss[2 * li + 1]
            else:
                x = comm.tp_all_reduce(ops.dgemm(act, lw.w_down, eps=eps, variant=plan["w_down"]))
        h, _ = ops.fused_add_rms_norm(x, residual, self.final_norm, eps)
        return h

    def compute_logits(self, h: torch.Tensor) -> torch.Tensor:
        logits = ops.linear(h, self.lm_head)
        if self.ps.tp_size > 1:
            logits = comm.tp_all_gather_last(logits)
        return logits[:, : self.cfg.vocab_size]
