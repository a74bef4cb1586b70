"""Plain-PyTorch (fp32-accumulating) reference implementations of every kernel.

They define the semantics the HIP kernels are tested against and serve the CPU
engine path.  Cache layouts (BS % 32 == 0, D = 128 on the GPU path):
  K [NB, Hkv, BS, D] shape, stored MFMA-fragment ordered inside each 32-token chunk:
    [BS/32][tile tt 2][k-step D/32][row r 16][32 dims], chunk token o = 8*(r>>2)+4*tt+(r&3)
    -- use k_tokens()/write_k() to index it;
  V [NB, Hkv, BS/8, D, 8] (8-token groups, dim-major).
The kernels' definition is csrc/kernels/host_contract.h ("paged KV cache layout"); this module
derives the layout on its own (views and permutes, no offset arithmetic shared with that header)
and tests/test_kv_layout_cpu.py checks the two against each other.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    F = x.shape[-1] // 2
    g, u = x[..., :F], x[..., F:]
    return (torch.nn.functional.silu(g.float()).to(x.dtype).float() * u.float()).to(x.dtype)


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, scaling: dict | None = None,
                 device=None) -> torch.Tensor:
    """fp32 table [max_pos, D] = [cos | sin] for NeoX-style (rotate-half) rotary."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = scaling["factor"]
        lo = scaling.get("low_freq_factor", 1.0)
        hi = scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        low_wl, high_wl = old / lo, old / hi
        wl = 2 * math.pi / inv_freq
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > low_wl, inv_freq / factor, inv_freq)
        mid = (wl <= low_wl) & (wl >= high_wl)
        scaled = torch.where(mid, (1 - smooth) * inv_freq / factor + smooth * inv_freq, scaled)
        inv_freq = scaled
    t = torch.arange(max_pos, dtype=torch.float64)
    freqs = torch.outer(t, inv_freq)
    cs = torch.cat([freqs.cos(), freqs.sin()], dim=-1).float()
    return cs.to(device) if device is not None else cs


def apply_rope(x: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x [T, H, D] (float) -> rotated (float)."""
    D = x.shape[-1]
    half = D // 2
    cs = cos_sin[positions.long()]
    c = cs[:, None, :half]
    s = cs[:, None, half:]
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


FP8_MAX = 448.0  # OCP e4m3fn


def to_cache(vals: torch.Tensor, cache: torch.Tensor) -> torch.Tensor:
    """Values -> the cache's storage: bf16, or OCP e4m3fn bytes (uint8 cache, scale 1,
    clamped to +-448, round-to-nearest-even like the kernels)."""
    if cache.dtype == torch.uint8:
        f8 = vals.float().clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
        return f8.view(torch.uint8)
    return vals.to(cache.dtype)


def from_cache(t: torch.Tensor) -> torch.Tensor:
    """Cache storage -> values (fp8 bytes widen exactly to bf16)."""
    if t.dtype == torch.uint8:
        return t.view(torch.float8_e4m3fn).to(torch.bfloat16)
    return t


def k_swz(o: int) -> tuple[int, int, int]:
    """Token offset within a block -> (32-token chunk, tile tt, row r) of the K layout."""
    c, oo = divmod(o, 32)
    return c, (oo >> 2) & 1, ((oo >> 3) << 2) | (oo & 3)


# position (tt * 16 + r) of chunk token o, for o = 0..31
K_CHUNK_POS = [k_swz(o)[1] * 16 + k_swz(o)[2] for o in range(32)]


def k_blocks_view(k_cache: torch.Tensor) -> torch.Tensor:
    NB, H, BS, D = k_cache.shape
    assert BS % 32 == 0 and D % 32 == 0, "K cache layout needs BS % 32 == 0"
    return k_cache.view(NB, H, BS // 32, 2, D // 32, 16, 32)


def write_k(k_cache: torch.Tensor, b: int, o: int, val: torch.Tensor) -> None:
    """k_cache[block b, :, token o, :] = val [Hkv, D] in the swizzled layout."""
    c, tt, r = k_swz(o)
    H, D = val.shape
    k_blocks_view(k_cache)[b, :, c, tt, :, r, :] = to_cache(val, k_cache).view(H, D // 32, 32)


def k_tokens(k_cache: torch.Tensor, blocks: torch.Tensor) -> torch.Tensor:
    """Logical K of `blocks` in token order: [len(blocks) * BS, Hkv, D]."""
    NB, H, BS, D = k_cache.shape
    v = k_blocks_view(k_cache)[blocks]                       # [nb, H, C, 2, D/32, 16, 32]
    nb = v.shape[0]
    t = v.permute(0, 2, 3, 5, 1, 4, 6).reshape(nb, BS // 32, 32, H, D)  # pos = tt*16 + r
    t = t[:, :, K_CHUNK_POS]
    return from_cache(t.reshape(nb * BS, H, D))


def write_cache(k: torch.Tensor, v: torch.Tensor, k_cache, v_cache, slots) -> None:
    BS = k_cache.shape[2]
    for t in range(k.shape[0]):
        s = int(slots[t])
        if s < 0:
            continue
        b, o = divmod(s, BS)
        write_k(k_cache, b, o, k[t])
        v_cache[b, :, o // 8, :, o % 8] = to_cache(v[t], v_cache)


def qk_norm_rope_cache(qkv, q_out, k_cache, v_cache, positions, slots, cos_sin, q_w, k_w, Hq,
                       Hkv, eps, apply_rope_flag=True):
    T = qkv.shape[0]
    D = k_cache.shape[3]
    q = qkv[:, : Hq * D].reshape(T, Hq, D)
    k = qkv[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].reshape(T, Hkv, D)
    if q_w is not None:
        q = rms_norm(q, q_w, eps)
    if k_w is not None:
        k = rms_norm(k, k_w, eps)
    qf, kf = q.float(), k.float()
    if apply_rope_flag:
        qf = apply_rope(qf, positions[:T], cos_sin)
        kf = apply_rope(kf, positions[:T], cos_sin)
    q_out.copy_(qf.to(q_out.dtype).reshape(q_out.shape))
    write_cache(kf.to(qkv.dtype), v, k_cache, v_cache, slots[:T])


def reshape_and_cache(k, v, k_cache, v_cache, slots):
    write_cache(k, v, k_cache, v_cache, slots)


def gather_kv(k_cache, v_cache, block_table, kv_len: int):
    """-> K [kv_len, Hkv, D], V [kv_len, Hkv, D] from the paged caches."""
    BS = k_cache.shape[2]
    nb = (kv_len + BS - 1) // BS
    blocks = block_table[:nb].long()
    K = k_tokens(k_cache, blocks)[:kv_len]
    # [nb, Hkv, BS/8, D, 8] -> [nb, BS/8, 8, Hkv, D] -> tokens
    V = v_cache[blocks].permute(0, 2, 4, 1, 3).reshape(nb * BS, v_cache.shape[1], -1)[:kv_len]
    return K, from_cache(V)


def paged_attention(q, k_cache, v_cache, block_tables, seq_lens, q_start, scale):
    """Causal attention of each sequence's new tokens over its paged context.
    q [T, Hq, D]; q_start [B+1] cumulative; seq_lens [B] (kv incl. new tokens)."""
    out = torch.zeros_like(q)
    B = seq_lens.numel()
    Hq = q.shape[1]
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    for b in range(B):
        q0, q1 = int(q_start[b]), int(q_start[b + 1])
        ql = q1 - q0
        if ql == 0:
            continue
        kv = int(seq_lens[b])
        K, V = gather_kv(k_cache, v_cache, block_tables[b], kv)
        Kf = K.float().repeat_interleave(G, dim=1)  # [kv, Hq, D]
        Vf = V.float().repeat_interleave(G, dim=1)
        qf = q[q0:q1].float()  # [ql, Hq, D]
        s = torch.einsum("qhd,khd->hqk", qf, Kf) * scale
        qpos = torch.arange(kv - ql, kv).view(-1, 1)
        kpos = torch.arange(kv).view(1, -1)
        s = s.masked_fill((kpos > qpos)[None], float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hqk,khd->qhd", p, Vf)
        out[q0:q1] = o.to(q.dtype)
    return out


def sample(logits, temperature, top_k, top_p, seeds, steps, greedy_logprobs=False):
    """Reference sampler: greedy for T<=0; else top-k, then top-p (on the top-k
    renormalised distribution), then a draw.  Draws use torch's RNG seeded per row,
    so only the distribution (not the exact token) matches the kernel."""
    B, V = logits.shape
    toks = torch.empty(B, dtype=torch.int64)
    lps = torch.empty(B, dtype=torch.float32)
    for i in range(B):
        x = logits[i].float().cpu()
        T = float(temperature[i])
        if T <= 0:
            toks[i] = int(x.argmax())
            lps[i] = float(torch.log_softmax(x, -1)[toks[i]]) if greedy_logprobs else 0.0
            continue
        z = x / T
        logp = torch.log_softmax(z, dim=-1)
        keep = torch.ones(V, dtype=torch.bool)
        k = int(top_k[i])
        if 0 < k < V:
            kth = torch.topk(z, k).values[-1]
            keep &= z >= kth
        p = float(top_p[i])
        if p < 1.0:
            zz = z.masked_fill(~keep, float("-inf"))
            probs = torch.softmax(zz, dim=-1)
            sp, si = probs.sort(descending=True)
            cum = sp.cumsum(0)
            n = int((cum < p).sum()) + 1
            thr = sp[min(n, V) - 1]
            keep &= probs >= thr
        g = torch.Generator().manual_seed(int(seeds[i]) * 1000003 + int(steps[i]))
        zz = z.masked_fill(~keep, float("-inf"))
        pr = torch.softmax(zz, dim=-1)
        t = int(torch.multinomial(pr, 1, generator=g))
        toks[i] = t
        lps[i] = float(logp[t])
    return toks.to(logits.device), lps.to(logits.device)


def embedding(ids, table, vs, ve):
    ids = ids.long()
    mask = (ids >= vs) & (ids < ve)
    local = (ids - vs).clamp(0, table.shape[0] - 1)
    out = table[local]
    return out * mask[:, None].to(out.dtype)


def moe_topk_softmax(logits, top_k, renorm=True):
    p = torch.softmax(logits.float(), dim=-1)
    w, ids = torch.topk(p, top_k, dim=-1)
    if renorm:
        w = w / w.sum(dim=-1, keepdim=True)
    return w, ids.to(torch.int32)


def moe_align(topk_ids, E, block, cap):
    flat = topk_ids.reshape(-1).long().cpu()
    n = flat.numel()
    sorted_ids = torch.full((cap,), n, dtype=torch.int32)
    offsets = torch.zeros(E + 1, dtype=torch.int32)
    acc = 0
    for e in range(E):  # ids outside [0, E) are skipped
        idx = (flat == e).nonzero().flatten()
        offsets[e] = acc
        sorted_ids[acc:acc + idx.numel()] = idx.to(torch.int32)
        acc += (idx.numel() + block - 1) // block * block
    offsets[E] = acc
    return sorted_ids.to(topk_ids.device), offsets.to(topk_ids.device), acc


def fused_moe(h, w13, w2, topk_w, topk_ids):
    """fp32 reference of the fused expert FFN (bf16 rounding at the same points as the
    kernels: after each GEMM and after silu_and_mul).  Expert ids outside [0, E) -- the
    padding rows of the expert-parallel dispatch -- contribute nothing (as in moe_align)."""
    T, d = h.shape
    E = w13.shape[0]
    out = torch.zeros(T, d, dtype=torch.float32, device=h.device)
    ids = topk_ids.long()
    for e in range(E):
        t_idx, k_idx = (ids == e).nonzero(as_tuple=True)
        if t_idx.numel() == 0:
            continue
        y1 = (h[t_idx].float() @ w13[e].float().t()).to(h.dtype)
        a = silu_and_mul(y1)
        y2 = (a.float() @ w2[e].float().t()).to(h.dtype)
        out.index_add_(0, t_idx, topk_w[t_idx, k_idx].float()[:, None] * y2.float())
    return out.to(h.dtype)


def apply_penalties(logits, rows, toks, counts, presence, frequency, repetition):
    out = logits.clone()
    for r, t, c in zip(rows.tolist(), toks.tolist(), counts.tolist()):
        x = float(out[r, t])
        rep = float(repetition[r])
        if rep != 1.0:
            x = x / rep if x > 0 else x * rep
        x -= float(frequency[r]) * c + (float(presence[r]) if c > 0 else 0.0)
        out[r, t] = x
    return out


def pgemm(x: torch.Tensor, w: torch.Tensor, silu: bool = False,
          offs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 reference of ops.pgemm: x @ w.T (bf16-rounded), or silu(gate) * up over the
    [gate; up] halves of w; offs (cumulative row ends): rows of group g use w[g]."""
    xf = x.float()
    if offs is None:
        y = (xf @ w.float().t()).to(x.dtype)
    else:
        y = torch.empty(x.shape[0], w.shape[-2], dtype=x.dtype, device=x.device)
        lo = 0
        for g, hi in enumerate(offs.tolist()):
            if hi > lo:
                y[lo:hi] = (xf[lo:hi] @ w[g].float().t()).to(x.dtype)
            lo = hi
    return silu_and_mul(y) if silu else y


# ----------------------------------------------------------------------------- exact GEMM oracle
# Operands for which a GEMM's fp32 accumulator is known bit for bit (tests/test_gemm_exact_*):
# small non-zero signed integers, the weight scaled by a power of two.  Every product and every
# partial sum is then an integer multiple of one unit below 2^24 units, so fp32 accumulation
# is exact in ANY order (MFMA, per-wave K splits, split-K slabs, reduce passes, in-launch
# combines) and the only roundings left are the ones the epilogue contract names
# (csrc/kernels/gemm_common.h).
EXACT_LIMIT = 1 << 24   # integers below this are exact in fp32
EXACT_BF16_INT = 256    # integers below this are exact in bf16 (8 significant bits)


class ExactOperands(NamedTuple):
    x: torch.Tensor      # bf16 [M, K] = xi
    w: torch.Tensor      # bf16 [N, K] = wi * unit
    xi: torch.Tensor     # int64 image of x
    wi: torch.Tensor     # int64 image of w (in units)
    unit: float          # the power of two one unit of x @ w.T is worth


def exact_vmax(K: int, resnorm_cols: int = 0) -> int:
    """Largest operand magnitude (3, 2 or 1) that keeps an exact GEMM of depth K readable:
    the integer result has standard deviation E[v^2] * sqrt(K) (v uniform over the non-zero
    integers of [-vmax, vmax]); it is kept <= 128 units, so that >= 95 % of the results lie
    within two standard deviations = 256 units and are exact in bf16 (a one-unit error is
    visible).  resnorm_cols = N of an EPI_RESNORM case: a row's sum of N squared results
    (mean N * std^2, relative spread sqrt(2 / N)) must also stay below 2^24 so the fp32 sum of
    squares is exact whatever the order of the atomics: mean <= 0.6 * 2^24."""
    for vmax in (3, 2, 1):
        ev2 = sum(v * v for v in range(1, vmax + 1)) / vmax
        std = ev2 * math.sqrt(K)
        if std <= 128 and (not resnorm_cols or resnorm_cols * (std * std + 16) <= 0.6 * EXACT_LIMIT):
            return vmax
    raise ValueError(f"no exact operand range for K = {K}, resnorm N = {resnorm_cols}")


def _nonzero_ints(shape, vmax: int, g: torch.Generator) -> torch.Tensor:
    mag = torch.randint(1, vmax + 1, shape, generator=g, dtype=torch.int64)
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
    return mag * sign


def exact_gemm_operands(M: int, N: int, K: int, seed: int, vmax: int = 0,
                        w_shift: int = 6) -> ExactOperands:
    """x [M, K] and w [N, K] in bf16 with no zero entry, their int64 images and the unit
    2^-w_shift: x = xi, w = wi * unit, entries uniform over the non-zero integers of
    [-vmax, vmax] (vmax = 0: exact_vmax(K))."""
    vmax = vmax or exact_vmax(K)
    assert 1 <= vmax <= 127, "operands must stay exact in bf16"
    g = torch.Generator().manual_seed(seed)
    xi = _nonzero_ints((M, K), vmax, g)
    wi = _nonzero_ints((N, K), vmax, g)
    unit = 2.0 ** -w_shift
    return ExactOperands(xi.to(torch.bfloat16), (wi.double() * unit).to(torch.bfloat16), xi, wi,
                         unit)


def exact_int_matmul(xi: torch.Tensor, wi: torch.Tensor) -> torch.Tensor:
    """xi @ wi.T as int64.  Computed in float64 (BLAS): every partial sum is an integer far
    below 2^53, so the double result is the integer result."""
    return (xi.double() @ wi.double().t()).round().to(torch.int64)


def bf16_rne(v: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16, one round-to-nearest-even (no intermediate fp32 rounding; normal
    range only)."""
    m, e = torch.frexp(v.double())
    return torch.ldexp(torch.round(m * 256.0), e - 8).to(torch.bfloat16)


def bf16_ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Number of bf16 values between a and b (0 = equal bits or +-0), int64."""
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordered(a) - ordered(b)).abs()


class ExactExpected(NamedTuple):
    out: torch.Tensor                    # bf16: y, the new residual s, or the SwiGLU output
    a: Optional[torch.Tensor] = None     # EPI_RESNORM: bf16(s * ln)
    ss: Optional[torch.Tensor] = None    # EPI_RESNORM: fp32 exact row sums of s^2


def _exact_bf16(vi: torch.Tensor, unit: float) -> torch.Tensor:
    """bf16(vi * unit) by one RNE; vi * unit is exact in fp32 (|vi| < 2^24)."""
    assert int(vi.abs().max()) < EXACT_LIMIT
    return (vi.double() * unit).float().to(torch.bfloat16)


def exact_gemm_expected(yi: torch.Tensor, unit: float, epi: int = 0,
                        residual_i: Optional[torch.Tensor] = None,
                        ln: Optional[torch.Tensor] = None,
                        row_scale: Optional[torch.Tensor] = None,
                        row_shift: Optional[torch.Tensor] = None) -> ExactExpected:
    """What the epilogue contract (csrc/kernels/gemm_common.h) makes of the exact accumulator
    yi (int64, in units; unit a power of two, or a [1, N] float64 tensor of them: per-channel
    fp8 scales), rounding to nearest even at exactly the points it names.
      epi 0 (EPI_STORE)    bf16(y)
      epi 1 (EPI_RESNORM)  s = bf16(bf16(y) + residual), a = bf16(s * ln), ss = sum_n s^2;
                           residual_i int64 in units, ln any bf16 (an 8-bit x 8-bit mantissa
                           product is exact in fp32)
      epi 2 (EPI_SILU)     yi = [gate | up] columns ([gate; up] weight rows -- the kernels read
                           them in silu_interleave_perm order and write features in natural
                           order): g = bf16(y_gate), u = bf16(y_up),
                           out = bf16(bf16(silu(g)) * u), silu and the product in float64
    row_scale (float64 [M], EPI_STORE only): bf16(y * row_scale) in float64 -- the ss_in row
    scale, whose hardware rsqrt is not exact (compare within one bf16 ulp).
    row_shift (int64 [M], any epilogue): an ss_in row scale of exactly 2^-row_shift[m].  Row m
    is then exact in units of unit * 2^-row_shift[m] (the residual, a multiple of the unit, is
    a multiple of that too), so every rounding of the contract stays known bit for bit."""
    if row_scale is not None:
        assert epi == 0 and row_shift is None
        return ExactExpected(bf16_rne(yi.double() * unit * row_scale.double()[:, None]))
    if row_shift is not None:
        unit = unit * 2.0 ** -row_shift.double()[:, None]
        if residual_i is not None:
            residual_i = residual_i * 2 ** row_shift[:, None]
    y = _exact_bf16(yi, unit)
    if epi == 0:
        return ExactExpected(y)
    if epi == 1:
        ti = (y.double() / unit).round().to(torch.int64) + residual_i
        s = _exact_bf16(ti, unit)
        si = (s.double() / unit).round().to(torch.int64)
        a = (s.float() * ln.float()).to(torch.bfloat16)
        ssi = (si * si).sum(-1)
        assert int(ssi.max()) < EXACT_LIMIT, "row sum of squares not exact in fp32"
        u2 = unit * unit
        return ExactExpected(s, a, (ssi.double() * (u2[:, 0] if row_shift is not None else u2)).float())
    F = yi.shape[1] // 2
    g, u = y[:, :F].double(), y[:, F:].double()
    sg = bf16_rne(g / (1.0 + torch.exp(-g)))
    return ExactExpected(bf16_rne(sg.double() * u))


# ----------------------------------------------------------------------------- attention probes
# Inputs for which paged attention's output is known without an attention reference
# (tests/test_attention_probes_*): a NEEDLE query is beta times one cached key, so that key
# scores ~beta * |k|^2 / sqrt(D) nats above keys that score beta * N(0, 1); the softmax is
# one-hot far below fp32 resolution and the output is the target's V row itself.  One wrong
# key, one rolled V group or one leaked stale slot then misses by order 1, not by 1 / kv_len.
#
# The stale-slot contract the poison encodes: cache slots at positions >= kv_len of a
# sequence's last block (the rest of its last 8-token V group included) and the blocks that
# unused block-table entries name hold FINITE values and are never attended.  The kernels
# multiply P = 0 into whatever V holds there, so a NaN or Inf would propagate by design; the
# engine's caches start zero-initialised.  Every block id stays in range: an out-of-range id
# would be an out-of-bounds read, not a probe.
NEEDLE_BETA = 4.0
POISON_K_GAIN = 8.0
POISON_V = 1e30          # bf16: 1e30; e4m3: clamps to 448
NEEDLE_ABS_FLOOR = 1e-6  # e4m3 V holds exact zeros; there the other keys' residue shows


def write_tokens(k_cache, v_cache, blocks, K, V) -> None:
    """Whole blocks at once: K, V [len(blocks) * BS, Hkv, D] in token order -> the paged
    layouts (the inverse of gather_kv over `blocks`)."""
    NB, H, BS, D = k_cache.shape
    blocks = blocks.long()
    nb = blocks.numel()
    assert K.shape == (nb * BS, H, D) and V.shape == K.shape
    arr = torch.empty(nb, BS // 32, 32, H, D, dtype=k_cache.dtype)
    arr[:, :, K_CHUNK_POS] = to_cache(K, k_cache).reshape(nb, BS // 32, 32, H, D)
    arr = arr.reshape(nb, BS // 32, 2, 16, H, D // 32, 32).permute(0, 4, 1, 2, 5, 3, 6)
    k_blocks_view(k_cache)[blocks] = arr
    # tokens [nb, BS/8, 8, H, D] -> [nb, H, BS/8, D, 8]
    v_cache[blocks] = to_cache(V, v_cache).reshape(nb, BS // 8, 8, H, D).permute(0, 3, 1, 4, 2)


def poison_direction(Hkv: int, D: int, seed: int) -> torch.Tensor:
    """[Hkv, D] bf16: the direction every poisoned K slot holds POISON_K_GAIN times."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Hkv, D, generator=g).bfloat16()


def poison_stale(k_cache, v_cache, block_tables, seq_lens, poison_block: int,
                 pdir: torch.Tensor, keep_group=()) -> None:
    """Poison, in place, what no sequence may attend (the contract above): every slot at a
    position >= kv_len of each sequence's last block gets K = POISON_K_GAIN * pdir and
    V = POISON_V, block `poison_block` (which no sequence owns) gets them in every slot, and
    the block-table entries past each sequence's last block point at it.  Sequences must not
    share blocks with longer ones."""
    BS = k_cache.shape[2]
    pk = pdir.float() * POISON_K_GAIN
    pv = torch.full_like(pk, POISON_V)
    for o in range(BS):
        write_k(k_cache, poison_block, o, pk)
        v_cache[poison_block, :, o // 8, :, o % 8] = to_cache(pv, v_cache)
    for s in range(seq_lens.numel()):
        L = int(seq_lens[s])
        nb = (L + BS - 1) // BS
        block_tables[s, nb:] = poison_block
        if L % BS == 0:
            continue
        b = int(block_tables[s, nb - 1])
        assert b != poison_block
        for o in range(L % BS, BS):
            write_k(k_cache, b, o, pk)
            v_cache[b, :, o // 8, :, o % 8] = to_cache(pv, v_cache)


def needle_q(K: torch.Tensor, targets: torch.Tensor, G: int, beta: float = NEEDLE_BETA,
             unit: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [T, Hq, D] = bf16(beta * K[targets[t, h], h // G]) for K [n, Hkv, D] in token order.
    unit [T, Hq] bool: those rows are scaled to length beta * sqrt(D) instead, whatever the
    key's own length (the forbidden needles, whose key may be poison)."""
    T, Hq = targets.shape
    kvh = (torch.arange(Hq) // G).expand(T, Hq)
    k = K.float()[targets.long(), kvh]                      # [T, Hq, D]
    q = beta * k
    if unit is not None:
        qn = beta * math.sqrt(k.shape[-1]) * k / k.norm(dim=-1, keepdim=True).clamp_min(1e-20)
        q = torch.where(unit[..., None], qn, q)
    return q.to(torch.bfloat16)


def needle_expect(V: torch.Tensor, targets: torch.Tensor, G: int) -> torch.Tensor:
    """[T, Hq, D] bf16: V[targets[t, h], h // G] for V [n, Hkv, D] in token order."""
    T, Hq = targets.shape
    kvh = (torch.arange(Hq) // G).expand(T, Hq)
    return V[targets.long(), kvh].to(torch.bfloat16)


def unrope(x: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """The inverse of apply_rope (the rotation is orthogonal): x [T, H, D] float."""
    half = cos_sin.shape[1] // 2
    inv = torch.cat([cos_sin[:, :half], -cos_sin[:, half:]], dim=-1)
    return apply_rope(x, positions, inv)


def needle_mismatch(out: torch.Tensor, expect: torch.Tensor):
    """Needle comparator: -> (bad [..] bool per element, largest bf16 ulp distance among the
    elements the absolute floor does not excuse).  An element passes within one bf16 ulp of
    the expected V entry or within NEEDLE_ABS_FLOOR of it."""
    out, expect = out.cpu(), expect.cpu()
    finite = torch.isfinite(out.float())
    ulp = bf16_ulp_distance(out, expect)
    near = (out.float() - expect.float()).abs() <= NEEDLE_ABS_FLOOR
    bad = ~finite | ((ulp > 1) & ~near)
    seen = torch.where(near | ~finite, torch.zeros_like(ulp), ulp)
    return bad, int(seen.max()) if seen.numel() else 0


def close_mismatch(out: torch.Tensor, expect: torch.Tensor, tol: float):
    """-> (bad per element, worst err / limit) for |out - expect| <= tol + tol * |expect|."""
    o, e = out.float().cpu(), expect.float().cpu()
    lim = tol + tol * e.abs()
    err = (o - e).abs()
    err = torch.where(torch.isfinite(o), err, torch.full_like(err, float("inf")))
    return err > lim, float((err / lim).max()) if err.numel() else 0.0


# Score patterns: key j's log2-domain score is a chosen function of j, constant or linear
# over `tile` keys (the prefill kernel's 64-key tile, the decode kernel's 32-key chunk), so the
# running maximum of a flash-style loop moves exactly where the pattern says.
SCORE_PATTERNS = ("rise6", "rise10", "step7.9", "step8.1", "fall10", "saw12", "spikes", "creep2",
                  "peak10")


def score_pattern(name: str, n: int, tile: int) -> torch.Tensor:
    """float64 [n]: the log2-domain score of key j.
      rise6 / rise10   linear, +6 / +10 per tile (crosses an 8-unit threshold every second
                       tile / every tile)
      step7.9/step8.1  constant per tile, +7.9 / +8.1 per tile (either side of the threshold)
      fall10           linear, -10 per tile from 10 * tiles (the first tile holds the maximum)
      saw12            constant per tile: 0, 12, 24, 0, 12, 24, ...
      spikes           0 everywhere but +900 on one key of the second tile and +1000 on one key
                       of the second-to-last tile
      creep2           constant per tile: 0, then 7.5 + 2 per tile (creeps past the threshold)
      peak10           +10 per tile up to the tile at a third of the context, then -10 per tile
                       (the maximum sits in an early split-KV partition)"""
    j = torch.arange(n, dtype=torch.float64)
    t = torch.div(j, tile, rounding_mode="floor")
    nt = (n + tile - 1) // tile
    if name == "rise6":
        return 6.0 * j / tile
    if name == "rise10":
        return 10.0 * j / tile
    if name == "step7.9":
        return 7.9 * t
    if name == "step8.1":
        return 8.1 * t
    if name == "fall10":
        return 10.0 * nt - 10.0 * j / tile
    if name == "saw12":
        return 12.0 * (t % 3)
    if name == "spikes":
        s = torch.zeros(n, dtype=torch.float64)
        if n > tile + 5:
            s[tile + 5] = 900.0
        if nt >= 4:
            s[(nt - 2) * tile + tile // 2] = 1000.0
        return s
    if name == "creep2":
        return torch.where(t == 0, torch.zeros_like(t), 7.5 + 2.0 * (t - 1))
    if name == "peak10":
        top = nt // 3
        return 10.0 * (top - (t - top).abs())
    raise ValueError(name)


def pattern_kq(scores: torch.Tensor, Hkv: int, rows: int, Hq: int, scale: float, seed: int,
               beta: float = NEEDLE_BETA, D: int = 128):
    """K [n, Hkv, D] (float) and q [rows, Hq, D] bf16 whose log2-domain scores
    q . k * scale * log2(e) follow `scores` [n]: K = c_j u + noise, q = beta u + noise, both
    noises orthogonal to the sign vector u (|u|^2 = 2), so the noise only decorrelates the
    bf16 roundings and adds a few hundredths of a unit of score."""
    g = torch.Generator().manual_seed(seed)
    n = scores.numel()
    u = (torch.randint(0, 2, (Hkv, D), generator=g).double() * 2 - 1) * 0.125
    c = scores.double() / (beta * 2.0 * scale * math.log2(math.e))

    def perp(x, uu):  # remove the component along u
        return x - (x * uu).sum(-1, keepdim=True) / 2.0 * uu
    kn = perp(torch.randn(n, Hkv, D, generator=g, dtype=torch.float64) * 0.25, u[None])
    K = c[:, None, None] * u[None] + kn
    uq = u.repeat_interleave(Hq // Hkv, dim=0)                # [Hq, D]
    qn = perp(torch.randn(rows, Hq, D, generator=g, dtype=torch.float64) * 0.02, uq[None])
    q = (beta * uq[None] + qn).to(torch.bfloat16)
    return K.float(), q


def fa_tile_model(s2: torch.Tensor, V: torch.Tensor, limit: int, T: float = 8.0,
                  tile: int = 64, rescale_o: bool = True):
    """A from-scratch model of one row of a flash-style tile loop with a deferred running
    maximum -- the specification the prefill kernel's loop is read against, not a port of it.
    s2 [n] float64 log2-domain scores, V [n, D]; keys 0..limit are visible.  Per `tile` keys:
    the running max m moves to the tile's max only when that exceeds m + T (T = 0: the exact
    max); P = bf16(2^(s - m)) feeds o, its fp32 value feeds l; o and l are fp32 and are
    rescaled by 2^(m_old - m_new) when m moves.  -> (o / l as float64 [D], number of moves
    of m after the first tile).  rescale_o=False leaves o unscaled (the bug the rising
    patterns must expose)."""
    m = float("-inf")
    l = torch.zeros((), dtype=torch.float32)
    o = torch.zeros(V.shape[1], dtype=torch.float32)
    moves = 0
    Vb = V.to(torch.bfloat16).float()
    for k0 in range(0, limit + 1, tile):
        k1 = min(k0 + tile, limit + 1)
        s = s2[k0:k1]
        mc = max(m, float(s.max()))
        m_new = mc if mc > m + T else m
        if m_new != m:
            alpha = torch.tensor(2.0 ** (m - m_new), dtype=torch.float32)
            l = l * alpha
            if rescale_o:
                o = o * alpha
            moves += k0 > 0
            m = m_new
        p = torch.exp2((s - m).float())
        l = l + p.sum()
        o = o + p.to(torch.bfloat16).float() @ Vb[k0:k1]
    return (o.double() / l.double()), int(moves)
