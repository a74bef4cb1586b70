"""MXFP4 expert weights for MoE on the GPU: the grouped 4-bit-weight GEMM (csrc/kernels/
moe_q4gemm.hip) bit for bit, the routing of every block scale, adversarial codes against the
fp32 contract, ops.fused_moe on Mxfp4Experts, the binding's checks, the prefill path through
the shared dequantization scratch, and the engine (captured, eager, fp8 KV, expert-parallel
over two processes).

The bit-exact part follows tests/test_moe_fp8_gpu.py: integer activations, weights in
{0, +-1, +-2, +-3} (exact e2m1 codes) and block scales 2^-s with s drawn independently per
(expert, channel, 32-block) from 3..8, so every product is a multiple of 2^-8 and -- checked
when the oracle is built -- every sum of |products| stays below 2^24 of those units: the fp32
accumulator is exact in any order, and a scale taken from the wrong expert, channel, block or
half of the gate/up interleave changes bits.  Only SwiGLU (__expf) gets the project's bound of
two bf16 ulps."""
import functools
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import _runtime_loader, ops
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
from aws_k8s_ansible_provisioner_amd.models.config import get_config
from aws_k8s_ansible_provisioner_amd.models.moe import MoEBlock
from aws_k8s_ansible_provisioner_amd.models.reference_forward import dense_logits
from aws_k8s_ansible_provisioner_amd.models.transformer import DecoderLM
from aws_k8s_ansible_provisioner_amd.ops import reference as ref
from aws_k8s_ansible_provisioner_amd.ops.quant import (Fp8Experts, Mxfp4Experts,
                                                       quantize_fp8_experts,
                                                       quantize_mxfp4_experts)
from aws_k8s_ansible_provisioner_amd.parallel.state import ParallelState

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -24576.0      # bf16 sentinel: exact in bf16, far outside every result
SENT_F32 = 1.5e30    # fp32 partials sentinel
PAD_ROWS = 3
ULP_SILU = 2         # __expf in silu: the bound tests/test_gemm_exact_gpu.py derives
E4, TOPK, COUNTS = 4, 2, (37, 0, 70, 1)   # rows per expert: one empty, one over 64 rows, tails
N_EXACT = 320        # two full 128-column tiles and a 64-column remainder
S_LO, S_HI = 3, 8    # block scales 2^-s, s in S_LO..S_HI: a span of 5 <= 6
UNIT = 2.0 ** -S_HI  # every product is a multiple of this
E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6],
                    dtype=torch.float64)
INT_CODE = {0: 0, 1: 2, 2: 4, 3: 5, -1: 10, -2: 12, -3: 13}   # integer -> e2m1 code


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.load_native(required=True)


def _seed(*k):
    s = 0
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def _close(a, b, atol, rtol=0.0):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    assert bool((err <= lim).all()), f"max err {err.max().item():.4g} (atol {atol})"


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    bad = (ref.bf16_ulp_distance(got, want) != 0) if got.dtype == torch.bfloat16 else got != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, "
                                 f"first at {bad.nonzero()[0].tolist()}: got "
                                 f"{got[bad][0].item()} want {want[bad][0].item()}")


def flat_canary(n, dtype, sent, tail=64):
    big = torch.full((n + tail,), sent, dtype=dtype, device=DEV)
    return big, big[:n]


def pack(codes):
    """e2m1 codes [..., K] (0..15) -> bytes [..., K/2], element 2j in the low nibble."""
    c = codes.to(torch.uint8)
    return c[..., 0::2] | (c[..., 1::2] << 4)


# ------------------------------------------------------------------ bit-exact moe_q4gemm
@functools.lru_cache(maxsize=None)
def hand_align(bm):
    """A hand-made moe_align result for COUNTS: (sorted_ids, inv, tile_expert, padded rows
    in use, n).  Flat index i = token i // TOPK, slot i % TOPK."""
    ids = [e for e, c in enumerate(COUNTS) for _ in range(c)]
    n = len(ids)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).tolist()
    ids = [ids[p] for p in perm]
    cap = ops.moe_capacity(n, E4, bm)
    sorted_ids = torch.full((cap,), n, dtype=torch.int32)
    inv = torch.full((n,), -1, dtype=torch.int32)
    tile_expert = torch.full((cap // bm,), -1, dtype=torch.int32)
    pos = 0
    for e in range(E4):
        idx = [i for i, x in enumerate(ids) if x == e]
        for j, i in enumerate(idx):
            sorted_ids[pos + j] = i
            inv[i] = pos + j
        nt = -(-len(idx) // bm)
        tile_expert[pos // bm:pos // bm + nt] = e
        pos += nt * bm
    assert pos < cap, "no tile without an expert"
    assert any(c > bm for c in COUNTS) and any(c % bm for c in COUNTS) and 0 in COUNTS
    return sorted_ids, inv, tile_expert, pos, n


@functools.lru_cache(maxsize=None)
def oracle(bm, N, K, gather):
    """Integer operands of a grouped GEMM over the hand-made alignment: x (bf16), per used row
    its integer A row and expert, the packed e2m1 codes, the e8m0 scale codes, and the weight
    integers in units of UNIT (wi * 2^(S_HI - s) per block).  Padding rows of a gathering launch
    read row 0."""
    sorted_ids, inv, tile_expert, used, n = hand_align(bm)
    cap = sorted_ids.numel()
    rows_a = n // TOPK if gather else cap
    g = torch.Generator().manual_seed(_seed(bm, N, K, gather))
    xi = ref.exact_gemm_operands(rows_a, 1, K, _seed(bm, N, K, gather, 1), ref.exact_vmax(K)).xi
    wi = torch.randint(-3, 4, (E4, N, K), generator=g)
    lut = torch.zeros(7, dtype=torch.uint8)
    for v, c in INT_CODE.items():
        lut[v + 3] = c
    codes = lut[wi + 3]
    assert torch.equal(E2M1[codes.long()], wi.double()), "weight integers exact in e2m1"
    shift = torch.randint(S_LO, S_HI + 1, (E4, N, K // 32), generator=g)
    wu = wi * (2 ** (S_HI - shift)).repeat_interleave(32, dim=2)       # in units of UNIT
    r = torch.arange(used)
    if gather:
        sid = sorted_ids[:used].long()
        arow = torch.where(sid < n, sid // TOPK, torch.zeros_like(sid))
    else:
        arow = r
    expert = tile_expert[r // bm].long()
    xr = xi[arow]
    # every fp32 partial sum, in any order, is an integer number of units below 2^24
    mag = int_matmul(xr.abs(), wu.abs(), expert)
    assert int(mag.max()) < ref.EXACT_LIMIT, "partial sums not exact in fp32"
    return xi.to(torch.bfloat16), xr, wu, pack(codes), (127 - shift).to(torch.uint8), expert


def int_matmul(xi, wi, expert, k0=0, k1=None):
    yi = torch.zeros(xi.shape[0], wi.shape[1], dtype=torch.int64)
    for e in range(wi.shape[0]):
        m = expert == e
        if bool(m.any()):
            yi[m] = ref.exact_int_matmul(xi[m][:, k0:k1], wi[e][:, k0:k1])
    return yi


def _exact_cases():
    """Enumerated from moe_q4gemm_supported: 32- and 64-row tiles, every compiled ring depth,
    1 / 2 / 4 K slices, gather and SwiGLU on and off; per slice one ring fill, or (pf 1, and
    the 64-row 4-slice case) several wraps; each with whole 128-deep steps and -- where K stays
    a multiple of 128, i.e. with 2 or 4 slices -- with slices that end in a 64-deep half step."""
    sup = _runtime_loader.contract().moe_q4gemm_supported
    out = []
    for bm in (32, 64):
        for pf in (1, 2, 4):
            for splitk in (1, 2, 4):
                for gather in (True, False):
                    for silu in (True, False):
                        wraps = 4 if (pf == 1 or (bm == 64 and splitk == 4)) else 1
                        for half in (False, True):
                            K = splitk * (pf * 128 * wraps - (64 if half else 0))
                            if sup(N_EXACT, K, pf, silu, splitk):
                                out.append((bm, pf, splitk, gather, silu, K))
    return out


EXACT_CASES = _exact_cases()


def test_exact_cases_cover_the_variants():
    sup = _runtime_loader.contract().moe_q4gemm_supported
    # per (bm, pf): silu 2 (splitk 1, whole steps), plain splitk 1: 2, splitk 2 and 4: 4 each
    assert len(EXACT_CASES) == 2 * 3 * (2 + 2 + 4 + 4)
    assert {c[1] for c in EXACT_CASES} == {1, 2, 4} and {c[2] for c in EXACT_CASES} == {1, 2, 4}
    assert all(c[5] % 128 == 0 for c in EXACT_CASES)
    for bm in (32, 64):
        for pf in (1, 2, 4):
            mine = [c for c in EXACT_CASES if c[0] == bm and c[1] == pf]
            assert any((c[5] // c[2]) % 128 == 64 for c in mine), "a half step"
            assert any(c[4] for c in mine) and any(c[3] and not c[4] for c in mine)
    assert any((c[5] // c[2] + 127) // 128 > c[1] for c in EXACT_CASES)   # several wraps
    assert not sup(N_EXACT, 1024, 8, 0, 1), "ring depth 8 is not compiled"
    assert not sup(320, 96, 1, 0, 1) and not sup(320, 192, 1, 0, 1)
    assert not sup(320, 256, 3, 0, 1) and not sup(324, 256, 1, 0, 1)


@pytest.mark.parametrize("bm,pf,splitk,gather,silu,K", EXACT_CASES)
def test_exact_moe_q4gemm(bm, pf, splitk, gather, silu, K):
    N = N_EXACT
    x, xi, wu, packed, scodes, expert = oracle(bm, N, K, gather)
    sorted_ids, inv, tile_expert, used, n = hand_align(bm)
    rows = tile_expert.numel() * bm
    a, wq, sc = x.to(DEV), packed.to(DEV), scodes.to(DEV)
    sid, te = sorted_ids.to(DEV), tile_expert.to(DEV)
    T, d = n // TOPK, N
    g = torch.Generator().manual_seed(_seed(bm, pf, splitk))
    wts = 2.0 ** -torch.randint(1, 4, (T, TOPK), generator=g).float()
    inv2 = inv.clone()
    inv2[5] = -1                                   # a skipped (expert-parallel padding) slot
    live = (inv2 >= 0).view(T, TOPK)
    yi = int_matmul(xi, wu, expert)
    if splitk > 1:
        pbig, pflat = flat_canary(splitk * rows * N, torch.float32, SENT_F32)
        P = pflat.view(splitk, rows, N)
        kps = K // splitk
        for launch in range(2):
            torch.ops.akap.moe_q4gemm(pflat, a, wq, sc, sid, te, n, TOPK, gather, False, pf,
                                      bm, splitk)
            for z in range(splitk):
                want = int_matmul(xi, wu, expert, z * kps, (z + 1) * kps).double() * UNIT
                assert_bits(P[z, :used], want.float(), f"partial slice {z} (launch {launch})")
                assert bool((P[z, used:] == SENT_F32).all()), "rows of expert-less tiles written"
            assert bool((pbig[pflat.numel():] == SENT_F32).all()), "write past the partials"
            if launch == 0:
                first = pflat.clone()
        assert torch.equal(first.view(torch.int32), pflat.view(torch.int32)), "second launch differs"
        cbig, cflat = flat_canary(T * d, torch.bfloat16, SENT)
        torch.ops.akap.moe_combine_split(pflat, wts.to(DEV), inv2.to(DEV), cflat.view(T, d),
                                         splitk, rows)
        y = (yi.double() * UNIT)[inv2.clamp(min=0).long()].view(T, TOPK, d)
        acc = (y * (wts.double() * live)[:, :, None]).sum(1)
        assert_bits(cflat.view(T, d), acc.float().to(torch.bfloat16), "moe_combine_split")
        assert bool((cbig[T * d:] == SENT).all())
        return
    cols = N // 2 if silu else N
    big = torch.full((rows + PAD_ROWS, cols), SENT, dtype=torch.bfloat16, device=DEV)
    out = big[:rows]
    want = ref.exact_gemm_expected(yi, UNIT, 2 if silu else 0).out
    for launch in range(2):
        torch.ops.akap.moe_q4gemm(out, a, wq, sc, sid, te, n, TOPK, gather, silu, pf, bm, 1)
        if silu:
            dist = int(ref.bf16_ulp_distance(out[:used].cpu(), want).max())
            print(f"[ulp] moe_q4gemm/silu: max distance {dist} (bound {ULP_SILU})")
            assert dist <= ULP_SILU
        else:
            assert_bits(out[:used], want, f"y (launch {launch})")
        assert bool((out[used:] == SENT).all()), "rows of expert-less tiles written"
        assert bool((big[rows:] == SENT).all()), "write past the output"
        if launch == 0:
            first = out.clone()
    assert torch.equal(first.view(torch.int16), out.view(torch.int16)), "second launch differs"
    if not silu:
        cbig, cflat = flat_canary(T * d, torch.bfloat16, SENT)
        torch.ops.akap.moe_combine(out, wts.to(DEV), inv2.to(DEV), cflat.view(T, d))
        y = want.double()[inv2.clamp(min=0).long()].view(T, TOPK, d)
        acc = (y * (wts.double() * live)[:, :, None]).sum(1)
        assert_bits(cflat.view(T, d), acc.float().to(torch.bfloat16), "moe_combine")
        assert bool((cbig[T * d:] == SENT).all())


# ------------------------------------------------------------------ scale routing
ROUTE_K, ROUTE_N = 384, 128   # 12 scale blocks: split 1 = 3 steps; split 2 = (step + half step) x 2


@functools.lru_cache(maxsize=None)
def _routing_operands():
    """Every weight is 1.0 (code 2); the 12 blocks of each (expert, channel) row carry 12
    distinct powers of two, 2^-6 .. 2^5, in an order drawn per row: a scale read from another
    block, channel, expert or half of the interleave is off by a power of two almost surely."""
    nb = ROUTE_K // 32
    g = torch.Generator().manual_seed(11)
    order = torch.stack([torch.randperm(nb, generator=g) for _ in range(E4 * ROUTE_N)])
    codes = (121 + order).view(E4, ROUTE_N, nb).to(torch.uint8)
    q = torch.full((E4, ROUTE_N, ROUTE_K // 2), 0x22, dtype=torch.uint8)
    return q, codes


@pytest.mark.parametrize("bm", [32, 64])
@pytest.mark.parametrize("mode", ["plain", "split2", "silu"])
def test_each_block_scale_reaches_its_block(bm, mode):
    """The input is 1 inside one 32-block and 0 elsewhere, so Y[r, n] = 32 * 2^(code - 127) of
    exactly that block of row n of the tile's expert.  Every block is probed: the first and
    last of a whole step, both of a half step (split2: 192-deep slices), every slice, and the
    gate and up rows of the SwiGLU interleave."""
    q, codes = _routing_operands()
    sorted_ids, inv, tile_expert, used, n = hand_align(bm)
    rows = tile_expert.numel() * bm
    sid, te = sorted_ids.to(DEV), tile_expert.to(DEV)
    wq, sc = q.to(DEV), codes.to(DEV)
    expert = tile_expert[torch.arange(used) // bm].long()
    N, K = ROUTE_N, ROUTE_K
    for b in range(K // 32):
        a = torch.zeros(rows, K, dtype=torch.bfloat16)
        a[:, 32 * b:32 * b + 32] = 1
        y = 32.0 * torch.exp2(codes[expert, :, b].double() - 127)          # [used, N], exact
        if mode == "split2":
            P = torch.full((2, rows, N), SENT_F32, device=DEV)
            torch.ops.akap.moe_q4gemm(P.view(-1), a.to(DEV), wq, sc, sid, te, n, TOPK, False,
                                      False, 1, bm, 2)
            z = b // 6
            assert_bits(P[z, :used], y.float(), f"block {b}: slice {z}")
            assert bool((P[1 - z, :used] == 0).all()), f"block {b}: the other slice is not zero"
        elif mode == "plain":
            out = torch.full((rows, N), SENT, dtype=torch.bfloat16, device=DEV)
            torch.ops.akap.moe_q4gemm(out, a.to(DEV), wq, sc, sid, te, n, TOPK, False, False, 1,
                                      bm, 1)
            assert_bits(out[:used], y.to(torch.bfloat16), f"block {b}")
        else:
            out = torch.full((rows, N // 2), SENT, dtype=torch.bfloat16, device=DEV)
            torch.ops.akap.moe_q4gemm(out, a.to(DEV), wq, sc, sid, te, n, TOPK, False, True, 1,
                                      bm, 1)
            gate, up = y[:, :N // 2], y[:, N // 2:]                         # powers of two
            want = ref.bf16_rne(ref.bf16_rne(gate / (1.0 + torch.exp(-gate))).double() * up)
            dist = int(ref.bf16_ulp_distance(out[:used].cpu(), want).max())
            assert dist <= ULP_SILU, f"block {b}: {dist} ulp"


# ------------------------------------------------------------------ adversarial codes
def _adversarial_experts(E, N, K):
    """Nibbles uniform over all 16 codes (+-0 and +-6 included); scale codes 127 + U{-6..6},
    independent per block, as tests/test_mxfp4_weights_gpu.py::_adversarial_weight."""
    g = torch.Generator().manual_seed(E * 17 + N * 13 + K)
    q = torch.randint(0, 256, (E, N, K // 2), generator=g).to(torch.uint8)
    scale = (127 + torch.randint(-6, 7, (E, N, K // 32), generator=g)).to(torch.uint8)
    return Mxfp4Experts(q, scale)


def _deq64(w):
    """The dequantized experts in fp64, written independently of Mxfp4Experts.float."""
    q = w.q.cpu()
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(w.shape).long()
    return E2M1[codes] * torch.exp2(w.scale.cpu().double() - 127).repeat_interleave(32, dim=2)


@pytest.mark.parametrize("E,topk,K,N", [(4, 2, 256, 320), (16, 4, 384, 128)])
@pytest.mark.parametrize("bm", [32, 64])
def test_adversarial_codes_match_the_fp32_contract(E, topk, K, N, bm):
    """The bound of tests/test_mxfp4_weights_gpu.py, from the number formats: every product
    x * w is exact in fp32; the fp32 summation errs by at most (K - 1) 2^-24 sum_k |x w| in any
    order, and the one rounding of the sum s to bf16 by at most 2^-8 |s|.  So |y - ref| <=
    2^-8 |ref| + 2^-23 K sum_k |x w|.  A wrong or missing block scale is off by a factor of two
    or more in a 32-deep block."""
    w = _adversarial_experts(E, N, K)
    T = 40
    g = torch.Generator().manual_seed(T + E)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    n = T * topk
    cap = ops.moe_capacity(n, E, bm)
    inv = torch.empty(n, dtype=torch.int32, device=DEV)
    te = torch.empty(cap // bm, dtype=torch.int32, device=DEV)
    sid, _, _ = ops.moe_align(ids.to(DEV), E, bm, inv=inv, tile_expert=te)
    big = torch.full((cap + PAD_ROWS, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    wd = w.to(DEV)
    torch.ops.akap.moe_q4gemm(big[:cap], x.to(DEV), wd.q, wd.scale, sid, te, n, topk, True, False,
                              ops._moe_qpf(K), bm, 1)
    torch.cuda.synchronize()
    assert bool(big[cap:].isnan().all()), "write past the output"
    got = big[:cap].cpu()[inv.cpu().long()].double()              # [n, N], flat (token, slot)
    deq = _deq64(w)
    flat = ids.reshape(-1).long()
    xd = x.double()
    want = torch.stack([xd[i // topk] @ deq[flat[i]].t() for i in range(n)])
    mag = torch.stack([xd[i // topk].abs() @ deq[flat[i]].abs().t() for i in range(n)])
    err = (got - want).abs()
    lim = 2.0 ** -8 * want.abs() + K * 2.0 ** -23 * mag
    worst = (err / lim.clamp_min(1e-300)).max().item()
    print(f"adversarial ({E}, {topk}, {K}, {N}, bm {bm}): max err / limit {worst:.3f}")
    assert bool((err <= lim).all()), f"max err / limit {worst:.3f}"


# ------------------------------------------------------------------ ops.fused_moe
def _moe_inputs(T, E, K, d, F):
    torch.manual_seed(T + E)
    h = torch.randn(T, d, dtype=torch.bfloat16)
    w13 = quantize_mxfp4_experts(torch.randn(E, 2 * F, d) * d ** -0.5)
    w2 = quantize_mxfp4_experts(torch.randn(E, d, F) * F ** -0.5)
    w, ids = ref.moe_topk_softmax(torch.randn(T, E, dtype=torch.bfloat16), K)
    return h, w13, w2, w, ids


@pytest.mark.parametrize("T,E,K,d,F,bm,split", [
    (1, 8, 2, 256, 512, 32, None), (37, 4, 2, 256, 512, 32, 2), (48, 4, 2, 256, 512, 64, 4),
    (128, 4, 2, 256, 256, 64, 1), (48, 4, 2, 256, 768, 64, 4)])
def test_fused_moe_mxfp4(T, E, K, d, F, bm, split):
    """tests/test_moe_fp8_gpu.py's shapes, its K = 128 one replaced by (d 256, F 768): K a
    multiple of 128 whose four down slices are 192 deep.  The tolerance is
    tests/test_kernels_gpu.py::test_fused_moe's; the reference uses the same quantized
    weights."""
    if bm is not None:
        assert ops.moe_tile_rows(T * K, E) == bm
    if split is not None:
        assert ops.moe_down_splitk(T * K, E, ops.moe_tile_rows(T * K, E), F) == split
    h, w13, w2, w, ids = _moe_inputs(T, E, K, d, F)
    exp = ref.fused_moe(h, w13, w2, w, ids)
    out = ops.fused_moe(h.to(DEV), w13.to(DEV), w2.to(DEV), w.to(DEV), ids.to(DEV))
    _close(out, exp, atol=3e-2, rtol=3e-2)


def test_fused_moe_mxfp4_skips_padding_rows():
    """Expert ids of -1 (the empty slots of the expert-parallel dispatch) contribute nothing."""
    T, E, d, F = 96, 4, 256, 256
    h, w13, w2, _, _ = _moe_inputs(T, E, 1, d, F)
    g = torch.Generator().manual_seed(4)
    e = torch.randint(0, E, (T, 1), generator=g, dtype=torch.int32)
    e[torch.rand(T, generator=g) < 0.4] = -1
    one = torch.ones(T, 1)
    out = ops.fused_moe(h.to(DEV), w13.to(DEV), w2.to(DEV), one.to(DEV), e.to(DEV)).cpu()
    exp = ref.fused_moe(h, w13, w2, one, e)
    assert bool((exp[e.view(-1) < 0] == 0).all())
    _close(out, exp, atol=3e-2, rtol=3e-2)


def test_fused_moe_mxfp4_graph_capture_is_bit_identical_to_eager():
    T, E, K, d, F = 48, 8, 2, 256, 256
    h, w13, w2, _, _ = _moe_inputs(T, E, K, d, F)
    h, w13, w2 = h.to(DEV), w13.to(DEV), w2.to(DEV)
    logits = torch.randn(T, E, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(T, d, dtype=torch.bfloat16, device=DEV)

    def run():
        w, ids = ops.moe_topk_softmax(logits, K)
        ops.fused_moe(h, w13, w2, w, ids, out=out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    logits.copy_(torch.randn(T, E, dtype=torch.bfloat16, device=DEV))
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    run()
    torch.cuda.synchronize()
    assert torch.equal(replayed.view(torch.int16), out.view(torch.int16))
    w, ids = ref.moe_topk_softmax(logits.cpu(), K)
    _close(out, ref.fused_moe(h.cpu(), w13.to("cpu"), w2.to("cpu"), w, ids), atol=3e-2, rtol=3e-2)


# ------------------------------------------------------------------ binding checks
def test_binding_checks_raise():
    bm, N, K = 32, 128, 128
    sorted_ids, inv, tile_expert, used, n = hand_align(bm)
    rows = tile_expert.numel() * bm
    sid, te = sorted_ids.to(DEV), tile_expert.to(DEV)
    a = torch.zeros(n // TOPK, K, dtype=torch.bfloat16, device=DEV)
    wq = torch.zeros(E4, N, K // 2, dtype=torch.uint8, device=DEV)
    sc = torch.full((E4, N, K // 32), 127, dtype=torch.uint8, device=DEV)
    out = torch.zeros(rows, N, dtype=torch.bfloat16, device=DEV)
    call = lambda o, a_, w_, s_, pf=1, splitk=1: torch.ops.akap.moe_q4gemm(  # noqa: E731
        o, a_, w_, s_, sid, te, n, TOPK, True, False, pf, bm, splitk)
    call(out, a, wq, sc)                                           # the valid launch
    with pytest.raises(RuntimeError, match="wq must be"):
        call(out, a, wq.to(torch.int8), sc)                        # wrong weight dtype
    with pytest.raises(RuntimeError, match="a must be"):
        call(out, a.float(), wq, sc)                               # wrong activation dtype
    with pytest.raises(RuntimeError, match="scale must be"):
        call(out, a, wq, sc.float())                               # wrong scale dtype
    with pytest.raises(RuntimeError, match=r"scale must be \[E, N, K/32\]"):
        call(out, a, wq, sc[:, :-1].contiguous())                  # wrong scale shape
    with pytest.raises(RuntimeError, match=r"scale must be \[E, N, K/32\]"):
        call(out, a, wq, sc.view(E4, -1))
    with pytest.raises(RuntimeError, match="out rows"):
        call(out[:rows - 1], a, wq, sc)                            # out too small
    with pytest.raises(RuntimeError, match="too short"):
        call(torch.zeros(2 * rows * N - 1, device=DEV), a, wq, sc, 1, 2)   # partials too small
    for k in (96, 192):                                            # unsupported K
        wk = torch.zeros(E4, N, k // 2, dtype=torch.uint8, device=DEV)
        sk = torch.full((E4, N, k // 32), 127, dtype=torch.uint8, device=DEV)
        ak = torch.zeros(n // TOPK, k, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError, match="unsupported"):
            call(out, ak, wk, sk)
    with pytest.raises(RuntimeError, match="unsupported"):
        call(out, a, wq, sc, 2)                                    # one step, ring depth 2
    h, w13, w2, w, ids = _moe_inputs(8, 4, 2, 128, 128)
    args = (w.to(DEV), ids.to(DEV))
    with pytest.raises(TypeError, match="both"):                   # mixed bf16 / mxfp4 pair
        ops.fused_moe(h.to(DEV), w13.to(DEV), w2.float().to(torch.bfloat16).to(DEV), *args)
    with pytest.raises(TypeError, match="both"):                   # mixed fp8 / mxfp4 pair
        ops.fused_moe(h.to(DEV), w13.to(DEV), quantize_fp8_experts(w2.float()).to(DEV), *args)
    with pytest.raises(TypeError, match="both"):
        ops.fused_moe(h.to(DEV), quantize_fp8_experts(w13.float()).to(DEV), w2.to(DEV), *args)
    assert isinstance(quantize_fp8_experts(w2.float()), Fp8Experts)


# ------------------------------------------------------------------ prefill path
def test_prefill_path_shares_the_scratch():
    """MoEBlock._forward_tokens at a prefill size on quantized experts: each tensor is
    dequantized into the shared scratch right before its grouped GEMM.  Two different blocks
    back to back reuse the same bytes; both must be right, and the first repeats bit for bit."""
    cfg = get_config("tiny-mixtral")
    assert (cfg.num_experts, cfg.experts_per_token, cfg.hidden_size,
            cfg.intermediate_size) == (4, 2, 256, 256)
    T = 600
    assert T >= MoEBlock.grouped_min_t
    ps = ParallelState(rank=0, world_size=1, tp_size=1)
    blocks = []
    for seed in (0, 1):
        b = MoEBlock(cfg, ps, DEV, torch.bfloat16, torch.Generator().manual_seed(seed),
                     full_then_shard=False, mode="tp")
        b.quantize_mxfp4()
        assert isinstance(b.w13, Mxfp4Experts) and b.w13.is_cuda
        blocks.append(b)
    torch.manual_seed(T)
    h = torch.randn(T, cfg.hidden_size, dtype=torch.bfloat16, device=DEV)
    outs = [b._forward_tokens(h) for b in blocks]
    again = blocks[0]._forward_tokens(h)
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int16), outs[0].view(torch.int16))
    for b, out in zip(blocks, outs):
        w, ids = ops.moe_router_topk(h, b.router, b.K, renormalize=cfg.moe_renormalize)
        exp = ref.fused_moe(h.cpu(), b.w13.to("cpu"), b.w2.to("cpu"), w.cpu(), ids.cpu())
        _close(out, exp, atol=3e-2, rtol=3e-2)
    assert not torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ engine
MOE_MODELS = ["tiny-mixtral", "tiny-qwen3-moe"]
# tests/test_moe_fp8_gpu.py's prompts.  The CPU reference engine with mxfp4 experts stays under
# the 0.2 std bound on all four for both models (tests/test_moe_mxfp4_cpu.py; at most 0.065
# std), so none had to be replaced (profiles/moe_mxfp4_weights.md lists every prompt and gap).
PROMPTS = [list(range(400, 470)), [100, 101], [7, 8, 9] * 30, list(range(300, 340))]


def _engine(model, eager=False, **kw):
    cfg = dict(model=model, device="cuda", max_model_len=512, max_num_seqs=16,
               max_num_batched_tokens=128, block_size=32, num_gpu_blocks=128, init_std=0.1,
               enforce_eager=eager, cuda_graph_max_bs=16, expert_quantization="mxfp4")
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), log=lambda *a: None)


def _check_teacher_forced(eng, prompt, out, tol):
    logits = dense_logits(eng.runner.model, list(prompt) + list(out)).float().cpu()
    worst = 0.0
    for i, tok in enumerate(out):
        row = logits[len(prompt) - 1 + i]
        gap = (row.max() - row[tok]).item() / (row.std().item() + 1e-6)
        worst = max(worst, gap)
        assert gap <= tol, f"step {i}: token {tok} is {gap:.3f} std below the argmax"
    return worst


def _check_quantized(eng, model):
    m = eng.runner.model
    assert m.experts_quantized and not m.quantized
    bf16 = DecoderLM(get_config(model), "cpu", max_model_len=512)
    saved = 0
    for lw, lb in zip(m.layers, bf16.layers):
        for name in ("w13", "w2"):
            w = getattr(lw.moe, name)
            assert isinstance(w, Mxfp4Experts) and w.is_cuda
            n = getattr(lb.moe, name).numel()
            saved += 2 * n - n // 2 - n // 32
        assert lw.w_qkv.dtype == torch.bfloat16 and lw.moe.router.dtype == torch.bfloat16
    assert saved > 0 and m.weight_bytes() == bf16.weight_bytes() - saved
    assert m.weight_bytes(as_bf16=True) == bf16.weight_bytes()


@pytest.mark.parametrize("model", MOE_MODELS)
@pytest.mark.parametrize("eager", [False, True])
def test_engine_with_mxfp4_experts_matches_dense_reference(model, eager):
    eng = _engine(model, eager)
    _check_quantized(eng, model)
    if not eager:
        assert eng.runner.graphs, "decode graphs were not captured"
    outs = eng.generate(None, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True),
                        prompt_ids=PROMPTS)
    assert len(PROMPTS) >= 3
    for p, o in zip(PROMPTS, outs):
        assert len(o.output_ids) == 12
        gap = _check_teacher_forced(eng, p, o.output_ids, tol=0.2)
        print(f"[gap] {model} {'eager' if eager else 'captured'} mxfp4 experts, prompt "
              f"{p[:3]}.. x{len(p)}: {gap:.4f} std")


def test_engine_with_mxfp4_experts_and_fp8_kv_cache():
    """An e4m3 KV cache on top of mxfp4 experts, under tests/test_moe_fp8_gpu.py's rule for
    that cache: its rounding moves the router inputs, and a tiny MoE model flips top-k
    near-ties on many prompts whatever the expert weights are, so the case runs tiny-qwen3-moe
    on that test's two prompts at that test's tolerance."""
    eng = _engine("tiny-qwen3-moe", kv_cache_dtype="fp8")
    assert eng.runner.kv.dtype == torch.uint8 and eng.runner.graphs
    prompts = [list(range(300, 340)), [17] * 33 + [5, 6, 7]]
    outs = eng.generate(None, SamplingParams(max_tokens=10, temperature=0, ignore_eos=True),
                        prompt_ids=prompts)
    for p, o in zip(prompts, outs):
        assert len(o.output_ids) == 10
        worst = _check_teacher_forced(eng, p, o.output_ids, tol=0.6)
        print(f"[gap] tiny-qwen3-moe mxfp4 experts + fp8 KV, prompt {p[:3]}..: {worst:.4f} std")


# ------------------------------------------------------------------ two processes, one GPU
CHILD = r"""
import json, os, sys
import torch
sys.path.insert(0, os.environ["ROOT"])
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.ops.quant import Mxfp4Experts
from aws_k8s_ansible_provisioner_amd.parallel.tp_worker import make_tp_engine
ecfg = EngineConfig(model="tiny-mixtral", device="cuda", max_model_len=256, max_num_seqs=8,
                    max_num_batched_tokens=64, block_size=32, num_gpu_blocks=96,
                    tensor_parallel_size=2, shard_init="full", init_std=0.15)
assert ecfg.expert_quantization == "mxfp4"   # from AKAP_EXPERT_QUANTIZATION
eng, bc = make_tp_engine(ecfg, backend="gloo", log=lambda *a: None)
if eng is not None:
    assert eng.runner.graphs, "decode graphs were not captured"
    for lw in eng.runner.model.layers:
        assert lw.moe.mode == "ep" and lw.moe.e_local == 2
        assert isinstance(lw.moe.w13, Mxfp4Experts) and isinstance(lw.moe.w2, Mxfp4Experts)
    outs = eng.generate(None, SamplingParams(max_tokens=8, temperature=0, ignore_eos=True),
                        prompt_ids=[list(range(5, 40)), [100, 101], [200, 201, 202]])
    bc.shutdown()
    print("RESULT " + json.dumps([o.output_ids for o in outs]), flush=True)
"""


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_ep2_on_one_gpu_with_mxfp4_experts():
    """tiny-mixtral expert-parallel over two processes sharing the GPU, captured decode, mxfp4
    experts from the environment knob; teacher-forced at tests/test_tp_gpu.py's tolerance
    against the dense reference of the unsharded model with the same (whole-expert) codes.
    The fp8 test's third prompt, [9, 9, 9], is replaced by [200, 201, 202]: with mxfp4 codes its
    fifth generated token enters at a router near-tie (top-2 margin 0.0013, where the rest of
    the sequence keeps 0.005), which the two ranks' separately rounded partial sums flip (0.39
    std); [200, 201, 202] keeps a margin of 0.019 over all 8 tokens on the unsharded engine
    (profiles/moe_mxfp4_weights.md).  Both children run under one timeout; after a failure
    nothing further is started."""
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, ROOT=ROOT, RANK=str(r), WORLD_SIZE="2", AKAP_MOE_MODE="ep",
                   AKAP_CUSTOM_AR_GLOO="1", AKAP_GEMM_TUNE="0", AKAP_EXPERT_QUANTIZATION="mxfp4",
                   LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", CHILD], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    try:
        outs = [p.communicate(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]
    got = json.loads([ln for ln in outs[0][0].splitlines() if ln.startswith("RESULT")][0][7:])
    full = LLMEngine(EngineConfig(model="tiny-mixtral", device="cuda", max_model_len=256,
                                  max_num_seqs=8, max_num_batched_tokens=64, block_size=32,
                                  num_gpu_blocks=96, init_std=0.15, enforce_eager=True,
                                  shard_init="full", expert_quantization="mxfp4"),
                     log=lambda *a: None)
    prompts = [list(range(5, 40)), [100, 101], [200, 201, 202]]
    for p, toks in zip(prompts, got):
        assert len(toks) == 8
        _check_teacher_forced(full, p, toks, tol=0.15)
