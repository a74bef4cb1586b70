"""The decode step's new-token K/V rows written by rider workgroups of the gate|up GEMM launch
(csrc/kernels/kv_write.h) against the attention kernel's own write.

Two arms from identical inputs and identical pre-filled caches:
  (a) paged_attention_decode_fused writes the K/V (write_kv=True);
  (b) paged_attention_decode_fused(write_kv=False), then the gate|up GEMM with kv_write.
k_cache, v_cache and v_tail must match byte for byte, the attention outputs bit for bit, and the
GEMM output must equal the same GEMM launched without riders.  Tolerance zero: both arms run
the same device functions in the same lane layout.
"""
import math

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.ops import reference as ref
from aws_k8s_ansible_provisioner_amd.ops.gemm_variant import Variant

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
STEPS_ROOM = 12  # cache blocks cover this many tokens past a sequence's first new token

# position of the new token per row.  In-group offsets 7 (group flush), 0, 3, 6; block offsets
# 31 (first row: the flush is also the last group of its block) and 0 (first token of a new
# block); 27 = offset 3 inside the last group of a block.
POSITIONS = [31, 32, 3, 6, 27, 7, 72, 45, 200, 15, 16, 23, 100, 63, 95, 33, 1, 0, 64]

# (name, variant, K): the smallest K each gate|up variant accepts (one 64-deep k-step for the
# LDS rings, pf k-steps for the register ring), N = 64 (one tile, EPI_SILU needs N % 32)
GEMMS = [
    ("gdgemm-deep", Variant(bn=128, ns=6), 64),
    ("gdgemm-shallow", Variant(bn=64, ns=0), 64),
    ("dgemm-pf2", Variant(pf=2), 128),
    ("dgemm-pf4", Variant(pf=4), 256),
]
GEMM_N = 64


class Case:
    """One decode batch: random pre-filled caches and tail, a block table, the new tokens."""

    def __init__(self, positions, hq, hkv, seed, dead=(), BS=32):
        g = torch.Generator().manual_seed(seed)
        self.BS = BS
        B = len(positions)
        self.B, self.hq, self.hkv, self.G = B, hq, hkv, hq // hkv
        nblk = [(p + STEPS_ROOM) // BS + 1 for p in positions]
        NB = sum(nblk) + 1
        perm = (torch.randperm(NB - 1, generator=g) + 1).tolist()  # block 0 stays unused
        self.bt = torch.zeros(B, max(nblk), dtype=torch.int32)
        for s, n in enumerate(nblk):
            self.bt[s, :n] = torch.tensor([perm.pop() for _ in range(n)], dtype=torch.int32)
        self.kc = (torch.randn(NB, hkv, BS, D, generator=g) * 0.5).bfloat16()
        self.vc = (torch.randn(NB, hkv, BS // 8, D, 8, generator=g) * 0.5).bfloat16()
        # tail slots in reverse order, twice as many as rows; every slot pre-filled
        self.tail = (torch.randn(2 * B, hkv, 8, D, generator=g) * 0.5).bfloat16()
        self.tslot = torch.tensor([2 * B - 1 - s for s in range(B)], dtype=torch.int32)
        self.cur = list(positions)
        for s, n in enumerate(positions):  # the context's partial V group sits in the tail
            g0 = n & ~7
            for p in range(g0, n):
                b = int(self.bt[s, p // BS])
                self.tail[int(self.tslot[s]), :, p - g0] = self.vc[b, :, (p % BS) // 8, :, p % 8]
        self.dead = dict(dead)  # row -> "slot" | "tail"
        self.cs = ref.rope_cos_sin(512, D, 1e6).to(DEV)
        self.kw = torch.randn(D, generator=g).bfloat16().to(DEV)
        self.qw = torch.randn(D, generator=g).bfloat16().to(DEV)
        self.gen = g
        self.btg = self.bt.to(DEV)

    def step_inputs(self):
        B, BS = self.B, self.BS
        pos = torch.tensor(self.cur, dtype=torch.int64)
        slots = torch.tensor([int(self.bt[s, self.cur[s] // BS]) * BS + self.cur[s] % BS
                              for s in range(B)], dtype=torch.int64)
        tslot = self.tslot.clone()
        for row, what in self.dead.items():
            if what == "slot":
                slots[row] = -1
            else:
                tslot[row] = -1
        sl = torch.tensor([c + 1 for c in self.cur], dtype=torch.int32)
        qkv = torch.randn(B, (self.hq + 2 * self.hkv) * D, generator=self.gen).bfloat16()
        return pos.to(DEV), slots.to(DEV), tslot.to(DEV), sl.to(DEV), qkv.to(DEV)


def _gemm_operands(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.3).bfloat16().to(DEV)
    w = (torch.randn(GEMM_N, K, generator=g) * 0.3).bfloat16().to(DEV)
    return x, w


def _attend(c, caches, inp, write_kv):
    kc, vc, tail = caches
    pos, slots, tslot, sl, qkv = inp
    out = torch.empty(c.B, c.hq, D, dtype=torch.bfloat16, device=DEV)
    ops.paged_attention_decode_fused(out, qkv, kc, vc, c.btg, sl, pos, slots, c.cs, c.qw, c.kw,
                                     c.G, 1 / math.sqrt(D), 1e-6, num_parts=1, part_size=512,
                                     v_tail=tail, tail_slot=tslot, write_kv=write_kv)
    return out


def _kv_write(c, caches, inp, blocks=0):
    kc, vc, tail = caches
    pos, slots, tslot, _, qkv = inp
    return ops.KvWrite(qkv, pos, slots, c.cs, c.kw, kc, vc, tail, tslot, c.hq, 1e-6, blocks)


def _both_arms(c, A, Bc, variant, x, w, blocks=0):
    """One decode step on both arms; returns the rider GEMM's and the plain GEMM's outputs."""
    inp = c.step_inputs()
    out_a = _attend(c, A, inp, True)
    out_b = _attend(c, Bc, inp, False)
    y_b = ops.dgemm(x, w, epi=ops.EPI_SILU, variant=variant,
                    kv_write=_kv_write(c, Bc, inp, blocks))
    y_0 = ops.dgemm(x, w, epi=ops.EPI_SILU, variant=variant)
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)
    for a, b, name in zip(A, Bc, ("k_cache", "v_cache", "v_tail")):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), name
    assert torch.equal(y_b, y_0)
    return inp


def _device_caches(c):
    return tuple(t.to(DEV) for t in (c.kc, c.vc, c.tail))


@pytest.mark.parametrize("name,variant,K", GEMMS, ids=[g[0] for g in GEMMS])
@pytest.mark.parametrize("heads", [(16, 8), (32, 8), (8, 4)], ids=["16/8", "32/8", "8/4"])
@pytest.mark.parametrize("B", [1, 5, 19])
def test_rider_writes_the_bytes_attention_writes(B, heads, name, variant, K, BS=32):
    """B = 19 with 8/4 heads: 19 * 4 pairs is no multiple of the 8 pairs of a rider pass.  Rows
    1 and 2 (B >= 5) are a slot = -1 row and a tail_slot = -1 row."""
    hq, hkv = heads
    assert ops.kv_rider_blocks(B, GEMM_N, variant, B, hkv) > 0
    dead = {1: "slot", 2: "tail"} if B >= 5 else {}
    c = Case(POSITIONS[:B], hq, hkv, seed=100 * B + hq, dead=dead, BS=BS)
    x, w = _gemm_operands(B, K, seed=B + K)
    A, Bc = _device_caches(c), _device_caches(c)
    before = tuple(t.clone() for t in A)
    _both_arms(c, A, Bc, variant, x, w)
    assert not torch.equal(Bc[0], before[0])  # the riders did write
    if B >= 5:
        assert not torch.equal(Bc[1], before[1])  # row 0 completes a V group
        assert not torch.equal(Bc[2], before[2])


# The same at cache block size 64: the K layout's chunk term, zero for every slot at 32, is
# non-zero for the POSITIONS with p % 64 >= 32 (45, 100, 63, 95, 33), in blocks never block 0.
@pytest.mark.parametrize("name,variant,K", GEMMS, ids=[g[0] for g in GEMMS])
@pytest.mark.parametrize("B", [5, 19])
def test_rider_writes_the_bytes_attention_writes_bs64(B, name, variant, K):
    test_rider_writes_the_bytes_attention_writes(B, (16, 8) if B == 5 else (8, 4), name, variant,
                                                 K, BS=64)


@pytest.mark.parametrize("name,variant,K", [GEMMS[0], GEMMS[2]], ids=[GEMMS[0][0], GEMMS[2][0]])
def test_ten_consecutive_steps_bs64(name, variant, K):
    test_ten_consecutive_steps(name, variant, K, BS=64)


def test_one_rider_loops_over_every_row_bs64():
    test_one_rider_loops_over_every_row(BS=64)


def test_dead_rows_leave_every_byte_untouched():
    """Every row has slot = -1 or tail_slot = -1: the rider launch writes nothing at all."""
    B, hq, hkv = 6, 16, 8
    c = Case(POSITIONS[:B], hq, hkv, seed=5,
             dead={r: ("slot" if r % 2 else "tail") for r in range(B)})
    x, w = _gemm_operands(B, 64, seed=9)
    caches = _device_caches(c)
    before = tuple(t.clone() for t in caches)
    inp = c.step_inputs()
    ops.dgemm(x, w, epi=ops.EPI_SILU, variant=Variant(bn=128, ns=6),
              kv_write=_kv_write(c, caches, inp))
    torch.cuda.synchronize()
    for a, b in zip(caches, before):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("name,variant,K", [GEMMS[0], GEMMS[2]], ids=[GEMMS[0][0], GEMMS[2][0]])
def test_ten_consecutive_steps(name, variant, K, BS=32):
    """Groups complete and restart; a slot = -1 row stays dead throughout.  Compared after
    every step."""
    positions = [1, 5, 8, 13, 31, 200, 30, 26] + ([58] if BS == 64 else [])
    c = Case(positions, 16, 8, seed=11, dead={3: "slot"}, BS=BS)
    x, w = _gemm_operands(len(positions), K, seed=2)
    A, Bc = _device_caches(c), _device_caches(c)
    for _ in range(10):
        _both_arms(c, A, Bc, variant, x, w)
        c.cur = [p + 1 for p in c.cur]


def test_one_rider_loops_over_every_row(BS=32):
    """n_blocks forced to 1: the single rider walks all 19 * 8 * 2 rows."""
    c = Case(POSITIONS, 16, 8, seed=21, dead={1: "slot", 2: "tail"}, BS=BS)
    x, w = _gemm_operands(19, 64, seed=4)
    A, Bc = _device_caches(c), _device_caches(c)
    _both_arms(c, A, Bc, Variant(bn=128, ns=6), x, w, blocks=1)


def test_unsupported_launches_are_refused():
    """A launch that cannot carry riders is an error, never a quiet no-write; and the attention
    kernel takes write_kv=False only with the bf16 V tail."""
    c = Case(POSITIONS[:2], 16, 8, seed=1)
    caches = _device_caches(c)
    inp = c.step_inputs()
    x, w = _gemm_operands(2, 256, seed=1)
    kw = _kv_write(c, caches, inp)
    with pytest.raises(RuntimeError, match="riders"):
        ops.dgemm(x, w, epi=ops.EPI_STORE, variant=Variant(pf=2), kv_write=kw)
    with pytest.raises(RuntimeError, match="riders"):
        ops.dgemm(x, w, epi=ops.EPI_SILU, variant=Variant(splitk=2, pf=2, inlaunch=True),
                  kv_write=kw)
    pos, slots, tslot, sl, qkv = inp
    out = torch.empty(2, 16, D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="write_kv"):
        ops.paged_attention_decode_fused(out, qkv, caches[0], caches[1], c.btg, sl, pos, slots,
                                         c.cs, c.qw, c.kw, 2, 1 / math.sqrt(D), 1e-6,
                                         num_parts=1, part_size=512, write_kv=False)
