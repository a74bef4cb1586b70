"""K/V rider workgroups of the gate|up decode GEMM (csrc/kernels/kv_write.h), the parts that
need no GPU: the host-side predicate kv_rider_blocks (host_contract.h) against hand-computed
capacities, and the CPU path of ops.dgemm(kv_write=...) / paged_attention_decode_fused(
write_kv=False) against ops/reference.py."""
import math

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.ops import reference as ref
from aws_k8s_ansible_provisioner_amd.ops.gemm_variant import Variant

CUS = 256          # MI355X
N_GATE_UP = 6144   # Qwen3-0.6B gate|up rows (2 x 3072), Hkv = 8
HKV = 8

# variant -> (workgroups per CU, tile rows, tile cols).  capacity = 256 x workgroups per CU;
# tiles = ceil(M / rows) x (6144 / cols); a step of B = M sequences needs ceil(M * 8 * 2 / 16) = M
# passes; riders = min(M, capacity - tiles).  The expected values below are worked by hand:
#   deep g128 (1/CU, 64 x 128): tiles 48, 48, 144, 192 of 256
#   ring / shallow g64 (2/CU, 64 x 64): tiles 96, 96, 288, 384 of 512
#   shallow g128 (2/CU, 64 x 128): tiles 48, 48, 144, 192 of 512
#   g128x128 (1/CU): tiles 48, 48, 96, 96 of 256;  g128x256 (1/CU): tiles 48 of 256
TABLE = [
    (Variant(bn=128, ns=6), {1: 1, 64: 64, 192: 112, 256: 64}),
    (Variant(pf=2), {1: 1, 64: 64, 192: 192, 256: 128}),
    (Variant(pf=4), {1: 1, 64: 64, 192: 192, 256: 128}),
    (Variant(bn=64, ns=0), {1: 1, 64: 64, 192: 192, 256: 128}),
    (Variant(bn=64, ns=8), {1: 1, 64: 64, 192: 0, 256: 0}),  # deep g64: 96 / 288 / 384 of 256
    (Variant(bn=128, ns=0), {1: 1, 64: 64, 192: 192, 256: 256}),
    (Variant(bn=128, ns=4, bm=128), {1: 1, 64: 64, 192: 160, 256: 160}),
    (Variant(bn=128, ns=3, bm=256), {1: 1, 64: 64, 192: 192, 256: 208}),
]


@pytest.mark.parametrize("variant,want", TABLE, ids=[v.name for v, _ in TABLE])
def test_rider_blocks_table(variant, want):
    for M, n in want.items():
        got = ops.kv_rider_blocks(M, N_GATE_UP, variant, M, HKV, cus=CUS)
        assert got == n, (variant.name, M, got, n)


def test_rider_blocks_zero_where_the_riders_are_not_legal():
    deep, ring = Variant(bn=128, ns=6), Variant(pf=2)
    ok = dict(B=256, num_kv_heads=HKV, cus=CUS)
    assert ops.kv_rider_blocks(256, N_GATE_UP, deep, **ok) == 64
    assert ops.kv_rider_blocks(256, N_GATE_UP, deep, epi=ops.EPI_STORE, **ok) == 0
    assert ops.kv_rider_blocks(256, N_GATE_UP, deep, epi=ops.EPI_RESNORM, **ok) == 0
    assert ops.kv_rider_blocks(256, N_GATE_UP, deep, kv_bf16_tail=False, **ok) == 0
    assert ops.kv_rider_blocks(256, N_GATE_UP, deep, tp=2, **ok) == 0
    assert ops.kv_rider_blocks(256, N_GATE_UP, deep, dense=False, **ok) == 0
    assert ops.kv_rider_blocks(256, N_GATE_UP, deep, quantized=True, **ok) == 0
    # more than one K slice, the kgemm family, the probe-only 256 x 256 body
    assert ops.kv_rider_blocks(256, N_GATE_UP, Variant(splitk=2, pf=2, inlaunch=True), **ok) == 0
    assert ops.kv_rider_blocks(256, N_GATE_UP, Variant(km=32), **ok) == 0
    assert ops.kv_rider_blocks(256, N_GATE_UP, Variant(bn=256, bm=256), **ok) == 0
    # the tiles alone fill the resident capacity: 4 x 192 = 768 tiles of 512 slots
    assert ops.kv_rider_blocks(256, 12288, ring, **ok) == 0
    # capacity follows the CU count: 4 x 96 = 384 tiles of 2 x 200 = 400 slots
    assert ops.kv_rider_blocks(256, N_GATE_UP, ring, B=256, num_kv_heads=HKV, cus=200) == 16
    assert ops.kv_rider_blocks(256, N_GATE_UP, ring, B=0, num_kv_heads=HKV, cus=CUS) == 0


def _cpu_case(B=5, hq=4, hkv=2, D=128, BS=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    NB = 2 * B + 1
    kc = (torch.randn(NB, hkv, BS, D, generator=g) * 0.5).bfloat16()
    vc = (torch.randn(NB, hkv, BS // 8, D, 8, generator=g) * 0.5).bfloat16()
    bt = torch.arange(1, 2 * B + 1, dtype=torch.int32).view(B, 2)
    pos = torch.tensor([31, 32, 3, 7, 40][:B], dtype=torch.int64)
    slots = torch.tensor([int(bt[s, int(pos[s]) // BS]) * BS + int(pos[s]) % BS
                          for s in range(B)], dtype=torch.int64)
    slots[1] = -1
    qkv = torch.randn(B, (hq + 2 * hkv) * D, generator=g).bfloat16()
    cs = ref.rope_cos_sin(64, D, 1e6)
    kw = torch.randn(D, generator=g).bfloat16()
    qw = torch.randn(D, generator=g).bfloat16()
    return dict(kc=kc, vc=vc, bt=bt, pos=pos, slots=slots, qkv=qkv, cs=cs, kw=kw, qw=qw, hq=hq,
                hkv=hkv, sl=(pos + 1).int())


@pytest.mark.parametrize("k_norm", [True, False])
def test_cpu_dgemm_kv_write_matches_the_reference_writer(k_norm):
    c = _cpu_case()
    kw = c["kw"] if k_norm else None
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(5, 64, generator=g) * 0.3).bfloat16()
    w = (torch.randn(64, 64, generator=g) * 0.3).bfloat16()
    k_ref, v_ref = c["kc"].clone(), c["vc"].clone()
    ref.qk_norm_rope_cache(c["qkv"], torch.empty(5, c["hq"], 128, dtype=torch.bfloat16), k_ref,
                           v_ref, c["pos"], c["slots"], c["cs"], None, kw, c["hq"], c["hkv"],
                           1e-6, True)
    k_new, v_new = c["kc"].clone(), c["vc"].clone()
    y = ops.dgemm(x, w, epi=ops.EPI_SILU, variant=Variant(bn=128, ns=6),
                  kv_write=ops.KvWrite(c["qkv"], c["pos"], c["slots"], c["cs"], kw, k_new, v_new,
                                       None, None, c["hq"], 1e-6))
    assert torch.equal(k_new, k_ref) and torch.equal(v_new, v_ref)
    assert not torch.equal(k_new, c["kc"]) and not torch.equal(v_new, c["vc"])
    assert torch.equal(y, ops.dgemm(x, w, epi=ops.EPI_SILU, variant=Variant(bn=128, ns=6)))


def test_cpu_attention_without_the_write_leaves_the_caches_alone():
    c = _cpu_case()
    outs = []
    for write_kv in (True, False):
        kc, vc = c["kc"].clone(), c["vc"].clone()
        out = torch.empty(5, c["hq"], 128, dtype=torch.bfloat16)
        ops.paged_attention_decode_fused(out, c["qkv"], kc, vc, c["bt"], c["sl"], c["pos"],
                                         c["slots"], c["cs"], c["qw"], c["kw"],
                                         c["hq"] // c["hkv"], 1 / math.sqrt(128), 1e-6,
                                         write_kv=write_kv)
        outs.append(out)
        assert torch.equal(kc, c["kc"]) != write_kv and torch.equal(vc, c["vc"]) != write_kv
    assert torch.equal(outs[0], outs[1])
