"""The paged KV-cache layout of csrc/kernels/host_contract.h, as Python sees it through the
CPU-built `_runtime.contract` module: every (token, dim) of a block-head has its own element,
and the layout ops/reference.py derives on its own (views and permutes) -- the oracle of the GPU
tests -- puts every element where the header says."""
import pytest
import torch

from aws_k8s_ansible_provisioner_amd import _runtime_loader, ops
from aws_k8s_ansible_provisioner_amd.ops import reference as ref

C = _runtime_loader.contract()
D, HKV, NB = 128, 2, 3
BLOCK_SIZES = (32, 64, 96)
# integers <= 128 that e4m3 (3 mantissa bits) and bf16 both hold exactly; none is 0
VALS = [v for v in range(1, 129) if v % (1 << max(0, v.bit_length() - 4)) == 0]


def test_constants():
    assert (C.KV_HEAD_DIM, C.KV_GROUP, C.KV_CHUNK, C.V_TAIL_ROWS) == (128, 8, 32, 8)
    for name in ("KV_HEAD_DIM", "KV_GROUP", "KV_CHUNK", "V_TAIL_ROWS"):
        assert getattr(ops, name) == getattr(C, name)


def test_vals_are_exact_in_both_formats():
    t = torch.tensor(VALS, dtype=torch.float32)
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert torch.equal(t.to(torch.float8_e4m3fn).float(), t)


@pytest.mark.parametrize("BS", BLOCK_SIZES)
def test_offsets_are_a_permutation_of_the_block_head(BS):
    k = sorted(C.k_token_offset(o) + C.k_dim_offset(d) for o in range(BS) for d in range(D))
    v = sorted(C.v_elem_offset(o, d) for o in range(BS) for d in range(D))
    assert k == list(range(BS * D))
    assert v == list(range(BS * D))
    for o in range(BS):
        assert C.v_group_offset(o) == C.v_elem_offset(o & ~7, 0)


@pytest.mark.parametrize("BS", BLOCK_SIZES)
def test_head_bases_tile_the_cache(BS):
    for base in (C.k_head_base, C.v_head_base):
        got = [base(b, HKV, h, BS) for b in range(NB) for h in range(HKV)]
        assert got == [i * BS * D for i in range(NB * HKV)]


def test_v_tail_rows_are_the_contiguous_tensor():
    t = torch.empty(3, HKV, C.V_TAIL_ROWS, D)
    for s in range(3):
        for h in range(HKV):
            for r in range(C.V_TAIL_ROWS):
                assert C.v_tail_row_offset(s, HKV, h, r) == t[s, h, r].storage_offset()


def _val(b, h, o, d):
    return VALS[(b * 7919 + h * 104729 + o * 613 + d * 37) % len(VALS)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.uint8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("BS", BLOCK_SIZES)
def test_reference_writes_where_the_contract_says(BS, dtype):
    k_cache = torch.zeros(NB, HKV, BS, D, dtype=dtype)
    v_cache = torch.zeros(NB, HKV, BS // 8, D, 8, dtype=dtype)
    blocks = (1, 2)
    slots = torch.tensor([b * BS + o for b in blocks for o in range(BS)])
    k = torch.tensor([[[_val(b, h, o, d) for d in range(D)] for h in range(HKV)]
                      for b in blocks for o in range(BS)], dtype=torch.float32)
    v = k.flip(-1).contiguous()  # another value per element than K's
    ref.write_cache(k.to(torch.bfloat16), v.to(torch.bfloat16), k_cache, v_cache, slots)

    want_k = torch.zeros(NB * HKV * BS * D)
    want_v = torch.zeros(NB * HKV * BS * D)
    for t, (b, o) in enumerate((b, o) for b in blocks for o in range(BS)):
        for h in range(HKV):
            kb, vb = C.k_head_base(b, HKV, h, BS), C.v_head_base(b, HKV, h, BS)
            kt = kb + C.k_token_offset(o)
            for d in range(D):
                want_k[kt + C.k_dim_offset(d)] = k[t, h, d]
                want_v[vb + C.v_elem_offset(o, d)] = v[t, h, d]
    # element by element, block 0 (never written) included: it stays zero
    assert torch.equal(ref.from_cache(k_cache).float().flatten(), want_k)
    assert torch.equal(ref.from_cache(v_cache).float().flatten(), want_v)

    K, V = ref.gather_kv(k_cache, v_cache, torch.tensor(blocks, dtype=torch.int32), 2 * BS)
    assert torch.equal(K.float(), k)
    assert torch.equal(V.float(), v)
