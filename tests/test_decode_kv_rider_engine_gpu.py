"""Engine with and without the K/V rider workgroups (AKAP_DECODE_KV_RIDER): a tiny random
model, 8 requests, 12 generated tokens.  After the first decode step the KV caches and V tails
are byte-equal, and the two leading ids of every request match (the criterion
`bench.py --dump-outputs` documents).  Both the hipGraph and the eager decode path, with a fixed
fused-chain plan whose gate|up variant can carry riders."""
import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
from aws_k8s_ansible_provisioner_amd.models import transformer
from aws_k8s_ansible_provisioner_amd.ops import gemm_tuner
from aws_k8s_ansible_provisioner_amd.ops.gemm_variant import Variant

pytestmark = pytest.mark.gpu

PROMPTS = [list(range(5 + i, 5 + i + n)) for i, n in enumerate([9, 2, 15, 8, 1, 7, 12, 16])]


def _run(eager, rider, monkeypatch):
    """-> (caches after the first decode step, output ids, decode steps that carried riders)"""
    monkeypatch.setattr(transformer, "DECODE_KV_RIDER", rider)
    seen = {"decode": 0, "riders": 0}
    dgemm = ops.dgemm

    def counting_dgemm(*a, **kw):  # graph mode: the launches are issued at capture time
        seen["riders"] += kw.get("kv_write") is not None
        return dgemm(*a, **kw)

    monkeypatch.setattr(ops, "dgemm", counting_dgemm)
    eng = LLMEngine(EngineConfig(model="tiny-qwen3", device="cuda", max_model_len=256,
                                 max_num_seqs=16, max_num_batched_tokens=256, block_size=32,
                                 num_gpu_blocks=64, init_std=0.1, enforce_eager=eager,
                                 cuda_graph_max_bs=16, async_decode=False),
                    log=lambda *a: None)
    assert eng.runner.v_tails is not None
    real = eng.runner.execute_decode

    def counted(info):
        seen["decode"] += 1
        return real(info)

    monkeypatch.setattr(eng.runner, "execute_decode", counted)
    sp = SamplingParams(max_tokens=12, temperature=0, ignore_eos=True)
    for i, p in enumerate(PROMPTS):
        eng.add_request(str(i), None, sp, prompt_ids=p)
    got, snap = {}, None
    for _ in range(200):
        for o in eng.step():
            if o.finished:
                got[o.req_id] = list(o.output_ids)
        if snap is None and seen["decode"] >= 1:
            torch.cuda.synchronize()
            snap = ([s.clone() for s in eng.runner.kv_segs], eng.runner._tail.clone())
        if len(got) == len(PROMPTS):
            break
    monkeypatch.setattr(ops, "dgemm", dgemm)
    assert len(got) == len(PROMPTS) and snap is not None
    return snap, got, seen["riders"]


@pytest.mark.parametrize("eager,gate_up", [(False, Variant(bn=128, ns=6)), (True, Variant(pf=2))],
                         ids=["graph-g128d", "eager-p2"])
def test_engine_rider_on_and_off_agree(eager, gate_up, monkeypatch):
    # a fixed plan for every batch size (tiny-qwen3: K = 256 / 512), no tuning
    monkeypatch.setenv("AKAP_GEMM_TUNE", "0")
    saved = dict(gemm_tuner._FUSED)
    plan = {"w_qkv": Variant(pf=2), "w_o": Variant(pf=2), "w_gate_up": gate_up,
            "w_down": Variant(pf=2)}
    try:
        for m in range(1, 17):
            gemm_tuner._FUSED[m] = dict(plan)
        (kv0, tail0), out0, riders0 = _run(eager, False, monkeypatch)
        (kv1, tail1), out1, riders1 = _run(eager, True, monkeypatch)
    finally:
        gemm_tuner._FUSED.clear()
        gemm_tuner._FUSED.update(saved)
    assert riders0 == 0 and riders1 > 0  # the knob switches the path, and the path ran
    for a, b in zip(kv0, kv1):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(tail0.view(torch.int16), tail1.view(torch.int16))
    for rid in out0:
        assert len(out1[rid]) == 12 and out0[rid][:2] == out1[rid][:2], rid
