"""FP8 expert weights for MoE on the CPU: the Fp8Experts weight type, the reference path of
ops.fused_moe, sharding, the expert_quantization knob, checkpoints and byte accounting."""
import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
from aws_k8s_ansible_provisioner_amd.models.config import get_config
from aws_k8s_ansible_provisioner_amd.models.moe import MoEBlock
from aws_k8s_ansible_provisioner_amd.models.reference_forward import dense_logits
from aws_k8s_ansible_provisioner_amd.models.transformer import DecoderLM
from aws_k8s_ansible_provisioner_amd.ops import reference as ref
from aws_k8s_ansible_provisioner_amd.ops.quant import (Fp8Experts, Fp8Weight, quantize_fp8,
                                                       quantize_fp8_experts)
from aws_k8s_ansible_provisioner_amd.parallel.state import ParallelState

MOE_MODELS = ["tiny-mixtral", "tiny-qwen3-moe"]
GAP_TOL = 0.2  # std: the engine tolerance of tests/test_moe_fp8_gpu.py


def _experts(E=4, N=64, K=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(E, N, K, generator=g) * 0.05


# ------------------------------------------------------------------------------ weight type
def test_construction_checks():
    q = torch.zeros(2, 8, 16, dtype=torch.uint8)
    s = torch.ones(2, 8)
    w = Fp8Experts(q.view(torch.float8_e4m3fn), s)   # float8 is viewed as uint8
    assert w.q.dtype == torch.uint8 and tuple(w.shape) == (2, 8, 16) and w.dim() == 3
    assert w.numel() == 2 * 8 * 16 and not w.is_cuda and w.device.type == "cpu"
    assert isinstance(w.to("cpu"), Fp8Experts)
    with pytest.raises(ValueError):
        Fp8Experts(q[0], s)                                  # 2-D codes
    with pytest.raises(ValueError):
        Fp8Experts(q.to(torch.int32), s)                     # wrong code dtype
    with pytest.raises(ValueError):
        Fp8Experts(q, torch.ones(2, 9))                      # wrong scale shape
    with pytest.raises(ValueError):
        Fp8Experts(q, s.double())                            # wrong scale dtype
    with pytest.raises(ValueError):
        quantize_fp8_experts(torch.zeros(8, 16))


def test_quantize_equals_per_expert_rule_and_nbytes():
    w = _experts()
    w[1, 3] = 0                                              # an all-zero channel: scale 1
    q = quantize_fp8_experts(w)
    E, N, K = w.shape
    assert q.nbytes == E * N * K + 4 * E * N
    assert not bool(((q.q & 0x7F) == 0x7F).any()), "a NaN code"
    for e in range(E):
        one = quantize_fp8(w[e])
        assert isinstance(q[e], Fp8Weight)
        assert torch.equal(q[e].q, one.q) and torch.equal(q[e].scale, one.scale)
        assert torch.equal(q[e].float(), one.float())
    assert torch.equal(q.float(), torch.stack([q[e].float() for e in range(E)]))
    assert float(q.scale[1, 3]) == 1.0


def test_indexing_and_slicing():
    q = quantize_fp8_experts(_experts(E=6, N=16, K=32))
    ep = q[2:4]                                              # expert slice (EP)
    assert isinstance(ep, Fp8Experts) and tuple(ep.shape) == (2, 16, 32)
    assert torch.equal(ep.q, q.q[2:4]) and torch.equal(ep.scale, q.scale[2:4])
    tp = q[:, :, 16:32]                                      # column slice (TP shard of w2)
    assert tuple(tp.shape) == (6, 16, 16) and torch.equal(tp.scale, q.scale)
    assert torch.equal(tp.float(), q.float()[:, :, 16:32])
    ch = q[:, 4:8]                                           # channel slice
    assert torch.equal(ch.q, q.q[:, 4:8]) and torch.equal(ch.scale, q.scale[:, 4:8])
    assert torch.equal(q[5][:, 8:16].float(), q.float()[5, :, 8:16])
    flat = q.flat()
    assert tuple(flat.shape) == (96, 32) and torch.equal(flat.float(), q.float().view(96, 32))
    with pytest.raises(TypeError):
        q[0, 1]
    with pytest.raises(TypeError):
        q[torch.tensor([0, 1])]


# ------------------------------------------------------------------------------ fused_moe
@pytest.mark.parametrize("T,E,K,d,F", [(1, 8, 2, 64, 128), (37, 4, 2, 64, 128), (20, 16, 4, 128, 192)])
def test_fused_moe_equals_reference_on_dequantized_weights(T, E, K, d, F):
    g = torch.Generator().manual_seed(T + E)
    h = torch.randn(T, d, generator=g).to(torch.bfloat16)
    w13 = quantize_fp8_experts(torch.randn(E, 2 * F, d, generator=g) * d ** -0.5)
    w2 = quantize_fp8_experts(torch.randn(E, d, F, generator=g) * F ** -0.5)
    w, ids = ref.moe_topk_softmax(torch.randn(T, E, generator=g), K)
    ids[0, 0] = -1                                           # an EP padding slot
    got = ops.fused_moe(h, w13, w2, w, ids)
    want = ref.fused_moe(h, w13.float(), w2.float(), w, ids)  # exactly dequantized fp32
    assert torch.equal(got, want)
    with pytest.raises(TypeError, match="both"):
        ops.fused_moe(h, w13, w2.float().to(torch.bfloat16), w, ids)
    with pytest.raises(TypeError, match="both"):
        ops.fused_moe(h, w13.float().to(torch.bfloat16), w2, w, ids)


# ------------------------------------------------------------------------------ sharding
def _block(cfg, rank, world, tp, mode):
    ps = ParallelState(rank=rank, world_size=world, tp_size=tp, tp_rank=rank % tp)
    blk = MoEBlock(cfg, ps, "cpu", torch.bfloat16, torch.Generator().manual_seed(0),
                   full_then_shard=True, mode=mode)
    blk.quantize_fp8()
    assert blk.quantized and isinstance(blk.w13, Fp8Experts) and isinstance(blk.w2, Fp8Experts)
    return blk


def _routed(blk, h, w, ids):
    """The block's experts on a given routing (ids global; this rank's experts only)."""
    local = ids - blk.e0
    local = torch.where((local >= 0) & (local < blk.e_local), local, torch.full_like(local, -1))
    return ops.fused_moe(h, blk.w13, blk.w2, w, local.to(torch.int32)).float()


@pytest.mark.parametrize("model", MOE_MODELS)
def test_sharded_quantized_blocks_match_the_unsharded_one(model):
    """tp = 2 (F shards, summed) and ep = 2 (expert halves, routed) quantized blocks against
    the unsharded quantized block.  The shards are quantized after sharding: a w13 shard has
    the same channels (same codes and scales); a w2 F shard has its own per-channel absmax,
    so it agrees within the quantization step, inside the bf16 tolerance of the CPU MoE tests
    (tests/test_ops_cpu.py)."""
    cfg = get_config(model)
    full = _block(cfg, 0, 1, 1, "tp")
    torch.manual_seed(1)
    T = 24
    h = torch.randn(T, cfg.hidden_size).to(torch.bfloat16)
    w, ids = ops.moe_router_topk(h, full.router, full.K, renormalize=cfg.moe_renormalize)
    want = _routed(full, h, w, ids)
    tp = [_block(cfg, r, 2, 2, "tp") for r in range(2)]
    F2 = cfg.intermediate_size // 2
    for r, b in enumerate(tp):
        assert tuple(b.w13.shape) == (cfg.num_experts, 2 * F2, cfg.hidden_size)
        assert tuple(b.w2.shape) == (cfg.num_experts, cfg.hidden_size, F2)
        # gate rows of the shard are the full block's gate rows r*F2 .. (r+1)*F2, bit for bit
        assert torch.equal(b.w13.q[:, :F2], full.w13.q[:, r * F2:(r + 1) * F2])
        assert torch.equal(b.w13.scale[:, :F2], full.w13.scale[:, r * F2:(r + 1) * F2])
    got_tp = sum(_routed(b, h, w, ids) for b in tp)
    assert torch.allclose(got_tp, want, atol=3e-2, rtol=3e-2)
    ep = [_block(cfg, r, 2, 1, "ep") for r in range(2)]
    for r, b in enumerate(ep):
        el = cfg.num_experts // 2
        assert b.e_local == el and torch.equal(b.w2.q, full.w2.q[r * el:(r + 1) * el])
    got_ep = sum(_routed(b, h, w, ids) for b in ep)
    assert torch.allclose(got_ep, want, atol=3e-2, rtol=3e-2)


# ------------------------------------------------------------------------------ config
def test_config_precedence(monkeypatch):
    monkeypatch.delenv("AKAP_EXPERT_QUANTIZATION", raising=False)
    assert EngineConfig().expert_quantization is None
    monkeypatch.setenv("AKAP_EXPERT_QUANTIZATION", "fp8")
    assert EngineConfig().expert_quantization == "fp8"
    assert EngineConfig(expert_quantization="none").expert_quantization == "none"  # field wins
    assert EngineConfig().quantization is None            # the dense knob is untouched
    monkeypatch.setenv("AKAP_EXPERT_QUANTIZATION", "int4")
    with pytest.raises(ValueError, match="expert_quantization"):
        EngineConfig()
    with pytest.raises(ValueError, match="expert_quantization"):
        EngineConfig(expert_quantization="mxfp4")


def _engine(model, **kw):
    cfg = dict(model=model, device="cpu", max_model_len=256, max_num_seqs=8,
               max_num_batched_tokens=64, block_size=32, num_gpu_blocks=64, init_std=0.1)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), log=lambda *a: None)


def test_knob_errors(monkeypatch):
    monkeypatch.delenv("AKAP_EXPERT_QUANTIZATION", raising=False)
    with pytest.raises(ValueError, match="no experts"):
        _engine("tiny-llama", expert_quantization="fp8")
    with pytest.raises(ValueError, match="no experts"):
        DecoderLM(get_config("tiny-qwen3"), "cpu", max_model_len=256).quantize_experts_fp8()
    with pytest.raises(ValueError, match="MoE"):          # --quantization stays dense-only
        _engine("tiny-mixtral", quantization="fp8", expert_quantization="fp8")
    with pytest.raises(ValueError, match="expert-quantization"):
        _engine("tiny-mixtral", quantization="fp8")
    with pytest.raises(ValueError, match="unknown expert quantization"):
        DecoderLM(get_config("tiny-mixtral"), "cpu", max_model_len=256, expert_quantization="int8")
    # "none" on a dense model is not a set value
    DecoderLM(get_config("tiny-qwen3"), "cpu", max_model_len=256, expert_quantization="none")
    from aws_k8s_ansible_provisioner_amd.server.api_server import (make_parser,
                                                                   engine_config_from_args)
    a = make_parser().parse_args(["--model", "tiny-mixtral", "--expert-quantization", "fp8"])
    assert engine_config_from_args(a).expert_quantization == "fp8"


# ------------------------------------------------------------------------------ checkpoints
def _quantized_model(model, seed=3):
    m = DecoderLM(get_config(model), "cpu", seed=seed, max_model_len=256, init_std=0.1)
    m.quantize_experts_fp8()
    assert m.experts_quantized and not m.quantized and m.quantization is None
    return m


def _fresh(model, eq="fp8"):
    return DecoderLM(get_config(model), "cpu", seed=99, max_model_len=256, expert_quantization=eq)


def _same_experts(a, b):
    for la, lb in zip(a.layers, b.layers):
        for n in ("w13", "w2"):
            wa, wb = getattr(la.moe, n), getattr(lb.moe, n)
            assert isinstance(wb, Fp8Experts)
            assert torch.equal(wa.q, wb.q) and torch.equal(wa.scale, wb.scale), n
        assert torch.equal(la.moe.router, lb.moe.router)
        assert torch.equal(la.w_qkv, lb.w_qkv) and torch.equal(la.w_o, lb.w_o)


def _expert_weight_keys(sd):
    return [k for k in sd if ".experts." in k and k.endswith(".weight")]


@pytest.mark.parametrize("model", MOE_MODELS)
def test_checkpoint_round_trip_per_channel(model):
    src = _quantized_model(model)
    sd = src.hf_state_dict()
    keys = _expert_weight_keys(sd)
    assert keys and all(sd[k].dtype == torch.float8_e4m3fn for k in keys)
    assert all(tuple(sd[k[:-7] + ".weight_scale"].shape) == (sd[k].shape[0], 1) for k in keys)
    assert sd["model.layers.0.self_attn.q_proj.weight"].dtype == torch.bfloat16
    dst = _fresh(model)
    dst.load_state_dict(sd)
    assert dst.experts_quantized and not dst.quantized
    _same_experts(src, dst)
    sd2 = dst.hf_state_dict()
    assert sd.keys() == sd2.keys()
    for k in sd:
        assert torch.equal(sd[k].view(torch.uint8) if sd[k].dtype == torch.float8_e4m3fn else sd[k],
                           sd2[k].view(torch.uint8) if sd2[k].dtype == torch.float8_e4m3fn else sd2[k]), k
    # [N] scales load the same
    flat = {k: (v.reshape(-1) if k.endswith(".weight_scale") else v) for k, v in sd.items()}
    dst2 = _fresh(model)
    dst2.load_state_dict(flat)
    _same_experts(src, dst2)
    # without the knob the fp8 checkpoint is refused as before
    with pytest.raises(ValueError, match="quantization"):
        _fresh(model, eq=None).load_state_dict(sd)


@pytest.mark.parametrize("model", MOE_MODELS)
def test_checkpoint_per_tensor_scales(model):
    bf = DecoderLM(get_config(model), "cpu", seed=4, max_model_len=256, init_std=0.1)
    sd = bf.hf_state_dict()
    for k in _expert_weight_keys(sd):
        w = sd[k].float()
        s = w.abs().max() / 448.0
        sd[k] = (w / s).to(torch.float8_e4m3fn)
        sd[k[:-7] + ".weight_scale"] = s.reshape(())        # scalar, broadcast over channels
    dst = _fresh(model)
    dst.load_state_dict(sd)
    Fn = dst.cfg.intermediate_size
    for i, lw in enumerate(dst.layers):
        names = lw.moe._hf_names(f"model.layers.{i}.", 1)
        assert torch.equal(lw.moe.w13.q[1, :Fn], sd[names[1]].view(torch.uint8))   # gate codes
        assert torch.equal(lw.moe.w13.q[1, Fn:], sd[names[2]].view(torch.uint8))   # up codes
        assert torch.equal(lw.moe.w2.q[1], sd[names[3]].view(torch.uint8))
        assert bool((lw.moe.w13.scale[1, :Fn] == sd[names[1][:-7] + ".weight_scale"]).all())
        assert bool((lw.moe.w13.scale[1, Fn:] == sd[names[2][:-7] + ".weight_scale"]).all())


@pytest.mark.parametrize("model", MOE_MODELS)
def test_checkpoint_block_scaled_and_plain_sources(model):
    bf = DecoderLM(get_config(model), "cpu", seed=5, max_model_len=256, init_std=0.1)
    plain = bf.hf_state_dict()
    # a plain bf16 source is quantized at load: the same as quantizing the loaded model
    want = DecoderLM(get_config(model), "cpu", seed=5, max_model_len=256, init_std=0.1)
    want.quantize_experts_fp8()
    dst = _fresh(model)
    dst.load_state_dict(plain)
    _same_experts(want, dst)
    # 128 x 128 block-scaled source: dequantized and re-quantized per channel
    blk = dict(plain)
    deq = {}
    for k in _expert_weight_keys(plain):
        w = plain[k].float()
        N, K = w.shape
        nb, kb = -(-N // 128), -(-K // 128)
        s = torch.empty(nb, kb)
        q = torch.empty(N, K, dtype=torch.float8_e4m3fn)
        full = torch.empty(N, K)
        for i in range(nb):
            for j in range(kb):
                t = w[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128]
                s[i, j] = t.abs().max() / 448.0
                q[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128] = (t / s[i, j]).to(torch.float8_e4m3fn)
                full[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128] = (
                    q[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128].float() * s[i, j])
        blk[k] = q
        blk[k[:-7] + ".weight_scale_inv"] = s
        deq[k] = full
    dst = _fresh(model)
    dst.load_state_dict(blk)
    Fn = dst.cfg.intermediate_size
    names = dst.layers[1].moe._hf_names("model.layers.1.", 2)
    w13 = quantize_fp8(torch.cat([deq[names[1]], deq[names[2]]], 0))
    assert torch.equal(dst.layers[1].moe.w13[2].q, w13.q)
    assert torch.equal(dst.layers[1].moe.w13[2].scale, w13.scale)
    w2 = quantize_fp8(deq[names[3]])
    assert torch.equal(dst.layers[1].moe.w2[2].q, w2.q)
    assert tuple(dst.layers[1].moe.w13.shape) == (dst.cfg.num_experts, 2 * Fn, dst.cfg.hidden_size)


@pytest.mark.parametrize("model", MOE_MODELS)
def test_checkpoint_with_fp8_attention_projections(model, capsys):
    src = _quantized_model(model)
    sd = src.hf_state_dict()
    want = {}
    for i in range(src.cfg.num_layers):
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            k = f"model.layers.{i}.self_attn.{n}"
            f = quantize_fp8(sd[k + ".weight"])
            sd[k + ".weight"] = f.q.view(torch.float8_e4m3fn)
            sd[k + ".weight_scale"] = f.scale.reshape(-1, 1)
            want[k] = f.float().to(torch.bfloat16)
    dst = _fresh(model)
    dst.load_state_dict(sd)
    assert capsys.readouterr().out.count("dequantized to bf16") == 1   # one log line
    for la, lb in zip(src.layers, dst.layers):
        assert torch.equal(la.moe.w13.q, lb.moe.w13.q) and torch.equal(la.moe.w2.scale, lb.moe.w2.scale)
    q = src.hq * src.D
    assert dst.layers[0].w_qkv.dtype == torch.bfloat16
    assert torch.equal(dst.layers[0].w_qkv[:q], want["model.layers.0.self_attn.q_proj"])
    assert torch.equal(dst.layers[1].w_o, want["model.layers.1.self_attn.o_proj"])
    # without the knob: refused, as today
    with pytest.raises(ValueError, match="--quantization fp8"):
        _fresh(model, eq=None).load_state_dict(sd)


# ------------------------------------------------------------------------------ bytes
@pytest.mark.parametrize("model", MOE_MODELS)
def test_weight_bytes(model):
    bf = DecoderLM(get_config(model), "cpu", max_model_len=256)
    total = bf.weight_bytes()
    numel = [lw.moe.numel() for lw in bf.layers]
    saved = sum(w.numel() - 4 * w.shape[0] * w.shape[1]
                for lw in bf.layers for w in (lw.moe.w13, lw.moe.w2))
    bf.quantize_experts_fp8()
    assert saved > 0 and bf.weight_bytes() == total - saved
    assert bf.weight_bytes(as_bf16=True) == total
    assert [lw.moe.numel() for lw in bf.layers] == numel     # numel keeps its meaning


# ------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("model", MOE_MODELS)
def test_cpu_engine_with_fp8_experts_matches_dense_reference(model):
    eng = _engine(model, expert_quantization="fp8")
    m = eng.runner.model
    assert m.experts_quantized and not m.quantized
    assert all(isinstance(lw.moe.w13, Fp8Experts) and isinstance(lw.moe.w2, Fp8Experts)
               for lw in m.layers)
    # the fp8 dense engine test's prompts, but for its first (range(5, 90)): on tiny-mixtral
    # that one meets a router near-tie on which this CPU reference path itself sits 0.214 std
    # below the dense argmax, so it cannot carry a 0.2 bound (profiles/moe_fp8_weights.md)
    prompts = [list(range(400, 470)), [100, 101], [7, 8, 9] * 30, list(range(300, 340))]
    outs = eng.generate(None, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True),
                        prompt_ids=prompts)
    worst = 0.0
    for p, o in zip(prompts, outs):
        assert len(o.output_ids) == 12
        logits = dense_logits(m, list(p) + list(o.output_ids)).float()
        for i, tok in enumerate(o.output_ids):
            row = logits[len(p) - 1 + i]
            worst = max(worst, (row.max() - row[tok]).item() / (row.std().item() + 1e-6))
    print(f"[gap] {model} cpu reference path, fp8 experts: worst {worst:.4f} std")
    assert worst <= GAP_TOL
