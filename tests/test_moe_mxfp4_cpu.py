"""MXFP4 expert weights for MoE on the CPU: the Mxfp4Experts weight type, the reference path of
ops.fused_moe, the kernel's support predicate, sharding, the expert_quantization knob,
checkpoints, byte accounting and the CPU reference engine on the GPU test's prompts."""
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
from aws_k8s_ansible_provisioner_amd.ops.quant import (Mxfp4Experts, Mxfp4Weight,
                                                       dequant_mxfp4_experts, quantize_fp8,
                                                       quantize_fp8_experts, quantize_mxfp4,
                                                       quantize_mxfp4_experts)
from aws_k8s_ansible_provisioner_amd.parallel.state import ParallelState

MOE_MODELS = ["tiny-mixtral", "tiny-qwen3-moe"]
GAP_TOL = 0.2  # std: the engine tolerance of tests/test_moe_mxfp4_gpu.py
# the prompts of tests/test_moe_mxfp4_gpu.py's engine cases: tests/test_moe_fp8_gpu.py's
PROMPTS = [list(range(400, 470)), [100, 101], [7, 8, 9] * 30, list(range(300, 340))]
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def _experts(E=4, N=64, K=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(E, N, K, generator=g) * 0.05


# ------------------------------------------------------------------------------ weight type
def test_construction_checks():
    q = torch.zeros(2, 8, 32, dtype=torch.uint8)
    s = torch.full((2, 8, 2), 127, dtype=torch.uint8)
    w = Mxfp4Experts(q, s)
    assert tuple(w.shape) == (2, 8, 64) and w.dim() == 3 and w.numel() == 2 * 8 * 64
    assert w.nbytes == 2 * 8 * 64 // 2 + 2 * 8 * 64 // 32
    assert not w.is_cuda and w.device.type == "cpu" and isinstance(w.to("cpu"), Mxfp4Experts)
    assert "Mxfp4Experts" in repr(w) and w.dtype is not None
    with pytest.raises(ValueError):
        Mxfp4Experts(q[0], s)                                # 2-D codes
    with pytest.raises(ValueError):
        Mxfp4Experts(q.to(torch.int32), s)                   # wrong code dtype
    with pytest.raises(ValueError):
        Mxfp4Experts(q, s[:, :, :1])                         # wrong scale shape
    with pytest.raises(ValueError):
        Mxfp4Experts(q, s.float())                           # wrong scale dtype
    with pytest.raises(ValueError):
        Mxfp4Experts(q[:, :, :24], s)                        # K = 48 is no multiple of 32
    for bad in (0, 1, 253, 255):
        s2 = s.clone()
        s2[1, 3, 1] = bad
        with pytest.raises(ValueError, match="e8m0"):
            Mxfp4Experts(q, s2)
        assert isinstance(Mxfp4Experts(q, s2, check=False), Mxfp4Experts)   # slices and copies
    for ok in (2, 252):
        s2 = s.clone()
        s2[0, 0, 0] = ok
        Mxfp4Experts(q, s2)
    with pytest.raises(ValueError):
        quantize_mxfp4_experts(torch.zeros(8, 32))
    with pytest.raises(ValueError):
        quantize_mxfp4_experts(torch.zeros(2, 8, 48))


def test_float_is_exact_against_a_table():
    """Every code in both nibble positions, under scale codes 2, 120, 127, 130 and 252."""
    q = torch.arange(256, dtype=torch.uint8).view(1, 16, 16)   # byte b: low nibble b % 16
    q = torch.cat([q, q.flip(2)], 0)
    scodes = torch.tensor([2, 120, 127, 130, 252, 126, 128, 64], dtype=torch.uint8)
    s = scodes.repeat(4).view(2, 16, 1)
    w = Mxfp4Experts(q, s)
    f = w.float()
    assert f.dtype == torch.float32 and tuple(f.shape) == (2, 16, 32)
    for e in range(2):
        for n in range(16):
            unit = 2.0 ** (int(s[e, n, 0]) - 127)
            for j in range(16):
                b = int(q[e, n, j])
                assert float(f[e, n, 2 * j]) == E2M1[b & 15] * unit        # low nibble first
                assert float(f[e, n, 2 * j + 1]) == E2M1[b >> 4] * unit
    assert torch.equal(dequant_mxfp4_experts(w).float(), f)                # all exact in bf16


def test_quantize_equals_per_expert_rule_and_nbytes():
    w = _experts()
    w[1, 3, :32] = 0                                         # an all-zero block: scale code 127
    q = quantize_mxfp4_experts(w)
    E, N, K = w.shape
    assert q.nbytes == E * N * K // 2 + E * N * K // 32
    assert tuple(q.q.shape) == (E, N, K // 2) and tuple(q.scale.shape) == (E, N, K // 32)
    for e in range(E):
        one = quantize_mxfp4(w[e])
        assert isinstance(q[e], Mxfp4Weight)
        assert torch.equal(q[e].q, one.q) and torch.equal(q[e].scale, one.scale)
        assert torch.equal(q[e].float(), one.float())
    assert torch.equal(q.float(), torch.stack([q[e].float() for e in range(E)]))
    assert int(q.scale[1, 3, 0]) == 127
    Mxfp4Experts(q.q, q.scale)                               # the codes pass the range check


def test_indexing_and_slicing():
    q = quantize_mxfp4_experts(_experts(E=6, N=16, K=128))
    ep = q[2:4]                                              # expert slice (EP)
    assert isinstance(ep, Mxfp4Experts) and tuple(ep.shape) == (2, 16, 128)
    assert torch.equal(ep.q, q.q[2:4]) and torch.equal(ep.scale, q.scale[2:4])
    tp = q[:, :, 64:128]                                     # column slice (TP shard of w2)
    assert tuple(tp.shape) == (6, 16, 64) and torch.equal(tp.scale, q.scale[:, :, 2:4])
    assert torch.equal(tp.float(), q.float()[:, :, 64:128])
    ch = q[:, 4:8]                                           # channel slice
    assert torch.equal(ch.q, q.q[:, 4:8]) and torch.equal(ch.scale, q.scale[:, 4:8])
    assert torch.equal(q[5][:, 32:96].float(), q.float()[5, :, 32:96])
    assert torch.equal(q[5, 2:4, 32:64].float(), q.float()[5, 2:4, 32:64])
    flat = q.flat()
    assert isinstance(flat, Mxfp4Weight) and tuple(flat.shape) == (96, 128)
    assert torch.equal(flat.float(), q.float().view(96, 128))
    assert flat.q.data_ptr() == q.q.data_ptr()               # a view
    with pytest.raises(ValueError, match="multiples of 32"):
        q[:, :, 16:64]
    with pytest.raises(ValueError, match="multiples of 32"):
        q[:, :, 0:48]
    with pytest.raises(TypeError):
        q[0, 1]
    with pytest.raises(TypeError):
        q[torch.tensor([0, 1])]
    with pytest.raises(IndexError):
        q[0, :, :, :]


# ------------------------------------------------------------------------------ fused_moe
@pytest.mark.parametrize("T,E,K,d,F", [(1, 8, 2, 64, 128), (37, 4, 2, 64, 128), (20, 16, 4, 128, 192)])
def test_fused_moe_equals_reference_on_dequantized_weights(T, E, K, d, F):
    g = torch.Generator().manual_seed(T + E)
    h = torch.randn(T, d, generator=g).to(torch.bfloat16)
    w13 = quantize_mxfp4_experts(torch.randn(E, 2 * F, d, generator=g) * d ** -0.5)
    w2 = quantize_mxfp4_experts(torch.randn(E, d, F, generator=g) * F ** -0.5)
    w, ids = ref.moe_topk_softmax(torch.randn(T, E, generator=g), K)
    ids[0, 0] = -1                                           # an EP padding slot
    got = ops.fused_moe(h, w13, w2, w, ids)
    assert torch.equal(got, ref.fused_moe(h, w13, w2, w, ids))   # ref.fused_moe works unchanged
    bf13, bf2 = w13.float().to(torch.bfloat16), w2.float().to(torch.bfloat16)
    assert torch.equal(bf13.float(), w13.float()), "dequantized values are exact in bf16"
    assert torch.equal(got, ref.fused_moe(h, bf13, bf2, w, ids))
    with pytest.raises(TypeError, match="both"):
        ops.fused_moe(h, w13, bf2, w, ids)
    with pytest.raises(TypeError, match="both"):
        ops.fused_moe(h, bf13, w2, w, ids)
    with pytest.raises(TypeError, match="both"):
        ops.fused_moe(h, w13, quantize_fp8_experts(w2.float()), w, ids)


# ------------------------------------------------------------------------------ predicate
def test_supported_wherever_the_bf16_kernel_is_and_k_is_a_multiple_of_128():
    c = _runtime_loader.contract()
    sup, dsup = c.moe_q4gemm_supported, c.moe_dgemm_supported
    pfs = (1, 2, 4)
    seen = 0
    for N in (8, 96, 192, 320, 4096):
        for K in (64, 128, 192, 256, 320, 384, 768, 1024, 14336):
            for silu in (0, 1):
                for s in (1, 2, 3, 4):
                    mine = any(sup(N, K, pf, silu, s) for pf in pfs)
                    if K % 128:
                        assert not mine, (N, K, silu, s)
                    elif any(dsup(N, K, pf, silu, s) for pf in pfs):
                        assert mine, (N, K, silu, s)
                        seen += 1
    assert seen > 50
    # 192-deep slices are a step and a half step: ring depths 1 and 2, not 4
    assert sup(320, 384, 1, 0, 2) and sup(320, 384, 2, 0, 2) and not sup(320, 384, 4, 0, 2)
    assert sup(2048, 768, 2, 0, 4)              # Qwen3-30B-A3B down, split 4: step + half step
    assert not sup(320, 256, 3, 0, 1) and not sup(320, 256, 8, 0, 1) and not sup(324, 256, 1, 0, 1)
    assert not sup(320, 256, 1, 1, 2), "SwiGLU with split-K"


# ------------------------------------------------------------------------------ sharding
def _block(cfg, rank, world, tp, mode):
    ps = ParallelState(rank=rank, world_size=world, tp_size=tp, tp_rank=rank % tp)
    blk = MoEBlock(cfg, ps, "cpu", torch.bfloat16, torch.Generator().manual_seed(0),
                   full_then_shard=True, mode=mode)
    blk.quantize_mxfp4()
    assert blk.quantized and isinstance(blk.w13, Mxfp4Experts) and isinstance(blk.w2, Mxfp4Experts)
    return blk


def _routed(blk, h, w, ids):
    """The block's experts on a given routing (ids global; this rank's experts only)."""
    local = ids - blk.e0
    local = torch.where((local >= 0) & (local < blk.e_local), local, torch.full_like(local, -1))
    return ops.fused_moe(h, blk.w13, blk.w2, w, local.to(torch.int32)).float()


@pytest.mark.parametrize("model", MOE_MODELS)
def test_sharded_quantized_blocks_match_the_unsharded_one(model):
    """tp = 2 (F shards, summed) and ep = 2 (expert halves, routed) quantized blocks against the
    unsharded quantized block.  Scales are per 32-block along K, and an F shard cuts w2's K on
    multiples of 128, so every shard holds exactly the unsharded block's codes and scales; only
    the bf16 rounding of the two partial down projections differs (the tolerance of the CPU MoE
    tests)."""
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
        assert torch.equal(b.w13.q[:, :F2], full.w13.q[:, r * F2:(r + 1) * F2])
        assert torch.equal(b.w13.scale[:, :F2], full.w13.scale[:, r * F2:(r + 1) * F2])
        sh = full.w2[:, :, r * F2:(r + 1) * F2]
        assert torch.equal(b.w2.q, sh.q) and torch.equal(b.w2.scale, sh.scale)
    got_tp = sum(_routed(b, h, w, ids) for b in tp)
    assert torch.allclose(got_tp, want, atol=3e-2, rtol=3e-2)
    ep = [_block(cfg, r, 2, 1, "ep") for r in range(2)]
    for r, b in enumerate(ep):
        el = cfg.num_experts // 2
        assert b.e_local == el and torch.equal(b.w2.q, full.w2.q[r * el:(r + 1) * el])
        assert torch.equal(b.w13.scale, full.w13.scale[r * el:(r + 1) * el])
    got_ep = sum(_routed(b, h, w, ids) for b in ep)
    assert torch.allclose(got_ep, want, atol=3e-2, rtol=3e-2)


def test_f_shard_that_is_no_multiple_of_128_is_refused():
    cfg = get_config("tiny-mixtral")
    ps = ParallelState(rank=0, world_size=4, tp_size=4, tp_rank=0)    # F shard 64
    blk = MoEBlock(cfg, ps, "cpu", torch.bfloat16, torch.Generator().manual_seed(0),
                   full_then_shard=False, mode="tp")
    with pytest.raises(ValueError, match="multiples of 128"):
        blk.quantize_mxfp4()
    assert blk.w13.dtype == torch.bfloat16, "refused before anything was dropped"
    blk.quantize_fp8()                                                # fp8 takes the shard


# ------------------------------------------------------------------------------ config
def test_config_precedence(monkeypatch):
    monkeypatch.delenv("AKAP_EXPERT_QUANTIZATION", raising=False)
    assert EngineConfig().expert_quantization is None
    assert EngineConfig(expert_quantization="mxfp4").expert_quantization == "mxfp4"
    monkeypatch.setenv("AKAP_EXPERT_QUANTIZATION", "mxfp4")
    assert EngineConfig().expert_quantization == "mxfp4"
    assert EngineConfig(expert_quantization="none").expert_quantization == "none"  # field wins
    assert EngineConfig(expert_quantization="fp8").expert_quantization == "fp8"
    assert EngineConfig().quantization is None            # the dense knob is untouched
    monkeypatch.setenv("AKAP_EXPERT_QUANTIZATION", "fp8")
    assert EngineConfig(expert_quantization="mxfp4").expert_quantization == "mxfp4"
    monkeypatch.setenv("AKAP_EXPERT_QUANTIZATION", "mxfp8")
    with pytest.raises(ValueError, match="expert_quantization"):
        EngineConfig()
    # an unknown value in the variable is an error even where a field overrides it
    for field in ("mxfp4", "fp8", "none"):
        with pytest.raises(ValueError, match="AKAP_EXPERT_QUANTIZATION"):
            EngineConfig(expert_quantization=field)
    monkeypatch.delenv("AKAP_EXPERT_QUANTIZATION")
    with pytest.raises(ValueError, match="expert_quantization"):
        EngineConfig(expert_quantization="int8")


def _engine(model, **kw):
    cfg = dict(model=model, device="cpu", max_model_len=256, max_num_seqs=8,
               max_num_batched_tokens=64, block_size=32, num_gpu_blocks=64, init_std=0.1)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), log=lambda *a: None)


def test_knob_errors_and_cli(monkeypatch):
    monkeypatch.delenv("AKAP_EXPERT_QUANTIZATION", raising=False)
    with pytest.raises(ValueError, match="no experts"):
        _engine("tiny-llama", expert_quantization="mxfp4")
    with pytest.raises(ValueError, match="no experts"):
        DecoderLM(get_config("tiny-qwen3"), "cpu", max_model_len=256).quantize_mxfp4_experts()
    with pytest.raises(ValueError, match="MoE"):          # --quantization stays dense-only
        _engine("tiny-mixtral", quantization="mxfp4", expert_quantization="mxfp4")
    with pytest.raises(ValueError, match="expert-quantization"):
        _engine("tiny-mixtral", quantization="mxfp4")
    from aws_k8s_ansible_provisioner_amd.server.api_server import (engine_config_from_args,
                                                                   make_parser)
    a = make_parser().parse_args(["--model", "tiny-mixtral", "--expert-quantization", "mxfp4"])
    assert engine_config_from_args(a).expert_quantization == "mxfp4"
    monkeypatch.setenv("AKAP_EXPERT_QUANTIZATION", "mxfp4")
    a = make_parser().parse_args(["--model", "tiny-mixtral"])
    assert engine_config_from_args(a).expert_quantization == "mxfp4"    # from the environment
    a = make_parser().parse_args(["--model", "tiny-mixtral", "--expert-quantization", "fp8"])
    assert engine_config_from_args(a).expert_quantization == "fp8"      # the flag wins
    a = make_parser().parse_args(["--model", "tiny-mixtral", "--expert-quantization", "none"])
    assert engine_config_from_args(a).expert_quantization == "none"


# ------------------------------------------------------------------------------ checkpoints
def _quantized_model(model, seed=3):
    m = DecoderLM(get_config(model), "cpu", seed=seed, max_model_len=256, init_std=0.1)
    m.quantize_mxfp4_experts()
    assert m.experts_quantized and not m.quantized and m.quantization is None
    assert m.expert_quantization == "mxfp4"
    return m


def _fresh(model, eq="mxfp4", ps=None):
    return DecoderLM(get_config(model), "cpu", seed=99, max_model_len=256, expert_quantization=eq,
                     pstate=ps)


def _same_experts(a, b):
    for la, lb in zip(a.layers, b.layers):
        for n in ("w13", "w2"):
            wa, wb = getattr(la.moe, n), getattr(lb.moe, n)
            assert isinstance(wb, Mxfp4Experts)
            assert torch.equal(wa.q, wb.q) and torch.equal(wa.scale, wb.scale), n
        assert torch.equal(la.moe.router, lb.moe.router)
        assert torch.equal(la.w_qkv, lb.w_qkv) and torch.equal(la.w_o, lb.w_o)


def _expert_weight_keys(sd):
    return [k for k in sd if ".experts." in k and k.endswith(".weight")]


@pytest.mark.parametrize("model", MOE_MODELS)
def test_checkpoint_round_trip_is_bit_exact(model):
    src = _quantized_model(model)
    sd = src.hf_state_dict()
    keys = _expert_weight_keys(sd)
    assert keys and all(sd[k].dtype == torch.uint8 for k in keys)
    for k in keys:                       # <proj>.weight [N, K/2] + <proj>.weight_scale [N, K/32]
        sc = sd[k[:-7] + ".weight_scale"]
        N, K2 = sd[k].shape
        assert sc.dtype == torch.uint8 and tuple(sc.shape) == (N, 2 * K2 // 32)
    assert sd["model.layers.0.self_attn.q_proj.weight"].dtype == torch.bfloat16
    dst = _fresh(model)
    dst.load_state_dict(sd)
    assert dst.experts_quantized and not dst.quantized
    _same_experts(src, dst)
    sd2 = dst.hf_state_dict()
    assert sd.keys() == sd2.keys()
    for k in sd:
        assert sd[k].dtype == sd2[k].dtype and torch.equal(sd[k], sd2[k]), k
    # without the knob, or with the fp8 knob, the checkpoint is refused
    with pytest.raises(ValueError, match="quantization"):
        _fresh(model, eq=None).load_state_dict(sd)
    with pytest.raises(ValueError, match="--expert-quantization mxfp4"):
        _fresh(model, eq="fp8").load_state_dict(sd)
    # a scale code outside 2..252 is refused at load
    bad = dict(sd)
    k = keys[0][:-7] + ".weight_scale"
    bad[k] = sd[k].clone()
    bad[k][0, 0] = 255
    with pytest.raises(ValueError, match="e8m0"):
        _fresh(model).load_state_dict(bad)


@pytest.mark.parametrize("model", MOE_MODELS)
@pytest.mark.parametrize("mode,tp", [("tp", 2), ("ep", 1)])
def test_checkpoint_loads_bit_exactly_into_two_shards(model, mode, tp, monkeypatch):
    """TP = 2 slices F on 128-element boundaries (whole scale blocks), EP = 2 takes half of the
    experts: both shards hold exactly the checkpoint's codes and scales."""
    monkeypatch.setenv("AKAP_MOE_MODE", mode)
    src = _quantized_model(model)
    sd = src.hf_state_dict()
    cfg = src.cfg
    Fn, F2, el = cfg.intermediate_size, cfg.intermediate_size // 2, cfg.num_experts // 2
    for r in range(2):
        ps = ParallelState(rank=r, world_size=2, tp_size=tp, tp_rank=r % tp)
        dst = _fresh(model, ps=ps)
        dst.load_state_dict(sd)
        for ls, ld in zip(src.layers, dst.layers):
            assert isinstance(ld.moe.w13, Mxfp4Experts) and ld.moe.mode == mode
            if mode == "ep":
                assert torch.equal(ld.moe.w13.q, ls.moe.w13.q[r * el:(r + 1) * el])
                assert torch.equal(ld.moe.w2.scale, ls.moe.w2.scale[r * el:(r + 1) * el])
                assert torch.equal(ld.moe.w2.q, ls.moe.w2.q[r * el:(r + 1) * el])
            else:
                fs = slice(r * F2, (r + 1) * F2)
                gate, up = ls.moe.w13[:, :Fn][:, fs], ls.moe.w13[:, Fn:][:, fs]
                assert torch.equal(ld.moe.w13.q, torch.cat([gate.q, up.q], 1))
                assert torch.equal(ld.moe.w13.scale, torch.cat([gate.scale, up.scale], 1))
                sh = ls.moe.w2[:, :, fs]
                assert torch.equal(ld.moe.w2.q, sh.q) and torch.equal(ld.moe.w2.scale, sh.scale)


@pytest.mark.parametrize("model", MOE_MODELS)
def test_checkpoint_plain_and_fp8_sources(model):
    bf = DecoderLM(get_config(model), "cpu", seed=5, max_model_len=256, init_std=0.1)
    plain = bf.hf_state_dict()
    # a plain bf16 source is quantized at load: the same as quantizing the loaded model
    want = DecoderLM(get_config(model), "cpu", seed=5, max_model_len=256, init_std=0.1)
    want.quantize_mxfp4_experts()
    dst = _fresh(model)
    dst.load_state_dict(plain)
    _same_experts(want, dst)
    # fp8 experts given to an mxfp4 engine: an error that names the right knob
    fp8 = dict(plain)
    for k in _expert_weight_keys(plain):
        f = quantize_fp8(plain[k])
        fp8[k] = f.q.view(torch.float8_e4m3fn)
        fp8[k[:-7] + ".weight_scale"] = f.scale.reshape(-1, 1)
    with pytest.raises(ValueError, match="FP8 experts.*--expert-quantization fp8"):
        _fresh(model).load_state_dict(fp8)


# ------------------------------------------------------------------------------ bytes
@pytest.mark.parametrize("model", MOE_MODELS)
def test_weight_bytes(model):
    bf = DecoderLM(get_config(model), "cpu", max_model_len=256)
    total = bf.weight_bytes()
    numel = [lw.moe.numel() for lw in bf.layers]
    experts = sum(w.numel() for lw in bf.layers for w in (lw.moe.w13, lw.moe.w2))
    bf.quantize_mxfp4_experts()
    # bf16: 2 bytes per element; mxfp4: 1/2 + 1/32
    assert bf.weight_bytes() == total - 2 * experts + experts // 2 + experts // 32
    assert bf.weight_bytes(as_bf16=True) == total
    assert [lw.moe.numel() for lw in bf.layers] == numel     # numel keeps its meaning
    for lw in bf.layers:
        E, N, K = lw.moe.w13.shape
        assert lw.moe.w13.nbytes == E * N * K // 2 + E * N * K // 32


# ------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("model", MOE_MODELS)
def test_cpu_engine_with_mxfp4_experts_matches_dense_reference(model):
    """The CPU reference engine, teacher-forced against dense_logits of the same quantized
    model on the GPU test's prompts, under that test's bound: a prompt on which this path
    itself missed 0.2 std would sit on a router near-tie and could not carry the GPU bound."""
    eng = _engine(model, expert_quantization="mxfp4")
    m = eng.runner.model
    assert m.experts_quantized and not m.quantized
    assert all(isinstance(lw.moe.w13, Mxfp4Experts) and isinstance(lw.moe.w2, Mxfp4Experts)
               for lw in m.layers)
    outs = eng.generate(None, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True),
                        prompt_ids=PROMPTS)
    worst = 0.0
    for p, o in zip(PROMPTS, outs):
        assert len(o.output_ids) == 12
        logits = dense_logits(m, list(p) + list(o.output_ids)).float()
        gap = 0.0
        for i, tok in enumerate(o.output_ids):
            row = logits[len(p) - 1 + i]
            gap = max(gap, (row.max() - row[tok]).item() / (row.std().item() + 1e-6))
        print(f"[gap] {model} cpu reference path, mxfp4 experts, prompt {p[:3]}.. x{len(p)}: "
              f"{gap:.4f} std")
        worst = max(worst, gap)
    assert worst <= GAP_TOL
