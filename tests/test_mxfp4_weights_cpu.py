"""MXFP4 (e2m1 codes + one e8m0 scale per 32 elements along K) weight quantization on the CPU
path: the quantizer's rule and error bound, Mxfp4Weight's surface, the
`y = bf16(sum_k x[m,k] * e2m1(q[n,k]) * 2^(scale[n,k/32] - 127))` contract of ops.linear /
linear_silu, the quantized engine against the dense reference, MXFP4 checkpoints through
load_state_dict (round trip, plain, tp=2 shards) and the error paths."""
import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
from aws_k8s_ansible_provisioner_amd.models.config import get_config
from aws_k8s_ansible_provisioner_amd.models.reference_forward import dense_logits
from aws_k8s_ansible_provisioner_amd.models.transformer import QUANTIZATIONS, DecoderLM
from aws_k8s_ansible_provisioner_amd.ops.quant import (Fp8Weight, Mxfp4Weight, QuantWeight,
                                                       quantize_fp8, quantize_mxfp4)
from aws_k8s_ansible_provisioner_amd.parallel.state import ParallelState

PROMPTS = [list(range(5, 40)), [100, 101], [9, 9, 9]]
PROJ = ("w_qkv", "w_o", "w_gate_up", "w_down")
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
LUT = torch.tensor(E2M1 + [-v for v in E2M1])


def _codes(w: Mxfp4Weight) -> torch.Tensor:
    """The [N, K] e2m1 codes: element 2j in the low nibble of byte j, 2j + 1 in the high."""
    return torch.stack((w.q & 15, w.q >> 4), dim=-1).reshape(w.shape)


def _deq(w: Mxfp4Weight) -> torch.Tensor:
    """The contract's dequantized matrix in fp64, written independently of Mxfp4Weight.float."""
    s = torch.exp2(w.scale.double() - 127).repeat_interleave(32, dim=1)
    return LUT[_codes(w).long()].double() * s


def _quantizer_bound(w: Mxfp4Weight, src: torch.Tensor) -> None:
    """|deq - src| <= max(0.25 |src|, 0.25 * 2^e) (1 + 1e-3): half a step of a 1-bit mantissa,
    half the subnormal step 0.5, and the saturated range (6, 8)."""
    src = src.double()
    err = (_deq(w) - src).abs()
    step = torch.exp2(w.scale.double() - 127).repeat_interleave(32, dim=1)
    lim = torch.maximum(src.abs() * 0.25, step * 0.25) * (1 + 1e-3)
    bad = int((err > lim).sum())
    assert bad == 0, f"{bad} elements outside the quantizer bound (max err {err.max():.4g})"


def _scales_in_range(w: Mxfp4Weight) -> None:
    assert int(w.scale.min()) >= 2 and int(w.scale.max()) <= 252


def test_quantizer_bound_codes_and_zero_block():
    torch.manual_seed(0)
    w = torch.randn(512, 1024) * 0.05
    w[7] = 0.0
    w[11] = 0.0
    w[11, 5] = 3.0   # a single outlier: every other element of its block is zero
    w[13, 100] = -40.0  # an outlier among ordinary values (they underflow to 0 in its block)
    mw = quantize_mxfp4(w)
    assert mw.q.dtype == torch.uint8 and mw.q.shape == (512, 512) and mw.q.is_contiguous()
    assert mw.scale.dtype == torch.uint8 and mw.scale.shape == (512, 32)
    assert mw.shape == (512, 1024) and mw.numel() == 512 * 1024 and mw.dim() == 2
    assert mw.nbytes == 512 * 1024 // 2 + 512 * 1024 // 32 and not mw.is_cuda
    assert mw.device == torch.device("cpu") and "Mxfp4Weight" in repr(mw)
    _quantizer_bound(mw, w)
    _scales_in_range(mw)
    assert torch.equal(mw.float().double(), _deq(mw))  # float() is the exact matrix
    # all-zero blocks: scale code 127, zero codes
    assert bool((mw.scale[7] == 127).all()) and int(mw.q[7].max()) == 0
    assert bool((mw.scale[11, 1:] == 127).all()) and int(mw.q[11, 16:].max()) == 0
    # the rule: e = floor(log2(amax)) - 2
    amax = w.view(512, 32, 32).abs().amax(2)
    want = torch.where(amax > 0, torch.floor(torch.log2(amax.double())) - 2 + 127,
                       torch.full_like(amax, 127, dtype=torch.float64))
    assert torch.equal(mw.scale.double(), want)
    # 3 = 6 * 2^-1 is on the grid; 40 = 5 * 2^3 is the tie between 4 and 6: the even one, 4
    assert mw.float()[11, 5].item() == 3.0 and mw.float()[13, 100].item() == -32.0
    # bf16 source
    wb = w.to(torch.bfloat16)
    mb = quantize_mxfp4(wb)
    _quantizer_bound(mb, wb)
    _scales_in_range(mb)
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros(4, 48))  # K not a multiple of 32


@pytest.mark.parametrize("e", [0, -5, 9])
def test_quantizer_ties_round_to_even_and_saturate(e):
    """amax = 7.5 * 2^e gives floor(log2) - 2 = e.  Ties go to the even mantissa: 2.5 -> 2,
    3.5 -> 4, 5 -> 4, 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2; 7.5 saturates at 6."""
    vals = [7.5, 2.5, 3.5, 5.0, 0.25, 0.75, 1.25, 1.75, -2.5, -3.5, -5.0, -7.5, 6.0, 0.0, -0.25,
            7.0]
    want = [6.0, 2.0, 4.0, 4.0, 0.0, 1.0, 1.0, 2.0, -2.0, -4.0, -4.0, -6.0, 6.0, 0.0, 0.0, 6.0]
    w = torch.zeros(2, 64)
    w[1, 32:32 + len(vals)] = torch.tensor(vals) * 2.0 ** e
    mw = quantize_mxfp4(w)
    assert int(mw.scale[1, 1]) == 127 + e and int(mw.scale[1, 0]) == 127
    got = mw.float()[1, 32:32 + len(vals)] / 2.0 ** e
    assert torch.equal(got, torch.tensor(want))
    assert _codes(mw)[1, 32].item() == 7 and _codes(mw)[1, 43].item() == 15  # +6 and -6
    # tiny and huge blocks clamp the scale code into 2..252
    w = torch.zeros(1, 64)
    w[0, 0], w[0, 32] = 1e-38, 3e38
    _scales_in_range(quantize_mxfp4(w))


def test_weight_slicing_and_constructor_checks():
    torch.manual_seed(2)
    mw = quantize_mxfp4(torch.randn(24, 128) * 0.05)
    full = mw.float()
    rows = mw[4:20]
    assert isinstance(rows, Mxfp4Weight) and rows.shape == (16, 128)
    assert torch.equal(rows.q, mw.q[4:20]) and torch.equal(rows.scale, mw.scale[4:20])
    assert torch.equal(rows.float(), full[4:20])
    cols = mw[:, 32:96]
    assert cols.shape == (24, 64) and cols.q.shape == (24, 32) and cols.scale.shape == (24, 2)
    assert torch.equal(cols.float(), full[:, 32:96])
    assert torch.equal(mw[2:10, 64:].float(), full[2:10, 64:])
    assert cols.q.is_contiguous() and cols.scale.is_contiguous()
    for bad in (slice(16, 96), slice(32, 80), slice(0, 128, 2)):
        with pytest.raises(ValueError):
            mw[:, bad]
    with pytest.raises(TypeError):
        mw[3]
    assert mw.to("cpu").shape == mw.shape and torch.equal(mw.to("cpu").q, mw.q)
    # the constructor refuses the NaN code and codes outside 2..252, and wrong shapes / dtypes
    for code in (255, 0, 1, 253):
        s = mw.scale.clone()
        s[3, 1] = code
        with pytest.raises(ValueError, match="scale"):
            Mxfp4Weight(mw.q, s)
    Mxfp4Weight(mw.q, torch.full_like(mw.scale, 252))
    Mxfp4Weight(mw.q, torch.full_like(mw.scale, 2))
    with pytest.raises(ValueError):
        Mxfp4Weight(mw.q, mw.scale[:, :3])
    with pytest.raises(ValueError):
        Mxfp4Weight(mw.q.to(torch.int32), mw.scale)
    with pytest.raises(ValueError):
        Mxfp4Weight(mw.q[:, :24], mw.scale[:, :1])  # K = 48
    assert QuantWeight == (Fp8Weight, Mxfp4Weight)
    assert isinstance(mw, QuantWeight) and isinstance(quantize_fp8(full), QuantWeight)


def test_linear_and_linear_silu_follow_the_contract():
    torch.manual_seed(1)
    mw = quantize_mxfp4(torch.randn(96, 128) * 0.05)
    x = torch.randn(5, 128).to(torch.bfloat16)
    ref = (x.double() @ _deq(mw).t()).float()
    y = ops.linear(x, mw)
    assert y.dtype == torch.bfloat16 and y.shape == (5, 96)
    # fp32 summation order differs from the fp64 sum: allow one bf16 ulp
    assert torch.allclose(y.float(), ref.to(torch.bfloat16).float(), rtol=2 ** -7, atol=1e-6)
    out = torch.empty(5, 96, dtype=torch.bfloat16)
    assert ops.linear(x, mw, out=out) is out and torch.equal(out, y)
    s = ops.linear_silu(x, mw)
    g, u = y.float()[:, :48], y.float()[:, 48:]
    want = (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
    assert s.shape == (5, 48)
    assert torch.allclose(s.float(), want.float(), rtol=2 ** -6, atol=1e-6)
    assert torch.equal(s, ops.silu_and_mul(y))


def _engine(model, **kw):
    cfg = dict(model=model, device="cpu", max_model_len=256, max_num_seqs=8,
               max_num_batched_tokens=64, block_size=32, num_gpu_blocks=64, init_std=0.1,
               quantization="mxfp4")
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), log=lambda *a: None)


def _check_teacher_forced(model, prompt, out, tol=0.15):
    logits = dense_logits(model, list(prompt) + list(out)).float().cpu()
    for i, tok in enumerate(out):
        row = logits[len(prompt) - 1 + i]
        gap = (row.max() - row[tok]).item() / (row.std().item() + 1e-6)
        assert gap <= tol, f"step {i}: token {tok} is {gap:.3f} std below the argmax"


def _formula_bytes(m: DecoderLM) -> int:
    n = m.embed.numel() + m.final_norm.numel()
    if m.lm_head is not m.embed:
        n += m.lm_head.numel()
    total = 2 * n
    for lw in m.layers:
        total += 2 * (lw.ln1.numel() + lw.ln2.numel())
        if lw.q_norm is not None:
            total += 2 * (lw.q_norm.numel() + lw.k_norm.numel())
        for name in PROJ:
            N, K = getattr(lw, name).shape
            total += N * K // 2 + N * K // 32
    return total


@pytest.mark.parametrize("model", ["tiny-qwen3", "tiny-llama"])
def test_quantized_engine_matches_dense_reference(model):
    eng = _engine(model)
    m = eng.runner.model
    assert m.quantized and m.quantization == "mxfp4"
    for lw in m.layers:
        for name in PROJ:
            assert isinstance(getattr(lw, name), Mxfp4Weight), name
    assert m.embed.dtype == torch.bfloat16 and m.lm_head.dtype == torch.bfloat16
    assert m.weight_bytes() == _formula_bytes(m)
    bf16 = DecoderLM(get_config(model), "cpu", max_model_len=256)
    assert m.weight_bytes(as_bf16=True) == bf16.weight_bytes()
    proj = sum(getattr(lw, n).numel() for lw in bf16.layers for n in PROJ)
    assert m.weight_bytes() == bf16.weight_bytes() - 2 * proj + proj // 2 + proj // 32
    prompts = [list(range(5, 60)), [100, 101], [7, 8, 9] * 10]
    outs = eng.generate(None, SamplingParams(max_tokens=8, temperature=0, ignore_eos=True),
                        prompt_ids=prompts)
    for p, o in zip(prompts, outs):
        assert len(o.output_ids) == 8
        _check_teacher_forced(m, p, o.output_ids)


def _quantized_model(model, seed):
    m = DecoderLM(get_config(model), "cpu", seed=seed, max_model_len=256, init_std=0.15,
                  quantization="mxfp4")
    m.quantize_mxfp4()
    return m


def _save(sd, d):
    from safetensors.torch import save_file

    d.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    return str(d)


@pytest.mark.parametrize("model", ["tiny-qwen3", "tiny-llama"])
def test_mxfp4_checkpoint_round_trip_is_bit_exact(model, tmp_path):
    from aws_k8s_ansible_provisioner_amd.engine.weights import load_safetensors_dir

    src = _quantized_model(model, 11)
    sd = src.hf_state_dict()
    w = sd["model.layers.0.self_attn.k_proj.weight"]
    s = sd["model.layers.0.self_attn.k_proj.weight_scale"]
    assert w.dtype == torch.uint8 and w.shape == (256, 128)   # [N, K/2]
    assert s.dtype == torch.uint8 and s.shape == (256, 8)     # [N, K/32]
    assert "model.layers.0.mlp.up_proj.weight_scale" in sd
    assert sd["model.embed_tokens.weight"].dtype == torch.bfloat16
    assert "model.embed_tokens.weight_scale" not in sd
    wdir = _save(sd, tmp_path / "ck")
    dst = _quantized_model(model, 99)
    assert not torch.equal(dst.layers[0].w_qkv.q, src.layers[0].w_qkv.q)
    dst.load_state_dict(load_safetensors_dir(wdir))
    for a, b in zip(src.layers, dst.layers):
        for name in PROJ:
            assert torch.equal(getattr(a, name).q, getattr(b, name).q), name
            assert torch.equal(getattr(a, name).scale, getattr(b, name).scale), name
    for p in PROMPTS:
        assert torch.equal(dense_logits(src, p), dense_logits(dst, p))
    # and the export of what was loaded is the file again
    again = dst.hf_state_dict()
    assert again.keys() == sd.keys() and all(torch.equal(again[k], sd[k]) for k in sd)


def test_plain_checkpoint_is_quantized_at_load():
    src = DecoderLM(get_config("tiny-llama"), "cpu", seed=3, max_model_len=256, init_std=0.15)
    dst = DecoderLM(get_config("tiny-llama"), "cpu", seed=4, max_model_len=256,
                    quantization="mxfp4")
    assert not dst.quantized
    dst.load_state_dict(src.hf_state_dict())
    assert dst.quantized
    for a, b in zip(src.layers, dst.layers):
        for name in PROJ:
            got = getattr(b, name)
            assert isinstance(got, Mxfp4Weight)
            _quantizer_bound(got, getattr(a, name))
            want = quantize_mxfp4(getattr(a, name))
            assert torch.equal(got.q, want.q) and torch.equal(got.scale, want.scale)


@pytest.mark.parametrize("model", ["tiny-qwen3", "tiny-llama"])
def test_mxfp4_checkpoint_sharded_load_tp2_equals_slices(model):
    """Each tp=2 rank's projections are slices of the unsharded weight: q | k | v and gate | up
    by rows (codes and scales), o and down by columns, on a multiple of 32."""
    src = _quantized_model(model, 11)
    sd = src.hf_state_dict()
    cfg = get_config(model)
    D, hq, hkv, F_ = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, cfg.intermediate_size
    for r in range(2):
        ps = ParallelState(rank=r, world_size=2, tp_size=2, tp_rank=r)
        m = DecoderLM(cfg, "cpu", seed=5, max_model_len=256, pstate=ps, quantization="mxfp4")
        m.load_state_dict(sd)
        for full, lw in zip(src.layers, m.layers):
            q0, k0 = hq * D, hkv * D
            nq, nk = q0 // 2, k0 // 2
            rows = torch.cat([torch.arange(r * nq, (r + 1) * nq),
                              q0 + torch.arange(r * nk, (r + 1) * nk),
                              q0 + k0 + torch.arange(r * nk, (r + 1) * nk)])
            assert torch.equal(lw.w_qkv.q, full.w_qkv.q[rows])
            assert torch.equal(lw.w_qkv.scale, full.w_qkv.scale[rows])
            h = F_ // 2
            rows = torch.cat([torch.arange(r * h, (r + 1) * h),
                              F_ + torch.arange(r * h, (r + 1) * h)])
            assert torch.equal(lw.w_gate_up.q, full.w_gate_up.q[rows])
            assert torch.equal(lw.w_gate_up.scale, full.w_gate_up.scale[rows])
            for name, K in (("w_o", q0), ("w_down", F_)):
                a, b = r * K // 2, (r + 1) * K // 2
                got, want = getattr(lw, name), getattr(full, name)
                assert got.shape == (cfg.hidden_size, K // 2)
                assert torch.equal(got.q, want.q[:, a // 2:b // 2])
                assert torch.equal(got.scale, want.scale[:, a // 32:b // 32])
                assert torch.equal(got.float(), want.float()[:, a:b])


def test_errors():
    src = _quantized_model("tiny-llama", 11)
    sd = src.hf_state_dict()
    bf16 = DecoderLM(get_config("tiny-llama"), "cpu", seed=1, max_model_len=256)
    with pytest.raises(ValueError, match="--quantization mxfp4"):
        bf16.load_state_dict(sd)
    fp8 = DecoderLM(get_config("tiny-llama"), "cpu", seed=1, max_model_len=256,
                    quantization="fp8")
    with pytest.raises(ValueError, match="--quantization mxfp4"):
        fp8.load_state_dict(sd)
    # a file whose scale codes include the NaN code is refused by the loader
    bad = dict(sd)
    s = bad["model.layers.1.mlp.down_proj.weight_scale"].clone()
    s[0, 0] = 255
    bad["model.layers.1.mlp.down_proj.weight_scale"] = s
    with pytest.raises(ValueError, match="scale"):
        _quantized_model("tiny-llama", 12).load_state_dict(bad)
    assert "mxfp4" in QUANTIZATIONS
    with pytest.raises(ValueError, match="quantization"):
        DecoderLM(get_config("tiny-llama"), "cpu", max_model_len=256, quantization="mxfp8")
    with pytest.raises(ValueError, match="quantization"):
        EngineConfig(quantization="int4")
    with pytest.raises(ValueError, match="MoE"):
        _engine("tiny-mixtral")
    with pytest.raises(ValueError, match="MoE"):
        DecoderLM(get_config("tiny-qwen3-moe"), "cpu", max_model_len=256).quantize_mxfp4()


def test_config_reads_the_environment(monkeypatch):
    monkeypatch.setenv("AKAP_QUANTIZATION", "mxfp4")
    assert EngineConfig().quantization == "mxfp4"
    assert EngineConfig(quantization="none").quantization == "none"  # the flag wins
    assert EngineConfig(quantization="fp8").quantization == "fp8"
    eng = _engine("tiny-llama", quantization="none")
    assert not eng.runner.model.quantized
    assert isinstance(eng.runner.model.layers[0].w_qkv, torch.Tensor)
    monkeypatch.setenv("AKAP_QUANTIZATION", "fp8")
    assert EngineConfig(quantization="mxfp4").quantization == "mxfp4"
    monkeypatch.setenv("AKAP_QUANTIZATION", "int4")
    with pytest.raises(ValueError):
        EngineConfig()


def test_server_flag():
    from aws_k8s_ansible_provisioner_amd.server.api_server import (engine_config_from_args,
                                                                    make_parser)

    ap = make_parser()
    a = ap.parse_args(["--quantization", "mxfp4"])
    assert engine_config_from_args(a).quantization == "mxfp4"
    with pytest.raises(SystemExit):
        ap.parse_args(["--quantization", "int4"])


def test_server_with_quantization_mxfp4_serves_a_completion():
    from fastapi.testclient import TestClient

    from aws_k8s_ansible_provisioner_amd.server.api_server import (build_app,
                                                                    engine_config_from_args,
                                                                    make_parser)

    a = make_parser().parse_args(["--model", "tiny-qwen3", "--quantization", "mxfp4", "--device",
                                  "cpu", "--max-model-len", "256", "--max-num-seqs", "8",
                                  "--max-num-batched-tokens", "64", "--num-gpu-blocks", "128"])
    app, ae = build_app(engine_config_from_args(a))
    with TestClient(app) as c:
        r = c.post("/v1/completions", json={"prompt": [[5, 6, 7]], "max_tokens": 4,
                                            "temperature": 0, "ignore_eos": True})
        assert r.status_code == 200, r.text
        assert r.json()["usage"]["completion_tokens"] == 4
