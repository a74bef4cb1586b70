"""FP8 (e4m3fn) weight quantization on the CPU path: the quantizer's error bound, the
`y = bf16(scale[n] * sum_k x[m,k] * q[n,k])` contract of ops.linear / linear_silu on an
Fp8Weight, the quantized engine against the dense reference, FP8 checkpoints (per-channel,
per-tensor and block-scaled) through load_state_dict, the error paths and the tp=2 load."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
from aws_k8s_ansible_provisioner_amd.models.config import get_config
from aws_k8s_ansible_provisioner_amd.models.reference_forward import dense_logits
from aws_k8s_ansible_provisioner_amd.models.transformer import DecoderLM
from aws_k8s_ansible_provisioner_amd.ops.quant import Fp8Weight, quantize_fp8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPTS = [list(range(5, 40)), [100, 101], [9, 9, 9]]
PROJ = ("w_qkv", "w_o", "w_gate_up", "w_down")


def _quantizer_bound(w: Fp8Weight, src: torch.Tensor) -> None:
    """|deq - src| <= max(2^-4 |src|, 2^-10 scale[n]) (1 + 1e-3): half an ulp of a 3-bit
    mantissa is 2^-4 relative, half the subnormal step 2^-9 is 2^-10 (in units of scale)."""
    src = src.float()
    err = (w.float() - src).abs()
    lim = torch.maximum(src.abs() * 2.0 ** -4, w.scale[:, None] * 2.0 ** -10) * (1 + 1e-3)
    bad = int((err > lim).sum())
    assert bad == 0, f"{bad} elements outside the quantizer bound (max err {err.max():.4g})"


def _no_nan_codes(q: torch.Tensor) -> None:
    assert not bool(((q & 0x7F) == 0x7F).any())


def test_quantizer_bound_codes_and_zero_row():
    torch.manual_seed(0)
    w = torch.randn(512, 1024) * 0.05
    w[7] = 0.0
    w[11] = 0.0
    w[11, 5] = 3.0   # a single outlier: every other element of the row underflows
    w[13, 100] = -40.0  # an outlier among ordinary values (they land in the subnormals)
    fw = quantize_fp8(w)
    assert fw.q.dtype == torch.uint8 and fw.q.shape == (512, 1024) and fw.q.is_contiguous()
    assert fw.scale.dtype == torch.float32 and fw.scale.shape == (512,)
    assert fw.shape == (512, 1024) and fw.numel() == 512 * 1024
    assert fw.nbytes == 512 * 1024 + 4 * 512 and not fw.is_cuda
    _quantizer_bound(fw, w)
    _no_nan_codes(fw.q)
    assert fw.scale[7].item() == 1.0 and int(fw.q[7].max()) == 0
    assert torch.equal(fw.scale, torch.where(w.abs().amax(1) > 0, w.abs().amax(1) / 448,
                                             torch.ones(512)))
    # the row maximum maps to +-448 exactly
    assert fw.float().abs().amax(1)[13].item() == pytest.approx(40.0, rel=1e-6)
    # bf16 source
    wb = w.to(torch.bfloat16)
    _quantizer_bound(quantize_fp8(wb), wb)


def test_linear_and_linear_silu_follow_the_contract():
    torch.manual_seed(1)
    fw = quantize_fp8(torch.randn(96, 128) * 0.05)
    x = torch.randn(5, 128).to(torch.bfloat16)
    ref = (fw.scale[None, :] * (x.float() @ fw.q.view(torch.float8_e4m3fn).float().t()))
    y = ops.linear(x, fw)
    assert y.dtype == torch.bfloat16 and y.shape == (5, 96)
    # fp32 summation order differs between the two matmuls: allow one bf16 ulp
    assert torch.allclose(y.float(), ref.to(torch.bfloat16).float(), rtol=2 ** -7, atol=1e-6)
    out = torch.empty(5, 96, dtype=torch.bfloat16)
    assert ops.linear(x, fw, out=out) is out and torch.equal(out, y)
    s = ops.linear_silu(x, fw)
    g, u = y.float()[:, :48], y.float()[:, 48:]
    want = (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
    assert s.shape == (5, 48)
    assert torch.allclose(s.float(), want.float(), rtol=2 ** -6, atol=1e-6)
    assert torch.equal(s, ops.silu_and_mul(y))


def _engine(model, **kw):
    cfg = dict(model=model, device="cpu", max_model_len=256, max_num_seqs=8,
               max_num_batched_tokens=64, block_size=32, num_gpu_blocks=64, init_std=0.1,
               quantization="fp8")
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
            total += N * K + 4 * N
    return total


@pytest.mark.parametrize("model", ["tiny-qwen3", "tiny-llama"])
def test_quantized_engine_matches_dense_reference(model):
    eng = _engine(model)
    m = eng.runner.model
    assert m.quantized
    for lw in m.layers:
        for name in PROJ:
            assert isinstance(getattr(lw, name), Fp8Weight), name
    assert m.embed.dtype == torch.bfloat16 and m.lm_head.dtype == torch.bfloat16
    assert m.weight_bytes() == _formula_bytes(m)
    bf16 = DecoderLM(get_config(model), "cpu", max_model_len=256)
    saved = sum(getattr(lw, n).numel() - 4 * getattr(lw, n).shape[0]
                for lw in bf16.layers for n in PROJ)
    assert m.weight_bytes() == bf16.weight_bytes() - saved
    prompts = [list(range(5, 60)), [100, 101], [7, 8, 9] * 10]
    outs = eng.generate(None, SamplingParams(max_tokens=8, temperature=0, ignore_eos=True),
                        prompt_ids=prompts)
    for p, o in zip(prompts, outs):
        assert len(o.output_ids) == 8
        _check_teacher_forced(m, p, o.output_ids)


def _quantized_model(model, seed):
    m = DecoderLM(get_config(model), "cpu", seed=seed, max_model_len=256, init_std=0.15,
                  quantization="fp8")
    m.quantize_fp8()
    return m


def _save(sd, d):
    from safetensors.torch import save_file

    d.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    return str(d)


@pytest.mark.parametrize("model", ["tiny-qwen3", "tiny-llama"])
def test_fp8_checkpoint_round_trip_is_bit_exact(model, tmp_path):
    from aws_k8s_ansible_provisioner_amd.engine.weights import load_safetensors_dir

    src = _quantized_model(model, 11)
    sd = src.hf_state_dict()
    w = sd["model.layers.0.self_attn.k_proj.weight"]
    s = sd["model.layers.0.self_attn.k_proj.weight_scale"]
    assert w.dtype == torch.float8_e4m3fn
    assert s.dtype == torch.float32 and s.shape == (w.shape[0], 1)
    assert "model.layers.0.mlp.up_proj.weight_scale" in sd
    assert sd["model.embed_tokens.weight"].dtype == torch.bfloat16
    assert "model.embed_tokens.weight_scale" not in sd
    wdir = _save(sd, tmp_path / "ck")
    dst = _quantized_model(model, 99)
    assert not torch.equal(dst.layers[0].w_qkv.q, src.layers[0].w_qkv.q)
    loaded = load_safetensors_dir(wdir)
    loaded["model.layers.0.self_attn.q_proj.input_scale"] = torch.tensor(0.5)  # ignored
    dst.load_state_dict(loaded)
    for a, b in zip(src.layers, dst.layers):
        for name in PROJ:
            assert torch.equal(getattr(a, name).q, getattr(b, name).q), name
            assert torch.equal(getattr(a, name).scale, getattr(b, name).scale), name
    for p in PROMPTS:
        assert torch.equal(dense_logits(src, p), dense_logits(dst, p))


def test_plain_checkpoint_is_quantized_at_load():
    src = DecoderLM(get_config("tiny-llama"), "cpu", seed=3, max_model_len=256, init_std=0.15)
    dst = DecoderLM(get_config("tiny-llama"), "cpu", seed=4, max_model_len=256,
                    quantization="fp8")
    dst.load_state_dict(src.hf_state_dict())
    assert dst.quantized
    for a, b in zip(src.layers, dst.layers):
        for name in PROJ:
            assert isinstance(getattr(b, name), Fp8Weight)
            _quantizer_bound(getattr(b, name), getattr(a, name))


def test_per_tensor_scalar_scales_match_the_per_channel_file():
    """A per-tensor (scalar weight_scale) checkpoint and the same one with the scalar written
    out per channel load to the same logits."""
    torch.manual_seed(5)
    src = DecoderLM(get_config("tiny-qwen3"), "cpu", seed=21, max_model_len=256, init_std=0.15)
    plain = src.hf_state_dict()
    scalar, channel = dict(plain), dict(plain)
    for k, w in plain.items():
        if "_proj.weight" not in k:
            continue
        s = w.float().abs().max() / 448
        q = (w.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn)
        base = k[: -len(".weight")]
        scalar[k] = channel[k] = q
        scalar[base + ".weight_scale"] = s.reshape(())
        channel[base + ".weight_scale"] = s.expand(w.shape[0], 1).contiguous()
    a = DecoderLM(get_config("tiny-qwen3"), "cpu", seed=1, max_model_len=256, quantization="fp8")
    b = DecoderLM(get_config("tiny-qwen3"), "cpu", seed=2, max_model_len=256, quantization="fp8")
    a.load_state_dict(scalar)
    b.load_state_dict(channel)
    q0 = plain["model.layers.0.self_attn.q_proj.weight"].shape[0]
    assert torch.equal(a.layers[0].w_qkv.q[:q0].view(torch.float8_e4m3fn),
                       scalar["model.layers.0.self_attn.q_proj.weight"])  # no bf16 detour
    for p in PROMPTS:
        assert torch.equal(dense_logits(a, p), dense_logits(b, p))


def test_block_scaled_checkpoint_is_requantized_per_channel():
    torch.manual_seed(6)
    src = DecoderLM(get_config("tiny-llama"), "cpu", seed=31, max_model_len=256, init_std=0.15)
    sd = src.hf_state_dict()
    deq = {}
    for k in [k for k in sd if "_proj.weight" in k]:
        w = sd[k].float()
        N, K = w.shape
        nb, kb = -(-N // 128), -(-K // 128)
        pad = torch.zeros(nb * 128, kb * 128)
        pad[:N, :K] = w
        amax = pad.view(nb, 128, kb, 128).abs().amax((1, 3)).clamp_min(1e-12)
        s_inv = (amax / 448).float()
        full = s_inv.repeat_interleave(128, 0)[:N].repeat_interleave(128, 1)[:, :K]
        q = (w / full).clamp(-448, 448).to(torch.float8_e4m3fn)
        base = k[: -len(".weight")]
        sd[k] = q
        sd[base + ".weight_scale_inv"] = s_inv
        deq[base] = q.float() * full
    m = DecoderLM(get_config("tiny-llama"), "cpu", seed=32, max_model_len=256, quantization="fp8")
    m.load_state_dict(sd)
    lw, p = m.layers[1], "model.layers.1."
    qkv = torch.cat([deq[p + "self_attn.q_proj"], deq[p + "self_attn.k_proj"],
                     deq[p + "self_attn.v_proj"]], 0)
    _quantizer_bound(lw.w_qkv, qkv)
    _quantizer_bound(lw.w_o, deq[p + "self_attn.o_proj"])
    _quantizer_bound(lw.w_gate_up, torch.cat([deq[p + "mlp.gate_proj"], deq[p + "mlp.up_proj"]], 0))
    _quantizer_bound(lw.w_down, deq[p + "mlp.down_proj"])
    for name in PROJ:
        _no_nan_codes(getattr(lw, name).q)


def test_errors():
    src = _quantized_model("tiny-llama", 11)
    sd = src.hf_state_dict()
    bf16 = DecoderLM(get_config("tiny-llama"), "cpu", seed=1, max_model_len=256)
    with pytest.raises(ValueError, match="--quantization fp8"):
        bf16.load_state_dict(sd)
    with pytest.raises(ValueError, match="quantization"):
        EngineConfig(quantization="int4")
    with pytest.raises(ValueError, match="MoE"):
        _engine("tiny-mixtral")
    with pytest.raises(ValueError, match="MoE"):
        DecoderLM(get_config("tiny-qwen3-moe"), "cpu", max_model_len=256).quantize_fp8()


def test_config_reads_the_environment(monkeypatch):
    monkeypatch.delenv("AKAP_QUANTIZATION", raising=False)
    assert EngineConfig().quantization is None
    monkeypatch.setenv("AKAP_QUANTIZATION", "fp8")
    assert EngineConfig().quantization == "fp8"
    assert EngineConfig(quantization="none").quantization == "none"
    eng = _engine("tiny-llama", quantization="none")
    assert not eng.runner.model.quantized
    assert isinstance(eng.runner.model.layers[0].w_qkv, torch.Tensor)
    monkeypatch.setenv("AKAP_QUANTIZATION", "int4")
    with pytest.raises(ValueError):
        EngineConfig()


def test_server_flag():
    from aws_k8s_ansible_provisioner_amd.server.api_server import (engine_config_from_args,
                                                                    make_parser)

    ap = make_parser()
    assert engine_config_from_args(ap.parse_args(["--quantization", "fp8"])).quantization == "fp8"
    with pytest.raises(SystemExit):
        ap.parse_args(["--quantization", "int4"])


def test_server_with_quantization_fp8_serves_a_completion():
    from fastapi.testclient import TestClient

    from aws_k8s_ansible_provisioner_amd.server.api_server import (build_app,
                                                                    engine_config_from_args,
                                                                    make_parser)

    a = make_parser().parse_args(["--model", "tiny-qwen3", "--quantization", "fp8", "--device",
                                  "cpu", "--max-model-len", "256", "--max-num-seqs", "8",
                                  "--max-num-batched-tokens", "64", "--num-gpu-blocks", "128"])
    app, ae = build_app(engine_config_from_args(a))
    with TestClient(app) as c:
        r = c.post("/v1/completions", json={"prompt": [[5, 6, 7]], "max_tokens": 4,
                                            "temperature": 0, "ignore_eos": True})
        assert r.status_code == 200, r.text
        assert r.json()["usage"]["completion_tokens"] == 4


CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["ROOT"])
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.parallel.tp_worker import make_tp_engine
ecfg = EngineConfig(model=os.environ["MODEL"], device="cpu", max_model_len=256, max_num_seqs=8,
                    max_num_batched_tokens=32, block_size=32, num_gpu_blocks=96,
                    tensor_parallel_size=2, seed=77, load_format="safetensors",
                    weights_path=os.environ["WEIGHTS"], quantization="fp8")
eng, bc = make_tp_engine(ecfg, backend="gloo", log=lambda *a: None)
if eng is not None:
    from aws_k8s_ansible_provisioner_amd.ops.quant import Fp8Weight
    assert all(isinstance(getattr(l, n), Fp8Weight) for l in eng.runner.model.layers
               for n in ("w_qkv", "w_o", "w_gate_up", "w_down"))
    outs = eng.generate(None, SamplingParams(max_tokens=6, temperature=0, ignore_eos=True),
                        prompt_ids=json.loads(os.environ["PROMPTS"]))
    bc.shutdown()
    print("RESULT " + json.dumps([o.output_ids for o in outs]), flush=True)
"""


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_fp8_checkpoint_sharded_load_tp2(tmp_path):
    """One FP8 checkpoint loaded by two gloo ranks (q / scale sliced by rows for qkv and
    gate|up, q by columns for o and down): its tokens are near-argmax of the tp=1 quantized
    model's dense reference."""
    model = "tiny-llama"
    src = _quantized_model(model, 11)
    wdir = _save(src.hf_state_dict(), tmp_path / model)
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ROOT=ROOT, MODEL=model,
                   WEIGHTS=wdir, PROMPTS=json.dumps(PROMPTS))
        procs.append(subprocess.Popen([sys.executable, "-c", CHILD], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-3000:] for o in outs]
    tp_out = json.loads([l for l in outs[0][0].splitlines() if l.startswith("RESULT ")][0][7:])
    for p, out in zip(PROMPTS, tp_out):
        assert len(out) == 6
        logits = dense_logits(src, p + out).float()
        for i, tok in enumerate(out):
            row = logits[len(p) - 1 + i]
            gap = (row.max() - row[tok]).item() / (row.std().item() + 1e-6)
            assert gap <= 0.1, (i, tok, gap)
