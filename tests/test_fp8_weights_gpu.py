"""FP8 (e4m3fn) weights on the GPU: csrc/kernels/qgemm.hip (the weight-streaming W8A16 decode
GEMM and the dequantizer) against the fp32 contract formula
    Y[m,n] = bf16(scale[n] * sum_k float(X[m,k]) * float(q[n,k])),
the dequantize-into-scratch path of ops.linear for prefill-sized M, and the quantized engine
(hipGraph and eager decode, bf16 and fp8 KV cache) against the dense reference."""
import functools
import math

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
from aws_k8s_ansible_provisioner_amd.models.config import get_config
from aws_k8s_ansible_provisioner_amd.models.reference_forward import dense_logits
from aws_k8s_ansible_provisioner_amd.models.transformer import DecoderLM
from aws_k8s_ansible_provisioner_amd.ops.quant import Fp8Weight, quantize_fp8

pytestmark = pytest.mark.gpu

DEV = "cuda"
PROJ = ("w_qkv", "w_o", "w_gate_up", "w_down")
MS = [1, 16, 37, 64, 100, 128, 200, 256]
SHAPES = [(256, 64), (1000, 256), (1024, 3072), (4104, 1024)]
PAD = 16  # guard rows / columns around the output, pre-filled with NaN


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _close(a, b, atol, rtol=0.0):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    assert bool((err <= lim).all()), f"max err {err.max().item():.4g} (atol {atol})"


def _tol(K):
    return dict(atol=0.02 * math.sqrt(K / 64), rtol=1e-2)  # the project's wgemm tolerance


def _contract(x, w: Fp8Weight):
    """The fp32 formula on the CPU (scale applied after the sum)."""
    q = w.q.cpu().view(torch.float8_e4m3fn).float()
    return w.scale.cpu()[None, :] * (x.cpu().float() @ q.t())


@functools.lru_cache(maxsize=None)
def _randn_weight(N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    return quantize_fp8(torch.randn(N, K, generator=g) * 0.05)


@functools.lru_cache(maxsize=None)
def _adversarial_weight(N, K):
    """Bytes uniform over the 254 finite codes (+-0, subnormals, +-448 included); scales
    0.05/100 * 2^U(-3,3): the finite codes' rms is ~100, and a 64x spread of scales exposes
    a dropped or mis-indexed scale."""
    g = torch.Generator().manual_seed(N * 13 + K)
    finite = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    q = finite[torch.randint(0, 254, (N, K), generator=g)]
    scale = (0.05 / 100) * torch.exp2(torch.rand(N, generator=g) * 6 - 3)
    return Fp8Weight(q, scale.float())


@functools.lru_cache(maxsize=None)
def _x(M, K):
    g = torch.Generator().manual_seed(M * 31 + K)
    return torch.randn(M, K, generator=g).to(torch.bfloat16)


def _run_qgemm_padded(x, w):
    """qgemm into the interior of a NaN-filled buffer: returns the [M, N] result after
    checking that nothing outside it was stored."""
    M, N = x.shape[0], w.shape[0]
    buf = torch.full((M + 2 * PAD, N + 2 * PAD), float("nan"), device=DEV, dtype=torch.bfloat16)
    out = buf[PAD:PAD + M, PAD:PAD + N]
    wd = w.to(DEV)
    torch.ops.akap.qgemm(out, x.to(DEV), wd.q, wd.scale)
    torch.cuda.synchronize()
    guard = buf.clone()
    guard[PAD:PAD + M, PAD:PAD + N] = float("nan")
    assert bool(guard.isnan().all()), "qgemm stored outside its [M, N] tile"
    assert not bool(out.isnan().any())
    return out


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_qgemm_matches_the_contract(M, N, K):
    w, x = _randn_weight(N, K), _x(M, K)
    _close(_run_qgemm_padded(x, w), _contract(x, w), **_tol(K))


@pytest.mark.parametrize("M,N,K", [(37, 1000, 256), (256, 264, 3072), (1, 256, 64)])
def test_qgemm_adversarial_codes_and_scales(M, N, K):
    w, x = _adversarial_weight(N, K), _x(M, K)
    _close(_run_qgemm_padded(x, w), _contract(x, w), **_tol(K))


def test_qgemm_is_deterministic_and_graph_capturable():
    M, N, K = 48, 1024, 3072
    w = _randn_weight(N, K).to(DEV)
    wide = torch.randn(M, K + 64, device=DEV).to(torch.bfloat16)
    x = wide[:, 8:8 + K]  # strided rows (a view of a wider buffer), 16-byte aligned
    assert x.stride(0) == K + 64
    eager = ops.linear(x, w)
    again = ops.linear(x, w)
    assert torch.equal(eager, again)
    _close(eager, _contract(x, w), **_tol(K))
    out = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.linear(x, w, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.linear(x, w, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("N,K", [(1000, 256), (264, 3072)])
def test_dequant_fp8_is_bit_exact(N, K):
    w = _adversarial_weight(N, K)
    want = (w.q.view(torch.float8_e4m3fn).float() * w.scale[:, None]).to(torch.bfloat16)
    wd = w.to(DEV)
    out = torch.empty(N, K, device=DEV, dtype=torch.bfloat16)
    torch.ops.akap.dequant_fp8(out, wd.q, wd.scale)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("M", [300, 2048])
def test_linear_prefill_path_through_the_shared_scratch(M):
    """M > 256: dequantize into the process-wide scratch + the bf16 GEMM.  Two different
    weights back to back reuse the scratch in stream order; both must be right.

    Weights are quantized randn * 0.05, the distribution the tolerance was written for (atol
    = 5 % of the output rms sqrt(K) * 0.05).  This path rounds the dequantized weights to bf16
    (relative error up to 2^-9 per weight, ~0.2 % of the output rms per sigma); with the
    adversarial scales (weight rms up to 0.4, atol = 0.6 % of the output rms) that rounding
    alone is 1 element in 540,672 outside the tolerance at M = 2048 (err / limit 1.18, the
    same with the fp32 matmul of the bf16-rounded weights on the CPU), so those weights
    check the dequantizer bit for bit above and qgemm, which never rounds the weights."""
    wa, wb = _randn_weight(1000, 256), _randn_weight(264, 3072)
    xa, xb = _x(M, 256), _x(M, 3072)
    ya = ops.linear(xa.to(DEV), wa.to(DEV))
    yb = ops.linear(xb.to(DEV), wb.to(DEV))
    ya2 = ops.linear(xa.to(DEV), wa.to(DEV))
    torch.cuda.synchronize()
    _close(ya, _contract(xa, wa), **_tol(256))
    _close(yb, _contract(xb, wb), **_tol(3072))
    assert torch.equal(ya, ya2)
    ws = _randn_weight(512, 256).to(DEV)  # [gate; up], F = 256
    s = ops.linear_silu(xa.to(DEV), ws)
    assert s.shape == (M, 256)
    assert torch.equal(s, ops.silu_and_mul(ops.linear(xa.to(DEV), ws)))


def test_binding_checks_raise():
    w = _randn_weight(256, 64).to(DEV)
    x = _x(16, 64).to(DEV)
    out = torch.empty(16, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        torch.ops.akap.qgemm(out, x.float(), w.q, w.scale)        # x dtype
    with pytest.raises(RuntimeError):
        torch.ops.akap.qgemm(out, x, w.q, w.scale[:-1])           # scale shape
    with pytest.raises(RuntimeError):
        torch.ops.akap.qgemm(out[:, :248], x, w.q, w.scale)       # out shape
    with pytest.raises(RuntimeError):
        torch.ops.akap.qgemm(out, x, w.q.to(torch.int32), w.scale)  # weight dtype
    with pytest.raises(RuntimeError):
        torch.ops.akap.dequant_fp8(out, w.q, w.scale)             # out shape


def _engine(model, eager=False, **kw):
    cfg = dict(model=model, device="cuda", max_model_len=512, max_num_seqs=16,
               max_num_batched_tokens=128, block_size=32, num_gpu_blocks=128, init_std=0.1,
               enforce_eager=eager, cuda_graph_max_bs=16, quantization="fp8")
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), log=lambda *a: None)


def _check_teacher_forced(eng, prompt, out, tol=0.15):
    logits = dense_logits(eng.runner.model, list(prompt) + list(out)).float().cpu()
    for i, tok in enumerate(out):
        row = logits[len(prompt) - 1 + i]
        gap = (row.max() - row[tok]).item() / (row.std().item() + 1e-6)
        assert gap <= tol, f"step {i}: token {tok} is {gap:.3f} std below the argmax"


def _check_quantized(eng, model, build_bf16=True):
    m = eng.runner.model
    assert m.quantized
    for lw in m.layers:
        for name in PROJ:
            assert isinstance(getattr(lw, name), Fp8Weight) and getattr(lw, name).is_cuda
    assert m.embed.dtype == torch.bfloat16 and m.lm_head.dtype == torch.bfloat16
    # each projection [N, K]: 2 N K bytes -> N K + 4 N
    if build_bf16:
        bf16 = DecoderLM(get_config(model), "cpu", max_model_len=512)
        layers, total = bf16.layers, bf16.weight_bytes()
    else:  # large model: the same count from the quantized model's own shapes
        layers, total = m.layers, m.weight_bytes(as_bf16=True)
    saved = sum(getattr(lw, n).numel() - 4 * getattr(lw, n).shape[0]
                for lw in layers for n in PROJ)
    assert saved > 0 and m.weight_bytes() == total - saved


@pytest.mark.parametrize("model", ["tiny-qwen3", "tiny-llama"])
@pytest.mark.parametrize("eager", [False, True])
def test_quantized_engine_matches_dense_reference(model, eager):
    eng = _engine(model, eager)
    _check_quantized(eng, model)
    if not eager:
        assert eng.runner.graphs, "decode graphs were not captured"
    prompts = [list(range(5, 90)), [100, 101], [7, 8, 9] * 30, list(range(300, 340))]
    outs = eng.generate(None, SamplingParams(max_tokens=12, temperature=0, ignore_eos=True),
                        prompt_ids=prompts)
    for p, o in zip(prompts, outs):
        assert len(o.output_ids) == 12
        _check_teacher_forced(eng, p, o.output_ids)


@pytest.mark.parametrize("model", ["tiny-qwen3", "tiny-llama"])
def test_quantized_engine_with_fp8_kv_cache(model):
    eng = _engine(model, kv_cache_dtype="fp8")
    assert eng.runner.kv.dtype == torch.uint8 and eng.runner.graphs
    prompts = [list(range(3, 80)), [17] * 33 + [5, 6, 7]]
    outs = eng.generate(None, SamplingParams(max_tokens=10, temperature=0, ignore_eos=True),
                        prompt_ids=prompts)
    for p, o in zip(prompts, outs):
        assert len(o.output_ids) == 10
        _check_teacher_forced(eng, p, o.output_ids, tol=0.6)


def test_quantized_qwen3_0_6b_shapes():
    eng = _engine("qwen3-0.6b", max_model_len=256, num_gpu_blocks=64, init_std=0.02)
    _check_quantized(eng, "qwen3-0.6b", build_bf16=False)
    assert eng.runner.graphs, "decode graphs were not captured"
    prompts = [list(range(1000, 1100)), list(range(50, 60))]
    outs = eng.generate(None, SamplingParams(max_tokens=3, temperature=0, ignore_eos=True),
                        prompt_ids=prompts)
    for p, o in zip(prompts, outs):
        _check_teacher_forced(eng, p, o.output_ids, tol=0.2)
