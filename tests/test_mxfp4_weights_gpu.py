"""MXFP4 weights on the GPU: csrc/kernels/q4gemm.hip (the weight-streaming W4A16 decode GEMM
and the dequantizer) against the contract formula
    Y[m,n] = bf16(sum_k float(X[m,k]) * e2m1(q[n,k]) * 2^(scale[n,k/32] - 127)),
the dequantize-into-scratch path of ops.linear for prefill-sized M, and the quantized engine
(hipGraph and eager decode, bf16 and fp8 KV cache) against the dense reference."""
import functools
import math

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import _runtime_loader, ops
from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
from aws_k8s_ansible_provisioner_amd.models.config import get_config
from aws_k8s_ansible_provisioner_amd.models.reference_forward import dense_logits
from aws_k8s_ansible_provisioner_amd.models.transformer import DecoderLM
from aws_k8s_ansible_provisioner_amd.ops.quant import Mxfp4Weight, quantize_mxfp4

pytestmark = pytest.mark.gpu

DEV = "cuda"
PROJ = ("w_qkv", "w_o", "w_gate_up", "w_down")
MS = [1, 16, 37, 64, 100, 128, 200, 256]
SHAPES = [(256, 256), (1000, 256), (1024, 3072), (4104, 1024)]
PAD = 16  # guard rows / columns around the output, pre-filled with NaN
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
LUT = torch.tensor(E2M1 + [-v for v in E2M1], dtype=torch.float64)


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


@functools.lru_cache(maxsize=None)
def _deq(w: Mxfp4Weight) -> torch.Tensor:
    """The dequantized matrix in fp64 on the CPU, written independently of Mxfp4Weight.float:
    element 2j of a row is the low nibble of byte j, element 2j + 1 the high nibble."""
    q = w.q.cpu()
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(w.shape).long()
    return LUT[codes] * torch.exp2(w.scale.cpu().double() - 127).repeat_interleave(32, dim=1)


def _contract(x, w: Mxfp4Weight):
    """The contract's sum in fp64 on the CPU."""
    return x.cpu().double() @ _deq(w).t()


@functools.lru_cache(maxsize=None)
def _randn_weight(N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    return quantize_mxfp4(torch.randn(N, K, generator=g) * 0.05)


@functools.lru_cache(maxsize=None)
def _adversarial_weight(N, K):
    """Nibbles uniform over all 16 codes (+-0 and +-6 included); scale codes 127 + U{-6..6},
    independent per block: a dropped, shifted or transposed block scale is off by a power of
    two, and swapped nibbles move every value."""
    g = torch.Generator().manual_seed(N * 13 + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    scale = (127 + torch.randint(-6, 7, (N, K // 32), generator=g)).to(torch.uint8)
    return Mxfp4Weight(q, scale)


@functools.lru_cache(maxsize=None)
def _x(M, K):
    g = torch.Generator().manual_seed(M * 31 + K)
    return torch.randn(M, K, generator=g).to(torch.bfloat16)


def _run_q4gemm_padded(x, w):
    """q4gemm into the interior of a NaN-filled buffer: returns the [M, N] result after
    checking that nothing outside it was stored."""
    M, N = x.shape[0], w.shape[0]
    buf = torch.full((M + 2 * PAD, N + 2 * PAD), float("nan"), device=DEV, dtype=torch.bfloat16)
    out = buf[PAD:PAD + M, PAD:PAD + N]
    wd = w.to(DEV)
    torch.ops.akap.q4gemm(out, x.to(DEV), wd.q, wd.scale)
    torch.cuda.synchronize()
    guard = buf.clone()
    guard[PAD:PAD + M, PAD:PAD + N] = float("nan")
    assert bool(guard.isnan().all()), "q4gemm stored outside its [M, N] tile"
    assert not bool(out.isnan().any())
    return out


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", MS)
def test_q4gemm_matches_the_contract(M, N, K):
    w, x = _randn_weight(N, K), _x(M, K)
    _close(_run_q4gemm_padded(x, w), _contract(x, w), **_tol(K))


@pytest.mark.parametrize("M,N,K", [(37, 1000, 256), (256, 264, 3072), (1, 256, 128)])
def test_q4gemm_adversarial_codes_and_scales(M, N, K):
    """These weights have an rms of ~3 * 2^(+-6), not the 0.05 the project's tolerance was
    written for, so the bound comes from the number formats instead.  Every product x * w is
    exact in fp32; what is left is the fp32 summation, at most (K - 1) 2^-24 sum_k |x w| for
    any order of K additions, and the one rounding of that sum s to bf16, at most half an ulp
    = 2^-8 |s| (8 significand bits, worst at the bottom of a binade).  So |y - ref| <=
    2^-8 |ref| + (1 + 2^-8) (K - 1) 2^-24 sum_k |x w|, which 2^-8 |ref| + 2^-23 K sum_k |x w|
    covers.  A wrong or missing block scale is off by a factor of two or more in a 32-deep
    block."""
    w, x = _adversarial_weight(N, K), _x(M, K)
    ref = _contract(x, w)
    mag = x.double().abs() @ _deq(w).abs().t()
    got = _run_q4gemm_padded(x, w).cpu().double()
    err = (got - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    worst = (err / lim.clamp_min(1e-300)).max().item()
    print(f"adversarial ({M}, {N}, {K}): max err / limit {worst:.3f}, max err {err.max():.4g}")
    assert bool((err <= lim).all()), f"max err / limit {worst:.3f}"


def _geometry(M, N, K):
    return _runtime_loader.contract().q4gemm_geometry(M, N, K)[:2]


# one shape per (bm, bn) tile q4gemm_geometry returns, K = 3072 for one of each row-tile
# height and for M = 256
EXACT_CASES = [(16, 264, 3072, (16, 16)), (32, 264, 3072, (32, 32)), (64, 264, 3072, (64, 32)),
               (256, 264, 3072, (64, 32)), (9, 4104, 512, (16, 32)), (16, 16392, 128, (16, 64)),
               (32, 16392, 128, (32, 64))]


@pytest.mark.parametrize("M,N,K,geom", EXACT_CASES)
def test_q4gemm_is_bit_exact_on_integer_inputs(M, N, K, geom):
    """x integers in [-2, 2], any codes, scale codes 127..130: every product is a multiple of
    0.5 and every partial sum is below 2 * 48 * 3072 = 2^18.2, so fp32 sums are exact in any
    order and the result is the fp64 sum rounded once to bf16."""
    assert _geometry(M, N, K) == geom
    g = torch.Generator().manual_seed(M * 5 + N + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    scale = torch.randint(127, 131, (N, K // 32), generator=g).to(torch.uint8)
    w = Mxfp4Weight(q, scale)
    x = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16)
    want = _contract(x, w).to(torch.bfloat16)
    got = _run_q4gemm_padded(x, w)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def test_q4gemm_is_deterministic_and_graph_capturable():
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
def test_dequant_mxfp4_is_bit_exact(N, K):
    w = _adversarial_weight(N, K)
    want = w.float().to(torch.bfloat16)
    assert torch.equal(want.double(), _deq(w))  # every value is exact in bf16
    wd = w.to(DEV)
    out = torch.empty(N, K, device=DEV, dtype=torch.bfloat16)
    torch.ops.akap.dequant_mxfp4(out, wd.q, wd.scale)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(ops.quant.dequant_mxfp4(wd).cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("M", [300, 2048])
def test_linear_prefill_path_through_the_shared_scratch(M):
    """M > 256: dequantize into the process-wide scratch + the bf16 GEMM.  Two different
    weights back to back reuse the scratch in stream order; both must be right.  The
    dequantized weights are exact in bf16, so the bf16 GEMM sees the contract's matrix."""
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


def test_predicate_and_binding_checks_raise():
    c = _runtime_loader.contract()
    for K in (256, 512, 1024, 2048, 3072, 4096, 14336):
        assert c.q4gemm_supported(1, 4096, K, K, 4096) and c.q4gemm_supported(256, 8, K, K, 8)
    assert not c.q4gemm_supported(c.Q4GEMM_MAX_M + 1, 256, 256, 256, 256)
    assert not c.q4gemm_supported(16, 256, 64, 64, 256)
    w = _randn_weight(256, 256).to(DEV)
    x = _x(16, 256).to(DEV)
    out = torch.empty(16, 256, device=DEV, dtype=torch.bfloat16)
    torch.ops.akap.q4gemm(out, x, w.q, w.scale)  # the valid call the cases below vary
    with pytest.raises(RuntimeError):
        torch.ops.akap.q4gemm(out, x.float(), w.q, w.scale)           # x dtype
    with pytest.raises(RuntimeError):
        torch.ops.akap.q4gemm(out, x, w.q.to(torch.int32), w.scale)   # weight dtype
    with pytest.raises(RuntimeError):
        torch.ops.akap.q4gemm(out, x, w.q, w.scale.float())           # scale dtype
    with pytest.raises(RuntimeError):
        torch.ops.akap.q4gemm(out, x, w.q, w.scale[:, :-1].contiguous())  # scale shape
    with pytest.raises(RuntimeError):
        torch.ops.akap.q4gemm(out, x, w.q, w.scale.reshape(-1))       # scale dims
    with pytest.raises(RuntimeError):
        torch.ops.akap.q4gemm(out[:, :248], x, w.q, w.scale)          # out shape
    w2 = _randn_weight(256, 512).to(DEV)
    with pytest.raises(RuntimeError):                                 # non-contiguous q
        torch.ops.akap.q4gemm(out, x, w2.q[:, :128], w.scale)
    xm = torch.zeros(16, 256 + 8, device=DEV, dtype=torch.bfloat16)[:, 4:260]
    assert xm.data_ptr() % 16 == 8 and xm.stride(0) % 8 == 0
    with pytest.raises(RuntimeError):
        torch.ops.akap.q4gemm(out, xm, w.q, w.scale)                  # misaligned x
    x300 = torch.zeros(300, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):                                 # M > 256
        torch.ops.akap.q4gemm(torch.empty(300, 256, device=DEV, dtype=torch.bfloat16), x300,
                              w.q, w.scale)
    w64 = _randn_weight(256, 64).to(DEV)
    with pytest.raises(RuntimeError):                                 # K below the minimum
        torch.ops.akap.q4gemm(out, x[:, :64].contiguous(), w64.q, w64.scale)
    with pytest.raises(RuntimeError):
        torch.ops.akap.dequant_mxfp4(out, w.q, w.scale[:, :-1].contiguous())  # scale shape
    with pytest.raises(RuntimeError):
        torch.ops.akap.dequant_mxfp4(out[:, :128], w.q, w.scale)      # out shape
    torch.cuda.synchronize()
    # K = 64 is a valid weight that q4gemm does not take: ops.linear dequantizes instead
    y = ops.linear(x[:, :64].contiguous(), w64)
    _close(y, _contract(x[:, :64], w64), **_tol(64))


def _engine(model, eager=False, **kw):
    cfg = dict(model=model, device="cuda", max_model_len=512, max_num_seqs=16,
               max_num_batched_tokens=128, block_size=32, num_gpu_blocks=128, init_std=0.1,
               enforce_eager=eager, cuda_graph_max_bs=16, quantization="mxfp4")
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
    assert m.quantized and m.quantization == "mxfp4"
    for lw in m.layers:
        for name in PROJ:
            assert isinstance(getattr(lw, name), Mxfp4Weight) and getattr(lw, name).is_cuda
    assert m.embed.dtype == torch.bfloat16 and m.lm_head.dtype == torch.bfloat16
    # each projection [N, K]: 2 N K bytes -> N K / 2 + N K / 32
    if build_bf16:
        bf16 = DecoderLM(get_config(model), "cpu", max_model_len=512)
        layers, total = bf16.layers, bf16.weight_bytes()
    else:  # large model: the same count from the quantized model's own shapes
        layers, total = m.layers, m.weight_bytes(as_bf16=True)
    proj = sum(getattr(lw, n).numel() for lw in layers for n in PROJ)
    assert proj > 0 and m.weight_bytes() == total - 2 * proj + proj // 2 + proj // 32


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
