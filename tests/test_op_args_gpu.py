"""A tensor on the wrong device, of the wrong dtype or too short is refused by the op glue
(csrc/ops.cpp through csrc/op_args.h) with a RuntimeError naming the op and the argument.

No case here can hand a bad pointer to a kernel: every call has a zero-row batch (T = 0, B = 0
or M = 0), and the launchers of these ops return before launching on an empty batch -- a check
that went missing fails its case without a kernel ever running.  The "short" cases are GPU
tensors one element short in an argument the empty launch does not reach.  The accessor's own
behaviour (alignment, strides, lengths at work sizes) is covered on the CPU by
tests/test_op_args.py; dgemm refuses M = 0 as unsupported after its operand checks, so it has
no accepted call here."""
import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
HQ = HKV = G = 1
EPS, SCALE = 1e-6, 0.1


@pytest.fixture(autouse=True, scope="module")
def _native():
    ops.load_native(required=True)


def _z(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def _cache():
    """One 32-token block, one KV head: K [NB, Hkv, BS, 128], V [NB, Hkv, BS/8, 128, 8]."""
    return {"k_cache": _z(1, HKV, 32, 128), "v_cache": _z(1, HKV, 4, 128, 8)}


def _split_kv():
    return {"part_m": _z(1, dtype=F32), "part_l": _z(1, dtype=F32), "part_o": _z(1, dtype=F32)}


# op -> its arguments in schema order (zero-row batch, smallest legal other dimensions)
ARGS = {
    "rmsnorm": lambda: {"out": _z(0, 128), "x": _z(0, 128), "w": _z(128), "eps": EPS},
    "qk_norm_rope_cache": lambda: {
        "qkv": _z(0, 384), "q_out": _z(0, HQ, 128), **_cache(), "positions": _z(0, dtype=I64),
        "slots": _z(0, dtype=I64), "cos_sin": _z(4, 128, dtype=F32), "q_w": _z(128),
        "k_w": _z(128), "Hq": HQ, "Hkv": HKV, "eps": EPS, "apply_rope": True, "decode": False,
        "v_tail": None, "tail_slot": None, "num_decode": 0, "q_rows": -1},
    "reshape_and_cache": lambda: {"k": _z(0, HKV, 128), "v": _z(0, HKV, 128), **_cache(),
                                  "slots": _z(0, dtype=I64)},
    "paged_attention_prefill": lambda: {
        "out": _z(0, HQ, 128), "q": _z(0, HQ, 128), **_cache(),
        "block_tables": _z(1, 1, dtype=I32), "seq_lens": _z(1, dtype=I32),
        "q_start": _z(2, dtype=I32), "tile_seq": _z(0, dtype=I32), "tile_row": _z(0, dtype=I32),
        "G": G, "scale": SCALE, "tile_rows": 128},
    "paged_attention_decode": lambda: {
        "out": _z(0, HQ, 128), "q": _z(0, HQ, 128), **_cache(),
        "block_tables": _z(0, 1, dtype=I32), "seq_lens": _z(0, dtype=I32), "q_start": None,
        **_split_kv(), "num_parts": 2, "part_size": 512, "G": G, "scale": SCALE,
        "v_tail": _z(1, HKV, 8, 128), "tail_slot": _z(0, dtype=I32)},
    "paged_attention_decode_fused": lambda: {
        "out": _z(0, HQ, 128), "qkv": _z(1, 384), **_cache(),
        "block_tables": _z(0, 1, dtype=I32), "seq_lens": _z(0, dtype=I32),
        "positions": _z(0, dtype=I64), "slots": _z(0, dtype=I64),
        "cos_sin": _z(4, 128, dtype=F32), "q_w": _z(128), "k_w": _z(128), **_split_kv(),
        "num_parts": 2, "part_size": 512, "G": G, "scale": SCALE, "eps": EPS,
        "v_tail": None, "tail_slot": None},
    "gemm": lambda: {"out": _z(0, 4), "x": _z(0, 8), "w": _z(4, 8), "ws": _z(1, dtype=F32),
                     "splitk": 2, "counters": _z(16, dtype=I32)},
    "dgemm": lambda: {"out": _z(0, 64), "x": _z(0, 256), "w": _z(64, 256),
                      "ws": _z(1, dtype=F32), "pro": 0, "splitk": 1, "pf": 2, "r": None,
                      "rout": None, "ln": None, "eps": EPS, "epi": 0,
                      "ss_in": _z(0, dtype=F32)},
    "qgemm": lambda: {"out": _z(0, 8), "x": _z(0, 64), "wq": _z(8, 64, dtype=torch.uint8),
                      "scale": _z(8, dtype=F32)},
    "sample": lambda: {
        "logits": _z(0, 8, dtype=F32), "temperature": _z(0, dtype=F32), "top_k": _z(0, dtype=I32),
        "top_p": _z(0, dtype=F32), "seeds": _z(0, dtype=I64), "steps": _z(0, dtype=I32),
        "out_tokens": _z(0, dtype=I64), "out_logprobs": _z(0, dtype=F32),
        "greedy_logprobs": False, "ws": _z(ops._contract().sample_ws_floats(0) + 1, dtype=F32),
        "tickets": _z(1, dtype=I32), "filtered": True},
    # its launcher returns early on an empty batch too (sampling.hip launch_argmax)
    "argmax": lambda: {"logits": _z(0, 8, dtype=F32), "out": _z(0, dtype=I64)},
}

CPU, SHORT = "cpu", "short"


def _offset_by_one(t):
    """The same shape one element into a larger allocation: a 2-byte-aligned base."""
    return torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape)


def _strided(t):
    return torch.zeros(t.shape[0], 2 * t.shape[1], dtype=t.dtype, device=DEV)[:, :t.shape[1]]


# (op, argument, what is wrong with it, the name the message gives it)
CASES = [
    ("rmsnorm", "x", CPU), ("rmsnorm", "w", CPU), ("rmsnorm", "out", CPU),
    ("rmsnorm", "w", F32), ("rmsnorm", "w", SHORT),
    ("qk_norm_rope_cache", "qkv", CPU), ("qk_norm_rope_cache", "slots", CPU),
    ("qk_norm_rope_cache", "positions", I32), ("qk_norm_rope_cache", "cos_sin", CPU),
    ("qk_norm_rope_cache", "k_w", F32), ("qk_norm_rope_cache", "q_w", SHORT),
    ("qk_norm_rope_cache", "v_cache", CPU), ("qk_norm_rope_cache", "q_out", CPU),
    ("qk_norm_rope_cache", "v_cache", lambda t: t.view(1, HKV, 32, 128)),
    ("reshape_and_cache", "slots", CPU), ("reshape_and_cache", "v", F32),
    ("reshape_and_cache", "v_cache", torch.uint8), ("reshape_and_cache", "k_cache", CPU),
    ("reshape_and_cache", "v_cache", lambda t: t.view(1, HKV, 32, 128)),
    ("paged_attention_prefill", "block_tables", CPU), ("paged_attention_prefill", "seq_lens", I64),
    ("paged_attention_prefill", "q_start", CPU), ("paged_attention_prefill", "q_start", SHORT),
    ("paged_attention_prefill", "tile_seq", CPU), ("paged_attention_prefill", "tile_row", I64),
    ("paged_attention_prefill", "out", CPU),
    ("paged_attention_decode", "seq_lens", CPU), ("paged_attention_decode", "block_tables", I64),
    ("paged_attention_decode", "part_l", CPU), ("paged_attention_decode", "part_m", I32),
    ("paged_attention_decode", "tail_slot", CPU), ("paged_attention_decode", "v_tail", F32),
    ("paged_attention_decode", "k_cache", CPU),
    ("paged_attention_decode_fused", "positions", CPU),
    ("paged_attention_decode_fused", "slots", I32), ("paged_attention_decode_fused", "cos_sin", CPU),
    ("paged_attention_decode_fused", "k_w", CPU), ("paged_attention_decode_fused", "part_o", CPU),
    # the union of the two raw-QKV check blocks: aligned rows and a contiguous rotary table
    ("paged_attention_decode_fused", "qkv", _offset_by_one),
    ("paged_attention_decode_fused", "cos_sin", _strided),
    ("gemm", "w", CPU), ("gemm", "out", F32), ("gemm", "ws", CPU, "workspace"),
    ("gemm", "counters", CPU), ("gemm", "counters", I64),
    ("dgemm", "w", CPU), ("dgemm", "out", CPU), ("dgemm", "x", F32), ("dgemm", "ss_in", CPU),
    ("qgemm", "wq", CPU), ("qgemm", "wq", I32), ("qgemm", "scale", CPU), ("qgemm", "x", F32),
    ("qgemm", "out", CPU),
    ("sample", "temperature", CPU), ("sample", "top_k", I64), ("sample", "top_p", CPU),
    ("sample", "seeds", CPU), ("sample", "steps", CPU), ("sample", "out_tokens", I32),
    ("sample", "ws", CPU, "workspace"), ("sample", "tickets", CPU), ("sample", "ws", I32, "workspace"),
    ("argmax", "out", CPU), ("argmax", "out", I32),
]


def _id(case):
    how = case[2]
    how = how if isinstance(how, str) else getattr(how, "__name__", str(how)).replace("torch.", "")
    return f"{case[0]}-{case[1]}-{how}"


@pytest.mark.parametrize("op", [op for op in ARGS if op != "dgemm"])
def test_valid_zero_row_call_is_accepted(op):
    getattr(torch.ops.akap, op)(*ARGS[op]().values())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bad_argument_is_refused_by_name(case):
    op, name, how = case[:3]
    label = case[3] if len(case) > 3 else name
    args = ARGS[op]()
    t = args[name]
    if how == CPU:
        args[name] = t.cpu()
    elif how == SHORT:
        args[name] = t[:-1]
    elif callable(how):
        args[name] = how(t)
    else:
        args[name] = t.to(how)
    with pytest.raises(RuntimeError, match=f"{op}: {label} "):
        getattr(torch.ops.akap, op)(*args.values())
