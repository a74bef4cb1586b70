"""The fused expert FFN of one decode layer with FP8 expert weights (moe_qgemm.hip) against the
same block with bf16 weights (moe_dgemm.hip), in one process, on cold weights: every timed call
takes the next of L layer copies, L chosen so that one rotation streams more than 3x the
256 MB MALL even in fp8 (as gemm_tuner._rot does).

python bench/moe_qgemm_micro.py [--model mixtral|qwen3-30b-a3b] [--T 1,16,64,128,256]
                                [--out results.jsonl]

Prints, per T, microseconds per block for both weight types, the achieved weight GB/s (bytes
of the experts actually routed to, each counted once) and the ratio bf16 / fp8 (halving the
weight bytes bounds it at 2).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aws_k8s_ansible_provisioner_amd import ops  # noqa: E402
from aws_k8s_ansible_provisioner_amd.ops.quant import Fp8Experts, quantize_fp8_experts  # noqa: E402

SHAPES = {  # name: (E, top-k, d, F, default T list)
    "mixtral": (8, 2, 4096, 14336, "1,16,64,128,256"),
    "qwen3-30b-a3b": (128, 8, 2048, 768, "16,256"),
}
COLD_BYTES = 768 << 20


def timed(fn, n, windows=3):
    """us per call of fn(i), i < n: best of `windows` single replays of a captured graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1000.0 / n)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mixtral", choices=sorted(SHAPES))
    ap.add_argument("--T", default=None, help="comma-separated token counts")
    ap.add_argument("--out", default=None, help="append one JSON line per T to this file")
    a = ap.parse_args()
    E, K, d, F, ts = SHAPES[a.model]
    Ts = [int(t) for t in (a.T or ts).split(",")]
    ops.load_native(required=True)
    dev = "cuda"
    fp8_layer = 3 * E * F * d                      # code bytes of one layer's experts
    L = max(2, -(-COLD_BYTES // fp8_layer))
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = [torch.randn(E, 2 * F, d, device=dev, dtype=torch.bfloat16, generator=g) * 0.02]
    w2 = [torch.randn(E, d, F, device=dev, dtype=torch.bfloat16, generator=g) * 0.02]
    q13, q2 = [quantize_fp8_experts(w13[0])], [quantize_fp8_experts(w2[0])]
    for _ in range(L - 1):  # distinct memory is what matters to the timing, not the values
        w13.append(w13[0].clone())
        w2.append(w2[0].clone())
        q13.append(Fp8Experts(q13[0].q.clone(), q13[0].scale.clone()))
        q2.append(Fp8Experts(q2[0].q.clone(), q2[0].scale.clone()))
    print(f"{a.model}: E={E} top-{K} d={d} F={F}, {L} layer copies "
          f"(bf16 {2 * fp8_layer / 1e9:.2f} GB, fp8 {fp8_layer / 1e9:.2f} GB each)", flush=True)
    for T in Ts:
        h = torch.randn(T, d, device=dev, dtype=torch.bfloat16, generator=g)
        logits = torch.randn(T, E, device=dev, dtype=torch.bfloat16, generator=g)
        tw, ids = ops.moe_topk_softmax(logits, K)
        out = torch.empty(T, d, device=dev, dtype=torch.bfloat16)
        hit = int(ids.unique().numel())            # experts whose weights a call streams
        t_bf = timed(lambda i: ops.fused_moe(h, w13[i % L], w2[i % L], tw, ids, out=out), L)
        t_q = timed(lambda i: ops.fused_moe(h, q13[i % L], q2[i % L], tw, ids, out=out), L)
        n = T * K
        bm = ops.moe_tile_rows(n, E)
        rec = dict(model=a.model, T=T, experts_hit=hit, tile_rows=bm,
                   down_splitk=ops.moe_down_splitk(n, E, bm, F),
                   bf16_us=round(t_bf, 1), fp8_us=round(t_q, 1),
                   bf16_gbs=round(2 * 3 * hit * F * d / t_bf / 1e3, 1),
                   fp8_gbs=round(3 * hit * F * d / t_q / 1e3, 1),
                   ratio=round(t_bf / t_q, 3))
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
