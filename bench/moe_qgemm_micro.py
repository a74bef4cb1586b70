"""The fused expert FFN of one decode layer with FP8 (moe_qgemm.hip) and MXFP4 (moe_q4gemm.hip)
expert weights against the same block with bf16 weights (moe_dgemm.hip), in one process, on
cold weights: every timed call takes the next of L layer copies, L chosen so that one rotation
streams more than 3x the 256 MB MALL even in mxfp4 (as gemm_tuner._rot does).

python bench/moe_qgemm_micro.py [--model mixtral|qwen3-30b-a3b] [--T 1,16,64,128,256]
                                [--rounds 3] [--rings 1,2,4] [--out results.jsonl]

The three weight types are timed in alternation, `--rounds` times, and the best round of each
is kept.  Prints, per T, microseconds per block for each weight type, the achieved weight GB/s
(bytes of the experts actually routed to, each counted once) and the ratios bf16 / fp8 and
bf16 / mxfp4 (the weight bytes bound them at 2 and 3.76).  `--rings` also times the mxfp4 block
with moe_q4gemm's load ring capped at each given depth (mxfp4_ring_us).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aws_k8s_ansible_provisioner_amd import ops  # noqa: E402
from aws_k8s_ansible_provisioner_amd.ops.quant import (Fp8Experts, Mxfp4Experts,  # noqa: E402
                                                       quantize_fp8_experts,
                                                       quantize_mxfp4_experts)

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
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds, best kept")
    ap.add_argument("--rings", default="", help="also time mxfp4 with the ring capped at these")
    ap.add_argument("--out", default=None, help="append one JSON line per T to this file")
    a = ap.parse_args()
    E, K, d, F, ts = SHAPES[a.model]
    Ts = [int(t) for t in (a.T or ts).split(",")]
    ops.load_native(required=True)
    dev = "cuda"
    fp8_layer = 3 * E * F * d                      # code bytes of one layer's experts
    mx_layer = fp8_layer // 2 + fp8_layer // 32    # codes + block scales
    L = max(2, -(-COLD_BYTES // mx_layer))
    rings = [int(r) for r in a.rings.split(",") if r]
    g = torch.Generator(device=dev).manual_seed(0)
    w13 = [torch.randn(E, 2 * F, d, device=dev, dtype=torch.bfloat16, generator=g) * 0.02]
    w2 = [torch.randn(E, d, F, device=dev, dtype=torch.bfloat16, generator=g) * 0.02]
    q13, q2 = [quantize_fp8_experts(w13[0])], [quantize_fp8_experts(w2[0])]
    m13, m2 = [quantize_mxfp4_experts(w13[0])], [quantize_mxfp4_experts(w2[0])]
    for _ in range(L - 1):  # distinct memory is what matters to the timing, not the values
        w13.append(w13[0].clone())
        w2.append(w2[0].clone())
        q13.append(Fp8Experts(q13[0].q.clone(), q13[0].scale.clone()))
        q2.append(Fp8Experts(q2[0].q.clone(), q2[0].scale.clone()))
        m13.append(Mxfp4Experts(m13[0].q.clone(), m13[0].scale.clone(), check=False))
        m2.append(Mxfp4Experts(m2[0].q.clone(), m2[0].scale.clone(), check=False))
    print(f"{a.model}: E={E} top-{K} d={d} F={F}, {L} layer copies "
          f"(bf16 {2 * fp8_layer / 1e9:.2f} GB, fp8 {fp8_layer / 1e9:.2f} GB, mxfp4 "
          f"{mx_layer / 1e9:.2f} GB each)", flush=True)
    full_ring = ops._moe_qpf
    for T in Ts:
        h = torch.randn(T, d, device=dev, dtype=torch.bfloat16, generator=g)
        logits = torch.randn(T, E, device=dev, dtype=torch.bfloat16, generator=g)
        tw, ids = ops.moe_topk_softmax(logits, K)
        out = torch.empty(T, d, device=dev, dtype=torch.bfloat16)
        hit = int(ids.unique().numel())            # experts whose weights a call streams
        t_bf = t_q = t_m = float("inf")
        t_ring = {r: float("inf") for r in rings}
        for _ in range(a.rounds):
            t_bf = min(t_bf, timed(
                lambda i: ops.fused_moe(h, w13[i % L], w2[i % L], tw, ids, out=out), L))
            t_q = min(t_q, timed(
                lambda i: ops.fused_moe(h, q13[i % L], q2[i % L], tw, ids, out=out), L))
            t_m = min(t_m, timed(
                lambda i: ops.fused_moe(h, m13[i % L], m2[i % L], tw, ids, out=out), L))
            for r in rings:   # the ring depth is chosen at capture time
                ops._moe_qpf = lambda k, r=r: min(r, full_ring(k))
                try:
                    t_ring[r] = min(t_ring[r], timed(
                        lambda i: ops.fused_moe(h, m13[i % L], m2[i % L], tw, ids, out=out), L))
                finally:
                    ops._moe_qpf = full_ring
        n = T * K
        bm = ops.moe_tile_rows(n, E)
        rec = dict(model=a.model, T=T, experts_hit=hit, tile_rows=bm,
                   down_splitk=ops.moe_down_splitk(n, E, bm, F),
                   bf16_us=round(t_bf, 1), fp8_us=round(t_q, 1), mxfp4_us=round(t_m, 1),
                   bf16_gbs=round(2 * 3 * hit * F * d / t_bf / 1e3, 1),
                   fp8_gbs=round(3 * hit * F * d / t_q / 1e3, 1),
                   mxfp4_gbs=round(3 * hit * F * d * (0.5 + 1 / 32) / t_m / 1e3, 1),
                   ratio=round(t_bf / t_q, 3), ratio_mxfp4=round(t_bf / t_m, 3),
                   mxfp4_vs_fp8=round(t_q / t_m, 3))
        if rings:
            rec["mxfp4_ring_us"] = {str(r): round(t, 1) for r, t in t_ring.items()}
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
