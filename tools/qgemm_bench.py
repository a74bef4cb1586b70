"""Microbench of the FP8-weight decode GEMM (csrc/kernels/qgemm.hip) and the MXFP4-weight one
(csrc/kernels/q4gemm.hip) against the bf16 path they replace: ops.linear's tuned choice for the
shape (gemm_tuner.tune: hipBLASLt or the fastest hand-written bf16 variant), for the four dense projections of Qwen3-0.6B and of Llama-3-8B at
M in {1, 16, 64, 256}.

All three paths are timed on COLD weights: the launches rotate over copies of the weight worth
>= 768 MB (3x the 256 MB MALL, gemm_tuner._rot), inside one captured graph.

    python tools/qgemm_bench.py [--json qgemm.json] [--models qwen3-0.6b,llama-3-8b]
Prints one line per (shape, M): us and effective weight GB/s (weight bytes / time) of each."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from aws_k8s_ansible_provisioner_amd import ops  # noqa: E402
from aws_k8s_ansible_provisioner_amd.models.config import get_config  # noqa: E402
from aws_k8s_ansible_provisioner_amd.ops import gemm_tuner  # noqa: E402
from aws_k8s_ansible_provisioner_amd.ops.quant import quantize_fp8, quantize_mxfp4  # noqa: E402

MS = (1, 16, 64, 256)
COLD_BYTES = 768 << 20


def projections(model: str) -> list:
    c = get_config(model)
    d, F = c.hidden_size, c.intermediate_size
    return [("qkv", c.q_size + 2 * c.kv_size, d), ("o", d, c.q_size), ("gate_up", 2 * F, d),
            ("down", d, F)]


def copies(per_bytes: int) -> int:
    return max(4, -(-COLD_BYTES // per_bytes))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--models", default="qwen3-0.6b,llama-3-8b")
    a = ap.parse_args()
    ops.load_native(required=True)
    dev = "cuda"
    rows = []
    for model in a.models.split(","):
        for name, N, K in projections(model):
            src = torch.randn(N, K, device=dev) * 0.05
            wb = [src.to(torch.bfloat16).clone() for _ in range(copies(2 * N * K))]
            q = quantize_fp8(src)
            wq = [(q.q.clone(), q.scale.clone()) for _ in range(copies(N * K))]
            q4 = quantize_mxfp4(src)
            w4 = [(q4.q.clone(), q4.scale.clone()) for _ in range(copies(q4.nbytes))]
            del src
            for M in MS:
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                choice = gemm_tuner.tune(M, wb)
                t_b = gemm_tuner._timed(gemm_tuner._choice_launcher(choice, M, y, x, wb), len(wb))
                nq = len(wq)
                t_q = gemm_tuner._timed(
                    lambda i: torch.ops.akap.qgemm(y, x, wq[i % nq][0], wq[i % nq][1]), nq)
                n4 = len(w4)
                t_4 = gemm_tuner._timed(
                    lambda i: torch.ops.akap.q4gemm(y, x, w4[i % n4][0], w4[i % n4][1]), n4)
                r = {"model": model, "proj": name, "M": M, "N": N, "K": K,
                     "bf16": gemm_tuner._label(choice), "bf16_us": round(t_b, 2),
                     "fp8_us": round(t_q, 2),
                     "bf16_gbs": round(2 * N * K / t_b / 1e3, 1),
                     "fp8_gbs": round((N * K + 4 * N) / t_q / 1e3, 1),
                     "speedup": round(t_b / t_q, 3),
                     "mxfp4_us": round(t_4, 2), "mxfp4_gbs": round(q4.nbytes / t_4 / 1e3, 1),
                     "fp8_over_mxfp4": round(t_q / t_4, 3), "bf16_over_mxfp4": round(t_b / t_4, 3)}
                rows.append(r)
                print(json.dumps(r), flush=True)
                del x, y
            del wb, wq, w4
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
