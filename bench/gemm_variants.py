"""Every decode-GEMM variant on the model's real, cold per-layer weights (the tuner's harness:
one captured hipGraph rotating through all layers), printed per shape, so the tuner's choice
can be read against the whole candidate field.

python bench/gemm_variants.py [--model qwen3-0.6b] [--m 64,256] [--proj w_qkv,w_o]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aws_k8s_ansible_provisioner_amd import ops  # noqa: E402
from aws_k8s_ansible_provisioner_amd.models.config import get_config  # noqa: E402
from aws_k8s_ansible_provisioner_amd.models.transformer import DecoderLM  # noqa: E402
from aws_k8s_ansible_provisioner_amd.ops import gemm_tuner as gt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="qwen3-0.6b")
ap.add_argument("--m", default="64,256")
ap.add_argument("--proj", default="w_qkv,w_o,w_gate_up,w_down")
a = ap.parse_args()
ops.load_native(required=True)
m = DecoderLM(get_config(a.model), device="cuda")
L = len(m.layers)
for M in [int(v) for v in a.m.split(",")]:
    for name in a.proj.split(","):
        ws = [getattr(lw, name) for lw in m.layers]
        N, K = ws[0].shape
        x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16) * 0.1
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        gb = N * K * 2 / 1e9
        rows = [("hipblaslt", gt._timed(lambda i: torch.nn.functional.linear(x, ws[i % L]), L)),
                ("wgemm", gt._timed(lambda i: torch.ops.akap.wgemm(y, x, ws[i % L]), L))]
        # floor: the same launch with K cut to one 64-deep step (boundary + one round trip)
        w64 = [w[:, :64].contiguous() for w in ws]
        x64 = x[:, :64].contiguous()
        rows.append(("floor(K=64,g64)", gt._timed(
            gt.launcher(gt.Variant(bn=64), M, y, x64, w64), L)))
        for v in gt.variants(M, N, K, splits=(1, 2, 4, 8)):  # the tuner's own candidates
            rows.append((f"s{v.splitk}{v.name}", gt._timed(gt.launcher(v, M, y, x, ws), L)))
        rows.sort(key=lambda r: r[1])
        print(f"M={M:4d} {name:10s} N={N:6d} K={K:6d}: " + "  ".join(
            f"{n} {t:.1f}" for n, t in rows), flush=True)
        print(f"    best {rows[0][0]} {rows[0][1]:.1f} us = {gb / rows[0][1] * 1e6 / 1e3:.2f} TB/s "
              f"weights", flush=True)
