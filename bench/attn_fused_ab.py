"""A/B in one process: decode attention on a ready q (plain kernel) vs the fused kernel that
also does q/k RMSNorm + RoPE + the new token's K/V write from the raw QKV projection, plus
the standalone qk_norm_rope_cache + plain attention pair.  Interleaved rounds, median.
Also the serving form with the K/V write left to the caller (write_kv=False), and the Qwen3-0.6B
gate|up GEMM (K 1024, N 6144, 28 rotating weights) with and without the K/V rider workgroups
that then do that write (csrc/kernels/kv_write.h), per gate|up variant that can carry them.

python bench/attn_fused_ab.py [--B 256] [--ctx 640]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aws_k8s_ansible_provisioner_amd import ops  # noqa: E402
from aws_k8s_ansible_provisioner_amd.ops.gemm_variant import Variant  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--ctx", type=int, default=640)
    ap.add_argument("--hq", type=int, default=16)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    ops.load_native(required=True)
    dev = "cuda"
    B, D, bs, Hq, Hkv = a.B, 128, 32, a.hq, a.hkv
    G = Hq // Hkv
    torch.manual_seed(0)
    lens = torch.randint(a.ctx - 128, a.ctx + 129, (B,), dtype=torch.int32)
    nb = [math.ceil(int(x) / bs) for x in lens]
    NB = sum(nb) + 8
    bt = torch.zeros(B, 4096 // bs, dtype=torch.int32)
    i = 0
    for s, n in enumerate(nb):  # sequential blocks, as the engine's allocator hands them out
        bt[s, :n] = torch.arange(i, i + n, dtype=torch.int32)
        i += n
    kc = torch.randn(NB, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
    vc = torch.randn(NB, Hkv, bs // 8, D, 8, dtype=torch.bfloat16, device=dev)
    q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=dev)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, dtype=torch.bfloat16, device=dev)
    out = torch.empty(B, Hq, D, dtype=torch.bfloat16, device=dev)
    pos = (lens - 1).to(torch.int64)
    slots = torch.tensor([int(bt[s, int(pos[s]) // bs]) * bs + int(pos[s]) % bs
                          for s in range(B)], dtype=torch.int64)
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(4096, dtype=torch.float32)[:, None] * inv[None, :]
    cos_sin = torch.cat([ang.cos(), ang.sin()], dim=-1).to(dev)
    qw = torch.ones(D, dtype=torch.bfloat16, device=dev)
    kw = torch.ones(D, dtype=torch.bfloat16, device=dev)
    bt, lens_d, pos_d, slots_d = bt.to(dev), lens.to(dev), pos.to(dev), slots.to(dev)
    ws = ops.decode_workspace(B, Hkv, G, int(os.environ.get("AB_WS_PARTS", "1")), dev)
    scale = 1 / math.sqrt(D)
    kv_bytes = int(lens.sum()) * Hkv * D * 2 * 2
    qbuf = torch.empty(B, Hq, D, dtype=torch.bfloat16, device=dev)

    def plain():
        ops.paged_attention_decode(out, q, kc, vc, bt, lens_d, G, scale, workspace=ws,
                                   num_parts=1, part_size=4096)

    def fused():
        ops.paged_attention_decode_fused(out, qkv, kc, vc, bt, lens_d, pos_d, slots_d, cos_sin,
                                         qw, kw, G, scale, 1e-6, workspace=ws, num_parts=1,
                                         part_size=4096)

    def split():
        ops.qk_norm_rope_cache(qkv, qbuf, kc, vc, pos_d, slots_d, cos_sin, qw, kw, Hq, Hkv, 1e-6,
                               True)
        ops.paged_attention_decode(out, qbuf, kc, vc, bt, lens_d, G, scale, workspace=ws,
                                   num_parts=1, part_size=4096)

    slots_none = torch.full_like(slots_d, -1)
    vtail = torch.zeros(B, Hkv, 8, D, dtype=torch.bfloat16, device=dev)
    tslot = torch.arange(B, dtype=torch.int32, device=dev)

    def fused_nowrite():  # the prologue without the new token's K/V writes (slot -1)
        ops.paged_attention_decode_fused(out, qkv, kc, vc, bt, lens_d, pos_d, slots_none,
                                         cos_sin, qw, kw, G, scale, 1e-6, workspace=ws,
                                         num_parts=1, part_size=4096)

    def fused_tail():  # the serving form: V written through the per-sequence V tail
        ops.paged_attention_decode_fused(out, qkv, kc, vc, bt, lens_d, pos_d, slots_d, cos_sin,
                                         qw, kw, G, scale, 1e-6, workspace=ws, num_parts=1,
                                         part_size=4096, v_tail=vtail, tail_slot=tslot)

    def plain_tail():  # ready q, partial last V group read from the tail (no writes)
        ops.paged_attention_decode(out, q, kc, vc, bt, lens_d, G, scale, workspace=ws,
                                   num_parts=1, part_size=4096, v_tail=vtail, tail_slot=tslot)

    def fused_tail_caller():  # serving form, the new token's K/V write left to the caller
        ops.paged_attention_decode_fused(out, qkv, kc, vc, bt, lens_d, pos_d, slots_d, cos_sin,
                                         qw, kw, G, scale, 1e-6, workspace=ws, num_parts=1,
                                         part_size=4096, v_tail=vtail, tail_slot=tslot,
                                         write_kv=False)

    variants = {"plain attention (q ready)": plain, "plain + V tail reads": plain_tail,
                "fused prologue attention": fused, "fused, no K/V write": fused_nowrite,
                "fused + V tail (serving)": fused_tail,
                "fused + V tail, caller writes": fused_tail_caller,
                "qk_norm_rope_cache + plain": split}
    # gate|up GEMM of Qwen3-0.6B at M = B, one weight per layer so they stream from HBM
    K_, N_, L_ = 1024, 6144, 28
    xg = torch.randn(B, K_, dtype=torch.bfloat16, device=dev) * 0.1
    wg = [torch.randn(N_, K_, dtype=torch.bfloat16, device=dev) * 0.05 for _ in range(L_)]
    yg = torch.empty(B, N_ // 2, dtype=torch.bfloat16, device=dev)
    ssg = torch.full((B,), float(K_), dtype=torch.float32, device=dev)
    w1 = torch.randn(64, 256, dtype=torch.bfloat16, device=dev)  # one tile column, 4 k-steps
    y1 = torch.empty(B, 32, dtype=torch.bfloat16, device=dev)
    turn = [0]
    gemm_keys = []

    def gemm_arm(v, riders, tiles=True):
        n = ops.kv_rider_blocks(B, N_, v, B, Hkv)
        kvw = ops.KvWrite(qkv, pos_d, slots_d, cos_sin, kw, kc, vc, vtail, tslot, Hq, 1e-6,
                          blocks=n) if riders else None

        def run():
            if tiles:
                turn[0] = (turn[0] + 1) % L_
                ops.dgemm(xg, wg[turn[0]], epi=ops.EPI_SILU, ss_in=ssg, out=yg, variant=v,
                          kv_write=kvw)
            else:  # the same riders behind a GEMM of 4 k-steps and one tile column
                ops.dgemm(xg[:, :256], w1, epi=ops.EPI_SILU, out=y1, variant=v, kv_write=kvw)
        return run

    for v in (Variant(bn=128, ns=6), Variant(pf=2)):
        n = ops.kv_rider_blocks(B, N_, v, B, Hkv)
        if n <= 0:
            continue
        for label, f in ((f"gate|up s1{v.name}", gemm_arm(v, False)),
                         (f"gate|up s1{v.name} + {n} riders", gemm_arm(v, True)),
                         (f"{n} riders, 4-k-step tiles s1{v.name}", gemm_arm(v, True, False))):
            variants[label] = f
            gemm_keys.append(label)
    graphs = {}
    for k, f in variants.items():
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            f()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(a.iters):
                f()
        graphs[k] = g
    res = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1000 / a.iters)
    for k, v in res.items():
        med = statistics.median(v)
        rate = "" if k in gemm_keys else f"  {kv_bytes / med / 1e6:5.2f} TB/s"
        print(f"B={B} ctx~{a.ctx} {k:38s} median {med:7.1f} us  min {min(v):7.1f} us  "
              f"max {max(v):7.1f} us{rate}", flush=True)


if __name__ == "__main__":
    main()
