#!/usr/bin/env python3
"""Serving benchmark: output tok/s + p50 TTFT (BASELINE.json headline) on MI355X.

One "step" = one WAVE of a fixed synthetic serving workload per GPU: `--num-requests`
requests (random token ids, `--input-len` prompt tokens, exactly `--output-len`
generated tokens, ignore_eos) all submitted at t=0 to the continuous-batching engine
and served to completion (chunked prefill + hipGraph decode).  Every wave uses fresh
random prompts, so prefix caching gets no hits.

Multi-GPU (torchrun, one process per GPU): every rank serves its own wave on its own
GPU -- a data-parallel replica, exactly how the gateway scales the deployment (weak
scaling: per-GPU work is fixed).  Ranks are synchronised with barriers around the K
timed waves; value = total output tokens of all ranks / max rank wall time.

--arrival-rate R: online serving instead of the t=0 burst -- requests arrive as a Poisson
process at R req/s (streaming, so every token is timestamped) and the line also reports
p50/p99 TTFT, TPOT (per-request mean inter-token time) and p99 inter-token latency; with
--no-mixed-batching the prefill-first policy is measured for comparison.

--mode pd: disaggregated prefill/decode -- ranks [0, N) prefill (N = --pd-prefill-ranks,
default W/2), [N, W) decode; each request's KV moves prefill->decode by a hipIpc pull of
the prefill engine's cache (one kv_pull launch per hand-off message; GPU default) or a
packed send/recv (parallel/pd_driver.py); TTFT is measured on the decode side (includes
the hand-off).

A plain run (`--gpus 1 --steps K --warmup W`) builds the engine, runs W warm-up and K timed
waves and prints the line; everything else is behind an option of its own.  --dump-outputs
DIR: rank 0 also writes the two leading ids its last timed wave generated for every request
(DIR/leading_token_ids.npy; dump_outputs says why those).

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="qwen3-0.6b")
    ap.add_argument("--num-requests", type=int, default=256)
    ap.add_argument("--input-len", type=int, default=512)
    ap.add_argument("--output-len", type=int, default=256)
    ap.add_argument("--max-num-seqs", type=int, default=256)
    ap.add_argument("--max-num-batched-tokens", type=int, default=16384)
    ap.add_argument("--block-size", type=int, default=32)
    ap.add_argument("--max-model-len", type=int, default=2048)
    ap.add_argument("--num-gpu-blocks", type=int, default=0,
                    help="KV cache blocks per engine (0: sized from free memory)")
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--enforce-eager", action="store_true")
    ap.add_argument("--kv-cache-dtype", default="auto", choices=["auto", "fp8"],
                    help="fp8 = e4m3 KV cache (NOT the headline config: bf16 KV like the "
                         "reference's vLLM default)")
    ap.add_argument("--device", default="auto")
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree: with --tp WORLD_SIZE the whole job is ONE "
                         "engine replica (Llama-3-70B TP=8 config; Mixtral EP with "
                         "AKAP_MOE_MODE=ep)")
    ap.add_argument("--mode", default="mono", choices=["mono", "pd"],
                    help="mono: every rank a monolithic replica (DP); pd: ranks [0,N) prefill, "
                         "[N,W) decode, KV by hipIpc pull or send/recv (Llama-3-8B disagg config)")
    ap.add_argument("--pd-push", default="auto", choices=["auto", "chunked", "whole"],
                    help="--mode pd: stream each prompt's KV chunk by chunk while the prefill "
                         "continues, or hand the whole prompt over at its end.  auto: chunked "
                         "on RCCL, whole on a host-staged gloo channel, where the transfer is "
                         "the bottleneck and per-chunk sends only add overhead "
                         "(profiles/r3_pd_push_gpu_gloo.log)")
    ap.add_argument("--pd-prefill-ranks", type=int, default=0,
                    help="--mode pd: N prefill ranks (the other W-N decode; W-N a multiple of N; "
                         "default W/2, i.e. 1:1 pairs)")
    ap.add_argument("--kv-transport", default="auto", choices=["auto", "ipc", "p2p"],
                    help="--mode pd: hipIpc pull of the prefill cache (GPU default) or packed "
                         "send/recv over the process group")
    ap.add_argument("--dist-backend", default=None,
                    help="override (gloo = single-GPU rehearsal of the multi-rank paths)")
    ap.add_argument("--arrival-rate", type=float, default=0.0,
                    help="Poisson arrivals at this many requests/s (0 = all at t=0)")
    ap.add_argument("--no-mixed-batching", action="store_true",
                    help="prefill-first scheduling (decodes stall while a prefill runs)")
    ap.add_argument("--torch-profile", action="store_true",
                    help="after timing, one more wave under torch.profiler; rank 0 prints the "
                         "kernel table")
    ap.add_argument("--profile-steps", type=int, default=0,
                    help="extra untimed waves run after timing (for rocprofv3 captures)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed waves, rank 0 writes the two leading token ids its last "
                         "timed wave generated for every request to DIR/leading_token_ids.npy "
                         "(float64, submission order); prompts and weights are seeded, so the "
                         "inputs are the same every run (not with --mode pd)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline figure (none today)")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64 << 20
# ids kept per request: the prefill's argmax and the first decode step's
DUMP_LEADING = 2


def dump_outputs(path: str, rows: list) -> None:
    """Write the leading generated ids of every request of one wave as
    DIR/leading_token_ids.npy: float64 [requests, DUMP_LEADING], in submission order, -1 where
    a request generated fewer.  Column 0 is the argmax of the request's prefill, column 1 the
    output of its first decode step (decode GEMM chain, paged decode attention, sampler) on
    that fixed context.  Past 64 MB a fixed, seeded sample of the requests (in order) is
    written instead.

    Why not every id: the dump is there to compare runs and builds, so it holds what is a
    function of the seeded inputs.  From the third id on a row is not: the fused decode GEMM
    epilogues sum the next RMSNorm's squares with fp32 atomics (csrc/kernels/dgemm.hip), in
    whatever order the workgroups arrive, and random-init weights soon generate repeating ids
    with near-flat logits, where that last-bit difference flips a greedy near-tie in about
    1 % of the rows per step; the rest of such a row follows the flipped id.  Measured on
    MI355X over 7 pairs of runs of one build: the two leading ids agreed in all 256 requests
    of every pair, the earliest difference was in the third id, whole rows agreed in 49-68 of
    256 (in all 256 with AKAP_FUSED_GEMM=0, at 2 % less throughput)."""
    lead = [[float(x) for x in r[:DUMP_LEADING]] + [-1.0] * (DUMP_LEADING - len(r[:DUMP_LEADING]))
            for r in rows]
    keep = max(1, DUMP_LIMIT_BYTES // (8 * DUMP_LEADING))
    if len(lead) > keep:
        pick = np.sort(np.random.default_rng(0).choice(len(lead), size=keep, replace=False))
        lead = [lead[i] for i in pick]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "leading_token_ids.npy"),
            np.asarray(lead, dtype=np.float64).reshape(len(lead), DUMP_LEADING))


def physical_devices(devs: list) -> int:
    """Distinct GPUs among the ranks' (host, device) ids (None = a CPU rank)."""
    return len({d for d in devs if d is not None})


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(a) -> int | None:
    """`python bench.py --gpus N` with N > 1 and no launcher: start the N ranks ourselves
    (torch.distributed.run as a CHILD process, one rank per GPU on 127.0.0.1 -- before this
    process touches the GPU, and never by exec) and return its exit code.  None: this
    process is already a rank (WORLD_SIZE set) or N == 1.  A GPU job asking for more GPUs
    than the node shows is refused (exit 2) instead of silently running fewer ranks; ranks
    sharing one GPU must say so with --dist-backend gloo (the single-GPU rehearsal)."""
    if "WORLD_SIZE" in os.environ or a.gpus <= 1:
        return None
    if a.device != "cpu":
        import torch

        ndev = torch.cuda.device_count()  # counts devices without initialising HIP
        if ndev and ndev < a.gpus and a.dist_backend != "gloo":
            print(f"error: --gpus {a.gpus} but only {ndev} GPU(s) are visible",
                  file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] launching {a.gpus} ranks: {' '.join(cmd[1:])}", file=sys.stderr, flush=True)
    import subprocess

    return subprocess.call(cmd)


def main() -> int:
    a = parse()
    if a.mode == "pd" and a.dump_outputs:
        print("error: --dump-outputs: the P/D driver returns token counts, not ids",
              file=sys.stderr)
        return 2
    rc = self_launch(a)
    if rc is not None:
        return rc
    if os.environ.get("AKAP_BENCH_STACKS"):
        # diagnostics: every N seconds, every thread's Python stack to stderr
        import faulthandler

        faulthandler.dump_traceback_later(float(os.environ["AKAP_BENCH_STACKS"]), repeat=True)
    import torch
    import torch.distributed as dist

    from aws_k8s_ansible_provisioner_amd.engine.config import EngineConfig, SamplingParams
    from aws_k8s_ansible_provisioner_amd.engine.llm_engine import LLMEngine
    from aws_k8s_ansible_provisioner_amd.models.config import get_config

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world != a.gpus and world > 1:
        print(f"warning: WORLD_SIZE={world} != --gpus {a.gpus}", file=sys.stderr)
    if a.gpus > 1 and world == 1:
        print(f"error: --gpus {a.gpus} in a one-rank job", file=sys.stderr)
        return 2
    gpu = torch.cuda.is_available() and a.device != "cpu"
    shared_ranks = 1
    if gpu:
        # more ranks than GPUs only in the single-GPU gloo rehearsal: share the device
        ndev = max(1, torch.cuda.device_count())
        shared_ranks = max(1, -(-world // ndev)) if world > ndev else 1
        local = local % ndev
        torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = a.dist_backend or ("nccl" if gpu else "gloo")
        kw = {"device_id": torch.device("cuda", local)} if (gpu and backend == "nccl") else {}
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    # physical devices behind the ranks: (host, device index) of every rank, de-duplicated --
    # a single-GPU rehearsal of a multi-rank layout (ranks sharing one device) is 1 GPU
    dev_id = (socket.gethostname(), local) if gpu else None
    devs = [dev_id]
    if world > 1:
        devs = [None] * world
        dist.all_gather_object(devs, dev_id)
    n_dev = physical_devices(devs)
    pd = a.mode == "pd"
    n_pre = 0
    if pd:
        from aws_k8s_ansible_provisioner_amd.parallel.pd_driver import pd_layout

        try:
            n_pre, _ = pd_layout(world, a.pd_prefill_ranks or None)
        except ValueError as e:
            print(f"error: --mode pd: {e}", file=sys.stderr)
            return 2
    is_prefill = pd and rank < n_pre

    mcfg = get_config(a.model)
    ecfg = EngineConfig(model=a.model, max_model_len=a.max_model_len,
                        max_num_seqs=a.max_num_seqs,
                        max_num_batched_tokens=a.max_num_batched_tokens,
                        block_size=a.block_size, enforce_eager=a.enforce_eager,
                        device="cuda" if gpu else "cpu",
                        seed=1234 if pd else 1234 + rank,  # P/D ranks: the same weights
                        num_gpu_blocks=(a.num_gpu_blocks or None) if gpu else 512,
                        kv_role=("prefill" if is_prefill else "decode") if pd else "both",
                        kv_cache_dtype=a.kv_cache_dtype,
                        mixed_batching=not a.no_mixed_batching,
                        # ranks sharing one GPU (single-GPU gloo rehearsal) split its memory.
                        # No P/D cache cap: the round-5 hipIpc import hang of 79-101 GiB peer
                        # caches was the bundled runtime's bit-31 allocation-size bug, and the
                        # KV segments are now sized around it (models.transformer.
                        # ipc_safe_alloc_bytes, profiles/r6_ipc_import_sweep.md)
                        gpu_memory_utilization=0.90 / max(1, shared_ranks))
    log = (lambda *x: print(*x, file=sys.stderr, flush=True)) if rank == 0 else (lambda *x: None)
    tp_bc = None
    if a.tp > 1:
        if a.tp != world or pd:
            print("error: --tp must equal WORLD_SIZE (one TP replica per job), no --mode pd",
                  file=sys.stderr)
            return 2
        from aws_k8s_ansible_provisioner_amd.parallel.tp_worker import make_tp_engine

        ecfg.tensor_parallel_size = a.tp
        ecfg.seed = 1234
        if gpu and dist.get_backend() == "gloo":
            # ranks sharing one GPU over a gloo control plane: the decode graphs' collectives
            # must be the IPC kernels (a gloo collective cannot be captured)
            os.environ.setdefault("AKAP_CUSTOM_AR_GLOO", "1")
        eng, tp_bc = make_tp_engine(ecfg, log=log)
        if eng is None:  # ranks != 0 mirrored every step until rank 0 shut the group down
            return 0
    else:
        eng = LLMEngine(ecfg, mcfg, log=log)
    sp = SamplingParams(max_tokens=a.output_len, temperature=a.temperature, ignore_eos=True)
    rng = np.random.default_rng(1000 + rank)
    vocab_hi = min(mcfg.vocab_size, 150000)
    pair = None
    if pd:
        from aws_k8s_ansible_provisioner_amd.parallel.pd_driver import PDPair

        ctrl = dist.new_group(backend="gloo")  # small metadata messages on the host
        transport = None if a.kv_transport == "auto" else a.kv_transport
        pair = PDPair(eng, rank, world, ctrl_group=ctrl, data_group=None,
                      prefill_ranks=n_pre, transport=transport)

    lat = {"itl": [], "tpot": []}

    def online_wave():
        """Poisson arrivals; every token event timestamped (streaming requests)."""
        prompts = rng.integers(10, vocab_hi, size=(a.num_requests, a.input_len)).tolist()
        gaps = rng.exponential(1.0 / a.arrival_rate, size=a.num_requests)
        t_arr = time.time() + np.cumsum(gaps) - gaps[0]
        last, first, ttft, ntok, i = {}, {}, [], 0, 0
        ids = [[] for _ in range(a.num_requests)]
        while i < a.num_requests or eng.has_unfinished():
            now = time.time()
            while i < a.num_requests and t_arr[i] <= now:
                rid = f"r{i}"
                eng.add_request(rid, None, sp, prompt_ids=prompts[i], stream=True)
                first[rid] = t_arr[i]
                i += 1
            if not eng.has_unfinished():
                time.sleep(max(0.0, min(t_arr[i] - time.time(), 0.01)))
                continue
            outs = eng.step()
            now = time.time()
            for o in outs:
                n = len(o.new_ids) if o.new_ids and o.new_ids[0] >= 0 else 0
                if not n:
                    continue
                ntok += n
                if o.req_id not in last:
                    ttft.append(now - first[o.req_id])
                    first[o.req_id] = now  # from here: first-token time
                else:
                    lat["itl"].append(now - last[o.req_id])
                last[o.req_id] = now
                if o.finished:
                    ids[int(o.req_id[1:])] = list(o.output_ids)
                    if len(o.output_ids) > 1:
                        lat["tpot"].append((now - first[o.req_id]) / (len(o.output_ids) - 1))
        return ntok, ttft, ids

    def wave():
        if a.arrival_rate > 0 and not pd:
            return online_wave()
        if pd:
            if is_prefill:
                prompts = rng.integers(10, vocab_hi, size=(a.num_requests, a.input_len)).tolist()
                # auto: chunk by chunk, except over a host-staged gloo send/recv channel
                chunked = a.pd_push == "chunked" or (a.pd_push == "auto" and (
                    pair.transport == "ipc" or dist.get_backend() != "gloo"))
                pair.run_prefill(prompts, sp, chunked=chunked)
                return 0, [], []
            r = pair.run_decode(sp, time.time())
            return r["output_tokens"], r["ttft"], []
        # int32 rows: the engine hands each to the scheduler in one copy (no per-id conversion)
        prompts = rng.integers(10, vocab_hi, size=(a.num_requests, a.input_len), dtype=np.int32)
        outs = eng.generate(None, sp, prompt_ids=prompts)
        ntok = sum(len(o.output_ids) for o in outs)
        ttfts = [o.ttft for o in outs if o.ttft is not None]
        return ntok, ttfts, [o.output_ids for o in outs]

    def barrier():
        if gpu:
            torch.cuda.synchronize()
        if world > 1 and tp_bc is None:  # TP ranks run in lock-step with rank 0 already
            dist.barrier()
        if gpu:
            torch.cuda.synchronize()

    for i in range(a.warmup):
        barrier()
        t = time.time()
        wave()
        log(f"[bench] warmup wave {i} {time.time() - t:.2f}s")
    barrier()
    t0 = time.perf_counter()
    total, ttfts, last_ids = 0, [], []
    for i in range(a.steps):
        if pd and i:
            barrier()  # P/D: every wave starts together on both sides (TTFT clock)
        n, tt, last_ids = wave()
        total += n
        ttfts += tt
    barrier()
    el = time.perf_counter() - t0
    log(f"[bench] host timers (all waves): {eng.timers}  steps={eng.steps}")
    log("[bench] execute s / steps by kind: " + ", ".join(
        f"{k} {v[0]:.3f}/{v[1]}" for k, v in getattr(eng, "step_kinds", {}).items()))
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, last_ids)
    for _ in range(a.profile_steps):
        wave()
    if a.torch_profile and rank == 0:
        # in-process kernel table of one more (untimed) wave on rank 0: works under torchrun,
        # where rocprofv3 cannot wrap the launcher
        from torch.profiler import ProfilerActivity, profile

        acts = [ProfilerActivity.CUDA] if gpu else [ProfilerActivity.CPU]
        with profile(activities=acts) as prof:
            wave()
            if gpu:
                torch.cuda.synchronize()
        key = "self_device_time_total" if gpu else "self_cpu_time_total"
        print(prof.key_averages().table(sort_by=key, row_limit=30), flush=True)
    elif a.torch_profile:
        wave()

    p50_local = statistics.median(ttfts) if ttfts else 0.0

    def pct(xs, q):
        return float(np.percentile(np.asarray(xs), q)) if xs else 0.0
    stats = torch.tensor([float(total), el, p50_local], dtype=torch.float64)
    if world > 1 and tp_bc is None:
        dev = torch.device("cuda", local) if gpu else torch.device("cpu")
        t_tok = torch.tensor([float(total)], dtype=torch.float64, device=dev)
        t_el = torch.tensor([el], dtype=torch.float64, device=dev)
        t_all = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_reduce(t_tok)
        dist.all_reduce(t_el, op=dist.ReduceOp.MAX)
        dist.all_gather(t_all, torch.tensor([p50_local], dtype=torch.float64, device=dev))
        p50s = [x.item() for x in t_all]
        if pd:  # TTFT is observed on the decode ranks
            p50s = p50s[n_pre:]
        stats = torch.tensor([t_tok.item(), t_el.item(), statistics.median(p50s)])
    tok, el, p50 = float(stats[0]), float(stats[1]), float(stats[2])
    kv_stats = None
    if pair is not None:
        # KV hand-off rate over the decode ranks' pulls (IPC transport)
        kt = torch.tensor([float(pair.pulled_bytes), pair.pull_seconds], dtype=torch.float64,
                          device=torch.device("cuda", local) if gpu else torch.device("cpu"))
        dist.all_reduce(kt)
        kv_stats = {"kv_transport": pair.transport,
                    "kv_pulled_gb": round(kt[0].item() / 1e9, 3),
                    "kv_pull_gbps": round(kt[0].item() / 1e9 / kt[1].item(), 1)
                    if kt[1].item() > 0 else None}
    if rank == 0:
        res = {
            "metric": "output tok/s + p50 TTFT",
            "value": round(tok / el, 2),
            "unit": "output tok/s",
            "n_gpus": n_dev,
            "ranks": max(world, 1),
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(el / a.steps * 1000, 3),
            "higher_is_better": True,
            "scaling": "strong" if a.tp > 1 else "weak",
            "vs_baseline": None,
            # compute dtype; an fp8 KV cache (storage only, not the headline) is named too
            "dtype": "bf16" if a.kv_cache_dtype == "auto" else "bf16+fp8kv",
            "data": "synthetic random token-id prompts, random-init weights",
            "p50_ttft_ms": round(p50 * 1000, 2),
            "config": {
                "model": mcfg.hf_id,
                "global_batch": a.num_requests * (n_pre if pd else
                                                  1 if a.tp > 1 else max(world, 1)),
                "seq_len": a.input_len + a.output_len,
                "input_len": a.input_len,
                "output_len": a.output_len,
                ("requests_per_prefill_rank" if pd else "requests_per_gpu"): a.num_requests,
                "parallelism": (f"pd{n_pre}x{world - n_pre}" if pd else
                                f"tp{a.tp}" if a.tp > 1 else f"dp{max(world, 1)}"),
                "max_num_seqs": a.max_num_seqs,
                "sampling": "greedy" if a.temperature <= 0 else f"T={a.temperature}",
                "hipgraph_decode": not a.enforce_eager,
                "kv_cache_dtype": "bf16" if a.kv_cache_dtype == "auto" else "fp8_e4m3",
                "mixed_batching": not a.no_mixed_batching,
            },
        }
        if kv_stats is not None:
            res.update(kv_stats)
        if a.arrival_rate > 0:
            res["arrival_rate_rps"] = a.arrival_rate
            res["p99_ttft_ms"] = round(pct(ttfts, 99) * 1000, 2)
            res["p50_tpot_ms"] = round(pct(lat["tpot"], 50) * 1000, 3)
            res["p99_tpot_ms"] = round(pct(lat["tpot"], 99) * 1000, 3)
            res["p50_itl_ms"] = round(pct(lat["itl"], 50) * 1000, 3)
            res["p99_itl_ms"] = round(pct(lat["itl"], 99) * 1000, 3)
            res["config"]["arrivals"] = "poisson"
        print(json.dumps(res), flush=True)
    if pair is not None:
        pair.close()
    if tp_bc is not None:
        tp_bc.shutdown()  # releases the mirroring ranks, destroys the process group
        return 0
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
