"""The kernels' host-side contract (csrc/kernels/host_contract.h) as Python sees it through the
CPU-built `_runtime.contract` module, against what the hand-written Python copies it replaced
answered (tests/golden/host_contract_parent.json, recorded from those copies before they were
deleted; where the header answers differently the record carries the new value and the tag of
its cause, listed in profiles/host_contract_refactor.md)."""
import collections
import json
import os
import shutil
import subprocess
import sys

import torch

from aws_k8s_ansible_provisioner_amd import _runtime_loader, build_ext, ops
from aws_k8s_ansible_provisioner_amd.ops import quant
from aws_k8s_ansible_provisioner_amd.ops.gemm_variant import Variant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(os.path.dirname(__file__), "golden", "host_contract_parent.json")) as _f:
    RECORDS = json.load(_f)


def _qgemm_supported(M, N, K, out):
    x = torch.empty(M, K, dtype=torch.bfloat16)
    w = quant.Fp8Weight(torch.empty(N, K, dtype=torch.uint8), torch.empty(N))
    pad = {"none": None, "ld+8": 8, "ld+4": 4}[out]
    o = None if pad is None else torch.empty(M, N + pad, dtype=torch.bfloat16)[:, :N]
    return quant.qgemm_supported(x, w, o)


def _workspace_sizes(M, N, s, pf, bn, inl, bm, pro):
    ws, tickets = ops.dgemm_workspace(M, N, Variant(s, pf, bn, 0, inl, 0, bm), pro, "meta")
    return [0 if s == 1 else ws.numel(), 0 if tickets is None else tickets.numel()]


ANSWER = {
    "dgemm_supported": lambda M, N, K, s, pf, epi, bn, inl, bm: ops.dgemm_supported(
        M, N, K, s, pf, epi, bn=bn, inlaunch=inl, bm=bm),
    "kgemm_supported": ops.kgemm_supported,
    "pgemm_supported": ops.pgemm_supported,
    "gemm_splitk": ops.gemm_splitk,
    "gdgemm_ws_floats": ops.gdgemm_ws_floats,
    "_combines_in_launch": ops._combines_in_launch,
    "dgemm_workspace": _workspace_sizes,
    "qgemm_supported": _qgemm_supported,
}

# Where the header (= what the bindings in ops.cpp accepted all along) answers differently from
# the Python copies: tag -> (function, what the arguments of such a record have in common).
DIFFERENCES = {
    # W smaller than M floats: the binding refuses the launch
    "D1": ("dgemm_supported", lambda M, N, K, s, pf, epi, bn, inl, bm: N * K * 2 < M * 4),
    # the 256 x 256 body needs M > 0 ...
    "D2": ("dgemm_supported", lambda M, N, K, s, pf, epi, bn, inl, bm: bn == 256 and M == 0),
    # ... and ignores bm (the Python copy insisted on bm = 256)
    "D3": ("dgemm_supported", lambda M, N, K, s, pf, epi, bn, inl, bm: bn == 256 and bm != 256),
    # the LDS-DMA branch of the Python copy never checked N > 0, K > 0, K / splitk >= 64
    "D4": ("dgemm_supported",
           lambda M, N, K, s, pf, epi, bn, inl, bm: bn in (64, 128) and (N == 0 or K == 0)),
    "D5": ("qgemm_supported", lambda M, N, K, out: N == 0),
    # a zero tile width sizes nothing (the Python copy divided by it)
    "D6": ("gdgemm_ws_floats", lambda M, N, s, bn, bm: bn == 0),
    # the 256 x 256 body combines in the launch whether asked to or not
    "D7": ("_combines_in_launch", lambda s, bn, inl, pro: bn == 256 and s > 1 and not inl),
    # sizes of launches the binding refuses anyway
    "D8": ("dgemm_workspace", lambda M, N, s, pf, bn, inl, bm, pro: M == 0 or N == 0),
    "D10": ("dgemm_workspace", lambda M, N, s, pf, bn, inl, bm, pro: bn in (64, 128) and pro != 0),
    "D11": ("dgemm_workspace", lambda M, N, s, pf, bn, inl, bm, pro: bn == 256 and N % 256 != 0),
    # LDS-DMA slices met by the separate reduce pass are dense [S, M, N], not tile-padded
    "D9": ("dgemm_workspace",
           lambda M, N, s, pf, bn, inl, bm, pro: bn in (64, 128) and not inl and s > 1),
    # the 256 x 256 body's slabs are 256 rows whatever bm says
    "D12": ("dgemm_workspace", lambda M, N, s, pf, bn, inl, bm, pro: bn == 256 and bm != 256),
}
# the new values of the differences with one value
NEW_VALUE = {"D1": False, "D2": False, "D3": True, "D4": False, "D5": False, "D6": 0, "D7": True}


def test_bindings_reproduce_the_recorded_python_copies():
    assert 300 <= len(RECORDS) <= 600
    seen = collections.Counter()
    for rec in RECORDS:
        fn, args = rec["fn"], rec["args"]
        got = ANSWER[fn](*args)
        why = rec.get("why")
        if why is None:
            assert got == rec["parent"], (fn, args)
            continue
        seen[why] += 1
        where, common = DIFFERENCES[why]
        assert where == fn and common(*args), (why, fn, args)
        assert rec["now"] != rec["parent"] and got == rec["now"], (why, fn, args, got)
        if why in NEW_VALUE:
            assert got == NEW_VALUE[why], (why, fn, args)
        if why == "D9":  # exactly what the binding asks for
            M, N, s = args[:3]
            assert got == [s * M * N, 0], args
        if why == "D12":  # pgemm_sk_ws_floats: whole 256 x 256 slabs, and the shared tickets
            M, N, s = args[:3]
            assert got == [-(-M // 256) * (N // 256) * s * 256 * 256, ops.GEMM_CTR_INTS], args
    assert set(seen) == set(DIFFERENCES) and min(seen.values()) >= 3, seen
    by_fn = collections.Counter(r["fn"] for r in RECORDS if "why" not in r)
    assert set(by_fn) == set(ANSWER) and min(by_fn.values()) >= 15, by_fn


def test_constants_come_from_the_header():
    c = _runtime_loader.contract()
    for name in ("CTR_STRIDE", "GEMM_CTR_INTS", "GEMM_CTR_ERR", "DECODE_MAX_PART",
                 "SAMPLE_MAX_CHUNKS", "SAMPLE_WS_PER_ROW"):
        assert name not in vars(ops), f"ops.{name} is a Python literal again"
        assert getattr(ops, name) == getattr(c, name)
    assert "QGEMM_MAX_M" not in vars(quant) and quant.QGEMM_MAX_M == c.QGEMM_MAX_M == 256
    assert (ops.CTR_STRIDE, ops.GEMM_CTR_INTS, ops.DECODE_MAX_PART) == (32, 1 << 18, 8192)
    assert ops.GEMM_CTR_ERR == ops.GEMM_CTR_INTS - 1
    for B in (1, 16, 256, 1000):
        assert ops.SAMPLE_WS_PER_ROW * B == c.sample_ws_floats(B)
    # the qgemm row limit is the predicate's
    assert c.qgemm_supported(c.QGEMM_MAX_M, 64, 64, 64, 64)
    assert not c.qgemm_supported(c.QGEMM_MAX_M + 1, 64, 64, 64, 64)
    # the contract function and the per-family predicates are one truth
    ok, family, inl, ws, tickets = c.dgemm_contract(16, 256, 512, 0, 0, 2, 1, 128, 0, 64, True, 256)
    assert (ok, family, inl) == (True, 1, True)
    assert ws == c.gdgemm_ws_floats(16, 256, 2, 128, 64) and tickets == 2 * c.CTR_STRIDE
    assert c.dgemm_contract(16, 256, 512, 0, 0, 16, 1, 0, 0, 64, True, 256)[2:] == \
        (False, 16 * 16 * 256, 0)   # 16 ring slices: the separate reduce pass, no tickets
    assert not c.pgemm_supported(1 << 20, 256, 1024, 1024) and c.pgemm_supported(1 << 19, 256, 1024, 1024)
    assert not c.pgemm_supported(1 << 19, 256, 1024, 2048)   # a row-strided X counts by its stride


def test_header_is_hashed_into_both_libraries(tmp_path, monkeypatch):
    """Editing nothing but host_contract.h changes the digest compiled into _runtime and the one
    compiled into _C.so (on a copy of the sources)."""
    pkg = tmp_path / "pkg"
    shutil.copytree(build_ext.CSRC, pkg / "csrc", ignore=shutil.ignore_patterns("build"))
    monkeypatch.setattr(build_ext, "PKG", str(pkg))
    monkeypatch.setattr(build_ext, "CSRC", str(pkg / "csrc"))
    header = pkg / "csrc" / "kernels" / "host_contract.h"
    assert str(header) in build_ext.runtime_sources() and str(header) in build_ext.kernel_sources()
    rt, kt = build_ext.runtime_tree_hash(), build_ext.kernel_tree_hash()
    monkeypatch.undo()
    assert (rt, kt) == (build_ext.runtime_tree_hash(), build_ext.kernel_tree_hash())
    monkeypatch.setattr(build_ext, "PKG", str(pkg))
    monkeypatch.setattr(build_ext, "CSRC", str(pkg / "csrc"))
    with open(header, "a") as f:
        f.write("// edited\n")
    assert build_ext.runtime_tree_hash() != rt
    assert build_ext.kernel_tree_hash() != kt


def test_ops_imports_and_runs_on_cpu_without_the_runtime_module():
    """The contract is loaded on first use: importing ops and running a CPU op must not touch
    `_runtime` (a child whose loader refuses to load it)."""
    code = (
        "import sys\n"
        "import aws_k8s_ansible_provisioner_amd._runtime_loader as rl\n"
        "def refuse():\n"
        "    raise AssertionError('_runtime loaded')\n"
        "rl.load = refuse\n"
        "import torch\n"
        "from aws_k8s_ansible_provisioner_amd import ops\n"
        "from aws_k8s_ansible_provisioner_amd.ops import quant, gemm_tuner, gemm_variant\n"
        "x = torch.arange(8.0).reshape(2, 4)\n"
        "y = ops.rms_norm(x, torch.ones(4), 1e-6)\n"
        "assert torch.allclose(y, x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6))\n"
        "assert not any(m.endswith('._runtime') or m == '_runtime' for m in sys.modules)\n"
        "try:\n"
        "    ops.CTR_STRIDE\n"
        "except AssertionError:\n"
        "    print('lazy ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "lazy ok" in r.stdout, r.stdout + r.stderr
