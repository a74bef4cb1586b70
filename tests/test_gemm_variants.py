"""The decode-GEMM Variant record against behaviour recorded before it existed
(tests/golden/gemm_variants_parent.json: candidate lists, log names, cache sections and the
*_supported predicates, written by the positional-tuple code), and the one launcher against the
CPU path of ops.dgemm on the GPU."""
import json
import os

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.models.config import get_config
from aws_k8s_ansible_provisioner_amd.models.transformer import DecoderLM
from aws_k8s_ansible_provisioner_amd.ops import gemm_tuner as gt
from aws_k8s_ansible_provisioner_amd.ops.gemm_variant import Variant

with open(os.path.join(os.path.dirname(__file__), "golden", "gemm_variants_parent.json")) as _f:
    GOLDEN = json.load(_f)


def _plain(rec):
    M, N, K = rec["M"], rec["N"], rec["K"]
    kw = rec["kwargs"]
    ws = [torch.empty(N, K, dtype=torch.bfloat16)]
    x = torch.empty(M, K, dtype=torch.bfloat16)
    y = torch.empty(M, N, dtype=torch.bfloat16)
    return [c for c, _ in gt._plain_candidates(
        M, ws, x, y, tuple(kw["splits"]), tuple(kw["pfs"]), tuple(kw["bns"]), tuple(kw["kms"]),
        kw["lm_head"])]


def test_plain_candidates_match_recorded_order_and_names():
    assert [len(r["choices"]) for r in GOLDEN["plain"]] == [61, 54, 54, 4, 2, 1]
    for rec in GOLDEN["plain"]:
        got = _plain(rec)
        assert got == [gt._choice(c) for c in rec["choices"]], (rec["M"], rec["N"], rec["K"])
        assert all(c[0] in ("wgemm", "hip", "dgemm") for c in got)
        names = [f"s{c[1].splitk}{c[1].name}" if c[0] == "dgemm" else None for c in got]
        assert names == rec["names"]


def test_fused_candidates_match_recorded_order_and_names():
    assert len(GOLDEN["fused"]) == 6
    for rec in GOLDEN["fused"]:
        got = gt._fused_candidates(rec["M"], rec["N"], rec["K"], rec["epi"], (1, 2, 4, 8),
                                   (2, 4, 8), (64, 128), (16, 32))
        assert got == [Variant.of(c) for c in rec["cands"]], rec["epi"]
        assert [f"s{v.splitk}{v.name}" for v in got] == rec["names"]
        # the same set the plain tuner's enumerator yields: one enumerator, two orders
        assert sorted(got) == sorted(gt.variants(rec["M"], rec["N"], rec["K"], rec["epi"],
                                                 (1, 2, 4, 8)))


def test_variant_of_defaults_and_properties():
    assert Variant.of((4, 2)) == Variant(4, 2, 0, 0, False, 0, 64) == Variant(splitk=4, pf=2)
    assert Variant.of([2, 1, 128, 8, 1]).inlaunch is True
    assert Variant.of(Variant(km=16)) == (1, 1, 0, 0, False, 16, 64)
    assert [Variant.of(v).family for v in ((1, 4), (1, 1, 64), (1, 1, 0, 0, False, 32))] == \
        ["ring", "lds", "kgemm"]
    assert Variant(bn=256, bm=256).probe_only and not Variant(bn=128, bm=256).probe_only
    assert [Variant.of(v).name for v in ((1, 2), (4, 4, 0, 0, True), (2, 1, 128, 8),
                                         (2, 1, 128, 3, True, 0, 256), (1, 1, 0, 0, False, 16))] \
        == ["p2", "p4i", "g128d", "g128x256i", "k16"]
    # the tuner's own rule on top of the kernel's predicate: K / splitk >= 256
    assert ops.dgemm_supported(16, 1024, 1024, 8, 2) and not Variant(8, 2).supported(16, 1024, 1024)
    assert Variant(4, 2).supported(16, 1024, 1024)


def test_supported_predicates_match_recorded():
    for rec in GOLDEN["supported"]:
        M, N, K = rec["M"], rec["N"], rec["K"]
        got = []
        for epi in (0, 1, 2):
            for s in (1, 2, 4, 8, 16):
                for pf in (2, 4, 8):
                    for inl in (False, True):
                        got.append(ops.dgemm_supported(M, N, K, s, pf, epi, inlaunch=inl))
                for bn in (64, 128):
                    for bm in (64, 128, 256):
                        for inl in (False, True):
                            got.append(ops.dgemm_supported(M, N, K, s, 1, epi, bn=bn,
                                                           inlaunch=inl, bm=bm))
            for km in (16, 32):
                got.append(ops.kgemm_supported(M, N, K, km, epi))
        assert got == rec["results"], (M, N, K)


def _write_cache(path, model, Ms, plan, fused):
    with open(path, "w") as f:
        json.dump({"key": gt.cache_key(model, Ms), "plan": plan, "fused": fused, "prefill": []}, f)


def test_cache_sections_of_every_legacy_length_load(tmp_path):
    """Cache sections written before the Variant type (dgemm choices of length 3, 6, 7 and 8,
    fused entries of length 3, 5, 6 and 7) load to the Variants their fields spell, and a plan
    naming the probe-only bn = 256 body is still refused."""
    m = DecoderLM(get_config("tiny-llama"), device="cpu", seed=0, max_model_len=64)
    Ms = [16, 160]
    plan, fused = GOLDEN["cache"]["plan"], GOLDEN["cache"]["fused"]
    assert {len(c) for _, c in plan if c[0] == "dgemm"} == {3, 6, 7, 8}
    assert {len(e) for _, pl in fused for e in pl.values()} == {3, 5, 6, 7}
    path = str(tmp_path / "tune.json")
    _write_cache(path, m, Ms, plan, fused)
    gt.reset()
    try:
        assert gt.load_cache(path, m, Ms)
        assert len(gt.plan()) == len(plan)
        for k, c in plan:
            got = gt.lookup(*k)
            want = ("dgemm", Variant.of(c[1:])) if c[0] == "dgemm" else tuple(c)
            assert got == want and got[0] == c[0]
        for M, pl in fused:
            assert gt.fused_plan(M) == {n: Variant.of(e) for n, e in pl.items()}
        # saved again, the file holds the same variants in the same list layout, full length
        gt.save_cache(path, m, Ms)
        with open(path) as f:
            data = json.load(f)
        assert [[k, c + list(Variant())[len(c) - 1:] if c[0] == "dgemm" else c]
                for k, c in plan] == data["plan"]
        assert [[M, {n: list(Variant.of(e)) for n, e in pl.items()}] for M, pl in fused] == \
            data["fused"]
        for bad_plan, bad_fused in (
                (plan + [[[256, 1024, 2048], ["dgemm", 2, 1, 256, 0, True, 0, 256]]], fused),
                (plan, fused + [[256, {"w_o": [2, 1, 256, 0, True, 0, 256]}]])):
            _write_cache(path, m, Ms, bad_plan, bad_fused)
            gt.reset()
            assert not gt.load_cache(path, m, Ms)
            assert not gt.plan() and gt.fused_plan(256) is None
    finally:
        gt.reset()


# ----------------------------------------------------------------------------- GPU: launcher
M_, N_, K_ = 160, 512, 1024
LAUNCHED = [
    Variant(1, 2), Variant(4, 2),            # register ring; split-K 4 with the separate reduce
    Variant(2, 2, inlaunch=True),            # its in-launch combine
    Variant(1, 1, 64, 0),                    # LDS-DMA 64-wide, shallow ring
    Variant(2, 1, 128, 8, True),             # LDS-DMA 128-wide, deep ring, in-launch combine
    Variant(1, 1, 128, 4, False, 0, 128),    # 128 x 128 tiles
    Variant(1, 1, 128, 3, False, 0, 256),    # 256-row tiles
    Variant(km=16), Variant(km=32),
]


@pytest.fixture(scope="module")
def launcher_inputs():
    """Inputs, and per epilogue the CPU path of ops.dgemm on them (shared, never modified)."""
    g = torch.Generator().manual_seed(11)
    bf = torch.bfloat16
    x = torch.randn(M_, K_, generator=g).to(bf)
    w = (torch.randn(2 * N_, K_, generator=g) * 0.03).to(bf)  # [:N_]: the store / residual weight
    res = torch.randn(M_, N_, generator=g).to(bf)
    ln = (torch.rand(N_, generator=g) + 0.5).to(bf)
    ssi = torch.rand(M_, generator=g) * K_ + 1.0
    inp = dict(x=x, w=w, res=res, ln=ln, ssi=ssi)
    ref = {ops.EPI_STORE: (ops.dgemm(x, w[:N_], ss_in=ssi),),
           ops.EPI_SILU: (ops.dgemm(x, w, ss_in=ssi, epi=ops.EPI_SILU),)}
    r, a, ss = res.clone(), torch.empty(M_, N_, dtype=bf), torch.zeros(M_)
    ops.dgemm(x, w[:N_], out=r, epi=ops.EPI_RESNORM, ss_out=ss, a_out=a, ln_out=ln)
    ref[ops.EPI_RESNORM] = (r, a, ss)
    return inp, ref


def _close(got, want):
    assert (got.float().cpu() - want.float()).abs().max().item() <= \
        2e-2 * want.float().abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("v", LAUNCHED, ids=lambda v: f"s{v.splitk}{v.name}")
def test_launcher_matches_cpu_dgemm(v, launcher_inputs):
    """gemm_tuner.launcher, once per variant and per epilogue its supported() admits, against
    the CPU path of ops.dgemm (outputs within 2e-2 of the reference's max, sums of squares
    rtol 1e-3 / atol 1e-2: the bounds of test_fused_epilogues_gpu)."""
    ops.load_native(required=True)
    inp, ref = launcher_inputs
    d = {k: t.cuda() for k, t in inp.items()}
    epis = [e for e in (ops.EPI_STORE, ops.EPI_RESNORM, ops.EPI_SILU)
            if v.supported(M_, 2 * N_ if e == ops.EPI_SILU else N_, K_, e)]
    # SwiGLU: not in kgemm, and with split-K only when the slices combine inside the launch
    silu_ok = v.family != "kgemm" and (v.splitk == 1 or v.inlaunch)
    assert epis == [ops.EPI_STORE, ops.EPI_RESNORM] + [ops.EPI_SILU] * silu_ok
    for epi in epis:
        if epi == ops.EPI_RESNORM:
            out = d["res"].clone()
            a = torch.empty(M_, N_, device="cuda", dtype=torch.bfloat16)
            ss = torch.zeros(M_, device="cuda")
            gt.launcher(v, M_, out, d["x"], [d["w"][:N_]], epi, None, ss, a, d["ln"])(0)
            _close(out, ref[epi][0])
            _close(a, ref[epi][1])
            assert torch.allclose(ss.cpu(), ref[epi][2], rtol=1e-3, atol=1e-2)
        else:
            silu = epi == ops.EPI_SILU
            out = torch.empty(M_, N_, device="cuda", dtype=torch.bfloat16)
            gt.launcher(v, M_, out, d["x"], [d["w"] if silu else d["w"][:N_]], epi,
                        d["ssi"])(0)
            _close(out, ref[epi][0])
