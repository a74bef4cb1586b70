"""The CPU side of the bit-exact GEMM tests (tests/test_gemm_exact_gpu.py).

* the preconditions of the exact oracle (ops.reference.exact_gemm_operands / _expected) for
  every shape the GPU file launches: no zero operand, every sum below 2^24 units, >= 90 % of
  the results exact in bf16, exact row sums of squares, and -- per epilogue -- a shape on which
  rounding mode and rounding order are really exercised;
* fp32 accumulation of those operands is exact in any order;
* the CPU paths of the ops -- the other side of the epilogue contract of
  csrc/kernels/gemm_common.h -- give exactly the expected tensors;
* sensitivity, on CPU tensors only: the exact comparator rejects a missing product, a truncating
  cast, a merged RESNORM rounding and a_out / ss_out taken from the unrounded sum, three of
  which the suite's `2e-2 * max` comparator accepts on its own randn inputs;
* the two derived ulp bounds (ss_in row scale: 1, SwiGLU: 2) hold for an fp32 emulation of the
  kernels' arithmetic with a perturbed rsqrt / exp.
"""
import collections

import pytest
import torch

import test_gemm_exact_gpu as G
from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.ops import reference as ref
from aws_k8s_ansible_provisioner_amd.ops.quant import Fp8Weight

STORE, RESNORM, SILU = ops.EPI_STORE, ops.EPI_RESNORM, ops.EPI_SILU
ROUNDING_SHAPE = (37, 256, 896, 3)   # M, N, K, vmax: > 1 % of y not exact in bf16


def trunc_bf16(v32):
    """fp32 -> bf16 by truncation (what a kernel with a wrong cast would store)."""
    return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def not_representable(yi):
    y = yi.double()
    return (y.to(torch.bfloat16).double() != y).double().mean().item()


# ------------------------------------------------------------------ the shapes the GPU file uses
def _gpu_shapes():
    """family -> set of (M, N, K, vmax, epi) of every launch in the GPU file."""
    s = collections.defaultdict(set)
    for f in ("ring", "lds", "kgemm", "pgemm_sk"):
        for c in G.FAMILY_CASES[f][1]:
            s[f].add((c.M, c.N, c.K, c.operand_vmax, c.epi))
    for M, N, K, _ in G.GEMM_CASES:
        s["gemm"].add((M, N, K, 3 if K == 896 else ref.exact_vmax(K), STORE))
    for M, N, K in G.WGEMM_CASES:
        s["wgemm"].add((M, N, K, ref.exact_vmax(K), STORE))
    for kind, m, N, K in G.PGEMM_CASES:
        if isinstance(m, int):
            s["pgemm"].add((m, N, K, 3 if K == 896 else ref.exact_vmax(K),
                            SILU if kind == "silu" else STORE))
    return s


GPU_SHAPES = _gpu_shapes()


def check_conditions(o, yi, epi, N):
    assert int((o.xi == 0).sum()) == 0 and int((o.wi == 0).sum()) == 0, "a zero hides a dropped element"
    assert bool((o.x == 0).sum() == 0) and bool((o.w == 0).sum() == 0)
    assert torch.equal(o.x.double(), o.xi.double()) and torch.equal(o.w.double(), o.wi.double() * o.unit)
    assert int(yi.abs().max()) < ref.EXACT_LIMIT
    below = (yi.abs() < ref.EXACT_BF16_INT).double().mean().item()
    assert below >= 0.90, f"only {below:.3f} of the results are exact in bf16"
    if epi == RESNORM:
        ri, ln = G.resnorm_inputs(yi.shape[0], N)
        assert int((ri == 0).sum()) == 0
        ref.exact_gemm_expected(yi, o.unit, RESNORM, residual_i=ri, ln=ln)  # asserts ss < 2^24


@pytest.mark.parametrize("family", sorted(GPU_SHAPES))
def test_oracle_conditions_hold_for_every_gpu_shape(family):
    assert GPU_SHAPES[family]
    for M, N, K, vmax, epi in sorted(GPU_SHAPES[family]):
        o, yi = G.oracle(M, N, K, vmax)
        check_conditions(o, yi, epi, N)
    if family in ("ring", "lds", "kgemm", "pgemm_sk"):
        for c in G.FAMILY_CASES[family][1]:
            if c.scaled:   # the expected tensors of a scaled case assert their own exactness
                o, ss_in, eps, ri, ln, want = G.dcase_expected(c)
                assert bool((ss_in > 0).all())
                if c.scaled == 2:   # ss_in / K + eps is exactly 4^j: the scale is 2^-j
                    m, e = torch.frexp(ss_in.double() / c.K + eps)
                    assert bool((m == 0.5).all()) and bool((e % 2 == 1).all())


def test_oracle_conditions_grouped_fp8_and_moe():
    for kind, m, N, K in G.PGEMM_CASES:
        if not isinstance(m, int):
            o, yi = G.grouped_oracle(m, N, K)
            check_conditions(o, yi, STORE, N)
    for M, N, K in G.QGEMM_CASES + [(300, 320, 512)]:
        o, q, scale, yi = G.fp8_oracle(M, N, K)
        check_conditions(o, yi, STORE, N)
        assert torch.equal(q.view(torch.float8_e4m3fn).double(), o.wi.double())
        m, e = torch.frexp(scale)
        assert bool((m == 0.5).all()), "channel scales must be powers of two"
    for bm in (32, 64):
        for gather in (True, False):
            for K in sorted({c[6] for c in G.MOE_DGEMM_CASES if c[0] == bm}):
                o, xi, wi, expert, _ = G.moe_oracle(bm, 320, K, gather, False)
                yi = G.moe_int_matmul(xi, wi, expert)
                assert int((o.xi == 0).sum()) == 0 and int((o.wi == 0).sum()) == 0
                assert (yi.abs() < ref.EXACT_BF16_INT).double().mean().item() >= 0.90


@pytest.mark.parametrize("epi", [STORE, RESNORM, SILU])
def test_rounding_mode_and_order_are_exercised(epi):
    """Per epilogue, the shape on which >= 1 % of y is not exact in bf16 is launched by the
    register-ring, LDS-DMA and pgemm_sk families (and kgemm / gemm / pgemm where they have the
    epilogue); on it a truncating cast and a single-rounding RESNORM each change the result."""
    M, N, K, vmax = ROUNDING_SHAPE
    for f in ("ring", "lds", "pgemm_sk"):
        assert (M, N, K, vmax, epi) in GPU_SHAPES[f] or (256, N, K, vmax, epi) in GPU_SHAPES[f]
    o, yi = G.oracle(M, N, K, vmax)
    assert not_representable(yi) >= 0.01
    y32 = (yi.double() * o.unit).float()
    want = ref.exact_gemm_expected(yi, o.unit).out
    assert not torch.equal(trunc_bf16(y32), want), "truncation is indistinguishable here"
    ri, ln = G.resnorm_inputs(M, N)
    res = ref.exact_gemm_expected(yi, o.unit, RESNORM, residual_i=ri, ln=ln)
    one_rounding = ((yi + ri).double() * o.unit).float().to(torch.bfloat16)
    assert not torch.equal(one_rounding, res.out), "rounding order is indistinguishable here"


def test_case_enumeration_reaches_every_dispatch():
    """The CPU-side enumeration the GPU file's count test relies on is not empty anywhere and
    names every template dispatch the issue lists."""
    ring = G.FAMILY_CASES["ring"][1]
    for epi in (STORE, RESNORM, SILU):
        assert {c.v.pf for c in ring if c.epi == epi} == {1, 2, 4, 8}
        assert {c.v.splitk for c in ring if c.epi == epi and c.v.inlaunch} == {2, 4, 8}
    assert {c.v.splitk for c in ring if c.epi == STORE and not c.v.inlaunch} == {1, 2, 4, 8, 16}
    assert {c.v.splitk for c in ring if c.epi == RESNORM and not c.v.inlaunch} == {1, 2, 4, 8, 16}
    rows = {(c.N, c.v.splitk, c.scaled) for c in ring if c.epi == RESNORM and not c.v.inlaunch}
    assert rows >= {(1024, 2, 0), (2048, 2, 0), (4096, 4, 0), (4096, 8, 0), (8192, 2, 0), (256, 16, 0),
                    (1024, 2, 2), (2048, 4, 2), (1024, 8, 2), (256, 2, 2), (256, 16, 2)}
    lds = G.FAMILY_CASES["lds"][1]
    for epi in (STORE, RESNORM, SILU):
        got = {(c.v.bm, c.v.bn, c.v.ns >= 6, c.v.splitk if c.v.inlaunch else 0) for c in lds if c.epi == epi}
        for bm, bn, ns in G.LDS_TILES:
            for s in (0, 2, 4, 8):
                assert (bm, bn, ns >= 6, s) in got, (epi, bm, bn, ns, s)
    assert {c.v.ns for c in lds} == {0, 6, 8}
    assert {c.K // c.v.splitk // 64 for c in lds} >= {1, 2, 16}
    assert {(c.v.km, c.epi) for c in G.FAMILY_CASES["kgemm"][1]} == {(16, 0), (16, 1), (32, 0), (32, 1)}
    sk = G.FAMILY_CASES["pgemm_sk"][1]
    assert {c.epi for c in sk if (c.K // 64) % c.v.splitk} == {STORE, RESNORM, SILU}, "uneven splits"
    for f in ("ring", "lds", "kgemm", "pgemm_sk"):
        assert any(c.scaled for c in G.FAMILY_CASES[f][1]), f"{f}: no ss_in case"
        assert all(c.epi == STORE for c in G.FAMILY_CASES[f][1] if c.scaled == 1)
        assert {c.epi for c in G.FAMILY_CASES[f][1] if c.scaled == 2} >= {RESNORM}
    assert {G.qgemm_geometry(M, N) for M, N, K in G.QGEMM_CASES} == G.QGEMM_GEOMETRIES
    moe = set(G.MOE_DGEMM_CASES)
    assert {(c[0], c[1], c[2]) for c in moe} == {(bm, pf, s) for bm in (32, 64) for pf in (1, 2, 4)
                                                 for s in (1, 2, 4)}
    assert {(c[3], c[4]) for c in moe} == {(True, True), (True, False), (False, True), (False, False)}
    assert 0 in G.MOE_COUNTS and any(n % 64 for n in G.MOE_COUNTS)
    for c in ring + lds:  # the predicate the launcher itself applies
        assert c.supported()
    for env, families in G.KNOBS:
        assert len(G.reduced_selection(families)) > 1
    picked = [c for f in ("ring", "lds") for c in G._reduced_dcases(G.FAMILY_CASES[f][1])]
    assert sum(c.stagger_exercised() for c in picked) >= 4


# ------------------------------------------------------------------------- order independence
@pytest.mark.parametrize("M,N,K,vmax", [(37, 256, 14336, 1), (65, 320, 512, 3), (256, 1024, 4096, 1),
                                        ROUNDING_SHAPE])
def test_fp32_accumulation_is_exact_in_any_order(M, N, K, vmax):
    o, yi = G.oracle(M, N, K, vmax)
    assert torch.equal(yi, o.xi @ o.wi.t()), "the float64 product is the int64 product"
    want = (yi.double() * o.unit).float()
    xf, wf = o.x.float(), o.w.float()
    assert torch.equal(xf @ wf.t(), want)
    strided = torch.zeros(M, N)
    for s in range(16):
        strided += xf[:, s::16] @ wf[:, s::16].t()
    assert torch.equal(strided, want)
    assert torch.equal(xf.flip(1) @ wf.flip(1).t(), want)
    sliced = sum(xf[:, k:k + K // 4] @ wf[:, k:k + K // 4].t() for k in range(0, K, K // 4))
    assert torch.equal(sliced, want)


# --------------------------------------------------------------------------------- CPU paths
@pytest.mark.parametrize("M,N,K,vmax", [ROUNDING_SHAPE, (65, 320, 512, 3), (37, 256, 14336, 1)])
def test_cpu_dgemm_keeps_the_contract(M, N, K, vmax):
    o, yi = G.oracle(M, N, K, vmax)
    assert torch.equal(ops.dgemm(o.x, o.w), ref.exact_gemm_expected(yi, o.unit).out)
    ri, ln = G.resnorm_inputs(M, N)
    want = ref.exact_gemm_expected(yi, o.unit, RESNORM, residual_i=ri, ln=ln)
    res = (ri.double() * o.unit).to(torch.bfloat16)
    a, ss = torch.empty(M, N, dtype=torch.bfloat16), torch.zeros(M + 2)
    ops.dgemm(o.x, o.w, out=res, epi=RESNORM, ss_out=ss, a_out=a, ln_out=ln)
    assert torch.equal(res, want.out) and torch.equal(a, want.a)
    assert torch.equal(ss[:M], want.ss) and bool((ss[M:] == 0).all())
    silu = ops.dgemm(o.x, o.w, epi=SILU)
    assert torch.equal(silu, ref.exact_gemm_expected(yi, o.unit, SILU).out)
    # the ss_in row scale: within one ulp of the float64 value
    ssi = torch.rand(M, generator=torch.Generator().manual_seed(1)) * K + 1.0
    want = ref.exact_gemm_expected(yi, o.unit, row_scale=1.0 / torch.sqrt(ssi.double() / K + 1e-6))
    got = ops.dgemm(o.x, o.w, ss_in=ssi, eps=1e-6)
    assert int(ref.bf16_ulp_distance(got, want.out).max()) <= G.ULP_SS_IN


def test_cpu_wgemm_pgemm_and_fp8_paths_keep_the_contract():
    M, N, K, vmax = ROUNDING_SHAPE
    o, yi = G.oracle(M, N, K, vmax)
    y = ref.exact_gemm_expected(yi, o.unit).out
    assert torch.equal(ops.wgemm(o.x, o.w), y)
    assert torch.equal(ops.pgemm(o.x, o.w), y)
    assert torch.equal(ops.linear(o.x, o.w), y)
    assert torch.equal(ops.pgemm(o.x, o.w, silu=True), ref.exact_gemm_expected(yi, o.unit, SILU).out)
    counts = (130, 0, 1, 257, 0, 40)
    og, yg = G.grouped_oracle(counts, 256, 128)
    offs = torch.tensor(counts).cumsum(0).to(torch.int32)
    wg = og.w.view(len(counts), 256, 128)
    assert torch.equal(ops.pgemm(og.x, wg, offs=offs), ref.exact_gemm_expected(yg, og.unit).out)
    assert torch.equal(ops.pgemm(og.x, wg, silu=True, offs=offs),
                       ref.exact_gemm_expected(yg, og.unit, SILU).out)
    of, q, scale, yq = G.fp8_oracle(37, 1000, 896)
    w8 = Fp8Weight(q, scale.float())
    want = ref.exact_gemm_expected(yq, scale[None, :]).out
    assert torch.equal(ops.linear_fp8(of.x, w8), want)
    assert torch.equal(ops.quant.dequant_fp8(w8), (of.wi.double() * scale[:, None]).to(torch.bfloat16))


def test_cpu_fused_moe_keeps_the_contract():
    """ref.fused_moe: the up projection and SwiGLU are exact; the down projection consumes
    SwiGLU outputs (not integers), so its fp32 sum can flip one bf16 rounding against the
    float64 value -- with one expert per token and a power-of-two routing weight, one ulp."""
    T, d, F, E = 37, 64, 128, 4
    o1 = ref.exact_gemm_operands(T, E * 2 * F, d, 11)
    o2 = ref.exact_gemm_operands(1, E * d, F, 12)
    w13, w2 = o1.w.view(E, 2 * F, d), o2.w.view(E, d, F)
    ids = (torch.arange(T) % 3).view(T, 1).to(torch.int32)      # expert 3 stays empty
    wts = torch.full((T, 1), 0.5)
    got = ref.fused_moe(o1.x, w13, w2, wts, ids)
    want = torch.zeros(T, d, dtype=torch.bfloat16)
    for e in range(3):
        m = ids[:, 0] == e
        yi = ref.exact_int_matmul(o1.xi[m], o1.wi.view(E, 2 * F, d)[e])
        act = ref.exact_gemm_expected(yi, o1.unit, SILU).out
        assert torch.equal(ref.silu_and_mul((o1.x[m].float() @ w13[e].float().t()).to(torch.bfloat16)), act)
        want[m] = ref.bf16_rne(0.5 * ref.bf16_rne(act.double() @ w2[e].double().t()).double())
    assert int(ref.bf16_ulp_distance(got, want).max()) <= 1


# --------------------------------------------------------------------------------- sensitivity
def test_exact_comparator_rejects_what_the_loose_one_accepts():
    """The justification for the exact tests.  Four faults, applied to CPU tensors only."""
    M, N, K, vmax = ROUNDING_SHAPE
    o, yi = G.oracle(M, N, K, vmax)
    ri, ln = G.resnorm_inputs(M, N)
    want = ref.exact_gemm_expected(yi, o.unit, RESNORM, residual_i=ri, ln=ln)
    y = ref.exact_gemm_expected(yi, o.unit).out
    y32 = (yi.double() * o.unit).float()
    res32 = (ri.double() * o.unit).float()
    # 1: one (m, k) product missing from the last row
    dropped = yi.clone()
    dropped[-1] -= o.xi[-1, K // 3] * o.wi[:, K // 3]
    bad = ref.exact_gemm_expected(dropped, o.unit).out
    assert int((bad[-1] != y[-1]).sum()) >= 0.9 * N and torch.equal(bad[:-1], y[:-1])
    # 2: truncation instead of round-to-nearest-even
    assert not torch.equal(trunc_bf16(y32), y)
    # 3: RESNORM with one rounding instead of two
    assert not torch.equal((y32 + res32).to(torch.bfloat16), want.out)
    # 4: a_out and ss_out from the unrounded sum
    t32 = y.float() + res32
    assert not torch.equal((t32 * ln.float()).to(torch.bfloat16), want.a)
    assert not torch.equal(t32.pow(2).sum(-1), want.ss)

    # ... and on the suite's own randn inputs its comparators accept faults 2, 3 and 4
    g = torch.Generator().manual_seed(37 + 1024 + 2048)
    x = torch.randn(37, 2048, generator=g).to(torch.bfloat16)
    w = (torch.randn(1024, 2048, generator=g) * 0.05).to(torch.bfloat16)
    res0 = torch.randn(37, 1024, generator=g).to(torch.bfloat16)
    lnr = (torch.rand(1024, generator=g) + 0.5).to(torch.bfloat16)
    yr = x.float() @ w.float().t()

    def close(a, b, atol):
        return bool(((a.float() - b.float()).abs() <= atol).all())

    assert close(trunc_bf16(yr), yr, 2e-2 * yr.abs().max().item())
    ref_res = yr.to(torch.bfloat16).float() + res0.float()
    one = (yr + res0.float()).to(torch.bfloat16)
    assert close(one, ref_res, 2e-2 * ref_res.abs().max().item())
    s = ref_res.to(torch.bfloat16)                      # the contract's residual
    a_unrounded = (ref_res * lnr.float()).to(torch.bfloat16)
    a_ref = s.float() * lnr.float()
    assert close(a_unrounded, a_ref, 1e-2 * a_unrounded.float().abs().max().item())
    assert torch.allclose(ref_res.pow(2).sum(-1), s.float().pow(2).sum(-1), rtol=1e-3, atol=1e-2)
    # the exact comparator would not: the same faults change bits on these inputs too
    assert not torch.equal(trunc_bf16(yr), yr.to(torch.bfloat16))
    assert not torch.equal(one, s) and not torch.equal(a_unrounded, a_ref.to(torch.bfloat16))


# ------------------------------------------------------------------- the two derived ulp bounds
@pytest.mark.parametrize("rel", [0.0, 3e-7, -3e-7])
def test_ulp_bounds_hold_for_an_fp32_emulation(rel):
    """ss_in: y * rsqrt(ss / K + eps) in fp32 with the rsqrt off by `rel` stays within one bf16
    ulp of the float64 value.  SwiGLU: bf16(bf16(g / (1 + exp(-g))) * u) in fp32 with exp off by
    `rel` stays within two (one possible flip at each rounding)."""
    M, N, K, vmax = ROUNDING_SHAPE
    o, yi = G.oracle(M, N, K, vmax)
    ssi = torch.rand(M, generator=torch.Generator().manual_seed(2)) * K + 1.0
    want = ref.exact_gemm_expected(yi, o.unit, row_scale=1.0 / torch.sqrt(ssi.double() / K + 1e-6)).out
    scale = torch.rsqrt(ssi * (1.0 / K) + 1e-6) * (1.0 + rel)
    got = ((yi.double() * o.unit).float() * scale[:, None]).to(torch.bfloat16)
    assert int(ref.bf16_ulp_distance(got, want).max()) <= G.ULP_SS_IN
    want = ref.exact_gemm_expected(yi, o.unit, SILU).out
    y = ref.exact_gemm_expected(yi, o.unit).out.float()
    g, u = y[:, :N // 2], y[:, N // 2:]
    sg = (g / (1.0 + torch.exp(-g) * (1.0 + rel))).to(torch.bfloat16)
    got = (sg.float() * u).to(torch.bfloat16)
    assert int(ref.bf16_ulp_distance(got, want).max()) <= G.ULP_SILU
