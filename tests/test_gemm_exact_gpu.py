"""Bit-exact tests of the GEMM kernels, their epilogues and their environment knobs.

The operands (ops.reference.exact_gemm_operands) are small non-zero integers, the weight
scaled by a power of two, so the fp32 accumulator a kernel holds before its epilogue is known
bit for bit from an integer matmul on the CPU -- whatever the order of the MFMAs, K splits,
slabs, reduce passes and in-launch combines.  The expected outputs then follow from the
epilogue contract of csrc/kernels/gemm_common.h by round-to-nearest-even at the points it names
(ops.reference.exact_gemm_expected) and are compared with torch.equal: one missing product, a
truncating cast or a merged rounding changes the bits.  Only two things are not bit-exact and get
their own, derived bound: the ss_in row scale (hardware rsqrt: one bf16 ulp) and SwiGLU (__expf:
two bf16 ulps).

Every output is a slice of a larger sentinel-filled buffer (spare rows, spare columns where the
binding takes a row stride, spare a_out / ss_out / workspace entries): the sentinels must
survive the launch.  A second launch on the same inputs must give the same bits and leave every
in-launch ticket at zero.

The case lists are enumerated on the CPU at import (no GPU needed) from the project's own
*_supported predicates; tests/test_gemm_exact_cpu.py checks the oracle's preconditions for every
shape listed here, and test_zz_case_counts checks that every enumerated case really ran.
"""
import collections
import functools
import os
import subprocess
import sys
import time

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import _runtime_loader, ops
from aws_k8s_ansible_provisioner_amd.ops import reference as ref
from aws_k8s_ansible_provisioner_amd.ops.gemm_variant import Variant

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, RESNORM, SILU = ops.EPI_STORE, ops.EPI_RESNORM, ops.EPI_SILU
SENT = -24576.0      # bf16 sentinel: exact in bf16, far outside every result
SENT_F32 = 1.5e30    # fp32 workspace / partials sentinel
SENT_SS = -7.0       # ss_out spare entries
PAD_ROWS, PAD_COLS = 3, 8
EPS = 1e-6
ULP_SS_IN, ULP_SILU = 1, 2   # derived bounds (module docstring; test_gemm_exact_cpu.py)
CHILD_FLAG = "AKAP_GEMM_EXACT_CHILD"   # set in the knob children: they start no children

RAN = collections.Counter()            # family -> cases that ran to the end
OBSERVED_ULP = collections.defaultdict(int)   # "family/kind" -> largest ulp distance seen


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.load_native(required=True)


# ------------------------------------------------------------------------------- the oracle
def _seed(*k):
    s = 0
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=None)
def oracle(M, N, K, vmax):
    """(operands, exact int64 accumulator) of one shape, computed once."""
    o = ref.exact_gemm_operands(M, N, K, _seed(M, N, K, vmax), vmax)
    return o, ref.exact_int_matmul(o.xi, o.wi)


@functools.lru_cache(maxsize=None)
def resnorm_inputs(M, N):
    """Residual (int64, in units; non-zero, up to +-7) and an arbitrary bf16 norm weight."""
    g = torch.Generator().manual_seed(_seed(M, N, 77))
    ri = torch.randint(1, 8, (M, N), generator=g) * (torch.randint(0, 2, (M, N), generator=g) * 2 - 1)
    ln = (torch.rand(N, generator=g) + 0.5).to(torch.bfloat16)
    return ri, ln


def vmax_for(K, N, epi):
    return ref.exact_vmax(K, N if epi == RESNORM else 0)


# ------------------------------------------------------------------------------- canaries
class Canary:
    """out = the first `rows` rows and `cols` columns of a larger sentinel-filled buffer."""

    def __init__(self, rows, cols, strided, dtype=torch.bfloat16, sent=SENT, pad_cols=PAD_COLS):
        self.sent = sent
        self.big = torch.full((rows + PAD_ROWS, cols + (pad_cols if strided else 0)), sent,
                              dtype=dtype, device=DEV)
        self.view = self.big[:rows, :cols]

    def intact(self):
        m = torch.ones_like(self.big, dtype=torch.bool)
        m[:self.view.shape[0], :self.view.shape[1]] = False
        return bool((self.big[m] == self.sent).all())


def flat_canary(n, dtype, sent, fill=None, tail=64):
    big = torch.full((n + tail,), sent, dtype=dtype, device=DEV)
    if fill is not None:
        big[:n] = fill
    return big, big[:n]


def tail_intact(big, n, sent):
    return bool((big[n:] == sent).all())


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    if got.dtype == torch.bfloat16:
        bad = ref.bf16_ulp_distance(got, want) != 0
    else:
        bad = got != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, "
                                 f"first at {bad.nonzero()[0].tolist()}: got "
                                 f"{got[bad][0].item()} want {want[bad][0].item()}")


def assert_ulp(got, want, bound, key):
    d = int(ref.bf16_ulp_distance(got.cpu(), want.cpu()).max())
    OBSERVED_ULP[key] = max(OBSERVED_ULP[key], d)
    print(f"[ulp] {key}: max distance {d} (bound {bound})")
    assert d <= bound, f"{key}: {d} bf16 ulps from the float64 contract value (bound {bound})"


# --------------------------------------------------------------- decode GEMMs (DGemmArgs form)
class DCase(collections.namedtuple("DCase", "M N K v epi vmax scaled")):
    """One launch of dgemm / gdgemm / pgemm_sk / kgemm: shape, Variant, epilogue, operand range
    (0 = exact_vmax) and the ss_in row scale: 0 none; 1 arbitrary (EPI_STORE, within one ulp);
    2 ss_in = K * 4^j with eps = 0, so the scale is exactly 2^-j (j = 0..3 by row) and every
    epilogue stays bit-exact (K a power of two, so ss_in / K is exact)."""

    @property
    def id(self):
        return (f"{self.M}x{self.N}x{self.K}-s{self.v.splitk}{self.v.name}-e{self.epi}"
                + (f"-ns{self.v.ns}" if self.v.ns else "")
                + (f"-v{self.vmax}" if self.vmax else "") + ("", "-ssin", "-ssin2")[self.scaled])

    @property
    def operand_vmax(self):
        return self.vmax or vmax_for(self.K, self.N, self.epi)

    def supported(self):
        v = self.v
        if v.family == "kgemm":
            return ops.kgemm_supported(self.M, self.N, self.K, v.km, self.epi)
        return ops.dgemm_supported(self.M, self.N, self.K, v.splitk, v.pf, self.epi, bn=v.bn,
                                   inlaunch=v.inlaunch, bm=v.bm)

    def combines_in_launch(self):
        v = self.v
        return v.probe_only or ops._combines_in_launch(v.splitk, v.bn, v.inlaunch)

    def stagger_exercised(self):
        """AKAP_GEMM_STAGGER: some tile starts its K walk off zero ((tn + 3 tm) % nk != 0)."""
        bm, bn = (self.v.bm, self.v.bn) if self.v.bn else (64, 64)
        nk = self.K // self.v.splitk // 64
        return nk > 1 and any((tn + 3 * tm) % nk for tm in range(-(-self.M // bm))
                              for tn in range(-(-self.N // bn)))


def _resnorm_n(K, reduce_pass, wrap):
    """N of an EPI_RESNORM case: the separate reduce pass needs N % 256 == 0 (N = 1024 also
    takes its row-parallel form); a row's sum of squares must stay exact (exact_vmax)."""
    if not reduce_pass:
        return 320
    return 1024 if wrap and K <= 8192 else 256


SPLITS = [(1, False), (2, False), (4, False), (8, False), (16, False), (2, True), (4, True),
          (8, True)]


def _ring_cases():
    out = []
    for pf in (1, 2, 4, 8):
        for splitk, inl in SPLITS:
            for epi in (STORE, RESNORM, SILU):
                # a slice of exactly one pipeline fill (empty steady state), and one that wraps
                # the ring many times
                for wrap in (False, True):
                    K = splitk * (1024 if wrap else 64 * pf)
                    M = 37 if wrap else 65
                    N = _resnorm_n(K, splitk > 1 and not inl, wrap) if epi == RESNORM else 320
                    out.append(DCase(M, N, K, Variant(splitk, pf, inlaunch=inl), epi, 0, False))
    for epi in (STORE, RESNORM, SILU):  # the rounding shape: > 1 % of y not exact in bf16
        out.append(DCase(37, 256, 896, Variant(1, 2), epi, 3, False))
        out.append(DCase(37, 256, 896, Variant(2, 1, inlaunch=True), epi, 3, False))
    for epi in (STORE, RESNORM):        # the reduction depth
        out.append(DCase(37, 256, 14336, Variant(4, 2), epi, 1, False))
    out.append(DCase(65, 320, 512, Variant(2, 2, inlaunch=True), STORE, 0, True))
    out.append(DCase(65, 320, 512, Variant(2, 2), STORE, 0, True))
    out.append(DCase(1, 256, 256, Variant(1, 4), STORE, 0, True))
    # the row-parallel RESNORM reduce: N / 1024 = 1 | 2 | 4 | 8 row chunks, 2 | 4 | 8 slabs
    for splitk, N in ((2, 2048), (4, 4096), (8, 4096), (2, 8192), (4, 1024)):
        out.append(DCase(37, N, 1024, Variant(splitk, 2), RESNORM, 1, False))
    # an exact (power of two) ss_in scale under the other epilogues and both reduce kernels
    for epi in (RESNORM, SILU):
        out.append(DCase(65, 320, 512, Variant(1, 2), epi, 0, 2))
        out.append(DCase(65, 320, 512, Variant(4, 1, inlaunch=True), epi, 0, 2))
    for splitk, N in ((2, 1024), (4, 2048), (8, 1024), (2, 256), (16, 256)):
        out.append(DCase(37, N, 1024, Variant(splitk, 1), RESNORM, 1, 2))
    out.append(DCase(37, 320, 1024, Variant(2, 1), STORE, 0, 2))
    return [c for c in out if c.supported()]


LDS_TILES = [(64, 64, 0), (64, 64, 6), (64, 64, 8), (64, 128, 0), (64, 128, 6), (64, 128, 8),
             (128, 128, 0), (256, 64, 0), (256, 128, 0)]   # (bm, bn, ns)
# (splitk, inlaunch, k-steps per slice): 1 = the ring prologue alone, 2 = fewer than the ring
# depth, 16 = wrap-around
LDS_SPLITS = [(1, False, 1), (1, False, 2), (1, False, 16), (2, False, 16), (16, False, 1),
              (2, True, 2), (4, True, 16), (8, True, 1)]
LDS_TAIL_M = {64: 65, 128: 130, 256: 300}


def _lds_cases():
    out = []
    for bm, bn, ns in LDS_TILES:
        for splitk, inl, steps in LDS_SPLITS:
            for epi in (STORE, RESNORM, SILU):
                K = splitk * steps * 64
                M = 37 if (bm == 64 and steps == 16) else LDS_TAIL_M[bm]
                N = _resnorm_n(K, splitk > 1 and not inl, steps == 16) if epi == RESNORM else 320
                out.append(DCase(M, N, K, Variant(splitk, 1, bn, ns, inl, 0, bm), epi, 0, False))
    for epi in (STORE, RESNORM, SILU):
        out.append(DCase(37, 256, 896, Variant(1, 1, 64), epi, 3, False))
        out.append(DCase(256, 256, 896, Variant(2, 1, 128, 0, True, 0, 256), epi, 3, False))
    out.append(DCase(37, 256, 14336, Variant(4, 1, 128, 6, True), STORE, 1, False))
    out.append(DCase(130, 320, 512, Variant(2, 1, 128, 0, True, 0, 128), STORE, 0, True))
    out.append(DCase(65, 320, 256, Variant(1, 1, 64, 8), STORE, 0, True))
    for epi in (RESNORM, SILU):   # an exact ss_in scale under the other epilogues
        out.append(DCase(65, 320, 512, Variant(1, 1, 64), epi, 0, 2))
        out.append(DCase(130, 320, 512, Variant(4, 1, 128, 0, True, 0, 128), epi, 0, 2))
        out.append(DCase(300, 320, 256, Variant(2, 1, 128, 0, True, 0, 256), epi, 0, 2))
    out.append(DCase(65, 1024, 1024, Variant(2, 1, 64, 8), RESNORM, 1, 2))   # reduce pass
    return [c for c in out if c.supported()]


def _kgemm_cases():
    out = []
    for km in (16, 32):
        for epi in (STORE, RESNORM):
            for M, N, K in [(37, 320, 256), (65, 1024, 1024), (1, 256, 2048), (130, 320, 1280)]:
                out.append(DCase(M, N, K, Variant(km=km), epi, 0, False))
            out.append(DCase(37, 256, 768, Variant(km=km), epi, 3, False))
        out.append(DCase(37, 320, 512, Variant(km=km), STORE, 0, True))
        out.append(DCase(37, 320, 512, Variant(km=km), RESNORM, 0, 2))
    return [c for c in out if c.supported()]


def _pgemm_sk_cases():
    out = []
    v = lambda s: Variant(s, 1, 256, 0, True, 0, 256)  # noqa: E731
    for epi in (STORE, RESNORM, SILU):
        out.append(DCase(37, 256, 128, v(1), epi, 0, False))
        out.append(DCase(130, 512, 640, v(3), epi, 0, False))     # 10 k-tiles over 3 slices
        out.append(DCase(300, 256, 1024, v(5), epi, 0, False))    # two row tiles, 16 over 5
        out.append(DCase(37, 256, 896, v(4), epi, 3, False))      # 14 over 4
    out.append(DCase(130, 512, 640, v(3), STORE, 0, True))
    for epi in (RESNORM, SILU):
        out.append(DCase(300, 256, 1024, v(5), epi, 0, 2))
    # not filtered here: this family's predicate asks the device for its CU count, which must
    # not happen while tests are collected; run_dcase asserts it (grids of at most 10 workgroups)
    return out


def dcase_expected(c):
    """CPU only: (operands, ss_in or None, eps, residual ints, ln, expected tensors)."""
    o, yi = oracle(c.M, c.N, c.K, c.operand_vmax)
    ri = ln = ss_in = None
    eps = EPS
    if c.epi == RESNORM:
        ri, ln = resnorm_inputs(c.M, c.N)
    if c.scaled == 1:
        assert c.epi == STORE
        g = torch.Generator().manual_seed(_seed(c.M, c.K, 5))
        ss_in = torch.rand(c.M, generator=g) * c.K + 1.0
        want = ref.exact_gemm_expected(yi, o.unit, STORE,
                                       row_scale=1.0 / torch.sqrt(ss_in.double() / c.K + EPS))
    elif c.scaled == 2:
        assert c.K & (c.K - 1) == 0
        j = torch.arange(c.M) % 4
        ss_in, eps = (c.K * 4.0 ** j).float(), 0.0
        want = ref.exact_gemm_expected(yi, o.unit, c.epi, residual_i=ri, ln=ln, row_shift=j)
    else:
        want = ref.exact_gemm_expected(yi, o.unit, c.epi, residual_i=ri, ln=ln)
    return o, ss_in, eps, ri, ln, want


def run_dcase(c, family):
    v = c.v
    M, N, K, epi = c.M, c.N, c.K, c.epi
    assert c.supported(), "the enumeration lists a combination the launcher refuses"
    o, ss_cpu, eps, ri, ln_cpu, want = dcase_expected(c)
    x, w = o.x.to(DEV), o.w.to(DEV)
    dev = x.device
    inl = c.combines_in_launch()
    cols = N // 2 if epi == SILU else N
    # a row-strided output: not for the dense residual stream, nor the separate reduce pass
    strided = epi != RESNORM and (v.splitk == 1 or inl)
    out = Canary(M, cols, strided)
    ss_in = None if ss_cpu is None else ss_cpu.to(DEV)
    ss_big = a_big = a = ln = None
    if epi == RESNORM:
        ln = ln_cpu.to(DEV)
        res0 = (ri.double() * o.unit).to(torch.bfloat16).to(DEV)
        out.view.copy_(res0)
        a_big, a = flat_canary(M * N, torch.bfloat16, SENT)
        a = a.view(M, N)
        ss_big, _ = flat_canary(M, torch.float32, SENT_SS, fill=0.0, tail=5)
    if v.family == "kgemm":
        ws_big = counters = None
        torch.ops.akap.kgemm(out.view, x, w, v.km, epi, eps, ss_in, ss_big, a, ln)
    else:
        need, counters = ops.dgemm_workspace(M, N, v, ops.PRO_PLAIN, dev)
        n_ws = need.numel() if v.splitk > 1 else 0
        ws_big, ws = flat_canary(n_ws, torch.float32, SENT_F32) if n_ws else (None, need)
        torch.ops.akap.dgemm(out.view, x, w, ws, ops.PRO_PLAIN, v.splitk, v.pf, None, None, None,
                             eps, epi, ss_in, ss_big, a, ln, v.bn, v.ns, counters, v.bm)
    torch.cuda.synchronize()

    # ---- the contract
    if c.scaled == 1:
        assert_ulp(out.view, want.out, ULP_SS_IN, f"{family}/ss_in")
    elif epi == SILU:
        assert_ulp(out.view, want.out, ULP_SILU, f"{family}/silu")
    elif epi == RESNORM:
        assert_bits(out.view, want.out, "residual")
        assert_bits(a, want.a, "a_out")
        assert_bits(ss_big[:M], want.ss, "ss_out")
    else:
        assert_bits(out.view, want.out, "y")

    # ---- nothing written outside the outputs
    assert out.intact(), "output sentinel rows / columns overwritten"
    if epi == RESNORM:
        assert tail_intact(a_big, M * N, SENT), "write past a_out"
        assert tail_intact(ss_big, M, SENT_SS), "write past ss_out[M]"
    if ws_big is not None:
        assert tail_intact(ws_big, n_ws, SENT_F32), "write past the split-K workspace"
    if inl:
        assert not bool(ops.gemm_counters(dev).any()), "an in-launch ticket (or GEMM_CTR_ERR) is left set"

    # ---- a second launch, through ops.dgemm, gives the same bits
    if epi == RESNORM:
        res2 = res0.clone()
        a2 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        ss2 = torch.zeros(M, device=DEV)
        ops.dgemm(x, w, out=res2, epi=epi, ss_in=ss_in, ss_out=ss2, a_out=a2, ln_out=ln, eps=eps,
                  variant=v)
        assert same_bits(res2, out.view) and same_bits(a2, a), "second launch differs"
        assert torch.equal(ss2, ss_big[:M]), "second launch: ss_out differs"
    else:
        out2 = ops.dgemm(x, w, epi=epi, ss_in=ss_in, eps=eps, variant=v)
        assert same_bits(out2, out.view), "second launch differs"
    if inl:
        assert not bool(ops.gemm_counters(dev).any()), "ticket left set by the second launch"
    RAN[family] += 1


RING_CASES = _ring_cases()
LDS_CASES = _lds_cases()
KGEMM_CASES = _kgemm_cases()
PGEMM_SK_CASES = _pgemm_sk_cases()
_ids = lambda cases: [c.id for c in cases]  # noqa: E731


@pytest.mark.parametrize("case", RING_CASES, ids=_ids(RING_CASES))
def test_exact_ring(case):
    """dgemm.hip, plain prologue: pf 1|2|4|8, split-K 1..16 through the reduce pass (its
    element- and row-parallel forms) and 2|4|8 combined in the launch, every epilogue."""
    run_dcase(case, "ring")


@pytest.mark.parametrize("case", LDS_CASES, ids=_ids(LDS_CASES))
def test_exact_lds(case):
    """gdgemm.hip: 64/128/256-row x 64/128-column tiles, shallow and deep rings, K slices of
    one step, fewer steps than the ring and many; reduce pass and in-launch combine."""
    run_dcase(case, "lds")


@pytest.mark.parametrize("case", KGEMM_CASES, ids=_ids(KGEMM_CASES))
def test_exact_kgemm(case):
    """kgemm.hip: 16- and 32-row tiles, store and residual epilogues."""
    run_dcase(case, "kgemm")


@pytest.mark.parametrize("case", PGEMM_SK_CASES, ids=_ids(PGEMM_SK_CASES))
def test_exact_pgemm_sk(case):
    """pgemm.hip split-K body (dgemm bn = 256): uneven K splits, every epilogue, and no
    combine timed out (GEMM_CTR_ERR is part of the ticket array checked to be zero)."""
    run_dcase(case, "pgemm_sk")


# --------------------------------------------------- the launch contract the binding checks
CONTRACT_VARIANTS = [Variant(2, 2), Variant(2, 2, inlaunch=True), Variant(2, 1, 64),
                     Variant(2, 1, 128, inlaunch=True)]


@pytest.mark.parametrize("v", CONTRACT_VARIANTS, ids=lambda v: f"s{v.splitk}{v.name}")
def test_contract_sizes_are_what_the_binding_accepts(v):
    """A workspace and tickets of exactly the sizes dgemm_contract (host_contract.h) gives are
    accepted by torch.ops.akap.dgemm and the result is bit-exact; one float less, or one ticket
    line less, is refused by the host check before anything is launched."""
    M, N, K = 16, 256, 512
    ok, _, inl, ws_floats, ticket_ints = ops._dgemm_contract(
        M, N, K, ops.PRO_PLAIN, STORE, v.splitk, v.pf, v.bn, v.ns, v.bm, v.inlaunch)
    assert ok and inl == v.inlaunch and ws_floats >= v.splitk * M * N
    assert (ticket_ints > 0) == v.inlaunch
    o, yi = oracle(M, N, K, vmax_for(K, N, STORE))
    x, w = o.x.to(DEV), o.w.to(DEV)
    out = torch.full((M, N), SENT, dtype=torch.bfloat16, device=DEV)

    def launch(ws, tickets):
        torch.ops.akap.dgemm(out, x, w, ws, ops.PRO_PLAIN, v.splitk, v.pf, None, None, None, EPS,
                             STORE, None, None, None, None, v.bn, v.ns, tickets, v.bm)

    ws = torch.empty(ws_floats, dtype=torch.float32, device=DEV)
    tickets = torch.zeros(ticket_ints, dtype=torch.int32, device=DEV) if ticket_ints else None
    with pytest.raises(RuntimeError, match="workspace"):
        launch(ws[:-1], tickets)
    if tickets is not None:
        with pytest.raises(RuntimeError, match="counters"):
            launch(ws, tickets[:-ops.CTR_STRIDE])
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused launch wrote its output"
    launch(ws, tickets)
    assert_bits(out, ref.exact_gemm_expected(yi, o.unit, STORE).out, "y")
    assert tickets is None or not bool(tickets.any()), "ticket left set"


# ------------------------------------------------------------------------------- gemm.hip
# (M, N, K, in-launch): split-K from ops.gemm_splitk
GEMM_CASES = [(37, 1000, 2048, False), (37, 1000, 2048, True), (300, 1000, 64, False),
              (64, 256, 512, False), (64, 256, 512, True), (130, 320, 1024, True),
              (1, 1000, 4096, False), (37, 256, 896, False)]


@pytest.mark.parametrize("M,N,K,inl", GEMM_CASES)
def test_exact_gemm(M, N, K, inl):
    """gemm.hip through torch.ops.akap.gemm: checked and full-tile kernels, split-K from
    gemm_splitk with the separate reduce and with in-launch tickets, row-strided output."""
    vmax = 3 if K == 896 else 0
    o, yi = oracle(M, N, K, vmax or ref.exact_vmax(K))
    x, w = o.x.to(DEV), o.w.to(DEV)
    s = ops.gemm_splitk(M, N, K)
    assert s == torch.ops.akap.gemm_splitk(M, N, K)
    out = Canary(M, N, True)
    ws_big, ws = flat_canary(s * M * N if s > 1 else 1, torch.float32, SENT_F32)
    tiles = -(-M // 64) * -(-N // 64)
    counters = torch.zeros(tiles * ops.CTR_STRIDE, dtype=torch.int32, device=DEV) if inl else None
    want = ref.exact_gemm_expected(yi, o.unit).out
    for launch in range(2):
        torch.ops.akap.gemm(out.view, x, w, ws, s, counters)
        assert_bits(out.view, want, f"y (launch {launch})")
        assert out.intact(), "output sentinel rows / columns overwritten"
        assert tail_intact(ws_big, ws.numel(), SENT_F32), "write past the split-K workspace"
        assert counters is None or not bool(counters.any()), "ticket left set"
    RAN["gemm"] += 1


# ------------------------------------------------------------------------------- wgemm.hip
WGEMM_CASES = [(M, N, K) for M in (37, 65, 130, 256, 300) for N, K in ((1000, 1024), (1004, 64))]


@pytest.mark.parametrize("M,N,K", WGEMM_CASES)
def test_exact_wgemm(M, N, K):
    """wgemm.hip: 64-, 128- and 256-row tiles and more than 256 rows; N = 1000 (a partial
    column tile) and N = 1004 (N % 8 != 0, inside a 1016-column buffer: rows stay 16-byte
    aligned)."""
    o, yi = oracle(M, N, K, ref.exact_vmax(K))
    x, w = o.x.to(DEV), o.w.to(DEV)
    out = Canary(M, N, True, pad_cols=PAD_COLS + (-N) % 8)
    want = ref.exact_gemm_expected(yi, o.unit).out
    for launch in range(2):
        ops.wgemm(x, w, out=out.view)
        assert_bits(out.view, want, f"y (launch {launch})")
        assert out.intact(), "output sentinel rows / columns overwritten"
    RAN["wgemm"] += 1


# ------------------------------------------------------------------------------- pgemm.hip
# (kind, M or group row counts, N, K)
PGEMM_CASES = [("dense", 1, 256, 64), ("dense", 300, 512, 128), ("dense", 37, 256, 896),
               ("dense", 257, 256, 1024),
               ("silu", 300, 512, 256), ("silu", 37, 256, 64), ("silu", 37, 256, 896),
               ("grouped", (130, 0, 1, 257, 0, 40), 256, 128),
               ("grouped", (0, 0, 65), 512, 1024),
               ("grouped-silu", (130, 0, 1, 257, 0, 40), 256, 128)]
_pg_id = lambda c: f"{c[0]}-{c[1] if isinstance(c[1], int) else 'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}"  # noqa: E731,E501


@functools.lru_cache(maxsize=None)
def grouped_oracle(counts, N, K):
    """x [sum(counts), K], w [G, N, K] and the exact accumulator of rows of group g vs w[g]."""
    M, G = sum(counts), len(counts)
    vmax = ref.exact_vmax(K)
    o = ref.exact_gemm_operands(M, G * N, K, _seed(M, G, N, K), vmax)
    wi = o.wi.view(G, N, K)
    yi = torch.zeros(M, N, dtype=torch.int64)
    lo = 0
    for g, n in enumerate(counts):
        yi[lo:lo + n] = ref.exact_int_matmul(o.xi[lo:lo + n], wi[g])
        lo += n
    return o, yi


@pytest.mark.parametrize("case", PGEMM_CASES, ids=_pg_id)
def test_exact_pgemm(case):
    """pgemm.hip through ops.pgemm: dense store and SwiGLU, expert-grouped with empty, 1-row
    and non-tile-multiple groups; row tails on the 256-row tile; row-strided output."""
    kind, m, N, K = case
    silu = kind.endswith("silu")
    if kind.startswith("grouped"):
        o, yi = grouped_oracle(m, N, K)
        M = sum(m)
        w = o.w.view(len(m), N, K).to(DEV)
        offs = torch.tensor(m, dtype=torch.int32).cumsum(0).to(torch.int32).to(DEV)
    else:
        M = m
        o, yi = oracle(M, N, K, 3 if K == 896 else ref.exact_vmax(K))
        w, offs = o.w.to(DEV), None
    assert ops.pgemm_supported(M, N, K)
    x = o.x.to(DEV)
    out = Canary(M, N // 2 if silu else N, True)
    want = ref.exact_gemm_expected(yi, o.unit, SILU if silu else STORE).out
    for launch in range(2):
        ops.pgemm(x, w, silu=silu, offs=offs, out=out.view)
        if silu:
            assert_ulp(out.view, want, ULP_SILU, "pgemm/silu")
        else:
            assert_bits(out.view, want, f"y (launch {launch})")
        assert out.intact(), "output sentinel rows / columns overwritten"
        if launch == 0:
            first = out.view.clone()
    assert same_bits(first, out.view), "second launch differs"
    RAN["pgemm"] += 1


# ------------------------------------------------------------------------------- qgemm.hip
def qgemm_geometry(M, N):
    """(bm, bn) of the tile launch_qgemm picks (qgemm_geometry of host_contract.h)."""
    return _runtime_loader.contract().qgemm_geometry(M, N, 64)[:2]


# one shape per geometry qgemm_geometry returns for M <= 256
QGEMM_CASES = [(1, 320, 1024), (16, 4104, 64), (1, 16384, 64), (17, 320, 512), (32, 16392, 64),
               (37, 1000, 896), (130, 8200, 64), (256, 320, 256)]
QGEMM_GEOMETRIES = {(16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 32), (64, 64)}


@functools.lru_cache(maxsize=None)
def fp8_oracle(M, N, K):
    """x, e4m3 codes of non-zero integers, power-of-two channel scales 2^-5 .. 2^-8, and the
    exact accumulator (in code units, before the scale)."""
    vmax = 3 if K == 896 else ref.exact_vmax(K)
    o = ref.exact_gemm_operands(M, N, K, _seed(M, N, K, 8), vmax, w_shift=0)
    q = o.wi.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), o.wi.float())
    scale = 2.0 ** -(5 + torch.arange(N) % 4).double()
    return o, q.view(torch.uint8), scale, ref.exact_int_matmul(o.xi, o.wi)


@pytest.mark.parametrize("M,N,K", QGEMM_CASES)
def test_exact_qgemm(M, N, K):
    """qgemm.hip through torch.ops.akap.qgemm: every (bm, bn) geometry, row-strided output."""
    o, q, scale, yi = fp8_oracle(M, N, K)
    x = o.x.to(DEV)
    out = Canary(M, N, True)
    want = ref.exact_gemm_expected(yi, scale[None, :]).out
    for launch in range(2):
        torch.ops.akap.qgemm(out.view, x, q.to(DEV), scale.float().to(DEV))
        assert_bits(out.view, want, f"y (launch {launch})")
        assert out.intact(), "output sentinel rows / columns overwritten"
    RAN["qgemm"] += 1


def test_exact_qgemm_dequant_then_bf16():
    """M above 256: dequant_fp8 gives exactly wi * scale, and the bf16 GEMM on it is exact."""
    M, N, K = 300, 320, 512
    o, q, scale, yi = fp8_oracle(M, N, K)
    wbig, wflat = flat_canary(N * K, torch.bfloat16, SENT)
    wd = wflat.view(N, K)
    torch.ops.akap.dequant_fp8(wd, q.to(DEV), scale.float().to(DEV))
    assert_bits(wd, (o.wi.double() * scale[:, None]).to(torch.bfloat16), "dequantized weight")
    assert tail_intact(wbig, N * K, SENT)
    out = Canary(M, N, True)
    s = ops.gemm_splitk(M, N, K)
    ws = torch.empty(max(1, s * M * N), dtype=torch.float32, device=DEV)
    torch.ops.akap.gemm(out.view, o.x.to(DEV), wd, ws, s, None)
    assert_bits(out.view, ref.exact_gemm_expected(yi, scale[None, :]).out, "y")
    assert out.intact()
    RAN["qgemm_dequant"] += 1


# ------------------------------------------------------------------------------- MoE GEMMs
MOE_E, MOE_TOPK, MOE_COUNTS = 4, 2, (37, 0, 42, 1)   # rows per expert: one empty, tails


def hand_align(bm):
    """A hand-made moe_align result for MOE_COUNTS: (flat expert ids, sorted_ids, inv,
    tile_expert, padded rows).  Flat index i = token i // topk, slot i % topk."""
    ids = [e for e, n in enumerate(MOE_COUNTS) for _ in range(n)]
    n = len(ids)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).tolist()
    ids = [ids[p] for p in perm]
    cap = ops.moe_capacity(n, MOE_E, bm)
    sorted_ids = torch.full((cap,), n, dtype=torch.int32)
    inv = torch.full((n,), -1, dtype=torch.int32)
    tile_expert = torch.full((cap // bm,), -1, dtype=torch.int32)
    pos = 0
    for e in range(MOE_E):
        idx = [i for i, x in enumerate(ids) if x == e]
        for j, i in enumerate(idx):
            sorted_ids[pos + j] = i
            inv[i] = pos + j
        nt = -(-len(idx) // bm)
        tile_expert[pos // bm:pos // bm + nt] = e
        pos += nt * bm
    return ids, sorted_ids, inv, tile_expert, pos


@functools.lru_cache(maxsize=None)
def moe_oracle(bm, N, K, gather, pad_zero):
    """Operands of a grouped GEMM over the hand-made alignment: a (token rows when gathering,
    else one row per sorted position), w [E, N, K], and per used row the A row it reads and its
    expert.  pad_zero: padding rows of a gathering launch read zeros (moe_gemm) instead of
    row 0 (moe_dgemm)."""
    ids, sorted_ids, inv, tile_expert, used = hand_align(bm)
    n, cap = len(ids), sorted_ids.numel()
    rows_a = n // MOE_TOPK if gather else cap
    vmax = ref.exact_vmax(K)
    o = ref.exact_gemm_operands(rows_a, MOE_E * N, K, _seed(bm, N, K, gather), vmax)
    r = torch.arange(used)
    if gather:
        sid = sorted_ids[:used].long()
        arow = torch.where(sid < n, sid // MOE_TOPK, torch.zeros_like(sid))
        live = sid < n
    else:
        arow, live = r, torch.ones(used, dtype=torch.bool)
    expert = tile_expert[r // bm].long()
    xi = o.xi[arow]
    if gather and pad_zero:
        xi = xi * live[:, None]
    return o, xi, o.wi.view(MOE_E, N, K), expert, (sorted_ids, inv, tile_expert, used, n)


def moe_int_matmul(xi, wi, expert, k0=0, k1=None):
    yi = torch.zeros(xi.shape[0], wi.shape[1], dtype=torch.int64)
    for e in range(wi.shape[0]):
        m = expert == e
        if bool(m.any()):
            yi[m] = ref.exact_int_matmul(xi[m][:, k0:k1], wi[e][:, k0:k1])
    return yi


MOE_GEMM_CASES = [(g, N, K) for g in (True, False) for N, K in ((320, 64), (72, 200), (256, 1024))]


@pytest.mark.parametrize("gather,N,K", MOE_GEMM_CASES)
def test_exact_moe_gemm(gather, N, K):
    """moe.hip moe_gemm (64-row tiles): gathered token rows and sorted rows, an empty expert,
    padding rows (zeros when gathering), K and N that are no multiple of the tile."""
    o, xi, wi, expert, (sorted_ids, _, tile_expert, used, n) = moe_oracle(64, N, K, gather, True)
    rows = tile_expert.numel() * 64
    out = Canary(rows, N, False)
    a, w = o.x.to(DEV), o.w.view(MOE_E, N, K).to(DEV)
    want = ref.exact_gemm_expected(moe_int_matmul(xi, wi, expert), o.unit).out
    for launch in range(2):
        torch.ops.akap.moe_gemm(out.view, a, w, sorted_ids.to(DEV), tile_expert.to(DEV), n,
                                MOE_TOPK, gather)
        assert_bits(out.view[:used], want, f"y (launch {launch})")
        assert bool((out.view[used:] == SENT).all()), "rows of tiles without an expert written"
        assert out.intact()
    RAN["moe_gemm"] += 1


def _moe_dgemm_cases():
    out = []
    for bm in (32, 64):
        for pf in (1, 2, 4):
            for splitk in (1, 2, 4):
                for gather in (True, False):
                    for silu in (True, False):
                        # one pipeline fill per slice, or (pf 1, and the bm = 64 x 4 slices
                        # case) several wraps
                        steps = 8 if (pf == 1 or (bm == 64 and splitk == 4)) else 1
                        K = splitk * pf * 64 * steps
                        if (K % splitk == 0 and (K // splitk) % (64 * pf) == 0
                                and not (silu and splitk > 1)):   # moe_dgemm_supported, N = 320
                            out.append((bm, pf, splitk, gather, silu, 320, K))
    return out


MOE_DGEMM_CASES = _moe_dgemm_cases()


@pytest.mark.parametrize("bm,pf,splitk,gather,silu,N,K", MOE_DGEMM_CASES)
def test_exact_moe_dgemm(bm, pf, splitk, gather, silu, N, K):
    """moe_dgemm.hip called directly: 32- and 64-row tiles, every ring depth, K slices as
    exact fp32 partials (each slice compared with its own integer product), gather and
    SwiGLU on and off, an empty expert, last tiles with padding rows (they read row 0), and
    moe_combine_split / moe_combine on the result with power-of-two routing weights."""
    o, xi, wi, expert, (sorted_ids, inv, tile_expert, used, n) = moe_oracle(bm, N, K, gather, False)
    rows = tile_expert.numel() * bm
    a, w = o.x.to(DEV), o.w.view(MOE_E, N, K).to(DEV)
    sid, te = sorted_ids.to(DEV), tile_expert.to(DEV)
    T, d = n // MOE_TOPK, N
    g = torch.Generator().manual_seed(_seed(bm, pf, splitk))
    wts = 2.0 ** -torch.randint(1, 4, (T, MOE_TOPK), generator=g).float()
    inv2 = inv.clone()
    inv2[5] = -1                                   # a skipped (expert-parallel padding) slot
    live = (inv2 >= 0).view(T, MOE_TOPK)
    yi = moe_int_matmul(xi, wi, expert)
    if splitk > 1:
        pbig, pflat = flat_canary(splitk * rows * N, torch.float32, SENT_F32)
        P = pflat.view(splitk, rows, N)
        kps = K // splitk
        for launch in range(2):
            torch.ops.akap.moe_dgemm(pflat, a, w, sid, te, n, MOE_TOPK, gather, False, pf, bm,
                                     splitk)
            for z in range(splitk):
                want = moe_int_matmul(xi, wi, expert, z * kps, (z + 1) * kps).double() * o.unit
                assert_bits(P[z, :used], want.float(), f"partial slice {z} (launch {launch})")
                assert bool((P[z, used:] == SENT_F32).all()), "rows of expert-less tiles written"
            assert tail_intact(pbig, pflat.numel(), SENT_F32), "write past the partials"
        # combine: out[t] = bf16(sum_k w[t, k] * sum_z P[z, inv[t, k]]), exact for 2^-j weights
        cbig, cflat = flat_canary(T * d, torch.bfloat16, SENT)
        torch.ops.akap.moe_combine_split(pflat, wts.to(DEV), inv2.to(DEV), cflat.view(T, d),
                                         splitk, rows)
        acc = (yi[inv2.clamp(min=0).long()].view(T, MOE_TOPK, d).double() * o.unit
               * (wts.double() * live)[:, :, None]).sum(1)
        assert_bits(cflat.view(T, d), acc.float().to(torch.bfloat16), "moe_combine_split")
        assert tail_intact(cbig, T * d, SENT)
    else:
        cols = N // 2 if silu else N
        out = Canary(rows, cols, False)
        want = ref.exact_gemm_expected(yi, o.unit, SILU if silu else STORE).out
        for launch in range(2):
            torch.ops.akap.moe_dgemm(out.view, a, w, sid, te, n, MOE_TOPK, gather, silu, pf, bm, 1)
            if silu:
                assert_ulp(out.view[:used], want, ULP_SILU, "moe_dgemm/silu")
            else:
                assert_bits(out.view[:used], want, f"y (launch {launch})")
            assert bool((out.view[used:] == SENT).all()), "rows of expert-less tiles written"
            assert out.intact()
            if launch == 0:
                first = out.view.clone()
        assert same_bits(first, out.view), "second launch differs"
        if not silu:
            cbig, cflat = flat_canary(T * d, torch.bfloat16, SENT)
            torch.ops.akap.moe_combine(out.view, wts.to(DEV), inv2.to(DEV), cflat.view(T, d))
            y = want.double()[inv2.clamp(min=0).long()].view(T, MOE_TOPK, d)
            acc = (y * (wts.double() * live)[:, :, None]).sum(1)
            assert_bits(cflat.view(T, d), acc.float().to(torch.bfloat16), "moe_combine")
            assert tail_intact(cbig, T * d, SENT)
    RAN["moe_dgemm"] += 1


def test_moe_dgemm_binding_refusals():
    """The moe_dgemm binding refuses what would read out of bounds or misaligned, as the FP8 and
    MXFP4 bindings do.  One 32-row tile of 2 experts, N = 32, K = 64; every call is refused before
    a kernel runs."""
    E, N, K, bm, topk, T = 2, 32, 64, 32, 2, 8
    n = T * topk
    sid = torch.full((bm,), n, dtype=torch.int32, device=DEV)
    sid[:n] = torch.arange(n, dtype=torch.int32)
    te = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = torch.zeros(T, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(E, N, K, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(bm, N, dtype=torch.bfloat16, device=DEV)
    call = lambda a_, topk_=topk, bm_=bm: torch.ops.akap.moe_dgemm(  # noqa: E731
        out, a_, w, sid, te, n, topk_, True, False, 1, bm_, 1)
    with pytest.raises(RuntimeError, match="topk >= 1"):
        call(a, topk_=0)
    with pytest.raises(RuntimeError, match="a rows must cover"):
        call(a[:T - 1])                                  # gathered a one token row short
    with pytest.raises(RuntimeError, match="tile rows 32"):
        call(a, bm_=48)
    off = torch.zeros(T * K + 8, dtype=torch.bfloat16, device=DEV)[1:1 + T * K].view(T, K)
    with pytest.raises(RuntimeError, match="a must be 16-byte aligned"):
        call(off)                                        # a offset by one element


# ------------------------------------------------------------------------- environment knobs
FAMILY_CASES = {
    "ring": ("test_exact_ring", RING_CASES), "lds": ("test_exact_lds", LDS_CASES),
    "kgemm": ("test_exact_kgemm", KGEMM_CASES), "pgemm_sk": ("test_exact_pgemm_sk", PGEMM_SK_CASES),
    "gemm": ("test_exact_gemm", GEMM_CASES), "wgemm": ("test_exact_wgemm", WGEMM_CASES),
    "pgemm": ("test_exact_pgemm", PGEMM_CASES), "qgemm": ("test_exact_qgemm", QGEMM_CASES),
    "qgemm_dequant": ("test_exact_qgemm_dequant_then_bf16", [None]),
    "moe_gemm": ("test_exact_moe_gemm", MOE_GEMM_CASES),
    "moe_dgemm": ("test_exact_moe_dgemm", MOE_DGEMM_CASES),
}


def _reduced_dcases(cases):
    """One row-tail and one wrap-around shape per epilogue (plus the ss_in cases)."""
    out, seen = [], set()
    for c in cases:
        nk = c.K // c.v.splitk // 64
        key = (c.epi, nk >= 8, c.scaled, c.v.km, bool(c.v.bn) and c.v.bm)
        tail = c.M % (c.v.bm if c.v.bn else 64) != 0
        if tail and key not in seen and not c.vmax and (c.v.splitk > 1 or nk >= 8 or c.scaled):
            seen.add(key)
            out.append(c)
    return out


def reduced_selection(families):
    """-k free: explicit node ids of the reduced selection for the knob children."""
    me = "tests/test_gemm_exact_gpu.py"
    nodes = []
    for f in families:
        name, cases = FAMILY_CASES[f]
        if f in ("ring", "lds", "kgemm", "pgemm_sk"):
            nodes += [f"{me}::{name}[{c.id}]" for c in _reduced_dcases(cases)]
        elif f == "pgemm":
            nodes += [f"{me}::{name}[{_pg_id(c)}]" for c in cases if c[1] != 1]
        else:  # moe_dgemm: every case is a few launches on one small routing
            nodes.append(f"{me}::{name}")
    return nodes + [f"{me}::test_zz_case_counts"]


KNOBS = [
    ({}, ("ring", "lds", "kgemm", "pgemm_sk", "pgemm", "moe_dgemm")),   # the baseline child
    ({"AKAP_GEMM_STAGGER": "1"}, ("ring", "lds")),
    ({"AKAP_WEIGHT_NT": "0"}, ("lds", "kgemm")),
    ({"AKAP_WEIGHT_NT": "1"}, ("lds", "kgemm")),
    ({"AKAP_PGEMM_SCHED": "1"}, ("pgemm", "pgemm_sk")),
    ({"AKAP_PGEMM_SCHED": "2"}, ("pgemm", "pgemm_sk")),
    ({"AKAP_PGEMM_SCHED": "3", "AKAP_PGEMM_STAGGER": "1"}, ("pgemm",)),
    ({"AKAP_PGEMM_WAVES": "4"}, ("pgemm", "pgemm_sk")),
    ({"AKAP_PGEMM_WAVES": "4", "AKAP_PGEMM_SCHED": "2"}, ("pgemm", "pgemm_sk")),
    ({"AKAP_PGEMM_GM": "2"}, ("pgemm",)),
    ({"AKAP_MOE_NT": "0"}, ("moe_dgemm",)),
    ({"AKAP_MOE_NT": "1"}, ("moe_dgemm",)),
]
KNOB_VARS = sorted({k for env, _ in KNOBS for k in env})
# The unset-environment child (the largest selection) took CHILD_BASELINE_S seconds on an MI355X,
# most of it interpreter and library start-up; every child gets 15 times that
# (profiles/gemm_exact_tests.md).
CHILD_BASELINE_S = 8
CHILD_TIMEOUT_S = 120
_child_died = []


@pytest.mark.parametrize("env,families", KNOBS,
                         ids=[",".join(f"{k}={v}" for k, v in e.items()) or "unset" for e, _ in KNOBS])
def test_env_knob(env, families):
    """Kernel paths behind environment variables read once per process: each setting runs the
    reduced selection of the exact cases of the families it touches in a fresh child process,
    one child at a time; after a child that died (signal, abort, timeout) nothing more is
    started on the GPU."""
    assert not os.environ.get(CHILD_FLAG), "a knob child must not start children"
    if _child_died:
        pytest.fail(f"not run: an earlier child died ({_child_died[0]})")
    nodes = reduced_selection(families)
    assert len(nodes) > 1
    if "AKAP_GEMM_STAGGER" in env:  # else the knob changes nothing and the child tests nothing
        picked = [c for f in families for c in _reduced_dcases(FAMILY_CASES[f][1])]
        assert picked and all(c.stagger_exercised() for c in picked if c.K // c.v.splitk > 64)
        assert sum(c.stagger_exercised() for c in picked) >= 4
    child_env = {k: v for k, v in os.environ.items() if k not in KNOB_VARS}
    child_env.update(env)
    child_env[CHILD_FLAG] = "1"
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", *nodes]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=child_env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _child_died.append(f"{env or 'unset'}: no result after {CHILD_TIMEOUT_S} s")
        pytest.fail(f"child timed out: {_child_died[0]}")
    took = time.time() - t0
    print(f"[knob child] {env or 'unset'}: {took:.1f} s, exit {r.returncode}")
    tail = (r.stdout + r.stderr)[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in tail:
        _child_died.append(f"{env or 'unset'}: exit {r.returncode}")
        pytest.fail(f"child died ({r.returncode}):\n{tail}")
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{tail}"
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], tail


# ------------------------------------------------------------------------------- the count
def test_zz_case_counts(request):
    """Every enumerated case of every family ran to the end: a family that silently skipped,
    or was never collected, fails here.  (A knob child checks the cases it was given.)"""
    by_name = {name: f for f, (name, _) in FAMILY_CASES.items()}
    selected = collections.Counter()
    for it in request.session.items:
        f = by_name.get(getattr(it, "originalname", None) or it.name.split("[")[0])
        if f and it.fspath == request.node.fspath:
            selected[f] += 1
    print("[ulp] observed:", dict(OBSERVED_ULP))
    print("[cases] ran:", dict(RAN))
    assert sum(selected.values()) > 0
    if not os.environ.get(CHILD_FLAG):
        for f, (_, cases) in FAMILY_CASES.items():
            assert len(cases) > 0 and selected[f] == len(cases), (
                f"{f}: {selected[f]} of {len(cases)} enumerated cases were collected")
    for f, n in selected.items():
        assert RAN[f] == n, f"{f}: {RAN[f]} of {n} cases ran to the end"
