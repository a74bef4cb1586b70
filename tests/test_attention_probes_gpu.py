"""Attention probes: inputs for which one wrong key, V group, stale slot or rescale is loud.

The statistical attention tests (test_kernels_gpu.py) feed randn q and K: the softmax is nearly
uniform and a fault confined to one key moves the output by ~1 / kv_len.  Here
  * NEEDLE queries are beta times one cached key (ops.reference.needle_q): the softmax is
    one-hot, the expected output is the target's V row itself (no attention reference at run
    time) and is compared within max(1 bf16 ulp, 1e-6);
  * FORBIDDEN needles align with a key the row must not see (prefill: key limit + 1; decode:
    the slot at position kv_len) and are compared with ops.reference.paged_attention;
  * every stale cache slot and every unused block-table entry is POISONED (large, finite, in
    range: ops.reference.poison_stale states the contract);
  * SCORE PATTERNS put the tile maxima of a row where the prefill kernel's deferred running
    max and the decode combine must rescale (ops.reference.score_pattern), and zero queries
    test the denominators alone; both are compared with ops.reference.paged_attention at the
    tolerances the statistical tests carry.
The case lists are built on the CPU, seeded, and shared with tests/test_attention_probes_cpu.py,
which proves there that the reference satisfies every needle row, that the patterns cross the
threshold as stated and that each comparator fails under five reference-level mutations.
Kernel variants behind once-per-process environment variables run a reduced selection in a
fresh child process each (test_env_knob); test_zz_probe_counts checks every case ran.
"""
import collections
import functools
import math
import os
import subprocess
import sys
import time

import pytest
import torch

from aws_k8s_ansible_provisioner_amd import ops
from aws_k8s_ansible_provisioner_amd.ops import reference as ref
from test_kernels_gpu import _setup_attn, _tiles, _to_fp8_cache

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, BS, HKV = 128, 32, 8
SCALE = 1 / math.sqrt(D)
EPS = 1e-6
TOL_BF16, TOL_FP8_PREFILL, TOL_FP8_DECODE, TOL_FP8_FUSED = 2e-2, 2e-2, 3e-2, 4e-2
CHILD_FLAG = "AKAP_ATTN_PROBE_CHILD"   # set in the knob children: they start no children

RAN = collections.Counter()                     # family -> cases that ran to the end
OBSERVED_ULP = collections.defaultdict(int)     # family -> largest needle ulp distance seen
OBSERVED_RATIO = collections.defaultdict(float)  # family -> worst err / limit of the other rows


@pytest.fixture(scope="module", autouse=True)
def _native():
    ops.load_native(required=True)


# ------------------------------------------------------------------------------- probes
class Probe:
    """The inputs of one case and what its output must be.  needle [T, Hq]: rows whose
    expected output is expect[t, h] (a V row); the others are compared with the reference."""

    def __init__(self, **kw):
        self.q_ref = None
        self.__dict__.update(kw)
        self._ref = None

    def ref_out(self):
        """ops.reference.paged_attention over the sequences that hold a non-needle row."""
        if self._ref is None:
            q = self.q if self.q_ref is None else self.q_ref
            out = torch.zeros_like(q)
            qs = self.qs.long()
            rest = ~self.needle.all(dim=1)
            seqs = [s for s in range(self.sl.numel()) if bool(rest[qs[s]:qs[s + 1]].any())]
            for s in seqs:
                a, b = int(qs[s]), int(qs[s + 1])
                out[a:b] = ref.paged_attention(
                    q[a:b], self.kc, self.vc, self.bt[s:s + 1], self.sl[s:s + 1],
                    torch.tensor([0, b - a], dtype=torch.int32), SCALE)
            self._ref = out
        return self._ref

    def ref_all(self):
        """The reference over every sequence (the CPU tests' stand-in for a kernel)."""
        q = self.q if self.q_ref is None else self.q_ref
        return ref.paged_attention(q, self.kc, self.vc, self.bt, self.sl, self.qs, SCALE)

    def check(self, out, family=None):
        """The case's assertion, on any [T, Hq, D] output."""
        out = out.cpu()
        ulp = ratio = 0
        if bool(self.needle.any()):
            bad, ulp = ref.needle_mismatch(out[self.needle], self.expect[self.needle])
            if family:
                print(f"[probe] {family}: needle max ulp {ulp}")
            assert not bool(bad.any()), (
                f"{int(bad.any(-1).sum())} of {int(self.needle.sum())} needle rows miss their V "
                f"row; first (token, head) {self.needle.nonzero()[bad.any(-1)][0].tolist()}")
        rest = ~self.needle
        if bool(rest.any()):
            bad, ratio = ref.close_mismatch(out[rest], self.ref_out()[rest], self.tol)
            if family:
                print(f"[probe] {family}: worst err / limit {ratio:.4f}")
            assert not bool(bad.any()), (
                f"{int(bad.any(-1).sum())} of {int(rest.sum())} reference rows past "
                f"{self.tol}: worst err / limit {ratio:.3g}; first (token, head) "
                f"{rest.nonzero()[bad.any(-1)][0].tolist()}")
        if family:
            OBSERVED_ULP[family] = max(OBSERVED_ULP[family], ulp)
            OBSERVED_RATIO[family] = max(OBSERVED_RATIO[family], ratio)
        return ulp, ratio


def _seed(*k):
    s = 0
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def _caches(seqs, Hq, seed, fp8, extra_cols=1):
    """randn paged caches for `seqs` (test_kernels_gpu._setup_attn), the block table widened by
    `extra_cols` unused columns, every stale slot and unused entry poisoned.
    -> (kc, vc, bt, sl, qs, pdir)"""
    _, kc, vc, bt, sl, qs = _setup_attn(seqs, Hq, HKV, BS, seed=seed)
    used = set()
    for s, (kv, _) in enumerate(seqs):
        used |= set(bt[s, :(kv + BS - 1) // BS].tolist())
    spare = [b for b in range(kc.shape[0]) if b not in used]
    assert len(spare) >= 3
    bt = torch.cat([bt, torch.zeros(bt.shape[0], extra_cols, dtype=torch.int32)], dim=1)
    if fp8:
        kc, vc = _to_fp8_cache(kc, vc)
    pdir = ref.poison_direction(HKV, D, seed + 1)
    ref.poison_stale(kc, vc, bt, sl, spare[0], pdir)
    assert int(bt.min()) >= 0 and int(bt.max()) < kc.shape[0]
    return kc, vc, bt, sl, qs, pdir


def _tokens(kc, vc, bt_row):
    """K, V of every slot a block-table row names, stale and poison slots included."""
    n = bt_row.numel() * BS
    return ref.gather_kv(kc, vc, bt_row, n)


# ------------------------------------------------------------------------------- decode sweep
SWEEP_LEN = 1500
SWEEP_SHORT = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257)
SWEEP_PLANS = [(1, 4096), (3, 512), (8, 256)]
SWEEP_CASES = [(G, fp8, parts, ps) for G in (2, 8) for fp8 in (False, True)
               for parts, ps in SWEEP_PLANS]


@functools.lru_cache(maxsize=None)
def sweep_probe(G, fp8):
    """Every key position of one 1500-token context is the needle of some (row, head) of each
    kv head: ceil(1500 / G) batch rows share the context's block-table row (block tables are
    read-only).  The short lengths are swept the same way twice: over the long context's own
    blocks (positions >= their kv_len hold its live keys) and over blocks of their own, whose
    stale slots and unused table entries are poisoned."""
    Hq = HKV * G
    lens = (SWEEP_LEN,) + SWEEP_SHORT
    kc, vc, bt, sl, _, _ = _caches([(L, 1) for L in lens], Hq, _seed(11, G), fp8)
    rows = [(0, L) for L in lens] + [(s, L) for s, L in enumerate(lens) if s]
    qs_, ex_, bt_, sl_, tg_, own_ = [], [], [], [], [], []
    for s, L in rows:
        K, V = ref.gather_kv(kc, vc, bt[s], L)
        n = (L + G - 1) // G
        r = torch.arange(n)[:, None]
        t = (r * G + (torch.arange(Hq) % G)[None]) % L
        qs_.append(ref.needle_q(K, t, G))
        ex_.append(ref.needle_expect(V, t, G))
        bt_.append(bt[s].expand(n, -1))
        sl_.append(torch.full((n,), L, dtype=torch.int32))
        tg_.append(t)
        own_.append(torch.full((n,), s, dtype=torch.int32))
    q = torch.cat(qs_)
    B = q.shape[0]
    return Probe(q=q, kc=kc, vc=vc, bt=torch.cat(bt_).contiguous(), sl=torch.cat(sl_),
                 qs=torch.arange(B + 1, dtype=torch.int32), expect=torch.cat(ex_),
                 needle=torch.ones(B, Hq, dtype=torch.bool), targets=torch.cat(tg_),
                 blocks_of=torch.cat(own_), G=G, tol=TOL_FP8_DECODE if fp8 else TOL_BF16)


def _run_decode(p, parts, ps):
    B, Hq = p.q.shape[0], p.q.shape[1]
    out = torch.empty(B, Hq, D, dtype=torch.bfloat16, device=DEV)
    ws = ops.decode_workspace(B, HKV, p.G, parts, DEV)
    ops.paged_attention_decode(out, p.q.to(DEV), p.kc.to(DEV), p.vc.to(DEV), p.bt.to(DEV),
                               p.sl.to(DEV), p.G, SCALE, workspace=ws, num_parts=parts,
                               part_size=ps)
    return out


def _sweep_id(c):
    return f"g{c[0]}-{'fp8' if c[1] else 'bf16'}-{c[2]}x{c[3]}"


@pytest.mark.parametrize("case", SWEEP_CASES, ids=_sweep_id)
def test_decode_sweep(case):
    """Plain decode kernel: all 1500 positions (and every position of the short contexts) as
    needles, per kv head, at the unsplit and two split-KV plans."""
    G, fp8, parts, ps = case
    p = sweep_probe(G, fp8)
    p.check(_run_decode(p, parts, ps), "decode_sweep")
    RAN["decode_sweep"] += 1


# ------------------------------------------------------------------------------- decode long
LONG_LEN = 32768
LONG_STALE_LEN = LONG_LEN - 11
LONG_PLANS = [(4, 8192), (128, 256)]
LONG_G = 8


def long_positions():
    edges = sorted({P for parts, ps in LONG_PLANS for P in range(ps, LONG_LEN, ps)})
    pos = {0, 1, LONG_LEN - 2, LONG_LEN - 1}
    for P in edges:
        pos |= {P - 1, P, P + 1}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def long_probe():
    """One 32768-token context (built once): needles at both ends and at P - 1, P, P + 1 of
    every partition edge of both plans; two forbidden rows -- one whose query aligns with the
    slot at position kv_len = 32768 (the poison block behind the unused table entry), one over
    the same blocks with kv_len = 32757 whose query aligns with the key at 32757."""
    G, Hq = LONG_G, HKV * LONG_G
    kc, vc, bt, sl, _, _ = _caches([(LONG_LEN, 1)], Hq, _seed(12), False)
    K, V = _tokens(kc, vc, bt[0])
    pos = torch.tensor(long_positions())
    n = (pos.numel() + G - 1) // G
    idx = (torch.arange(n)[:, None] * G + (torch.arange(Hq) % G)[None]) % pos.numel()
    t = pos[idx]
    forb = torch.tensor([LONG_LEN, LONG_STALE_LEN])[:, None].expand(2, Hq)
    targets = torch.cat([t, forb])
    unit = torch.cat([torch.zeros(n, Hq, dtype=torch.bool), torch.ones(2, Hq, dtype=torch.bool)])
    q = ref.needle_q(K, targets, G, unit=unit)
    expect = ref.needle_expect(V, targets, G)
    B = n + 2
    sl = torch.full((B,), LONG_LEN, dtype=torch.int32)
    sl[-1] = LONG_STALE_LEN
    return Probe(q=q, kc=kc, vc=vc, bt=bt[0].expand(B, -1).contiguous(), sl=sl,
                 qs=torch.arange(B + 1, dtype=torch.int32), expect=expect, needle=~unit,
                 targets=targets, G=G, tol=TOL_BF16)


@pytest.mark.parametrize("parts,ps", LONG_PLANS)
def test_decode_long_context(parts, ps):
    """32k context: the partition edges of a 4 x 8192 and a 128 x 256 plan, and the slot past
    the context's end."""
    p = long_probe()
    p.check(_run_decode(p, parts, ps), "decode_long")
    RAN["decode_long"] += 1


# ------------------------------------------------------------------------------- decode fused
FUSED_LENS = (1, 5, 8, 13, 31, 32, 33, 200, 777)
FUSED_PAD_LEN = 21          # one more row, slot = -1: writes nothing, attends what is cached
FUSED_PLANS = [(1, 4096), (3, 512)]
# (G, tail, qk_norm, fp8): fp8 caches have no V tail
FUSED_FORMS = [(2, False, False, False), (2, False, True, False), (2, True, False, False),
               (2, True, True, False), (2, False, False, True), (2, False, True, True),
               (8, True, True, False)]
FUSED_CASES = [f + pl for f in FUSED_FORMS for pl in FUSED_PLANS]
FUSED_KINDS = ("new", "len-2", "group-first", "prev-group-last", "first", "random")


@functools.lru_cache(maxsize=None)
def fused_probe(G, tail, qk_norm, fp8):
    """The serving decode step: raw QKV rows whose q part is the needle rotated back by the
    row's position (with q/k norm: weights q_w = 4, k_w = 1, so the normed q has length
    4 sqrt(128) whatever its raw length).  kc / vc are the caches AFTER the reference writer
    (what the reference attends); kc0 / vc0 what the kernel is handed: the new token's slot
    still unwritten, stale slots poisoned, and with a V tail the still-partial group in the
    tail and poison in the cache's copy of it."""
    Hq = HKV * G
    lens = FUSED_LENS + (FUSED_PAD_LEN,)
    B = len(lens)
    kc0, vc0, bt, sl, qs, _ = _caches([(L, 1) for L in lens], Hq, _seed(13, G, tail), fp8)
    g = torch.Generator().manual_seed(_seed(14, G, tail, qk_norm, fp8))
    qkv = torch.randn(B, (Hq + 2 * HKV) * D, generator=g).bfloat16()
    pos = (sl - 1).to(torch.int64)
    slots = torch.tensor([int(bt[s, int(pos[s]) // BS]) * BS + int(pos[s]) % BS
                          for s in range(B)], dtype=torch.int64)
    slots[B - 1] = -1
    cs = ref.rope_cos_sin(4096, D, 1e6)
    qw = torch.full((D,), 4.0).bfloat16() if qk_norm else None
    kw = torch.ones(D).bfloat16() if qk_norm else None
    kc, vc = kc0.clone(), vc0.clone()
    scratch = torch.empty(B, Hq, D).bfloat16()
    ref.qk_norm_rope_cache(qkv, scratch, kc, vc, pos, slots, cs, qw, kw, Hq, HKV, EPS)
    targets = torch.zeros(B, Hq, dtype=torch.int64)
    expect = torch.empty(B, Hq, D).bfloat16()
    for s, L in enumerate(lens):
        gs = (L - 1) & ~7
        cyc = [L - 1, L - 2, gs, gs - 1, 0, int(torch.randint(0, L, (1,), generator=g))]
        t = torch.tensor([max(cyc[(s * Hq + h) % 6], 0) for h in range(Hq)])[None]
        K, V = ref.gather_kv(kc, vc, bt[s], L)
        want = ref.needle_q(K, t, G, beta=1.0 if qk_norm else ref.NEEDLE_BETA).float()
        raw = ref.unrope(want, pos[s:s + 1], cs).to(torch.bfloat16)
        qkv[s, :Hq * D] = raw.reshape(-1)
        targets[s] = t[0]
        expect[s] = ref.needle_expect(V, t, G)[0]
    q_ref = torch.empty(B, Hq, D).bfloat16()
    k2, v2 = kc0.clone(), vc0.clone()
    ref.qk_norm_rope_cache(qkv, q_ref, k2, v2, pos, slots, cs, qw, kw, Hq, HKV, EPS)
    assert torch.equal(k2, kc) and torch.equal(v2, vc)   # the q part does not reach K / V
    v_tail = None
    if tail:
        v_tail = torch.zeros(B, HKV, 8, D).bfloat16()
        pv = torch.full((HKV, D), ref.POISON_V).bfloat16()
        for s, L in enumerate(lens):
            gs = (L - 1) & ~7
            b = int(bt[s, (L - 1) // BS])
            # the padding row writes nothing: its last token is cached already, so it belongs to
            # the tail too, and the fused kernel reads that row's group from the cache
            for pp in range(gs, L - 1 if slots[s] >= 0 else L):
                v_tail[s, :, pp - gs] = vc0[b, :, (pp % BS) // 8, :, pp % 8]
                if slots[s] >= 0:
                    vc0[b, :, (pp % BS) // 8, :, pp % 8] = pv
    return Probe(q=qkv, q_ref=q_ref, kc=kc, vc=vc, kc0=kc0, vc0=vc0, bt=bt, sl=sl, qs=qs,
                 pos=pos, slots=slots, cs=cs, qw=qw, kw=kw, v_tail=v_tail, expect=expect,
                 needle=torch.ones(B, Hq, dtype=torch.bool), targets=targets, G=G, fp8=fp8,
                 tol=TOL_FP8_FUSED if fp8 else TOL_BF16)


def _dq(t):
    return ref.from_cache(t.cpu()).float()


def check_fused_writes(p, kg, vg, tailg):
    """The new token's K row and V row (cache, or V tail while its group is partial; a
    completed group whole) against the reference writer, at the tolerances of
    test_paged_attention_decode_fused / _fp8."""
    kg, vg = kg.cpu(), vg.cpu()
    for s in range(p.sl.numel()):
        L, slot = int(p.sl[s]), int(p.slots[s])
        if slot < 0:
            continue
        Kg, Vg = ref.gather_kv(kg, vg, p.bt[s], L)
        Kr, Vr = ref.gather_kv(p.kc, p.vc, p.bt[s], L)
        a, b = Kg[L - 1].float(), Kr[L - 1].float()
        atol, rtol = (1e-2, 0.13) if p.fp8 else (3e-2, 2e-2)
        assert bool(((a - b).abs() <= atol + rtol * b.abs()).all()), f"new K row, sequence {s}"
        assert torch.equal(Kg[:L - 1], Kr[:L - 1]), f"older K rows changed, sequence {s}"
        if tailg is None:
            assert torch.equal(Vg[L - 1], Vr[L - 1]), f"new V row, sequence {s}"
        elif L % 8 == 0:   # the group completed: written to the cache whole
            assert torch.equal(Vg[L - 8:], Vr[L - 8:]), f"completed V group, sequence {s}"
        else:
            assert torch.equal(tailg[s, :, (L - 1) % 8].cpu(), Vr[L - 1]), f"V tail, sequence {s}"


def _fused_id(c):
    G, tail, norm, fp8, parts, ps = c
    return (f"g{G}-{'fp8' if fp8 else 'bf16'}-{'tail' if tail else 'cache'}-"
            f"{'norm' if norm else 'raw'}-{parts}x{ps}")


@pytest.mark.parametrize("case", FUSED_CASES, ids=_fused_id)
def test_decode_fused(case):
    """paged_attention_decode_fused: raw-QKV needles on the new token, its V group, the
    previous group, position 0 and a random position; the K / V it writes; a padding row.
    With a V tail the plain decode kernel then attends the caches and tail the step left (the
    cache's copy of a still-partial group is poison) with the reference's q rows."""
    G, tail, norm, fp8, parts, ps = case
    p = fused_probe(G, tail, norm, fp8)
    B, Hq = p.q_ref.shape[0], p.q_ref.shape[1]
    kg, vg = p.kc0.to(DEV), p.vc0.to(DEV)
    tailg = p.v_tail.to(DEV) if tail else None
    tslot = torch.arange(B, dtype=torch.int32, device=DEV) if tail else None
    out = torch.empty(B, Hq, D, dtype=torch.bfloat16, device=DEV)
    ws = ops.decode_workspace(B, HKV, G, parts, DEV)
    ops.paged_attention_decode_fused(out, p.q.to(DEV), kg, vg, p.bt.to(DEV), p.sl.to(DEV),
                                     p.pos.to(DEV), p.slots.to(DEV), p.cs.to(DEV),
                                     None if p.qw is None else p.qw.to(DEV),
                                     None if p.kw is None else p.kw.to(DEV), G, SCALE, EPS,
                                     workspace=ws, num_parts=parts, part_size=ps,
                                     v_tail=tailg, tail_slot=tslot)
    p.check(out, "decode_fused")
    check_fused_writes(p, kg, vg, tailg)
    if tail:   # the plain kernel on what the step left: partial groups come from the tail
        out2 = torch.empty_like(out)
        ops.paged_attention_decode(out2, p.q_ref.to(DEV), kg, vg, p.bt.to(DEV), p.sl.to(DEV), G,
                                   SCALE, workspace=ws, num_parts=parts, part_size=ps,
                                   v_tail=tailg, tail_slot=tslot)
        p.check(out2, "decode_plain_tail")
    RAN["decode_fused"] += 1


# ------------------------------------------------------------------------------- prefill needles
PREFILL_SEQS = [(1, 1), (37, 37), (129, 64), (300, 300), (520, 7), (64, 1)]
# (G, fp8, qprep, tile_rows, reversed tile map)
PREFILL_CASES = (
    [(2, False, False, tr, rev) for tr in (128, 256) for rev in (False, True)] +
    [(2, True, False, 128, rev) for rev in (False, True)] +
    [(8, False, False, 128, False), (8, False, False, 256, True), (1, False, False, 256, False),
     (2, False, True, 128, False), (2, False, True, 256, True)])
FORBIDDEN = 4   # the kind (of 5) whose key is limit + 1


@functools.lru_cache(maxsize=None)
def prefill_probe(G, fp8, qprep):
    """Targets cycle per (token, head) through the diagonal, limit - 1, 0, a random key
    <= limit and the forbidden limit + 1 (a later token's key, or the poisoned slot at kv_len:
    the block table has one unused column, so the slot exists for every sequence).  qprep: the
    raw-QKV form, q rotated back by the token's position, q norm weight 4."""
    Hq = HKV * G
    kc, vc, bt, sl, qs, _ = _caches(PREFILL_SEQS, Hq, _seed(15, G), fp8)
    g = torch.Generator().manual_seed(_seed(16, G, fp8))
    T = int(qs[-1])
    targets = torch.zeros(T, Hq, dtype=torch.int64)
    kind = torch.zeros(T, Hq, dtype=torch.int64)
    q = torch.empty(T, Hq, D).bfloat16()
    expect = torch.empty(T, Hq, D).bfloat16()
    for s, (kv, ql) in enumerate(PREFILL_SEQS):
        K, V = _tokens(kc, vc, bt[s])
        a = int(qs[s])
        lim = (kv - ql + torch.arange(ql))[:, None].expand(ql, Hq)
        kd = ((a + torch.arange(ql))[:, None] * Hq + torch.arange(Hq)[None]) % 5
        rnd = (torch.rand(ql, Hq, generator=g) * (lim + 1)).long().clamp(max=lim)
        t = torch.where(kd == 0, lim, torch.where(kd == 1, (lim - 1).clamp(min=0), torch.where(
            kd == 2, torch.zeros_like(lim), torch.where(kd == 3, rnd, lim + 1))))
        q[a:a + ql] = ref.needle_q(K, t, G, unit=kd == FORBIDDEN)
        expect[a:a + ql] = ref.needle_expect(V, t, G)
        targets[a:a + ql], kind[a:a + ql] = t, kd
    p = Probe(q=q, kc=kc, vc=vc, bt=bt, sl=sl, qs=qs, expect=expect, needle=kind != FORBIDDEN,
              targets=targets, kind=kind, G=G, tol=TOL_FP8_PREFILL if fp8 else TOL_BF16)
    if qprep:
        p.pos = torch.cat([torch.arange(kv - ql, kv) for kv, ql in PREFILL_SEQS]).to(torch.int64)
        p.cs = ref.rope_cos_sin(1024, D, 1e6)
        p.qw = torch.full((D,), 4.0).bfloat16()
        qkv = (torch.randn(T, (Hq + 2 * HKV) * D, generator=g) * 2.0).bfloat16()
        qkv[:, :Hq * D] = ref.unrope(q.float() / ref.NEEDLE_BETA, p.pos, p.cs).to(
            torch.bfloat16).reshape(T, -1)
        p.qkv = qkv
        p.q_ref = torch.empty(T, Hq, D).bfloat16()
        ref.qk_norm_rope_cache(qkv, p.q_ref, kc.clone(), vc.clone(), p.pos,
                               torch.full((T,), -1, dtype=torch.int64), p.cs, p.qw, None, Hq,
                               HKV, EPS)
    return p


def _run_prefill(p, seqs, tile_rows, rev, qprep=False):
    ts, tr = _tiles(seqs, p.G, tile_rows)
    if rev:
        ts, tr = ts.flip(0).contiguous(), tr.flip(0).contiguous()
    out = torch.empty(p.q.shape, dtype=torch.bfloat16, device=DEV)
    args = (p.kc.to(DEV), p.vc.to(DEV), p.bt.to(DEV), p.sl.to(DEV), p.qs.to(DEV), ts.to(DEV),
            tr.to(DEV), p.G, SCALE)
    if qprep:
        ops.paged_attention_prefill(out, torch.empty_like(out), *args, tile_rows=tile_rows,
                                    qprep=(p.qkv.to(DEV), p.pos.to(DEV), p.cs.to(DEV),
                                           p.qw.to(DEV), EPS))
    else:
        ops.paged_attention_prefill(out, p.q.to(DEV), *args, tile_rows=tile_rows)
    return out


def _prefill_id(c):
    G, fp8, qprep, tr, rev = c
    return (f"g{G}-{'fp8' if fp8 else 'bf16'}-{'qprep' if qprep else 'q'}-{tr}-"
            f"{'rev' if rev else 'fwd'}")


@pytest.mark.parametrize("case", PREFILL_CASES, ids=_prefill_id)
def test_prefill_needles(case):
    """Prefill kernels (4-wave, 8-wave, fp8 register-staged, q-prep): needles on the diagonal,
    next to it, at key 0 and at random; forbidden needles on limit + 1; the tile map in
    dispatch order and reversed."""
    G, fp8, qprep, tr, rev = case
    p = prefill_probe(G, fp8, qprep)
    p.check(_run_prefill(p, PREFILL_SEQS, tr, rev, qprep), "prefill_needles")
    RAN["prefill_needles"] += 1


# ------------------------------------------------------------------------------- score patterns
PATTERN_KV = 520
PATTERN_PAIRS = [(520, 520), (520, 130), (520, 7)]
PATTERN_G = 2
PATTERN_PREFILL_CASES = [(ql, fp8, tr) for _, ql in PATTERN_PAIRS
                         for fp8, tr in ((False, 128), (False, 256), (True, 128))]
PATTERN_DECODE_LENS = (900, 1500)
PATTERN_DECODE_PLANS = [(1, 4096), (4, 256), (3, 512)]
PATTERN_DECODE_CASES = [(fp8, parts, ps) for fp8 in (False, True)
                        for parts, ps in PATTERN_DECODE_PLANS]


def _pattern_caches(seqs, tile, fp8, seed):
    """One sequence per score pattern plus one with randn keys (the zero-query sequence), each
    (kv, ql) of `seqs`; stale slots of the last block and the unused table column poisoned.
    -> (kc, vc, bt, sl, qs, q)"""
    Hq = HKV * PATTERN_G
    nb = [(kv + BS - 1) // BS for kv, _ in seqs]
    NB = sum(nb) + 2
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(NB, generator=g)
    kc = torch.zeros(NB, HKV, BS, D).bfloat16()
    vc = torch.zeros(NB, HKV, BS // 8, D, 8).bfloat16()
    if fp8:
        kc, vc = _to_fp8_cache(kc, vc)
    bt = torch.zeros(len(seqs), max(nb) + 1, dtype=torch.int32)
    qs = torch.zeros(len(seqs) + 1, dtype=torch.int32)
    qrows, i = [], 0
    for s, (kv, ql) in enumerate(seqs):
        blocks = perm[i:i + nb[s]]
        i += nb[s]
        bt[s, :nb[s]] = blocks.to(torch.int32)
        qs[s + 1] = qs[s] + ql
        V = torch.randn(nb[s] * BS, HKV, D, generator=g)
        if s < len(ref.SCORE_PATTERNS):
            sc = ref.score_pattern(ref.SCORE_PATTERNS[s], kv, tile)
            K, q = ref.pattern_kq(sc, HKV, ql, Hq, SCALE, seed + 7 * s + 1)
            K = torch.cat([K, torch.zeros(nb[s] * BS - kv, HKV, D)])
        else:
            K = torch.randn(nb[s] * BS, HKV, D, generator=g)
            q = torch.zeros(ql, Hq, D).bfloat16()
        ref.write_tokens(kc, vc, blocks, K, V)
        qrows.append(q)
    sl = torch.tensor([kv for kv, _ in seqs], dtype=torch.int32)
    ref.poison_stale(kc, vc, bt, sl, int(perm[i]), ref.poison_direction(HKV, D, seed + 3))
    assert int(bt.min()) >= 0 and int(bt.max()) < NB
    return kc, vc, bt, sl, qs, torch.cat(qrows)


@functools.lru_cache(maxsize=None)
def pattern_prefill_probe(ql, fp8):
    seqs = [(PATTERN_KV, ql)] * (len(ref.SCORE_PATTERNS) + 1)
    kc, vc, bt, sl, qs, q = _pattern_caches(seqs, 64, fp8, _seed(17, ql))
    T, Hq = q.shape[0], q.shape[1]
    return Probe(q=q, kc=kc, vc=vc, bt=bt, sl=sl, qs=qs, seqs=seqs, expect=torch.zeros_like(q),
                 needle=torch.zeros(T, Hq, dtype=torch.bool), G=PATTERN_G,
                 tol=TOL_FP8_PREFILL if fp8 else TOL_BF16)


@functools.lru_cache(maxsize=None)
def pattern_decode_probe(lens, fp8):
    seqs = [(L, 1) for L in lens for _ in range(len(ref.SCORE_PATTERNS) + 1)]
    # one pattern per sequence, cycling: _pattern_caches takes sequence s's pattern from s
    n = len(ref.SCORE_PATTERNS) + 1
    parts = [_pattern_caches(seqs[i * n:(i + 1) * n], 32, fp8, _seed(18, L))
             for i, L in enumerate(lens)]
    # merge the per-length caches into one (block ids shifted)
    kc = torch.cat([p[0] for p in parts])
    vc = torch.cat([p[1] for p in parts])
    width = max(p[2].shape[1] for p in parts)
    bts, off = [], 0
    for p in parts:
        b = p[2] + off
        pad = b[:, -1:].expand(-1, width - b.shape[1])   # more unused entries: the poison block
        bts.append(torch.cat([b, pad], dim=1))
        off += p[0].shape[0]
    q = torch.cat([p[5] for p in parts])
    B, Hq = q.shape[0], q.shape[1]
    return Probe(q=q, kc=kc, vc=vc, bt=torch.cat(bts).contiguous(),
                 sl=torch.cat([p[3] for p in parts]), qs=torch.arange(B + 1, dtype=torch.int32),
                 expect=torch.zeros_like(q), needle=torch.zeros(B, Hq, dtype=torch.bool),
                 G=PATTERN_G, tol=TOL_FP8_DECODE if fp8 else TOL_BF16)


def pattern_decode_lens(parts, ps):
    return tuple(min(L, parts * ps) for L in PATTERN_DECODE_LENS)


@pytest.mark.parametrize("case", PATTERN_PREFILL_CASES,
                         ids=lambda c: f"q{c[0]}-{'fp8' if c[1] else 'bf16'}-{c[2]}")
def test_prefill_patterns(case):
    """The deferred running max of the prefill loop: rows whose tile maxima rise, fall, step
    either side of the threshold, spike and creep, starting at tile 0, mid-tile and deep in
    the context; plus zero queries (the prefix mean of V)."""
    ql, fp8, tr = case
    p = pattern_prefill_probe(ql, fp8)
    p.check(_run_prefill(p, p.seqs, tr, False), "prefill_patterns")
    RAN["prefill_patterns"] += 1


@pytest.mark.parametrize("case", PATTERN_DECODE_CASES,
                         ids=lambda c: f"{'fp8' if c[0] else 'bf16'}-{c[1]}x{c[2]}")
def test_decode_patterns(case):
    """The same score functions over the decode kernel's 32-key chunks, four waves and split-KV
    combine (peak10 and fall10 hold their maximum in an early partition); zero queries."""
    fp8, parts, ps = case
    p = pattern_decode_probe(pattern_decode_lens(parts, ps), fp8)
    p.check(_run_decode(p, parts, ps), "decode_patterns")
    RAN["decode_patterns"] += 1


# ------------------------------------------------------------------------------- env knobs
FAMILY_CASES = {
    "decode_sweep": ("test_decode_sweep", SWEEP_CASES, _sweep_id),
    "decode_long": ("test_decode_long_context", LONG_PLANS, lambda c: f"{c[0]}-{c[1]}"),
    "decode_fused": ("test_decode_fused", FUSED_CASES, _fused_id),
    "prefill_needles": ("test_prefill_needles", PREFILL_CASES, _prefill_id),
    "prefill_patterns": ("test_prefill_patterns", PATTERN_PREFILL_CASES,
                         lambda c: f"q{c[0]}-{'fp8' if c[1] else 'bf16'}-{c[2]}"),
    "decode_patterns": ("test_decode_patterns", PATTERN_DECODE_CASES,
                        lambda c: f"{'fp8' if c[0] else 'bf16'}-{c[1]}x{c[2]}"),
}

KNOBS = [
    ({}, None),   # the baseline child: the union of the selections below
    ({"AKAP_PREFILL_STAGGER": "1"}, "stagger"),
    ({"AKAP_FA_RESCALE_T": "0"}, "exact_max"),
    ({"AKAP_DECODE_DEFER_KV": "0"}, "prologue_stores"),
]
KNOB_VARS = sorted({k for env, _ in KNOBS for k in env})


def knob_selection(which):
    """(family, case) pairs of the reduced selection of cases 3-5 a knob's child runs."""
    stagger = ([("prefill_needles", c) for c in PREFILL_CASES if c[3] == 256 and not c[1]] +
               [("prefill_patterns", c) for c in PATTERN_PREFILL_CASES if c[2] == 256])
    exact = ([("prefill_patterns", c) for c in PATTERN_PREFILL_CASES] +
             [("prefill_needles", c) for c in PREFILL_CASES if c[0] == 2 and not c[4]])
    stores = [("decode_fused", c) for c in FUSED_CASES if c[1] or c[3]]
    sel = {"stagger": stagger, "exact_max": exact, "prologue_stores": stores}
    if which is None:
        seen, out = set(), []
        for pair in stagger + exact + stores:
            if pair not in seen:
                seen.add(pair)
                out.append(pair)
        return out
    return sel[which]


def knob_nodes(which):
    me = "tests/test_attention_probes_gpu.py"
    nodes = []
    for fam, c in knob_selection(which):
        name, _, idf = FAMILY_CASES[fam]
        nodes.append(f"{me}::{name}[{idf(c)}]")
    return nodes + [f"{me}::test_zz_probe_counts"]


# The unset-environment child (the largest selection) took CHILD_BASELINE_S seconds on an MI355X,
# most of it interpreter and library start-up and the CPU-side input generation; every child
# gets 15 times that (profiles/attention_probe_tests.md).
CHILD_BASELINE_S = 6
CHILD_TIMEOUT_S = 15 * CHILD_BASELINE_S
_child_died = []


@pytest.mark.parametrize("env,which", KNOBS,
                         ids=[",".join(f"{k}={v}" for k, v in e.items()) or "unset" for e, _ in KNOBS])
def test_env_knob(env, which):
    """Kernel variants selected by environment variables read once per process -- the 8-wave
    ping-pong prefill kernel, the exact-max mode of the prefill loop, the fused decode kernel's
    prologue stores -- each run a reduced selection of the fused, prefill-needle and pattern
    cases in a fresh child process, one child at a time; after a child that died (signal,
    abort, timeout) nothing more is started on the GPU."""
    assert not os.environ.get(CHILD_FLAG), "a knob child must not start children"
    if _child_died:
        pytest.fail(f"not run: an earlier child died ({_child_died[0]})")
    sel = knob_selection(which)
    nodes = knob_nodes(which)
    assert len(nodes) > 1
    # the selection must reach the knob's code, else the child tests nothing
    if which == "stagger":     # the ping-pong variant exists for 256-row tiles, bf16 caches
        assert all(c[-2 if f == "prefill_needles" else -1] == 256 and not c[1] for f, c in sel)
        assert {f for f, _ in sel} == {"prefill_needles", "prefill_patterns"}
    if which == "exact_max":   # every prefill kernel form, patterns included
        assert {c[2] for f, c in sel if f == "prefill_patterns"} == {128, 256}
        assert any(c[1] for f, c in sel if f == "prefill_patterns")
    if which == "prologue_stores":   # deferred stores exist on the fused V-tail path only
        assert sum(1 for _, c in sel if c[1]) >= 4 and all(f == "decode_fused" for f, _ in sel)
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
def test_zz_probe_counts(request):
    """Every enumerated case of every family ran to the end: a family that silently skipped,
    or was never collected, fails here.  (A knob child checks the cases it was given.)"""
    by_name = {name: f for f, (name, _, _) in FAMILY_CASES.items()}
    selected = collections.Counter()
    for it in request.session.items:
        f = by_name.get(getattr(it, "originalname", None) or it.name.split("[")[0])
        if f and it.fspath == request.node.fspath:
            selected[f] += 1
    print("[probe] needle ulp observed:", dict(OBSERVED_ULP))
    print("[probe] worst err / limit observed:",
          {k: round(v, 4) for k, v in OBSERVED_RATIO.items()})
    print("[probe] cases ran:", dict(RAN))
    assert sum(selected.values()) > 0
    if not os.environ.get(CHILD_FLAG):
        for f, (_, cases, _) in FAMILY_CASES.items():
            assert len(cases) > 0 and selected[f] == len(cases), (
                f"{f}: {selected[f]} of {len(cases)} enumerated cases were collected")
    for f, n in selected.items():
        assert RAN[f] == n, f"{f}: {RAN[f]} of {n} cases ran to the end"
