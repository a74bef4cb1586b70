"""The CPU side of the attention probes (tests/test_attention_probes_gpu.py).

Everything the GPU tests rely on is proved here, on their own inputs, without a GPU:
  * the reference satisfies every needle row of every case (100 % of rows: a failing seed
    means another beta or seed for the whole case, never a dropped row);
  * the decode sweep targets every key position of every kv head;
  * the score patterns move a deferred running max as often as stated, a from-scratch model of
    the tile loop stays within MODEL_SHARE of the GPU tolerance against an fp64 softmax, and
    the same model without the rescale of o exceeds the tolerance on every rising pattern;
  * the poison is finite, in range and never visible to the reference;
  * five reference-level mutations each fail the cases' own assertions, so the GPU tests can
    fail.
"""
import math

import pytest
import torch

import test_attention_probes_gpu as P
from aws_k8s_ansible_provisioner_amd.ops import reference as ref

LOG2E = math.log2(math.e)


# ------------------------------------------------------------------------------- helpers
def test_write_tokens_inverts_gather_kv():
    g = torch.Generator().manual_seed(1)
    for fp8 in (False, True):
        kc = torch.zeros(7, 8, 64, 128).bfloat16()
        vc = torch.zeros(7, 8, 8, 128, 8).bfloat16()
        if fp8:
            kc, vc = P._to_fp8_cache(kc, vc)
        blocks = torch.tensor([5, 0, 3])
        K = torch.randn(192, 8, 128, generator=g)
        V = torch.randn(192, 8, 128, generator=g)
        ref.write_tokens(kc, vc, blocks, K, V)
        Kg, Vg = ref.gather_kv(kc, vc, blocks.to(torch.int32), 192)
        assert torch.equal(Kg, ref.from_cache(ref.to_cache(K, kc)))
        assert torch.equal(Vg, ref.from_cache(ref.to_cache(V, vc)))
        k2, v2 = torch.zeros_like(kc), torch.zeros_like(vc)   # against the per-token writer
        slots = torch.cat([torch.arange(64) + 64 * int(b) for b in blocks])
        ref.write_cache(K.bfloat16(), V.bfloat16(), k2, v2, slots)
        if not fp8:
            assert torch.equal(k2, kc) and torch.equal(v2, vc)


def test_unrope_inverts_apply_rope():
    cs = ref.rope_cos_sin(4096, 128, 1e6)
    x = torch.randn(5, 3, 128)
    pos = torch.tensor([0, 1, 777, 4095, 31])
    back = ref.unrope(ref.apply_rope(x, pos, cs), pos, cs)
    assert float((back - x).abs().max()) < 1e-5


# ------------------------------------------------------------------------------- needle rows
NEEDLE_PROBES = (
    [("sweep", P.sweep_probe, k) for k in sorted({c[:2] for c in P.SWEEP_CASES})] +
    [("long", P.long_probe, ())] +
    [("fused", P.fused_probe, f) for f in P.FUSED_FORMS] +
    [("prefill", P.prefill_probe, k) for k in sorted({c[:3] for c in P.PREFILL_CASES})])


@pytest.mark.parametrize("name,build,key", NEEDLE_PROBES,
                         ids=[f"{n}-{'-'.join(str(int(v)) for v in k)}" for n, _, k in NEEDLE_PROBES])
def test_reference_satisfies_every_needle_row(name, build, key):
    """ops.reference.paged_attention (after ops.reference.qk_norm_rope_cache for the raw-QKV
    forms) returns V[target] within the needle tolerance for every needle row, and the case's
    whole assertion passes on the reference's output."""
    p = build(*key)
    out = p.ref_all()
    assert int(p.needle.sum()) > 0
    bad, ulp = ref.needle_mismatch(out[p.needle], p.expect[p.needle])
    assert not bool(bad.any()), f"{int(bad.any(-1).sum())} of {int(p.needle.sum())} rows"
    p.check(out)
    # the poison contract: finite, every block id in range
    assert bool(torch.isfinite(ref.from_cache(p.kc).float()).all())
    assert bool(torch.isfinite(ref.from_cache(p.vc).float()).all())
    assert 0 <= int(p.bt.min()) and int(p.bt.max()) < p.kc.shape[0]


@pytest.mark.parametrize("G,fp8", sorted({c[:2] for c in P.SWEEP_CASES}))
def test_sweep_targets_every_position_of_every_kv_head(G, fp8):
    p = P.sweep_probe(G, fp8)
    first = 0
    groups = [(0, L) for L in (P.SWEEP_LEN,) + P.SWEEP_SHORT] + \
             [(s + 1, L) for s, L in enumerate(P.SWEEP_SHORT)]
    for s, L in groups:
        n = (L + G - 1) // G
        t = p.targets[first:first + n]
        assert bool((p.sl[first:first + n] == L).all()) and bool(
            (p.blocks_of[first:first + n] == s).all())
        for hk in range(P.HKV):
            seen = set(t[:, hk * G:(hk + 1) * G].reshape(-1).tolist())
            assert seen == set(range(L)), (s, L, hk)
        first += n
    assert first == p.q.shape[0]


def test_long_probe_targets_every_partition_edge():
    p = P.long_probe()
    pos = set(P.long_positions())
    for parts, ps in P.LONG_PLANS:
        for e in range(ps, P.LONG_LEN, ps):
            assert {e - 1, e, e + 1} <= pos
    for hk in range(P.HKV):
        seen = set(p.targets[:-2, hk * P.LONG_G:(hk + 1) * P.LONG_G].reshape(-1).tolist())
        assert seen == pos
    assert p.targets[-2].tolist() == [P.LONG_LEN] * (P.HKV * P.LONG_G)
    assert not bool(p.needle[-2:].any())


def test_fused_targets_cycle_through_every_kind():
    p = P.fused_probe(2, True, True, False)
    for s, L in enumerate(P.FUSED_LENS):
        gs = (L - 1) & ~7
        want = {L - 1, max(L - 2, 0), gs, max(gs - 1, 0), 0}
        assert want <= set(p.targets[s].tolist()), (L, p.targets[s].tolist())
    assert int(p.slots[-1]) == -1 and int((p.slots < 0).sum()) == 1


# ------------------------------------------------------------------------------- patterns
# moves of the running max after the first tile, 520 keys, 64-key tiles, threshold 8:
#   rise6    tile maxima 5.9 + 6 t: every second tile -> tiles 2, 4, 6
#   rise10   9.8 + 10 t: tiles 1..7 (tile 8 holds 8 keys: +1.3)
#   step7.9  tiles 2, 4, 6, 8;   step8.1  tiles 1..8;   fall10  none
#   saw12    0 12 24 0 12 24 ...: tiles 1, 2
#   spikes   the tiles of the two spikes
#   creep2   0 7.5 9.5 ... 21.5: tile 2 (9.5), then tile 7 (19.5 > 17.5); tile 6 (17.5) equals
#            9.5 + 8 exactly, so the bf16 noise of real inputs may move it there too: 2 or 3
#   peak10   0 10 20 30 20 ...: tiles 1, 2, 3
CROSSINGS = {"rise6": 3, "rise10": 7, "step7.9": 4, "step8.1": 8, "fall10": 0, "saw12": 2,
             "spikes": 2, "creep2": 2, "peak10": 3}
RISING = ("rise6", "rise10", "step7.9", "step8.1", "creep2")
LIMITS = (0, 63, 64, 127, 128, 200, 255, 300, 519)
MODEL_SHARE = 0.2   # of 2e-2 + 2e-2 |ref|


def _softmax64(s2, V, limit):
    s = s2[:limit + 1].double()
    p = torch.exp2(s - s.max())
    return (p / p.sum()) @ V[:limit + 1].double()


@pytest.mark.parametrize("name", ref.SCORE_PATTERNS)
def test_pattern_crossings_and_tile_model(name):
    s2 = ref.score_pattern(name, 520, 64)
    g = torch.Generator().manual_seed(5)
    V = torch.randn(520, 128, generator=g).bfloat16().float()
    worst = 0.0
    for lim in LIMITS:
        o, moves = ref.fa_tile_model(s2, V, lim)
        want = _softmax64(s2, V, lim)
        worst = max(worst, float(((o - want).abs() / (2e-2 + 2e-2 * want.abs())).max()))
        o0, _ = ref.fa_tile_model(s2, V, lim, T=0.0)   # the exact-max mode
        worst = max(worst, float(((o0 - want).abs() / (2e-2 + 2e-2 * want.abs())).max()))
        if lim == 519:
            assert moves == CROSSINGS[name], (name, moves)
    print(f"[model] {name}: worst err / limit {worst:.4f}")
    assert worst <= MODEL_SHARE, (name, worst)
    if name in RISING:
        o, _ = ref.fa_tile_model(s2, V, 519, rescale_o=False)
        want = _softmax64(s2, V, 519)
        over = float(((o - want).abs() / (2e-2 + 2e-2 * want.abs())).max())
        print(f"[model] {name}: without the o rescale {over:.3g} x the limit")
        assert over > 1.0, (name, over)


@pytest.mark.parametrize("ql", [ql for _, ql in P.PATTERN_PAIRS])
def test_pattern_inputs_cross_as_stated(ql):
    """The bf16 inputs of the GPU pattern cases themselves: the last row of each pattern's
    sequence (limit 519), every head, moves the model's running max the stated number of
    times (creep2: its tie may fall either way)."""
    p = P.pattern_prefill_probe(ql, False)
    for s, name in enumerate(ref.SCORE_PATTERNS):
        K, V = ref.gather_kv(p.kc, p.vc, p.bt[s], P.PATTERN_KV)
        row = int(p.qs[s + 1]) - 1
        for h in range(0, P.HKV * P.PATTERN_G, 5):
            s2 = (p.q[row, h].double() @ K[:, h // P.PATTERN_G].double().t()) * P.SCALE * LOG2E
            want = ref.score_pattern(name, P.PATTERN_KV, 64)
            assert float((s2 - want).abs().max()) < (0.08 if name != "spikes" else 4.0), name
            _, moves = ref.fa_tile_model(s2, V[:, h // P.PATTERN_G], P.PATTERN_KV - 1)
            ok = (CROSSINGS[name], CROSSINGS[name] + 1) if name == "creep2" else (CROSSINGS[name],)
            assert moves in ok, (name, h, moves)


def test_decode_patterns_hold_their_maximum_in_an_early_partition():
    for name in ("peak10", "fall10"):
        for L in P.PATTERN_DECODE_LENS:
            s2 = ref.score_pattern(name, L, 32)
            for parts, ps in P.PATTERN_DECODE_PLANS[1:]:
                n = min(L, parts * ps)
                last = (n - 1) // ps
                assert int(s2[:n].argmax()) // ps < last, (name, L, parts, ps)


# ------------------------------------------------------------------------------- mutations
def _sub(p, rows):
    """The decode probe restricted to some batch rows (one token each)."""
    rows = torch.as_tensor(rows)
    return P.Probe(q=p.q[rows], kc=p.kc, vc=p.vc, bt=p.bt[rows].clone(), sl=p.sl[rows].clone(),
                   qs=torch.arange(rows.numel() + 1, dtype=torch.int32), expect=p.expect[rows],
                   needle=p.needle[rows], G=p.G, tol=p.tol)


def _sweep_own_rows():
    p = P.sweep_probe(2, False)
    return _sub(p, (p.blocks_of > 0).nonzero().flatten())


MUTATION_PROBES = {
    "sweep": _sweep_own_rows,
    "sweep_fp8": lambda: _sub(P.sweep_probe(2, True),
                              (P.sweep_probe(2, True).blocks_of > 0).nonzero().flatten()),
    "fused": lambda: P.fused_probe(2, True, True, False),
    "prefill": lambda: P.prefill_probe(2, False, False),
    "prefill_fp8": lambda: P.prefill_probe(2, True, False),
    "prefill_patterns": lambda: P.pattern_prefill_probe(130, False),
    "decode_patterns": lambda: P.pattern_decode_probe(P.PATTERN_DECODE_LENS, False),
}
MUTATIONS = ("drop_key", "limit+1", "limit-1", "bt_entry", "roll_v_group", "poison_block")
# needles ignore an extra visible key unless it is theirs: limit + 1 is what the forbidden
# needles (prefill) and the rising patterns are for
APPLIES = {
    "drop_key": ("sweep", "sweep_fp8", "fused", "decode_patterns"),
    "limit+1": ("prefill", "prefill_fp8", "prefill_patterns"),
    "limit-1": ("prefill", "prefill_fp8", "prefill_patterns"),
    "bt_entry": tuple(MUTATION_PROBES),
    "roll_v_group": tuple(MUTATION_PROBES),
    "poison_block": tuple(MUTATION_PROBES),
}


def _mutated_reference(p, mutation):
    q = p.q if p.q_ref is None else p.q_ref
    kc, vc, bt, sl = p.kc, p.vc, p.bt.clone(), p.sl.clone()
    if mutation in ("drop_key", "limit-1"):   # the newest key is gone: every limit moves down
        sl = torch.where(sl > 1, sl - 1, sl)
    elif mutation == "limit+1":
        sl = sl + 1
    elif mutation == "bt_entry":              # each row's newest block from another sequence
        last = [(int(sl[s]) - 1) // P.BS for s in range(sl.numel())]
        mine = [int(bt[s, last[s]]) for s in range(sl.numel())]
        for s in range(sl.numel()):
            bt[s, last[s]] = next(b for b in mine if b != mine[s])
    elif mutation == "poison_block":          # the last column is unused: the poison block
        for s in range(sl.numel()):
            bt[s, (int(sl[s]) - 1) // P.BS] = bt[s, -1]
    elif mutation == "roll_v_group":          # the tokens of each sequence's last group, rolled
        vc = vc.clone()
        for s in range(sl.numel()):
            pos = int(sl[s]) - 1
            b = int(bt[s, pos // P.BS])
            vc[b, :, (pos % P.BS) // 8] = vc[b, :, (pos % P.BS) // 8].roll(1, dims=-1)
    return ref.paged_attention(q, kc, vc, bt, sl, p.qs, P.SCALE)


@pytest.mark.parametrize("mutation,name",
                         [(m, n) for m in MUTATIONS for n in APPLIES[m]])
def test_mutated_reference_fails_the_case(mutation, name):
    p = MUTATION_PROBES[name]()
    p.check(p.ref_all())
    with pytest.raises(AssertionError):
        p.check(_mutated_reference(p, mutation))


# ------------------------------------------------------------------------------- knob selections
def test_knob_selections_name_enumerated_cases():
    for _, which in P.KNOBS:
        sel = P.knob_selection(which)
        assert sel and all(c in P.FAMILY_CASES[f][1] for f, c in sel)
        nodes = P.knob_nodes(which)
        assert len(set(nodes)) == len(nodes) == len(sel) + 1
    base = set(P.knob_selection(None))
    for _, which in P.KNOBS[1:]:
        assert set(P.knob_selection(which)) <= base
