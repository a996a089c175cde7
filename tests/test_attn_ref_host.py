"""The float64 attention restatement and its per-element bound (tests/attn_ref.py), checked on the CPU: no GPU, no GPU library.

`simulate` is a float64 softmax with exactly the roundings the 16-bit kernels make (P to 16 bits, the row sum from the unrounded p,
one output rounding; the scores are measured against the standing max of the first tile where the true max is within 2^16 / 2^15 of
it, as the lazy running max of attention_bf16.hip leaves them, so P is not 1.0 at the row's best key). It pins the bound from BOTH
sides: the simulation stays under it on every input family of tests/test_gpu_attention.py, and every defect below — a dropped tile, a
dropped or leaked key, the wrong kv head, the lost cls key, a split that starts one row late — put into the simulation exceeds it.
Measured when written (printed by the tests, none is a limit): the clean simulation reaches 0.26 .. 0.88 of the bound in bfloat16 and
0.17 .. 0.69 in float16 (and 1.1 .. 1.3 x 3 * 2^-9 A, which is therefore no bound: bfloat16 rounds with up to 2^-8); the Gaussian defects
at S = 3700 give 4.9 .. 10.3 x the bound, a leaked key 2.8e3 / 1.1e4 x, the defects on addressed inputs 1.2e2 .. 3e5 x."""
import pytest
import torch

from attn_ref import (adversarial_pad, attention_bound, attention_ref, causal_targets, decode_targets, key_weight, make_inputs,
                      score_chunks, score_scale, visible, vit_targets, worst)

HALF = [torch.bfloat16, torch.float16]


def simulate(Q, K, V, causal, dt, kv_lo=None, kv_len=None, rule=visible, chunk=None, first_tile=None):
    """the kernel's arithmetic in f64 with its roundings; ``rule`` = the visibility rule (a defect goes here). ``first_tile``: index
    [B] of the 64-key tile whose max the lazy path keeps (default: kv_lo's tile)."""
    B, Hq, n, hd = Q.shape
    Hkv = K.shape[1]
    kv_len = K.shape[2] if kv_len is None else kv_len
    Vd = V[:, :, :kv_len].double()
    lazy = {torch.bfloat16: 16.0, torch.float16: 15.0, torch.float32: 0.0}[dt]
    lo = torch.zeros(B, dtype=torch.long) if kv_lo is None else torch.as_tensor(kv_lo).clamp(0, kv_len - 1)
    t0 = (lo // 64 if first_tile is None else torch.as_tensor(first_tile)).tolist()
    out = torch.empty(B, Hq, n, hd, dtype=torch.float64)
    for r0, r1, s in score_chunks(Q, K, causal, kv_lo, kv_len, chunk, rule):
        m = s.amax(-1, keepdim=True)
        m0 = torch.stack([s[b, ..., 64 * t0[b]:64 * t0[b] + 64].amax(-1, keepdim=True) for b in range(B)])
        base = torch.where((m - m0 < lazy) & torch.isfinite(m0), m0, m)
        e = torch.exp2(s - base).float()                                        # f32 p
        l = e.double().sum(-1, keepdim=True)                                    # the row sum of the unrounded p
        p16 = e.to(dt).double()                                                 # P as the PV MFMA reads it
        o = (p16.view(B, Hkv, -1, kv_len) @ Vd).view(B, Hq, r1 - r0, hd) / l.view(B, Hq, r1 - r0, 1)
        out[:, :, r0:r1] = o.float().to(dt).double()                            # one output rounding
    return out


def ratio(out, Q, K, V, causal, dt, kv_lo=None, kv_len=None, rows_from=None, refA=None):
    """worst |out - ref| / bound over the rows that are compared (sequence b: rows >= rows_from[b])"""
    ref, A = refA if refA is not None else attention_ref(Q, K, V, causal, kv_lo, kv_len)
    n_keys = K.shape[2] if kv_len is None else kv_len
    bound = attention_bound(A, ref, dt, n_keys, score_scale(Q, K, kv_len))
    if rows_from is not None:
        for b, r in enumerate(rows_from):
            out = out.clone()
            out[b, :, :r] = ref[b, :, :r]
    return worst(out, ref, bound)


def causal_case(family, S, hd, dt, kv_lo, B=None, Hq=8, Hkv=2, seed=3):
    B = len(kv_lo) if kv_lo is not None else 1
    lo = kv_lo if kv_lo is not None else [0] * B
    rows = (S + 64) // 64 * 64
    peak = {"addressed12": 12.0, "addressed24": 24.0, "future": 12.0}.get(family)
    if family == "gauss":
        target = None
    elif family == "future":
        i = torch.arange(S)
        target = torch.stack([torch.where((i % 2 == 1) & (i >= l) & (l > 0), l - 1, i + 1) for l in lo])[:, None].expand(B, Hq, S)
    else:
        target = causal_targets(S, Hq, lo)
    Q, K, V = make_inputs("gauss" if family == "gauss" else "addressed", B, Hq, Hkv, S, rows, hd, dt, seed, target, peak)
    if family != "future":
        adversarial_pad(Q, K, V, S)
    V[:, :, S:] = 1e4
    return Q, K, V, target


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("family", ["gauss", "addressed12", "addressed24", "future"])
def test_simulated_kernel_stays_under_the_bound_causal(family, hd, dt):
    """1300 rows, a left pad of three q-blocks that ends inside a tile, four query heads per kv head"""
    S, lo = 1300, [0, 400]
    Q, K, V, target = causal_case(family, S, hd, dt, lo)
    out = simulate(Q, K, V, True, dt, lo, S, chunk=512)
    r, idx, err, bnd = ratio(out, Q, K, V, True, dt, lo, S, rows_from=lo)
    print(f"causal {family} hd {hd} {dt}: worst err / bound {r:.3f} at (b, head, row, d) = {idx}: {err:.3e} vs {bnd:.3e}")
    assert r <= 1.0
    if family.startswith("addressed"):
        w = key_weight(Q, K, target, True, lo, S)
        for b, l in enumerate(lo):
            assert float(w[b, :, l:].min()) >= 0.3, float(w[b, :, l:].min())
    if family == "future":       # the hidden key is the row's best key: it would take most of the weight if it leaked
        w = key_weight(Q[:1], K[:1], target[:1].clamp(max=S - 1), True, None, S)
        assert float(w[:, :, :S - 1].max()) == 0.0                              # ... and is hidden (row S - 1 aims at a pad row)
        s = next(score_chunks(Q[:1], K[:1], False, None, S + 1))[2].view(1, Q.shape[1], S, S + 1)
        assert bool((s.argmax(-1) == target[:1]).all())


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("hd", [64, 96])
@pytest.mark.parametrize("family", ["gauss", "addressed12", "addressed24"])
def test_simulated_kernel_stays_under_the_bound_vit(family, hd, dt):
    """the ViT's 1025 keys (16 tiles and the cls key), non-causal; the sweep covers every (q-block, kv tile) pair of a full q-block"""
    T, H, N = 2, 4, 1025
    target = vit_targets(N, H)[None].expand(T, H, N)
    peak = 24.0 if family.endswith("24") else 12.0
    Q, K, V = make_inputs(family.rstrip("124"), T, H, H, N, 1088, hd, dt, 5, target, peak)
    adversarial_pad(Q, K, V, N)
    out = simulate(Q, K, V, False, dt, None, N, first_tile=[0] * T)
    r, idx, err, bnd = ratio(out, Q, K, V, False, dt, None, N)
    print(f"vit {family} hd {hd} {dt}: worst err / bound {r:.3f} at {idx}")
    assert r <= 1.0
    if family != "gauss":
        assert float(key_weight(Q, K, target, False, None, N).min()) >= 0.3
        # cls key dropped (kv_prefix started from l0 = 0): the rows aimed at key 0 lose most of their weight
        nocls = lambda qi, kj, lo, n, coff, c: visible(qi, kj, lo, n, coff, c) & (kj != 0)
        r = ratio(simulate(Q, K, V, False, dt, None, N, rule=nocls, first_tile=[0] * T), Q, K, V, False, dt, None, N)[0]
        print(f"    cls key lost: {r:.1f} x the bound")
        assert r > 10.0


def test_vit_sweep_covers_every_q_block_kv_tile_pair():
    N, H = 1025, 16
    t = vit_targets(N, H)
    assert int(t.min()) == 0 and int(t.max()) == N - 1
    ntiles = (N + 63) // 64
    for h in range(H):
        pairs = {(r // 128, int(t[h, r]) // 64) for r in range(N)}
        for qb in range(N // 128):                          # the full q-blocks (the last one holds row 1024 alone)
            assert all((qb, kt) in pairs for kt in range(ntiles)), (h, qb)
        keys = set(t[h].tolist())
        assert {0, N - 1} <= keys and all(64 * k in keys and 64 * k - 1 in keys for k in range(1, 17))


def test_causal_targets_cycle_and_stay_visible():
    lo = [0, 1500]
    t = causal_targets(4718, 32, lo)
    i = torch.arange(4718)
    for b, l in enumerate(lo):
        assert bool((t[b] >= l).all()) and bool((t[b] <= torch.clamp(i, min=l)[None]).all())
    # every kind of target occurs in every head, at rows where it is not clamped
    for h in (0, 5, 31):
        row = 8 * 300 + (8 - h % 8) % 8                     # mode 0 at this row, then 1, 2, ...
        got = [int(t[0, h, row + k]) for k in range(8)]
        r = [row + k for k in range(8)]
        assert got == [r[0], r[1] - 1, 0, r[3] // 64 * 64 - 1, r[4] // 64 * 64, r[5] - 64, r[6] - 127, r[7] - 128]
    assert decode_targets(4718, 0, 8) == [0, 4717, 0, 639, 640, 1279, 1280, 1919, 1920, 2559, 2560, 3199, 3200, 3839, 3840, 4479,
                                          4480, 4717]
    assert decode_targets(4737, 1500, 8)[:6] == [1500, 4736, 1500, 1919, 1920, 2367]


# ---- the defects -------------------------------------------------------------------------------------------------------------------
def _with(extra):
    """the visibility rule with ``extra(qi, kj, coff)`` keys removed"""
    return lambda qi, kj, lo, n, coff, c: visible(qi, kj, lo, n, coff, c) & ~extra(qi, kj, coff)


@pytest.mark.parametrize("hd", [64, 128])
def test_gaussian_defects_in_late_rows_exceed_the_bound(hd):
    """The four defects the max-norm criterion of tests/test_gpu_ops.py lets through at S = 3700 (Gaussian inputs: 0.1 .. 0.4 of its
    tolerance), and the mutations of a causal kernel, against the per-element bound, in bfloat16."""
    S, dt = 3700, torch.bfloat16
    Q, K, V, _ = causal_case("gauss", S, hd, dt, None, Hq=4, Hkv=1, seed=11)
    refA = attention_ref(Q, K, V, True, None, S, chunk=1024)
    clean = ratio(simulate(Q, K, V, True, dt, None, S, chunk=1024), Q, K, V, True, dt, None, S, refA=refA)[0]
    print(f"hd {hd}: clean {clean:.3f}")
    assert clean <= 1.0
    last = (S - 1) // 128 * 128
    last_tile = (S - 1) // 64
    defects = {
        "last q-block skips kv tile 16": lambda qi, kj, coff: (qi >= last) & (kj // 64 == 16),
        "rows >= 2048 miss key 0": lambda qi, kj, coff: (qi >= 2048) & (kj == 0),
        "rows >= 2048 miss the diagonal key": lambda qi, kj, coff: (qi >= 2048) & (kj == qi + coff),
        "rows >= 2048 miss key i - 1": lambda qi, kj, coff: (qi >= 2048) & (kj == qi + coff - 1),
        "kv_end one tile short for the last q-block": lambda qi, kj, coff: (qi >= last) & (kj // 64 == last_tile),
    }
    for name, extra in defects.items():
        r = ratio(simulate(Q, K, V, True, dt, None, S, rule=_with(extra), chunk=1024), Q, K, V, True, dt, None, S, refA=refA)[0]
        print(f"    {name}: {r:.2f} x the bound")
        assert r > 1.0, name
    leak = lambda qi, kj, lo, n, coff, c: visible(qi, kj, lo, n, coff + 1, c)
    r = ratio(simulate(Q, K, V, True, dt, None, S, rule=leak, chunk=1024), Q, K, V, True, dt, None, S, refA=refA)[0]
    print(f"    causal limit kv <= q + coff + 1: {r:.2f} x the bound")
    assert r > 1.0


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("hd", [64, 128])
def test_edge_defects_on_addressed_inputs_exceed_the_bound_by_far(hd, dt):
    S, lo = 1300, [0, 400]
    Q, K, V, _ = causal_case("addressed12", S, hd, dt, lo)
    refA = attention_ref(Q, K, V, True, lo, S)
    last = (S - 1) // 128 * 128
    defects = {
        "miss the diagonal key": lambda qi, kj, coff: (kj == qi + coff) & (qi > 400),       # (rows 0 and 400 see no other key)
        "miss key i - 1": lambda qi, kj, coff: kj == qi + coff - 1,
        "miss the first key of a tile": lambda qi, kj, coff: (kj % 64 == 0) & (kj < qi),
        "miss the last key of a tile": lambda qi, kj, coff: (kj % 64 == 63) & (kj < qi),
        "miss key i - 128": lambda qi, kj, coff: kj == qi + coff - 128,
        "kv_end one tile short for the last q-block": lambda qi, kj, coff: (qi >= last) & (kj // 64 == (S - 1) // 64),
    }
    for name, extra in defects.items():
        r = ratio(simulate(Q, K, V, True, dt, lo, S, rule=_with(extra)), Q, K, V, True, dt, lo, S, rows_from=lo, refA=refA)[0]
        print(f"hd {hd} {dt} {name}: {r:.0f} x the bound")
        assert r > 50.0, name
    # the first live key of the padded sequence dropped / the key in front of it let in
    nofirst = lambda qi, kj, lo_, n, coff, c: visible(qi, kj, lo_, n, coff, c) & (kj != lo_)
    r = ratio(simulate(Q, K, V, True, dt, lo, S, rule=nofirst), Q, K, V, True, dt, lo, S, rows_from=[1, 401], refA=refA)[0]
    assert r > 50.0
    Q, K, V, _ = causal_case("future", S, hd, dt, lo)
    refA = attention_ref(Q, K, V, True, lo, S)
    leak = lambda qi, kj, lo_, n, coff, c: visible(qi, kj, lo_, n, coff + 1, c)
    r = ratio(simulate(Q, K, V, True, dt, lo, S, rule=leak), Q, K, V, True, dt, lo, S, rows_from=lo, refA=refA)[0]
    print(f"hd {hd} {dt} future, causal limit + 1: {r:.0f} x the bound")
    assert r > 50.0
    early = lambda qi, kj, lo_, n, coff, c: visible(qi, kj, (lo_ - 1).clamp(min=0), n, coff, c)
    r = ratio(simulate(Q, K, V, True, dt, lo, S, rule=early), Q, K, V, True, dt, lo, S, rows_from=lo, refA=refA)[0]
    print(f"hd {hd} {dt} future, key kv_lo - 1 visible: {r:.0f} x the bound")
    assert r > 50.0
    # kvh = head % Hkv instead of head // (Hq // Hkv): V (and K) of the wrong kv head
    Hq, Hkv = Q.shape[1], K.shape[1]
    wrong = [h % Hkv for h in range(Hq)]
    for fam in ("gauss", "addressed12"):
        Q, K, V, _ = causal_case(fam, S, hd, dt, lo)
        r = ratio(simulate(Q, K[:, wrong], V[:, wrong], True, dt, lo, S), Q, K, V, True, dt, lo, S, rows_from=lo)[0]
        print(f"hd {hd} {dt} {fam}, kvh = head % Hkv: {r:.0f} x the bound")
        assert r > 50.0


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("kv_len,kv_lo", [(4718, 0), (4737, 1500)])
def test_decode_split_that_starts_one_row_late(kv_len, kv_lo, dt):
    """one query per (sequence, head), each aimed at another key of decode_targets; a split whose range starts one key late"""
    hd, Hq, Hkv, nsplit = 64, 32, 8, 8
    tg = decode_targets(kv_len, kv_lo, nsplit)
    target = torch.tensor([tg[h % len(tg)] for h in range(Hq)])[None, :, None]
    gen = torch.Generator().manual_seed(9)
    K = torch.nn.functional.normalize(torch.randn(1, Hkv, kv_len, hd, generator=gen), dim=-1)
    V = torch.randn(1, Hkv, kv_len, hd, generator=gen).to(dt)
    Q = (12.0 * K.repeat_interleave(Hq // Hkv, 1).gather(2, target[..., None].expand(1, Hq, 1, hd))).to(dt)
    K = K.to(dt)
    lo = [kv_lo]
    assert float(key_weight(Q, K, target, False, lo, kv_len).min()) >= 0.3
    tile = [kv_lo // 64]
    r = ratio(simulate(Q, K, V, False, dt, lo, kv_len, first_tile=tile), Q, K, V, False, dt, lo, kv_len)[0]
    print(f"decode kv_len {kv_len} kv_lo {kv_lo} {dt}: clean {r:.3f}")
    assert r <= 1.0
    for s in range(1, nsplit):
        first = tg[2 + 2 * s]
        late = _with(lambda qi, kj, coff: kj == first)
        r = ratio(simulate(Q, K, V, False, dt, lo, kv_len, rule=late, first_tile=tile), Q, K, V, False, dt, lo, kv_len)[0]
        assert r > 50.0, (s, r)
