"""GPU (-m gpu): the attention kernels at the models' head geometry — Hq = 32, Hkv = 8 (four query heads per kv head), head_dim 64
(GAR-1B) and 128 (GAR-8B), prompts of 4718 / 4296 / 5660 rows (37 q-blocks of 128 rows, 74 kv tiles of 64 per head), the ViT's 16
heads x 17 tiles x 1025 tokens, a decode step over a cache of that length — against the float64 restatement of tests/attn_ref.py,
ELEMENT BY ELEMENT: |out - ref| <= attention_bound, a bound derived from the kernels' roundings (two 16-bit roundings and the f32
arithmetic; see attn_ref.py), relative to A_d = sum_j p_j |v_jd| of the element's own row. The max-norm criterion of
tests/test_gpu_ops.py measures every row against the largest value of the whole output; a causal row 4000 is an average of thousands
of values and smaller than that allowance altogether.

Inputs (attn_ref.py): 'gauss' as in tests/test_gpu_ops.py; 'addressed' — every row puts >= 0.3 of its weight (asserted on the
reference) on ONE chosen key: the diagonal, i - 1, the first live key of a left-padded sequence, the keys at both edges of a 64-key
tile, i - 64 / 127 / 128, the ViT's cls key and last key and a sweep over every (q-block, kv tile) pair, the first and last key of every
split of the decode kernel — with a peak of 12 (under the lazy running max's re-base threshold) and of 24 (over it: the redo path);
'future' — the best-scoring key is the first one the mask hides (i + 1, or kv_lo - 1 of a left pad).
Every output buffer starts as NaN; rows >= kv_len of K hold finite rows that would score highest and of V hold 1e4 (they meet P = 0
only; NaN there would prove nothing). Every head is checked, V differs per kv head. The reference runs in float64 on the device,
in chunks of query rows. tests/test_attn_ref_host.py pins the bound on the CPU from both sides.

Measured on an MI355X when the file was written (the tests print these figures, `-s`; none is a limit). Worst |err| / bound:
causal 16-bit 0.85 (S 4718, addressed, peak 12, hd 64, bf16, the left-padded sequence: head 31, row 1704, d 52; fp16 0.67), causal
f32 0.018 (S 128; 0.002 at S 4718); ViT 0.91 in each of its three forms (addressed, peak 24, hd 64, bf16: tile 16, head 6, row 177;
fp16 0.71; f32 0.016); decode 0.39 (kv_len 4781, B 64, hd 128, bf16, addressed, with kv_start; fp16 0.24; gauss 0.15). Against
3 * 2^-9 A, the count this file's issue started from, the same runs reach 1.24 (causal), 1.29 (ViT) and 0.55 (decode): bf16's
rounding errs by up to 2^-8, not 2^-9, and the kernel is right — hence the derivation in attn_ref.py. The whole file: 198 tests, 10 s.
One-line mutants of the kernels (scratch builds, never committed), this file / the attention tests of tests/test_gpu_ops.py /
tests/test_gpu_e2e.py + tests/test_gpu_continuous.py:
    rows >= 2048 miss their diagonal key (v2 kernel)  32 fail: every 16-bit case with S >= 4296, 4.7 .. 3e5 x the bound / pass / pass
    causal limit kv <= q + coff + 1 (v2 kernel)       79 fail: every 16-bit causal case but one, up to 8e5 (gauss, future) / 48 fail / 9 fail
    kv_end one tile short for the last q-block        80 fail: every 16-bit causal case, 1.8 .. 1e6 / 38 fail / 14 fail
    kvh = head % Hkv                                  80 fail: every 16-bit causal case, 6e4 .. 2e7 / 32 fail / 11 fail
    kv_prefix starts from l0 = 0                      12 fail: every 16-bit ViT case, kv_prefix form alone, 2.3 .. 3e6 / 35 fail / pass
    decode: split 1 starts one row late               20 fail: every B = 1 case (8 splits), 1.2 .. 98 / 32 fail / 1 fails
The f32 cases stay green under all of them: they run attn_f32_kernel, which the mutants leave alone."""
import gc

import pytest
import torch

from attn_ref import (LOG2E, adversarial_pad, attention_bound, attention_ref, causal_targets, decode_targets, key_weight, make_inputs,
                      score_scale, vit_targets, worst)

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]
HQ, HKV = 32, 8
PEAK = {"addressed12": 12.0, "addressed24": 24.0, "future": 12.0}
ISSUE_EPS = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}


@pytest.fixture(scope="module")
def dev():
    from gar_amd import hip
    hip.require_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def log():
    """worst err / bound per kernel family, printed when the module is done"""
    seen = {}

    def add(key, r, where):
        if key not in seen or r > seen[key][0]:
            seen[key] = (r, where)
    yield add
    for key in sorted(seen):
        print(f"\n[attention] {key}: worst err / bound {seen[key][0]:.3f} at {seen[key][1]}", end="")
    print()
    gc.collect()
    torch.cuda.empty_cache()


def check(log, key, label, out, Q, K, V, causal, dt, kv_lo, kv_len, rows_from=None):
    """out [B, Hq, n, hd] (a view of the kernel's O) against the f64 restatement: finite everywhere, under the bound in every
    element of the rows that are compared (sequence b: rows >= rows_from[b]; the rows in front of a left pad are padding)."""
    assert bool(torch.isfinite(out.float()).all()), f"{label}: non-finite output"
    ref, A = attention_ref(Q, K, V, causal, kv_lo, kv_len)
    bound = attention_bound(A, ref, dt, kv_len, score_scale(Q, K, kv_len))
    o = out.double()
    if rows_from is not None:
        o = o.clone()
        for b, r in enumerate(rows_from):
            o[b, :, :r] = ref[b, :, :r]
    r, idx, err, bnd = worst(o, ref, bound)
    where = f"{label} (b, head, row, d) = {idx}: |err| {err:.3e}, bound {bnd:.3e}, ref {float(ref[idx]):+.3e}"
    extra = ""
    if dt in ISSUE_EPS:      # the figure against 3 * 2^-9 A (bf16), the count this file's issue started from; not asserted
        extra = f"; err / (3 eps A) {float(((o - ref).abs() / (3 * ISSUE_EPS[dt] * A + 1e-30)).max()):.3f}"
    print(f"{key} | {label}: worst err / bound {r:.3f} at {idx}{extra}")
    log(key, r, where)
    assert r <= 1.0, f"worst err / bound {r:.3f}: {where}"
    if dt == torch.float32:  # nothing gets looser: close(out, ref, f32, extra=2.0) of tests/test_gpu_ops.py as well
        assert float((o - ref).abs().max()) <= 2.0 * 2e-5 * max(float(ref.abs().max()), 1e-6) + 1e-6, label
    return ref


def heads_view(O, B, n, H, hd):
    return O.view(B, n, H, hd).permute(0, 2, 1, 3)


# ---- 1. causal prefill ---------------------------------------------------------------------------------------------------------
def causal_inputs(family, S, hd, dt, lo, dev, seed):
    B = len(lo)
    rows = (S + 64) // 64 * 64                      # at least one row behind the last key
    if family == "gauss":
        target = None
    elif family == "future":
        i = torch.arange(S, device=dev)
        target = torch.stack([torch.where((i % 2 == 1) & (i >= l) & (l > 0), l - 1, i + 1) for l in lo])[:, None].expand(B, HQ, S)
    else:
        target = causal_targets(S, HQ, lo, dev)
    Q, K, V = make_inputs("gauss" if family == "gauss" else "addressed", B, HQ, HKV, S, rows, hd, dt, seed, target, PEAK.get(family),
                          device=dev)
    if family != "future":                          # ('future': row S - 1 aims at row S, which already scores highest for it)
        adversarial_pad(Q, K, V, S)
    V[:, :, S:] = 1e4
    return Q, K, V, target, rows


# (S, family, left-padded): all families at 4718 on a left-padded batch of two (pads 0 and 1500: more than eleven q-blocks, ending
# inside a tile) and one at B = 1 without kv_start; the video (4296) and relationship (5660) prompts with one family each; the q-block
# edge 127 / 128 / 129 at the real head counts
CAUSAL = [(4718, "gauss", True), (4718, "addressed12", True), (4718, "addressed24", True), (4718, "future", True),
          (4718, "addressed12", False), (4296, "addressed24", False), (5660, "future", False), (5660, "gauss", False)]
CAUSAL += [(S, f, p) for S in (127, 128, 129) for f, p in (("gauss", False), ("addressed12", True), ("addressed24", False),
                                                           ("future", True))]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("S,family,padded", CAUSAL)
def test_causal_prefill_at_the_models_geometry(dev, log, S, family, padded, hd, dt):
    """gar_attention_vrow, causal, V row-major as GARModel calls it; 16-bit: attn_bf16_v2_kernel, f32: attn_f32_kernel"""
    from gar_amd import ops
    lo = ([0, 1500] if S > 2000 else [0, 70]) if padded else [0]
    B = len(lo)
    Q, K, V, target, rows = causal_inputs(family, S, hd, dt, lo, dev, seed=S + hd + len(family))
    Spad = (S + 63) // 64 * 64
    Qp = torch.zeros(B, HQ, Spad, hd, dtype=dt, device=dev)
    Qp[:, :, :S] = Q
    O = torch.full((B * S, HQ * hd), float("nan"), dtype=dt, device=dev)
    kv_start = torch.tensor(lo, dtype=torch.int32, device=dev) if padded else None
    ops.attention(Qp, K, V, O, B, HQ, HKV, hd, S, Spad, S, rows, causal=True, kv_start=kv_start, v_row_major=True)
    torch.cuda.synchronize()
    key = "causal f32" if dt == torch.float32 else "causal 16-bit"
    label = f"S {S} {family} hd {hd} {str(dt)[6:]} B {B}{' kv_start ' + str(lo) if padded else ''}"
    if target is not None and family != "future":
        w = key_weight(Q, K, target, True, lo, S)
        for b, l in enumerate(lo):
            assert float(w[b, :, l:].min()) >= 0.3, f"{label}: target weight {float(w[b, :, l:].min()):.3f}"
    check(log, key, label, heads_view(O, B, S, HQ, hd), Q, K, V, True, dt, lo, S, rows_from=lo)


# ---- 2. ViT ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,hd", [(torch.bfloat16, 64), (torch.bfloat16, 96), (torch.float16, 64), (torch.float16, 96),
                                   (torch.float32, 64), (torch.float32, 128)])
@pytest.mark.parametrize("family", ["gauss", "addressed12", "addressed24"])
def test_vit_attention_at_the_models_geometry(dev, log, family, dt, hd):
    """non-causal, 16 heads, 17 tiles, 1025 tokens in rows of 1088: V transposed, V row-major (bit-equal to it), and in 16-bit
    V row-major with the cls key folded into the initial softmax state (kv_prefix = 1)"""
    from gar_amd import ops
    T, H, N, Npad = 17, 16, 1025, 1088
    target = vit_targets(N, H, dev)[None].expand(T, H, N)
    Q, K, V = make_inputs("gauss" if family == "gauss" else "addressed", T, H, H, N, Npad, hd, dt, 100 + hd, target, PEAK.get(family),
                          device=dev)
    adversarial_pad(Q, K, V, N)
    Qp = torch.zeros(T, H, Npad, hd, dtype=dt, device=dev)
    Qp[:, :, :N] = Q
    Vt = V.transpose(2, 3).contiguous()
    if family != "gauss":
        w = key_weight(Q, K, target, False, None, N)
        assert float(w.min()) >= 0.3, float(w.min())
    label = f"{family} hd {hd} {str(dt)[6:]}"
    outs = []
    for form, vv, kw in (("Vt", Vt, {}), ("row-major", V, {"v_row_major": True}), ("kv_prefix", V, {"v_row_major": True, "kv_prefix": 1})):
        if form == "kv_prefix" and dt == torch.float32:
            continue
        O = torch.full((T * N, H * hd), float("nan"), dtype=dt, device=dev)
        ops.attention(Qp, K, vv, O, T, H, H, hd, N, Npad, N, Npad, causal=False, **kw)
        torch.cuda.synchronize()
        check(log, f"vit {form}" + (" f32" if dt == torch.float32 else ""), label, heads_view(O, T, N, H, hd), Q, K, V, False, dt, None, N)
        outs.append(O)
    assert torch.equal(outs[0], outs[1])            # same P, same V, same MFMA order


# ---- 3. decode over a real-length cache --------------------------------------------------------------------------------------------
def _rope_tables(rows, hd, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    fr = torch.arange(rows, device=dev, dtype=torch.float32)[:, None] * inv[None]
    return fr.cos().contiguous(), fr.sin().contiguous()


def _unrope(x, c, s):
    """x [..., hd] with cos / sin [..., hd / 2] of its position: the vector that the half-split rotation turns into x"""
    x1, x2 = x.chunk(2, -1)
    return torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], -1)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("B", [1, 16, 64])
@pytest.mark.parametrize("kv_len", [4718, 4719, 4736, 4737, 4718 + 63])
def test_decode_over_a_real_length_cache(dev, log, kv_len, B, hd, dt):
    """gar_llm_qkv_post (S = 1) + gar_attention_decode against f64, and gar_attention_decode_qkv bit-equal to the pair, caches
    included; nsplit as GARModel chooses it and 1; with and without kv_start; 'gauss', and 'addressed' with the query of (b, head)
    aimed at the ((b Hq + head) % len)-th key of decode_targets: the first live key, the appended key, both ends of every split."""
    from gar_amd import ops
    from gar_amd.modeling_gar import GARModel
    Smax = 4864
    G = HQ // HKV
    Wd = (HQ + 2 * HKV) * hd
    scale = hd ** -0.5 * LOG2E
    cos, sin = _rope_tables(Smax, hd, dev)
    model_nsplit = max(1, min(GARModel.DECODE_ATTN_MAX_SPLITS, GARModel.DECODE_ATTN_BLOCKS // max(1, B * HKV)))
    pos = torch.tensor([kv_len - 1], dtype=torch.int32, device=dev)
    kvl = torch.tensor([kv_len], dtype=torch.int32, device=dev)
    for padded in (False, True):
        lo = [(0, 1500)[b % 2] if B > 1 else 1500 for b in range(B)] if padded else [0] * B
        lp = torch.tensor(lo, dtype=torch.int32, device=dev) if padded else None
        rp = torch.tensor([kv_len - 1 - l for l in lo], device=dev)                          # RoPE position of the step's token
        c1, s1 = cos[rp][:, None], sin[rp][:, None]                                          # [B, 1, hd / 2]
        for family in ("gauss", "addressed"):
            for nsplit in sorted({model_nsplit, 1}):
                gen = torch.Generator(device=dev).manual_seed(kv_len * 7 + B + hd + nsplit)
                V0 = torch.randn(B, HKV, Smax, hd, generator=gen, device=dev).to(dt)
                raw = torch.randn(B, HQ + 2 * HKV, hd, generator=gen, device=dev)
                target = None
                if family == "gauss":
                    K0 = torch.randn(B, HKV, Smax, hd, generator=gen, device=dev).to(dt)
                else:
                    codes = torch.nn.functional.normalize(torch.randn(B, HKV, Smax, hd, generator=gen, device=dev), dim=-1)
                    K0 = codes.to(dt)
                    tg = [decode_targets(kv_len, l, nsplit) for l in lo]
                    target = torch.tensor([[tg[b][(b * HQ + h) % len(tg[b])] for h in range(HQ)] for b in range(B)], device=dev)
                    want = 12.0 * codes.repeat_interleave(G, 1).gather(2, target[:, :, None, None].expand(B, HQ, 1, hd))[:, :, 0]
                    raw[:, HQ:HQ + HKV] = _unrope(codes[:, :, kv_len - 1], c1, s1)            # the appended key: the code of its row
                    raw[:, :HQ] = _unrope(want / scale, c1, s1)
                raw = raw.to(dt).view(B, Wd)
                Q1 = torch.empty(B, HQ, 1, hd, dtype=dt, device=dev)
                Kc, Vc = K0.clone(), V0.clone()
                ops.llm_qkv_post(raw, cos, sin, Q1, Kc, Vc, B, 1, 1, HQ, HKV, hd, Smax, 0, pos, scale, left_pad=lp)
                for Kx, Vx in ((K0, V0), (Kc, Vc)):
                    adversarial_pad(Q1, Kx, Vx, kv_len)
                ws = torch.empty(ops.attention_decode_workspace(B, HQ, hd, nsplit), dtype=torch.uint8, device=dev)
                O = torch.full((B, HQ * hd), float("nan"), dtype=dt, device=dev)
                ops.attention_decode(Q1, Kc, Vc, O, B, HQ, HKV, hd, Smax, kvl, nsplit, ws, kv_start=lp)
                Kf, Vf, O2 = K0.clone(), V0.clone(), torch.full_like(O, float("nan"))
                assert ops.attention_decode_qkv(raw, cos, sin, Kf, Vf, O2, B, HQ, HKV, hd, Smax, pos, scale, nsplit, ws, left_pad=lp)
                torch.cuda.synchronize()
                label = f"kv_len {kv_len} B {B} hd {hd} {str(dt)[6:]} {family} nsplit {nsplit}{' kv_start' if padded else ''}"
                assert torch.equal(O2, O) and torch.equal(Kf, Kc) and torch.equal(Vf, Vc), label
                if target is not None:
                    w = key_weight(Q1, Kc, target[:, :, None], False, lo, kv_len)
                    assert float(w.min()) >= 0.3, f"{label}: target weight {float(w.min()):.3f}"
                check(log, "decode", label, O.view(B, HQ, 1, hd), Q1, Kc, Vc, False, dt, lo, kv_len)
                del K0, V0, Kc, Vc, Kf, Vf
