"""GPU (-m gpu): the opt-in FP8 (OCP e4m3fn) KV cache of the decode path — GARModel(kv_cache_dtype="fp8").

Numerics restated here (include/gar_hip.h, FP8 KV cache): a 16-bit vector x is stored as
    amax = max|x|, inv = 448 / amax, q = e4m3(RNE(x * inv)), scale = amax / 448     (inv not finite: q = 0, scale = 0)
and the decode attention computes score_j = (q . k8_j) * sk_j and weights V by p_j * sv_j."""

import pytest
import torch

pytestmark = pytest.mark.gpu

# fp8 decode attention vs an fp32 attention over the DEQUANTIZED cache: the kernel rounds p * sv to the 16-bit type before the PV
# product and sums in another order — relative L2 error of the output bounded by a few 16-bit roundings
DECODE_FP8_REL_L2 = {torch.bfloat16: 1.5e-2, torch.float16: 3e-3}
# decode-step logits of the fp8 cache vs the default cache, teacher-forced on the default cache's tokens (synthetic weights): e4m3
# keeps 3 mantissa bits (relative rounding up to 2^-4 per cached element, against 2^-8 for bf16), so this is a looser bound than
# bf16's 6e-2 against f32; the token-level gate is the agreement measured by tools/bench_kv_fp8.py
FP8_STEP_REL_L2 = 0.2


def _quant_ref(x: torch.Tensor):
    """torch restatement of gar_kv_quantize_fp8 on [..., hd] 16-bit vectors -> (uint8 bytes, f32 scales), on the CPU (correctly
    rounded f32 divisions; a CUDA tensor / scalar division multiplies by the reciprocal)"""
    xf = x.float().cpu()
    amax = xf.abs().amax(-1, keepdim=True)
    inv = torch.tensor(448.0, dtype=torch.float32) / amax
    q = (xf * inv).to(torch.float8_e4m3fn).view(torch.uint8)
    zero = ~(inv < float("inf"))          # amax == 0, or amax < 448 / FLT_MAX (bf16 holds such values)
    q = torch.where(zero, torch.zeros_like(q), q)
    scale = torch.where(zero, torch.zeros_like(amax), amax / 448.0)
    return q, scale.squeeze(-1)


def _dequant(q8: torch.Tensor, s: torch.Tensor):
    return q8.view(torch.float8_e4m3fn).float() * s.unsqueeze(-1)


def _vectors(kind, shape, dt, g):
    x = torch.randn(shape, generator=g)
    if kind == "zero":
        x[..., :] = 0
        x[0, 0, 1::3] = -0.0
    elif kind == "huge":
        x = x * 1e30 if dt == torch.bfloat16 else x * 6e3
    elif kind == "below_inv_range":      # bf16: amax < 448 / FLT_MAX, 448 / amax overflows -> stored as zeros, not NaN
        x = x * 1e-38 if dt == torch.bfloat16 else x * 1e-5
        x[0, 0, 0, 0] = 3e-36 if dt == torch.bfloat16 else 1e-3         # one vector just inside the range
    elif kind == "tiny":
        x = x * 1e-30 if dt == torch.bfloat16 else x * 1e-3
    elif kind == "mixed":       # a wide dynamic range inside one vector (small elements go subnormal / to zero in e4m3)
        x = x * torch.logspace(-12, 2, shape[-1]) if dt == torch.bfloat16 else x * torch.logspace(-5, 2, shape[-1])
    return x.to(dt).cuda()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind", ["random", "zero", "huge", "tiny", "mixed", "below_inv_range"])
def test_kv_quantize_matches_torch_restatement(dt, hd, kind):
    from gar_amd import ops
    g = torch.Generator().manual_seed(hd + len(kind))
    B, Hkv, S, Spad, Smax, k0 = 2, 3, 70, 128, 192, 5
    K = _vectors(kind, (B, Hkv, Spad, hd), dt, g)
    V = _vectors("random" if kind == "zero" else kind, (B, Hkv, Spad, hd), dt, g)
    Kc8 = torch.full((B, Hkv, Smax, hd), 0x5A, dtype=torch.uint8, device="cuda")
    Vc8 = Kc8.clone()
    Ks = torch.full((B, Hkv, Smax), -1.0, device="cuda")
    Vs = Ks.clone()
    ops.kv_quantize_fp8(K, V, Kc8, Vc8, Ks, Vs, B, Hkv, hd, Smax, S, kv_start=k0)
    torch.cuda.synchronize()
    for src, c8, sc in ((K, Kc8, Ks), (V, Vc8, Vs)):
        q, s = _quant_ref(src[:, :, k0:S])
        assert torch.equal(c8[:, :, k0:S].cpu(), q)
        assert torch.equal(sc[:, :, k0:S].cpu(), s)
        assert bool(torch.isfinite(_dequant(c8[:, :, k0:S], sc[:, :, k0:S])).all())
        # rows outside kv_start .. S - 1 untouched
        assert bool((c8[:, :, :k0] == 0x5A).all()) and bool((c8[:, :, S:] == 0x5A).all())
        assert bool((sc[:, :, :k0] == -1).all()) and bool((sc[:, :, S:] == -1).all())


def _attn_ref(q, K, V, kv_len, kv_start, G):
    """fp32 attention of q [B, Hq, hd] (pre-scaled by hd^-0.5 * log2 e: exp2 softmax) over K / V [B, Hkv, >= kv_len, hd]"""
    B, Hq, hd = q.shape
    out = torch.empty(B, Hq, hd, dtype=torch.float64)
    for b in range(B):
        lo = int(kv_start[b]) if kv_start is not None else 0
        for hq in range(Hq):
            k = K[b, hq // G, lo:kv_len].double()
            v = V[b, hq // G, lo:kv_len].double()
            sc = k @ q[b, hq].double()
            p = torch.pow(2.0, sc - sc.max())
            out[b, hq] = (p @ v) / p.sum()
    return out


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kv_len", [1, 63, 65, 200, 1000])
def test_attention_decode_fp8_against_dequantized_fp32(dt, hd, kv_len):
    """GQA 4 (8 query heads over 2 kv heads), one split and several, with and without left padding: the fp8 kernel against an
    fp32 attention over the dequantized cache."""
    from gar_amd import ops
    g = torch.Generator().manual_seed(kv_len * 7 + hd)
    B, Hq, Hkv, Smax = 3, 8, 2, 1024
    K16 = (torch.randn(B, Hkv, Smax, hd, generator=g) * 2).to(dt).cuda()
    V16 = torch.randn(B, Hkv, Smax, hd, generator=g).to(dt).cuda()
    Kc8 = torch.empty(B, Hkv, Smax, hd, dtype=torch.uint8, device="cuda")
    Vc8 = torch.empty_like(Kc8)
    Ks = torch.empty(B, Hkv, Smax, device="cuda")
    Vs = torch.empty_like(Ks)
    ops.kv_quantize_fp8(K16, V16, Kc8, Vc8, Ks, Vs, B, Hkv, hd, Smax, Smax)
    Kd, Vd = _dequant(Kc8, Ks).cpu(), _dequant(Vc8, Vs).cpu()
    q = (torch.randn(B, Hq, hd, generator=g) * (hd ** -0.5) * 1.4426950408889634).to(dt).cuda()
    kvl = torch.tensor([kv_len], dtype=torch.int32, device="cuda")
    for kv_start in (None, [0, min(kv_len - 1, 3), max(0, kv_len - 70)]):
        ks = None if kv_start is None else torch.tensor(kv_start, dtype=torch.int32, device="cuda")
        ref = _attn_ref(q.float().cpu(), Kd, Vd, kv_len, kv_start, Hq // Hkv)
        for nsplit in (1, 5):
            ws = torch.empty(ops.attention_decode_fp8_workspace(B, Hq, hd, nsplit), dtype=torch.uint8, device="cuda")
            O = torch.full((B, Hq * hd), float("nan"), dtype=dt, device="cuda")
            ops.attention_decode_fp8(q, Kc8, Vc8, Ks, Vs, O, B, Hq, Hkv, hd, Smax, kvl, nsplit, ws, kv_start=ks)
            torch.cuda.synchronize()
            err = _rel_l2(O.view(B, Hq, hd).float(), ref)
            assert err < DECODE_FP8_REL_L2[dt], (kv_start, nsplit, err)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hd", [64, 128])
def test_fused_qkv_fp8_equals_unfused(dt, hd):
    """gar_attention_decode_qkv_fp8 (RoPE + quantize + append + attend in one launch) against gar_llm_qkv_post into a 16-bit
    row, gar_kv_quantize_fp8 of that row, gar_attention_decode_fp8: the same cache bytes and scales, the same output."""
    from gar_amd import ops
    g = torch.Generator().manual_seed(hd)
    B, Hq, Hkv, Smax, pos = 3, 8, 2, 256, 130
    qd = (Hq + 2 * Hkv) * hd
    ang = torch.arange(Smax, dtype=torch.float32)[:, None] * torch.pow(1e4, -torch.arange(hd // 2) / (hd // 2))[None]
    cos, sin = ang.cos().cuda(), ang.sin().cuda()
    qkv = torch.randn(B, qd, generator=g).to(dt).cuda()
    q_scale = (hd ** -0.5) * 1.4426950408889634
    lp = torch.tensor([0, 5, 64], dtype=torch.int32, device="cuda")
    K16 = torch.randn(B, Hkv, Smax, hd, generator=g).to(dt).cuda()
    V16 = torch.randn(B, Hkv, Smax, hd, generator=g).to(dt).cuda()
    caches = []
    for _ in range(2):
        Kc8 = torch.zeros(B, Hkv, Smax, hd, dtype=torch.uint8, device="cuda")
        Vc8, Ks, Vs = torch.zeros_like(Kc8), torch.zeros(B, Hkv, Smax, device="cuda"), torch.zeros(B, Hkv, Smax, device="cuda")
        ops.kv_quantize_fp8(K16, V16, Kc8, Vc8, Ks, Vs, B, Hkv, hd, Smax, pos)
        caches.append((Kc8, Vc8, Ks, Vs))
    pos_dev = torch.tensor([pos], dtype=torch.int32, device="cuda")
    kvl = torch.tensor([pos + 1], dtype=torch.int32, device="cuda")
    for nsplit in (1, 4):
        ws = torch.empty(ops.attention_decode_fp8_workspace(B, Hq, hd, nsplit), dtype=torch.uint8, device="cuda")
        Of = torch.empty(B, Hq * hd, dtype=dt, device="cuda")
        Kc8, Vc8, Ks, Vs = caches[0]
        ops.attention_decode_qkv_fp8(qkv, cos, sin, Kc8, Vc8, Ks, Vs, Of, B, Hq, Hkv, hd, Smax, pos_dev, q_scale, nsplit, ws,
                                     left_pad=lp)
        Q = torch.empty(B, Hq, 1, hd, dtype=dt, device="cuda")
        K1, V1 = K16.clone(), V16.clone()
        ops.llm_qkv_post(qkv, cos, sin, Q, K1, V1, B, 1, 1, Hq, Hkv, hd, Smax, 0, pos_dev, q_scale, left_pad=lp)
        Ku8, Vu8, Kus, Vus = caches[1]
        ops.kv_quantize_fp8(K1, V1, Ku8, Vu8, Kus, Vus, B, Hkv, hd, Smax, pos + 1, kv_start=pos)
        Ou = torch.empty_like(Of)
        ops.attention_decode_fp8(Q, Ku8, Vu8, Kus, Vus, Ou, B, Hq, Hkv, hd, Smax, kvl, nsplit, ws, kv_start=lp)
        torch.cuda.synchronize()
        for a, b in zip(caches[0], caches[1]):
            assert torch.equal(a, b)
        assert torch.equal(Of, Ou), _rel_l2(Of.float(), Ou.float())


@pytest.fixture(scope="module")
def tiny():
    from gar_amd import GARConfig
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.tiny()
    return cfg, synthetic_weights(cfg), GARProcessor.from_config(cfg, max_num_tiles=4)


def _sample(cfg, proc, i, w=200, h=160, dtype=torch.bfloat16, multi=False):
    from gar_amd.eval_dataset import MultiRegionDataset, SingleRegionCaptionDataset
    from gar_amd.synthetic import synthetic_disjoint_masks, synthetic_image, synthetic_mask
    img = synthetic_image(i, w, h)
    if multi:
        masks = synthetic_disjoint_masks(i, 3, w, h)
        qs = "What is the relationship between <Prompt0>, <Prompt1> and <Prompt2>?"
        return MultiRegionDataset(img, masks, qs, proc, data_dtype=dtype, device="cpu")[0]
    return SingleRegionCaptionDataset(img, synthetic_mask(i, w, h), proc, data_dtype=dtype, device="cpu")[0]


def _batch(ss):
    return dict(input_ids=torch.cat([s["input_ids"] for s in ss]), pixel_values=torch.cat([s["pixel_values"] for s in ss]),
                global_mask_values=torch.cat([s["global_mask_values"] for s in ss]), bboxes=[b for s in ss for b in s["bboxes"]],
                aspect_ratios=torch.cat([s["aspect_ratios"] for s in ss]))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_fp8_cache_end_to_end_tiny(tiny, dt):
    """prefill logits and the first token bit-identical to the default cache; graph replay == eager launches; the cache is one
    byte per element and its bytes (scales included) <= 0.57 x the default cache's; decode logits stay near the default's."""
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    ss = [_sample(cfg, proc, i, dtype=dt) for i in (3, 4)]
    b = _batch(ss)
    n = 10
    m16 = GARModel(cfg, W, dt)
    m8 = GARModel(cfg, W, dt, kv_cache_dtype="fp8")
    r16 = m16.generate(**b, max_new_tokens=n, return_logits=True)
    r8 = m8.generate(**b, max_new_tokens=n, return_logits=True)
    assert torch.equal(r8.logits[:, 0], r16.logits[:, 0]) and torch.equal(r8.sequences[:, 0], r16.sequences[:, 0])
    e8 = m8.generate(**b, max_new_tokens=n, return_logits=True, use_graph=False)
    assert torch.equal(e8.logits, r8.logits) and torch.equal(e8.sequences, r8.sequences)
    # teacher-forced on the default cache's tokens: every step's logits close to the default's
    t8 = m8.generate(**b, max_new_tokens=n, return_logits=True, forced_tokens=r16.sequences)
    for j in range(n):
        err = _rel_l2(t8.logits[:, j], r16.logits[:, j])
        print(f"step {j}: fp8 vs default cache, teacher-forced logits rel-L2 {err:.3e}")
        assert err < FP8_STEP_REL_L2, (j, err)
    (k8, st8), (k16, st16) = [next((k, m._ws[k]) for k in m._ws if k[0] == "llm") for m in (m8, m16)]
    assert st8["Kc"].dtype == torch.uint8 and st8["Kc"].element_size() == 1 and st8["Ks"].dtype == torch.float32
    bytes8 = sum(st8[k].numel() * st8[k].element_size() for k in ("Kc", "Vc", "Ks", "Vs"))
    bytes16 = sum(st16[k].numel() * st16[k].element_size() for k in ("Kc", "Vc"))
    assert bytes8 <= 0.57 * bytes16, (bytes8, bytes16)
    assert "Ks" not in st16


def test_fp8_cache_left_padded_batch_equals_singles(tiny):
    """a batch of prompts of different lengths (single- and three-region questions: left-padded) against each prompt alone: the
    same first tokens, and teacher-forced on the single runs' tokens, every step's logits within the fp8 bound of the single run's
    (the padded rows sit at other cache rows, so tile boundaries and 16-bit roundings differ; an fp8 rounding boundary can
    amplify such a difference into one e4m3 step)"""
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    m = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype="fp8")
    ss = [_sample(cfg, proc, 30), _sample(cfg, proc, 31, multi=True)]
    assert ss[0]["input_ids"].shape[1] != ss[1]["input_ids"].shape[1]
    n = 8
    singles = [m.generate(**s, max_new_tokens=n).sequences[0].cpu() for s in ss]
    S = max(int(s["input_ids"].shape[1]) for s in ss)
    pad_id = 0
    ids = torch.full((2, S), pad_id, dtype=torch.int64)
    mask = torch.zeros(2, S, dtype=torch.int64)
    for i, s in enumerate(ss):
        L = int(s["input_ids"].shape[1])
        ids[i, S - L:] = s["input_ids"][0]
        mask[i, S - L:] = 1
    b = dict(pixel_values=torch.cat([s["pixel_values"] for s in ss]),
             global_mask_values=torch.cat([s["global_mask_values"] for s in ss]), bboxes=[x for s in ss for x in s["bboxes"]],
             aspect_ratios=torch.cat([s["aspect_ratios"] for s in ss]), input_ids=ids, attention_mask=mask)
    out = m.generate(**b, max_new_tokens=n).sequences.cpu()
    for i in range(2):
        print(f"row {i}: batch {out[i].tolist()} alone {singles[i].tolist()}")
        assert torch.equal(out[i, :3], singles[i][:3]), i
    one = [m.generate(**s, max_new_tokens=n, return_logits=True) for s in ss]
    tf = m.generate(**b, max_new_tokens=n, return_logits=True, forced_tokens=torch.stack(singles).cuda())
    for i in range(2):
        assert _rel_l2(tf.logits[i, 0], one[i].logits[0, 0]) < 2e-2
        for j in range(n):
            err = _rel_l2(tf.logits[i, j], one[i].logits[0, j])
            print(f"row {i} step {j}: batch vs alone, teacher-forced logits rel-L2 {err:.3e}")
            assert err < FP8_STEP_REL_L2, (i, j, err)


def _pick_eos(streams, n_ids, max_new):
    """eos ids out of the regions' own streams whose cuts give MIXED caption lengths (tests/test_gpu_continuous.py's rule): short
    rows retire and let later groups in while long ones still run, so the shared clock outgrows Smax and rows are re-based"""
    cand = sorted({t for s in streams for t in s})

    def lengths(eos):
        return [next((j + 1 for j, t in enumerate(s) if t in eos), max_new) for s in streams]
    eos = set()
    for _ in range(n_ids):
        best = None
        for c in cand:
            if c in eos:
                continue
            ls = lengths(eos | {c})
            spread = len(set(ls)) - 0.02 * abs(sum(ls) / len(ls) - 0.5 * max_new)
            if best is None or spread > best[0]:
                best = (spread, c)
        eos.add(best[1])
    return sorted(eos)


def test_fp8_cache_continuous_batcher_equals_generate(tiny):
    """a ContinuousBatcher on an fp8 model decodes with the fp8 cache. The row moves are checked exactly: every admitted row's
    bytes and scales equal its staging row's, every re-based row's equal what it held before the shift. The tokens equal each
    region's own fp8 generate() for most regions (measured 13-14 of 16); a region may part at a near-tie, because in 16-bit modes
    its prompt is prefilled in a batch whose make-up depends on admission timing, and its row sits at other cache rows (tile
    boundaries, roundings) than in the single run."""
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    B, NT = 4, 40            # Smax = round_up(261 + 40, 64) = 320: rows are re-based inside the cache while they decode
    m = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype="fp8")
    samples = [_sample(cfg, proc, 200 + i, multi=(i % 3 == 1)) for i in range(16)]
    streams = [m.generate(**s, max_new_tokens=NT).sequences[0].cpu().tolist() for s in samples]
    eos = _pick_eos(streams, 5, NT)
    exp = []
    for s in streams:
        cut = next((j + 1 for j, t in enumerate(s) if t in eos), len(s))
        exp.append(s[:cut])
    cb = ContinuousBatcher(m, slots=B, max_new_tokens=NT, eos_token_id=eos, poll_every=2, admit_min=1, horizon=0, smax_multiple=64)
    planes = ("Kc", "Vc", "Ks", "Vs")
    checked = {"admitted": 0, "rebased": 0}
    # exact checks of the row moves: an admitted row's cache bytes and scales equal its staging row's; a re-based row's equal
    # what the same row held before the shift
    staged = []
    begin = m.generate_begin

    def begin_recorded(*a, **kw):
        staged.append(begin(*a, **kw))
        return staged[-1]
    m.generate_begin = begin_recorded
    admit, rebase = cb._prompt_phase_and_admit, cb._rebase

    def admit_checked(group, free):
        admit(group, free)
        sg, S, P = staged[-1].st, max(int(x["input_ids"].shape[1]) for _, x in group), cb.P
        for i, (ticket, x) in enumerate(group):
            r = next(r for r, row in enumerate(cb.rows) if row is not None and row.ticket == ticket)
            n = int(x["input_ids"].shape[1])
            for k in planes:
                assert torch.equal(cb.st[k][:, r, :, P - n:P], sg[k][:, i, :, S - n:S]), (k, ticket)
            checked["admitted"] += 1

    def rebase_checked():
        P = cb.P
        live = [(r, row.left_pad) for r, row in enumerate(cb.rows) if row is not None]
        before = {k: cb.st[k].clone() for k in planes}
        moved = rebase()
        if moved:
            for r, lo in live:
                d = lo - cb.rows[r].left_pad
                assert d > 0
                for k in planes:
                    assert torch.equal(cb.st[k][:, r, :, lo - d:P - d], before[k][:, r, :, lo:P]), (k, r)
                checked["rebased"] += 1
        return moved
    cb._prompt_phase_and_admit, cb._rebase = admit_checked, rebase_checked
    tickets = [cb.submit(s) for s in samples]
    res = cb.flush()
    m.generate_begin = begin
    assert "Ks" in cb.st and cb.st["Kc"].dtype == torch.uint8
    print(f"row moves checked exactly: {checked}")
    assert checked["admitted"] == len(samples), checked
    agree = sum(res[t] == e for t, e in zip(tickets, exp))
    print(f"continuous fp8: {agree}/{len(exp)} regions equal their generate(); stats {cb.stats}")
    assert agree >= 0.6 * len(exp), agree


def test_fp8_continuous_rebase_moves_scale_planes_exactly(tiny):
    """the re-base (live rows shifted down inside the decode cache) moves the fp8 bytes AND the scale planes of every live row
    by the same d rows, byte for byte, and leaves free rows alone — driven directly on a batcher state filled with random bytes"""
    from gar_amd.continuous import ContinuousBatcher, _Row
    from gar_amd.modeling_gar import GARModel
    cfg, W, _ = tiny
    m = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype="fp8")
    cb = ContinuousBatcher(m, slots=4, max_new_tokens=16, use_graph=False, horizon=0, smax_multiple=64)
    P = 100
    cb._new_base(P)                                       # Smax = round_up(100 + 16, 64) = 128, clock at row 100
    st = cb.st
    g = torch.Generator(device="cuda").manual_seed(5)
    for k in ("Kc", "Vc"):
        st[k].copy_(torch.randint(0, 256, st[k].shape, generator=g, device="cuda", dtype=torch.int32).to(torch.uint8))
    for k in ("Ks", "Vs"):
        st[k].copy_(torch.rand(st[k].shape, generator=g, device="cuda"))
    pads = [7, None, 12, 30]                             # row 1 is free
    cb.rows = [None if lp is None else _Row(r, 0, lp, P - lp) for r, lp in enumerate(pads)]
    before = {k: st[k].clone() for k in ("Kc", "Vc", "Ks", "Vs")}
    cb._rebase()
    d = 7
    assert cb.P == P - d and cb.stats["rebases"] == 1
    for r, lp in enumerate(pads):
        for k in ("Kc", "Vc", "Ks", "Vs"):
            if lp is None:
                assert torch.equal(st[k][:, r], before[k][:, r]), (k, r)
            else:
                assert torch.equal(st[k][:, r, :, lp - d:P - d], before[k][:, r, :, lp:P]), (k, r)
    assert st["left_pad"][[0, 2, 3]].tolist() == [0, 5, 23]


def test_fp8_cache_gar1b_dims():
    """GAR-1B dims (head_dim 64, GQA 4), two Llama layers, a 16-tile prompt: first token and prefill logits bit-identical to
    the default cache, graph == eager, decode logits near the default's"""
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b(**{"vision.depth": 1, "text.num_hidden_layers": 2})
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    s = _sample(cfg, proc, 3, 1024, 1024)
    n = 6
    r16 = GARModel(cfg, W, torch.bfloat16).generate(**s, max_new_tokens=n, return_logits=True)
    m8 = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype="fp8")
    r8 = m8.generate(**s, max_new_tokens=n, return_logits=True)
    assert torch.equal(r8.logits[:, 0], r16.logits[:, 0]) and torch.equal(r8.sequences[:, 0], r16.sequences[:, 0])
    e8 = m8.generate(**s, max_new_tokens=n, return_logits=True, use_graph=False)
    assert torch.equal(e8.logits, r8.logits)
    t8 = m8.generate(**s, max_new_tokens=n, return_logits=True, forced_tokens=r16.sequences)
    for j in range(n):
        err = _rel_l2(t8.logits[:, j], r16.logits[:, j])
        print(f"step {j}: fp8 vs default cache, teacher-forced logits rel-L2 {err:.3e}")
        assert err < FP8_STEP_REL_L2, (j, err)



# ---- quality gate (DESIGN.md section 7 holds the table): teacher-forced top-1 agreement of the fp8 cache, synthetic weights.
# Floors = measured - 3 sigma of a binomial with the test's own n, frozen like FULL_DEPTH_BF16_AGREE (0.929; measured 0.9404) and
# FULL_DEPTH_8B_BF16_AGREE (0.787; measured 0.8359) in tests/test_gpu_e2e.py.
# (the bf16 cache in the same runs: 0.9392 vs f32 at GAR-1B, 0.8359 at GAR-8B — the e2e tests' values)
FP8_AGREE_F32_1B = 0.923     # fp8 cache vs the f32 path, GAR-1B B = 64 x 64 steps (n = 4096): measured 0.9348, sigma 0.0039
FP8_AGREE_BF16_1B = 0.950    # fp8 cache vs the bf16 cache, same steps: measured 0.9602, sigma 0.0031
FP8_AGREE_F32_8B = 0.776     # fp8 cache vs the f32 path, GAR-8B 16 regions x 32 steps (n = 512): measured 0.8262, sigma 0.0167
FP8_AGREE_BF16_8B = 0.849    # fp8 cache vs the bf16 cache, same steps: measured 0.8906, sigma 0.0138


def _agreement(name, seq_ref, seqs):
    out = {}
    for k, q in seqs.items():
        a = (q == seq_ref).float()
        n = a.numel()
        p = float(a.mean())
        out[k] = p
        print(f"{name}: {k} top-1 agreement {p:.4f} ({int(a.sum())} of {n}; sigma {((p * (1 - p)) / n) ** 0.5:.4f}; "
              f"worst region {float(a.mean(1).min()):.3f})")
    return out


def _forced_runs(cfg, W, batch, seq32, NT):
    """bf16 cache and fp8 cache, each teacher-forced on the f32 path's tokens: their top-1 choices at every step"""
    from gar_amd.modeling_gar import GARModel
    bb = {k: (v.to(torch.bfloat16) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    seqs = {}
    for name, kv in (("bf16", None), ("fp8", "fp8")):
        m = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype=kv)
        seqs[name] = m.generate(**bb, max_new_tokens=NT, forced_tokens=seq32).sequences.clone()
        del m
        torch.cuda.empty_cache()
    return seqs


def test_fp8_quality_gate_gar1b_bench_configuration():
    """The configuration bench.py times (full-depth GAR-1B, B = 64 distinct regions, 64 steps): top-1 agreement of the fp8 cache
    with the f32 path and with the bf16 cache, teacher-forced on the f32 path's tokens."""
    from gar_amd import GARConfig
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    W = synthetic_weights(cfg)
    B, NT = 64, 64
    proc = GARProcessor.from_config(cfg, max_num_tiles=16).use_gpu_preprocessing("cuda:0", torch.float32)
    ss = [SingleRegionCaptionDataset(synthetic_image(700 + i), synthetic_mask(700 + i), proc, data_dtype=torch.float32,
                                     device="cuda:0")[0] for i in range(B)]
    batch = dict(input_ids=torch.cat([x["input_ids"] for x in ss]), pixel_values=torch.cat([x["pixel_values"] for x in ss]),
                 global_mask_values=torch.cat([x["global_mask_values"] for x in ss]), bboxes=[x["bboxes"][0] for x in ss],
                 aspect_ratios=torch.cat([x["aspect_ratios"] for x in ss]))
    del ss
    m32 = GARModel(cfg, W, torch.float32)
    seq32 = m32.generate(**batch, max_new_tokens=NT).sequences.clone()
    del m32
    torch.cuda.empty_cache()
    seqs = _forced_runs(cfg, W, batch, seq32, NT)
    r32 = _agreement("GAR-1B B = 64 x 64 steps vs f32", seq32, seqs)
    r16 = _agreement("GAR-1B B = 64 x 64 steps vs bf16 cache", seqs["bf16"], {"fp8": seqs["fp8"]})
    assert r32["fp8"] >= FP8_AGREE_F32_1B, r32
    assert r16["fp8"] >= FP8_AGREE_BF16_1B, r16


def test_fp8_quality_gate_gar8b():
    """Full-depth GAR-8B (head_dim 128), 16 distinct regions x 32 steps: top-1 agreement of the fp8 cache with the f32 path and
    with the bf16 cache, teacher-forced on the f32 path's tokens."""
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_8b()
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=8)
    R, NT = 16, 32
    ss = [_sample(cfg, proc, i, 1024, 1024, dtype=torch.float32) for i in range(R)]
    batch = _batch(ss)
    m32 = GARModel(cfg, W, torch.float32)
    seq32 = m32.generate(**batch, max_new_tokens=NT).sequences.clone()
    del m32
    torch.cuda.empty_cache()
    seqs = _forced_runs(cfg, W, batch, seq32, NT)
    r32 = _agreement("GAR-8B 16 regions x 32 steps vs f32", seq32, seqs)
    r16 = _agreement("GAR-8B 16 regions x 32 steps vs bf16 cache", seqs["bf16"], {"fp8": seqs["fp8"]})
    assert r32["fp8"] >= FP8_AGREE_F32_8B, r32
    assert r16["fp8"] >= FP8_AGREE_BF16_8B, r16
