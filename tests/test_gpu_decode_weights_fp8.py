"""GPU (-m gpu): the opt-in FP8 (OCP e4m3fn) weights of the decode GEMVs — GARModel(decode_weight_dtype="fp8").

Numerics restated here (include/gar_hip.h, FP8 weights): a weight row w is stored as
    amax = max|w|, inv = 448 / amax, q = e4m3(RNE(w * inv)), scale = amax / 448     (inv not finite: q = 0, scale = 0)
and the GEMV computes C[m][n] = epilogue(rstd_m * scale_n * sum_k x[m][k] q[n][k]) with f32 accumulation."""

import gc

import pytest
import torch

# GEMV tolerance: f32 summation in another order (K * 2^-24 of sum |x q| per element, a bound) plus one rounding of the output type
# (tests/gemv_ref.py: the restatement shared with the 16-bit GEMVs' tests/test_gpu_decode_gemv.py)
from gemv_ref import OUT_EPS, gemv_ref

pytestmark = pytest.mark.gpu

SHAPES = {   # (hidden, intermediate, qkv rows, vocab) of the two Llama configurations
    "gar_1b": (2048, 8192, (32 + 2 * 8) * 64, 128262),
    "gar_8b": (4096, 14336, (32 + 2 * 8) * 128, 128262),
}
MS = (1, 8, 9, 16, 17, 32, 33, 64)
LEFT_PAD_REL_L2 = 5e-2      # teacher-forced logits of a left-padded batch row vs the same prompt alone (same fp8-weight model)
TIE_MARGIN = 0.025          # top-1 margin (in logit standard deviations) below which a batcher row may part from its single run
                            # (measured partings: 0 — exact ties of the bf16 logits — and at most 0.0117)


def _quant_ref(w: torch.Tensor):
    """torch restatement of gar_weight_quantize_fp8 on the CPU (correctly rounded f32 divisions) -> (uint8 [N, K], f32 [N])"""
    wf = w.float().cpu()
    amax = wf.abs().amax(-1, keepdim=True)
    inv = torch.tensor(448.0, dtype=torch.float32) / amax
    q = (wf * inv).to(torch.float8_e4m3fn).view(torch.uint8)
    zero = ~(inv < float("inf"))
    q = torch.where(zero, torch.zeros_like(q), q)
    scale = torch.where(zero, torch.zeros_like(amax), amax / 448.0)
    return q, scale.squeeze(-1)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [64, 2048, 8192, 14336])
def test_weight_quantize_matches_torch_restatement(dt, K):
    from gar_amd import ops
    g = torch.Generator().manual_seed(K)
    N = 48
    w = torch.randn(N, K, generator=g) * torch.logspace(-3, 1, N)[:, None]
    w[3] = 0                                                              # a zero row: zeros, scale 0
    w[5, 1::2] = -0.0
    if dt == torch.bfloat16:
        w[7] = torch.randn(K, generator=g) * 1e-38                       # amax < 448 / FLT_MAX: inv overflows -> zeros, not NaN
        w[8] = torch.randn(K, generator=g) * 1e30
        w[9] = 0
        w[9, 0] = 3e-36                                                  # just inside the range
    else:
        w[7] = torch.randn(K, generator=g) * 6e3
        w[8] = torch.randn(K, generator=g) * 1e-5
    w[10] = w[10] * torch.logspace(-12 if dt == torch.bfloat16 else -5, 2, K)   # small elements go subnormal / to zero in e4m3
    w = w.to(dt)
    big = torch.zeros(N, K + 64, dtype=dt, device="cuda")               # row-strided source
    big[:, :K] = w.cuda()
    q, s = ops.weight_quantize_fp8(big[:, :K])
    torch.cuda.synchronize()
    qr, sr = _quant_ref(w)
    assert torch.equal(q.cpu(), qr), (q.cpu() != qr).nonzero()[:5]
    assert torch.equal(s.cpu(), sr)
    assert float(s[3]) == 0 and int(q[3].max()) == 0
    if dt == torch.bfloat16:
        assert float(s[7]) == 0 and int(q[7].max()) == 0 and float(s[9]) > 0


@pytest.fixture(scope="module")
def weights():
    """per configuration, GEMV and type: (16-bit weight [N, K], its e4m3 bytes, scales) — built once"""
    from gar_amd import ops
    cache = {}

    def get(cfg, name, dt=torch.bfloat16):
        key = (cfg, name, dt)
        if key not in cache:
            C, F, Nq, V = SHAPES[cfg]
            N, K = {"qkv": (Nq, C), "o": (C, C), "gu": (2 * F, C), "down": (C, F), "lm_head": (V, C)}[name]
            g = torch.Generator(device="cuda").manual_seed(len(cfg) * 1000 + len(name) * 10 + (dt == torch.float16))
            w = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(dt)
            q, s = ops.weight_quantize_fp8(w)
            cache[key] = (w, q, s)
        return cache[key]
    return get


def _ref(x, q, s, epi, res=None, norm_w=None, folded=False, eps=1e-5, dt=torch.bfloat16):
    """f64 restatement of gar_gemm_w8 -> (reference, bound on |kernel - reference|)"""
    return gemv_ref(x, (q, s), epi, res, norm_w, folded, eps, dt)


def _case(weights, cfg, name, M, split=1, dt=torch.bfloat16, lda=0):
    from gar_amd import hip, ops
    w, q, s = weights(cfg, name, dt)
    N, K = q.shape
    g = torch.Generator(device="cuda").manual_seed(M * 131 + len(name))
    if lda:         # the last activation row beyond 2 GiB: the per-lane fragment path (buffer descriptors take 32-bit offsets)
        store = torch.zeros((M - 1) * lda + K, dtype=dt, device="cuda")
        x = store.as_strided((M, K), (lda, 1))
        x.copy_(torch.randn(M, K, generator=g, device="cuda").to(dt))
    else:
        x = torch.randn(M, K, generator=g, device="cuda").to(dt)
    kw, epi, res, norm_w, folded = {}, hip.EPI_NONE, None, None, False
    if name in ("qkv", "gu"):
        folded = True
        kw = dict(norm_folded=True, norm_eps=1e-5)
    if name == "gu":
        epi = hip.EPI_SWIGLU
    if name in ("o", "down") and split == 1:
        epi = hip.EPI_RES
        res = torch.randn(M, N, generator=g, device="cuda").to(dt)
        kw = dict(residual=res)
    if name == "lm_head" and M <= 16:
        norm_w = (1 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(dt)
        kw = dict(norm_w=norm_w, norm_eps=1e-5)
    if split > 1:
        part = torch.full((split, M, N), float("nan"), device="cuda")
        ops.gemm(x, q, None, partial=part, w_scale=s)
        torch.cuda.synchronize()
        ks = K // split
        for j in range(split):        # every slice before the reduce (f32: no output rounding)
            rj, tj = _ref(x[:, j * ks:(j + 1) * ks], q[:, j * ks:(j + 1) * ks], s, hip.EPI_NONE, dt=dt)
            tj = tj - rj.abs() * OUT_EPS[dt]
            bad = ~((part[j].double() - rj).abs() <= tj)              # a NaN (an element never stored) is out of bound too
            assert not bad.any(), (cfg, name, M, split, j, int(bad.sum()))
        return
    ref, tol = _ref(x, q, s, epi, res, norm_w, folded, dt=dt)
    out = torch.full((M, N // 2 if epi == hip.EPI_SWIGLU else N), float("nan"), dtype=dt, device="cuda")
    ops.gemm(x, q, out, epi, w_scale=s, **kw)
    torch.cuda.synchronize()
    bad = ~((out.double() - ref).abs() <= tol)
    assert not bad.any(), (cfg, name, M, int(bad.sum()), float(((out.double() - ref).abs() / tol).max()))


@pytest.mark.parametrize("cfg", ["gar_1b", "gar_8b"])
@pytest.mark.parametrize("name", ["qkv", "o", "gu", "down", "lm_head"])
def test_gemm_w8_matches_f64_restatement(weights, cfg, name):
    """every M of the decode step: 8-row half tiles and the DEEP ring (o / down at N = 2048, M <= 16), MT 1 / 2 / 4, NT 1 / 2 / 4,
    NORM 0 / 1 (lm_head at M <= 16) / 2 (qkv, gate/up), EPI NONE / RES / SWIGLU"""
    for M in MS:
        _case(weights, cfg, name, M)


@pytest.mark.parametrize("cfg,split", [("gar_1b", 4), ("gar_8b", 2), ("gar_1b", 2), ("gar_8b", 4)])
def test_gemm_w8_split_k_partials(weights, cfg, split):
    for M in MS:
        _case(weights, cfg, "down", M, split=split)


@pytest.mark.parametrize("name,M", [("o", 2), ("lm_head", 3), ("gu", 33), ("qkv", 20)])
def test_gemm_w8_per_lane_fragment_path(weights, name, M):
    """the per-lane fragment loads: half tile, NORM 1, NT 4 with NORM 2, MT 2 with NORM 2"""
    lda = ((2 ** 30) // (M - 1)) // 64 * 64 + 128
    _case(weights, "gar_1b", name, M, lda=lda)


@pytest.mark.parametrize("name", ["qkv", "o", "gu", "down", "lm_head"])
def test_gemm_w8_fp16_twin(weights, name):
    for M in (1, 9, 16, 33, 64):
        _case(weights, "gar_1b", name, M, dt=torch.float16)
    if name == "down":
        _case(weights, "gar_1b", "down", 24, split=4, dt=torch.float16)


def test_gemm_w8_argument_checks(weights):
    from gar_amd import hip, ops
    w, q, s = weights("gar_1b", "o")
    x = torch.zeros(65, 2048, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(65, 2048, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(hip.GarError, match="gemm_w8.*M <= 64"):
        ops.gemm(x, q, out, w_scale=s)
    with pytest.raises(hip.GarError, match="gemm_w8.*aligned"):
        ops.gemm(x[:4], q.view(-1)[8:8 + 2047 * 2048].view(2047, 2048), out[:4, :2047], w_scale=s[:2047])
    with pytest.raises(hip.GarError, match="gemm_w8.*epilogue"):
        ops.gemm(x[:4], q, out[:4], hip.EPI_BIAS, bias=torch.zeros(2048, dtype=torch.bfloat16, device="cuda"), w_scale=s)


# ---- the model ------------------------------------------------------------------------------------------------------------------
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


def _identities(m16, m8, b, n):
    """prefill logits and the first token bit-identical to the 16-bit model; graph == eager; seeded sampling reproducible; the
    decode steps' logits (teacher-forced on the 16-bit model's tokens) differ from the 16-bit model's, within a bound"""
    r16 = m16.generate(**b, max_new_tokens=n, return_logits=True)
    r8 = m8.generate(**b, max_new_tokens=n, return_logits=True)
    assert torch.equal(r8.logits[:, 0], r16.logits[:, 0]) and torch.equal(r8.sequences[:, 0], r16.sequences[:, 0])
    e8 = m8.generate(**b, max_new_tokens=n, return_logits=True, use_graph=False)
    assert torch.equal(e8.logits, r8.logits) and torch.equal(e8.sequences, r8.sequences)
    s1 = m8.generate(**b, max_new_tokens=n, do_sample=True, temperature=0.9, top_k=20, seed=11).sequences
    s2 = m8.generate(**b, max_new_tokens=n, do_sample=True, temperature=0.9, top_k=20, seed=11).sequences
    assert torch.equal(s1, s2)
    t8 = m8.generate(**b, max_new_tokens=n, return_logits=True, forced_tokens=r16.sequences)
    assert not torch.equal(t8.logits[:, 1:], r16.logits[:, 1:])
    for j in range(1, n):
        err = float((t8.logits[:, j].float() - r16.logits[:, j].float()).norm() / r16.logits[:, j].float().norm())
        print(f"step {j}: fp8 vs 16-bit decode weights, teacher-forced logits rel-L2 {err:.3e}")
        assert err < 0.2, (j, err)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kv", [None, "fp8"])
def test_fp8_weights_end_to_end_tiny(tiny, dt, kv):
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    b = _batch([_sample(cfg, proc, i, dtype=dt) for i in (3, 4)])
    m16 = GARModel(cfg, W, dt, kv_cache_dtype=kv)
    m8 = GARModel(cfg, W, dt, kv_cache_dtype=kv, decode_weight_dtype="fp8")
    assert m8.decode_weight_dtype == "fp8" and m16.decode_weight_fp8_bytes() == 0
    assert m8.weight_arena_bytes() == m16.weight_arena_bytes() and m8.decode_weight_fp8_bytes() > 0
    _identities(m16, m8, b, 10)


def test_fp8_weights_gar1b_dims():
    """GAR-1B dims (head_dim 64, GQA 4, vocab 128262), two Llama layers, batch 1 (the DEEP ring, the lm_head norm prologue) and
    batch 20 (two row tiles, split-K down): the identities of the tiny model, with and without the fp8 KV cache"""
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b(**{"vision.depth": 1, "text.num_hidden_layers": 2})
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=4)
    one = _sample(cfg, proc, 3, 512, 512)
    many = _batch([_sample(cfg, proc, 40 + i, 512, 512) for i in range(20)])
    C, F, Nq, V = SHAPES["gar_1b"]
    for kv in (None, "fp8"):
        m16 = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype=kv)
        m8 = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype=kv, decode_weight_dtype="fp8")
        rows = Nq + C + 2 * F + C
        assert m8.decode_weight_fp8_bytes() == 2 * (Nq * C + C * C + 2 * F * C + C * F) + V * C + 4 * (2 * rows + V)
        _identities(m16, m8, one, 6)
        _identities(m16, m8, many, 4)
        del m16, m8
        gc.collect()            # their captured decode graphs are destroyed here, not inside the next model's capture
        torch.cuda.empty_cache()


def test_fp8_weights_refuse_more_than_64_rows(tiny):
    from gar_amd import hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    m8 = GARModel(cfg, W, torch.bfloat16, decode_weight_dtype="fp8")
    b = _batch([_sample(cfg, proc, 1)] * 65)
    with pytest.raises(hip.GarError, match="at most 64 rows"):
        m8.generate(**b, max_new_tokens=2)
    with pytest.raises(hip.GarError, match="at most 64 rows"):
        ContinuousBatcher(m8, slots=65)


def test_fp8_weights_left_padded_batch_equals_singles(tiny):
    """a batch of prompts of different lengths (left-padded) against each prompt alone, both on the fp8-weight model: the same
    tokens, and teacher-forced on the single runs' tokens, every decode step's logits close to the single run's (the per-row GEMV
    is the same kernel at M = 1 and 2; the padded rows sit at other cache rows, so only the attention's order of sums differs)"""
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    m = GARModel(cfg, W, torch.bfloat16, decode_weight_dtype="fp8")
    ss = [_sample(cfg, proc, 30), _sample(cfg, proc, 31, multi=True)]
    n = 8
    one = [m.generate(**s, max_new_tokens=n, return_logits=True) for s in ss]
    S = max(int(s["input_ids"].shape[1]) for s in ss)
    ids = torch.zeros(2, S, dtype=torch.int64)
    mask = torch.zeros(2, S, dtype=torch.int64)
    for i, s in enumerate(ss):
        L = int(s["input_ids"].shape[1])
        ids[i, S - L:] = s["input_ids"][0]
        mask[i, S - L:] = 1
    b = dict(pixel_values=torch.cat([s["pixel_values"] for s in ss]),
             global_mask_values=torch.cat([s["global_mask_values"] for s in ss]), bboxes=[x for s in ss for x in s["bboxes"]],
             aspect_ratios=torch.cat([s["aspect_ratios"] for s in ss]), input_ids=ids, attention_mask=mask)
    out = m.generate(**b, max_new_tokens=n).sequences.cpu()
    forced = torch.cat([o.sequences for o in one]).cuda()
    tf = m.generate(**b, max_new_tokens=n, return_logits=True, forced_tokens=forced)
    for i in range(2):
        print(f"row {i}: batch {out[i].tolist()} alone {one[i].sequences[0].tolist()}")
        assert torch.equal(out[i], one[i].sequences[0].cpu()), i
        for j in range(n):
            a, r = tf.logits[i, j].float(), one[i].logits[0, j].float()
            err = float((a - r).norm() / r.norm())
            print(f"row {i} step {j}: batch vs alone, teacher-forced logits rel-L2 {err:.3e}")
            assert err < LEFT_PAD_REL_L2, (i, j, err)


def _margin(logits_row):
    """top-1 minus top-2 logit over the logits' standard deviation: how near a tie the step's choice is"""
    t = logits_row.float().topk(2).values
    return float((t[0] - t[1]) / logits_row.float().std())


def test_fp8_weights_continuous_batcher_parts_only_at_near_ties(tiny):
    """a ContinuousBatcher on the fp8-weight model against that model's single-region generate(), 16 regions. A row's prompt is
    prefilled in a group whose make-up depends on admission timing and it decodes at other cache rows, so its 16-bit K / V and
    its attention sums differ in the last bits from the single run's; the GEMV forms per row are the same. A region may therefore
    part from its single run only at a step whose single-run choice is a near-tie: every parting step's top-1 margin is below
    TIE_MARGIN (printed with the 16-bit-weight model's count for comparison)."""
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    NT, R = 24, 16
    samples = [_sample(cfg, proc, 200 + i, multi=(i % 3 == 1)) for i in range(R)]
    for dw in (None, "fp8"):
        m = GARModel(cfg, W, torch.bfloat16, decode_weight_dtype=dw)
        runs = [m.generate(**s, max_new_tokens=NT, return_logits=True) for s in samples]
        exp = [r.sequences[0].cpu().tolist() for r in runs]
        cb = ContinuousBatcher(m, slots=4, max_new_tokens=NT, poll_every=2, admit_min=1, smax_multiple=64)
        tickets = [cb.submit(s) for s in samples]
        res = cb.flush()
        parts = []
        for k, (t, e) in enumerate(zip(tickets, exp)):
            j = next((j for j, (a, c) in enumerate(zip(res[t], e)) if a != c), None)
            if j is not None:
                parts.append((k, j, _margin(runs[k].logits[0, j])))
        agree = R - len(parts)
        print(f"continuous, decode weights {dw or '16-bit'}: {agree}/{R} regions equal their generate(); partings "
              f"(region, step, top-1 margin) {[(k, j, round(g, 4)) for k, j, g in parts]}")
        if dw == "fp8":
            for k, j, g in parts:
                assert g < TIE_MARGIN, (k, j, g)
        del cb, m
        gc.collect()


def test_fp8_weights_rebuilt_after_broadcast(tiny):
    """the e4m3 copies are derived weights: broadcast_weights rebuilds them in place from the (received) 16-bit weights"""
    from gar_amd.modeling_gar import GARModel
    cfg, W, _ = tiny
    m = GARModel(cfg, W, torch.bfloat16, decode_weight_dtype="fp8")
    o = m.layers[0]["o"]
    q, s = m._w8[o.data_ptr()]
    q0, s0, ptr0 = q.clone(), s.clone(), q.data_ptr()
    o.mul_(2)                                  # what an exchange could bring: other 16-bit weights in the arena
    m.broadcast_weights()
    q, s = m._w8[o.data_ptr()]
    assert q.data_ptr() == ptr0 and torch.equal(q, q0) and torch.equal(s, 2 * s0)


# ---- quality gate (DESIGN.md 7.2 holds the table): teacher-forced top-1 agreement of the fp8 decode weights, synthetic weights.
# Floors = measured - 3 sigma of a binomial with the test's own n, frozen like tests/test_gpu_kv_fp8.py's.
W8_AGREE_F32_1B = 0.638      # fp8 weights vs the f32 path, GAR-1B B = 64 x 64 steps (n = 4096): measured 0.6609, sigma 0.0074
W8_AGREE_BF16_1B = 0.644     # fp8 weights vs the bf16 model, same steps: measured 0.6665, sigma 0.0074
W8_AGREE_F32_8B = 0.439      # fp8 weights vs the f32 path, GAR-8B 16 regions x 32 steps (n = 512): measured 0.5059, sigma 0.0221
W8_AGREE_BF16_8B = 0.478     # fp8 weights vs the bf16 model, same steps: measured 0.5449, sigma 0.0220


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
    """the bf16 model and the fp8-weight model, each teacher-forced on the f32 path's tokens: their top-1 choices at every step"""
    from gar_amd.modeling_gar import GARModel
    bb = {k: (v.to(torch.bfloat16) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    seqs = {}
    for name, dw in (("bf16", None), ("fp8", "fp8")):
        m = GARModel(cfg, W, torch.bfloat16, decode_weight_dtype=dw)
        seqs[name] = m.generate(**bb, max_new_tokens=NT, forced_tokens=seq32).sequences.clone()
        del m
        gc.collect()
        torch.cuda.empty_cache()
    return seqs


def test_fp8_weights_quality_gate_gar1b_bench_configuration():
    """full-depth GAR-1B, B = 64 distinct regions, 64 steps: top-1 agreement of the fp8 decode weights with the f32 path and with
    the bf16 model, teacher-forced on the f32 path's tokens"""
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
    gc.collect()
    torch.cuda.empty_cache()
    seqs = _forced_runs(cfg, W, batch, seq32, NT)
    r32 = _agreement("GAR-1B B = 64 x 64 steps vs f32", seq32, seqs)
    r16 = _agreement("GAR-1B B = 64 x 64 steps vs bf16 weights", seqs["bf16"], {"fp8": seqs["fp8"]})
    assert r32["fp8"] >= W8_AGREE_F32_1B, r32
    assert r16["fp8"] >= W8_AGREE_BF16_1B, r16


def test_fp8_weights_quality_gate_gar8b():
    """full-depth GAR-8B, 16 distinct regions x 32 steps: top-1 agreement of the fp8 decode weights with the f32 path and with the
    bf16 model, teacher-forced on the f32 path's tokens"""
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_8b()
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=8)
    R, NT = 16, 32
    batch = _batch([_sample(cfg, proc, i, 1024, 1024, dtype=torch.float32) for i in range(R)])
    m32 = GARModel(cfg, W, torch.float32)
    seq32 = m32.generate(**batch, max_new_tokens=NT).sequences.clone()
    del m32
    gc.collect()
    torch.cuda.empty_cache()
    seqs = _forced_runs(cfg, W, batch, seq32, NT)
    r32 = _agreement("GAR-8B 16 regions x 32 steps vs f32", seq32, seqs)
    r16 = _agreement("GAR-8B 16 regions x 32 steps vs bf16 weights", seqs["bf16"], {"fp8": seqs["fp8"]})
    assert r32["fp8"] >= W8_AGREE_F32_8B, r32
    assert r16["fp8"] >= W8_AGREE_BF16_8B, r16
