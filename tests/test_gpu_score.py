"""GPU (-m gpu): teacher-forced caption scoring — GARModel.forward(mode="loss") / score() and the kernels under them
(gar_gather_rmsnorm, the fused lm_head + cross-entropy tile GEMM gar_lm_head_xent, gar_xent_combine) against restatements:
f64 torch for the kernels, the CPU oracle (oracle/gar_oracle.py) with HF's causal-LM loss restated for the model."""
import pytest
import torch

from parity_util import F32_LOGIT_TOL      # 2e-4 * max|logit|: the f32 path's logit bound against the oracle

pytestmark = pytest.mark.gpu

# f32 scoring against the oracle: a log-probability is a difference of two logit-sized terms (target, log-sum-exp), each
# within the f32 logit bound -> 2 x F32_LOGIT_TOL x max|logit|
F32_LP_TOL = 2 * F32_LOGIT_TOL
# kernels against the f64 restatement (which rounds every logit to the model dtype): f32 summation order, plus — 16-bit only —
# a logit whose f32 accumulation sits next to a rounding point may round one ulp away from the f64 product's rounding. One
# such flip moves the target term or the log-sum-exp by at most one ulp of the largest |logit|: bound 2 ulp(max|logit|).
KERNEL_F32_TOL = 2e-5


def _ulp16(dt, x):
    return float(x) * (2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10)


# ---- kernels ---------------------------------------------------------------------------------------------------------
def _head(dt, A, W, tg, S):
    """what GARModel._score_rows runs on normed rows A: the fused head when it takes R, else 64-row dense chunks"""
    from gar_amd import ops
    R, C = A.shape
    V = W.shape[0]
    dest = torch.arange(R, dtype=torch.int32, device=A.device)
    out = torch.zeros(R + S, dtype=torch.float32, device=A.device)
    sm = torch.zeros((R + S) // S + 1, dtype=torch.float32, device=A.device)
    n = torch.zeros_like(sm, dtype=torch.int32)
    flags = torch.zeros(1, dtype=torch.int32, device=A.device)
    fused = ops.lm_head_xent_takes(dt, R, V, C)
    if fused:
        part = torch.full((R * ops.lm_head_xent_strips(V) * 2,), float("nan"), dtype=torch.float32, device=A.device)
        tl = torch.full((R,), float("nan"), dtype=torch.float32, device=A.device)
        ops.lm_head_xent(A, W, tg, part, tl)
        ops.xent_combine(tg, dest, S, out, sm, n, V, partials=part, target_logit=tl, flags=flags)
    else:
        lg = torch.empty((64, (V + 63) // 64 * 64), dtype=dt, device=A.device)
        for r0 in range(0, R, 64):
            r1 = min(R, r0 + 64)
            ops.gemm(A[r0:r1], W, lg[:r1 - r0])
            ops.xent_combine(tg[r0:r1], dest[r0:r1], S, out, sm, n, V, logits=lg[:r1 - r0], flags=flags)
    torch.cuda.synchronize()
    return fused, out[:R], sm, n, int(flags.item())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [37, 512, 128262])
def test_fused_head_and_combine_against_f64(dt, V):
    """every row's log-probability, the per-row sums and counts, the ignored rows (-100, all-ignored groups) and the
    label-range flag, at R = 1, 63, 64, 65, 300, 4097 (the fused head takes R > 64 in 16-bit; the rest is the dense form)"""
    from gar_amd import hip
    hip.require_device(0)
    C, S = 256, 7
    g = torch.Generator().manual_seed(V)
    W = (torch.randn(V, C, generator=g) * (3.0 / C ** 0.5)).to("cuda").to(dt)
    for R in (1, 63, 64, 65, 300, 4097):
        A = torch.randn(R, C, generator=g).to("cuda").to(dt)
        tg = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
        tg[::5] = V - 1                                   # the V tail (128262 = 501 x 256 + 6)
        tg[1::11] = V - 3 if V > 3 else 0
        if R >= 14:
            tg[7:14] = -100                               # a whole group of S = 7 rows ignored
        if R >= 40:
            tg[30], tg[31] = V, -5                       # out of range: ignored, flagged
        tg = tg.to("cuda")
        fused, lp, sm, n, flags = _head(dt, A, W, tg, S)
        assert fused == (dt != torch.float32 and R > 64), (dt, R)
        # f64 restatement, every logit rounded to the model dtype
        x = A.double() @ W.double().t()
        if dt != torch.float32:
            x = x.to(dt).double()
        t64 = tg.long()
        ok = (t64 >= 0) & (t64 < V)
        ref = torch.zeros(R, dtype=torch.float64, device="cuda")
        lse = torch.logsumexp(x, 1)
        ref[ok] = x[ok].gather(1, t64[ok][:, None])[:, 0] - lse[ok]
        err = (lp.double() - ref).abs()
        tol = KERNEL_F32_TOL * max(1.0, float(x.abs().max())) if dt == torch.float32 else \
            2 * _ulp16(dt, x.abs().max()) + KERNEL_F32_TOL * float(x.abs().max())
        assert float(err.max()) <= tol, (dt, V, R, float(err.max()), tol)
        assert float(err.median()) <= KERNEL_F32_TOL * max(1.0, float(x.abs().max())), (dt, V, R)
        assert torch.all(lp[~ok] == 0)
        grp = torch.arange(R, device="cuda") // S
        ns = torch.zeros_like(n).index_add_(0, grp[ok], torch.ones_like(grp[ok], dtype=torch.int32))
        assert torch.equal(n, ns)
        ss = torch.zeros(sm.numel(), dtype=torch.float64, device="cuda").index_add_(0, grp[ok], ref[ok])
        assert float((sm.double() - ss).abs().max()) <= tol * S
        assert flags == (32 if R >= 40 else 0), (R, flags)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,D", [(300, 128), (600, 2048), (5000, 2048), (70, 4096)])
def test_gather_rmsnorm_bitwise(dt, M, D):
    """gar_gather_rmsnorm == gar_rmsnorm on the gathered rows, bit for bit (both gar_rmsnorm kernels: M >= 4096 takes the
    multi-row one in 16-bit); an index outside [0, M) gives zeros"""
    from gar_amd import hip, ops
    hip.require_device(0)
    g = torch.Generator().manual_seed(M + D)
    x = (torch.randn(M, D, generator=g) * 3).to("cuda").to(dt)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to("cuda").to(dt)
    rows = torch.randint(0, M, (M,), generator=g, dtype=torch.int32).to("cuda")
    y = torch.empty(M, D, dtype=dt, device="cuda")
    ops.gather_rmsnorm(x, rows, w, 1e-5, y)
    ref = ops.rmsnorm(x[rows.long()].contiguous(), w, 1e-5, out=torch.empty_like(y))
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16 if dt != torch.float32 else torch.int32),
                       ref.view(torch.int16 if dt != torch.float32 else torch.int32))
    bad = torch.tensor([0, M, -1], dtype=torch.int32, device="cuda")
    y3 = torch.full((3, D), 7.0, dtype=dt, device="cuda")
    ops.gather_rmsnorm(x, bad, w, 1e-5, y3)
    ref0 = ops.rmsnorm(x[:1].contiguous(), w, 1e-5, out=torch.empty(1, D, dtype=dt, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(y3[:1], ref0) and not y3[1:].any()


# ---- end to end --------------------------------------------------------------------------------------------------------
def _sample(cfg, proc, i=0, w=200, h=160, multi=False):
    from gar_amd.eval_dataset import MultiRegionDataset, SingleRegionCaptionDataset
    from gar_amd.synthetic import synthetic_disjoint_masks, synthetic_image, synthetic_mask
    img = synthetic_image(i, w, h)
    if multi:
        masks = synthetic_disjoint_masks(i, 4, w, h)
        qs = "Relate <Prompt0>, <Prompt1>, <Prompt2> and <Prompt3>."
        return MultiRegionDataset(img, masks, qs, proc, data_dtype=torch.float32, device="cpu")[0]
    return SingleRegionCaptionDataset(img, synthetic_mask(i, w, h), proc, data_dtype=torch.float32, device="cpu")[0]


def _oracle_logprobs(W, cfg, s, labels):
    """oracle: prompt embeddings + RoI replay, Llama forward with the final norm, lm_head; token log-probabilities and HF's
    loss restated (labels in replayed spans -> -100, shift by one, mean over valid tokens)"""
    from gar_amd.modeling_gar import causal_lm_loss, score_targets
    from oracle import gar_oracle as O
    t = cfg.mllm_config.text_config
    emb = O.build_inputs_embeds(W, cfg, s["pixel_values"].float(), s["global_mask_values"].float(), s["aspect_ratios"],
                                s["bboxes"], s["input_ids"])
    h = O.llama_forward(emb, W, t, O.KVCache(t.num_hidden_layers))
    logits = torch.nn.functional.linear(h, O.lm_head_weight(W, t))
    tgt = score_targets(s["input_ids"], labels, cfg.crop_tokens_ids)                         # [B, S - 1]
    lab = torch.cat([torch.full_like(tgt[:, :1], -100), tgt], 1)
    lp = torch.log_softmax(logits.double(), -1)[:, :-1]
    ok = tgt != -100
    tok = torch.zeros(lab.shape, dtype=torch.float64)
    tok[:, 1:][ok] = lp[ok].gather(-1, tgt[ok][:, None])[:, 0]
    return tok, causal_lm_loss(logits, lab), float(logits.abs().max())


def _data(s, labels):
    return dict(pixel_values=s["pixel_values"], global_mask_values=s["global_mask_values"], input_ids=s["input_ids"],
                aspect_ratios=s["aspect_ratios"], bboxes=s["bboxes"], labels=labels)


def _caption(cfg, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    V = cfg.mllm_config.text_config.vocab_size
    special = set(cfg.crop_tokens_ids) | {cfg.mllm_config.image_token_id}      # a caption never holds these
    return [3 if x in special else x for x in torch.randint(3, min(V - 1, 100000), (n,), generator=g).tolist()]


@pytest.fixture(scope="module")
def tiny():
    from gar_amd import GARConfig
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.tiny()
    return cfg, synthetic_weights(cfg), GARProcessor.from_config(cfg, max_num_tiles=4)


def _check_against_oracle(model, cfg, W, s, labels, what):
    tok, loss, mx = _oracle_logprobs(W, cfg, s, labels)
    out = model.score(s["pixel_values"], s["global_mask_values"], s["aspect_ratios"], s["bboxes"], s["input_ids"], labels)
    fl = model.forward(_data(s, labels))["loss"]
    torch.cuda.synchronize()
    err = float((out.token_logprobs.cpu().double() - tok).abs().max())
    assert err <= F32_LP_TOL * mx, (what, err, F32_LP_TOL * mx)
    assert abs(float(fl) - float(loss)) <= F32_LP_TOL * mx, (what, float(fl), float(loss))
    assert int(out.n_tokens.sum()) == int((tok != 0).sum())
    return err / mx


def test_f32_score_and_loss_tiny_against_oracle(tiny):
    """caption labels (append_target) and full-sequence labels (input_ids: the crop-token span must be masked)"""
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import append_target
    cfg, W, proc = tiny
    model = GARModel(cfg, W, torch.float32, "cuda:0")
    s = append_target(_sample(cfg, proc, 0), _caption(cfg, 12), eos_token_id=cfg.mllm_config.text_config.vocab_size - 1)
    _check_against_oracle(model, cfg, W, s, s["labels"], "caption")
    _check_against_oracle(model, cfg, W, s, s["input_ids"].clone(), "full sequence")
    with pytest.raises(hip_error()):
        model.forward(_data(s, s["labels"]), mode="predict")


def hip_error():
    from gar_amd.hip import GarError
    return GarError


def test_f32_score_gar1b_dims_one_and_four_masks():
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor, append_target
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b(**{"vision.depth": 1, "text.num_hidden_layers": 2})
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=2)
    model = GARModel(cfg, W, torch.float32, "cuda:0")
    for multi in (False, True):
        s = append_target(_sample(cfg, proc, 3, 300, 220, multi=multi), _caption(cfg, 16, 1))
        rel = _check_against_oracle(model, cfg, W, s, s["labels"], f"gar1b multi={multi}")
        print(f"gar1b dims multi={multi}: max |logprob err| / max|logit| = {rel:.3g}")


def test_left_padded_batch_equals_single_rows(tiny):
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import append_target
    cfg, W, proc = tiny
    model = GARModel(cfg, W, torch.float32, "cuda:0")
    ss = [append_target(_sample(cfg, proc, i), _caption(cfg, n, i)) for i, n in ((1, 5), (2, 14))]
    S = max(s["input_ids"].shape[1] for s in ss)
    ids, lab, am = [], [], []
    for s in ss:
        p = S - s["input_ids"].shape[1]
        ids.append(torch.cat([torch.zeros(1, p, dtype=torch.int64), s["input_ids"]], 1))
        lab.append(torch.cat([torch.full((1, p), -100, dtype=torch.int64), s["labels"]], 1))
        am.append(torch.cat([torch.zeros(1, p), torch.ones(1, s["input_ids"].shape[1])], 1))
    pv = torch.cat([s["pixel_values"] for s in ss])
    gm = torch.cat([s["global_mask_values"] for s in ss])
    ar = torch.cat([torch.as_tensor(s["aspect_ratios"]).reshape(1, -1) for s in ss])
    bb = [s["bboxes"][0] for s in ss]
    for validate in (True, False):
        out = model.score(pv, gm, ar, bb, torch.cat(ids), torch.cat(lab), attention_mask=torch.cat(am), validate=validate)
        torch.cuda.synchronize()
        if not validate:
            assert int(out.input_flags.item()) == 0
        for b, s in enumerate(ss):
            one = model.score(s["pixel_values"], s["global_mask_values"], s["aspect_ratios"], s["bboxes"], s["input_ids"],
                              s["labels"])
            n = s["input_ids"].shape[1]
            a, r = out.token_logprobs[b, S - n:].cpu(), one.token_logprobs[0].cpu()
            assert float((a - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max())), (validate, b)
            assert int(out.n_tokens[b]) == int(one.n_tokens[0])
            assert not out.token_logprobs[b, :S - n].any()


def test_scores_of_a_generate_output_equal_its_logits(tiny):
    """score() of the caption generate() produced == log_softmax of that run's return_logits at the generated tokens"""
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import append_target
    cfg, W, proc = tiny
    model = GARModel(cfg, W, torch.float32, "cuda:0")
    s = _sample(cfg, proc, 4)
    g = model.generate(**s, max_new_tokens=10, return_logits=True)
    seq = g.sequences[0].cpu()
    d = append_target(s, seq)
    out = model.score(d["pixel_values"], d["global_mask_values"], d["aspect_ratios"], d["bboxes"], d["input_ids"], d["labels"])
    torch.cuda.synchronize()
    ref = torch.log_softmax(g.logits[0].double().cpu(), -1).gather(-1, seq[:, None])[:, 0]
    got = out.token_logprobs[0, -len(seq):].double().cpu()
    mx = float(g.logits.abs().max())
    assert float((got - ref).abs().max()) <= F32_LP_TOL * mx, (got, ref)
    assert abs(float(out.sum_logprobs[0]) - float(ref.sum())) <= F32_LP_TOL * mx * len(seq)


def test_label_checks_and_flag(tiny):
    from gar_amd.modeling_gar import INPUT_LABEL_RANGE, GARModel
    from gar_amd.processing import append_target
    cfg, W, proc = tiny
    V = cfg.mllm_config.text_config.vocab_size
    model = GARModel(cfg, W, torch.float32, "cuda:0")
    s = append_target(_sample(cfg, proc, 0), _caption(cfg, 6))
    bad = s["labels"].clone()
    bad[0, -2] = V
    with pytest.raises(ValueError):
        model.score(s["pixel_values"], s["global_mask_values"], s["aspect_ratios"], s["bboxes"], s["input_ids"], bad)
    with pytest.raises(ValueError):
        model.score(s["pixel_values"], s["global_mask_values"], s["aspect_ratios"], s["bboxes"], s["input_ids"], bad[:, 1:])
    out = model.score(s["pixel_values"], s["global_mask_values"], s["aspect_ratios"], s["bboxes"], s["input_ids"], bad,
                      validate=False)
    good = model.score(s["pixel_values"], s["global_mask_values"], s["aspect_ratios"], s["bboxes"], s["input_ids"], s["labels"])
    torch.cuda.synchronize()
    assert int(out.input_flags.item()) == INPUT_LABEL_RANGE
    assert int(out.n_tokens[0]) == int(good.n_tokens[0]) - 1
    none = torch.full_like(s["labels"], -100)
    nl = model.forward(_data(s, none))["loss"]
    assert torch.isnan(nl)


# bf16 / fp16 against the f32 path (same synthetic weights): relative loss error and max per-token error over max|logprob|.
# Both cases score more than 64 rows, so the 16-bit models run the fused head (asserted). Bounds: the measured value (printed;
# MI355X) x 1.5, rounded up. Measured (loss, token): tiny R = 80 bf16 2.3e-4, 4.8e-3; fp16 3.0e-5, 5.7e-4; GAR-1B dims R = 128
# bf16 1.8e-5, 7.3e-3; fp16 8.3e-6, 9.4e-4.
HALF_BOUNDS = {("tiny", torch.bfloat16): (3.5e-4, 7.3e-3), ("tiny", torch.float16): (4.5e-5, 8.6e-4),
               ("gar1b", torch.bfloat16): (2.7e-5, 1.1e-2), ("gar1b", torch.float16): (1.3e-5, 1.5e-3)}


def _batch(ss):
    """left-to-right concatenation of samples with equal prompt shapes (one batch)"""
    cat = lambda k: torch.cat([x[k] for x in ss])
    return dict(pixel_values=cat("pixel_values"), global_mask_values=cat("global_mask_values"),
                aspect_ratios=torch.cat([torch.as_tensor(x["aspect_ratios"]).reshape(1, -1) for x in ss]),
                bboxes=[x["bboxes"][0] for x in ss], input_ids=cat("input_ids"), labels=cat("labels"))


def _score(m, d, dt=torch.float32):
    return m.score(d["pixel_values"].to(dt), d["global_mask_values"].to(dt), d["aspect_ratios"], d["bboxes"], d["input_ids"],
                   d["labels"])


@pytest.mark.parametrize("which", ["tiny", "gar1b"])
def test_half_precision_score_against_f32(which):
    from gar_amd import GARConfig, ops
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor, append_target
    from gar_amd.weights import synthetic_weights
    if which == "tiny":           # one region, an 80-token caption: R = 80
        cfg = GARConfig.tiny()
        proc = GARProcessor.from_config(cfg, max_num_tiles=4)
        d = _batch([append_target(_sample(cfg, proc, 5), _caption(cfg, 80, 5))])
    else:                         # two regions x 64-token captions: R = 128
        cfg = GARConfig.gar_1b(**{"vision.depth": 1, "text.num_hidden_layers": 2})
        proc = GARProcessor.from_config(cfg, max_num_tiles=2)
        s = _sample(cfg, proc, 3, 300, 220)
        d = _batch([append_target(s, _caption(cfg, 64, 3)), append_target(s, _caption(cfg, 64, 4))])
    t = cfg.mllm_config.text_config
    W = synthetic_weights(cfg)
    ref = _score(GARModel(cfg, W, torch.float32, "cuda:0"), d)
    torch.cuda.synchronize()
    R = int(ref.n_tokens.sum())
    for dt in (torch.bfloat16, torch.float16):
        assert ops.lm_head_xent_takes(dt, R, t.vocab_size, t.hidden_size), (which, dt, R)
        m = GARModel(cfg, W, dt, "cuda:0")
        out = _score(m, d, dt)
        torch.cuda.synchronize()
        mx = float(ref.token_logprobs.abs().max())
        lerr = abs(float(out.loss) - float(ref.loss)) / abs(float(ref.loss))
        terr = float((out.token_logprobs - ref.token_logprobs).abs().max()) / max(1.0, mx)
        print(f"{which} {dt} R={R}: loss rel err {lerr:.4g}, token err / max|logprob| {terr:.4g}")
        lb, tb = HALF_BOUNDS[(which, dt)]
        assert lerr <= lb and terr <= tb, (which, dt, lerr, terr)
        assert torch.equal(out.n_tokens, ref.n_tokens)


def test_fused_head_chunk_plan_tiny():
    """the fused branch of GARModel._score_rows over several row chunks (XENT_CHUNK_ROWS set low on the instance): 160 rows
    with 80 -> two chunks of 80 on the fused head, the token log-probabilities equal the one-chunk run's bit for bit (a row's
    logits do not depend on the tile it lands in); with 60 -> chunks of 54 / 54 / 52 rows, which the fused head does not take,
    so they run in the dense form (another GEMM kernel: a logit may round one 16-bit ulp apart, so the bound is 2 ulp of the
    largest |log-probability|). Counts exact, sums up to the order of the atomics."""
    from gar_amd import GARConfig, ops
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor, append_target
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.tiny()
    t = cfg.mllm_config.text_config
    proc = GARProcessor.from_config(cfg, max_num_tiles=4)
    s = _sample(cfg, proc, 6)
    d = _batch([append_target(s, _caption(cfg, 80, 7)), append_target(s, _caption(cfg, 80, 8))])
    m = GARModel(cfg, synthetic_weights(cfg), torch.bfloat16, "cuda:0")
    one = _score(m, d, torch.bfloat16)
    torch.cuda.synchronize()
    assert int(one.n_tokens.sum()) == 160 and ops.lm_head_xent_takes(torch.bfloat16, 160, t.vocab_size, t.hidden_size)
    for ch, fused in ((80, True), (60, False)):
        m.XENT_CHUNK_ROWS = ch
        out = _score(m, d, torch.bfloat16)
        torch.cuda.synchronize()
        n = -(-160 // -(-160 // ch))
        assert ops.lm_head_xent_takes(torch.bfloat16, n, t.vocab_size, t.hidden_size) == fused, ch
        if fused:
            assert torch.equal(out.token_logprobs, one.token_logprobs), ch
        bound = 1e-4 * max(1.0, float(one.sum_logprobs.abs().max()))
        if not fused:
            bound = 2 * 2.0 ** -7 * max(1.0, float(one.token_logprobs.abs().max()))
            assert float((out.token_logprobs - one.token_logprobs).abs().max()) <= bound, ch
            bound *= 80                                   # 80 scored tokens per row
        assert torch.equal(out.n_tokens, one.n_tokens)
        assert float((out.sum_logprobs - one.sum_logprobs).abs().max()) <= bound, ch
