"""GPU (-m gpu): generate(beam_search=BeamSearch(...)) — gar_beam_step against tests/beam_search_ref.py bit for
bit, gar_kv_beam_reorder against index_select byte for byte, then GARModel.generate end to end: f32 against the restatement driven
by the model's own teacher-forced replicated logits, 16-bit by teacher-forcing every returned hypothesis through the replicated
16-bit path."""
import itertools

import pytest
import torch

import beam_search_ref as R

pytestmark = pytest.mark.gpu

EARLY = (False, True, "never")
V_K = 37                # vocabulary of the kernel tests
STEPS = 8


@pytest.fixture(scope="module")
def dev():
    from gar_amd import hip
    hip.require_device(0)
    return torch.device("cuda:0")


# ---- gar_beam_step ----------------------------------------------------------------------------------------------------------
def _planes(B, K, M, seed):
    """[STEPS] x (ids int32 [B, K, M], lp f32 [B, K, M]): the M best of random V_K-token distributions, built on the CPU — the
    kernel is driven without gar_topk_lp"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(STEPS):
        ids, lp = R.top_m(torch.randn(B, K, V_K, generator=g) * 2.5, M)
        out.append((ids.to(torch.int32).contiguous(), lp.contiguous()))
    return out


def _device_state(B, K, M, T, beam, max_new, eos, dev):
    from gar_amd import ops
    ref = R.new_state(B, K, T)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)
    bs = dict(B=B, K=K, M=M, T=T, top_ids=z(B * K, M), top_lp=z(B * K, M, dt=torch.float32),
              run_scores=ref["run_scores"].reshape(-1).to(dev), cur_tokens=z(B * K, dt=torch.int64), parent=z(B * K),
              hist=z(2, B * K, T), fin_tokens=z(B * K, T), fin_scores=ref["fin_scores"].reshape(-1).to(dev), fin_len=z(B * K),
              fin_flag=z(B * K), heur=torch.ones(B, dtype=torch.int32, device=dev), done=z(B), done_count=z(1),
              params=torch.tensor(beam.pack(max_new, eos), dtype=torch.int32, device=dev),
              len_pow=torch.tensor(beam.length_powers(T), dtype=torch.float32, device=dev))
    assert bs["params"].numel() == ops.BEAM_PARAM_WORDS
    return ref, bs


def _compare(ref, bs, t, what):
    B, K, T = bs["B"], bs["K"], bs["T"]
    for name in ("run_scores", "cur_tokens", "parent", "fin_scores", "fin_len", "fin_flag"):
        got = bs[name].cpu().view(B, K)
        assert torch.equal(got, ref[name]), (what, t, name, got, ref[name])
    assert torch.equal(bs["fin_tokens"].cpu().view(B, K, T), ref["fin_tokens"]), (what, t, "fin_tokens")
    live = ~ref["done"].bool() | torch.tensor(ref["_just_done"])
    hist = bs["hist"][(t + 1) & 1].cpu().view(B, K, T)[live][:, :, :t + 1]
    assert torch.equal(hist, ref["hist"][live][:, :, :t + 1]), (what, t, "hist")
    assert torch.equal(bs["heur"].cpu(), ref["heur"]) and torch.equal(bs["done"].cpu(), ref["done"]), (what, t, "latches")
    assert int(bs["done_count"].item()) == ref["done_count"], (what, t, "done_count")


def _run(B, K, M, planes, early, lp, eos, dev):
    """STEPS steps of kernel and restatement side by side, all state compared after every step"""
    from gar_amd import BeamSearch, ops
    beam = BeamSearch(K, length_penalty=lp, early_stopping=early)
    T = 16
    ref, bs = _device_state(B, K, M, T, beam, STEPS, eos, dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    what = (B, K, M, early, lp, eos)
    for t, (ids, lpl) in enumerate(planes):
        before = ref["done"].clone()
        R.beam_step_ref(ref, ids, lpl, t, STEPS, early, lp, eos, V_K)
        ref["_just_done"] = (ref["done"] != before).tolist()
        bs["top_ids"].copy_(ids.view(B * K, M))
        bs["top_lp"].copy_(lpl.view(B * K, M))
        step.fill_(t)
        ops.beam_step(bs, step, V_K)
        _compare(ref, bs, t, what)
        if int(ref["done"].sum()) == B:
            break
    assert ref["tied_candidates"] == 0, what        # no two live candidate scores of a prompt were equal
    assert int(ref["done"].sum()) == B, what
    return ref


SHAPES = [(B, K, M) for B in (1, 3) for K in (2, 3, 4, 16) for M in (2 * K, 3 * K) if M <= 32]


@pytest.mark.parametrize("B,K,M", SHAPES)
def test_beam_step_bit_for_bit(dev, B, K, M):
    """every (eos placement) x (stopping mode) x (length penalty): all state equal to the restatement's after every one of 8 steps"""
    planes = _planes(B, K, M, 3 if (B, K) == (3, 16) else 1)             # seeds under which no live candidate scores tie
    free = _run(B, K, M, planes, False, 1.0, [], dev)                    # no eos: runs to the last step, which finishes everything
    assert free["fin_len"].min() == STEPS and bool(free["fin_flag"].all())
    # eos ids by where they fall among prompt 0's candidates in the eos-free run
    probe = R.new_state(B, K, 16)
    cands = []
    for t, (ids, lpl) in enumerate(planes[:3]):
        R.beam_step_ref(probe, ids, lpl, t, STEPS, False, 1.0, [], V_K)
        cands.append(probe["last_tokens"][0].tolist())
    at0 = cands[0][1]                                                   # met at step 0
    inside = cands[2][0]                                                # inside the first K at step 2
    behind = next(tk for tk in cands[2][K:] if tk not in cands[2][:K])  # among K .. M - 1 at step 2
    eos_sets = ([], [at0], [inside], [behind], [inside, behind])
    ends = set()
    for eos, early, lp in itertools.product(eos_sets, EARLY, (0.0, 1.0, 2.0)):
        ref = _run(B, K, M, planes, early, lp, eos, dev)
        ends.update(ref["fin_len"].reshape(-1).tolist())
    assert min(ends) == 1 and max(ends) == STEPS, ends


def test_beam_step_clamps_ids_and_step(dev):
    """ids outside the vocabulary are read as their clamped value and the step as T - 1 at most: nothing outside the prompt's rows
    is touched (guard rows around every buffer keep their bytes)"""
    from gar_amd import BeamSearch, ops
    B, K, M, T = 2, 4, 8, 16
    planes = _planes(B, K, M, 7)
    beam = BeamSearch(K)
    ref, bs = _device_state(B, K, M, T, beam, STEPS, [3], dev)
    ids, lpl = planes[0]
    ids = ids.clone()
    ids[0, 0, 1], ids[1, 0, 2] = -5, 100000
    R.beam_step_ref(ref, ids, lpl, 0, STEPS, False, 1.0, [3], V_K)
    ref["_just_done"] = [False] * B
    bs["top_ids"].copy_(ids.view(B * K, M))
    bs["top_lp"].copy_(lpl.view(B * K, M))
    ops.beam_step(bs, None, V_K)
    _compare(ref, bs, 0, "clamped ids")
    assert int(bs["cur_tokens"].min()) >= 0 and int(bs["cur_tokens"].max()) < V_K
    # a step beyond the capacity writes column T - 1, not behind the rows
    guard = torch.full((3, B * K, T), 77, dtype=torch.int32, device=dev)
    bs["fin_tokens"] = guard[1]
    bs["fin_tokens"].zero_()
    ops.beam_step(bs, torch.tensor([10 ** 6], dtype=torch.int32, device=dev), V_K)
    torch.cuda.synchronize()
    assert bool((guard[0] == 77).all()) and bool((guard[2] == 77).all())


# ---- gar_kv_beam_reorder ----------------------------------------------------------------------------------------------------
def _parents(kind, B, K, g):
    if kind == "identity":
        p = torch.arange(K).repeat(B, 1)
    elif kind == "one":
        p = torch.full((B, K), K - 1)
    elif kind == "cycle":
        p = ((torch.arange(K) + 1) % K).repeat(B, 1)
    else:
        p = torch.randint(0, K, (B, K), generator=g)
    return p.to(torch.int32)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_kv_beam_reorder_against_index_select(dev, dt, hd):
    """every (B, K, s0, t, parents): the caches equal, byte for byte, the copy whose rows were gathered by parent over positions
    s0 .. s0 + t — every other byte (random, so its own sentinel) unchanged"""
    from gar_amd import ops
    L, Hkv, CAP = 2, 2, 128
    it = torch.int16 if dt != torch.float32 else torch.int32
    g = torch.Generator().manual_seed(hd + it.itemsize)
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    s0_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    for B, K, s0 in itertools.product((1, 3), (2, 4, 16), (0, 256)):
        Rr, cap = B * K, s0 + CAP
        info = torch.iinfo(it)
        base = [torch.randint(info.min, info.max, (L, Rr, Hkv, cap, hd), generator=g, dtype=it).to(dev) for _ in range(2)]
        for t, kind in itertools.product((0, 1, 63, 64, 65, 127), ("identity", "one", "cycle", "random")):
            par = _parents(kind, B, K, g)
            src = (torch.arange(B)[:, None] * K + par).reshape(-1).to(dev)
            Kc, Vc = (x.clone().view(dt) for x in base)
            n_dev.fill_(t + 1)
            if s0 and t % 2:                # the device word in place of the argument
                s0_dev.fill_(s0)
                ops.kv_beam_reorder(Kc, Vc, K, n_dev, par.reshape(-1).to(dev), s0=0, s0_dev=s0_dev)
            else:
                ops.kv_beam_reorder(Kc, Vc, K, n_dev, par.reshape(-1).to(dev), s0=s0)
            for got, x in zip((Kc, Vc), base):
                want = x.clone()
                want[:, :, :, s0:s0 + t + 1] = x.index_select(1, src)[:, :, :, s0:s0 + t + 1]
                assert torch.equal(got.view(it), want), (dt, hd, B, K, s0, t, kind)
        # a count beyond the capacity is clamped to it; parents outside 0 .. K - 1 to the nearest sibling
        Kc, Vc = (x.clone().view(dt) for x in base)
        n_dev.fill_(10 ** 6)
        par = torch.full((B, K), 99, dtype=torch.int32)
        par[:, -1] = -4
        ops.kv_beam_reorder(Kc, Vc, K, n_dev, par.reshape(-1).to(dev), s0=s0)
        src = (torch.arange(B)[:, None] * K + par.clamp(0, K - 1)).reshape(-1).to(dev)
        for got, x in zip((Kc, Vc), base):
            want = x.clone()
            want[:, :, :, s0:] = x.index_select(1, src)[:, :, :, s0:]
            assert torch.equal(got.view(it), want), (dt, hd, B, K, s0, "clamped")


# ---- end to end -------------------------------------------------------------------------------------------------------------
NT = 8
MARGIN = 1e-4           # every order the reference decided had at least this gap: the f32 run cannot legitimately differ
HEAD_GAIN, WEIGHT_SEED = 8.0, 1      # measured reference margins with these: 3.8e-4 at the least, K = 2 and K = 4


def _half(batch, dt):
    return {k: (v.to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}


def _teacher_logits(m, batch, K):
    """logits_fn of the restatement: the model's own teacher-forced REPLICATED run — generate(forced_tokens=, return_logits=True)
    on the repeat_interleave'd batch, today's code (the f32 fan-out and replicated paths agree bit for bit)"""
    from test_gpu_fanout import _repeat
    rep = _repeat(batch, K)
    B = batch["input_ids"].shape[0]
    cache = {}

    def fn(hist, t):
        key = (t, hist.numpy().tobytes())
        if key not in cache:
            forced = hist.reshape(B * K, t).to(torch.int64) if t else None
            out = m.generate(**rep, max_new_tokens=t + 1, forced_tokens=forced, return_logits=True)
            cache[key] = out.logits[:, t].float().cpu().view(B, K, -1)
        return cache[key]
    return fn


@pytest.fixture(scope="module")
def tiny_f32(dev):
    from gar_amd.modeling_gar import GARModel
    from test_gpu_fanout import _tiny_setup
    from gar_amd.weights import LM
    cfg, W, batch = _tiny_setup()
    # the synthetic tiny model's distributions are nearly flat (a tied head over 0.03-scale embeddings): candidate scores then lie
    # closer than MARGIN. A larger gain of the final norm scales every logit, which spreads them as a trained head's are
    from gar_amd.weights import synthetic_weights
    W = dict(synthetic_weights(cfg, WEIGHT_SEED))
    W[LM + "norm.weight"] = W[LM + "norm.weight"] * HEAD_GAIN
    m = GARModel(cfg, W, torch.float32)
    return cfg, W, batch, m, {}


def _reference(tiny, K, early, lp, eos, n):
    cfg, W, batch, m, memo = tiny
    key = (K, early, lp, tuple(eos), n)
    if key not in memo:
        fn = memo.setdefault(("fn", K), _teacher_logits(m, batch, K))
        V = cfg.mllm_config.text_config.vocab_size
        memo[key] = R.beam_search_ref(fn, batch["input_ids"].shape[0], K, NT, early, lp, eos, V, n, 1)
    return memo[key]


def _eos_for(tiny, K):
    """an eos id the beams meet: a token the eos-free best hypotheses hold a few steps in"""
    seq, _, _ = _reference(tiny, K, False, 1.0, [], 1)
    return [int(seq[0, 2])], [int(seq[1, 3]), int(seq[2, 1])]


@pytest.mark.parametrize("K", [2, 4])
def test_beam_search_f32_tiny_end_to_end(tiny_f32, K):
    """a ragged left-padded batch of 3, f32 parity mode: sequences equal to the restatement's, scores within 1e-5, with and
    without eos ids, all K hypotheses in descending order, graph against eager, each prompt alone against the batch"""
    from gar_amd import BeamSearch
    cfg, W, batch, m, _ = tiny_f32
    B = 3
    one, two = _eos_for(tiny_f32, K)
    worst = 0.0
    for early, lp, eos, n in ((False, 1.0, [], K), (False, 1.0, one, K), (True, 0.0, two, 1), ("never", 2.0, one, K),
                              (False, 2.0, two, K), (True, 1.0, one, K)):
        seq, sc, st = _reference(tiny_f32, K, early, lp, eos, n)
        print(f"K {K} early {early} lp {lp} eos {eos}: reference min margin {st['min_margin']:.3g}, lengths "
              f"{st['fin_len'][:, :n].reshape(-1).tolist()}")
        assert st["min_margin"] > MARGIN, (K, early, lp, eos, st["min_margin"])
        kw = dict(max_new_tokens=NT, eos_token_id=eos or None, pad_token_id=1, sync_every=4,
                  beam_search=BeamSearch(K, length_penalty=lp, early_stopping=early, num_return_sequences=n))
        out = m.generate(**batch, **kw)
        assert out.sequences.dtype == torch.int64 and tuple(out.sequences_scores.shape) == (B * n,)
        assert out.sequences.cpu().tolist() == seq.tolist(), (K, early, lp, eos)
        err = float((out.sequences_scores.cpu() - sc).abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, (K, early, lp, eos, err)
        sco = out.sequences_scores.cpu().view(B, n)
        assert bool((sco[:, :-1] >= sco[:, 1:]).all())                                      # best first
        if not eos:
            assert tuple(out.sequences.shape) == (B * n, NT)                                # nothing ends before max_new_tokens
        eager = m.generate(**batch, use_graph=False, **kw)
        assert torch.equal(eager.sequences, out.sequences) and torch.equal(eager.sequences_scores, out.sequences_scores)
    print(f"K {K}: worst |score - reference| {worst:.3g}")
    # each prompt alone gives what it gives in the batch
    early, lp, eos, n = False, 1.0, one, K
    seq, sc, st = _reference(tiny_f32, K, early, lp, eos, n)
    samples = _single_prompts()
    for b in range(B):
        alone = m.generate(**samples[b], max_new_tokens=NT, eos_token_id=eos, pad_token_id=1,
                           beam_search=BeamSearch(K, length_penalty=lp, early_stopping=early, num_return_sequences=n))
        rows = seq[b * n:(b + 1) * n]
        width = alone.sequences.shape[1]
        assert alone.sequences.cpu().tolist() == rows[:, :width].tolist() and bool((rows[:, width:] == 1).all()), b
        assert float((alone.sequences_scores.cpu() - sc[b * n:(b + 1) * n]).abs().max()) <= 1e-5


def _single_prompts():
    """the three prompts of _tiny_setup()'s batch, each as a batch of its own"""
    from gar_amd import GARConfig
    from gar_amd.processing import GARProcessor
    from test_gpu_e2e import _left_pad_batch, _lengthen, _sample
    cfg = GARConfig.tiny()
    proc = GARProcessor.from_config(cfg, max_num_tiles=4)
    base = [_sample(cfg, proc, i) for i in (3, 4, 6)]
    ss = [_lengthen(x, e, 300 + i) for i, (x, e) in enumerate(zip(base, (0, 21, 21)))]
    return [_left_pad_batch([s]) for s in ss]


def _scores_from_logits(logits, seq, lens, lp, V):
    """sum over a hypothesis's own tokens of log_softmax(logits)[token], divided by len ** length_penalty"""
    lsm = torch.log_softmax(logits[:, :, :V].float().cpu(), -1)
    tok = lsm.gather(2, seq.cpu()[:, :, None])[:, :, 0]
    keep = torch.arange(seq.shape[1])[None, :] < lens[:, None]
    return (tok * keep).sum(1) / lens.float() ** lp


@pytest.mark.parametrize("which", ["tiny", "gar1b"])
def test_beam_search_half_scores_against_replicated_half(dev, which):
    """bf16 / fp16 over the shared prompt cache: every returned hypothesis, teacher-forced through the REPLICATED 16-bit path,
    has the score the beam search reports. The replicated run's logits are read with return_logits and the log-probabilities of the
    forced tokens formed from them (return_logprobs reports the model's own choice of a step, not the forced token's). Allowance:
    twice the worst difference between the existing num_return_sequences fan-out run and the replicated run on the same tokens.
    Measured on an MI355X."""
    from gar_amd import BeamSearch, GARConfig, ops
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    from test_gpu_e2e import _left_pad_batch, _sample
    from test_gpu_fanout import _repeat, _tiny_setup
    if which == "tiny":
        cfg, W, batch = _tiny_setup()
    else:
        cfg = GARConfig.gar_1b(**{"vision.depth": 1, "text.num_hidden_layers": 2})
        W = synthetic_weights(cfg)
        proc = GARProcessor.from_config(cfg, max_num_tiles=2)
        batch = _left_pad_batch([_sample(cfg, proc, 3, 300, 220), _sample(cfg, proc, 4, 300, 220)])
    V = cfg.mllm_config.text_config.vocab_size
    B, K, lp = batch["input_ids"].shape[0], 4, 1.0
    for dt in (torch.bfloat16, torch.float16):
        m = GARModel(cfg, W, dt)
        hb = _half(batch, dt)
        n0 = ops.FANOUT_LAUNCHES
        free = m.generate(**hb, max_new_tokens=NT, beam_search=BeamSearch(K, num_return_sequences=K))
        assert ops.FANOUT_LAUNCHES > n0, "the shared-prefix kernel did not run"
        eos = [int(free.sequences[0, 3]), int(free.sequences[K, 2])]
        out = m.generate(**hb, max_new_tokens=NT, eos_token_id=eos, pad_token_id=1, sync_every=4,
                         beam_search=BeamSearch(K, length_penalty=lp, num_return_sequences=K))
        seq = out.sequences
        lens = torch.tensor([next((j + 1 for j, tk in enumerate(r) if tk in eos), len(r)) for r in seq.cpu().tolist()])
        assert int(lens.min()) < seq.shape[1] or seq.shape[1] < NT, "no hypothesis met an eos id"
        width = seq.shape[1]
        fan = m.generate(**hb, do_sample=True, num_return_sequences=K, seed=1, max_new_tokens=width, forced_tokens=seq,
                         return_logits=True)
        rep = m.generate(**_repeat(hb, K), do_sample=True, seed=1, max_new_tokens=width, forced_tokens=seq, return_logits=True)
        s_fan, s_rep = (_scores_from_logits(x.logits, seq, lens, lp, V) for x in (fan, rep))
        parent_gap = float((s_fan - s_rep).abs().max())
        err = float((out.sequences_scores.cpu() - s_rep).abs().max())
        print(f"{which} {dt}: |beam score - replicated| {err:.4g}; fan-out vs replicated on the same tokens {parent_gap:.4g} "
              f"(allowance {2 * parent_gap:.4g}); lengths {lens.tolist()}")
        assert err <= 2 * parent_gap, (which, dt, err, parent_gap)
        eager = m.generate(**hb, max_new_tokens=NT, eos_token_id=eos, pad_token_id=1, use_graph=False,
                           beam_search=BeamSearch(K, length_penalty=lp, num_return_sequences=K))
        assert torch.equal(eager.sequences, seq) and torch.equal(eager.sequences_scores, out.sequences_scores)


def test_beam_states_do_not_leak_and_refusals(dev):
    """greedy and sampled fan-out calls before and after a beam call give the same tokens (the fan-out request shares the beam
    request's state and has a graph of its own); the refusals that need a model"""
    from gar_amd import BeamSearch, hip
    from gar_amd.modeling_gar import GARModel
    from test_gpu_fanout import _gc, _tiny_setup
    cfg, W, batch = _tiny_setup()
    for dt in (torch.bfloat16, torch.float32):
        hb = _half(batch, dt)
        m = GARModel(cfg, W, dt)
        g0 = m.generate(**hb, max_new_tokens=NT).sequences.cpu()
        f0 = m.generate(**hb, generation_config=_gc(cfg, NT, 4), seed=5).sequences.cpu()
        b0 = m.generate(**hb, max_new_tokens=NT, beam_search=BeamSearch(4, num_return_sequences=2))
        assert tuple(b0.sequences.shape) == (6, NT) and b0.token_logprobs is None
        assert torch.equal(m.generate(**hb, max_new_tokens=NT).sequences.cpu(), g0)
        assert torch.equal(m.generate(**hb, generation_config=_gc(cfg, NT, 4), seed=5).sequences.cpu(), f0)
        b1 = m.generate(**hb, max_new_tokens=NT, beam_search=dict(num_beams=4, num_return_sequences=2))
        assert torch.equal(b1.sequences, b0.sequences) and torch.equal(b1.sequences_scores, b0.sequences_scores)
        assert m.generate(**hb, max_new_tokens=NT).sequences_scores is None
    with pytest.raises(hip.GarError, match="beam_search"):
        m.generate_pipelined([hb], max_new_tokens=4, beam_search=BeamSearch(2))
    with pytest.raises(hip.GarError, match="num_beams"):
        m.generate(**hb, max_new_tokens=4, num_beams=4)
    with pytest.raises(hip.GarError, match="32"):
        m.generate(**hb, max_new_tokens=4, eos_token_id=[1, 2], beam_search=BeamSearch(16))
    m8 = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype="fp8")
    with pytest.raises(hip.GarError, match="fp8"):
        m8.generate(**_half(batch, torch.bfloat16), max_new_tokens=4, beam_search=BeamSearch(2))
