"""GPU (-m gpu): generate(logits_processing=...) — gar_logits_process against the restatement
tests/logits_process_ref.py bit for bit (f32, bf16, fp16 through the twin library), and GARModel.generate with processors against a
replay of the same tokens: greedy and sampled, graph and eager, a ragged left-padded batch, fan-out, and the default path untouched."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import logits_process_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
V_A, LD_A, SENTINEL = 1000, 1024, 12345.0
NT = 24


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "logits_process.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def _params(P, V, eos=()):
    from gar_amd import LogitsProcessing
    return torch.tensor(LogitsProcessing.coerce(P).pack(V, eos), dtype=torch.int32, device="cuda:0")


def _run_kernel(x, V, hist, P, eos, step_dev=True, stride=None):
    """one gar_logits_process on a device copy of ``x`` [B, ld]; the histories [B, t] sit in a wider token matrix (out_stride > t)
    whose other columns hold an id the processors would act on if they read it"""
    from gar_amd import ops
    B, t = hist.shape
    stride = stride or t + 5
    toks = torch.full((B, stride), 3, dtype=torch.int64)
    toks[:, :t] = hist
    toks = toks.cuda()
    xd = x.cuda()
    eos_d = torch.tensor(list(eos) + [-1], dtype=torch.int64, device="cuda:0")
    step = torch.tensor([t], dtype=torch.int32, device="cuda:0") if step_dev else None
    ops.logits_process(xd, V, toks[:, :max(t, 1)], step, eos_d, _params(P, V, eos))
    torch.cuda.synchronize()
    return xd.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_equals_restatement_bit_for_bit_on_the_golden_cases(dtype):
    """B = 3, V = 1000, ld = 1024: every history of golden (a) (lengths 0, 1, 2 and 300 over a 6-id alphabet — the case that fails if
    duplicates compound or one block's thread count bounds t) x every option set (each processor alone, all together), the logits
    as stored in ``dtype``; columns 1000..1023 hold a sentinel that must survive; step_dev as a device value and, for the empty
    history, NULL; a history with ids outside [0, V) names no entry."""
    from gar_amd import hip
    hip.require_device(0)
    g, meta = _golden()
    eos = g["a_eos"].tolist()
    x = torch.full((3, LD_A), SENTINEL, dtype=dtype)
    x[:, :V_A] = torch.from_numpy(g["a_logits"]).to(dtype)
    n = 0
    for hname, oi in meta["a_cases"]:
        P, hist = meta["a_options"][oi], torch.from_numpy(g["a_" + hname])
        want = R.process(hist.tolist(), x, V_A, P, eos)
        for step_dev in ((True, False) if hist.shape[1] == 0 else (True,)):
            got = _run_kernel(x, V_A, hist, P, eos, step_dev)
            assert torch.equal(_bits(got), _bits(want)), (hname, P, step_dev, (got != want).nonzero().tolist()[:8])
            assert (got[:, V_A:] == SENTINEL).all()
        n += 1
    assert n == 48
    # f32: what transformers' own classes produced
    if dtype == torch.float32:
        idx, val = torch.from_numpy(g["a_idx"]).long(), torch.from_numpy(g["a_val"])
        c = meta["a_cases"].index(["h300", len(meta["a_options"]) - 1])
        exp = x.clone()
        sel = idx[:, 0] == c
        exp[idx[sel, 1], idx[sel, 2]] = val[sel]
        got = _run_kernel(x, V_A, torch.from_numpy(g["a_h300"]), meta["a_options"][-1], eos)
        assert torch.equal(_bits(got), _bits(exp))
    # ids outside the vocabulary: skipped in the history, never dereferenced
    hist = torch.tensor([[5, -3, 1000, 5], [2 ** 40, 999, 0, 999], [-1, -1, -1, -1]])
    P = dict(repetition_penalty=1.7, no_repeat_ngram_size=2)
    got = _run_kernel(x, V_A, hist, P, eos)
    assert torch.equal(_bits(got), _bits(R.process(hist.tolist(), x, V_A, P, eos)))
    assert torch.equal(_bits(got[2]), _bits(x[2]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_at_the_real_vocabulary(dtype):
    """B = 64, V = 128256, t = 1024: the bitmap size of the real vocabulary, histories over the whole id range (even rows) and over
    8 ids (odd rows: repeated 3-grams and duplicates), the penalty, n = 3 and a suppress list"""
    from gar_amd import hip
    hip.require_device(0)
    B, V, t = 64, 128256, 1024
    g = torch.Generator().manual_seed(3)
    x = torch.full((B, V + 64), SENTINEL, dtype=dtype)
    x[:, :V] = (torch.randn(B, V, generator=g) * 2.5).to(dtype)
    hist = torch.randint(0, V, (B, t), generator=g)
    small = torch.tensor([0, V - 1, 31, 32, 63, 64, 4095, 70000])
    hist[1::2] = small[torch.randint(0, 8, (B // 2, t), generator=g)]
    P = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, suppress_tokens=[V - 1, 77])
    got = _run_kernel(x, V, hist, P, (), stride=t + 64)
    want = R.process(hist.tolist(), x, V, P)
    assert torch.equal(_bits(got), _bits(want))
    assert int((got != x).sum()) > B * 8


# ---- end to end on the tiny fixture ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shared():
    import test_gpu_logprobs as T
    cfg, W, proc, batch, ragged = T._setup()
    return T, cfg, ragged


@functools.lru_cache(maxsize=None)
def _plain(dtype):
    """plain greedy on the ragged batch, made before any processed request on the model of that dtype"""
    T, cfg, ragged = _shared()
    return T._model(dtype).generate(**ragged, max_new_tokens=NT).sequences.cpu()


def _option_sets(dtype):
    """each one suppresses plain greedy's first tokens, so it has to change every row"""
    first = sorted(set(_plain(dtype)[:, 0].tolist()))
    return [dict(repetition_penalty=1.3, begin_suppress_tokens=first),
            dict(no_repeat_ngram_size=2, suppress_tokens=first),
            dict(repetition_penalty=1.25, no_repeat_ngram_size=3, min_new_tokens=12, suppress_tokens=first[:1],
                 begin_suppress_tokens=first, bad_words_ids=[[int(_plain(dtype)[0, 1])], _plain(dtype)[1, 2:4].tolist()])]


def _replay_raw(m, batch, seq, dtype):
    """the raw logits of every step on the context ``seq`` fixes: the same inputs without processing, teacher-forced"""
    out = m.generate(**batch, max_new_tokens=seq.shape[1], forced_tokens=seq, return_logits=True)
    return out.logits.cpu().to(dtype)


def _ends(seq, eos):
    """per row: tokens up to and including its first eos"""
    return [next((j + 1 for j, tk in enumerate(r.tolist()) if tk in eos), seq.shape[1]) for r in seq]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_generate_with_processors_against_replay(dtype, which):
    """seq = generate(logits_processing=P) on a ragged left-padded batch of 3; the same inputs again without processing, forced on
    seq, give every step's raw logits on the identical context; the restatement on history seq[:, :t] + first-index argmax must
    give seq[:, t] at every step. P changes every row against plain greedy; its properties hold on seq; graph and eager runs agree;
    return_logits returns the processed scores."""
    from gar_amd import LogitsProcessing
    T, cfg, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(dtype)
    plain = _plain(dtype)
    P = _option_sets(dtype)[which]
    eos = []
    if which == 2:          # an eos id the run would produce before min_new_tokens allows it
        free = m.generate(**ragged, max_new_tokens=NT, logits_processing=P).sequences.cpu()
        eos = [int(free[0, 5]), int(free[1, 7])]
    kw = dict(max_new_tokens=NT, eos_token_id=eos or None, pad_token_id=0)
    out = m.generate(**ragged, **kw, logits_processing=LogitsProcessing(**P), return_logits=True)
    seq = out.sequences.cpu()
    n = seq.shape[1]
    assert seq.shape[0] == 3 and (n == NT or eos)
    for b in range(3):
        assert seq[b].tolist() != plain[b, :n].tolist(), (b, P)
    assert torch.equal(m.generate(**ragged, **kw, logits_processing=P, use_graph=False).sequences.cpu(), seq)
    ends = _ends(seq, eos)
    raw = _replay_raw(m, ragged, seq, dtype)
    scores = out.logits.cpu()
    for b in range(3):
        for t in range(ends[b]):
            want = R.process_row(seq[b, :t].tolist(), raw[b, t], V, P, eos)
            assert R.first_argmax(want) == int(seq[b, t]), (b, t)
            assert torch.equal(scores[b, t], want.float()), (b, t)       # HF's `scores`
    # the properties the processors promise
    o = R.options(P)
    banned_always = set(o["suppress_tokens"]) | {w[0] for w in o["bad_words_ids"] if len(w) == 1 and w[0] not in eos}
    for b in range(3):
        row = seq[b, :ends[b]].tolist()
        assert not banned_always & set(row), (b, row)
        assert row[0] not in o["begin_suppress_tokens"]
        k = o["no_repeat_ngram_size"]
        if k:
            grams = [tuple(row[j:j + k]) for j in range(len(row) - k + 1)]
            assert len(grams) == len(set(grams)), (b, row)
        assert not set(eos) & set(row[:o["min_new_tokens"]]), (b, row)
        for w in (w for w in o["bad_words_ids"] if len(w) > 1):
            assert all(row[j:j + len(w)] != list(w) for j in range(1, len(row))), (b, w, row)


SAMPLING = dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=50)


def test_sampling_and_fanout_with_a_penalty_against_the_oracle_draw():
    """do_sample, num_return_sequences = 3, f32: every token of row b * N + i is oracle.sampling.sample of the restated processed
    logits (raw logits from the forced replay of the replicated batch), drawn with row counter b * N + i; the N first draws of a
    prompt share one processed row."""
    from oracle import sampling as S
    from test_gpu_fanout import _repeat
    T, cfg, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(torch.float32)
    N, seed, n = 3, 4242, 16
    P = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    counted = _count_launches()
    out = m.generate(**ragged, **SAMPLING, num_return_sequences=N, seed=seed, max_new_tokens=n, logits_processing=P, return_logits=True)
    seq = out.sequences.cpu()
    assert tuple(seq.shape) == (3 * N, n)
    assert counted.shapes[0] == 3 and all(s == 3 * N for s in counted.shapes[1:])       # once on the prompts' rows, then per step
    counted.undo()
    raw = _replay_raw(m, _repeat(ragged, N), seq, torch.float32)
    for b in range(3):
        assert all(torch.equal(out.logits[b * N, 0], out.logits[b * N + i, 0]) for i in range(N))
    for r in range(3 * N):
        for t in range(n):
            want = R.process_row(seq[r, :t].tolist(), raw[r, t], V, P)
            tok, margin, keep = S.sample(want.numpy(), 0.8, 50, 0.9, seed, r, t)
            assert tok == int(seq[r, t]), (r, t, tok, int(seq[r, t]), margin)
        grams = [tuple(seq[r, j:j + 2].tolist()) for j in range(n - 1)]
        assert len(grams) == len(set(grams))
    assert torch.equal(m.generate(**ragged, **SAMPLING, num_return_sequences=N, seed=seed, max_new_tokens=n, logits_processing=P,
                                  use_graph=False).sequences.cpu(), seq)
    plain = m.generate(**ragged, **SAMPLING, num_return_sequences=N, seed=seed, max_new_tokens=n).sequences.cpu()
    assert not torch.equal(plain, seq)


class _count_launches:
    """wraps ops.logits_process: the row count of every launch"""

    def __init__(self):
        from gar_amd import ops
        self.ops, self.orig, self.shapes = ops, ops.logits_process, []

        def counted(logits, *a, **kw):
            self.shapes.append(logits.shape[0])
            return self.orig(logits, *a, **kw)
        ops.logits_process = counted

    def undo(self):
        self.ops.logits_process = self.orig


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_default_path_is_untouched(dtype):
    """without the parameter — and with None or all-neutral values — the sequences are those of a run made before any processed
    request on the same model, bit for bit, and gar_logits_process is never launched; a processed request launches it once per step"""
    from gar_amd import LogitsProcessing
    T, cfg, ragged = _shared()
    m = T._model(dtype)
    before = _plain(dtype)
    c = _count_launches()
    try:
        m.generate(**ragged, max_new_tokens=NT, logits_processing=dict(repetition_penalty=1.5), use_graph=False)
        assert c.shapes == [3] * NT
        del c.shapes[:]
        for kw in ({}, dict(logits_processing=None), dict(logits_processing=LogitsProcessing()), dict(logits_processing={}),
                   dict(use_graph=False)):
            assert torch.equal(m.generate(**ragged, max_new_tokens=NT, **kw).sequences.cpu(), before), kw
        sampled = [m.generate(**ragged, **SAMPLING, seed=9, max_new_tokens=NT, **kw).sequences.cpu()
                   for kw in ({}, dict(logits_processing=LogitsProcessing(repetition_penalty=1.0)))]
        assert torch.equal(*sampled)
        assert c.shapes == []
    finally:
        c.undo()


def test_fp8_modes_pipeline_and_chunks_carry_the_processors():
    """both opt-in FP8 modes, the GenerationPipeline and a prompt phase cut into chunks: the processed run's properties hold and the
    pipeline / chunked runs equal the plain call bit for bit"""
    from gar_amd.modeling_gar import GARModel, GenerationPipeline
    T, cfg, ragged = _shared()
    W = T._setup()[1]
    first = sorted(set(_plain(torch.bfloat16)[:, 0].tolist()))
    P = dict(no_repeat_ngram_size=2, suppress_tokens=first)
    for kw in (dict(kv_cache_dtype="fp8"), dict(decode_weight_dtype="fp8")):
        seq = GARModel(cfg, W, torch.bfloat16, "cuda:0", **kw).generate(**ragged, max_new_tokens=NT, logits_processing=P).sequences.cpu()
        for row in seq.tolist():
            grams = [tuple(row[j:j + 2]) for j in range(len(row) - 1)]
            assert len(grams) == len(set(grams)) and not set(first) & set(row)
    m = T._model(torch.bfloat16)
    want = m.generate(**ragged, max_new_tokens=NT, logits_processing=P).sequences.cpu()
    outs = m.generate_pipelined([ragged, ragged], max_new_tokens=NT, logits_processing=P)
    torch.cuda.synchronize()
    assert all(torch.equal(o.sequences.cpu(), want) for o in outs) and len(outs) == 2
    assert isinstance(GenerationPipeline(m, logits_processing=P), GenerationPipeline)
    # a prompt phase cut into passes of one sequence each: every chunk's first-token head processes its own rows (to.rows(b0, b1))
    mf = T._model(torch.float32)
    wantf = mf.generate(**ragged, max_new_tokens=NT, logits_processing=P).sequences.cpu()
    S = ragged["input_ids"].shape[1]
    try:
        mf.PREFILL_CHUNK_ROWS = S
        assert len(mf._plan_passes(3, ragged["pixel_values"].shape[0] // 3, S)[1]) == 3
        assert torch.equal(mf.generate(**ragged, max_new_tokens=NT, logits_processing=P).sequences.cpu(), wantf)
    finally:
        del mf.PREFILL_CHUNK_ROWS


def test_one_captured_step_serves_other_lengths_and_other_values():
    """the graph captured by a 4-token request replays for a 24-token request (the history's bound is the token buffer's row, not
    the first request's width) and for other processor values (the parameter block is read on every launch)"""
    from gar_amd.modeling_gar import GARModel
    T, cfg, ragged = _shared()
    m = GARModel(cfg, T._setup()[1], torch.float32, "cuda:0")
    P = dict(no_repeat_ngram_size=1)
    short = m.generate(**ragged, max_new_tokens=4, logits_processing=P).sequences.cpu()
    n_graphs = len(m._graphs)
    long = m.generate(**ragged, max_new_tokens=NT, logits_processing=P).sequences.cpu()
    assert torch.equal(long[:, :4], short) and all(len(set(r)) == NT for r in long.tolist())
    assert torch.equal(m.generate(**ragged, max_new_tokens=NT, logits_processing=P, use_graph=False).sequences.cpu(), long)
    P2 = dict(repetition_penalty=1.4, suppress_tokens=long[:, 0].tolist())
    other = m.generate(**ragged, max_new_tokens=NT, logits_processing=P2).sequences.cpu()
    assert len(m._graphs) == n_graphs
    assert torch.equal(m.generate(**ragged, max_new_tokens=NT, logits_processing=P2, use_graph=False).sequences.cpu(), other)
    assert not torch.equal(other, long)
