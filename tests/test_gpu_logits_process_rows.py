"""GPU (-m gpu): per-request logits processing in ContinuousBatcher — gar_logits_process_rows against gar_logits_process
on every row alone and against the restatement tests/logits_process_ref.py, bit for bit; its clamps; and
ContinuousBatcher(processing=True) end to end: processed, unprocessed and sampled tickets in one decode batch, each against its own
single-region generate(logits_processing=...), through ragged prompts and re-basing, in bf16 by the properties the processors
guarantee, and the default path untouched. The batcher helpers are those of tests/test_gpu_sample_rows.py, re-stated."""
import pytest
import torch

import logits_process_ref as R

pytestmark = pytest.mark.gpu

B, COLS, C = 8, 24, 17                  # rows of one launch, columns of the token matrix, the shared column
SENTINEL = 12288.0                      # (exact in bf16 and fp16)
A = [0, 1, 2, 3, 4, 5]                  # the histories' alphabet; every other column of the token matrix holds ids >= 8
EOS_SLOT = 6                            # the first eos id (the second is V - 1)


def _round_up(x, m):
    return (x + m - 1) // m * m


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _hist(kind, t):
    """t ids over the alphabet, built to repeat: period 3 (every 2- and 3-gram recurs), or pseudo-random with duplicates"""
    if kind == "period3":
        return [A[j % 3] for j in range(t)]
    return [A[(j * j + 3 * j) % 5] for j in range(t)]


def _request_sets(V):
    """two sets of eight (options or None, col0, history kind): the rows of one launch carry different requests"""
    eos = [EOS_SLOT, V - 1]
    tail = _hist("period3", C - 3)[-2:]                                    # the last two ids of the bad-word row's history
    everything = dict(repetition_penalty=1.25, no_repeat_ngram_size=3, min_new_tokens=9, suppress_tokens=[9, V - 2],
                      begin_suppress_tokens=[10], bad_words_ids=[[11], tail + [12], [7, 7, 13]])
    set_a = [(None, 3, "mixed"),                                                            # no request: a zero header
             (dict(repetition_penalty=1.7), 0, "mixed"),                                    # penalty only, t = 17
             (dict(no_repeat_ngram_size=1), 3, "mixed"),                                    # t = 14
             (dict(no_repeat_ngram_size=2), 11, "period3"),                                 # t = 6
             (dict(no_repeat_ngram_size=3), 0, "period3"),                                  # t = 17
             (dict(min_new_tokens=7), 11, "mixed"),                                         # t = 6 < 7: both eos ids banned
             (dict(min_new_tokens=7, repetition_penalty=0.8), 3, "mixed"),                  # t = 14 >= 7: no eos ban
             (everything, 11, "period3")]                                                   # t = 6
    set_b = [(dict(suppress_tokens=[8, 9, V - 1], begin_suppress_tokens=[10, 11, 0]), C, "mixed"),      # col0 = c: t = 0
             (dict(bad_words_ids=[[12], tail + [13], [1, 1, 14]]), 3, "period3"),           # 1 and 3 tokens, the prefix ends the history
             (None, 0, "period3"),
             (everything, 0, "period3"),                                                    # t = 17 >= 9: no eos ban, n = 3 bans
             (dict(repetition_penalty=1.3, begin_suppress_tokens=[9]), C, "mixed"),         # t = 0: nothing to penalise
             (dict(no_repeat_ngram_size=2, repetition_penalty=1.1), 3, "period3"),
             (dict(suppress_tokens=[V - 1]), 11, "mixed"),
             (dict(no_repeat_ngram_size=3, min_new_tokens=18), 0, "period3")]               # t = 17 < 18
    return eos, [set_a, set_b]


def _token_matrix(V, reqs, c, seed, cols=COLS):
    """[B, cols] int64: row b's history at columns col0 .. c-1, every other column a random valid id >= 8 — ids no history
    holds, so a read in front of col0 or at / behind c marks entries the row's request must not touch"""
    g = torch.Generator().manual_seed(seed)
    toks = torch.randint(8, V, (len(reqs), cols), generator=g)
    hists = []
    for b, (_, col0, kind) in enumerate(reqs):
        lo = max(0, min(col0, c))
        h = _hist(kind, c - lo)
        toks[b, lo:c] = torch.tensor(h, dtype=torch.int64)
        hists.append(h)
    return toks, hists


def _blocks(reqs, V, eos):
    from gar_amd import LogitsProcessing, ops
    from gar_amd.continuous import pack_process_row
    blocks = torch.zeros((len(reqs), ops.LOGITS_PROCESS_WORDS), dtype=torch.int32)
    for b, (P, col0, _) in enumerate(reqs):
        w = pack_process_row(None if P is None else LogitsProcessing.coerce(P), V, eos, col0)
        blocks[b, :len(w)] = torch.tensor(w, dtype=torch.int32)
    return blocks


def _logits(V, dtype, seed, rows=B):
    ld = _round_up(V, 64) + (64 if V % 64 == 0 else 0)                      # always some padding columns
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), SENTINEL, dtype=dtype)
    x[:, :V] = (torch.randn(rows, V, generator=g) * 2.5).to(dtype)
    return x


def _alone(x_row, V, hist, P, eos):
    """gar_logits_process on one row alone, its history copied to columns 0 .. t-1 of a token matrix of its own"""
    from gar_amd import LogitsProcessing, ops
    t = len(hist)
    toks = torch.full((1, COLS), 3, dtype=torch.int64)
    toks[0, :t] = torch.tensor(hist, dtype=torch.int64)
    xd = x_row.clone().cuda()
    params = torch.tensor(LogitsProcessing.coerce(P).pack(V, eos), dtype=torch.int32, device="cuda:0")
    ops.logits_process(xd, V, toks.cuda(), torch.tensor([t], dtype=torch.int32, device="cuda:0"),
                       torch.tensor(list(eos) + [-1], dtype=torch.int64, device="cuda:0"), params)
    torch.cuda.synchronize()
    return xd.cpu()


def _rows(x, V, toks, c, eos, blocks):
    from gar_amd import ops
    xd = x.clone().cuda()
    ops.logits_process_rows(xd, V, toks.cuda(), None if c is None else torch.tensor([c], dtype=torch.int32, device="cuda:0"),
                            torch.tensor(list(eos) + [-1], dtype=torch.int64, device="cuda:0"), blocks.cuda())
    torch.cuda.synchronize()
    return xd.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [128256, 1000, 37])
def test_rows_kernel_equals_gar_logits_process_and_the_restatement_bit_for_bit(dtype, V):
    """eight different requests in one launch at column 17 of a 24-column token matrix, col0 in {0, 3, 11, 17}: every row is, bit for
    bit, what gar_logits_process writes on that row alone with its history at columns 0 .. t-1, and what the restatement computes;
    the rows without a request and the columns V .. ld-1 keep their bytes; the columns outside col0 .. c-1 are never read"""
    from gar_amd import hip
    hip.require_device(0)
    eos, sets = _request_sets(V)
    assert {col0 for s in sets for _, col0, _ in s} == {0, 3, 11, C}
    for si, reqs in enumerate(sets):
        x = _logits(V, dtype, seed=V + si)
        toks, hists = _token_matrix(V, reqs, C, seed=7 * V + si)
        got = _rows(x, V, toks, C, eos, _blocks(reqs, V, eos))
        assert bool((got[:, V:] == SENTINEL).all())
        for b, (P, col0, _) in enumerate(reqs):
            if P is None:
                assert torch.equal(_bits(got[b]), _bits(x[b])), (si, b)
                continue
            want = R.process_row(hists[b], x[b], V, P, eos)
            assert not torch.equal(_bits(want), _bits(x[b])), (si, b, "a request that changes nothing checks nothing")
            assert torch.equal(_bits(got[b]), _bits(want)), (si, b, P, (got[b] != want).nonzero().tolist()[:8])
            alone = _alone(x[b:b + 1], V, hists[b], P, eos)
            assert torch.equal(_bits(got[b]), _bits(alone[0])), (si, b, P)
            # the history's window matters: one column more in front of col0 is another result (an id no history holds)
            front = int(toks[b, col0 - 1]) if col0 > 0 else None
            if front is not None and float(want[front]) == float(x[b, front]) != 0.0 and \
                    (P.get("repetition_penalty", 1.0) != 1.0 or P.get("no_repeat_ngram_size") == 1):
                wider = R.process_row([front] + hists[b], x[b], V, P, eos)
                assert not torch.equal(_bits(wider), _bits(want)), (si, b)


def test_rows_kernel_clamps():
    """col0 behind the column, col0 < 0, a column behind out_cols, a header whose lists exceed the block, ids outside [0, V) in the
    history and in the lists: ordinary inputs inside allocated buffers — the result is that of the clamped values"""
    from gar_amd import hip, ops
    hip.require_device(0)
    V, dtype = 1000, torch.float32
    eos = [EOS_SLOT, V - 1]
    P = dict(repetition_penalty=1.4, no_repeat_ngram_size=2, min_new_tokens=3, suppress_tokens=[9], begin_suppress_tokens=[10])
    x = _logits(V, dtype, seed=5, rows=5)
    reqs = [(P, C + 4, "period3"), (P, -5, "period3"), (P, 3, "mixed"), (P, 3, "mixed"), (P, 0, "mixed")]
    toks, hists = _token_matrix(V, reqs, C, seed=11)
    assert hists[0] == [] and len(hists[1]) == C                            # what the clamps of col0 mean
    toks[3, 5], toks[3, 8], toks[3, 9] = -3, V, 2 ** 40                      # row 3: ids outside the vocabulary in its history
    hists[3] = toks[3, 3:C].tolist()
    blocks = _blocks(reqs, V, eos)
    assert blocks[0, 7] == C + 4 and blocks[1, 7] == -5
    blocks[2, 3] = ops.LOGITS_PROCESS_WORDS                                 # row 2: n_suppress beyond the block — it names no list
    blocks[4, 8], blocks[4, 9] = V, -1                                      # row 4: list ids outside the vocabulary
    got = _rows(x, V, toks, C, eos, blocks)
    no_lists = dict(P, suppress_tokens=[], begin_suppress_tokens=[])
    wants = [R.process_row(hists[0], x[0], V, P, eos), R.process_row(hists[1], x[1], V, P, eos),
             R.process_row(hists[2], x[2], V, no_lists, eos), R.process_row(hists[3], x[3], V, P, eos),
             R.process_row(hists[4], x[4], V, dict(P, suppress_tokens=[V], begin_suppress_tokens=[-1]), eos)]
    for b, want in enumerate(wants):
        assert torch.equal(_bits(got[b]), _bits(want)), (b, (got[b] != want).nonzero().tolist()[:8])
    assert float(got[0, 10]) == float("-inf") and float(got[1, 10]) != float("-inf")     # t = 0 on row 0 only
    # the shared column behind out_cols: c = 30 over 24 columns is column 24, and a NULL step_dev is column 0
    full, hists_full = _token_matrix(V, reqs[2:3], COLS, seed=13)
    got = _rows(x[:1], V, full, 30, eos, _blocks(reqs[2:3], V, eos))
    assert len(hists_full[0]) == COLS - 3
    assert torch.equal(_bits(got[0]), _bits(R.process_row(hists_full[0], x[0], V, P, eos)))
    got = _rows(x[:1], V, full, None, eos, _blocks(reqs[2:3], V, eos))
    assert torch.equal(_bits(got[0]), _bits(R.process_row([], x[0], V, P, eos)))


# ---- the batcher ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from gar_amd import GARConfig
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.tiny()
    return cfg, synthetic_weights(cfg), GARProcessor.from_config(cfg, max_num_tiles=4)


def _sample(cfg, proc, i, w=200, h=160, dtype=torch.float32, multi=False):
    from gar_amd.eval_dataset import MultiRegionDataset, SingleRegionCaptionDataset
    from gar_amd.synthetic import synthetic_disjoint_masks, synthetic_image, synthetic_mask
    img = synthetic_image(i, w, h)
    if multi:
        masks = synthetic_disjoint_masks(i, 3, w, h)
        qs = "What is the relationship between <Prompt0>, <Prompt1> and <Prompt2>?"
        return MultiRegionDataset(img, masks, qs, proc, data_dtype=dtype, device="cpu")[0]
    return SingleRegionCaptionDataset(img, synthetic_mask(i, w, h), proc, data_dtype=dtype, device="cpu")[0]


def _pick_eos(streams, n_ids, max_new):
    """synthetic EOS ids: token ids out of the regions' own free-running streams, chosen greedily so that the captions they cut
    have MIXED lengths (some rows stop after a few tokens, some run to max_new_tokens)."""
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
    return sorted(eos), lengths(eos)


def _cut(row, eos):
    return row[:next((j + 1 for j, t in enumerate(row) if t in eos), len(row))]


def _alone_tokens(m, sample, NT, eos, P=None, sampling=None, seed=None):
    """the single-region run a ticket has to reproduce: generate() on that sample alone under the ticket's options"""
    kw = {} if P is None else dict(logits_processing=P)
    if sampling is not None:
        kw.update(do_sample=True, seed=seed, **sampling)
    return _cut(m.generate(**sample, max_new_tokens=NT, eos_token_id=eos or None, **kw).sequences[0].cpu().tolist(), eos)


SAMPLING = [dict(temperature=0.8, top_k=50, top_p=0.9), dict(temperature=1.2, top_k=0, top_p=0.95)]


@pytest.fixture(scope="module")
def mixed(tiny):
    """the model, eight tickets and their single-region references, computed once. The regions of the processed greedy tickets are
    chosen — out of a pool, by the single-region generate() alone — so that the processing changes their caption."""
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    NT = 16
    m = GARModel(cfg, W, torch.float32)
    pool = [_sample(cfg, proc, 300 + i) for i in range(12)]
    streams = [m.generate(**s, max_new_tokens=NT).sequences[0].cpu().tolist() for s in pool]
    eos, lens = _pick_eos(streams, 4, NT)
    plain = [_cut(s, eos) for s in streams]
    assert min(lens) <= NT - 3 and len(set(lens)) >= 3, lens
    free = list(range(len(pool)))

    def choose(make):
        """the first unused region whose options (made from its plain caption) change its single-region caption"""
        for i in free:
            P = make(i)
            if P is not None and _alone_tokens(m, pool[i], NT, eos, P) != plain[i]:
                free.remove(i)
                return i, P
        raise AssertionError("no region of the pool is changed by these options")

    def min_new(i):             # the plain caption ends at an eos id before max_new_tokens: two more tokens are demanded
        return dict(min_new_tokens=len(plain[i]) + 2) if len(plain[i]) <= NT - 3 else None

    def bans(i):                # plain's first token is banned at step 0, its second always, and a bad word of its own
        p = streams[i]
        return dict(begin_suppress_tokens=[p[0]], suppress_tokens=[p[1]], bad_words_ids=[[p[2]], [p[3], p[4], p[5]]])
    tickets = [(None, None)]                                                        # 0: unprocessed greedy
    tickets += [choose(min_new)]                                                    # (first: it needs a short plain caption)
    tickets += [choose(lambda i: dict(repetition_penalty=1.3)), choose(lambda i: dict(no_repeat_ngram_size=2)), choose(bans),
                choose(lambda i: dict(repetition_penalty=1.2, no_repeat_ngram_size=3, suppress_tokens=[streams[i][0]]))]
    tickets[0] = (free.pop(0), None)
    sampled = [(free.pop(0), dict(repetition_penalty=1.3)), (free.pop(0), dict(repetition_penalty=1.5, no_repeat_ngram_size=2))]
    reqs = [dict(sample=pool[i], P=P, sampling=None, seed=None, plain=plain[i]) for i, P in tickets]
    reqs += [dict(sample=pool[i], P=P, sampling=SAMPLING[k], seed=900 + k, plain=plain[i]) for k, (i, P) in enumerate(sampled)]
    for r in reqs:
        r["exp"] = _alone_tokens(m, r["sample"], NT, eos, r["P"], r["sampling"], r["seed"])
    return dict(m=m, reqs=reqs, eos=eos, NT=NT, pool=pool, plain=plain)


def _submit(cb, r):
    kw = {} if r["P"] is None else dict(logits_processing=r["P"])
    if r["sampling"] is not None:
        kw.update(do_sample=True, seed=r["seed"], **r["sampling"])
    return cb.submit(r["sample"], **kw)


@pytest.mark.parametrize("use_graph", [True, False])
def test_processed_unprocessed_and_sampled_tickets_share_one_decode_batch(mixed, use_graph):
    """eight tickets in four slots, f32: unprocessed greedy, penalty, n-gram ban, min_new_tokens over the batcher's eos ids, bad words
    + suppress + begin-suppress, everything, and two sampled tickets with a penalty — each ticket's tokens are those of generate() on
    that sample alone with the same options and seed, and every processed greedy ticket differs from its own unprocessed run"""
    from gar_amd.continuous import ContinuousBatcher
    c = mixed
    cb = ContinuousBatcher(c["m"], slots=4, max_new_tokens=c["NT"], eos_token_id=c["eos"], sampling=True, processing=True,
                           poll_every=1, admit_min=1, use_graph=use_graph)
    tickets = [_submit(cb, r) for r in c["reqs"]]
    assert len(tickets) == 8
    res = cb.flush()
    print(f"stats {cb.stats}; lengths {[len(res[t]) for t in tickets]}")
    for i, (t, r) in enumerate(zip(tickets, c["reqs"])):
        assert res[t] == r["exp"], (i, r["P"], r["sampling"], res[t], r["exp"])
        if r["P"] is not None and r["sampling"] is None:
            assert res[t] != r["plain"], (i, r["P"], "the processing changed nothing: the comparison above checks nothing")
    assert res[tickets[0]] == c["reqs"][0]["plain"]
    assert cb.stats["admitted"] == cb.stats["retired"] == 8 and not cb._processing
    assert not bool(cb.st["row_proc"][:, :8].any())                          # every retired row's header is zero again


def test_processed_tickets_through_ragged_prompts_and_rebasing(tiny):
    """prompts of two lengths, a cache of a few buckets and no horizon: a re-base shifts the token log under live processed rows, and
    their col0 with it — a col0 left behind would move every later history. The schedule is built, not found:
    * the first four tickets (one of them the longer prompt) are processed ones that fill the four slots at column 0: the third
      token of three of them is made an eos id, so they leave by column 3, and the fourth, S, ends within 4 .. 12 tokens (an idle
      batcher would restart its clock, and its columns, at 0);
    * the next ones are admitted at a column > 0: three run all 40 tokens (min_new_tokens = 40 bans every eos id), and K —
      min_new_tokens = 20, and a token of its own from steps 20 .. 33 made an eos id — ends while they are live and the clock is past
      what the cache holds for a new row: the admission into K's slot re-bases with dT > 0 under three live processed rows;
    * six more tickets, processed and unprocessed, run in slots that processed tickets have left."""
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    slots, NT = 4, 40
    m = GARModel(cfg, W, torch.float32)
    pool = [_sample(cfg, proc, 200 + i, multi=(i % 3 == 1)) for i in range(16)]
    n_prompt = [int(s["input_ids"].shape[1]) for s in pool]
    assert len(set(n_prompt)) == 2 and all((n == max(n_prompt)) == (i % 3 == 1) for i, n in enumerate(n_prompt))
    plain = [m.generate(**s, max_new_tokens=NT).sequences[0].cpu().tolist() for s in pool]

    def short(i):
        return [dict(repetition_penalty=1.3, begin_suppress_tokens=[plain[i][0]]), dict(no_repeat_ngram_size=2, suppress_tokens=[plain[i][0]])][i % 2]

    def full(i):
        return dict(no_repeat_ngram_size=2, min_new_tokens=NT, suppress_tokens=[plain[i][0]])
    shorts, long_ones = [0, 1, 2], [5, 4, 6]                               # (1 and 4 are the longer prompts)
    eos = {_alone_tokens(m, pool[i], NT, [], short(i))[2] for i in shorts}
    s_ = k = None
    for c in (3, 7, 9, 10):         # S: the first region whose processed caption can be made to end within 4 .. 12 tokens
        Fs = _alone_tokens(m, pool[c], NT, [], short(c))
        hit = next((j for j, tok in enumerate(Fs) if tok in eos), NT)
        own = next((Fs[j] for j in range(3, 12) if Fs[j] not in Fs[:3]), None)
        if hit < 3 or (hit > 11 and own is None):
            continue
        eos, s_ = (eos | {own} if hit > 11 else eos), c
        break
    assert s_ is not None
    for c in (8, 12, 13, 15):       # K: min_new_tokens = 20, and an end within 21 .. 34 tokens
        P_k = dict(repetition_penalty=1.3, min_new_tokens=20, begin_suppress_tokens=[plain[c][0]])
        F = _alone_tokens(m, pool[c], NT, sorted(eos), P_k)
        # no eos id in time: one of K's own tokens of steps 20 .. 33 that neither it nor S's first tokens have produced before
        own = next((F[j] for j in range(20, min(34, len(F))) if F[j] not in F[:20] and F[j] not in Fs[:3]), None)
        if len(F) > 34 and own is None:
            continue
        eos, k = (eos | {own} if len(F) > 34 else eos), c
        break
    assert k is not None
    eos = sorted(eos)
    first = shorts + [s_]
    rest = [i for i in (3, 7, 9, 10, 11, 12, 13, 15, 14) if i not in (s_, k)][:6]
    order = first + [long_ones[0], long_ones[1], k, long_ones[2]] + rest
    Ps = [short(i) for i in first] + [full(long_ones[0]), full(long_ones[1]), P_k, full(long_ones[2])] + \
        [None if j % 2 == 0 else dict(short(i), min_new_tokens=12) for j, i in enumerate(rest)]
    exp = [_alone_tokens(m, pool[i], NT, eos, P) for i, P in zip(order, Ps)]
    lens = [len(e) for e in exp]
    assert max(lens[:3]) <= 3 and 4 <= lens[3] <= 12 and lens[4] == lens[5] == lens[7] == NT and 21 <= lens[6] <= 34, lens
    cb = ContinuousBatcher(m, slots=slots, max_new_tokens=NT, eos_token_id=eos, processing=True, poll_every=2, admit_min=1,
                           horizon=0, smax_multiple=64)
    shifts, rebase = [], cb._rebase

    def watched():
        before, live = cb.T, sum(row is not None and row.processed for row in cb.rows)
        ok = rebase()
        shifts.append((before - cb.T, live))
        return ok
    cb._rebase = watched
    tickets = [cb.submit(pool[i], logits_processing=P) for i, P in zip(order, Ps)]
    res = cb.flush()
    print(f"prompts {[n_prompt[i] for i in order]}; lengths {lens}; eos {eos}; re-bases (dT, live processed rows) {shifts}; "
          f"stats {cb.stats}; Smax {cb.Smax}")
    assert cb.stats["rebases"] >= 1, cb.stats
    assert any(dT > 0 and live > 0 for dT, live in shifts), shifts          # a token-log shift under live processed rows
    for j, (i, t) in enumerate(zip(order, tickets)):
        assert res[t] == exp[j], (j, i, Ps[j], res[t], exp[j])
        if Ps[j] is None:
            assert res[t] == _cut(plain[i], eos)
        else:
            assert res[t][0] != plain[i][0]                                # (every set bans plain's first token)
    assert cb.stats["admitted"] == cb.stats["retired"] == len(order)


def _bigrams_repeat(toks):
    seen = set()
    for a in zip(toks, toks[1:]):
        if a in seen:
            return True
        seen.add(a)
    return False


def test_bf16_properties_hold_by_construction(tiny):
    """bf16 (and one ticket over an fp8 KV cache): the kernels a batch selects differ from the single-region run's, so the tokens
    are checked by what the processors guarantee whatever the logits — no suppressed or bad-word id in any caption, no repeated bigram
    under no_repeat_ngram_size=2, no eos before min_new_tokens"""
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    NT = 24
    samples = [_sample(cfg, proc, 400 + i, dtype=torch.bfloat16) for i in range(6)]
    for kv in (None, "fp8"):
        m = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype=kv)
        use = samples if kv is None else samples[:1]
        streams = [m.generate(**s, max_new_tokens=NT).sequences[0].cpu().tolist() for s in use]
        eos, _ = _pick_eos(streams, 3, NT)
        Ps = [dict(no_repeat_ngram_size=2, min_new_tokens=NT // 2, suppress_tokens=p[:3], begin_suppress_tokens=[p[3]],
                   bad_words_ids=[[p[4]], [p[5]]], repetition_penalty=1.2) if i % 3 != 2 else None for i, p in enumerate(streams)]
        cb = ContinuousBatcher(m, slots=3, max_new_tokens=NT, eos_token_id=eos, processing=True, poll_every=2, admit_min=1)
        tickets = [cb.submit(s, logits_processing=P) for s, P in zip(use, Ps)]
        res = cb.flush()
        for t, P in zip(tickets, Ps):
            toks = res[t]
            assert 1 <= len(toks) <= NT
            if P is None:
                continue
            banned = set(P["suppress_tokens"]) | {w[0] for w in P["bad_words_ids"] if w[0] not in eos}
            assert not banned & set(toks), (kv, banned & set(toks), toks)
            assert toks[0] != P["begin_suppress_tokens"][0]
            assert not _bigrams_repeat(toks), (kv, toks)
            assert not set(eos) & set(toks[:P["min_new_tokens"]]) and len(toks) > P["min_new_tokens"], (kv, eos, toks)


class _count_launches:
    """wraps ops.logits_process_rows: the row count of every launch"""

    def __init__(self):
        from gar_amd import ops
        self.ops, self.orig, self.shapes = ops, getattr(ops, "logits_process_rows", None), []

        def counted(logits, *a, **kw):
            self.shapes.append(logits.shape[0])
            return self.orig(logits, *a, **kw)
        ops.logits_process_rows = counted

    def undo(self):
        self.ops.logits_process_rows = self.orig


def test_default_path_is_untouched(mixed):
    """a batcher built without ``processing`` carries no blocks and never launches gar_logits_process_rows; with the flag and
    unprocessed tickets only, the same tokens come out — one launch per prompt pass and step, every row left alone"""
    from gar_amd.continuous import ContinuousBatcher
    c = mixed
    m, samples, eos, plain = c["m"], c["pool"][:8], c["eos"], c["plain"][:8]
    counted = _count_launches()
    try:
        for use_graph in (True, False):
            cb = ContinuousBatcher(m, slots=4, max_new_tokens=c["NT"], eos_token_id=eos, poll_every=1, admit_min=1, use_graph=use_graph)
            tickets = [cb.submit(s, logits_processing=None) for s in samples]
            res = cb.flush()
            assert [res[t] for t in tickets] == plain
            assert "row_proc" not in cb.st and "row_words" not in cb.st and counted.shapes == []
        cb = ContinuousBatcher(m, slots=4, max_new_tokens=c["NT"], eos_token_id=eos, processing=True, poll_every=1, admit_min=1,
                               use_graph=False)
        tickets = [cb.submit(s, logits_processing={}) for s in samples]
        res = cb.flush()
        assert [res[t] for t in tickets] == plain
        assert "row_words" not in cb.st and tuple(cb.st["row_proc"].shape) == (4, 4096)
        assert len(counted.shapes) >= cb.stats["prompt_passes"] + cb.stats["decode_steps"]
        assert sum(counted.shapes) == 4 * cb.stats["decode_steps"] + len(samples)
    finally:
        counted.undo()
