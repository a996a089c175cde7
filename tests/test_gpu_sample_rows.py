"""GPU (-m gpu): per-request sampling in ContinuousBatcher — gar_sample_rows against gar_sample / gar_argmax on the same
rows, bit for bit; its eos latches and its step clamp; and ContinuousBatcher(sampling=True) end to end: greedy and sampled tickets
in one decode batch, each against its own single-region generate() and against oracle/sampling.py on the logits of its own forced
replay. Fixture and helpers are those of tests/test_gpu_continuous.py, re-stated."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 2e-5        # tests/test_gpu_sampling.py's: a float32 running sum against the oracle's float64 may sit this close to a boundary

# the parameter sets of tests/test_gpu_sampling.py::test_sample_kernel_equals_oracle
PARAM_SETS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.6, 40, 0.8), (1.0, 5, 0.5), (2.0, 20000, 0.999)]
STEP = 7


def _round_up(x, m):
    return (x + m - 1) // m * m


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
def _padded_logits(B, V, dtype, seed):
    """[B, V] view of a [B, round_up(V, 64)] buffer whose padding columns hold a sentinel that would win any maximum"""
    ld = _round_up(V, 64)
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((B, ld), 6.0e4 if dtype == torch.float16 else 3.0e38, dtype=torch.float32)
    buf[:, :V] = torch.randn(B, V, generator=g) * 2.5
    return buf


def _requests(V):
    """eight different requests for the eight rows of one launch: rows 0 and 4 greedy, the others the six parameter sets with
    distinct keys (one >= 2**61, one >= 2**62), distinct col0 in 0..5 and counter rows 0 / 3"""
    seeds = [1, 123456789012345, 2 ** 61 + 7, 5, 6, 2 ** 62 + 11]
    sampled = iter([(PARAM_SETS[i], seeds[i], i, 3 * (i % 2)) for i in range(6)])
    reqs = []
    for b in range(8):
        if b in (0, 4):
            reqs.append((None, None, b % 3, 0))
        else:
            (temperature, top_k, top_p), seed, col0, crow = next(sampled)
            reqs.append(((temperature, top_p, min(top_k, V)), seed, col0, crow))
    return reqs


def _launch_rows(logits, V, reqs, step, eos=None, cols=12):
    from gar_amd import ops
    from gar_amd.continuous import pack_sample_row
    B, dev = logits.shape[0], logits.device
    words = torch.tensor([pack_sample_row(s, seed, col0, crow) for s, seed, col0, crow in reqs], dtype=torch.int32, device=dev)
    out = torch.full((B, cols), -1, dtype=torch.int64, device=dev)
    cur = torch.full((B,), -1, dtype=torch.int64, device=dev)
    stepd = None if step is None else torch.tensor([step], dtype=torch.int32, device=dev)
    kw = {}
    if eos is not None:
        kw = dict(eos_ids=torch.tensor(eos, dtype=torch.int64, device=dev), finished=torch.full((B,), -1, dtype=torch.int32, device=dev),
                  done_count=torch.zeros(1, dtype=torch.int32, device=dev))
    ops.sample_rows(logits, V, out, out.stride(0), stepd, cur, words, **kw)
    torch.cuda.synchronize()
    col = 0 if step is None else step
    rest = torch.ones(cols, dtype=torch.bool)
    rest[col] = False
    assert torch.equal(out[:, col], cur) and bool((out[:, rest] == -1).all())       # written at the shared column and into cur only
    return cur.cpu().tolist(), kw


def _sample_alone(logits, V, b, req, step):
    """gar_sample on row b alone: B = 1, the row's parameters and key, its own step, row_offset = its counter row"""
    from gar_amd import ops
    (temperature, top_p, top_k), seed, _, crow = req
    dev = logits.device
    out = torch.full((1, 12), -1, dtype=torch.int64, device=dev)
    cur = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.sample(logits[b:b + 1], V, out, out.stride(0), torch.tensor([step], dtype=torch.int32, device=dev), cur,
               torch.tensor([temperature, top_p, float(top_k), 0.0], dtype=torch.float32, device=dev),
               torch.tensor([seed], dtype=torch.int64, device=dev), row_offset=crow)
    torch.cuda.synchronize()
    assert int(out[0, step]) == int(cur[0])
    return int(cur[0])


def _kernel_case(dtype, V):
    from gar_amd import hip
    hip.require_device(0)
    B = 8
    buf = _padded_logits(B, V, dtype, seed=V)
    dup_lo, dup_hi, lone = V // 3, V - 2, V // 2
    buf[0, dup_lo] = buf[0, dup_hi] = 40.0                 # row 0: the maximum at two indices
    buf[4, :V] = float("-inf")                             # row 4: one finite entry
    buf[4, lone] = -3.0
    logits = buf.to(dtype).to("cuda:0")[:, :V]
    assert logits.stride(0) == _round_up(V, 64)
    return logits, _requests(V), (dup_lo, lone)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [128256, 1000, 37])
def test_rows_kernel_equals_gar_sample_and_gar_argmax_bit_for_bit(dtype, V):
    """eight requests in one launch at column 7: every sampled row's token is gar_sample's on that row alone (step 7 - col0, row_offset
    = its counter row) — exact equality —, the greedy rows' are gar_argmax's, with a duplicated maximum (the lower index wins) and a
    row of -inf but one entry; the padding columns' sentinel is never read"""
    from gar_amd import ops
    logits, reqs, (dup_lo, lone) = _kernel_case(dtype, V)
    toks, _ = _launch_rows(logits, V, reqs, STEP)
    assert all(0 <= t < V for t in toks), toks
    for b, req in enumerate(reqs):
        if req[0] is not None:
            alone = _sample_alone(logits, V, b, req, STEP - req[2])
            assert toks[b] == alone, (b, req, toks[b], alone)
    B = logits.shape[0]
    out = torch.full((B, 12), -1, dtype=torch.int64, device=logits.device)
    cur = torch.zeros(B, dtype=torch.int64, device=logits.device)
    ws = torch.empty(ops.argmax_workspace(B, V), dtype=torch.uint8, device=logits.device)
    ops.argmax(logits, V, out, out.stride(0), torch.tensor([STEP], dtype=torch.int32, device=logits.device), cur, ws)
    torch.cuda.synchronize()
    am = cur.cpu().tolist()
    assert toks[0] == am[0] == dup_lo and toks[4] == am[4] == lone, (toks, am)
    # the table is read on every launch: the same launch with rows 1 and 2 made greedy gives gar_argmax's token there too
    greedy = [(None, None, 0, 0) if b in (1, 2) else r for b, r in enumerate(reqs)]
    toks2, _ = _launch_rows(logits, V, greedy, STEP)
    assert toks2[1] == am[1] and toks2[2] == am[2] and [toks2[b] for b in (0, 3, 4, 5, 6, 7)] == [toks[b] for b in (0, 3, 4, 5, 6, 7)]


def test_rows_kernel_latches_and_step_clamp():
    """finished[b] = the shared column exactly for the rows whose token is an eos id, -1 elsewhere, done_count their number; a NULL
    step_dev with col0 = 0 is step 0; col0 behind the column is clamped to the row's step 0"""
    V = 1000
    logits, reqs, _ = _kernel_case(torch.float32, V)
    toks, _ = _launch_rows(logits, V, reqs, STEP)
    eos = [toks[0], toks[2], toks[5], -1]                  # a greedy row and two sampled ones (and an unused entry)
    again, kw = _launch_rows(logits, V, reqs, STEP, eos=eos)
    assert again == toks
    hit = [t in eos[:3] for t in toks]
    assert sum(hit) >= 3
    assert kw["finished"].cpu().tolist() == [STEP if h else -1 for h in hit]
    assert int(kw["done_count"].item()) == sum(hit)
    # a row that is latched keeps its first step
    kw["finished"].fill_(2)
    from gar_amd import ops
    from gar_amd.continuous import pack_sample_row
    words = torch.tensor([pack_sample_row(s, seed, c, r) for s, seed, c, r in reqs], dtype=torch.int32, device=logits.device)
    ops.sample_rows(logits, V, None, 0, torch.tensor([STEP], dtype=torch.int32, device=logits.device),
                    torch.zeros(8, dtype=torch.int64, device=logits.device), words, **kw)
    torch.cuda.synchronize()
    assert kw["finished"].cpu().tolist() == [2] * 8
    # step 0: NULL step_dev with col0 = 0, and col0 = 5 at column 2 (the clamp) — gar_sample's step-0 draw, written at the column
    at0 = [(s, seed, 0, crow) for s, seed, _, crow in reqs]
    ahead = [(s, seed, 5, crow) for s, seed, _, crow in reqs]
    t_null, _ = _launch_rows(logits, V, at0, None)
    t_clamp, _ = _launch_rows(logits, V, ahead, 2)
    want = [_sample_alone(logits, V, b, r, 0) if r[0] is not None else toks[b] for b, r in enumerate(reqs)]
    assert t_null == want and t_clamp == want
    t_step2, _ = _launch_rows(logits, V, at0, 2)           # (and the step does move the draw)
    assert t_step2 != want


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


OPTION_SETS = [dict(temperature=0.8, top_k=50, top_p=0.9), dict(temperature=1.2, top_k=0, top_p=0.95),
               dict(temperature=0.7, top_k=20, top_p=1.0)]


def _check_against_oracle(m, V, sample, toks, opts, seed):
    """check (b): the ticket replayed with its own tokens forced; at every step j its token is the oracle's draw (key seed, counter row
    0, step j) from that step's logits, or the neighbour in the kept set within MARGIN. Returns the near steps."""
    from oracle import sampling as S
    n = len(toks)
    forced = torch.tensor([toks + [0] * (max(n, 2) - n)], dtype=torch.int64)
    lg = m.generate(**sample, forced_tokens=forced, return_logits=True, max_new_tokens=max(n, 2)).logits.float().cpu().numpy()
    top_k = min(opts["top_k"], V)
    near = []
    for j, tok in enumerate(toks):
        exp, margin, keep = S.sample(lg[0, j, :V], opts["temperature"], top_k, opts["top_p"], seed, 0, j)
        assert keep[tok], (j, tok, "token outside the kept set")
        if tok != exp:
            kept = np.flatnonzero(keep)
            a, b = int(np.searchsorted(kept, tok)), int(np.searchsorted(kept, exp))
            assert margin < MARGIN and abs(a - b) == 1, (j, tok, exp, margin)
            near.append(j)
    return near


@pytest.fixture(scope="module")
def mixed(tiny):
    """the model, 12 regions and their single-region references, computed once: even tickets greedy, odd tickets sampled under one
    of three option sets and the key 1000 + i; eos ids out of the tickets' own free-running streams (mixed lengths)"""
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    NT = 16
    m = GARModel(cfg, W, torch.float32)
    samples = [_sample(cfg, proc, 100 + i) for i in range(12)]
    opts = [None if i % 2 == 0 else OPTION_SETS[(i // 2) % 3] for i in range(12)]
    seeds = [None if o is None else 1000 + i for i, o in enumerate(opts)]

    def alone(i, **kw):
        o = {} if opts[i] is None else dict(do_sample=True, seed=seeds[i], **opts[i])
        return m.generate(**samples[i], max_new_tokens=NT, **o, **kw).sequences[0].cpu().tolist()
    streams = [alone(i) for i in range(12)]
    eos, lens = _pick_eos(streams, 6, NT)
    assert len(set(lens)) >= 4 and min(lens) <= NT // 3, lens
    exp = [_cut(alone(i, eos_token_id=eos), eos) for i in range(12)]
    assert [len(e) for e in exp] == lens
    greedy = [_cut(m.generate(**samples[i], max_new_tokens=NT, eos_token_id=eos).sequences[0].cpu().tolist(), eos) for i in range(12)]
    return dict(m=m, samples=samples, opts=opts, seeds=seeds, eos=eos, exp=exp, greedy=greedy, NT=NT,
                V=cfg.mllm_config.text_config.vocab_size)


@pytest.mark.parametrize("use_graph", [True, False])
def test_greedy_and_sampled_tickets_share_one_decode_batch(mixed, use_graph):
    from gar_amd.continuous import ContinuousBatcher
    c = mixed
    m, samples, opts, seeds, eos = c["m"], c["samples"], c["opts"], c["seeds"], c["eos"]
    cb = ContinuousBatcher(m, slots=6, max_new_tokens=c["NT"], eos_token_id=eos, sampling=True, poll_every=1, admit_min=1,
                           use_graph=use_graph)
    tickets = [cb.submit(s) if o is None else cb.submit(s, do_sample=True, seed=sd, **o) for s, o, sd in zip(samples, opts, seeds)]
    res = cb.flush()
    assert cb.seeds == {t: sd for t, sd in zip(tickets, seeds) if sd is not None}
    near, total = set(), 0
    for i, t in enumerate(tickets):
        if opts[i] is None:
            assert res[t] == c["exp"][i], (i, res[t], c["exp"][i])                     # (a)
        else:
            near |= {(i, j) for j in _check_against_oracle(m, c["V"], samples[i], res[t], opts[i], seeds[i])}      # (b)
            total += len(res[t])
    print(f"sampled tokens {total}, near the oracle's boundary {sorted(near)}; stats {cb.stats}")
    assert len(near) <= max(1, total // 100), (near, total)
    for i, t in enumerate(tickets):                                                    # (c)
        if opts[i] is not None and res[t] != c["exp"][i]:
            d = next((j for j, (a, b) in enumerate(zip(res[t], c["exp"][i])) if a != b), min(len(res[t]), len(c["exp"][i])))
            assert (i, d) in near, (i, d, res[t], c["exp"][i])
    odd = [i for i in range(12) if opts[i] is not None]
    assert [res[tickets[i]] for i in odd] != [c["greedy"][i] for i in odd]             # (d) it does sample
    assert cb.stats["admitted"] == cb.stats["retired"] == 12                           # (e)


def test_sampled_tickets_through_ragged_prompts_and_rebasing(tiny):
    """the shape of test_admission_of_ragged_prompts_and_rebasing with every ticket sampled: a re-base shifts the token log under the
    live rows, and their col0 with it — a col0 left behind would change the step of every later draw"""
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc = tiny
    B, NT = 4, 40
    V = cfg.mllm_config.text_config.vocab_size
    m = GARModel(cfg, W, torch.float32)
    samples = [_sample(cfg, proc, 200 + i, multi=(i % 3 == 1)) for i in range(16)]
    assert len({int(s["input_ids"].shape[1]) for s in samples}) >= 2
    opts = [OPTION_SETS[i % 3] for i in range(16)]
    seeds = [5000 + i for i in range(16)]
    streams = [m.generate(**s, max_new_tokens=NT, do_sample=True, seed=sd, **o).sequences[0].cpu().tolist()
               for s, o, sd in zip(samples, opts, seeds)]
    eos, lens = _pick_eos(streams, 5, NT)
    cb = ContinuousBatcher(m, slots=B, max_new_tokens=NT, eos_token_id=eos, sampling=True, poll_every=2, admit_min=1, horizon=0,
                           smax_multiple=64)
    tickets = [cb.submit(s, do_sample=True, seed=sd, **o) for s, o, sd in zip(samples, opts, seeds)]
    res = cb.flush()
    near, total = set(), 0
    for i, t in enumerate(tickets):
        near |= {(i, j) for j in _check_against_oracle(m, V, samples[i], res[t], opts[i], seeds[i])}
        total += len(res[t])
    print(f"lengths {lens}; sampled tokens {total}, near {sorted(near)}; stats {cb.stats}; Smax {cb.Smax}")
    assert len(near) <= max(1, total // 100), (near, total)
    assert cb.stats["rebases"] >= 1, cb.stats
    # a draw depends on (key, step, logits) only, so a ticket is also its own free-running stream cut at its first eos
    for i, t in enumerate(tickets):
        want = _cut(streams[i], eos)
        if res[t] != want:
            d = next((j for j, (a, b) in enumerate(zip(res[t], want)) if a != b), min(len(res[t]), len(want)))
            assert (i, d) in near, (i, d, res[t], want)
    assert cb.stats["admitted"] == cb.stats["retired"] == 16


class _count_launches:
    """wraps ops.sample_rows: the row count of every launch"""

    def __init__(self):
        from gar_amd import ops
        self.ops, self.orig, self.shapes = ops, getattr(ops, "sample_rows", None), []

        def counted(logits, *a, **kw):
            self.shapes.append(logits.shape[0])
            return self.orig(logits, *a, **kw)
        ops.sample_rows = counted

    def undo(self):
        self.ops.sample_rows = self.orig


def test_default_path_is_untouched(mixed):
    """a batcher built without ``sampling`` gives every region its greedy single-region run and never launches gar_sample_rows; with
    the flag and greedy tickets only, the same tokens come out of gar_sample_rows' greedy mode — one launch per prompt pass and step"""
    from gar_amd.continuous import ContinuousBatcher
    c = mixed
    m, samples, eos = c["m"], c["samples"], c["eos"]
    counted = _count_launches()
    try:
        for use_graph in (True, False):
            cb = ContinuousBatcher(m, slots=6, max_new_tokens=c["NT"], eos_token_id=eos, poll_every=1, admit_min=1, use_graph=use_graph)
            assert "row_words" not in (cb.st or {})
            tickets = [cb.submit(s) for s in samples]
            res = cb.flush()
            assert [res[t] for t in tickets] == c["greedy"]
            assert "row_words" not in cb.st and counted.shapes == []
        cb = ContinuousBatcher(m, slots=6, max_new_tokens=c["NT"], eos_token_id=eos, sampling=True, poll_every=1, admit_min=1,
                               use_graph=False)
        tickets = [cb.submit(s, do_sample=False) for s in samples]
        res = cb.flush()
        assert [res[t] for t in tickets] == c["greedy"]
        # every decode step picks its 6 rows with one launch, every region's first token comes out of one row of a prompt launch
        assert len(counted.shapes) >= cb.stats["prompt_passes"] + cb.stats["decode_steps"]
        assert sum(counted.shapes) == 6 * cb.stats["decode_steps"] + len(samples)
    finally:
        counted.undo()
