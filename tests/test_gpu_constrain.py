"""GPU (-m gpu): generate(constraint=PhraseConstraint(...)) — gar_constrain against the restatement
tests/constraint_ref.py bit for bit (f32, bf16, fp16 through the twin library): the mask and the node plane, odd shapes, the real
vocabulary, wide nodes, long phrases, idempotence, an inconsistent block between guard regions; and GARModel.generate with a
constraint against a forced replay of the same tokens: greedy and sampled, graph and eager, a ragged left-padded batch with
per-prompt sets, fan-out, with logits_processing, log-probabilities over the masked scores, and the default path untouched."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import constraint_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SENTINEL, GUARD = 12345.0, 64
OTHER = 3           # the id in the token matrix's columns behind the history: it would change the walk if it were read


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "constraint.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def _logits(B, V, ld, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + V)
    x = torch.full((B, ld), SENTINEL, dtype=dtype)
    x[:, :V] = (torch.randn(B, V, generator=g) * 2.5).to(dtype)
    return x


def _guarded(t, fill):
    """a device copy of ``t`` inside a flat buffer with GUARD elements of ``fill`` on both sides: (view, whole buffer)"""
    flat = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype)
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1)
    d = flat.cuda()
    return d[GUARD:GUARD + t.numel()].view(t.shape), d


def _guards_intact(buf, fill):
    h = buf.cpu()
    return bool((h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all())


def _launch(x, V, words, hists, eos, step_dev=True, roots=None, launches=1):
    """gar_constrain on a device copy of ``x`` [B, ld] at step t = len(hists[b]): the node plane is walked launch by launch from
    column 1 (on scratch logits), then the step itself runs ``launches`` times on the copy. The histories sit in a token
    matrix wider than t whose other columns hold OTHER. Every buffer lies between guard regions. Returns (logits, plane) on the
    host."""
    from gar_amd import ops
    B, t = len(hists), len(hists[0])
    cols = t + 5
    toks = torch.full((B, cols), OTHER, dtype=torch.int64)
    if t:
        toks[:, :t] = torch.tensor(hists, dtype=torch.int64)
    toks_d, toks_buf = _guarded(toks, -7)
    trie_d, trie_buf = _guarded(torch.tensor(words, dtype=torch.int32), 2 ** 30)     # a huge index on both sides of the block
    plane = torch.full((B, cols + 1), -5, dtype=torch.int32)
    plane[:, 0] = torch.tensor(words[4:4 + B] if roots is None else roots, dtype=torch.int32)
    plane_d, plane_buf = _guarded(plane, -9)
    eos_d, eos_buf = _guarded(torch.tensor(list(eos), dtype=torch.int64), V - 1)
    xd, x_buf = _guarded(x, 768.0)
    step = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    scratch = x.cuda()
    for s in range(1, t):           # the steps before t, as the decode loop ran them
        step.fill_(s)
        ops.constrain(scratch, V, toks_d, step, eos_d, trie_d, plane_d)
    step.fill_(t)
    for _ in range(launches):
        ops.constrain(xd, V, toks_d if (t or step_dev) else None, step if step_dev else None, eos_d, trie_d, plane_d)
    torch.cuda.synchronize()
    assert _guards_intact(toks_buf, -7) and _guards_intact(trie_buf, 2 ** 30) and _guards_intact(plane_buf, -9)
    assert _guards_intact(eos_buf, V - 1) and _guards_intact(x_buf, 768.0)
    assert torch.equal(toks_d.cpu(), toks) and torch.equal(trie_d.cpu(), torch.tensor(words, dtype=torch.int32))
    return xd.cpu(), plane_d.cpu()


def _check(x, V, sets, hists, eos, words=None, **kw):
    from gar_amd import PhraseConstraint
    B = len(hists)
    words = words or PhraseConstraint(sets).pack(V, B)
    per = sets if isinstance(sets[0][0], (list, tuple)) else [sets] * B
    got, plane = _launch(x, V, words, hists, eos, **kw)
    want = R.mask(per, hists, x, V, eos)
    assert torch.equal(_bits(got), _bits(want)), (hists, (got != want).nonzero().tolist()[:8])
    assert (got[:, V:] == SENTINEL).all()
    t = len(hists[0])
    for b in range(B):
        assert [int(v) for v in plane[b, :t + 1]] == [R.walk(words, b, hists[b][:j], V) for j in range(t + 1)], (b, plane[b])
        assert (plane[b, t + 1:] == -5).all()           # columns behind the step are not the launch's
    return got, plane


SETS = [[[5, 6], [5, 6, 7], [9], [5, 6]], [[3, 4, 8, 10, 11, 12, 13, 14]], [[20, 21, 22], [20, 30], [31], [20, 21]]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,ld", [(1000, 1024), (1003, 1024), (37, 64)])
def test_kernel_equals_restatement_bit_for_bit(dtype, V, ld):
    """B = 3 with per-prompt sets at steps 0..5: histories that follow a phrase, end one (terminal and a prefix of another), leave
    the trie, run behind a phrase's eos (the eos-only state) and hold ids outside [0, V); V = 1003: the last bitmap byte and the
    last 16-byte piece are partial; step_dev NULL and as a device value at step 0; 1 and 2 eos ids; columns V..ld-1 survive."""
    from gar_amd import hip
    hip.require_device(0)
    x = _logits(3, V, ld, dtype)
    for eos in ([2], [2, 33]):
        _check(x, V, SETS, [[], [], []], eos, step_dev=False)
        for hists in ([[], [], []],
                      [[5], [3], [20]], [[9], [4], [31]],
                      [[5, 6], [3, 4], [20, 21]], [[9, 2], [3, 9], [20, 30]],
                      [[5, 6, 7], [3, 4, 8], [20, 21, 22]], [[5, 6, 2], [3, 4, OTHER], [20, 30, 33]],
                      [[5, 6, 7, 2], [3, 4, 8, 10], [V, 21, 22, 2]], [[5, 6, 2, 0], [3, 4, 8, -1], [20, 21, 2 ** 40, 22]],
                      [[5, 6, 7, 2, 0], [3, 4, 8, 10, 11], [20, 21, 22, 33, 0]]):
            _check(x, V, SETS, hists, eos)
    # a shared set, and an unaligned base: the row starts one element behind a 16-byte boundary
    shared = [[5, 6], [5, 6, 7], [9]]
    _check(x, V, shared, [[5, 6], [9, 2], [7, 7]], [2])
    from gar_amd import PhraseConstraint, ops
    wide = torch.full((3, ld + 8), SENTINEL, dtype=dtype)
    wide[:, 1:1 + V] = x[:, :V]
    wd = wide.cuda()
    view = wd[:, 1:]            # data_ptr one element on, row stride ld + 8
    words = PhraseConstraint(shared).pack(V, 3)
    plane = torch.zeros((3, 2), dtype=torch.int32, device="cuda:0")
    ops.constrain(view, V, None, None, torch.tensor([2], device="cuda:0"), torch.tensor(words, dtype=torch.int32, device="cuda:0"), plane)
    torch.cuda.synchronize()
    got = wd.cpu()
    assert torch.equal(_bits(got[:, 1:1 + V]), _bits(R.mask([shared] * 3, [[]] * 3, x, V, [2])[:, :V]))
    assert (got[:, 0] == SENTINEL).all() and (got[:, 1 + V:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_at_the_real_vocabulary(dtype):
    """B = 2 at V = 128256 (ld = V + 64): ids over the whole range, the first and the last id among them"""
    from gar_amd import hip
    hip.require_device(0)
    V = 128256
    x = _logits(2, V, V + 64, dtype)
    sets = [[0, V - 1], [0, 31, 32], [V - 1], [70000, 4095, 63], [128000], [0, V - 1, 64]]
    _check(x, V, sets, [[], []], [128001, 128009])
    _check(x, V, sets, [[0], [70000]], [128001, 128009])
    _check(x, V, sets, [[0, V - 1], [V - 1, 128009]], [128001, 128009])


def test_kernel_along_the_golden_sets():
    """the golden cases (V = 37 in ld = 64, f32): HF's raw logits in, HF's scores out, bit for bit, at every step of every case"""
    from gar_amd import hip
    hip.require_device(0)
    g, meta = _golden()
    V, n = meta["vocab"], 0
    for i, c in enumerate(meta["cases"]):
        raw, scores, seq = torch.from_numpy(g[f"raw{i}"]), torch.from_numpy(g[f"scores{i}"]), g[f"seq{i}"].astype(np.int64).tolist()
        for t in range(raw.shape[0]):
            x = torch.full((c["batch"], 64), SENTINEL)
            x[:, :V] = raw[t]
            got, _ = _check(x, V, c["sets"] if c["per_prompt"] else c["sets"][0], [r[:t] for r in seq], c["eos"])
            assert torch.equal(_bits(got[:, :V]), _bits(scores[t])), (i, t)
            n += 1
    assert n >= 30


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_wide_nodes_long_phrases_and_idempotence(dtype):
    """a root with 1500 children (more than the workgroup has threads) and a phrase of 40 tokens walked to its end, V = 2000 in
    ld = 2048; a second launch at the same step leaves the plane and the logits unchanged"""
    from gar_amd import hip
    hip.require_device(0)
    V = 2000
    x = _logits(2, V, 2048, dtype)
    long = [1999 - j for j in range(40)]
    sets = [[i] for i in range(0, 1500)] + [long] + [[1700, 5], [1700, 1999]]
    _check(x, V, sets, [[], []], [1600])
    _check(x, V, sets, [[1499], [1700]], [1600])
    for t in (1, 17, 39, 40):
        _check(x, V, sets, [long[:t], long[:t - 1] + [7]], [1600])
    once, p1 = _check(x, V, sets, [long[:2], [1700, 5]], [1600], launches=1)
    twice, p2 = _check(x, V, sets, [long[:2], [1700, 5]], [1600], launches=2)
    assert torch.equal(_bits(once), _bits(twice)) and torch.equal(p1, p2)


def test_inconsistent_blocks_give_eos_only_rows_and_stay_in_bounds():
    """a child index above n_nodes, an edge range above n_edges, sizes that do not fit the block, a root outside the table: the rows
    that meet them get eos only, nothing outside the buffers is touched (the guard regions of _launch) and nothing is followed"""
    from gar_amd import PhraseConstraint, hip
    hip.require_device(0)
    V = 1000
    x = _logits(3, V, 1024, torch.float32)
    sets = [[5, 6], [5, 6, 7], [9]]
    good = PhraseConstraint(sets).pack(V, 3)
    n_nodes, n_edges, root, first, tok, child, term = R.block_arrays(good)
    eos_only = R.mask([[[1]]] * 3, [[OTHER]] * 3, x, V, [2])           # a history that is no prefix: exactly the eos ids
    o_first = 4 + 3
    o_child = o_first + n_nodes + 1 + n_edges

    def run(words, hists, roots=None):
        got, plane = _launch(x, V, words, hists, [2], roots=roots)
        return got, plane

    # child of the edge (root, 5) above n_nodes: the walk behind 5 names DEAD
    bad = list(good)
    e = first[root[0]] + tok[first[root[0]]:first[root[0] + 1]].index(5)
    bad[o_child + e] = n_nodes + 1000
    got, plane = run(bad, [[5], [5], [9]])
    assert plane[:2, 1].tolist() == [-1, -1] and plane[2, 1] >= 0
    assert torch.equal(_bits(got[:2]), _bits(eos_only[:2])) and torch.equal(_bits(got[2]), _bits(R.mask_row(sets, [9], x[2], V, [2])))
    # the edge range of the root above n_edges (and a negative start): no child is marked, the row is not terminal: nothing allowed
    for lo, hi in ((0, n_edges + 10 ** 6), (-4, 2)):
        bad = list(good)
        bad[o_first + root[0]], bad[o_first + root[0] + 1] = lo, hi
        got, _ = run(bad, [[], [], []])
        assert torch.isneginf(got[:, :V]).all() and (got[:, V:] == SENTINEL).all()
        got, plane = run(bad, [[5], [5], [5]])
        assert plane[:, 1].tolist() == [-1] * 3 and torch.equal(_bits(got), _bits(eos_only))
    # sizes that do not fit the block: no node exists
    for k, v in ((0, 10 ** 6), (1, 2 ** 31 - 1), (0, -1), (2, 10 ** 6)):
        bad = list(good)
        bad[k] = v
        got, _ = run(bad, [[], [], []])
        assert torch.equal(_bits(got), _bits(eos_only))
    # a root outside the node table
    got, _ = run(good, [[], [], []], roots=[n_nodes, -3, root[2]])
    assert torch.equal(_bits(got[:2]), _bits(eos_only[:2])) and torch.equal(_bits(got[2]), _bits(R.mask_row(sets, [], x[2], V, [2])))


# ---- end to end on the tiny fixture ---------------------------------------------------------------------------------------------
NT = 6
E2E_SETS = [[[5, 6], [5, 6, 7], [9], [5, 6], [300, 301]], [[3, 4, 8, 10, 11, 12, 13, 14]], [[20, 21, 22], [20, 30], [31], [20, 21], [400]]]
SAMPLING = dict(do_sample=True, temperature=1.5, top_p=0.95, top_k=50)


@functools.lru_cache(maxsize=None)
def _shared():
    import test_gpu_logprobs as T
    cfg, W, proc, batch, ragged = T._setup()
    return T, cfg, ragged


@functools.lru_cache(maxsize=None)
def _plain(dtype):
    """plain greedy on the ragged batch, made before any constrained request on the model of that dtype"""
    T, cfg, ragged = _shared()
    return T._model(dtype).generate(**ragged, max_new_tokens=NT).sequences.cpu()


class _count_launches:
    """wraps ops.constrain: the row count of every launch"""

    def __init__(self):
        from gar_amd import ops
        self.ops, self.orig, self.shapes = ops, ops.constrain, []

        def counted(logits, *a, **kw):
            self.shapes.append(logits.shape[0])
            return self.orig(logits, *a, **kw)
        ops.constrain = counted

    def undo(self):
        self.ops.constrain = self.orig


def _ends(seq, eos):
    """per row: tokens up to and including its first eos"""
    return [next((j + 1 for j, tk in enumerate(r) if tk in eos), len(r)) for r in seq]


def _check_run(m, batch, out, sets, eos, V, N=1, greedy=True, P=None, replay=True):
    """what every constrained run has to satisfy, from its sequences and its returned scores. Returns the rows' phrase indices."""
    import logits_process_ref as LP
    seq = out.sequences.cpu().tolist()
    n = len(seq[0])
    scores = out.logits.cpu()[:, :n]
    ends = _ends(seq, eos)
    # the tokens the device fed back behind a row's first eos: its own pick among the eos ids (`sequences` holds pad there)
    fed = [list(r) for r in seq]
    for r, row in enumerate(fed):
        for t in range(ends[r], n):
            row[t] = eos[0] if len(eos) == 1 else R.first_argmax(scores[r, t])
    raw = None
    if replay:
        rep = m.generate(**batch, max_new_tokens=n, forced_tokens=torch.tensor(fed), return_logits=True, use_graph=False)
        raw = rep.logits.cpu()
    idx = []
    for r, row in enumerate(seq):
        phrases = sets[r // N]
        for t in range(n):
            ok = R.allowed_ids(phrases, row[:t], V, eos)
            if P is not None:       # a processor's ban stays -inf under the mask
                ok -= LP.banned_ids(fed[r][:t], V, P, eos)
            fin = torch.isfinite(scores[r, t])
            assert set(fin.nonzero().reshape(-1).tolist()) == ok, (r, t)
            assert torch.isneginf(scores[r, t][~fin]).all()
            if raw is not None:
                want = raw[r, t] if P is None else LP.process_row(fed[r][:t], raw[r, t], V, P, eos).float()
                assert torch.equal(scores[r, t][fin], want[fin]), (r, t)
            if t < ends[r]:
                assert row[t] in ok, (r, t)
                if greedy:
                    assert row[t] == R.first_argmax(scores[r, t]), (r, t)
        head = row[:ends[r] - 1] if row[ends[r] - 1] in eos else row
        i = R.phrase_index(phrases, row, eos)
        assert head in [list(p) for p in phrases] or (ends[r] == n and row[n - 1] not in eos), (r, row)    # a phrase, or cut inside one
        idx.append(i)
    assert out.phrase_index.dtype == torch.int32 and out.phrase_index.tolist() == idx
    return idx


@pytest.mark.parametrize("dtype", DTYPES)
def test_generate_greedy_constrained_against_forced_replay(dtype):
    """a ragged left-padded batch of 3 with per-prompt sets, greedy, two eos ids, eager: the scores are -inf exactly outside the
    set the restatement derives from the sequences, their finite entries are bit for bit the logits of the forced replay without
    a constraint, every token is the argmax of its masked row, every row ends in one of its phrases (prompt 1's only phrase is
    longer than max_new_tokens: cut, phrase_index -1), the graph run returns the same tokens and scores"""
    T, cfg, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(dtype)
    plain = _plain(dtype)
    eos = [2, 33]
    kw = dict(max_new_tokens=NT, eos_token_id=eos, pad_token_id=0, constraint=dict(phrases=E2E_SETS), return_logits=True)
    out = m.generate(**ragged, **kw, use_graph=False)
    idx = _check_run(m, ragged, out, E2E_SETS, eos, V)
    assert idx[1] == -1 and idx[0] >= 0 and idx[2] >= 0
    assert out.sequences.cpu()[1].tolist() == E2E_SETS[1][0][:NT]
    graph = m.generate(**ragged, **kw)
    assert torch.equal(graph.sequences, out.sequences) and torch.equal(graph.phrase_index, out.phrase_index)
    assert torch.equal(_bits(graph.logits.float().cpu()), _bits(out.logits.float().cpu()))
    # the default path afterwards: the tokens of the run made before any constrained request
    assert torch.equal(m.generate(**ragged, max_new_tokens=NT).sequences.cpu(), plain)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_sampled_constrained(dtype):
    """do_sample on the ragged batch, one eos id: every sampled token is allowed, the scores and their finite entries as in the
    greedy test, graph == eager for the same seed"""
    from gar_amd import PhraseConstraint
    T, cfg, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(dtype)
    pc = PhraseConstraint(E2E_SETS)
    kw = dict(SAMPLING, max_new_tokens=NT, eos_token_id=2, pad_token_id=0, constraint=pc, return_logits=True)
    for seed in (11, 12, 13):
        out = m.generate(**ragged, **kw, seed=seed, use_graph=False)
        _check_run(m, ragged, out, E2E_SETS, [2], V, greedy=False, replay=seed == 11)
        assert torch.equal(m.generate(**ragged, **kw, seed=seed).sequences, out.sequences)


def test_fanout_with_processing_and_logprobs_over_the_masked_scores():
    """f32, num_return_sequences = 3, do_sample. With logits_processing: the mask runs behind the processors (finite entries = the
    restated processors on the forced replay of the replicated batch), fan-out rows of prompt b use prompt b's set, one launch on
    the prompts' rows, then one per step on all rows. With return_logprobs / top_logprobs (not combined with logits_processing,
    7.7): token_logprobs are log_softmax of the returned masked scores at the chosen tokens (the tolerance of test_gpu_logprobs),
    sum_logprobs their sum, top_logprobs beyond the allowed ids are -inf by ascending id"""
    from logprob_ref import LP_TOL, raw_logprob_at
    from test_gpu_fanout import _repeat
    T, cfg, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(torch.float32)
    N, eos = 3, [2]
    kw = dict(SAMPLING, num_return_sequences=N, seed=5, max_new_tokens=NT, eos_token_id=eos, pad_token_id=0,
              constraint=dict(phrases=E2E_SETS))
    P = dict(repetition_penalty=1.3, suppress_tokens=[7])           # 7: the longer phrase of prompt 0 can no longer be taken
    c = _count_launches()
    try:
        out = m.generate(**ragged, **kw, logits_processing=P, return_logits=True, use_graph=False)
        n = out.sequences.shape[1]
        assert c.shapes[0] == 3 and all(s == 3 * N for s in c.shapes[1:]) and len(c.shapes) >= n
    finally:
        c.undo()
    assert tuple(out.sequences.shape) == (3 * N, n)
    _check_run(m, _repeat(ragged, N), out, E2E_SETS, eos, V, N=N, greedy=False, P=P)
    assert all(7 not in r for r in out.sequences.tolist())
    assert torch.equal(m.generate(**ragged, **kw, logits_processing=P).sequences, out.sequences)
    # log-probabilities over the masked scores
    out = m.generate(**ragged, **kw, return_logits=True, return_logprobs=True, top_logprobs=4, use_graph=False)
    n = out.sequences.shape[1]
    _check_run(m, _repeat(ragged, N), out, E2E_SETS, eos, V, N=N, greedy=False)
    seq = out.sequences.cpu()
    ends = _ends(seq.tolist(), eos)
    ref = raw_logprob_at(out.logits[:, :n], out.sequences)
    tlp = out.token_logprobs.cpu()
    for r in range(3 * N):
        e = ends[r]
        assert float((tlp[r, :e].double() - ref[r, :e]).abs().max()) <= LP_TOL, r
        assert not tlp[r, e:].any() and int(out.n_tokens[r]) == e
        tol = e * 2.0 ** -23 * max(1.0, float(tlp[r, :e].abs().sum()))         # a float32 sum of e terms, as test_gpu_logprobs bounds it
        assert abs(float(out.sum_logprobs[r]) - float(tlp[r, :e].double().sum())) <= tol
        assert abs(float(out.sum_logprobs[r]) - float(ref[r, :e].sum())) <= tol + e * LP_TOL
        for t in range(e):
            ok = sorted(R.allowed_ids(E2E_SETS[r // N], seq[r, :t].tolist(), V, eos))
            ids, lps = out.top_logprob_ids[r, t].tolist(), out.top_logprobs[r, t].tolist()
            k = min(4, len(ok))
            assert set(ids[:k]) <= set(ok) and len(set(ids[:k])) == k and (len(ok) > 4 or set(ids[:k]) == set(ok)), (r, t, ids, ok)
            assert all(np.isfinite(v) for v in lps[:k]) and all(v == float("-inf") for v in lps[k:]), (r, t, lps)
            rest = ids[k:]          # k above the number of allowed ids: -inf entries by ascending id
            assert rest == sorted(rest) and not set(rest) & set(ok), (r, t, ids)
    graph = m.generate(**ragged, **kw, return_logprobs=True)
    assert torch.equal(graph.sequences, out.sequences) and torch.equal(graph.token_logprobs, out.token_logprobs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_default_path_is_untouched(dtype):
    """without the parameter and with None: the sequences of a run made before any constrained request on the same model, no
    gar_constrain launch, no new captured graph; a constrained request launches it once per token; one captured step serves
    another phrase set"""
    T, cfg, ragged = _shared()
    m = T._model(dtype)
    before = _plain(dtype)
    c = _count_launches()
    try:
        out = m.generate(**ragged, max_new_tokens=NT, eos_token_id=2, constraint=dict(phrases=[[5, 6, 7, 8, 9, 10, 11]]), use_graph=False)
        assert c.shapes == [3] * NT and out.sequences.cpu().tolist() == [[5, 6, 7, 8, 9, 10]] * 3
        assert out.phrase_index.tolist() == [-1] * 3
        a = m.generate(**ragged, max_new_tokens=NT, eos_token_id=2, constraint=dict(phrases=[[5, 6], [9]]))
        n_graphs = len(m._graphs)
        b = m.generate(**ragged, max_new_tokens=NT, eos_token_id=2, constraint=dict(phrases=[[[40, 41, 42]], [[50]], [[60, 61]]]))
        assert len(m._graphs) == n_graphs
        assert b.sequences.cpu().tolist() == [[40, 41, 42, 2], [50, 2, 2, 2], [60, 61, 2, 2]] and b.phrase_index.tolist() == [0, 0, 0]
        assert all(i >= 0 for i in a.phrase_index.tolist())
        del c.shapes[:]
        m.generate(**ragged, max_new_tokens=NT)
        n_graphs = len(m._graphs)
        for kw in ({}, dict(constraint=None), dict(use_graph=False), dict(constraint=None, use_graph=False)):
            assert torch.equal(m.generate(**ragged, max_new_tokens=NT, **kw).sequences.cpu(), before), kw
        assert c.shapes == [] and len(m._graphs) == n_graphs
    finally:
        c.undo()


def test_fp8_modes_carry_the_constraint():
    """the FP8 KV cache and the FP8 decode weights never see logits: every row is one of its phrases"""
    from gar_amd.modeling_gar import GARModel
    T, cfg, ragged = _shared()
    W = T._setup()[1]
    sets = [E2E_SETS[0], E2E_SETS[2], E2E_SETS[0]]
    for kw in (dict(kv_cache_dtype="fp8"), dict(decode_weight_dtype="fp8")):
        out = GARModel(cfg, W, torch.bfloat16, "cuda:0", **kw).generate(**ragged, max_new_tokens=NT, eos_token_id=2,
                                                                         constraint=dict(phrases=sets))
        for b, (row, i) in enumerate(zip(out.sequences.cpu().tolist(), out.phrase_index.tolist())):
            assert i >= 0 and row[:len(sets[b][i]) + 1] == list(sets[b][i]) + [2], (kw, b, row)


def test_gar_bench_constrain_options(tmp_path):
    """evaluation/GAR-Bench/inference.py --mode vqa --constrain_options on a synthetic annotation file with the stub tokenizer: three
    items with different option sets — one of them with letters of two tokens — run as ONE generate (per-prompt sets); every
    record's model_output is one of its item's letters and option_pick names it"""
    import re
    from gar_amd import rle
    from gar_amd.synthetic import synthetic_disjoint_masks, synthetic_image
    from test_gpu_bench_loops import _run
    os.makedirs(tmp_path / "images")
    letters = [["A", "B"], ["AA", "AB", "C"], ["X", "Y"]]
    items = []
    for i, ls in enumerate(letters):
        synthetic_image(40 + i, 260, 200).save(tmp_path / "images" / f"c_{i}.png")
        masks = synthetic_disjoint_masks(40 + i, 2, 260, 200)
        items.append({"image": f"images/c_{i}.png", "mask_rles": [rle.encode(m) for m in masks],
                      "question": "Which one is larger, <Prompt0> or <Prompt1>?",
                      "choices": [f"{l}. <Prompt{k % 2}>" for k, l in enumerate(ls)], "answer": ls[0], "type": "size"})
    anno = tmp_path / "c.json"
    json.dump(items, open(anno, "w"))
    out = _run("GAR-Bench", "--anno_file", str(anno), "--image_folder", str(tmp_path), "--mode", "vqa", "--cache_name", "c",
               "--output_dir", str(tmp_path / "out"), "--batch_size", "4", "--constrain_options")
    res = json.load(open(tmp_path / "out" / "c_vqa.json"))
    assert re.search(r"\[batcher\] 3 items in 1 generate calls", out)
    assert [r["image"] for r in res] == [it["image"] for it in items]
    for r, ls in zip(res, letters):
        assert r["option_pick"] in ls and r["model_output"] == r["option_pick"], r
    assert json.load(open(tmp_path / "out" / "c_vqa.meta.json"))["constrain_options"] is True


def test_demo_choices(tmp_path):
    """demo/gar_with_mask.py --choices: the printed line is one of the choices; with --return_logprobs it stands behind its
    probability among the choices, which is in (0, 1]"""
    import re
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    from test_gpu_demo import _run
    from PIL import Image
    ip, mp = str(tmp_path / "img.png"), str(tmp_path / "mask.png")
    synthetic_image(11, 300, 220).save(ip)
    Image.fromarray(synthetic_mask(11, 300, 220).astype(np.uint8) * 255).save(mp)
    choices = ["a cat", "a dog", "a cathedral", "tree"]
    out = _run("gar_with_mask.py", "--image_path", ip, "--mask_path", mp, "--choices", ",".join(choices), "--return_logprobs")
    m = re.fullmatch(r"\[([0-9.]+)\] (.+)", out)
    assert m and m.group(2) in choices and 0.0 < float(m.group(1)) <= 1.0, out
