"""GPU (-m gpu): generate(sampling_warpers=...) — gar_sample_ext (min_p / typical_p / epsilon / eta cutoff between top-p and the
draw) against tests/sampling_warpers_ref.py on the same logits, and GARModel.generate against the restatement's draw
from the logits the run itself returns.

Rules, per row, with the restatement's kept and AMBIGUOUS ids (tokens within the 1e-4 band of a cut):
  (a) every row: the token lies in kept | ambiguous, and |kept - ambiguous| <= n_kept <= |kept | ambiguous|;
  (b) a row with no ambiguous token: n_kept is the restatement's count, and the token is the restatement's draw, or its neighbour in
      the kept set when the draw lies within MARGIN = 2e-5 of the boundary — at most max(1, 1 %) of those draws
      (tests/test_gpu_sampling.py's rule and cap)."""
import functools

import numpy as np
import pytest
import torch

import sampling_warpers_ref as R
from logprob_ref import LP_TOL

pytestmark = pytest.mark.gpu

MARGIN = 2e-5
SENTINEL = 12345.0
SET7 = R.PARAM_SETS[6]


def _params8(ps):
    t, k, p, mp, typ, eps, eta = ps
    return [t, p, float(k), 0.0, mp, typ, eps, eta]


def _run_ext(logits, V, ps, seed, step, lp=False, eos=None, step_dev=True):
    """gar_sample_ext on logits [B, ld >= V]: (tokens, n_kept, planes or None, latches)"""
    from gar_amd import ops
    B = logits.shape[0]
    dev = logits.device
    out = torch.full((B, 8), -1, dtype=torch.int64, device=dev)
    cur = torch.zeros(B, dtype=torch.int64, device=dev)
    stepd = torch.tensor([step], dtype=torch.int32, device=dev) if step_dev else None
    params = torch.tensor(_params8(ps), dtype=torch.float32, device=dev)
    seedd = torch.tensor([seed], dtype=torch.int64, device=dev)
    nk = torch.full((B,), -7, dtype=torch.int32, device=dev)
    kw = {}
    if eos is not None:
        kw = dict(eos_ids=torch.tensor(eos, dtype=torch.int64, device=dev), finished=torch.full((B,), -1, dtype=torch.int32, device=dev),
                  done_count=torch.zeros(1, dtype=torch.int32, device=dev))
    planes = None
    if lp:
        planes = [torch.full((B, 8), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
        kw.update(logprobs=planes[0], logprobs_warped=planes[1])
    ops.sample_ext(logits, V, out, out.stride(0), stepd, cur, params, seedd, n_kept=nk, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out[:, step if step_dev else 0], cur)
    return cur.cpu().tolist(), nk.cpu().tolist(), None if planes is None else [p.cpu() for p in planes], kw


def _run_plain(logits, V, t, k, p, seed, step, lp=False):
    from gar_amd import ops
    B = logits.shape[0]
    dev = logits.device
    out = torch.full((B, 8), -1, dtype=torch.int64, device=dev)
    cur = torch.zeros(B, dtype=torch.int64, device=dev)
    planes, kw = None, {}
    if lp:
        planes = [torch.full((B, 8), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
        kw = dict(logprobs=planes[0], logprobs_warped=planes[1])
    ops.sample(logits, V, out, out.stride(0), torch.tensor([step], dtype=torch.int32, device=dev), cur,
               torch.tensor([t, p, float(k), 0.0], dtype=torch.float32, device=dev), torch.tensor([seed], dtype=torch.int64, device=dev), **kw)
    torch.cuda.synchronize()
    return cur.cpu().tolist(), None if planes is None else [p.cpu() for p in planes]


class _Tally:
    """rule (b)'s cap and what the run saw, over the launches of one test"""

    def __init__(self):
        self.near = self.clean = self.amb_rows = self.amb_differ = 0
        self.worst = 0.0            # largest band distance at which device and restatement were seen to decide differently

    def check_row(self, lg_row, V, ps, kept, amb, tok, n_kept, seed, row, step, where):
        from oracle import sampling as S
        ks, as_ = set(kept.tolist()), set(amb.tolist())
        assert tok in ks | as_, (where, tok, "token outside kept | ambiguous")
        assert len(ks - as_) <= n_kept <= len(ks | as_), (where, n_kept, len(ks), len(as_))
        if as_:
            self.amb_rows += 1
            if n_kept != len(ks) or tok not in ks:
                # which ambiguous tokens the device decided the other way is not observable; the |difference| nearest ones are the
                # likeliest, so their largest distance is what is recorded
                t, k, p, mp, typ, eps, eta = ps
                dist = R.warp_ext(lg_row, t, min(k, V), p, mp, typ, eps, eta, with_distance=True)[3]
                d = np.sort(dist[amb])[max(abs(n_kept - len(ks)), 1) - 1]
                self.amb_differ += 1
                self.worst = max(self.worst, float(d))
            return
        assert n_kept == len(ks), (where, n_kept, len(ks))
        keep = np.zeros(V, dtype=bool)
        keep[kept] = True
        z = (lg_row / np.float32(ps[0])).astype(np.float32)
        exp, margin = S.draw(z, keep, S.uniform(seed, row, step))
        self.clean += 1
        if tok != exp:
            i, j = int(np.searchsorted(kept, tok)), int(np.searchsorted(kept, exp))
            assert margin < MARGIN and abs(i - j) == 1, (where, tok, exp, margin)
            self.near += 1

    def finish(self, what):
        print(f"{what}: {self.clean} unambiguous draws, {self.near} at a neighbouring boundary; {self.amb_rows} ambiguous rows, "
              f"{self.amb_differ} decided differently, largest band distance of those {self.worst:.3g}")
        assert self.near <= max(1, self.clean // 100), (self.near, self.clean)


_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


@pytest.mark.parametrize("dtype_name", R.DTYPES)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_sample_ext_kernel_equals_restatement(name, dtype_name):
    from gar_amd import hip
    hip.require_device(0)
    lg, sets = R.group(name, dtype_name)
    B, V = lg.shape
    x = torch.full((B, V + 24), SENTINEL, dtype=_DT[dtype_name])           # a padded leading dimension: columns V.. are never read
    x[:, :V] = torch.from_numpy(lg).to(_DT[dtype_name])
    assert torch.equal(x[:, :V].float(), torch.from_numpy(lg))
    x = x.to("cuda:0")
    tally = _Tally()
    for si, ps in enumerate(R.PARAM_SETS):
        ps = (ps[0], min(ps[1], V)) + ps[2:]
        for seed, step in R.SEEDS_STEPS:
            toks, nk, _, _ = _run_ext(x, V, ps, seed, step)
            for b in range(B):
                kept, amb = sets[si][b]
                tally.check_row(lg[b], V, ps, kept, amb, toks[b], nk[b], seed, b, step, (name, dtype_name, si, seed, step, b))
    assert torch.equal(x[:, V:].cpu(), torch.full((B, 24), SENTINEL, dtype=_DT[dtype_name]))
    tally.finish(f"{name} {dtype_name}")


def test_sample_ext_dense_flat_rows():
    """V = 128256 flat: the cuts fall into dense runs of tokens (up to 33 of 80 rows ambiguous, up to 215 ids in a row), so rule
    (a) only — sets 3, 6 and 8, whose typical_p / eta cuts exercise the deep levels of the descent"""
    from gar_amd import hip
    hip.require_device(0)
    V = 128256
    g = torch.Generator().manual_seed(V)
    lg = (torch.randn(8, V, generator=g) * 2.5).numpy()
    x = torch.from_numpy(lg).to("cuda:0")
    seen_amb = differ = 0
    worst = 0.0
    for si in (2, 5, 7):
        ps = R.PARAM_SETS[si]
        toks, nk, _, _ = _run_ext(x, V, ps, 1, 0)
        for b in range(8):
            _, keep, amb, dist = R.warp_ext(lg[b], *ps, with_distance=True)
            ks, as_ = set(np.flatnonzero(keep).tolist()), set(np.flatnonzero(amb).tolist())
            assert toks[b] in ks | as_, (si, b, toks[b])
            assert len(ks - as_) <= nk[b] <= len(ks | as_), (si, b, nk[b], len(ks), len(as_))
            seen_amb += bool(as_)
            if nk[b] != len(ks):            # the |difference| ambiguous ids nearest a cut are the likeliest to have gone the other way
                differ += 1
                worst = max(worst, float(np.sort(dist[amb])[abs(nk[b] - len(ks)) - 1]))
    print(f"dense flat rows with an ambiguous token: {seen_amb} of 24; n_kept differs from the restatement's in {differ}, largest band "
          f"distance of those {worst:.3g}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [128256, 1000, 37])
def test_all_four_off_is_gar_sample_bit_for_bit(dtype, V):
    from gar_amd import hip
    hip.require_device(0)
    g = torch.Generator().manual_seed(V)
    B = 8
    logits = (torch.randn(B, V, generator=g) * 2.5).to(dtype).to("cuda:0")
    for t, k, p in [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.6, 40, 0.8), (1.0, 5, 0.5), (2.0, 20000, 0.999)]:
        k = min(k, V)
        for seed, step in R.SEEDS_STEPS:
            off = (t, k, p, 0.0, 1.0, 0.0, 0.0)
            want, _ = _run_plain(logits, V, t, k, p, seed, step)
            got, nk, _, _ = _run_ext(logits, V, off, seed, step)
            assert got == want, (t, k, p, seed, step)
            assert all(1 <= n <= V for n in nk)
            if (t, k, p) == (1.0, 0, 1.0):
                assert nk == [V] * B
            if k == 5:
                assert all(n <= 5 for n in nk)
        want, wp = _run_plain(logits, V, t, k, p, 77, 2, lp=True)
        got, _, gp, _ = _run_ext(logits, V, (t, k, p, 0.0, 1.0, 0.0, 0.0), 77, 2, lp=True)
        assert got == want
        for a, b in zip(gp, wp):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_sample_ext_kernel_properties():
    from gar_amd import hip, ops
    from oracle import sampling as S
    hip.require_device(0)
    g = torch.Generator().manual_seed(3)
    B, V = 16, 4096
    logits = (torch.randn(B, V, generator=g) * 3.0).to("cuda:0")
    am = logits.argmax(1).cpu().tolist()
    # min_p = 1 and epsilon = 0.9 (no token of these rows holds 90 %) leave the most likely token whatever the draw
    for ps in [(1.0, 0, 1.0, 1.0, 1.0, 0.0, 0.0), (1.0, 0, 1.0, 0.0, 1.0, 0.9, 0.0)]:
        toks, nk, _, _ = _run_ext(logits, V, ps, 5, 0)
        assert toks == am and nk == [1] * B
    # the same (seed, step) repeats; another seed or step moves some rows
    a, nka, _, _ = _run_ext(logits, V, SET7, 42, 2)
    assert _run_ext(logits, V, SET7, 42, 2)[:2] == (a, nka)
    wide = (1.0, 0, 1.0, 0.0, 0.9, 0.0, 1e-4)
    w = _run_ext(logits, V, wide, 42, 2)[0]
    assert _run_ext(logits, V, wide, 43, 2)[0] != w and _run_ext(logits, V, wide, 42, 3)[0] != w
    # suppressed tokens (-inf) are never drawn or counted; a row with ONE finite logit returns it
    lg = torch.full((B, V), float("-inf"), device="cuda:0")
    lg[torch.arange(B), torch.arange(B) * 7 + 1] = 0.5
    for ps in (SET7, (1.0, 0, 1.0, 0.0, 0.5, 0.0, 0.0), (1.0, 0, 1.0, 0.0, 1.0, 0.0, 2e-3), (1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0)):
        toks, nk, _, _ = _run_ext(lg, V, ps, 9, 0)
        assert toks == [b * 7 + 1 for b in range(B)] and nk == [1] * B, ps
    half = logits.clone()
    half[:, ::2] = float("-inf")
    for seed in range(4):
        toks, nk, _, _ = _run_ext(half, V, (1.0, 0, 1.0, 0.0, 0.9, 0.0, 1e-4), seed, 1)
        assert all(t % 2 == 1 for t in toks) and all(n <= V // 2 for n in nk)
    assert _run_ext(half, V, (1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0), 3, 1)[1] == [V // 2] * B      # all off: the finite scores
    # a NULL step_dev is step 0; NULL n_kept and planes are allowed
    assert _run_ext(logits, V, SET7, 42, 0, step_dev=False)[0] == _run_ext(logits, V, SET7, 42, 0)[0]
    cur = torch.zeros(B, dtype=torch.int64, device="cuda:0")
    ops.sample_ext(logits, V, None, 0, None, cur, torch.tensor(_params8(SET7), dtype=torch.float32, device="cuda:0"),
                   torch.tensor([42], dtype=torch.int64, device="cuda:0"))
    torch.cuda.synchronize()
    assert cur.cpu().tolist() == _run_ext(logits, V, SET7, 42, 0)[0]
    # the eos latch is gar_argmax's
    toks, _, _, kw = _run_ext(logits, V, SET7, 42, 2, eos=[a[0], a[5], -1])
    fin = kw["finished"].cpu().tolist()
    hit = [t in (a[0], a[5]) for t in toks]
    assert toks == a and [f == 2 for f in fin] == hit and int(kw["done_count"].item()) == sum(hit)
    # the empirical distribution of 4000 draws of one row under set seven follows the restatement's
    row = torch.randn(1, 64, generator=g) * 1.5
    z, keep, amb = R.warp_ext(row[0].numpy(), *((SET7[0], min(SET7[1], 64)) + SET7[2:]))
    assert not amb.any() and 1 < keep.sum() < 64
    p = np.where(keep, np.exp(z.astype(np.float64) - z[keep].max()), 0.0)
    p /= p.sum()
    counts = np.zeros(64)
    big = row.expand(64, 64).contiguous().to("cuda:0")
    for s in range(4000 // 64):
        toks, nk, _, _ = _run_ext(big, 64, SET7, 2024 + s, s % 8)
        assert nk == [int(keep.sum())] * 64
        for t in toks:
            counts[t] += 1
    assert counts[~keep].sum() == 0
    assert np.abs(counts / counts.sum() - p).max() < 0.03, (counts / counts.sum(), p)


def test_sample_ext_warped_plane_against_f64():
    """the warped plane is the drawn token's log-probability under the FINAL kept set; the raw plane is gar_sample_lp's"""
    from gar_amd import hip
    hip.require_device(0)
    for name in ("flat1000", "peaked128256"):
        lg, sets = R.group(name, "float32")
        B, V = lg.shape
        x = torch.from_numpy(lg).to("cuda:0")
        checked = 0
        for si, ps in enumerate(R.PARAM_SETS):
            toks, nk, planes, _ = _run_ext(x, V, ps, 11, 4, lp=True)
            assert toks == _run_ext(x, V, ps, 11, 4)[0]                    # the planes do not move the token
            raw = torch.log_softmax(torch.from_numpy(lg).double(), -1)
            for b in range(B):
                kept, amb = sets[si][b]
                assert abs(float(planes[0][b, 4]) - float(raw[b, toks[b]])) <= LP_TOL
                if len(amb) == 0:
                    keep = np.zeros(V, dtype=bool)
                    keep[kept] = True
                    z = (lg[b] / np.float32(ps[0])).astype(np.float32)
                    assert abs(float(planes[1][b, 4]) - R.warped_logprob(z, keep, toks[b])) <= LP_TOL, (name, si, b)
                    checked += 1
            for pl in planes:
                assert (pl[:, [0, 1, 2, 3, 5, 6, 7]] == SENTINEL).all()
        assert checked >= 64


# ---- end to end on the tiny fixture ---------------------------------------------------------------------------------------------
NT = 24
SEED = 777


@functools.lru_cache(maxsize=None)
def _shared():
    import test_gpu_logprobs as T
    cfg, W, proc, batch, ragged = T._setup()
    return T, cfg, W, ragged


def _gc(V, ps, **kw):
    return dict(do_sample=True, temperature=ps[0], top_k=min(ps[1], V), top_p=ps[2], max_new_tokens=NT, **kw)


def _sw(ps):
    from gar_amd import SamplingWarpers
    return SamplingWarpers(min_p=ps[3], typical_p=ps[4], epsilon_cutoff=ps[5], eta_cutoff=ps[6])


def _check_run(out, V, ps, seed, what, row_counter=lambda r: r, warped=False, mostly_clean=True):
    """rules (a) and (b) for every token of ``out`` against the restatement's draw from the run's own logits of that step.
    ``mostly_clean``: at least half of the steps have to be unambiguous, so that rule (b) is not vacuous (the tiny fixture's
    near-flat rows under typical_p alone are mostly ambiguous: that run passes False and is held to rule (a) and to rule (b) on the
    steps that are unambiguous)"""
    from oracle import sampling as S
    seq, lg = out.sequences.cpu(), out.logits.float().cpu().numpy()
    ps = (ps[0], min(ps[1], V)) + tuple(ps[2:])
    near = clean = amb_steps = 0
    for r in range(seq.shape[0]):
        for j in range(seq.shape[1]):
            z, keep, amb = R.warp_ext(lg[r, j, :V], *ps)
            tok = int(seq[r, j])
            assert keep[tok] or amb[tok], (what, r, j, tok)
            if amb.any():
                amb_steps += 1
                continue
            exp, margin = S.draw(z, keep, S.uniform(seed, row_counter(r), j))
            clean += 1
            if tok != exp:
                kept = np.flatnonzero(keep)
                assert margin < MARGIN and abs(int(np.searchsorted(kept, tok)) - int(np.searchsorted(kept, exp))) == 1, (what, r, j, tok, exp)
                near += 1
            if warped:
                got = float(out.token_logprobs_warped[r, j])
                assert abs(got - R.warped_logprob(z, keep, tok)) <= LP_TOL, (what, r, j, got)
    print(f"{what}: {clean} unambiguous steps, {near} at a neighbouring boundary, {amb_steps} ambiguous")
    assert near <= max(1, clean // 100) and (2 * clean >= seq.numel() or not mostly_clean), (near, clean, amb_steps)


class _count_launches:
    """wraps ops.sample / ops.sample_ext: the row count of every launch"""

    def __init__(self):
        from gar_amd import ops
        self.ops, self.orig, self.rows = ops, {n: getattr(ops, n) for n in ("sample", "sample_ext")}, {"sample": [], "sample_ext": []}
        for n in self.orig:
            setattr(ops, n, self._wrap(n))

    def _wrap(self, n):
        def counted(logits, *a, **kw):
            self.rows[n].append(logits.shape[0])
            return self.orig[n](logits, *a, **kw)
        return counted

    def undo(self):
        for n, f in self.orig.items():
            setattr(self.ops, n, f)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_with_sampling_warpers(dtype):
    """ragged left-padded batch of 3, 24 tokens: every token is the restatement's draw from that step's returned logits; graph ==
    eager; a chunked prompt phase == the unchunked one; num_return_sequences = 3 == the replicated batch; a dict is read like the
    dataclass; typical_p alone (a set that removes the most likely token) too"""
    from gar_amd.modeling_gar import GARModel
    from test_gpu_fanout import _repeat
    T, cfg, W, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(dtype)
    gc = _gc(V, SET7)
    plain = m.generate(**ragged, **gc, seed=SEED).sequences.cpu()
    out = m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7), return_logits=True)
    seq = out.sequences.cpu()
    assert tuple(seq.shape) == (3, NT) and not torch.equal(seq, plain)
    _check_run(out, V, SET7, SEED, f"set seven {dtype}")
    assert torch.equal(m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7), use_graph=False).sequences.cpu(), seq)
    as_dict = dict(min_p=SET7[3], typical_p=SET7[4], epsilon_cutoff=SET7[5], eta_cutoff=SET7[6])
    assert torch.equal(m.generate(**ragged, **gc, seed=SEED, sampling_warpers=as_dict).sequences.cpu(), seq)
    assert not torch.equal(m.generate(**ragged, **gc, seed=SEED + 1, sampling_warpers=as_dict).sequences.cpu(), seq)
    # other values through the SAME captured graph: the eight floats are read on every launch
    typ = (1.3, 0, 1.0, 0.0, 0.2, 0.0, 0.0)
    o2 = m.generate(**ragged, **_gc(V, typ), seed=SEED, sampling_warpers=_sw(typ), return_logits=True)
    _check_run(o2, V, typ, SEED, f"typical_p alone {dtype}", mostly_clean=False)
    # a prompt phase cut into chunks of one sequence: the first tokens are counted by the global batch row
    m1 = GARModel(cfg, W, dtype, "cuda:0", prefill_chunk=1)
    assert torch.equal(m1.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7)).sequences.cpu(), seq)
    # N samples per prompt == the replicated batch
    N = 3
    fan = m.generate(**ragged, **gc, seed=SEED, num_return_sequences=N, sampling_warpers=_sw(SET7), return_logits=True)
    assert tuple(fan.sequences.shape) == (3 * N, NT)
    _check_run(fan, V, SET7, SEED, f"num_return_sequences {dtype}")
    if dtype == torch.float32:          # parity mode: the replicated batch computes the same logits bit for bit
        rep = m.generate(**_repeat(ragged, N), **gc, seed=SEED, sampling_warpers=_sw(SET7)).sequences.cpu()
        assert torch.equal(rep, fan.sequences.cpu())
    assert len({tuple(r.tolist()) for r in fan.sequences.cpu()[:N]}) > 1
    with pytest.raises(ValueError, match="do_sample"):
        m.generate(**ragged, max_new_tokens=4, sampling_warpers=_sw(SET7))
    with pytest.raises(ValueError, match="do_sample"):
        m.generate_begin(**ragged, max_new_tokens=4, do_sample=False, sampling_warpers=dict(min_p=0.1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_warpers_with_logprobs_and_alternatives(dtype):
    """return_logprobs: token_logprobs_warped is the drawn token's log-probability under the final kept set, token_logprobs stays
    raw; top_logprobs / candidate_token_ids ride along; the tokens are those of the call without them"""
    from logprob_ref import raw_logprob_at
    T, cfg, W, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(dtype)
    gc = _gc(V, SET7)
    base = m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7)).sequences.cpu()
    out = m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7), return_logits=True, return_logprobs=True, top_logprobs=3,
                     candidate_token_ids=[0, 5])
    assert torch.equal(out.sequences.cpu(), base)
    _check_run(out, V, SET7, SEED, f"logprobs {dtype}", warped=True)
    assert float((out.token_logprobs.cpu().double() - raw_logprob_at(out.logits, out.sequences)).abs().max()) <= LP_TOL
    assert tuple(out.top_logprobs.shape) == (3, NT, 3) and tuple(out.candidate_logprobs.shape) == (3, NT, 2)
    assert not torch.equal(out.token_logprobs_warped, out.token_logprobs)
    eager = m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7), return_logprobs=True, use_graph=False)
    assert torch.equal(eager.token_logprobs_warped, out.token_logprobs_warped) and torch.equal(eager.sequences.cpu(), base)


def test_generate_warpers_with_logits_processing():
    """logits_processing runs first: the restatement is applied to the processed scores the run returns"""
    T, cfg, W, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(torch.float32)
    gc = _gc(V, SET7)
    P = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    out = m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7), logits_processing=P, return_logits=True)
    _check_run(out, V, SET7, SEED, "with logits_processing")
    for row in out.sequences.cpu().tolist():
        grams = [tuple(row[j:j + 2]) for j in range(len(row) - 1)]
        assert len(grams) == len(set(grams))
    assert not torch.equal(out.sequences.cpu(), m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7)).sequences.cpu())


def test_fp8_modes_pipeline_and_forced_tokens_carry_the_warpers():
    from gar_amd.modeling_gar import GARModel
    T, cfg, W, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    gc = _gc(V, SET7)
    for kw in (dict(kv_cache_dtype="fp8"), dict(decode_weight_dtype="fp8")):
        out = GARModel(cfg, W, torch.bfloat16, "cuda:0", **kw).generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7),
                                                                       return_logits=True)
        _check_run(out, V, SET7, SEED, str(kw))
    m = T._model(torch.bfloat16)
    want = m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7)).sequences.cpu()
    outs = m.generate_pipelined([ragged, ragged], **gc, seed=SEED, sampling_warpers=_sw(SET7))
    torch.cuda.synchronize()
    assert len(outs) == 2 and all(torch.equal(o.sequences.cpu(), want) for o in outs)
    # forced_tokens: the model's own picks are still reported, drawn on the forced context
    forced = m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7), forced_tokens=want, return_logits=True)
    assert torch.equal(forced.sequences.cpu(), want)
    _check_run(forced, V, SET7, SEED, "forced_tokens")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_default_path_is_untouched(dtype):
    """without the parameter — and with None or all-neutral values — tokens are bit-identical and gar_sample_ext is never launched;
    a request with warpers launches it in gar_sample's place, once per chunk of first tokens and once per step"""
    from gar_amd import SamplingWarpers
    T, cfg, W, ragged = _shared()
    V = cfg.mllm_config.text_config.vocab_size
    m = T._model(dtype)
    gc = _gc(V, SET7)
    greedy = m.generate(**ragged, max_new_tokens=NT).sequences.cpu()
    before = m.generate(**ragged, **gc, seed=SEED).sequences.cpu()
    c = _count_launches()
    try:
        m.generate(**ragged, **gc, seed=SEED, sampling_warpers=_sw(SET7), use_graph=False)
        assert c.rows["sample_ext"] == [3] * NT and c.rows["sample"] == []
        c.rows["sample_ext"].clear()
        for kw in ({}, dict(sampling_warpers=None), dict(sampling_warpers=SamplingWarpers()), dict(sampling_warpers={}),
                   dict(sampling_warpers=dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)),
                   dict(sampling_warpers=SamplingWarpers(typical_p=2.0)), dict(use_graph=False)):
            assert torch.equal(m.generate(**ragged, **gc, seed=SEED, **kw).sequences.cpu(), before), kw
        assert c.rows["sample_ext"] == [] and len(c.rows["sample"]) > 0
        assert torch.equal(m.generate(**ragged, max_new_tokens=NT, sampling_warpers=SamplingWarpers()).sequences.cpu(), greedy)
        assert c.rows["sample_ext"] == []
    finally:
        c.undo()


def test_fails_without_the_feature():
    """what did not exist before: the binding, the parameter, the export"""
    import inspect
    from gar_amd import SamplingWarpers, hip, ops
    from gar_amd.modeling_gar import GARModel
    assert callable(ops.sample_ext) and "gar_sample_ext" in hip.SIGNATURES
    assert "sampling_warpers" in inspect.signature(GARModel.generate_begin).parameters
    assert SamplingWarpers(min_p=0.05).pack()[0] == 0.05
