"""GPU (-m gpu): per-token log-probabilities of generated tokens — gar_argmax_lp / gar_sample_lp against float64 on the same stored
logits (tests/logprob_ref.py) and against gar_argmax / gar_sample for the token, and GARModel.generate(return_logprobs=True)
against the logits the run itself returns, oracle/sampling.py's kept set, and score()."""
import functools

import numpy as np
import pytest
import torch

from logprob_ref import LP_TOL, check_warped, raw_logprob_at

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.6, 40, 0.8), (1.0, 5, 0.5), (2.0, 20000, 0.999)]
SEED_STEP = (123456789012345, 3)
STEP, WIDE, COL0, NCOL = 3, 16, 2, 8         # step_dev = 3; out_tokens / planes = columns 2..9 of [B, 16] buffers
SENTINEL = 7.0
# test 5 (generate's token_logprobs against score()'s on the same caption, f32 tiny): the two sides come out of different GEMM paths
# (decode GEMV vs prefill GEMM + fused head). SCORE_VS_DECODE_MEASURED is the largest difference between
# log_softmax(generate(return_logits=True).logits) and score().token_logprobs — neither side uses the new kernels — measured on an
# MI355X on this test's inputs; the bound is 4 x it (the new kernels add the reduction error LP_TOL bounds; the factor covers
# another machine).
SCORE_VS_DECODE_MEASURED = 1.31e-6
SCORE_VS_DECODE_BOUND = 4 * SCORE_VS_DECODE_MEASURED


@functools.lru_cache(maxsize=None)
def _logits(V, dtype):
    """[8, round_up(V, 64)] on the device: randn * 2.5 from manual_seed(V) in columns 0..V-1, +1e4 in the padding columns — a
    kernel that reads past V finds a huge maximum / mass and fails visibly. Shared, never written."""
    g = torch.Generator().manual_seed(V)
    x = torch.randn(8, V, generator=g) * 2.5
    buf = torch.full((8, (V + 63) // 64 * 64), 1e4)
    buf[:, :V] = x
    return buf.to(dtype).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _raw_ref(V, dtype):
    from logprob_ref import raw_logprobs_f64
    return raw_logprobs_f64(_logits(V, dtype)[:, :V])


def _run(kind, logits, V, lp: bool, setting=None, eos=None):
    """one launch of argmax / sample with (lp) or without the planes, into column slices of wider buffers"""
    from gar_amd import ops
    B, dev = logits.shape[0], logits.device
    out = torch.full((B, WIDE), -1, dtype=torch.int64, device=dev)[:, COL0:COL0 + NCOL]
    cur = torch.zeros(B, dtype=torch.int64, device=dev)
    stepd = torch.tensor([STEP], dtype=torch.int32, device=dev)
    kw = {}
    if eos is not None:
        kw = dict(eos_ids=torch.tensor(eos, dtype=torch.int64, device=dev), finished=torch.full((B,), -1, dtype=torch.int32, device=dev),
                  done_count=torch.zeros(1, dtype=torch.int32, device=dev))
    raw = warped = None
    if lp:
        raw = torch.full((B, WIDE), SENTINEL, dtype=torch.float32, device=dev)[:, COL0:COL0 + NCOL]
        warped = torch.full((B, WIDE), SENTINEL, dtype=torch.float32, device=dev)[:, COL0:COL0 + NCOL]
        kw.update(logprobs=raw, logprobs_warped=warped)
    if kind == "argmax":
        size = ops.argmax_lp_workspace(B, V) if lp else ops.argmax_workspace(B, V)
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        ops.argmax(logits, V, out, out.stride(0), stepd, cur, ws, **kw)
    else:
        T, k, p = setting
        params = torch.tensor([T, p, float(min(k, V)), 0.0], dtype=torch.float32, device=dev)
        seedd = torch.tensor([SEED_STEP[0]], dtype=torch.int64, device=dev)
        ops.sample(logits, V, out, out.stride(0), stepd, cur, params, seedd, **kw)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), cur=cur.cpu(), raw=None if raw is None else raw.cpu(), warped=None if warped is None else warped.cpu(),
                finished=kw["finished"].cpu() if eos is not None else None,
                done=int(kw["done_count"].item()) if eos is not None else None)


def _same_token_and_latches(a, b):
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["cur"], b["cur"])
    assert torch.equal(a["out"][:, STEP], a["cur"]) and (a["out"][:, [c for c in range(NCOL) if c != STEP]] == -1).all()
    if a["finished"] is not None:
        assert torch.equal(a["finished"], b["finished"]) and a["done"] == b["done"]


def _only_step_column_written(plane):
    assert (plane[:, [c for c in range(NCOL) if c != STEP]] == SENTINEL).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [128256, 1000, 37])
def test_argmax_lp_kernel_against_f64(dtype, V):
    """gar_argmax_lp: token, cur and eos latches are gar_argmax's; the raw plane at the step's column is log_softmax in float64 of
    the same stored logits at that token, the warped plane the same value, other columns untouched. V = 37: 63 of the 64 partial
    blocks are empty."""
    from gar_amd import hip
    hip.require_device(0)
    x = _logits(V, dtype)
    am = x[:, :V].float().argmax(1).cpu()
    eos = [int(am[0]), int(am[5]), -1]
    base, lp = _run("argmax", x, V, False, eos=eos), _run("argmax", x, V, True, eos=eos)
    _same_token_and_latches(lp, base)
    assert lp["done"] >= 1 and torch.equal(lp["cur"], am)
    ref = _raw_ref(V, dtype)[torch.arange(8), lp["cur"]]
    err = float((lp["raw"][:, STEP].double() - ref).abs().max())
    print(f"argmax_lp {dtype} V={V}: max |lp - f64| {err:.3g}")
    assert err <= LP_TOL, (err, lp["raw"][:, STEP], ref)
    assert torch.equal(lp["warped"], lp["raw"])
    _only_step_column_written(lp["raw"])
    # either plane alone
    from gar_amd import ops
    only = torch.full((8, NCOL), SENTINEL, dtype=torch.float32, device=x.device)
    out = torch.zeros(8, NCOL, dtype=torch.int64, device=x.device)
    ws = torch.empty(ops.argmax_lp_workspace(8, V), dtype=torch.uint8, device=x.device)
    ops.argmax(x, V, out, NCOL, None, None, ws, logprobs_warped=only)
    assert torch.equal(only[:, 0].cpu(), lp["raw"][:, STEP]) and torch.equal(out[:, 0].cpu(), am)


@pytest.mark.parametrize("dtype", DTYPES)
def test_argmax_lp_minus_inf_rows(dtype):
    """a row with ONE finite logit has log-probability 0.0 exactly (in a block of its own, or beside empty / all -inf blocks); rows
    with scattered -inf logits stay finite and right"""
    from gar_amd import hip
    hip.require_device(0)
    for V in (37, 1000, 5000):
        ld = (V + 63) // 64 * 64
        x = torch.full((8, ld), float("-inf"))
        x[:, V:] = 1e4
        pos = [(b * 131 + 5) % V for b in range(8)]
        x[torch.arange(8), pos] = torch.linspace(-3, 3, 8)
        x = x.to(dtype).to("cuda:0")
        r = _run("argmax", x, V, True)
        assert r["cur"].tolist() == pos
        assert r["raw"][:, STEP].tolist() == [0.0] * 8, r["raw"][:, STEP]
        g = torch.Generator().manual_seed(V + 1)
        y = torch.randn(8, V, generator=g) * 2.5
        y[torch.rand(8, V, generator=g) < 0.3] = float("-inf")
        y[7, : V // 2] = float("-inf")                       # whole partial blocks of -inf beside live ones
        buf = torch.full((8, ld), 1e4)
        buf[:, :V] = y
        buf = buf.to(dtype).to("cuda:0")
        r = _run("argmax", buf, V, True)
        got = r["raw"][:, STEP]
        assert torch.isfinite(got).all()
        assert float((got.double() - raw_logprob_at(buf[:, :V], r["cur"])).abs().max()) <= LP_TOL


@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_lp_kernel_against_f64_and_oracle(dtype):
    """gar_sample_lp on test 1's logits, the six settings of test_sample_kernel_equals_oracle: the token is gar_sample's; the raw
    plane is log_softmax in float64 at the drawn token; the warped plane is z[tok] - logsumexp(z[keep]) in float64 with
    oracle/sampling.py's keep — or, where the oracle's top-p cut lies within MARGIN of top_p x Z1, with the one neighbouring run of
    equal logits added or dropped, for at most 1 % of the cases."""
    from gar_amd import hip
    hip.require_device(0)
    near = total = 0
    worst_raw = 0.0
    for V in (128256, 1000, 37):
        x = _logits(V, dtype)
        rows = x[:, :V].float().cpu().numpy()
        ref = _raw_ref(V, dtype)
        for setting in SETTINGS:
            T, k, p = setting
            base, lp = _run("sample", x, V, False, setting), _run("sample", x, V, True, setting)
            _same_token_and_latches(lp, base)
            _only_step_column_written(lp["raw"])
            _only_step_column_written(lp["warped"])
            tok = lp["cur"]
            err = float((lp["raw"][:, STEP].double() - ref[torch.arange(8), tok]).abs().max())
            worst_raw = max(worst_raw, err)
            assert err <= LP_TOL, (V, setting, err)
            for b in range(8):
                hit = check_warped(rows[b], int(tok[b]), float(lp["warped"][b, STEP]), T, min(k, V), p)
                if hit:
                    print(f"top-p cut within MARGIN: {dtype} V={V} setting={setting} row={b}")
                near += hit
                total += 1
            if setting == (1.0, 0, 1.0):             # nothing warped: both planes hold the same quantity
                assert float((lp["warped"] - lp["raw"])[:, STEP].abs().max()) <= LP_TOL
    print(f"sample_lp {dtype}: max |raw - f64| {worst_raw:.3g}; {near} of {total} warped values at a neighbouring top-p cut")
    assert near * 100 <= total, (near, total)


def test_sample_lp_latches_and_fallback_rows():
    """the eos latches with the planes, and rows with one finite logit (the draw's rounding fall-backs end at that token too):
    log-probability 0 in both planes"""
    from gar_amd import hip
    hip.require_device(0)
    V = 1000
    x = _logits(V, torch.float32)
    setting = (0.7, 50, 1.0)
    t0 = _run("sample", x, V, False, setting)["cur"]
    eos = [int(t0[1]), int(t0[6]), -1]
    base, lp = _run("sample", x, V, False, setting, eos=eos), _run("sample", x, V, True, setting, eos=eos)
    _same_token_and_latches(lp, base)
    assert lp["done"] >= 2 and lp["finished"][1] == STEP
    one = torch.full((8, 1024), float("-inf"))
    one[:, V:] = 1e4
    one[torch.arange(8), torch.arange(8) * 7 + 1] = 0.5
    r = _run("sample", one.to("cuda:0"), V, True, (1.0, 50, 0.9))
    assert r["cur"].tolist() == [b * 7 + 1 for b in range(8)]
    assert float(r["raw"][:, STEP].abs().max()) <= LP_TOL and float(r["warped"][:, STEP].abs().max()) <= LP_TOL


# ---- generate(return_logprobs=True) -------------------------------------------------------------------------------------------
NT = 12
SAMPLING = dict(do_sample=True, temperature=0.8, top_p=0.9)


@functools.lru_cache(maxsize=None)
def _setup():
    from gar_amd import GARConfig
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    from test_gpu_e2e import _left_pad_batch, _lengthen, _sample
    cfg = GARConfig.tiny()
    proc = GARProcessor.from_config(cfg, max_num_tiles=4)
    smp = [_sample(cfg, proc, i) for i in range(3)]
    batch = {k: torch.cat([s[k] for s in smp], 0) if isinstance(smp[0][k], torch.Tensor) else [x for s in smp for x in s[k]]
             for k in smp[0]}
    ragged = _left_pad_batch([_lengthen(_sample(cfg, proc, i), e, 300 + j) for j, (i, e) in enumerate(zip((3, 4, 6), (0, 21, 21)))])
    return cfg, synthetic_weights(cfg), proc, batch, ragged


@functools.lru_cache(maxsize=None)
def _model(dtype):
    from gar_amd.modeling_gar import GARModel
    cfg, W = _setup()[:2]
    return GARModel(cfg, W, dtype, "cuda:0")


def _gc(N=1, **kw):
    V = _setup()[0].mllm_config.text_config.vocab_size
    return dict(SAMPLING, top_k=min(50, V), max_new_tokens=NT, num_return_sequences=N, **kw)


def _check_raw_against_own_logits(out):
    """token_logprobs == log_softmax (float64) of the run's own return_logits logits at the chosen tokens"""
    ref = raw_logprob_at(out.logits, out.sequences)
    err = float((out.token_logprobs.cpu().double() - ref).abs().max())
    assert err <= LP_TOL, err
    return err


def _check_warped_against_oracle(out):
    V = _setup()[0].mllm_config.text_config.vocab_size
    lg, seq, w = out.logits.float().cpu().numpy(), out.sequences.cpu(), out.token_logprobs_warped.cpu()
    near = total = 0
    for r in range(seq.shape[0]):
        for j in range(seq.shape[1]):
            near += check_warped(lg[r, j, :V], int(seq[r, j]), float(w[r, j]), 0.8, min(50, V), 0.9)
            total += 1
    assert near * 100 <= total, (near, total)


def _full_rows(out, n):
    R = out.sequences.shape[0]
    assert tuple(out.token_logprobs.shape) == tuple(out.token_logprobs_warped.shape) == (R, n)
    assert out.token_logprobs.dtype == torch.float32 and out.n_tokens.tolist() == [n] * R
    for s, t in ((out.sum_logprobs, out.token_logprobs), (out.sum_logprobs_warped, out.token_logprobs_warped)):
        assert tuple(s.shape) == (R,)
        # a float32 sum of n terms: n roundings of at most eps x the running magnitude
        tol = n * 2.0 ** -23 * max(1.0, float(t.abs().sum(1).max()))
        assert float((s.double() - t.double().sum(1)).abs().max()) <= tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_greedy_logprobs(dtype):
    """greedy, 3 regions x 12 tokens: sequences equal the run without the flag; token_logprobs equal log_softmax of the same run's
    logits at the chosen tokens; warped == raw; hipGraph loop == eager loop bit for bit; with an eos id taken from the run's own
    tokens the columns behind a row's eos are 0 and sum / count match a host recomputation; one left-padded ragged batch"""
    cfg, W, proc, batch, ragged = _setup()
    m = _model(dtype)
    plain = m.generate(**batch, max_new_tokens=NT)
    assert plain.token_logprobs is None and plain.sum_logprobs is None and plain.n_tokens is None
    out = m.generate(**batch, max_new_tokens=NT, return_logprobs=True, return_logits=True)
    assert torch.equal(out.sequences, plain.sequences)
    err = _check_raw_against_own_logits(out)
    print(f"generate greedy {dtype}: max |token_logprobs - f64 of own logits| {err:.3g}")
    assert torch.equal(out.token_logprobs_warped, out.token_logprobs)
    _full_rows(out, NT)
    eager = m.generate(**batch, max_new_tokens=NT, return_logprobs=True, use_graph=False)
    assert torch.equal(eager.sequences, out.sequences) and torch.equal(eager.token_logprobs, out.token_logprobs)
    assert torch.equal(m.generate(**batch, max_new_tokens=NT, use_graph=False).sequences, plain.sequences)
    # without return_logits, and again: the planes are the state's, a second request overwrites them
    again = m.generate(**batch, max_new_tokens=NT, return_logprobs=True)
    assert torch.equal(again.token_logprobs, out.token_logprobs) and torch.equal(again.sum_logprobs, out.sum_logprobs)
    # a synthetic eos from the run's own tokens, so that rows end at different columns
    seq = out.sequences.cpu()
    first = lambda e: [next((j + 1 for j, tk in enumerate(r.tolist()) if tk == e), None) for r in seq]
    eos = max(set(seq.flatten().tolist()), key=lambda e: (len(set(first(e))), -min(f or NT for f in first(e))))
    hit = first(eos)
    assert len(set(hit)) >= 2 and any(h is not None and h < NT for h in hit), hit
    for graph in (True, False):
        e = m.generate(**batch, max_new_tokens=NT, eos_token_id=eos, pad_token_id=1, return_logprobs=True, sync_every=4,
                       use_graph=graph)
        n = e.sequences.shape[1]
        assert tuple(e.token_logprobs.shape) == (3, n) == tuple(e.token_logprobs_warped.shape)
        for r in range(3):
            end = min(hit[r] if hit[r] is not None else n, n)
            assert torch.equal(e.token_logprobs[r, :end], out.token_logprobs[r, :end]), (r, graph)
            assert not e.token_logprobs[r, end:].any() and not e.token_logprobs_warped[r, end:].any()
            assert (e.sequences[r, end:] == 1).all() and int(e.n_tokens[r]) == end
            host = float(out.token_logprobs[r, :end].double().sum())
            assert abs(float(e.sum_logprobs[r]) - host) <= end * 2.0 ** -23 * max(1.0, float(out.token_logprobs[r, :end].abs().sum()))
            assert float(e.sum_logprobs_warped[r]) == float(e.sum_logprobs[r])
    # a left-padded batch of two prompt lengths
    rp = m.generate(**ragged, max_new_tokens=NT)
    ro = m.generate(**ragged, max_new_tokens=NT, return_logprobs=True, return_logits=True)
    assert torch.equal(ro.sequences, rp.sequences)
    _check_raw_against_own_logits(ro)
    _full_rows(ro, NT)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_sampled_logprobs(dtype):
    """temperature 0.8, top_k 50, top_p 0.9, seed 777: sequences equal the run without the flag; raw against the run's own
    logits; warped against z[tok] - logsumexp(z[keep]) with the oracle's keep; graph == eager bit for bit; forced_tokens leave
    the planes reporting the model's own choice"""
    cfg, W, proc, batch, ragged = _setup()
    m = _model(dtype)
    plain = m.generate(**batch, generation_config=_gc(), seed=777)
    out = m.generate(**batch, generation_config=_gc(), seed=777, return_logprobs=True, return_logits=True)
    assert torch.equal(out.sequences, plain.sequences)
    _check_raw_against_own_logits(out)
    _check_warped_against_oracle(out)
    _full_rows(out, NT)
    assert not torch.equal(out.token_logprobs_warped, out.token_logprobs)
    eager = m.generate(**batch, generation_config=_gc(), seed=777, return_logprobs=True, use_graph=False)
    assert torch.equal(eager.sequences, out.sequences) and torch.equal(eager.token_logprobs, out.token_logprobs)
    assert torch.equal(eager.token_logprobs_warped, out.token_logprobs_warped)
    forced = m.generate(**batch, generation_config=_gc(), seed=777, return_logprobs=True, return_logits=True,
                        forced_tokens=out.sequences.flip(0))
    _check_raw_against_own_logits(forced)            # at forced.sequences: what the model chose, not what was fed back
    _check_warped_against_oracle(forced)
    # the pipeline carries the fields through unchanged
    from gar_amd.modeling_gar import GenerationPipeline
    pipe = GenerationPipeline(m, generation_config=_gc(), seed=777, return_logprobs=True)
    outs = pipe.submit(batch) + pipe.submit(batch) + pipe.flush()
    torch.cuda.synchronize()
    assert len(outs) == 2
    for o in outs:
        assert torch.equal(o.sequences, out.sequences) and torch.equal(o.token_logprobs, out.token_logprobs)
        assert torch.equal(o.token_logprobs_warped, out.token_logprobs_warped) and torch.equal(o.n_tokens, out.n_tokens)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fanout_logprobs(dtype):
    """num_return_sequences = 4 over a left-padded batch, bf16 (shared-prefix decode) and f32 (copied prefix): planes [B * 4, n],
    row b * 4 + i = sample i of prompt b — each row checked against that row's own logits"""
    cfg, W, proc, batch, ragged = _setup()
    m = _model(dtype)
    N = 4
    plain = m.generate(**ragged, generation_config=_gc(N), seed=777)
    out = m.generate(**ragged, generation_config=_gc(N), seed=777, return_logprobs=True, return_logits=True)
    assert tuple(out.sequences.shape) == (3 * N, NT) and torch.equal(out.sequences, plain.sequences)
    _full_rows(out, NT)
    _check_raw_against_own_logits(out)
    _check_warped_against_oracle(out)
    for b in range(3):                 # the N first tokens are N draws from ONE row of logits: equal tokens, equal values
        for i in range(1, N):
            if int(out.sequences[b * N + i, 0]) == int(out.sequences[b * N, 0]):
                assert float(out.token_logprobs[b * N + i, 0]) == float(out.token_logprobs[b * N, 0])
    eager = m.generate(**ragged, generation_config=_gc(N), seed=777, return_logprobs=True, use_graph=False)
    assert torch.equal(eager.sequences, out.sequences) and torch.equal(eager.token_logprobs, out.token_logprobs)
    assert torch.equal(eager.token_logprobs_warped, out.token_logprobs_warped)


def test_generate_logprobs_with_fp8_cache_and_fp8_decode_weights():
    """the opt-in fp8 KV cache and fp8 decode weights carry the fields through: values against the run's own logits"""
    from gar_amd.modeling_gar import GARModel
    cfg, W, proc, batch, ragged = _setup()
    for kw in (dict(kv_cache_dtype="fp8"), dict(decode_weight_dtype="fp8")):
        m = GARModel(cfg, W, torch.bfloat16, "cuda:0", **kw)
        plain = m.generate(**batch, max_new_tokens=NT)
        out = m.generate(**batch, max_new_tokens=NT, return_logprobs=True, return_logits=True)
        assert torch.equal(out.sequences, plain.sequences), kw
        _check_raw_against_own_logits(out)
        _full_rows(out, NT)


def test_generate_logprobs_agree_with_score():
    """f32, tiny: the greedy caption appended to its prompt and scored teacher-forced (labels -100 on the prompt) —
    score().token_logprobs on the caption columns against generate().token_logprobs. Two GEMM paths (decode GEMV vs prefill GEMM
    and fused head), so the bound is not LP_TOL: the dense route log_softmax(generate(return_logits=True).logits) against score()
    — the parent commit's two sides — measured 1.31e-6 on these inputs on an MI355X; the bound is 4 x that, 5.24e-6 (this test
    measured 1.43e-6 there)."""
    from gar_amd.processing import append_target
    from test_gpu_e2e import _sample
    cfg, W, proc, batch, ragged = _setup()
    m = _model(torch.float32)
    s = _sample(cfg, proc, 4)
    g = m.generate(**s, max_new_tokens=NT, return_logprobs=True)
    seq = g.sequences[0].cpu()
    d = append_target(s, seq)
    sc = m.score(d["pixel_values"], d["global_mask_values"], d["aspect_ratios"], d["bboxes"], d["input_ids"], d["labels"])
    got = sc.token_logprobs[0, -len(seq):].double().cpu()
    err = float((got - g.token_logprobs[0].double().cpu()).abs().max())
    print(f"generate vs score token_logprobs: max |d| {err:.3g} (bound {SCORE_VS_DECODE_BOUND})")
    assert err <= SCORE_VS_DECODE_BOUND, (err, SCORE_VS_DECODE_BOUND)
    assert abs(float(sc.sum_logprobs[0]) - float(g.sum_logprobs[0])) <= NT * SCORE_VS_DECODE_BOUND
    assert int(sc.n_tokens[0]) == int(g.n_tokens[0]) == NT


def test_demo_cli_orders_captions_by_mean_logprob(tmp_path):
    """demo/gar_with_mask.py --return_logprobs with --num_return_sequences N: the N captions of the run without the flag, each
    behind its mean token log-probability, best first"""
    import os
    import re
    import subprocess
    import sys

    from PIL import Image

    from gar_amd.synthetic import synthetic_image, synthetic_mask
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ip, mp = str(tmp_path / "img.png"), str(tmp_path / "mask.png")
    synthetic_image(11, 300, 220).save(ip)
    Image.fromarray(synthetic_mask(11, 300, 220).astype(np.uint8) * 255).save(mp)

    def run(*args):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "grasp-any-region_amd")]), PYTHONHASHSEED="0")
        r = subprocess.run([sys.executable, os.path.join(root, "demo", "gar_with_mask.py"), "--synthetic_weights", "--model_name_or_path",
                            "tiny", "--data_type", "bf16", "--max_num_tiles", "4", "--max_new_tokens", "12", "--image_path", ip,
                            "--mask_path", mp, "--num_return_sequences", "3", "--temperature", "0.8", "--seed", "7", *args],
                           capture_output=True, text=True, timeout=600, env=env, cwd=os.path.join(root, "demo"))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.rstrip("\n").split("\n")
    plain, scored = run(), run("--return_logprobs")
    assert len(scored) == 3
    parts = [re.fullmatch(r"\[(-?\d+\.\d{4})\] (.*)", ln) for ln in scored]
    assert all(parts), scored
    vals = [float(m.group(1)) for m in parts]
    assert vals == sorted(vals, reverse=True) and all(v < 0 for v in vals), vals
    assert sorted(m.group(2) for m in parts) == sorted(plain)
