"""GPU (-m gpu): top-k and candidate-token log-probabilities — gar_topk_lp against float64 on the same stored logits
(tests/top_logprobs_ref.py: ids exactly, values within LP_TOL) and against gar_argmax for entry 0, and
GARModel.generate(top_logprobs=, candidate_token_ids=) against the logits the run itself returns: greedy and sampled, graph and eager,
left-padded batches, fan-out, fp8 cache / weights, the pipeline, and the GAR-Bench loop's --option_logprobs."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from logprob_ref import LP_TOL
from top_logprobs_ref import candidates_ref, close_or_both_minus_inf, topk_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
STEP, WIDE, COL0, NCOL = 3, 16, 2, 8         # step_dev = 3; the planes = columns 2..9 of [B, 16, k] buffers
ID_SENTINEL, LP_SENTINEL = -7, 7.0
KMAX = 32


@functools.lru_cache(maxsize=None)
def _case(V, dtype):
    """test_gpu_logprobs._logits (randn * 2.5, 1e4 in the padding columns) with row 6 one constant — every entry ties, the expected
    ids are 0..k-1 — and row 7 -inf except three finite entries, two of them equal. Returns (logits, candidate ids, float64
    reference ids / values for k = min(32, V), float64 candidate values). Shared, never written."""
    from test_gpu_logprobs import _logits
    x = _logits(V, dtype).clone()
    x[6, :V] = 0.75
    x[7, :V] = float("-inf")
    x[7, V // 3], x[7, 5], x[7, V - 2] = 0.5, 2.0, 0.5
    cands = [0, V - 1, int(x[0, :V].float().argmax()), 1]           # id 1 is -inf in row 7 (so are 0 and V - 1)
    ids, lp = topk_ref(x[:, :V], min(KMAX, V))
    return x, cands, ids, lp, candidates_ref(x[:, :V], cands)


def _topk(x, V, k, cands, top=True):
    """one gar_topk_lp into column slices of wider sentinel-primed planes; returns the wide planes on the host"""
    from gar_amd import ops
    B, dev = x.shape[0], x.device
    stepd = torch.tensor([STEP], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.topk_lp_workspace(B, V, k if top else 0), dtype=torch.uint8, device=dev)
    kw, wide = {}, {}
    if top:
        wide["ids"] = torch.full((B, WIDE, k), ID_SENTINEL, dtype=torch.int32, device=dev)
        wide["lp"] = torch.full((B, WIDE, k), LP_SENTINEL, dtype=torch.float32, device=dev)
        kw.update(top_ids=wide["ids"][:, COL0:COL0 + NCOL], top_lp=wide["lp"][:, COL0:COL0 + NCOL])
    if cands:
        wide["cand"] = torch.full((B, WIDE, len(cands)), LP_SENTINEL, dtype=torch.float32, device=dev)
        kw.update(cand_ids=torch.tensor(cands, dtype=torch.int32, device=dev), cand_lp=wide["cand"][:, COL0:COL0 + NCOL])
    ops.topk_lp(x, V, stepd, ws, **kw)
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in wide.items()}


def _only_step_column_written(plane, sentinel):
    other = [c for c in range(WIDE) if c != COL0 + STEP]
    assert (plane[:, other] == sentinel).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [37, 1000, 128256, 150001])
def test_topk_lp_kernel_against_f64(dtype, V):
    """k in {1, 5, 20, 32} (k <= V), B = 8: ids equal the float64 reference's exactly (value descending, index ascending — bf16 rows
    hold many genuine ties), values within LP_TOL with -inf equal to -inf, entry 0 is gar_argmax's token on the same buffer and its
    value gar_argmax_lp's lp_raw bit for bit, only the step's column of the wide planes is written, either output group alone gives
    the same bits. V = 37: 63 of 64 partial blocks hold at most one element and k exceeds it; V = 1000: 16 per block, fewer than
    k = 20; V = 128256: the real vocabulary; V = 150001: past the in-register form's 64 x 256 x 8 elements, the form that re-reads
    its block every round."""
    from gar_amd import hip, ops
    hip.require_device(0)
    x, cands, ref_ids, ref_lp, ref_cand = _case(V, dtype)
    cur = torch.zeros(8, dtype=torch.int64, device=x.device)
    ops.argmax(x, V, None, 0, None, cur, torch.empty(ops.argmax_workspace(8, V), dtype=torch.uint8, device=x.device))
    am = cur.cpu()
    # gar_argmax_lp on the same buffer: its lp_raw is entry 0's value bit for bit (include/gar_hip.h: "formed the same way")
    out, raw = torch.zeros(8, NCOL, dtype=torch.int64, device=x.device), torch.zeros(8, NCOL, device=x.device)
    ops.argmax(x, V, out, NCOL, torch.tensor([STEP], dtype=torch.int32, device=x.device), None,
               torch.empty(ops.argmax_lp_workspace(8, V), dtype=torch.uint8, device=x.device), logprobs=raw)
    assert torch.equal(out[:, STEP].cpu(), am)
    lp_raw = raw[:, STEP].cpu()
    worst = 0.0
    for k in (1, 5, 20, 32):
        if k > V:            # none of the sizes above: every V here holds 32 entries
            continue
        got = _topk(x, V, k, cands)
        ids, lp, cand = (got[n][:, COL0 + STEP] for n in ("ids", "lp", "cand"))
        assert torch.equal(ids.long(), ref_ids[:, :k]), (k, ids, ref_ids[:, :k])
        worst = max(worst, close_or_both_minus_inf(lp, ref_lp[:, :k], LP_TOL), close_or_both_minus_inf(cand, ref_cand, LP_TOL))
        assert torch.equal(ids[:, 0].long(), am)
        assert torch.equal(lp[:, 0], lp_raw), (k, lp[:, 0], lp_raw)
        assert ids[6].tolist() == list(range(k))
        assert ids[7, :3].tolist()[:k] == [5, V // 3, V - 2][:k] and torch.isneginf(lp[7, 3:]).all()
        assert torch.isneginf(cand[7, [0, 1, 3]]).all()
        _only_step_column_written(got["ids"], ID_SENTINEL)
        _only_step_column_written(got["lp"], LP_SENTINEL)
        _only_step_column_written(got["cand"], LP_SENTINEL)
        # the candidate of row 0's argmax is entry 0's value: two reads of one quantity
        assert torch.equal(cand[:, 2][:1], lp[:1, 0])
        if k in (1, 20):        # either group alone, and the same launch again: the same bits
            alone = _topk(x, V, k, None)
            assert set(alone) == {"ids", "lp"} and torch.equal(alone["ids"], got["ids"]) and torch.equal(alone["lp"], got["lp"])
            again = _topk(x, V, k, cands)
            assert all(torch.equal(again[n], got[n]) for n in got)
    only = _topk(x, V, 0, cands, top=False)
    assert set(only) == {"cand"} and torch.equal(only["cand"], got["cand"])
    print(f"topk_lp {dtype} V={V}: max |lp - f64| {worst:.3g}")


def test_topk_lp_refuses_bad_arguments():
    from gar_amd import hip, ops
    hip.require_device(0)
    x = _case(37, torch.float32)[0]
    dev = x.device
    ws = torch.empty(ops.topk_lp_workspace(8, 37, 32), dtype=torch.uint8, device=dev)
    plane = lambda k, dt: torch.zeros(8, 1, k, dtype=dt, device=dev)
    with pytest.raises(hip.GarError, match="topk_lp"):           # k = 33
        ops.topk_lp(x, 37, None, torch.empty(ops.topk_lp_workspace(8, 37, 33), dtype=torch.uint8, device=dev),
                    top_ids=plane(33, torch.int32), top_lp=plane(33, torch.float32))
    with pytest.raises(hip.GarError, match="topk_lp"):           # k > V
        ops.topk_lp(x, 20, None, ws, top_ids=plane(21, torch.int32), top_lp=plane(21, torch.float32))
    with pytest.raises(hip.GarError, match="topk_lp"):           # 65 candidates
        ops.topk_lp(x, 37, None, ws, cand_ids=torch.zeros(65, dtype=torch.int32, device=dev), cand_lp=plane(65, torch.float32))
    with pytest.raises(hip.GarError, match="topk_lp"):           # neither group
        ops.topk_lp(x, 37, None, ws)
    assert ops.topk_lp_workspace(8, 37, 32) == 8 * 64 * 65 * 4 and ops.topk_lp_workspace(8, 37, 0) == ops.topk_lp_workspace(8, 37, 1)


# ---- generate(top_logprobs=, candidate_token_ids=) ----------------------------------------------------------------------------
K = 5


def _shared():
    """tests/test_gpu_logprobs.py's tiny model, inputs and sampling settings (cached there: one model per dtype for both files)"""
    import test_gpu_logprobs as T
    cfg, W, proc, batch, ragged = T._setup()
    V = cfg.mllm_config.text_config.vocab_size
    return T, batch, ragged, V, [0, V - 1, 65, 66]


def _opts(cands):
    return dict(top_logprobs=K, candidate_token_ids=cands)


def _check_against_own_logits(out, cands, k=K):
    """every column's ids equal the float64 reference on the run's own logits, values within LP_TOL (callers pass unmasked outputs)"""
    ref_ids, ref_lp = topk_ref(out.logits, k)
    assert out.top_logprob_ids.dtype == torch.int64 and out.top_logprobs.dtype == out.candidate_logprobs.dtype == torch.float32
    R, n = out.sequences.shape
    assert tuple(out.top_logprob_ids.shape) == tuple(out.top_logprobs.shape) == (R, n, k)
    assert tuple(out.candidate_logprobs.shape) == (R, n, len(cands))
    assert torch.equal(out.top_logprob_ids.cpu(), ref_ids)
    return max(close_or_both_minus_inf(out.top_logprobs, ref_lp, LP_TOL),
               close_or_both_minus_inf(out.candidate_logprobs, candidates_ref(out.logits, cands), LP_TOL))


def _same_fields(a, b):
    assert torch.equal(a.sequences, b.sequences)
    for n in ("top_logprob_ids", "top_logprobs", "candidate_logprobs"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_top_logprobs(dtype, sampled):
    """3 regions x 12 tokens with top_logprobs=5 and 4 candidates, beside return_logits and return_logprobs: every step's ids and
    values against the float64 reference on out.logits — RAW log-probabilities also when sampling; greedy: entry 0 is the token
    and its value token_logprobs'; sequences and token_logprobs bit-equal to the call without the two options; hipGraph loop ==
    eager loop bit for bit; behind an eos the run really emits ids are -1 and values 0.0; one left-padded ragged batch;
    forced_tokens leave the fields describing the model's own distribution."""
    T, batch, ragged, V, cands = _shared()
    m = T._model(dtype)
    NT = T.NT
    kw = dict(generation_config=T._gc(), seed=777) if sampled else dict(max_new_tokens=NT)
    base = m.generate(**batch, **kw, return_logprobs=True)
    assert base.top_logprob_ids is None and base.top_logprobs is None and base.candidate_logprobs is None
    out = m.generate(**batch, **kw, return_logprobs=True, return_logits=True, **_opts(cands))
    assert torch.equal(out.sequences, base.sequences) and torch.equal(out.token_logprobs, base.token_logprobs)
    assert torch.equal(out.token_logprobs_warped, base.token_logprobs_warped)
    err = _check_against_own_logits(out, cands)
    print(f"generate top_logprobs {dtype} sampled={sampled}: max |lp - f64 of own logits| {err:.3g}")
    if sampled:
        assert not torch.equal(out.top_logprob_ids[..., 0], out.sequences)       # the draws are not all the arg-max
    else:
        assert torch.equal(out.top_logprob_ids[..., 0], out.sequences)
        assert float((out.top_logprobs[..., 0] - out.token_logprobs).abs().max()) <= LP_TOL
    # independent of return_logprobs / return_logits; either option alone; graph == eager
    bare = m.generate(**batch, **kw, **_opts(cands))
    assert bare.token_logprobs is None
    _same_fields(bare, out)
    top_only = m.generate(**batch, **kw, top_logprobs=K)
    assert top_only.candidate_logprobs is None and torch.equal(top_only.top_logprobs, out.top_logprobs)
    cand_only = m.generate(**batch, **kw, candidate_token_ids=cands)
    assert cand_only.top_logprobs is None and cand_only.top_logprob_ids is None
    assert torch.equal(cand_only.candidate_logprobs, out.candidate_logprobs) and torch.equal(cand_only.sequences, out.sequences)
    eager = m.generate(**batch, **kw, use_graph=False, **_opts(cands))
    _same_fields(eager, out)
    assert torch.equal(m.generate(**batch, **kw).sequences, out.sequences)
    # an eos the run really emits, rows ending at different columns (as test_gpu_logprobs picks it)
    seq = out.sequences.cpu()
    first = lambda e: [next((j + 1 for j, tk in enumerate(r.tolist()) if tk == e), None) for r in seq]
    eos = max(set(seq.flatten().tolist()), key=lambda e: (len(set(first(e))), -min(f or NT for f in first(e))))
    hit = first(eos)
    assert any(h is not None and h < NT for h in hit), hit
    ekw = dict(generation_config=T._gc(eos_token_id=eos, pad_token_id=1), seed=777) if sampled else \
        dict(max_new_tokens=NT, eos_token_id=eos, pad_token_id=1)
    for graph in (True, False):
        e = m.generate(**batch, **ekw, sync_every=4, use_graph=graph, **_opts(cands))
        n = e.sequences.shape[1]
        assert tuple(e.top_logprob_ids.shape) == (3, n, K) and tuple(e.candidate_logprobs.shape) == (3, n, 4)
        for r in range(3):
            end = min(hit[r] if hit[r] is not None else n, n)
            assert torch.equal(e.top_logprob_ids[r, :end], out.top_logprob_ids[r, :end]), (r, graph)
            assert torch.equal(e.top_logprobs[r, :end], out.top_logprobs[r, :end])
            assert torch.equal(e.candidate_logprobs[r, :end], out.candidate_logprobs[r, :end])
            assert (e.top_logprob_ids[r, end:] == -1).all() and (e.top_logprobs[r, end:] == 0.0).all()
            assert (e.candidate_logprobs[r, end:] == 0.0).all() and (e.sequences[r, end:] == 1).all()
    # a left-padded batch of two prompt lengths
    rp = m.generate(**ragged, **kw)
    ro = m.generate(**ragged, **kw, return_logits=True, **_opts(cands))
    assert torch.equal(ro.sequences, rp.sequences)
    _check_against_own_logits(ro, cands)
    if not sampled:
        forced = m.generate(**batch, **kw, return_logits=True, forced_tokens=out.sequences.flip(0), **_opts(cands))
        _check_against_own_logits(forced, cands)
        assert torch.equal(forced.top_logprob_ids[..., 0], forced.sequences)
        # refused by value, before anything is launched
        for bad in (dict(top_logprobs=33), dict(candidate_token_ids=[V]), dict(candidate_token_ids=list(range(65)))):
            with pytest.raises(ValueError):
                m.generate(**batch, **kw, **bad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fanout_top_logprobs(dtype):
    """num_return_sequences = 4 over a left-padded batch, bf16 (shared-prefix decode) and f32 (copied prefix): the 4 rows of a prompt
    carry that prompt's values at step 0, bit for bit; every step matches the reference on the run's own logits; graph == eager"""
    T, batch, ragged, V, cands = _shared()
    m = T._model(dtype)
    N = 4
    plain = m.generate(**ragged, generation_config=T._gc(N), seed=777)
    out = m.generate(**ragged, generation_config=T._gc(N), seed=777, return_logits=True, **_opts(cands))
    assert tuple(out.sequences.shape) == (3 * N, T.NT) and torch.equal(out.sequences, plain.sequences)
    _check_against_own_logits(out, cands)
    for b in range(3):
        for i in range(1, N):
            for name in ("top_logprob_ids", "top_logprobs", "candidate_logprobs"):
                f = getattr(out, name)
                assert torch.equal(f[b * N + i, 0], f[b * N, 0]), (name, b, i)
    assert not torch.equal(out.top_logprobs[1:N, 1:], out.top_logprobs[0:N - 1, 1:])         # later steps are per row
    eager = m.generate(**ragged, generation_config=T._gc(N), seed=777, use_graph=False, **_opts(cands))
    _same_fields(eager, out)


def test_top_logprobs_with_fp8_cache_fp8_weights_and_pipeline():
    from gar_amd.modeling_gar import GARModel, GenerationPipeline
    T, batch, ragged, V, cands = _shared()
    cfg, W = T._setup()[:2]
    for kw in (dict(kv_cache_dtype="fp8"), dict(decode_weight_dtype="fp8")):
        m = GARModel(cfg, W, torch.bfloat16, "cuda:0", **kw)
        plain = m.generate(**batch, max_new_tokens=T.NT)
        out = m.generate(**batch, max_new_tokens=T.NT, return_logits=True, **_opts(cands))
        assert torch.equal(out.sequences, plain.sequences), kw
        _check_against_own_logits(out, cands)
        assert torch.equal(out.top_logprob_ids[..., 0], out.sequences)
    m = T._model(torch.bfloat16)
    ref = m.generate(**batch, max_new_tokens=T.NT, **_opts(cands))
    pipe = GenerationPipeline(m, max_new_tokens=T.NT, **_opts(cands))
    outs = pipe.submit(batch) + pipe.submit(batch) + pipe.flush()
    torch.cuda.synchronize()
    assert len(outs) == 2
    for o in outs:
        _same_fields(o, ref)
    outs = m.generate_pipelined([batch, batch], max_new_tokens=T.NT, top_logprobs=K)
    torch.cuda.synchronize()
    assert all(torch.equal(o.top_logprobs, ref.top_logprobs) and o.candidate_logprobs is None for o in outs)


def test_gar_bench_option_logprobs(tmp_path):
    """evaluation/GAR-Bench/inference.py --mode vqa --option_logprobs on a synthetic annotation file (built as
    test_gpu_bench_loops builds its own), batch sizes 1 and 4: option_logprobs equals candidate_logprobs[0, 0] of a direct generate
    on the same sample within LP_TOL, option_pick is its arg-max, model_output is the record of the run without the flag"""
    from PIL import Image

    from gar_amd import GARConfig, rle
    from gar_amd.bench_loops import gar_bench_question, option_letters, option_token_ids
    from gar_amd.eval_dataset import MultiRegionDataset
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.synthetic import synthetic_disjoint_masks, synthetic_image
    from test_gpu_bench_loops import _run, _set_order
    os.makedirs(tmp_path / "images")
    items = []
    for i, nm in enumerate((2, 3, 2, 2, 2)):                 # four items share the letters A, B: one batch of 4
        synthetic_image(20 + i, 260, 200).save(tmp_path / "images" / f"vqa_{i}.png")
        masks = synthetic_disjoint_masks(20 + i, nm, 260, 200)
        names = " or ".join(f"<Prompt{k}>" for k in range(nm))
        items.append({"image": f"images/vqa_{i}.png", "mask_rles": [rle.encode(m) for m in masks],
                      "question": f"Which one is larger, {names}?", "choices": [f"{'ABC'[k]}. <Prompt{k}>" for k in range(nm)],
                      "answer": "A", "type": "size" if i < 2 else "shape"})
    anno = tmp_path / "vqa.json"
    json.dump(items, open(anno, "w"))
    common = ("--anno_file", str(anno), "--image_folder", str(tmp_path), "--mode", "vqa", "--output_dir", str(tmp_path / "out"))
    plain_out = _run("GAR-Bench", *common, "--cache_name", "p")
    plain = json.load(open(tmp_path / "out" / "p_vqa.json"))
    assert all("option_logprobs" not in r and "option_pick" not in r for r in plain)
    runs = {}
    for bs in (1, 4):
        stdout = _run("GAR-Bench", *common, "--cache_name", f"o{bs}", "--option_logprobs", "--batch_size", str(bs))
        runs[bs] = json.load(open(tmp_path / "out" / f"o{bs}_vqa.json"))
        assert [ln for ln in stdout.split("\n") if "overall" in ln] == [ln for ln in plain_out.split("\n") if "overall" in ln]
        if bs == 4:
            assert "5 items in 2 generate calls" in stdout
    cfg = GARConfig.tiny()
    proc = GARProcessor.from_config(cfg, max_num_tiles=4)
    model = GARModel.from_synthetic(cfg, 0, torch.float32)
    pt = [f"<Prompt{i}>" for i in range(cfg.prompt_numbers)] + ["<NO_Prompt>"]
    for j, it in enumerate(items):
        letters = option_letters(it)
        assert letters == list("ABC"[:len(it["choices"])])
        q = gar_bench_question(it, "vqa")
        masks = [(rle.decode(r) * 255).astype(np.uint8) for r in it["mask_rles"]]
        s = MultiRegionDataset(image=Image.open(tmp_path / it["image"]), masks=masks, question_str=q, processor=proc,
                               prompt_number=cfg.prompt_numbers, visual_prompt_tokens=pt, data_dtype=torch.float32,
                               device="cuda:0", prompt_order=_set_order(q))[0]
        o = model.generate(**s, generation_config=dict(max_new_tokens=8, do_sample=False, eos_token_id=proc.tokenizer.eos_token_id,
                                                       pad_token_id=proc.tokenizer.pad_token_id),
                           candidate_token_ids=option_token_ids(proc.tokenizer, letters))
        direct = o.candidate_logprobs[0, 0].double().cpu()
        for bs in (1, 4):
            r = runs[bs][j]
            got = torch.tensor(r["option_logprobs"], dtype=torch.float64)
            err = float((got - direct).abs().max())
            print(f"item {j} batch_size {bs}: option_logprobs {r['option_logprobs']} max |d| to direct generate {err:.3g}")
            assert len(r["option_logprobs"]) == len(letters) and err <= LP_TOL, (j, bs, err)
            assert r["option_pick"] == letters[int(np.argmax(r["option_logprobs"]))]
            assert r["model_output"] == plain[j]["model_output"]
            assert {k: v for k, v in r.items() if k not in ("option_logprobs", "option_pick")} == plain[j]


def test_demo_cli_prints_top_logprobs(tmp_path):
    """demo/gar_with_mask.py --top_logprobs 3: the caption of the run without the flag, then one line per generated token with three
    decoded-token:probability pairs, probabilities descending and summing to at most 1"""
    from PIL import Image

    from gar_amd.synthetic import synthetic_image, synthetic_mask
    ip, mp = str(tmp_path / "img.png"), str(tmp_path / "mask.png")
    synthetic_image(11, 300, 220).save(ip)
    Image.fromarray(synthetic_mask(11, 300, 220).astype(np.uint8) * 255).save(mp)

    def run(*args):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "grasp-any-region_amd")]), PYTHONHASHSEED="0")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "gar_with_mask.py"), "--synthetic_weights", "--model_name_or_path",
                            "tiny", "--data_type", "bf16", "--max_num_tiles", "4", "--max_new_tokens", "6", "--image_path", ip,
                            "--mask_path", mp, *args], capture_output=True, text=True, timeout=600, env=env,
                           cwd=os.path.join(ROOT, "demo"))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.rstrip("\n").split("\n")
    plain, top = run(), run("--top_logprobs", "3")
    assert top[:len(plain)] == plain and 1 <= len(top) - len(plain) <= 6
    for ln in top[len(plain):]:
        probs = [float(p) for p in re.findall(r":(\d\.\d{4})(?:  |$)", ln)]
        assert len(probs) == 3 and probs == sorted(probs, reverse=True) and sum(probs) <= 1.0 + 3e-4, ln
