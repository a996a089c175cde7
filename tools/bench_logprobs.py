#!/usr/bin/env python
"""generate(return_logprobs=True): what the chosen token's log-probability costs. Writes profiles/logprobs.json:

  kernels    us per launch of gar_argmax against gar_argmax_lp and of gar_sample against gar_sample_lp (temperature 0.8, top_k 50,
             top_p 0.9), V = 128256 (GAR-1B's vocabulary, ld rounded up to 64), bf16, B = 1 and B = 64; hipGraph replays of
             LAUNCHES launches on one logits buffer (in a decode step the lm_head has just written it: cache-resident here too)
  generate   a 64-token generate at B = 64, synthetic GAR-1B bf16, eos disabled, greedy — wall ms of the whole call and decode
             ms / token ((full - the same call with max_new_tokens = 1) / 63) — in three forms: without the flag; with
             return_logprobs=True; the dense route (return_logits=True, then torch log_softmax + gather on the [B, 64, V] f32
             logits). And the other way to the same numbers: a second, teacher-forced score() pass over the finished captions.

The forms are timed in turns; every figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_logprobs.py [--skip-e2e] [--skip-kernels] [--reps R] [--image-size S]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grasp-any-region_amd"))
import torch  # noqa: E402

from gar_amd import hip, ops  # noqa: E402

REPS = 5
LAUNCHES = 20
V = 128256


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def _graph(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def _alternate(launches, reps):
    out = [[] for _ in launches]
    for _ in range(REPS):
        for i, launch in enumerate(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1) / reps / LAUNCHES * 1e3)
    return [_stat(x) for x in out]


def bench_kernels(B, reps=10):
    dev = "cuda:0"
    ld = (V + 63) // 64 * 64
    logits = (torch.randn(B, ld, device=dev) * 2.5).to(torch.bfloat16)
    out = torch.zeros(B, 256, dtype=torch.int64, device=dev)
    raw, warped = torch.zeros(B, 256, device=dev), torch.zeros(B, 256, device=dev)
    cur = torch.zeros(B, dtype=torch.int64, device=dev)
    step = torch.tensor([3], dtype=torch.int32, device=dev)
    params = torch.tensor([0.8, 0.9, 50.0, 0.0], device=dev)
    seed = torch.tensor([777], dtype=torch.int64, device=dev)
    ws = torch.empty(ops.argmax_workspace(B, V), dtype=torch.uint8, device=dev)
    wsl = torch.empty(ops.argmax_lp_workspace(B, V), dtype=torch.uint8, device=dev)
    many = lambda fn: (lambda: [fn() for _ in range(LAUNCHES)])
    runs = [
        _graph(many(lambda: ops.argmax(logits, V, out, 256, step, cur, ws))),
        _graph(many(lambda: ops.argmax(logits, V, out, 256, step, cur, wsl, logprobs=raw, logprobs_warped=warped))),
        _graph(many(lambda: ops.sample(logits, V, out, 256, step, cur, params, seed))),
        _graph(many(lambda: ops.sample(logits, V, out, 256, step, cur, params, seed, logprobs=raw, logprobs_warped=warped))),
    ]
    us = _alternate(runs, reps)
    res = {"B": B, "V": V, "dtype": "bf16", "gar_argmax_us": us[0], "gar_argmax_lp_us": us[1], "gar_sample_us": us[2],
           "gar_sample_lp_us": us[3], "argmax_lp_extra_us": us[1]["median"] - us[0]["median"],
           "sample_lp_extra_us": us[3]["median"] - us[2]["median"]}
    print(json.dumps(res), flush=True)
    return res


def _batch(ss):
    return dict(input_ids=torch.cat([s["input_ids"] for s in ss]), pixel_values=torch.cat([s["pixel_values"] for s in ss]),
                global_mask_values=torch.cat([s["global_mask_values"] for s in ss]), bboxes=[b for s in ss for b in s["bboxes"]],
                aspect_ratios=torch.cat([s["aspect_ratios"] for s in ss]))


def bench_generate(new_tokens, image_size, B=64):
    from gar_amd import GARConfig
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor, append_target
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    distinct = [SingleRegionCaptionDataset(synthetic_image(i, image_size, image_size), synthetic_mask(i, image_size, image_size), proc,
                                           data_dtype=torch.bfloat16, device="cpu")[0] for i in range(8)]
    ss = [distinct[i % 8] for i in range(B)]
    batch = _batch(ss)
    m = GARModel(cfg, synthetic_weights(cfg), torch.bfloat16)

    def dense(n):
        o = m.generate(**batch, max_new_tokens=n, return_logits=True)
        lp = torch.log_softmax(o.logits, -1).gather(-1, o.sequences[..., None])[..., 0]
        return o, lp

    forms = {
        "plain": lambda n: m.generate(**batch, max_new_tokens=n),
        "return_logprobs": lambda n: m.generate(**batch, max_new_tokens=n, return_logprobs=True),
        "dense_logits_then_torch": lambda n: dense(n)[0],
    }
    seq = None
    for name, fn in forms.items():                     # warm-up: graphs, workspaces
        seq = fn(new_tokens).sequences
        fn(1)
    torch.cuda.synchronize()
    scored = [append_target(s, seq[i].cpu()) for i, s in enumerate(ss)]
    sb = dict(_batch(scored), labels=torch.cat([s["labels"] for s in scored]))
    score = lambda: m.score(sb["pixel_values"], sb["global_mask_values"], sb["aspect_ratios"], sb["bboxes"], sb["input_ids"],
                            sb["labels"])
    score()
    torch.cuda.synchronize()
    full = {name: [] for name in forms}
    stepms = {name: [] for name in forms}
    score_ms = []
    for _ in range(REPS):
        for name, fn in forms.items():                 # in turns
            t0 = time.perf_counter()
            fn(new_tokens)
            torch.cuda.synchronize()
            f = time.perf_counter() - t0
            t0 = time.perf_counter()
            fn(1)
            torch.cuda.synchronize()
            p = time.perf_counter() - t0
            full[name].append(f * 1e3)
            stepms[name].append((f - p) / (new_tokens - 1) * 1e3)
        t0 = time.perf_counter()
        score()
        torch.cuda.synchronize()
        score_ms.append((time.perf_counter() - t0) * 1e3)
    out = {"model": "GAR-1B bf16 (synthetic weights)", "B": B, "new_tokens": new_tokens, "image_size": image_size,
           "generate": {name: {"full_ms": _stat(full[name]), "decode_ms_per_token": _stat(stepms[name])} for name in forms},
           "second_score_pass_ms": _stat(score_ms)}
    print(json.dumps(out), flush=True)
    return out


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprobs.json"))
    a = ap.parse_args()
    REPS = a.reps
    hip.require_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_kernels:
        res["kernels"] = [bench_kernels(B) for B in (1, 64)]
    if not a.skip_e2e:
        res["generate"] = bench_generate(a.new_tokens, a.image_size)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
