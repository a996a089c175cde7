#!/usr/bin/env python
"""generate(top_logprobs=k, candidate_token_ids=[...]): what the k alternatives and the candidate values cost. Writes
profiles/top_logprobs.json:

  kernels    us per call of gar_topk_lp (its two launches), V = 128256 (GAR-1B's vocabulary, ld rounded up to 64), bf16, B in {1, 64},
             k in {1, 5, 20}, without and with 4 candidates, and gar_argmax / gar_argmax_lp on the same buffer for scale; hipGraph
             replays of LAUNCHES calls on one logits buffer (in a decode step the lm_head has just written it: cache-resident here
             too), device events around the replays
  generate   a 64-token greedy generate at B = 64, synthetic GAR-1B bf16, eos disabled — wall ms of the whole call and decode
             ms / token ((full - the same call with max_new_tokens = 1) / 63) — without the option, with top_logprobs=5, and with
             top_logprobs=5 plus 4 candidates
  bench      `python bench.py --gpus 1 --steps 10 --warmup 3` (the default path, which asks for neither option) in a checkout of the
             parent commit (--parent-tree, built) and in this tree, in turns: the result line's value per run

The forms are timed in turns; every figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_top_logprobs.py [--skip-kernels] [--skip-e2e] [--skip-bench] [--reps R] [--bench-reps R]
                                          [--parent-tree DIR] [--image-size S]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grasp-any-region_amd"))
import torch  # noqa: E402

from gar_amd import hip, ops  # noqa: E402

REPS = 5
LAUNCHES = 20
V = 128256
CANDS = [32, 33, 34, 35]


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
    T = 8
    logits = (torch.randn(B, ld, device=dev) * 2.5).to(torch.bfloat16)
    out = torch.zeros(B, 256, dtype=torch.int64, device=dev)
    raw = torch.zeros(B, 256, device=dev)
    cur = torch.zeros(B, dtype=torch.int64, device=dev)
    step = torch.tensor([3], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.argmax_workspace(B, V), dtype=torch.uint8, device=dev)
    wsl = torch.empty(ops.argmax_lp_workspace(B, V), dtype=torch.uint8, device=dev)
    cand_ids = torch.tensor(CANDS, dtype=torch.int32, device=dev)
    cand_lp = torch.zeros(B, T, len(CANDS), device=dev)
    many = lambda fn: (lambda: [fn() for _ in range(LAUNCHES)])
    names = ["gar_argmax", "gar_argmax_lp"]
    runs = [_graph(many(lambda: ops.argmax(logits, V, out, 256, step, cur, ws))),
            _graph(many(lambda: ops.argmax(logits, V, out, 256, step, cur, wsl, logprobs=raw)))]
    keep = []
    for k in (1, 5, 20):
        ids = torch.zeros(B, T, k, dtype=torch.int32, device=dev)
        lp = torch.zeros(B, T, k, device=dev)
        wsk = torch.empty(ops.topk_lp_workspace(B, V, k), dtype=torch.uint8, device=dev)
        keep.append((ids, lp, wsk))
        names += [f"gar_topk_lp_k{k}", f"gar_topk_lp_k{k}_cand4"]
        runs.append(_graph(many(lambda ids=ids, lp=lp, wsk=wsk: ops.topk_lp(logits, V, step, wsk, top_ids=ids, top_lp=lp))))
        runs.append(_graph(many(lambda ids=ids, lp=lp, wsk=wsk: ops.topk_lp(logits, V, step, wsk, top_ids=ids, top_lp=lp,
                                                                          cand_ids=cand_ids, cand_lp=cand_lp))))
    names.append("gar_topk_lp_cand4_only")
    ws0 = torch.empty(ops.topk_lp_workspace(B, V, 0), dtype=torch.uint8, device=dev)
    runs.append(_graph(many(lambda: ops.topk_lp(logits, V, step, ws0, cand_ids=cand_ids, cand_lp=cand_lp))))
    us = _alternate(runs, reps)
    res = {"B": B, "V": V, "dtype": "bf16", "us_per_call": dict(zip(names, us))}
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
    from gar_amd.processing import GARProcessor
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    distinct = [SingleRegionCaptionDataset(synthetic_image(i, image_size, image_size), synthetic_mask(i, image_size, image_size), proc,
                                           data_dtype=torch.bfloat16, device="cpu")[0] for i in range(8)]
    batch = _batch([distinct[i % 8] for i in range(B)])
    m = GARModel(cfg, synthetic_weights(cfg), torch.bfloat16)
    forms = {
        "plain": lambda n: m.generate(**batch, max_new_tokens=n),
        "top_logprobs_5": lambda n: m.generate(**batch, max_new_tokens=n, top_logprobs=5),
        "top_logprobs_5_cand4": lambda n: m.generate(**batch, max_new_tokens=n, top_logprobs=5, candidate_token_ids=CANDS),
    }
    seqs = {}
    for name, fn in forms.items():                     # warm-up: graphs, workspaces
        seqs[name] = fn(new_tokens).sequences
        fn(1)
    torch.cuda.synchronize()
    same = all(torch.equal(s, seqs["plain"]) for s in seqs.values())
    full = {name: [] for name in forms}
    stepms = {name: [] for name in forms}
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
    out = {"model": "GAR-1B bf16 (synthetic weights)", "B": B, "new_tokens": new_tokens, "image_size": image_size,
           "sequences_equal_plain": same,
           "generate": {name: {"full_ms": _stat(full[name]), "decode_ms_per_token": _stat(stepms[name])} for name in forms}}
    print(json.dumps(out), flush=True)
    return out


def bench_default_path(parent_tree, reps):
    """bench.py's result line in the parent commit's tree and in this one, in turns (a fresh process per run)"""
    trees = {"parent": parent_tree, "this": ROOT}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3"]
    vals = {name: [] for name in trees}
    meta = {}
    for _ in range(reps):
        for name, tree in trees.items():
            r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=1500)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py in {tree} failed: {r.stderr[-2000:]}")
            line = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])
            vals[name].append(float(line["value"]))
            meta = {"metric": line.get("metric"), "unit": line.get("unit")}
            print(json.dumps({"tree": name, "value": line["value"]}), flush=True)
    out = dict(meta, command=" ".join(cmd[1:]), **{name: _stat(v) for name, v in vals.items()})
    out["this_over_parent"] = out["this"]["median"] / out["parent"]["median"]
    print(json.dumps(out), flush=True)
    return out


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--bench-reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "_base"),
                    help="a built checkout of the parent commit (git worktree / git archive, then python __graft_entry__.py in it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_logprobs.json"))
    a = ap.parse_args()
    REPS = a.reps
    hip.require_device(0)
    res = json.load(open(a.out)) if os.path.isfile(a.out) else {}         # a skipped section keeps the figures of its last run
    res["device"] = torch.cuda.get_device_name(0)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not a.skip_kernels:
        res["kernels"] = [bench_kernels(B) for B in (1, 64)]
        save()
    if not a.skip_e2e:
        res["generate"] = bench_generate(a.new_tokens, a.image_size)
        save()
    if not a.skip_bench:
        if not os.path.isfile(os.path.join(a.parent_tree, "bench.py")):
            raise SystemExit(f"--parent-tree {a.parent_tree}: no checkout of the parent commit there (or pass --skip-bench)")
        torch.cuda.empty_cache()
        res["bench_default_path"] = bench_default_path(a.parent_tree, a.bench_reps)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
