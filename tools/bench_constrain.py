#!/usr/bin/env python
"""generate(constraint=PhraseConstraint(...)): what the phrase constraint costs. Writes profiles/constrain.json:

  kernels    us per call of gar_constrain at B = 64, V = 128256 (GAR-1B's vocabulary) in bf16 for sets of 4, 64 and 1200 phrases
             (up to 8 tokens each), at step 0 (every row at its root, the widest node) and at step 3, and of gar_logits_process
             (repetition penalty 1.2 + no_repeat_ngram_size 3, history of 64 tokens) at the same shape in the same run; hipGraph
             replays of LAUNCHES calls on one logits buffer, device events around the replays
  generate   a greedy generate at B = 64, synthetic GAR-1B bf16 — decode ms / token ((full - the same call with
             max_new_tokens = 1) / (n - 1)) without the parameter and with a set of 64 phrases longer than the run, so both
             decode n tokens; in turns in one process
  headline   `python bench.py --steps 10 --warmup 3` in a built checkout of the parent commit (--parent-tree) and in this tree:
             parent, this, parent, this — each a fresh process. Recorded: the four values, and whether both of this tree's are
             at or above the slower parent run minus twice the parents' gap

Every kernel / generate figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_constrain.py [--skip-kernels] [--skip-e2e] [--skip-headline] [--reps R] [--parent-tree DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "grasp-any-region_amd"
sys.path.insert(0, os.path.join(ROOT, PKG))
import torch  # noqa: E402

from gar_amd import hip, ops  # noqa: E402

REPS = 5
LAUNCHES = 20
V = 128256
PROCESSING = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)


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


def phrase_set(n, seed=0):
    """n distinct phrases of 1..8 tokens over the whole vocabulary, a few of them prefixes of others"""
    gen = torch.Generator().manual_seed(seed + n)
    out, seen = [], set()
    while len(out) < n:
        p = tuple(torch.randint(0, V, (int(torch.randint(1, 9, (1,), generator=gen)) if out else 8,), generator=gen).tolist())
        if len(out) % 7 == 6 and len(out[-1]) > 1:
            p = out[-1][:-1]
        if p not in seen:
            seen.add(p)
            out.append(p)
    return [list(p) for p in out]


def bench_kernels(B=64, reps=10):
    from gar_amd import LogitsProcessing, PhraseConstraint
    dev = "cuda:0"
    ld = (V + 63) // 64 * 64
    gen = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, ld, generator=gen) * 2.5).to(torch.bfloat16).to(dev)
    eos = torch.tensor([128001, 128009], dtype=torch.int64, device=dev)
    names, runs, keep = [], [], []
    for n in (4, 64, 1200):
        phrases = phrase_set(n)
        words = PhraseConstraint(phrases).pack(V, B)
        trie = torch.zeros(ops.CONSTRAINT_WORDS, dtype=torch.int32, device=dev)
        trie[:len(words)] = torch.tensor(words, dtype=torch.int32)
        long = [p for p in phrases if len(p) >= 4]
        for t in (0, 3):
            toks = torch.zeros((B, 64), dtype=torch.int64)
            for b in range(B):
                toks[b, :4] = torch.tensor(long[b % len(long)][:4])
            toks = toks.to(dev)
            nodes = torch.zeros((B, 65), dtype=torch.int32, device=dev)
            nodes[:, 0] = trie[4:4 + B]
            step = torch.zeros(1, dtype=torch.int32, device=dev)
            for s in range(1, t + 1):                       # walk the plane to step t
                step.fill_(s)
                ops.constrain(logits.clone(), V, toks, step, eos, trie, nodes)
            keep.append((trie, toks, nodes, step))
            names.append(f"constrain_{n}_phrases_t{t}")
            runs.append(_graph(lambda toks=toks, step=step, trie=trie, nodes=nodes:
                               [ops.constrain(logits, V, toks, step, eos, trie, nodes) for _ in range(LAUNCHES)]))
    params = torch.tensor(LogitsProcessing(**PROCESSING).pack(V), dtype=torch.int32, device=dev)
    ids = torch.randint(0, V, (64,), generator=gen)
    hist = ids[torch.randint(0, 64, (B, 64), generator=gen)].to(dev)
    step64 = torch.tensor([64], dtype=torch.int32, device=dev)
    plain = (torch.randn(B, ld, generator=gen) * 2.5).to(torch.bfloat16).to(dev)       # its own buffer: no -inf from the mask
    names.append("logits_process_penalty_ngram3_t64")
    runs.append(_graph(lambda: [ops.logits_process(plain, V, hist, step64, None, params) for _ in range(LAUNCHES)]))
    out = [[] for _ in runs]
    for _ in range(REPS):
        for i, launch in enumerate(runs):              # in turns
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1) / reps / LAUNCHES * 1e3)
    res = {"B": B, "V": V, "dtype": "bf16", "row_bytes": ld * 2, "processing": PROCESSING,
           "note": "repeated launches on one buffer: after the first, the rows already hold the mask (the stores are the same)",
           "us_per_call": dict(zip(names, (_stat(x) for x in out)))}
    worst = max(v["median"] for k, v in res["us_per_call"].items() if k.startswith("constrain"))
    res["constrain_at_most_logits_process"] = worst <= res["us_per_call"]["logits_process_penalty_ngram3_t64"]["median"]
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
    # 64 phrases longer than the run that share their first token and part at the second: every row walks one, none ends early
    phrases = [[1000, 2000 + k] + [3000 + j for j in range(new_tokens - 1)] for k in range(64)]
    forms = {"plain": lambda n: m.generate(**batch, max_new_tokens=n),
             "constrained": lambda n: m.generate(**batch, max_new_tokens=n, eos_token_id=128009, constraint=dict(phrases=phrases))}
    for name, fn in forms.items():                     # warm-up: graphs, workspaces
        fn(new_tokens)
        fn(1)
    torch.cuda.synchronize()
    full = {name: [] for name in forms}
    stepms = {name: [] for name in forms}
    for _ in range(REPS):
        for name, fn in forms.items():                 # in turns
            t0 = time.perf_counter()
            out = fn(new_tokens)
            torch.cuda.synchronize()
            f = time.perf_counter() - t0
            assert out.sequences.shape[1] == new_tokens
            t0 = time.perf_counter()
            fn(1)
            torch.cuda.synchronize()
            p = time.perf_counter() - t0
            full[name].append(f * 1e3)
            stepms[name].append((f - p) / (new_tokens - 1) * 1e3)
    res = {"model": "GAR-1B bf16 (synthetic weights)", "B": B, "new_tokens": new_tokens, "image_size": image_size,
           "note": "the constrained call polls its eos latch once per 16 tokens, the plain call has no eos id",
           "generate": {name: {"full_ms": _stat(full[name]), "decode_ms_per_token": _stat(stepms[name])} for name in forms}}
    print(json.dumps(res), flush=True)
    return res


def bench_headline(parent_tree):
    """bench.py --steps 10 --warmup 3: parent, this, parent, this, a fresh process each"""
    runs = []
    for name, tree in (("parent", parent_tree), ("this", ROOT)) * 2:
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3"], cwd=tree,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"bench.py in {tree} failed: {r.stderr[-2000:]}")
        line = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])
        runs.append({"tree": name, "value": line["value"], "unit": line["unit"], "metric": line["metric"]})
        print(json.dumps(runs[-1]), flush=True)
    parent = [x["value"] for x in runs if x["tree"] == "parent"]
    this = [x["value"] for x in runs if x["tree"] == "this"]
    floor = min(parent) - 2 * abs(parent[0] - parent[1])
    res = {"command": "python bench.py --gpus 1 --steps 10 --warmup 3", "order": "parent, this, parent, this", "runs": runs,
           "floor": floor, "rule": "both runs of this tree >= the slower parent run - 2 x the parents' gap",
           "holds": all(v >= floor for v in this)}
    print(json.dumps(res), flush=True)
    return res


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=448)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "_base"),
                    help="a built checkout of the parent commit (git worktree / git archive, then python __graft_entry__.py in it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain.json"))
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
        res["kernels"] = bench_kernels()
        save()
    if not a.skip_e2e:
        res["generate"] = bench_generate(a.new_tokens, a.image_size)
        save()
    if not a.skip_headline:
        if not os.path.isdir(os.path.join(a.parent_tree, PKG, "gar_amd")):
            raise SystemExit(f"--parent-tree {a.parent_tree}: no checkout of the parent commit there (or pass --skip-headline)")
        torch.cuda.empty_cache()
        res["headline"] = bench_headline(a.parent_tree)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
