#!/usr/bin/env python
"""generate(logits_processing=...): what the device-side logits processors cost. Writes profiles/logits_process.json:

  kernels    us per call of gar_logits_process at B = 64, V = 128256 (GAR-1B's vocabulary), history length t in {1, 64, 1024}, f32 and
             bf16, repetition penalty 1.2 + no_repeat_ngram_size 3 (histories over 64 ids, so n-grams do repeat); hipGraph replays
             of LAUNCHES calls on one logits buffer, device events around the replays
  generate   a 64-token greedy generate at B = 64, synthetic GAR-1B bf16, eos disabled — decode ms / token ((full - the same
             call with max_new_tokens = 1) / 63) without the parameter and with penalty 1.2 + n = 3, in turns in one process
  default    the same loop WITHOUT the parameter in a built checkout of the parent commit (--parent-tree) and in this tree: a fresh
             process per run, the two trees in turns (which one goes first alternates), --loop-reps runs each. Recorded: every
             run's figure, each tree's run-to-run spread (max - min of its runs), and whether this tree's median lies within the
             parent's spread of the parent's median

Every figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_logits_process.py [--skip-kernels] [--skip-e2e] [--skip-default] [--reps R] [--loop-reps R]
                                            [--parent-tree DIR] [--image-size S]
       python tools/bench_logits_process.py --loop-only --package-root DIR     (one run of the plain loop, one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "grasp-any-region_amd"
if "--package-root" in sys.argv:            # the plain loop of another tree (the parent commit's): its package, its libraries
    sys.path.insert(0, os.path.join(os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]), PKG))
else:
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


def bench_kernels(B=64, reps=10):
    from gar_amd import LogitsProcessing
    dev = "cuda:0"
    ld = (V + 63) // 64 * 64
    params = torch.tensor(LogitsProcessing(**PROCESSING).pack(V), dtype=torch.int32, device=dev)
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(0, V, (64,), generator=gen)
    names, runs, keep = [], [], []
    for dtype, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        logits = (torch.randn(B, ld, generator=gen) * 2.5).to(dtype).to(dev)
        for t in (1, 64, 1024):
            hist = ids[torch.randint(0, 64, (B, 1024), generator=gen)].to(dev)
            step = torch.tensor([t], dtype=torch.int32, device=dev)
            keep.append((logits, hist, step))
            names.append(f"{dname}_t{t}")
            runs.append(_graph(lambda logits=logits, hist=hist, step=step:
                               [ops.logits_process(logits, V, hist, step, None, params) for _ in range(LAUNCHES)]))
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
    res = {"B": B, "V": V, "processing": PROCESSING, "us_per_call": dict(zip(names, (_stat(x) for x in out)))}
    print(json.dumps(res), flush=True)
    return res


def _batch(ss):
    return dict(input_ids=torch.cat([s["input_ids"] for s in ss]), pixel_values=torch.cat([s["pixel_values"] for s in ss]),
                global_mask_values=torch.cat([s["global_mask_values"] for s in ss]), bboxes=[b for s in ss for b in s["bboxes"]],
                aspect_ratios=torch.cat([s["aspect_ratios"] for s in ss]))


def bench_generate(new_tokens, image_size, B=64, plain_only=False):
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
    forms = {"plain": lambda n: m.generate(**batch, max_new_tokens=n)}
    if not plain_only:
        forms["penalty_1.2_ngram_3"] = lambda n: m.generate(**batch, max_new_tokens=n, logits_processing=PROCESSING)
    seqs = {}
    for name, fn in forms.items():                     # warm-up: graphs, workspaces
        seqs[name] = fn(new_tokens).sequences
        fn(1)
    torch.cuda.synchronize()
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
           "generate": {name: {"full_ms": _stat(full[name]), "decode_ms_per_token": _stat(stepms[name])} for name in forms}}
    if not plain_only:
        out["sequences_differ_from_plain"] = not torch.equal(seqs["plain"], seqs["penalty_1.2_ngram_3"])
    print(json.dumps(out), flush=True)
    return out


def bench_default_path(parent_tree, reps, new_tokens, image_size):
    """the plain loop's decode ms / token in the parent commit's tree and in this one: a fresh process per run, in turns"""
    trees = {"parent": parent_tree, "this": ROOT}
    vals = {name: [] for name in trees}
    for rep in range(reps):
        for name, tree in (list(trees.items())[::-1] if rep % 2 else trees.items()):      # in turns, the first one alternating too
            cmd = [sys.executable, os.path.abspath(__file__), "--loop-only", "--package-root", tree, "--new-tokens", str(new_tokens),
                   "--image-size", str(image_size), "--reps", str(REPS)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"the plain loop with the package of {tree} failed: {r.stderr[-2000:]}")
            line = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])
            vals[name].append(line["generate"]["plain"]["decode_ms_per_token"]["median"])
            print(json.dumps({"tree": name, "decode_ms_per_token": vals[name][-1]}), flush=True)
    out = {"what": "decode ms / token of the plain loop (no logits_processing), median of each fresh process",
           "runs": vals, "order": "parent first in even repeats, this tree first in odd ones", **{name: _stat(v) for name, v in vals.items()}}
    for name in trees:
        out[name]["spread"] = out[name]["max"] - out[name]["min"]
    out["this_minus_parent"] = out["this"]["median"] - out["parent"]["median"]
    out["within_parent_spread"] = abs(out["this_minus_parent"]) <= out["parent"]["spread"]
    print(json.dumps(out), flush=True)
    return out


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-default", action="store_true")
    ap.add_argument("--loop-only", action="store_true", help="one run of the plain loop with the package under --package-root")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=448)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--loop-reps", type=int, default=4)
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "_base"),
                    help="a built checkout of the parent commit (git worktree / git archive, then python __graft_entry__.py in it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logits_process.json"))
    a = ap.parse_args()
    REPS = a.reps
    hip.require_device(0)
    if a.loop_only:
        bench_generate(a.new_tokens, a.image_size, plain_only=True)
        return
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
    if not a.skip_default:
        if not os.path.isdir(os.path.join(a.parent_tree, PKG, "gar_amd")):
            raise SystemExit(f"--parent-tree {a.parent_tree}: no checkout of the parent commit there (or pass --skip-default)")
        torch.cuda.empty_cache()
        res["default_path"] = bench_default_path(a.parent_tree, a.loop_reps, a.new_tokens, a.image_size)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
