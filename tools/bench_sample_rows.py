#!/usr/bin/env python
"""ContinuousBatcher(sampling=True): what per-request sampling costs. Writes profiles/sample_rows.json:

  kernels    us per call at B = 64, V = 128256 (GAR-1B's vocabulary), f32 and bf16: gar_sample_rows with every row sampled against
             gar_sample at the same parameters (temperature 0.8, top_k 50, top_p 0.9), and gar_sample_rows with every row greedy
             against gar_argmax; hipGraph replays of LAUNCHES calls on one logits buffer, device events around the replays, the
             four forms in turns in one process
  loop       ContinuousBatcher, 64 rows, synthetic GAR-1B bf16, eos disabled, 64 tokens per region: decode ms / step (the cycles
             after the one prompt phase that fills the rows: graph replays and polls) for sampling=False, sampling=True with greedy
             tickets and sampling=True with sampled tickets, in turns in one process
  default    the sampling=False loop in a built checkout of the parent commit (--parent-tree) and in this tree: a fresh process per
             run, the two trees in turns (which one goes first alternates), --loop-reps runs each. Recorded: every run's figure, each
             tree's run-to-run spread (max - min of its runs), and whether this tree's median lies within the parent's spread of the
             parent's median

Every figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_sample_rows.py [--skip-kernels] [--skip-loop] [--skip-default] [--reps R] [--loop-reps R]
                                          [--parent-tree DIR] [--image-size S]
       python tools/bench_sample_rows.py --loop-only --package-root DIR     (one run of the sampling=False loop, one JSON line)"""
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
SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.9)


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
    from gar_amd.continuous import pack_sample_row
    dev = "cuda:0"
    ld = (V + 63) // 64 * 64
    gen = torch.Generator().manual_seed(0)
    request = (SAMPLING["temperature"], SAMPLING["top_p"], SAMPLING["top_k"])
    params = torch.tensor([request[0], request[1], float(request[2]), 0.0], dtype=torch.float32, device=dev)
    seed = torch.tensor([1234], dtype=torch.int64, device=dev)
    # the same draws in both forms: key 1234, step 3, counter row b
    sampled = torch.tensor([pack_sample_row(request, 1234, 0, b) for b in range(B)], dtype=torch.int32, device=dev)
    greedy = torch.tensor([pack_sample_row(None, None, 0) for _ in range(B)], dtype=torch.int32, device=dev)
    step = torch.tensor([3], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.argmax_workspace(B, V), dtype=torch.uint8, device=dev)
    names, runs, keep, same = [], [], [], {}
    for dtype, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        logits = (torch.randn(B, ld, generator=gen) * 2.5).to(dtype).to(dev)
        outs = [torch.zeros((B, 8), dtype=torch.int64, device=dev) for _ in range(4)]
        curs = [torch.zeros(B, dtype=torch.int64, device=dev) for _ in range(4)]
        keep.append((logits, outs, curs))
        forms = (("gar_sample", lambda o, c, lg=logits: ops.sample(lg, V, o, 8, step, c, params, seed)),
                 ("gar_sample_rows_sampled", lambda o, c, lg=logits: ops.sample_rows(lg, V, o, 8, step, c, sampled)),
                 ("gar_argmax", lambda o, c, lg=logits: ops.argmax(lg, V, o, 8, step, c, ws)),
                 ("gar_sample_rows_greedy", lambda o, c, lg=logits: ops.sample_rows(lg, V, o, 8, step, c, greedy)))
        for (name, fn), o, c in zip(forms, outs, curs):
            names.append(f"{dname}_{name}")
            runs.append(_graph(lambda fn=fn, o=o, c=c: [fn(o, c) for _ in range(LAUNCHES)]))
        torch.cuda.synchronize()
        same[dname] = bool(torch.equal(curs[0], curs[1]) and torch.equal(curs[2], curs[3]))      # both pairs picked the same tokens
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
    us = dict(zip(names, (_stat(x) for x in out)))
    res = {"B": B, "V": V, "sampling": SAMPLING, "us_per_call": us, "tokens_equal": same, "ratios": {}}
    for dname in ("f32", "bf16"):
        base = us[f"{dname}_gar_sample"]
        res["ratios"][dname] = {
            "rows_sampled_over_gar_sample": us[f"{dname}_gar_sample_rows_sampled"]["median"] / base["median"],
            "gar_sample_spread_over_median": (base["max"] - base["min"]) / base["median"],
            "rows_greedy_over_gar_argmax": us[f"{dname}_gar_sample_rows_greedy"]["median"] / us[f"{dname}_gar_argmax"]["median"]}
    print(json.dumps(res), flush=True)
    return res


def bench_loop(new_tokens, image_size, B=64, plain_only=False):
    from gar_amd import GARConfig
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    distinct = [SingleRegionCaptionDataset(synthetic_image(i, image_size, image_size), synthetic_mask(i, image_size, image_size), proc,
                                           data_dtype=torch.bfloat16, device="cpu")[0] for i in range(8)]
    m = GARModel(cfg, synthetic_weights(cfg), torch.bfloat16)
    # (constructor keywords, submit keywords of ticket i); the plain form uses nothing the parent commit's batcher lacks
    forms = {"sampling_off": ({}, lambda i: {})}
    if not plain_only:
        forms["sampling_on_greedy_tickets"] = (dict(sampling=True), lambda i: {})
        forms["sampling_on_sampled_tickets"] = (dict(sampling=True), lambda i: dict(do_sample=True, seed=1000 + i, **SAMPLING))
    cbs = {name: ContinuousBatcher(m, slots=B, max_new_tokens=new_tokens, **ckw) for name, (ckw, _) in forms.items()}

    def run(name):
        """(ms per decode step, decode steps, tokens): the rows are filled by ONE prompt phase, timed from behind it"""
        cb, skw = cbs[name], forms[name][1]
        tickets = [cb.submit(distinct[i % 8], **skw(i)) for i in range(B)]
        with torch.cuda.device(m.device):
            cb._admit(True)
        assert cb.n_active == B and not cb.queue
        steps0 = cb.stats["decode_steps"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cb.flush()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = cb.stats["decode_steps"] - steps0
        toks = [cb.results[t] for t in tickets]
        cb.pop_finished()
        return dt / steps * 1e3, steps, toks
    toks = {name: run(name)[2] for name in forms}           # warm-up: states, graphs
    ms = {name: [] for name in forms}
    steps = 0
    for _ in range(REPS):
        for name in forms:                                  # in turns
            v, steps, _ = run(name)
            ms[name].append(v)
    out = {"model": "GAR-1B bf16 (synthetic weights)", "slots": B, "new_tokens": new_tokens, "decode_steps": steps,
           "image_size": image_size, "decode_ms_per_step": {name: _stat(ms[name]) for name in forms}}
    if not plain_only:
        out["sampling"] = SAMPLING
        out["greedy_tickets_equal_sampling_off"] = toks["sampling_on_greedy_tickets"] == toks["sampling_off"]
        out["sampled_tickets_differ"] = toks["sampling_on_sampled_tickets"] != toks["sampling_off"]
    print(json.dumps(out), flush=True)
    return out


def bench_default_path(parent_tree, reps, new_tokens, image_size):
    """the sampling=False loop's decode ms / step in the parent commit's tree and in this one: a fresh process per run, in turns"""
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
            vals[name].append(line["decode_ms_per_step"]["sampling_off"]["median"])
            print(json.dumps({"tree": name, "decode_ms_per_step": vals[name][-1]}), flush=True)
    out = {"what": "decode ms / step of the sampling=False loop, median of each fresh process",
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
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-default", action="store_true")
    ap.add_argument("--loop-only", action="store_true", help="one run of the sampling=False loop with the package under --package-root")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=448)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--loop-reps", type=int, default=4)
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "_base"),
                    help="a built checkout of the parent commit (git worktree / git archive, then python __graft_entry__.py in it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rows.json"))
    a = ap.parse_args()
    REPS = a.reps
    hip.require_device(0)
    if a.loop_only:
        bench_loop(a.new_tokens, a.image_size, plain_only=True)
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
    if not a.skip_loop:
        res["loop"] = bench_loop(a.new_tokens, a.image_size)
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
