#!/usr/bin/env python
"""generate(sampling_warpers=...): what the four further warpers cost. Writes profiles/sampling_warpers.json:

  kernels    us per call at B = 64, V = 128256 (GAR-1B's vocabulary), f32 and bf16, temperature 0.8 / top_k 50 / top_p 0.95:
             gar_sample, gar_sample_ext with all four off, with each warper alone (min_p 0.02, typical_p 0.95, epsilon 1e-3, eta
             2e-3) and with all four; hipGraph replays of LAUNCHES calls on one logits buffer, device events around the replays, the
             forms in turns in one process. Each form as a ratio to gar_sample in the same run, beside the spread of gar_sample's
             own repeats
  generate   synthetic GAR-1B bf16, 64 rows, eos disabled, 64 tokens, do_sample: the whole call and the decode loop alone
             (generate_finish, ms / step) without the parameter and with all four warpers, in turns in one process
  default    the decode ms / step of the call WITHOUT the parameter (greedy and sampled) in a built checkout of the parent commit
             (--parent-tree) and in this tree: a fresh process per run, the two trees in turns (which one goes first alternates),
             --loop-reps runs each. Recorded: every run's figure, each tree's run-to-run spread, and whether this tree's median lies
             within the parent's spread of the parent's median

Every figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_sampling_warpers.py [--skip-kernels] [--skip-generate] [--skip-default] [--reps R] [--loop-reps R]
                                               [--parent-tree DIR] [--image-size S]
       python tools/bench_sampling_warpers.py --default-only --package-root DIR     (one run of the default path, one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "grasp-any-region_amd"
if "--package-root" in sys.argv:            # the default path of another tree (the parent commit's): its package, its libraries
    sys.path.insert(0, os.path.join(os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]), PKG))
else:
    sys.path.insert(0, os.path.join(ROOT, PKG))
import torch  # noqa: E402

from gar_amd import hip, ops  # noqa: E402

REPS = 5
LAUNCHES = 20
V = 128256
SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.95)
WARPERS = dict(min_p=0.02, typical_p=0.95, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


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
    dev = "cuda:0"
    ld = (V + 63) // 64 * 64
    gen = torch.Generator().manual_seed(0)
    head = [SAMPLING["temperature"], SAMPLING["top_p"], float(SAMPLING["top_k"]), 0.0]
    seed = torch.tensor([1234], dtype=torch.int64, device=dev)
    step = torch.tensor([3], dtype=torch.int32, device=dev)
    forms = {"gar_sample": None, "ext_all_off": OFF}
    forms.update({f"ext_{k}": dict(OFF, **{k: v}) for k, v in WARPERS.items()})
    forms["ext_all_four"] = WARPERS
    names, runs, keep, same, kept = [], [], [], {}, {}
    for dtype, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        logits = (torch.randn(B, ld, generator=gen) * 2.5).to(dtype).to(dev)
        curs = {}
        for name, w in forms.items():
            out, cur = torch.zeros((B, 8), dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
            nk = torch.zeros(B, dtype=torch.int32, device=dev)
            if w is None:
                p = torch.tensor(head, dtype=torch.float32, device=dev)
                fn = (lambda lg=logits, o=out, c=cur, p=p: ops.sample(lg, V, o, 8, step, c, p, seed))
            else:
                p = torch.tensor(head + [w[k] for k in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")], dtype=torch.float32,
                                 device=dev)
                fn = (lambda lg=logits, o=out, c=cur, p=p, nk=nk: ops.sample_ext(lg, V, o, 8, step, c, p, seed, n_kept=nk))
            keep.append((logits, out, cur, nk, p))
            curs[name] = (cur, nk)
            names.append(f"{dname}_{name}")
            runs.append(_graph(lambda fn=fn: [fn() for _ in range(LAUNCHES)]))
        torch.cuda.synchronize()
        same[dname] = bool(torch.equal(curs["gar_sample"][0], curs["ext_all_off"][0]))       # all off: gar_sample's tokens
        kept[dname] = {name: float(nk.float().mean()) for name, (_, nk) in curs.items() if name != "gar_sample"}
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
    res = {"B": B, "V": V, "sampling": SAMPLING, "warpers": WARPERS, "us_per_call": us, "all_off_tokens_equal_gar_sample": same,
           "mean_n_kept": kept, "ratios_to_gar_sample": {}}
    for dname in ("f32", "bf16"):
        base = us[f"{dname}_gar_sample"]
        r = {name: us[f"{dname}_{name}"]["median"] / base["median"] for name in forms if name != "gar_sample"}
        r["gar_sample_spread_over_median"] = (base["max"] - base["min"]) / base["median"]
        res["ratios_to_gar_sample"][dname] = r
    print(json.dumps(res), flush=True)
    return res


def _model_and_batch(image_size, B=64):
    from gar_amd import GARConfig
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    smp = [SingleRegionCaptionDataset(synthetic_image(i, image_size, image_size), synthetic_mask(i, image_size, image_size), proc,
                                      data_dtype=torch.bfloat16, device="cpu")[0] for i in range(8)]
    smp = [smp[i % 8] for i in range(B)]
    batch = {k: torch.cat([s[k] for s in smp], 0) if isinstance(smp[0][k], torch.Tensor) else [x for s in smp for x in s[k]]
             for k in smp[0]}
    return GARModel(cfg, synthetic_weights(cfg), torch.bfloat16), batch


def bench_generate(new_tokens, image_size, default_only=False):
    m, batch = _model_and_batch(image_size)
    gc = dict(do_sample=True, max_new_tokens=new_tokens, **SAMPLING)
    forms = {"greedy": dict(max_new_tokens=new_tokens), "sampled": dict(gc, seed=7)}
    if not default_only:
        forms["sampled_all_four_warpers"] = dict(gc, seed=7, sampling_warpers=WARPERS)

    def run(name):
        """(ms of the whole call, ms per decode step): the decode loop is generate_finish, timed from behind the prompt phase"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pend = m.generate_begin(**batch, **forms[name])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = m.generate_finish(pend)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert out.sequences.shape[1] == new_tokens
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3 / (new_tokens - 1), out.sequences.cpu()
    seqs = {name: run(name)[2] for name in forms}           # warm-up: states, graphs
    whole, step = {n: [] for n in forms}, {n: [] for n in forms}
    for _ in range(REPS):
        for name in forms:                                  # in turns
            a, b, _ = run(name)
            whole[name].append(a)
            step[name].append(b)
    out = {"model": "GAR-1B bf16 (synthetic weights)", "rows": 64, "new_tokens": new_tokens, "image_size": image_size,
           "call_ms": {n: _stat(whole[n]) for n in forms}, "decode_ms_per_step": {n: _stat(step[n]) for n in forms}}
    if not default_only:
        out["sampling"], out["warpers"] = SAMPLING, WARPERS
        out["warpers_change_tokens"] = not torch.equal(seqs["sampled"], seqs["sampled_all_four_warpers"])
    print(json.dumps(out), flush=True)
    return out


def bench_default_path(parent_tree, reps, new_tokens, image_size):
    """the parameter-free call's decode ms / step in the parent commit's tree and in this one: a fresh process per run, in turns"""
    trees = {"parent": parent_tree, "this": ROOT}
    vals = {form: {name: [] for name in trees} for form in ("greedy", "sampled")}
    for rep in range(reps):
        for name, tree in (list(trees.items())[::-1] if rep % 2 else trees.items()):      # in turns, the first one alternating too
            cmd = [sys.executable, os.path.abspath(__file__), "--default-only", "--package-root", tree, "--new-tokens", str(new_tokens),
                   "--image-size", str(image_size), "--reps", str(REPS)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"the default path with the package of {tree} failed: {r.stderr[-2000:]}")
            line = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])
            for form in vals:
                vals[form][name].append(line["decode_ms_per_step"][form]["median"])
            print(json.dumps({"tree": name, **{form: vals[form][name][-1] for form in vals}}), flush=True)
    out = {"what": "decode ms / step of generate() without sampling_warpers, median of each fresh process",
           "order": "parent first in even repeats, this tree first in odd ones"}
    for form, v in vals.items():
        o = {"runs": v, **{name: _stat(x) for name, x in v.items()}}
        for name in trees:
            o[name]["spread"] = o[name]["max"] - o[name]["min"]
        o["this_minus_parent"] = o["this"]["median"] - o["parent"]["median"]
        o["within_parent_spread"] = abs(o["this_minus_parent"]) <= o["parent"]["spread"]
        out[form] = o
    print(json.dumps(out), flush=True)
    return out


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-default", action="store_true")
    ap.add_argument("--default-only", action="store_true", help="one run of the parameter-free calls with the package under --package-root")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=448)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--loop-reps", type=int, default=4)
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "_base"),
                    help="a built checkout of the parent commit (git worktree / git archive, then python __graft_entry__.py in it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_warpers.json"))
    a = ap.parse_args()
    REPS = a.reps
    hip.require_device(0)
    if a.default_only:
        bench_generate(a.new_tokens, a.image_size, default_only=True)
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
    if not a.skip_generate:
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
