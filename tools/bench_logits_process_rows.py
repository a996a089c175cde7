#!/usr/bin/env python
"""ContinuousBatcher(processing=True): what per-request logits processing costs. Writes profiles/logits_process_rows.json:

  kernels    us per call at B = 64, V = 128256 (GAR-1B's vocabulary), f32 and bf16, history 64 and 1023 tokens over 64 ids, repetition
             penalty 1.2 + no_repeat_ngram_size 3 (the parameter set of tools/bench_logits_process.py): gar_logits_process_rows with
             every row under that block (col0 = 0) against gar_logits_process on the same work, gar_logits_process_rows with every
             header zero, and — with --parent-lib — gar_logits_process out of the parent commit's library; hipGraph replays of
             LAUNCHES calls on one logits buffer, device events around the replays, the forms in turns in one process
  loop       ContinuousBatcher, 64 rows, synthetic GAR-1B bf16, eos disabled, 64 tokens per region: decode ms / step (the cycles
             after the one prompt phase that fills the rows: graph replays and polls) for processing=False, processing=True with
             unprocessed tickets and processing=True with every ticket processed, in turns in one process; and processing=False
             once more out of a batcher built last, the control for what two KV states of one form differ by

Every figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_logits_process_rows.py [--skip-kernels] [--skip-loop] [--reps R] [--parent-lib libgar_hip.so] [--image-size S]"""
import argparse
import ctypes
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


def _parent_entry(path):
    """gar_logits_process of another build of the library (the parent commit's), with ops.logits_process's arguments"""
    lib = ctypes.CDLL(os.path.abspath(path))
    fn = lib.gar_logits_process
    fn.argtypes, fn.restype = hip.SIGNATURES["gar_logits_process"]

    def call(logits, V_, out_tokens, step_dev, eos_ids, params):
        head = ops._logits_process_args(logits, V_, out_tokens, step_dev, eos_ids)
        ops.check(fn(*head, ops.ptr(params), params.numel(), ops.stream()), "gar_logits_process (parent library)")
    return call


def bench_kernels(parent_lib=None, B=64, reps=10):
    from gar_amd import LogitsProcessing
    from gar_amd.continuous import pack_process_row
    dev = "cuda:0"
    ld = (V + 63) // 64 * 64
    proc = LogitsProcessing(**PROCESSING)
    params = torch.tensor(proc.pack(V), dtype=torch.int32, device=dev)
    words = pack_process_row(proc, V, (), 0)
    rows = torch.zeros((B, ops.LOGITS_PROCESS_WORDS), dtype=torch.int32)
    rows[:, :len(words)] = torch.tensor(words, dtype=torch.int32)
    rows, zero = rows.to(dev), torch.zeros((B, ops.LOGITS_PROCESS_WORDS), dtype=torch.int32, device=dev)
    parent = _parent_entry(parent_lib) if parent_lib else None
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(0, V, (64,), generator=gen)
    names, runs, keep, same = [], [], [], {}
    for dtype, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        base = (torch.randn(B, ld, generator=gen) * 2.5).to(dtype)
        for t in (64, 1023):
            hist = ids[torch.randint(0, 64, (B, 1024), generator=gen)].to(dev)
            step = torch.tensor([t], dtype=torch.int32, device=dev)
            forms = [("gar_logits_process", lambda lg: ops.logits_process(lg, V, hist, step, None, params)),
                     ("gar_logits_process_rows", lambda lg: ops.logits_process_rows(lg, V, hist, step, None, rows)),
                     ("gar_logits_process_rows_no_request", lambda lg: ops.logits_process_rows(lg, V, hist, step, None, zero))]
            if parent is not None:
                forms.append(("gar_logits_process_parent", lambda lg: parent(lg, V, hist, step, None, params)))
            once = {}
            for name, fn in forms:                     # one launch each on a copy of the same logits: the same bytes come out
                lg = base.to(dev)
                fn(lg)
                torch.cuda.synchronize()
                once[name] = lg
            same[f"{dname}_t{t}"] = all(torch.equal(once["gar_logits_process"].view(torch.uint8), once[n].view(torch.uint8))
                                        for n in once if n != "gar_logits_process_rows_no_request") and \
                torch.equal(once["gar_logits_process_rows_no_request"].cpu(), base)
            for name, fn in forms:
                lg = base.to(dev)
                keep.append((lg, hist, step))
                names.append(f"{dname}_t{t}_{name}")
                runs.append(_graph(lambda fn=fn, lg=lg: [fn(lg) for _ in range(LAUNCHES)]))
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
    res = {"B": B, "V": V, "processing": PROCESSING, "us_per_call": us, "bytes_equal": same, "ratios": {}}
    for key in same:
        old = us[f"{key}_gar_logits_process"]
        r = {"rows_over_gar_logits_process": us[f"{key}_gar_logits_process_rows"]["median"] / old["median"],
             "gar_logits_process_spread_over_median": (old["max"] - old["min"]) / old["median"]}
        if parent is not None:
            r["this_tree_over_parent_library"] = old["median"] / us[f"{key}_gar_logits_process_parent"]["median"]
        res["ratios"][key] = r
    print(json.dumps(res), flush=True)
    return res


def bench_loop(new_tokens, image_size, B=64):
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
    forms = {"processing_off": ({}, {}), "processing_on_unprocessed_tickets": (dict(processing=True), {}),
             "processing_on_processed_tickets": (dict(processing=True), dict(logits_processing=PROCESSING)),
             # the control: a second batcher of the first form, built last — every form decodes out of a KV state of its own, and
             # what two states of ONE form differ by is not the processing's cost
             "processing_off_again": ({}, {})}
    cbs = {name: ContinuousBatcher(m, slots=B, max_new_tokens=new_tokens, **ckw) for name, (ckw, _) in forms.items()}

    def run(name):
        """(ms per decode step, decode steps, tokens): the rows are filled by ONE prompt phase, timed from behind it"""
        cb, skw = cbs[name], forms[name][1]
        tickets = [cb.submit(distinct[i % 8], **skw) for i in range(B)]
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
           "image_size": image_size, "processing": PROCESSING, "decode_ms_per_step": {name: _stat(ms[name]) for name in forms},
           "unprocessed_tickets_equal_processing_off": toks["processing_on_unprocessed_tickets"] == toks["processing_off"],
           "processed_tickets_differ": toks["processing_on_processed_tickets"] != toks["processing_off"]}
    print(json.dumps(out), flush=True)
    return out


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=448)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--parent-lib", default=None, help="libgar_hip.so of a build of the parent commit: its gar_logits_process is timed "
                                                       "beside this tree's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logits_process_rows.json"))
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
        res["kernels"] = bench_kernels(a.parent_lib)
        save()
    if not a.skip_loop:
        res["loop"] = bench_loop(a.new_tokens, a.image_size)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
