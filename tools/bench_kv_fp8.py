#!/usr/bin/env python
"""FP8 KV cache (GARModel(kv_cache_dtype="fp8")) against the default 16-bit cache. Writes profiles/kv_fp8.json:

  attention   us per launch and fraction of HBM of gar_attention_decode vs gar_attention_decode_fp8 (hipGraph replays over
              distinct caches, so the bytes come from HBM) at GAR-1B (Hq 32, Hkv 8, hd 64) B = 64, kv = S = 4718 and at GAR-8B
              (hd 128); algorithmic bytes: K + V (+ their f32 scales for fp8)
  quantize    gar_kv_quantize_fp8 over one layer of the B = 64 prefill (reads 16-bit K / V, writes bytes + scales)
  generate    regions/s of GARModel.generate, default cache and fp8, synthetic GAR-1B weights, 16-tile regions
  continuous  regions/s of a ContinuousBatcher run with long captions (max_new_tokens >= 256, eos ids cutting them at mixed
              lengths), both caches

Every figure is the median of --reps timed repeats, with their min and max ("spread"). Every number is from synthetic weights;
the quality side is in tests/test_gpu_kv_fp8.py.
Usage: python tools/bench_kv_fp8.py [--skip-e2e] [--regions N] [--long-tokens T] [--reps R]"""
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

PEAK_HBM_GBS = 8000.0
REPS = 5


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def _time(launch, reps):
    """median / min / max over REPS timed batches of `reps` launches each, us per launch"""
    launch()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return _stat(out)


def _row(us, nb):
    return {"us": us, "bytes": nb, "TB/s": nb / us["median"] / 1e6, "hbm_frac": nb / us["median"] / 1e3 / PEAK_HBM_GBS}


def _per(st, L):
    return {k: (v / L if k != "n" else v) for k, v in st.items()}


def bench_attention(B, Hq, Hkv, hd, kv, L=4, reps=20):
    dev, dt = "cuda:0", torch.bfloat16
    Smax = (kv + 63) // 64 * 64
    nsplit = max(1, min(8, 192 // (B * Hkv)))           # GARModel.DECODE_ATTN_* at this batch
    q = torch.randn(B, Hq, hd, device=dev).to(dt)
    O = torch.empty(B, Hq * hd, device=dev, dtype=dt)
    kvl = torch.tensor([kv], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.attention_decode_workspace(B, Hq, hd, nsplit), dtype=torch.uint8, device=dev)
    res = {"B": B, "Hq": Hq, "Hkv": Hkv, "hd": hd, "kv_len": kv, "nsplit": nsplit}
    K16 = [torch.randn(B, Hkv, Smax, hd, device=dev).to(dt) for _ in range(L)]
    V16 = [torch.randn(B, Hkv, Smax, hd, device=dev).to(dt) for _ in range(L)]

    def graph(fn):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g.replay

    run16 = graph(lambda: [ops.attention_decode(q, K16[i], V16[i], O, B, Hq, Hkv, hd, Smax, kvl, nsplit, ws) for i in range(L)])
    us16 = _per(_time(run16, reps), L)
    res["bf16"] = _row(us16, B * Hkv * kv * hd * 2 * 2)
    K8 = [torch.empty(B, Hkv, Smax, hd, dtype=torch.uint8, device=dev) for _ in range(L)]
    V8 = [torch.empty_like(K8[0]) for _ in range(L)]
    Ks = [torch.empty(B, Hkv, Smax, device=dev) for _ in range(L)]
    Vs = [torch.empty_like(Ks[0]) for _ in range(L)]
    for i in range(L):
        ops.kv_quantize_fp8(K16[i], V16[i], K8[i], V8[i], Ks[i], Vs[i], B, Hkv, hd, Smax, Smax)
    # one layer of a prefill's quantize launch (the B sequences' S rows)
    qus = _time(lambda: ops.kv_quantize_fp8(K16[0], V16[0], K8[0], V8[0], Ks[0], Vs[0], B, Hkv, hd, Smax, kv), reps)
    res["quantize"] = _row(qus, B * Hkv * kv * (hd * 2 * 2 + hd * 2 + 8))
    del K16, V16
    run8 = graph(lambda: [ops.attention_decode_fp8(q, K8[i], V8[i], Ks[i], Vs[i], O, B, Hq, Hkv, hd, Smax, kvl, nsplit, ws)
                          for i in range(L)])
    us8 = _per(_time(run8, reps), L)
    res["fp8"] = _row(us8, B * Hkv * kv * (hd + 4) * 2)
    res["fp8_speedup"] = us16["median"] / us8["median"]
    print(json.dumps(res), flush=True)
    return res


def _samples(cfg, proc, n, base=0):
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    return [SingleRegionCaptionDataset(synthetic_image(base + i, 1024, 1024), synthetic_mask(base + i, 1024, 1024), proc,
                                       data_dtype=torch.bfloat16, device="cpu")[0] for i in range(n)]


def _batch(ss):
    return dict(input_ids=torch.cat([s["input_ids"] for s in ss]), pixel_values=torch.cat([s["pixel_values"] for s in ss]),
                global_mask_values=torch.cat([s["global_mask_values"] for s in ss]), bboxes=[b for s in ss for b in s["bboxes"]],
                aspect_ratios=torch.cat([s["aspect_ratios"] for s in ss]))


def bench_e2e(n_regions, new_tokens, long_tokens, slots):
    from gar_amd import GARConfig
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    ss = _samples(cfg, proc, n_regions)
    batch = _batch(ss)
    out = {"model": "GAR-1B (synthetic weights)", "regions": n_regions, "new_tokens": new_tokens}
    streams = None
    for mode in (None, "fp8"):
        m = GARModel(cfg, W, torch.bfloat16, kv_cache_dtype=mode)
        name = mode or "bf16"
        m.generate(**batch, max_new_tokens=new_tokens)                  # warm-up: graphs, workspaces
        m.generate(**batch, max_new_tokens=1)
        torch.cuda.synchronize()
        rps, step_ms = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            r = m.generate(**batch, max_new_tokens=new_tokens)
            torch.cuda.synchronize()
            dt_full = time.perf_counter() - t0
            t0 = time.perf_counter()
            m.generate(**batch, max_new_tokens=1)
            torch.cuda.synchronize()
            dt_prompt = time.perf_counter() - t0
            rps.append(n_regions / dt_full)
            step_ms.append((dt_full - dt_prompt) / (new_tokens - 1) * 1e3)
        out[name] = {"regions_per_s": _stat(rps), "decode_step_ms": _stat(step_ms)}
        if mode is None:
            base_tokens = r.sequences.cpu()
        else:
            out["fp8_tokens_equal_bf16_fraction"] = float((r.sequences.cpu() == base_tokens).float().mean())
        # long captions through the continuous batcher: eos ids picked from the default cache's own streams
        if streams is None:
            lt = m.generate(**batch, max_new_tokens=long_tokens).sequences.cpu().tolist()
            cand = sorted({t for s in lt for t in s[long_tokens // 8:]})
            eos = cand[:: max(1, len(cand) // 6)][:6]
            streams = lt
            lens = [next((j + 1 for j, t in enumerate(s) if t in eos), long_tokens) for s in lt]
            out["continuous_eos_lengths"] = {"mean": sum(lens) / len(lens), "min": min(lens), "max": max(lens)}
        cb = ContinuousBatcher(m, slots=slots, max_new_tokens=long_tokens, eos_token_id=eos, poll_every=4, admit_min=1)
        for s in ss[: slots // 2]:
            cb.submit(s)
        cb.flush()                                                      # warm-up
        torch.cuda.synchronize()
        crps, steps = [], []
        for _ in range(REPS):
            s0 = cb.stats["decode_steps"]
            t0 = time.perf_counter()
            for s in ss:
                cb.submit(s)
            cb.flush()
            torch.cuda.synchronize()
            crps.append(n_regions / (time.perf_counter() - t0))
            steps.append(cb.stats["decode_steps"] - s0)
        out[name]["continuous"] = {"regions_per_s": _stat(crps), "slots": slots, "max_new_tokens": long_tokens,
                                   "decode_steps": steps}
        print(json.dumps({name: out[name]}), flush=True)
        del m, cb
        torch.cuda.empty_cache()
    return out


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--regions", type=int, default=64)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--long-tokens", type=int, default=256)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_fp8.json"))
    a = ap.parse_args()
    REPS = a.reps
    hip.require_device(0)
    res = {"device": torch.cuda.get_device_name(0), "peak_hbm_GBs": PEAK_HBM_GBS,
           # GAR-1B at B = 64 (bench), 32 (the continuous run's slots) and 16; GAR-8B at 64 and 16
           "attention": [bench_attention(64, 32, 8, 64, 4718), bench_attention(32, 32, 8, 64, 4718),
                         bench_attention(16, 32, 8, 64, 4718), bench_attention(64, 32, 8, 128, 4718),
                         bench_attention(16, 32, 8, 128, 4718)]}
    if not a.skip_e2e:
        res["e2e"] = bench_e2e(a.regions, a.new_tokens, a.long_tokens, a.slots)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
