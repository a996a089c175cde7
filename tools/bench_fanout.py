#!/usr/bin/env python
"""generate(num_return_sequences = N) against the same rows as a replicated batch. Writes profiles/fanout.json:

  attention   us per launch of gar_attention_decode_fanout (B prompts x N siblings, shared prompt cache + per-row suffix) against
              gar_attention_decode_qkv on R = B * N replicated full caches, R = 64 as 64x1, 32x2, 16x4, 8x8, 4x16, P = 4718, t = 32,
              GAR-1B (Hq 32, Hkv 8, hd 64) and GAR-8B (hd 128) head shapes; hipGraph replays over enough distinct caches that
              the bytes come from HBM; algorithmic bytes B*Hkv*P*hd*2*2 + R*Hkv*t*hd*2*2 (fan-out) / R*Hkv*(P+t)*hd*2*2
  generate    captions/s, decode ms / token and peak KV bytes of GARModel.generate, synthetic GAR-1B bf16, 1024^2 images, eos
              disabled: 16 regions x N = 4 and 8 regions x N = 8 through num_return_sequences against the same 64 rows as a
              replicated batch (--replicated-only: that leg alone — it uses no new API)

The two forms are timed alternately; every figure is the median of --reps repeats with their min and max.
Usage: python tools/bench_fanout.py [--skip-e2e] [--replicated-only] [--reps R] [--new-tokens T]"""
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


def _graph(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def _alternate(launches, reps, per):
    """us per launch of each callable, timed in turns: REPS rounds of `reps` replays (of per[i] launches) each"""
    out = [[] for _ in launches]
    for _ in range(REPS):
        for i, launch in enumerate(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1) / reps / per[i] * 1e3)
    return [_stat(x) for x in out]


def _row(us, nb):
    return {"us": us, "bytes": nb, "TB/s": nb / us["median"] / 1e6, "hbm_frac": nb / us["median"] / 1e3 / PEAK_HBM_GBS}


def bench_attention(B, N, Hq, Hkv, hd, P=4718, t=32, reps=10):
    dev, dt = "cuda:0", torch.bfloat16
    R, G = B * N, Hq // Hkv
    Sp, T = (P + 255) // 256 * 256, 64
    Smax = Sp + T
    fan_bytes = B * Hkv * P * hd * 2 * 2 + R * Hkv * t * hd * 2 * 2
    rep_bytes = R * Hkv * (P + t) * hd * 2 * 2
    L = max(4, -(-(1 << 30) // fan_bytes))          # distinct caches: >= 1 GiB streamed per replay, beyond the 256 MiB last-level cache
    x = torch.randn(R, (Hq + 2 * Hkv) * hd, device=dev).to(dt)
    O = torch.empty(R, Hq * hd, device=dev, dtype=dt)
    fr = torch.arange(Smax, dtype=torch.float32, device=dev)[:, None] / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    cos, sin = fr.cos().contiguous(), fr.sin().contiguous()
    qs = hd ** -0.5 * 1.4426950408889634
    cnt = torch.tensor([t, P + t, 0, P], dtype=torch.int32, device=dev)
    ns_rep = max(1, min(8, 192 // (R * Hkv)))        # GARModel.DECODE_ATTN_* at these shapes
    ns_fan = max(1, min(8, 192 // (B * Hkv * -(-N // max(1, 32 // G)))))
    ws = torch.empty(ops.attention_decode_workspace(R, Hq, hd, ns_rep), dtype=torch.uint8, device=dev)
    wsf = torch.empty(ops.attention_decode_fanout_workspace(R, Hq, hd, ns_fan), dtype=torch.uint8, device=dev)
    mk = lambda *s: torch.randn(*s, device=dev).to(dt)
    Lr = max(4, -(-(1 << 30) // rep_bytes))
    Kf, Vf = [mk(R, Hkv, Smax, hd) for _ in range(Lr)], [mk(R, Hkv, Smax, hd) for _ in range(Lr)]
    run_rep = _graph(lambda: [ops.attention_decode_qkv(x, cos, sin, Kf[i], Vf[i], O, R, Hq, Hkv, hd, Smax, cnt[1:2], qs, ns_rep, ws)
                              for i in range(Lr)])
    Kp, Vp = [mk(B, Hkv, Sp, hd) for _ in range(L)], [mk(B, Hkv, Sp, hd) for _ in range(L)]
    Ks, Vs = [mk(R, Hkv, T, hd) for _ in range(L)], [mk(R, Hkv, T, hd) for _ in range(L)]
    run_fan = _graph(lambda: [ops.attention_decode_fanout(x, cos, sin, Kp[i], Vp[i], Ks[i], Vs[i], O, B, N, Hq, Hkv, hd, Sp, T,
                                                          cnt[3:4], cnt[0:1], qs, ns_fan, wsf) for i in range(L)])
    us_rep, us_fan = _alternate([run_rep, run_fan], reps, [Lr, L])      # (the graphs differ in launches per replay)
    res = {"B": B, "N": N, "R": R, "Hq": Hq, "Hkv": Hkv, "hd": hd, "P": P, "t": t, "nsplit_replicated": ns_rep, "nsplit_fanout": ns_fan,
           "replicated": _row(us_rep, rep_bytes), "fanout": _row(us_fan, fan_bytes),
           "fanout_speedup": us_rep["median"] / us_fan["median"]}
    print(json.dumps(res), flush=True)
    return res


def _samples(cfg, proc, n):
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    return [SingleRegionCaptionDataset(synthetic_image(i, 1024, 1024), synthetic_mask(i, 1024, 1024), proc,
                                       data_dtype=torch.bfloat16, device="cpu")[0] for i in range(n)]


def _batch(ss):
    return dict(input_ids=torch.cat([s["input_ids"] for s in ss]), pixel_values=torch.cat([s["pixel_values"] for s in ss]),
                global_mask_values=torch.cat([s["global_mask_values"] for s in ss]), bboxes=[b for s in ss for b in s["bboxes"]],
                aspect_ratios=torch.cat([s["aspect_ratios"] for s in ss]))


def _kv_bytes(m):
    return sum(t.numel() * t.element_size() for k, d in m._ws.items() if k[0] == "llm" for n, t in d.items() if n in ("Kc", "Vc"))


def bench_generate(new_tokens, replicated_only):
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    ss = _samples(cfg, proc, 16)
    V = cfg.mllm_config.text_config.vocab_size
    out = {"model": "GAR-1B bf16 (synthetic weights)", "new_tokens": new_tokens, "shapes": []}
    for B, N in ((16, 4), (8, 8)):
        legs = {"replicated": (_batch([s for s in ss[:B] for _ in range(N)]), 1)}
        if not replicated_only:
            legs["fanout"] = (_batch(ss[:B]), N)
        models = {name: GARModel(cfg, W, torch.bfloat16) for name in legs}          # a model per leg: peak KV bytes apart
        gc = lambda n, N_: dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, max_new_tokens=n, num_return_sequences=N_)
        for name, (batch, N_) in legs.items():                                      # warm-up: graphs, workspaces
            models[name].generate(**batch, generation_config=gc(new_tokens, N_), seed=1)
            models[name].generate(**batch, generation_config=gc(1, N_), seed=1)
        torch.cuda.synchronize()
        cps = {name: [] for name in legs}
        step = {name: [] for name in legs}
        for _ in range(REPS):
            for name, (batch, N_) in legs.items():                                  # in turns
                t0 = time.perf_counter()
                r = models[name].generate(**batch, generation_config=gc(new_tokens, N_), seed=1)
                torch.cuda.synchronize()
                full = time.perf_counter() - t0
                assert tuple(r.sequences.shape) == (B * N, new_tokens)
                t0 = time.perf_counter()
                models[name].generate(**batch, generation_config=gc(1, N_), seed=1)
                torch.cuda.synchronize()
                prompt = time.perf_counter() - t0
                cps[name].append(B * N / full)
                step[name].append((full - prompt) / (new_tokens - 1) * 1e3)
        row = {"B": B, "N": N}
        for name in legs:
            row[name] = {"captions_per_s": _stat(cps[name]), "decode_ms_per_token": _stat(step[name]),
                         "kv_cache_bytes": _kv_bytes(models[name])}
        if "fanout" in row:
            row["fanout_speedup"] = row["fanout"]["captions_per_s"]["median"] / row["replicated"]["captions_per_s"]["median"]
        print(json.dumps(row), flush=True)
        out["shapes"].append(row)
        del models
        torch.cuda.empty_cache()
    return out


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-attention", action="store_true")
    ap.add_argument("--replicated-only", action="store_true", help="generate: the replicated leg alone (no new API)")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fanout.json"))
    a = ap.parse_args()
    REPS = a.reps
    hip.require_device(0)
    res = {"device": torch.cuda.get_device_name(0), "peak_hbm_GBs": PEAK_HBM_GBS}
    if not (a.skip_attention or a.replicated_only):
        res["attention"] = [bench_attention(B, N, 32, 8, hd) for hd in (64, 128) for B, N in ((64, 1), (32, 2), (16, 4), (8, 8), (4, 16))]
    if not a.skip_e2e:
        res["generate"] = bench_generate(a.new_tokens, a.replicated_only)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
