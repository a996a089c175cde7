"""The decode GEMVs with 16-bit against e4m3 weights (GARModel(decode_weight_dtype="fp8"), gar_gemm_w8), weights streamed cold.
Writes profiles/decode_weights_fp8.json.

    python tools/bench_decode_weights_fp8.py [--reps 5]

Every figure is the median of --reps repeats with its min and max. A GEMV round cycles through enough distinct weight matrices to
stream >= 1.5 GB, so that no shape stays resident in the 256 MB Infinity Cache (tools/bench_skinny.py's COLD=1; a decode step
streams every weight once), and is captured in a hipGraph and replayed, so that the figure is kernel time, not Python dispatch.
The end-to-end figures (GAR-1B decode step at B = 1 / 64, regions/s at B = 64, ms per region at batch 1) run GARModel.generate."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grasp-any-region_amd"))

from gar_amd import hip, ops  # noqa: E402

SHAPES = {"gar_1b": (2048, 8192, 3072), "gar_8b": (4096, 14336, 6144)}
VOCAB = 128262


def _stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def gemv_times(cfg, name, M, reps):
    C, F, Nq = SHAPES[cfg]
    N, K = {"qkv": (Nq, C), "o": (C, C), "gu": (2 * F, C), "down": (C, F), "lm_head": (VOCAB, C)}[name]
    L = max(16 if N < 100000 else 2, -(-int(1.5e9) // (N * K * 2)))
    ws = [(torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(L)]
    w8 = [ops.weight_quantize_fp8(w) for w in ws]
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    kw, epi = {}, hip.EPI_NONE
    if name in ("qkv", "gu"):
        kw = dict(norm_folded=True, norm_eps=1e-5)
    if name == "gu":
        epi = hip.EPI_SWIGLU
    if name in ("o", "down"):
        epi, kw = hip.EPI_RES, dict(residual=out)
    if name == "lm_head" and M <= 16:
        kw = dict(norm_w=torch.ones(K, dtype=torch.bfloat16, device="cuda"), norm_eps=1e-5)
    res = {}
    for kind in ("bf16", "fp8"):
        def run():          # the L-launch round, captured once and replayed: kernel time, not Python dispatch
            for i in range(L):
                if kind == "bf16":
                    ops.gemm(x, ws[i], out, epi, **kw)
                else:
                    ops.gemm(x, w8[i][0], out, epi, w_scale=w8[i][1], **kw)
        run()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(4):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / (4 * L))
        res[kind] = _stat(ts)
        del g
    del ws, w8
    torch.cuda.empty_cache()
    res["fp8_over_bf16"] = res["fp8"]["median"] / res["bf16"]["median"]
    res["weight_bytes_bf16"] = N * K * 2
    return res


def _regions(cfg, B, seed0=700):
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.processing import GARProcessor
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    proc = GARProcessor.from_config(cfg, max_num_tiles=16).use_gpu_preprocessing("cuda:0", torch.bfloat16)
    ss = [SingleRegionCaptionDataset(synthetic_image(seed0 + i), synthetic_mask(seed0 + i), proc, data_dtype=torch.bfloat16,
                                     device="cuda:0")[0] for i in range(B)]
    return dict(input_ids=torch.cat([x["input_ids"] for x in ss]), pixel_values=torch.cat([x["pixel_values"] for x in ss]),
                global_mask_values=torch.cat([x["global_mask_values"] for x in ss]), bboxes=[x["bboxes"][0] for x in ss],
                aspect_ratios=torch.cat([x["aspect_ratios"] for x in ss]))


def end_to_end(reps, n_tok=64):
    """GAR-1B, full depth, synthetic weights, eos never met: the decode step = (generate(n_tok) - generate(1)) / (n_tok - 1) at
    B = 1 and 64; generate regions/s at B = 64 and ms per region at B = 1, both with n_tok new tokens; bf16 vs fp8 weights"""
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    W = synthetic_weights(cfg)
    out = {}
    for kind in ("bf16", "fp8"):
        m = GARModel(cfg, W, torch.bfloat16, "cuda:0", decode_weight_dtype="fp8" if kind == "fp8" else None)
        if kind == "fp8":
            out["decode_weight_fp8_bytes_gar1b"] = m.decode_weight_fp8_bytes()
        for B in (1, 64):
            batch = _regions(cfg, B)

            def gen(n):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m.generate(**batch, max_new_tokens=n, eos_token_id=None, validate=False)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)
            gen(n_tok)
            gen(1)
            step, full = [], []
            for _ in range(reps):
                t1, tn = gen(1), gen(n_tok)
                step.append((tn - t1) / (n_tok - 1))
                full.append(tn)
            out[f"decode_step_ms/B{B}/{kind}"] = _stat(step)
            if B == 1:
                out[f"ms_per_region_b1_{n_tok}tok/{kind}"] = _stat(full)
            else:
                out[f"regions_per_s_b64_{n_tok}tok/{kind}"] = _stat([B * 1e3 / t for t in full])
            print(f"GAR-1B {kind} B={B}: decode step {statistics.median(step):.3f} ms, generate({n_tok}) "
                  f"{statistics.median(full):.1f} ms", flush=True)
        del m
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_weights_fp8.json"))
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    hip.require_device(0)
    rep = {"reps": args.reps, "unit_gemv": "us", "gemv": {}}
    for cfg in SHAPES:
        for name in ("qkv", "o", "gu", "down", "lm_head"):
            for M in (1, 8, 16, 64):
                r = gemv_times(cfg, name, M, args.reps)
                rep["gemv"][f"{cfg}/{name}/M{M}"] = r
                print(f"{cfg} {name:7s} M={M:2d}: bf16 {r['bf16']['median']:8.2f} us  fp8 {r['fp8']['median']:8.2f} us  "
                      f"ratio {r['fp8_over_bf16']:.3f}", flush=True)
    ratios = [r["fp8_over_bf16"] for r in rep["gemv"].values()]
    rep["gate_max_fp8_over_bf16"] = max(ratios)
    rep["goal_max_fp8_over_bf16_m_le_8"] = max(r["fp8_over_bf16"] for k, r in rep["gemv"].items() if k.endswith(("/M1", "/M8")))
    if not args.skip_e2e:
        rep["end_to_end"] = end_to_end(args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
    print("gate (max fp8/bf16 over all GEMVs and M):", round(rep["gate_max_fp8_over_bf16"], 3),
          "| goal (max at M <= 8):", round(rep["goal_max_fp8_over_bf16_m_le_8"], 3))


if __name__ == "__main__":
    main()
