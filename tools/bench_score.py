"""Caption scoring on one MI355X (GAR-1B, synthetic weights, bf16): writes profiles/score.json (or --out).

  head:     the fused lm_head + cross-entropy (gar_lm_head_xent + gar_xent_combine) against the same persistent 256 x 256
            tile GEMM storing bf16 logits + the dense log-sum-exp (gar_xent_combine's dense form), R = 4096 normed rows. The
            storing GEMM takes N % 8 == 0 only: lm_head is zero-padded to round_up(V, 256) rows for it (logits [R, Vpad], the
            log-sum-exp reads the first V columns), so both sides run on gemm_bf16_pp_kernel (checked: tile_gemm_takes)
  score:    GARModel.score of 64 regions x 64-token captions against the prompt phase of a 64-region generate (generate_begin)
            and against the same scores read off generate(forced_tokens=..., return_logits=True); score(validate=False), which
            runs the head over every row (the labelled-row count is not known without a host sync)
Every figure is the median of alternated repeats (HIP events around each measured call, one warm-up each)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "grasp-any-region_amd")]

from gar_amd import GARConfig, ops  # noqa: E402
from gar_amd.modeling_gar import GARModel  # noqa: E402


def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps):
    for f in fns.values():
        f()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(_ms(f))
    return {k: {"median_ms": statistics.median(v), "all_ms": [round(x, 4) for x in v]} for k, v in out.items()}


def bench_head(reps):
    cfg = GARConfig.gar_1b()
    t = cfg.mllm_config.text_config
    V, C, R = t.vocab_size, t.hidden_size, 4096
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    A = torch.randn(R, C, generator=g).to("cuda", dt)
    W = (torch.randn(V, C, generator=g) * C ** -0.5).to("cuda", dt)
    tg = torch.randint(0, V, (R,), generator=g, dtype=torch.int32).cuda()
    dest = torch.arange(R, dtype=torch.int32, device="cuda")
    out = torch.zeros(R, dtype=torch.float32, device="cuda")
    sm = torch.zeros(1, dtype=torch.float32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    part = torch.empty(R * ops.lm_head_xent_strips(V) * 2, dtype=torch.float32, device="cuda")
    tl = torch.empty(R, dtype=torch.float32, device="cuda")
    Vpad = (V + 255) // 256 * 256
    Wp = torch.zeros(Vpad, C, dtype=dt, device="cuda")
    Wp[:V] = W
    logits = torch.empty(R, Vpad, dtype=dt, device="cuda")
    assert ops.tile_gemm_takes(R, Vpad, C), "the storing baseline must run on the persistent tile GEMM"

    def fused():
        ops.lm_head_xent(A, W, tg, part, tl)
        ops.xent_combine(tg, dest, R, out, sm, n, V, partials=part, target_logit=tl)

    def unfused():
        ops.gemm(A, Wp, logits)
        ops.xent_combine(tg, dest, R, out, sm, n, V, logits=logits)

    def fused_gemm_only():
        ops.lm_head_xent(A, W, tg, part, tl)

    def unfused_gemm_only():
        ops.gemm(A, Wp, logits)

    def dense_lse_only():
        ops.xent_combine(tg, dest, R, out, sm, n, V, logits=logits)

    r = alternate({"fused": fused, "unfused": unfused, "fused_head_kernel": fused_gemm_only,
                   "unfused_tile_gemm": unfused_gemm_only, "dense_logsumexp": dense_lse_only}, reps)
    # agreement of the two on the same rows
    fused()
    a = out.clone()
    unfused()
    torch.cuda.synchronize()
    r["max_abs_logprob_diff"] = float((a - out).abs().max())
    r["shape"] = {"R": R, "V": V, "C": C, "Vpad": Vpad, "logits_bytes_avoided": R * Vpad * 2,
                  "partials_bytes": R * ops.lm_head_xent_strips(V) * 8}
    r["kernels"] = {"fused_head_kernel": "gemm_bf16_pp_kernel<PP_EPI_XENT> (lm_head [V, C])",
                    "unfused_tile_gemm": "gemm_bf16_pp_kernel<GAR_EPI_NONE> (lm_head zero-padded to [Vpad, C], logits [R, Vpad])",
                    "dense_logsumexp": "xent_combine_kernel dense form, one pass, 16-byte loads"}
    r["tflops_fused_kernel"] = 2.0 * R * V * C / (r["fused_head_kernel"]["median_ms"] * 1e-3) / 1e12
    return r


def bench_score(reps, B, n_cap):
    from gar_amd.eval_dataset import SingleRegionCaptionDataset
    from gar_amd.processing import GARProcessor, append_target
    from gar_amd.synthetic import synthetic_image, synthetic_mask
    cfg = GARConfig.gar_1b()
    model = GARModel.from_synthetic(cfg, dtype=torch.bfloat16)
    proc = GARProcessor.from_config(cfg)
    s = SingleRegionCaptionDataset(synthetic_image(0, 1024, 770), synthetic_mask(0, 1024, 770), proc,
                                   data_dtype=torch.bfloat16, device="cuda")[0]
    g = torch.Generator().manual_seed(1)
    cap = torch.randint(1000, 100000, (n_cap,), generator=g)
    d = append_target(s, cap)
    rep = lambda x: torch.cat([x] * B)
    pv, gm = rep(s["pixel_values"]), rep(s["global_mask_values"])
    ar = rep(torch.as_tensor(s["aspect_ratios"]).reshape(1, -1))
    bb = list(s["bboxes"]) * B
    ids_p = rep(s["input_ids"])
    ids_s, lab = rep(d["input_ids"]), rep(d["labels"])
    forced = rep(cap.reshape(1, -1)).cuda()

    def score():
        model.score(pv, gm, ar, bb, ids_s, lab)

    def prompt_phase():
        model.generate_begin(pixel_values=pv, global_mask_values=gm, aspect_ratios=ar, bboxes=bb, input_ids=ids_p,
                             max_new_tokens=n_cap)

    def via_generate():
        o = model.generate(pixel_values=pv, global_mask_values=gm, aspect_ratios=ar, bboxes=bb, input_ids=ids_p,
                           max_new_tokens=n_cap, forced_tokens=forced, return_logits=True)
        torch.log_softmax(o.logits, -1).gather(-1, forced[:, :, None])

    def score_no_validate():
        model.score(pv, gm, ar, bb, ids_s, lab, validate=False)

    r = alternate({"score": score, "generate_prompt_phase": prompt_phase, "generate_forced_return_logits": via_generate,
                   "score_validate_false": score_no_validate}, reps)
    r["score_over_prompt_phase"] = r["score"]["median_ms"] / r["generate_prompt_phase"]["median_ms"]
    r["validate_false_head_rows"] = B * (int(ids_s.shape[1]) - 1)
    r["validate_true_head_rows"] = B * n_cap
    r["shape"] = {"regions": B, "caption_tokens": n_cap, "prompt_tokens": int(s["input_ids"].shape[1])}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=64)
    ap.add_argument("--caption", type=int, default=64)
    a = ap.parse_args()
    t0 = time.time()
    res = {"device": torch.cuda.get_device_name(0), "head": bench_head(a.reps)}
    print(json.dumps(res["head"], indent=1), flush=True)
    res["score"] = bench_score(a.reps, a.regions, a.caption)
    print(json.dumps(res["score"], indent=1), flush=True)
    res["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
