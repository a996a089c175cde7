#!/usr/bin/env python
"""generate(beam_search=BeamSearch(...)). Writes profiles/beam_search.json:

  launches    us per launch of gar_beam_step and gar_kv_beam_reorder at GAR-1B geometry (16 layers, Hkv 8, hd 64, bf16 suffix caches
              of capacity 1024) for B prompts x K beams = 16x4, 8x8, 4x16 rows at t = 32, 256, 1023 cache rows. The reorder with
              every row moving (a cycle of parents) and with random parents, as achieved TB/s over the bytes it moves (each moved
              row read once and written once)
  generate    decode ms / token of GARModel.generate with beams against the sampled num_return_sequences fan-out at the same rows
              on the same commit, synthetic GAR-1B bf16, 1024^2 images, eos disabled

Every figure is the median of --reps repeats with their min and max; the forms of a comparison are timed in turns.
Usage: python tools/bench_beam.py [--skip-e2e] [--skip-launches] [--reps R] [--new-tokens T]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grasp-any-region_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import bench_fanout as BF  # noqa: E402
from gar_amd import BeamSearch, hip, ops  # noqa: E402

L, HKV, HD, CAP, V = 16, 8, 64, 1024, 128262


def bench_launches(B, K, reps):
    dev = "cuda:0"
    R, M = B * K, 2 * K
    g = torch.Generator(device=dev).manual_seed(B * 100 + K)
    Kc, Vc = (torch.randn(L, R, HKV, CAP, HD, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    beam = BeamSearch(K)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)
    lp = torch.log_softmax(torch.randn(R, 4 * M, device=dev, generator=g) * 3, -1).sort(-1, descending=True)[0][:, :M].contiguous()
    bs = dict(B=B, K=K, M=M, T=CAP, top_ids=torch.randint(0, V, (R, M), device=dev, generator=g, dtype=torch.int32), top_lp=lp,
              run_scores=z(R, dt=torch.float32), cur_tokens=z(R, dt=torch.int64), parent=z(R), hist=z(2, R, CAP), fin_tokens=z(R, CAP),
              fin_scores=torch.full((R,), -1.0e9, device=dev), fin_len=z(R), fin_flag=z(R),
              heur=torch.ones(B, dtype=torch.int32, device=dev), done=z(B), done_count=z(1),
              params=torch.tensor(beam.pack(CAP, []), dtype=torch.int32, device=dev),
              len_pow=torch.tensor(beam.length_powers(CAP), dtype=torch.float32, device=dev))
    cyc = ((torch.arange(K) + 1) % K).repeat(B).to(torch.int32).to(dev)
    rnd = torch.randint(0, K, (R,), generator=torch.Generator().manual_seed(K)).to(torch.int32).to(dev)
    moved = {"cycle": R, "random": int((rnd.cpu() != torch.arange(K).repeat(B)).sum())}
    rows = []
    for t in (32, 256, 1023):
        n_dev.fill_(t)

        def fills():        # every replay is a live step: the scores and the done latches of the previous one are cleared
            bs["run_scores"].zero_()
            bs["done"].zero_()

        def step():
            fills()
            ops.beam_step(bs, n_dev, V)
        launches = [BF._graph(step), BF._graph(fills),
                    BF._graph(lambda: ops.kv_beam_reorder(Kc, Vc, K, n_dev, cyc)),
                    BF._graph(lambda: ops.kv_beam_reorder(Kc, Vc, K, n_dev, rnd))]
        us = BF._alternate(launches, reps, [1, 1, 1, 1])
        row = {"B": B, "K": K, "M": M, "t": t, "beam_step_with_two_fills_us": us[0], "two_fills_us": us[1]}
        for name, u in (("cycle", us[2]), ("random", us[3])):
            nb = 2 * L * moved[name] * HKV * t * HD * 2 * 2         # both caches, read + write
            row[f"reorder_{name}"] = {"us": u, "rows_moved": moved[name], "bytes": nb, "TB/s": nb / u["median"] / 1e6}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_generate(new_tokens):
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    cfg = GARConfig.gar_1b()
    W = synthetic_weights(cfg)
    proc = GARProcessor.from_config(cfg, max_num_tiles=16)
    ss = BF._samples(cfg, proc, 16)
    m = GARModel(cfg, W, torch.bfloat16)
    out = {"model": "GAR-1B bf16 (synthetic weights)", "new_tokens": new_tokens, "shapes": []}
    for B, K in ((16, 4), (8, 8), (4, 16)):
        batch = BF._batch(ss[:B])
        legs = {"sampled_fanout": lambda n: dict(generation_config=dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9,
                                                                        max_new_tokens=n, num_return_sequences=K), seed=1),
                "beam_search": lambda n: dict(max_new_tokens=n, beam_search=BeamSearch(K, num_return_sequences=K))}
        for kw in legs.values():
            m.generate(**batch, **kw(new_tokens))
            m.generate(**batch, **kw(1))
        torch.cuda.synchronize()
        step = {name: [] for name in legs}
        for _ in range(BF.REPS):
            for name, kw in legs.items():
                t0 = time.perf_counter()
                m.generate(**batch, **kw(new_tokens))
                torch.cuda.synchronize()
                full = time.perf_counter() - t0
                t0 = time.perf_counter()
                m.generate(**batch, **kw(1))
                torch.cuda.synchronize()
                step[name].append((full - (time.perf_counter() - t0)) / (new_tokens - 1) * 1e3)
        row = {"B": B, "K": K, **{name: {"decode_ms_per_token": BF._stat(v)} for name, v in step.items()}}
        row["beam_over_fanout"] = row["beam_search"]["decode_ms_per_token"]["median"] / row["sampled_fanout"]["decode_ms_per_token"]["median"]
        print(json.dumps(row), flush=True)
        out["shapes"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_search.json"))
    a = ap.parse_args()
    hip.require_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_launches:
        res["launches"] = [r for B, K in ((16, 4), (8, 8), (4, 16)) for r in bench_launches(B, K, a.reps)]
    if not a.skip_e2e:
        res["generate"] = bench_generate(a.new_tokens)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
