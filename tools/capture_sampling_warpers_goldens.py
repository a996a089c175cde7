#!/usr/bin/env python
"""Writes tests/golden/sampling_warpers.npz with transformers installed (run on the build machine, like
tools/capture_logits_process_goldens.py): what HF's own MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and
EtaLogitsWarper KEEP, for tests/test_sampling_warpers_host.py to hold tests/sampling_warpers_ref.py against.

Fixed logits [6, 1000] f32: four random rows, a row with tied maxima and a row with -inf entries. Cases: each warper alone at three
values, and chains in GenerationMixin._get_logits_processor's order behind temperature / top-k / top-p. Per case the kept set of
every row (score finite after the chain) as packed bits. Asserted here: no row of any case has an ambiguous token
(sampling_warpers_ref.warp_ext), so float32-vs-float64 rounding cannot decide a stored bit; and the restatement reproduces every
mask."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
V = 1000
KEYS = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def inputs():
    g = torch.Generator().manual_seed(79)
    x = torch.randn(6, V, generator=g) * 2.5
    x[3] *= 0.4                                              # a flatter row: the entropy-dependent branch of eta is the smaller one
    top = float(x[4].max()) + 0.75
    x[4, [17, 401, 998]] = top                               # tied maxima
    x[5, torch.randperm(V, generator=g)[:300]] = float("-inf")
    x[5, 0] = float("-inf")
    return x


def cases():
    c = []
    for v in (0.06, 0.3, 1.0):
        c.append(dict(min_p=v))
    for v in (0.18, 0.6, 0.89):
        c.append(dict(typical_p=v))
    for v in (3e-4, 5e-3, 0.9):
        c.append(dict(epsilon_cutoff=v))
    for v in (6e-4, 2e-3, 0.05):
        c.append(dict(eta_cutoff=v))
    c += [dict(temperature=0.8, top_k=50, top_p=0.95, min_p=0.02, typical_p=0.95, epsilon_cutoff=1e-3, eta_cutoff=2e-3),
          dict(temperature=1.2, top_p=0.8, typical_p=0.5, eta_cutoff=6e-4),
          dict(temperature=0.7, min_p=0.1, epsilon_cutoff=2e-3),
          dict(temperature=1.3, top_k=200, typical_p=0.3, epsilon_cutoff=4e-3, eta_cutoff=4e-3),
          dict(top_p=0.8, min_p=0.01, typical_p=0.65)]
    return c


def hf_chain(o):
    from transformers.generation import logits_process as LP
    procs = LP.LogitsProcessorList()
    if o.get("temperature", 1.0) != 1.0:
        procs.append(LP.TemperatureLogitsWarper(o["temperature"]))
    if o.get("top_k", 0) > 0:
        procs.append(LP.TopKLogitsWarper(top_k=o["top_k"], min_tokens_to_keep=1))
    if o.get("top_p", 1.0) < 1.0:
        procs.append(LP.TopPLogitsWarper(top_p=o["top_p"], min_tokens_to_keep=1))
    if o.get("min_p"):
        procs.append(LP.MinPLogitsWarper(min_p=o["min_p"], min_tokens_to_keep=1))
    if 0 < o.get("typical_p", 1.0) < 1.0:
        procs.append(LP.TypicalLogitsWarper(mass=o["typical_p"], min_tokens_to_keep=1))
    if 0 < o.get("epsilon_cutoff", 0.0) < 1.0:
        procs.append(LP.EpsilonLogitsWarper(epsilon=o["epsilon_cutoff"], min_tokens_to_keep=1))
    if 0 < o.get("eta_cutoff", 0.0) < 1.0:
        procs.append(LP.EtaLogitsWarper(epsilon=o["eta_cutoff"], min_tokens_to_keep=1, device="cpu"))
    return procs


def main():
    import sampling_warpers_ref as R
    x = inputs()
    defaults = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    masks, cs = [], cases()
    for o in cs:
        out = hf_chain(o)(torch.zeros(x.shape[0], 0, dtype=torch.int64), x.clone())
        kept = torch.isfinite(out).numpy()
        full = dict(defaults, **o)
        for b in range(x.shape[0]):
            _, keep, amb = R.warp_ext(x[b].numpy(), *[full[k] for k in KEYS])
            assert not amb.any(), f"case {o} row {b}: ambiguous ids {np.flatnonzero(amb).tolist()} — choose other values"
            assert np.array_equal(keep, kept[b]), (o, b, np.flatnonzero(keep != kept[b]).tolist())
        print(o, "kept per row:", kept.sum(1).tolist())
        masks.append(np.packbits(kept, axis=1))
    arrays = {"logits": x.numpy(), "masks": np.stack(masks),
              "meta": np.frombuffer(json.dumps({"cases": cs, "keys": KEYS}).encode(), dtype=np.uint8)}
    path = os.path.join(OUT, "sampling_warpers.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    sys.exit(main())
