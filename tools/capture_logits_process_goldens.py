#!/usr/bin/env python
"""Writes tests/golden/logits_process.npz with transformers installed (run on the build machine, like tools/make_goldens.py):
what HF's own logits processors do, for tests/test_logits_process_host.py to hold tests/logits_process_ref.py against.

(a) transformers' processor classes applied to fixed logits [3, 1000] over histories of length 0, 1, 2 and 300 (the long one drawn
    from a 6-id alphabet that holds ids 0 and 999, so duplicates and repeated n-grams are certain; one logit is -inf), for every
    option set of A_OPTIONS. Stored sparsely: the (case, row, column, value) of every entry whose bytes changed.
(b) token sequences of LlamaForCausalLM.generate(inputs_embeds=...) — the reference's call, no input_ids — on the model rebuilt from
    tests/golden/llama_tiny.npz, for the option sets of b_options(). Asserted here: every sequence differs from plain greedy, and at
    every step HF's processed top-1 score leads top-2 by >= 1e-3 (two orders above the f32 agreement test_oracle_goldens.py demands
    of the oracle's logits, so a legitimate rounding difference cannot flip a token).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
V_A = 1000
ALPHABET = (0, 999, 1, 2, 3, 4)
MARGIN = 1e-3
B_TOKENS = 40


def a_inputs():
    g = torch.Generator().manual_seed(20)
    logits = torch.randn(3, V_A, generator=g) * 3.0
    logits[0, 2] = float("-inf")             # an id of the alphabet: the penalty meets -inf
    logits[1, 500] = float("-inf")
    logits[2, 1] = 0.0
    long = torch.tensor(ALPHABET)[torch.randint(0, len(ALPHABET), (3, 300), generator=g)]
    hist = {"h0": torch.zeros(3, 0, dtype=torch.int64), "h1": torch.tensor([[0], [999], [5]]),
            "h2": torch.tensor([[1, 2], [999, 0], [2, 2]]), "h300": long}
    return logits, hist


def a_options(hist):
    h = hist["h300"][0].tolist()
    bad = [[4], [1, 2, 52], [2, 53], [h[-2], h[-1], 50], [7, 8, 51], [h[-3], h[-2], h[-1], 54]]
    opts = [dict(repetition_penalty=1.3), dict(repetition_penalty=0.7)]
    opts += [dict(no_repeat_ngram_size=n) for n in (1, 2, 3, 4)]
    opts += [dict(min_new_tokens=2), dict(min_new_tokens=1), dict(suppress_tokens=[0, 999, 17]), dict(begin_suppress_tokens=[3, 999]),
             dict(bad_words_ids=bad),
             dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=2, suppress_tokens=[0, 999, 17],
                  begin_suppress_tokens=[3, 999], bad_words_ids=bad)]
    return opts


A_EOS = [5, 998]


def hf_processors(o, eos):
    """the request's processors in the order GenerationMixin._get_logits_processor builds them"""
    from transformers.generation import logits_process as LP
    procs = LP.LogitsProcessorList()
    if o.get("repetition_penalty", 1.0) != 1.0:
        procs.append(LP.RepetitionPenaltyLogitsProcessor(penalty=o["repetition_penalty"]))
    if o.get("no_repeat_ngram_size", 0) > 0:
        procs.append(LP.NoRepeatNGramLogitsProcessor(o["no_repeat_ngram_size"]))
    if o.get("bad_words_ids"):
        procs.append(LP.NoBadWordsLogitsProcessor(o["bad_words_ids"], eos or None))
    if o.get("min_new_tokens", 0) > 0 and eos:
        procs.append(LP.MinNewTokensLengthLogitsProcessor(0, o["min_new_tokens"], eos, device="cpu"))
    if o.get("suppress_tokens"):
        procs.append(LP.SuppressTokensLogitsProcessor(o["suppress_tokens"], device="cpu"))
    if o.get("begin_suppress_tokens"):
        procs.append(LP.SuppressTokensAtBeginLogitsProcessor(o["begin_suppress_tokens"], 0, device="cpu"))
    return procs


def hf_apply(o, eos, hist, logits):
    return hf_processors(o, eos)(hist.to(torch.int64), logits.clone())


def changed_entries(before, after):
    """(row, column) and value wherever the bytes of the two f32 tensors differ"""
    diff = (before.view(torch.int32) != after.view(torch.int32)).nonzero()
    return diff, after[diff[:, 0], diff[:, 1]]


def part_a():
    logits, hist = a_inputs()
    opts = a_options(hist)
    idx, val, cases = [], [], []
    for hname, h in hist.items():
        for oi, o in enumerate(opts):
            out = hf_apply(o, A_EOS, h, logits)
            d, v = changed_entries(logits, out)
            c = len(cases)
            cases.append([hname, oi])
            idx.append(torch.cat([torch.full((len(d), 1), c, dtype=torch.int64), d], 1))
            val.append(v)
    arrays = {"a_logits": logits.numpy(), "a_idx": torch.cat(idx).numpy().astype(np.int32), "a_val": torch.cat(val).numpy(),
              "a_eos": np.array(A_EOS, dtype=np.int64)}
    arrays.update({"a_" + k: v.numpy() for k, v in hist.items()})
    meta = {"a_options": opts, "a_cases": cases}
    print(f"(a): {len(cases)} cases, {len(arrays['a_val'])} changed entries")
    return arrays, meta


def tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    g = np.load(os.path.join(OUT, "llama_tiny.npz"))
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=64, vocab_size=512, rms_norm_eps=1e-5, rope_theta=500000.0,
                      rope_scaling={"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                    "original_max_position_embeddings": 8192, "rope_type": "llama3"},
                      max_position_embeddings=131072, tie_word_embeddings=True, attention_bias=False,
                      mlp_bias=False, attn_implementation="eager")
    m = LlamaForCausalLM(cfg).eval().to(torch.float32)
    sd = {"model." + k[2:][len("mllm.model.language_model."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("W:")}
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    m.load_state_dict(sd)
    return m, torch.from_numpy(g["inputs_embeds"])


def hf_generate(m, emb, o, eos, n=B_TOKENS):
    with torch.no_grad():
        gen = m.generate(inputs_embeds=emb, max_new_tokens=n, do_sample=False, use_cache=True, return_dict_in_generate=True,
                         output_scores=True, pad_token_id=0, eos_token_id=eos or None, **o)
    top2 = torch.stack([s[0].topk(2).values for s in gen.scores])
    return gen.sequences[0], float((top2[:, 0] - top2[:, 1]).min())


def b_options(plain):
    """the option sets of part (b), chosen from the plain greedy sequence so that each one acts"""
    p = plain.tolist()
    combo = dict(repetition_penalty=1.25, min_new_tokens=12, suppress_tokens=[p[1], p[2]], begin_suppress_tokens=[p[0]],
                 bad_words_ids=[[p[3]], [p[4], p[5]]])
    return [(dict(repetition_penalty=1.3), []), (dict(no_repeat_ngram_size=1), []), (combo, None)]


def part_b():
    m, emb = tiny_llama()
    plain, margin = hf_generate(m, emb, {}, [])
    print("(b) plain greedy:", plain.tolist(), "min margin", margin)
    arrays, meta = {"b_plain": plain.numpy()}, {"b_options": [], "b_eos": []}
    for i, (o, eos) in enumerate(b_options(plain)):
        if eos is None:
            # eos ids taken from what the option set generates without one: the token of step 6 would end the caption there, and
            # min_new_tokens = 12 has to hold it off
            free, _ = hf_generate(m, emb, o, [])
            eos = [int(free[6]), 511]
        seq, margin = hf_generate(m, emb, o, eos)
        print(f"(b) {o} eos {eos}:", seq.tolist(), "min margin", margin)
        assert seq.tolist() != plain.tolist()[:len(seq)], "the options leave plain greedy unchanged"
        assert margin >= MARGIN, f"top-1 leads top-2 by {margin} < {MARGIN}: choose other values or lengths"
        arrays[f"b_seq{i}"] = seq.numpy()
        meta["b_options"].append(o)
        meta["b_eos"].append(eos)
    return arrays, meta


def main():
    arrays, meta = part_a()
    b_arrays, b_meta = part_b()
    arrays.update(b_arrays)
    meta.update(b_meta)
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(OUT, "logits_process.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    sys.exit(main())
