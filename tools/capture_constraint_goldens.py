"""Records tests/golden/constraint.npz: what transformers' own ``generate(inputs_embeds=..., prefix_allowed_tokens_fn=...,
output_scores=True)`` does on a tiny random LlamaForCausalLM (built from a config, nothing is downloaded) under the callback
"the history remains a prefix of one of the prompt's phrases" (DESIGN 7.13): per case the raw next-token logits HF consumed at
every step, the scores PrefixConstrainedLogitsProcessor produced from them, and the sequences.

Cases: batch in {1, 3} x a shared set / one set per prompt x 1 / 2 eos ids, greedy search, max_new_tokens 6, vocabulary 37. The
sets hold a phrase that is a proper prefix of another, a one-token phrase, duplicates and a phrase longer than max_new_tokens.
Data only: ids, floats and the cases' settings.

    python tools/capture_constraint_goldens.py [out.npz]
"""
import itertools
import json
import os
import sys

import numpy as np
import torch

V, P, MAX_NEW, PAD, HIDDEN = 37, 4, 6, 0, 32
LONG = [3, 4, 8, 10, 11, 12, 13, 14]            # longer than MAX_NEW: a row that takes it is cut by max_new_tokens
SHARED = [[5, 6], [5, 6, 7], [9], [5, 6], LONG, [20, 21, 22], [20, 30]]
PER_PROMPT = [[[5, 6], [5, 6, 7], [9], [5, 6]], [LONG], [[20, 21, 22], [20, 30], [31], [20, 21]]]
EOS_SETS = ([2], [2, 33])


def build_model():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(4321)
    cfg = LlamaConfig(vocab_size=V, hidden_size=HIDDEN, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for p in model.parameters():            # the default init gives near-uniform distributions
            if p.dim() > 1:
                p.mul_(8.0)
    return model


def inputs_embeds():
    g = torch.Generator().manual_seed(99)
    return torch.randn(3, P, HIDDEN, generator=g)


def callback(sets, eos):
    """HF's prefix_allowed_tokens_fn for "the history remains a prefix of one of the prompt's phrases": the tokens that extend
    it, eos as well behind a complete phrase, eos alone when it is no prefix of any"""
    def fn(batch_id, ids):
        h = ids.tolist()
        ps = sets[batch_id]
        ok = {p[len(h)] for p in ps if len(p) > len(h) and p[:len(h)] == h}
        if h in ps:
            ok |= set(eos)
        return sorted(ok) if ok else sorted(eos)
    return fn


def hf_generate(model, emb, sets, eos):
    """(raw logits [T, B, V], scores [T, B, V], sequences [B, T], the histories the callback saw)"""
    raw, seen = [], []
    fn = callback(sets, eos)

    def spy(batch_id, ids):
        seen.append((batch_id, ids.tolist()))
        return fn(batch_id, ids)

    def hook(_m, _args, _kwargs, output):
        raw.append(output.logits[:, -1, :].detach().to(torch.float32).clone())
    h = model.register_forward_hook(hook, with_kwargs=True)
    try:
        with torch.no_grad():
            o = model.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.int64), do_sample=False,
                               max_new_tokens=MAX_NEW, eos_token_id=eos, pad_token_id=PAD, prefix_allowed_tokens_fn=spy,
                               return_dict_in_generate=True, output_scores=True)
    finally:
        h.remove()
    scores = torch.stack([s.to(torch.float32) for s in o.scores])
    return torch.stack(raw[:scores.shape[0]]), scores, o.sequences, seen


def cases():
    for batch, per_prompt, eos in itertools.product((1, 3), (False, True), EOS_SETS):
        sets = [PER_PROMPT[b] for b in range(batch)] if per_prompt else [SHARED] * batch
        yield dict(batch=batch, per_prompt=per_prompt, eos=list(eos), sets=sets)


def main(out):
    model, emb = build_model(), inputs_embeds()
    arrays, meta = {}, []
    for i, c in enumerate(cases()):
        raw, scores, seq, seen = hf_generate(model, emb[:c["batch"]], c["sets"], c["eos"])
        assert seen[0][1] == [] and max(len(h) for _, h in seen) == seq.shape[1] - 1      # the history is the generated tokens
        arrays[f"raw{i}"], arrays[f"scores{i}"] = raw.numpy(), scores.numpy()
        arrays[f"seq{i}"] = seq.numpy().astype(np.int16)
        meta.append(c)
        print(i, {k: c[k] for k in ("batch", "per_prompt", "eos")}, seq.tolist())
    arrays["meta"] = np.frombuffer(json.dumps(dict(cases=meta, vocab=V, max_new_tokens=MAX_NEW, pad_token_id=PAD)).encode(),
                                   dtype=np.uint8)
    np.savez_compressed(out, **arrays)
    print(f"{len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "tests", "golden", "constraint.npz"))
