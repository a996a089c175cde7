"""Records tests/golden/beam_search.npz: what transformers' own ``generate(num_beams=...)`` returns on a tiny random
LlamaForCausalLM (built from a config, nothing is downloaded), together with every next-token logits row it consumed, keyed by
(prompt, generated history) — the inputs tests/beam_search_ref.py needs to replay each search without transformers.

Cases: K in {2, 4} x 1 / 2 eos ids x early_stopping in {False, True, "never"} x length_penalty in {0, 1, 2} x
num_return_sequences in {1, K} x batch in {1, 3}, max_new_tokens 8, vocabulary 50. The logits depend on (prompt, history) only, so
one table serves every case. Data only: ids, floats and the cases' settings.

    python tools/capture_beam_goldens.py [out.npz]
"""
import itertools
import os
import sys

import numpy as np
import torch

V, P, MAX_NEW, PAD = 50, 3, 8, 1
EARLY = (False, True, "never")


def build_model():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(1234)
    cfg = LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for p in model.parameters():            # the default init gives near-uniform distributions: no beam would meet an eos
            if p.dim() > 1:
                p.mul_(8.0)
    return model


def main(out):
    model = build_model()
    prompts = torch.tensor([[7, 11, 13], [5, 23, 42], [31, 2, 19]])
    table = {}

    def hook(_m, args, kwargs, output):
        ids = kwargs.get("input_ids", args[0] if args else None)
        rows = hook.rows
        lg = output.logits[:, -1, :].detach().to(torch.float32)
        for r in range(ids.shape[0]):
            key = (rows[r], tuple(int(x) for x in ids[r, P:]))
            prev = table.get(key)
            assert prev is None or np.array_equal(prev, lg[r].numpy()), "one (prompt, history), two logits rows"
            table[key] = lg[r].numpy().copy()

    model.register_forward_hook(hook, with_kwargs=True)

    def run(batch, K, eos, early, lp, n):
        hook.rows = [b for b in range(batch) for _ in range(K)]
        with torch.no_grad():
            o = model.generate(prompts[:batch], attention_mask=torch.ones_like(prompts[:batch]), num_beams=K, do_sample=False,
                               max_new_tokens=MAX_NEW, eos_token_id=eos, pad_token_id=PAD, early_stopping=early,
                               length_penalty=float(lp), num_return_sequences=n, return_dict_in_generate=True, output_scores=True,
                               use_cache=False)
        return o.sequences[:, P:], o.sequences_scores

    # eos ids the beams do meet: tokens of the best eos-free hypotheses, a few steps in
    free, _ = run(3, 4, None, False, 1.0, 1)
    eos_sets = ([int(free[0, 3])], [int(free[1, 2]), int(free[2, 4])])
    cases, seqs, scores = [], [], []
    for K, eos, early, lp, all_n, batch in itertools.product((2, 4), eos_sets, range(3), (0.0, 1.0, 2.0), (0, 1), (1, 3)):
        n = K if all_n else 1
        s, sc = run(batch, K, eos, EARLY[early], lp, n)
        full = np.full((12, MAX_NEW), -1, dtype=np.int16)
        full[:s.shape[0], :s.shape[1]] = s.numpy()
        fsc = np.zeros(12, dtype=np.float32)
        fsc[:sc.shape[0]] = sc.numpy()
        cases.append([K, len(eos), eos[0], eos[-1], early, int(lp), n, batch, s.shape[0], s.shape[1]])
        seqs.append(full)
        scores.append(fsc)
    keys = sorted(table)
    hist = np.full((len(keys), 2 + MAX_NEW), -1, dtype=np.int16)
    for i, (b, h) in enumerate(keys):
        hist[i, 0], hist[i, 1] = b, len(h)
        hist[i, 2:2 + len(h)] = h
    np.savez_compressed(out, case_fields=np.array("K n_eos eos0 eos1 early lp n batch rows width".split()),
                        cases=np.array(cases, dtype=np.int32), sequences=np.stack(seqs), sequences_scores=np.stack(scores),
                        logits_keys=hist, logits=np.stack([table[k] for k in keys]).astype(np.float32),
                        vocab=np.int32(V), max_new_tokens=np.int32(MAX_NEW), pad_token_id=np.int32(PAD))
    lens = [int((q[:c[8]] != PAD).sum(1).min()) for q, c in zip(seqs, cases)]
    print(f"{len(cases)} cases, {len(keys)} logits rows, {os.path.getsize(out)} bytes; shortest hypothesis per case: "
          f"min {min(lens)} max {max(lens)}")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "tests", "golden", "beam_search.npz"))
