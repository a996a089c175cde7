"""CPU: the label semantics of GARModel.forward(mode="loss") / score() — HF's causal-LM loss as restated in
gar_amd.modeling_gar.causal_lm_loss against transformers, the replayed-span masking of the reference (modeling_gar.py:176-190),
padding, append_target, and the argument errors that need no device."""
import os

import numpy as np
import pytest
import torch

from gar_amd import GARConfig
from gar_amd.modeling_gar import GARModel, causal_lm_loss, score_targets
from gar_amd.processing import append_target


def test_restated_loss_equals_transformers(golden_dir):
    transformers = pytest.importorskip("transformers")
    g = np.load(os.path.join(golden_dir, "llama_tiny.npz"))
    W = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("W:")}
    lm = "mllm.model.language_model."
    E = W[lm + "embed_tokens.weight"]
    V, C = E.shape
    t = W[lm + "layers.0.self_attn.k_proj.weight"].shape[0]
    cfg = transformers.LlamaConfig(vocab_size=V, hidden_size=C, intermediate_size=W[lm + "layers.0.mlp.gate_proj.weight"].shape[0],
                                   num_hidden_layers=2, num_attention_heads=W[lm + "layers.0.self_attn.q_proj.weight"].shape[0] // 32,
                                   num_key_value_heads=t // 32, head_dim=32, rms_norm_eps=1e-5, tie_word_embeddings=True,
                                   attn_implementation="eager")
    model = transformers.LlamaForCausalLM(cfg).eval()
    sd = {k[len("mllm.model.language_model."):]: v for k, v in W.items()}
    missing = model.model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys
    model.tie_weights()
    emb = torch.from_numpy(g["inputs_embeds"])
    S = emb.shape[1]
    gen = torch.Generator().manual_seed(0)
    for case in range(3):
        labels = torch.randint(0, V, (1, S), generator=gen)
        if case == 1:
            labels[0, :S // 2] = -100
        if case == 2:
            labels[0, ::3] = -100
        with torch.no_grad():
            out = model(inputs_embeds=emb, labels=labels)
        ours = causal_lm_loss(out.logits, labels)
        assert abs(float(ours) - float(out.loss)) <= 1e-6 * abs(float(out.loss)), (case, float(ours), float(out.loss))
    assert torch.isnan(causal_lm_loss(out.logits, torch.full((1, S), -100)))


def test_replay_span_and_padding_masking():
    crop = [900, 901]
    ids = torch.tensor([[5, 6, 900, 900, 900, 7, 901, 901, 8, 9],
                        [0, 0, 5, 901, 901, 901, 6, 7, 8, 9]])
    labels = ids.clone()                       # every position labelled, spans included
    am = torch.tensor([[1] * 10, [0, 0] + [1] * 8])
    tgt = score_targets(ids, labels, crop, am)
    assert tgt.shape == (2, 9)
    # row 0: span 900 at 2..4 and 901 at 6..7 -> labels -100 there; row t predicts label t + 1
    exp0 = [6, -100, -100, -100, 7, -100, -100, 8, 9]
    # row 1: padding rows 0..1 predict nothing (so the first real token is not scored); span 901 at 3..5
    exp1 = [-100, -100, -100, -100, -100, 6, 7, 8, 9]
    assert tgt.tolist() == [exp0, exp1]
    # a crop token that is absent masks nothing; labels not -100 inside a span are masked too
    assert score_targets(ids[:1], labels[:1], [902]).tolist() == [labels[0, 1:].tolist()]


def test_append_target():
    s = {"input_ids": torch.tensor([[3, 4, 5]]), "attention_mask": torch.ones(1, 3, dtype=torch.bfloat16), "bboxes": [{}]}
    d = append_target(s, [7, 8], eos_token_id=9)
    assert d["input_ids"].tolist() == [[3, 4, 5, 7, 8, 9]]
    assert d["labels"].tolist() == [[-100, -100, -100, 7, 8, 9]]
    assert d["attention_mask"].dtype == torch.bfloat16 and d["attention_mask"].tolist() == [[1] * 6]
    assert d["bboxes"] is s["bboxes"] and s["input_ids"].shape == (1, 3)
    d2 = append_target({"input_ids": torch.tensor([[1]])}, torch.tensor([2]))
    assert d2["labels"].tolist() == [[-100, 2]] and "attention_mask" not in d2


def test_forward_mode_and_argument_errors():
    from gar_amd.hip import GarError
    m = object.__new__(GARModel)               # no device needed: the checks run before any launch
    with pytest.raises(GarError, match="predict"):
        m.forward({}, mode="predict")
    with pytest.raises(GarError, match="tensor"):
        m.forward({}, mode="tensor")
    m.config = GARConfig.tiny()
    m.device = torch.device("cpu")
    ids = torch.zeros(1, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="shape"):
        GARModel.score.__wrapped__(m, None, None, None, None, ids, torch.zeros(1, 4, dtype=torch.int64))
    V = m.config.mllm_config.text_config.vocab_size
    for bad in (V, -1, -99):
        lab = torch.full((1, 5), -100)
        lab[0, 3] = bad
        with pytest.raises(ValueError, match="labels must be in"):
            GARModel.score.__wrapped__(m, None, None, None, None, ids, lab)
