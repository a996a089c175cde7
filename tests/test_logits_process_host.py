"""CPU: host side of generate(logits_processing=...) — the restatement tests/logits_process_ref.py against what
transformers' own processors did (tests/golden/logits_process.npz, written by tools/capture_logits_process_goldens.py) and, where
transformers is importable, against the live classes; LogitsProcessing's argument checks and packing; the refused combinations; the
GenerationConfig spellings that stay refused; the exported symbol."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logits_process_ref as R
from oracle import gar_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "logits_process.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def _golden_a_cases(golden):
    """(name, option dict, histories [3, t], expected processed logits [3, 1000]) of every case of part (a)"""
    g, meta = golden
    logits = torch.from_numpy(g["a_logits"])
    idx, val = torch.from_numpy(g["a_idx"]).long(), torch.from_numpy(g["a_val"])
    for c, (hname, oi) in enumerate(meta["a_cases"]):
        exp = logits.clone()
        sel = idx[:, 0] == c
        exp[idx[sel, 1], idx[sel, 2]] = val[sel]
        yield f"{hname}/{oi}", meta["a_options"][oi], torch.from_numpy(g["a_" + hname]), exp


def _same_bytes(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_golden_covers_what_the_kernel_can_get_wrong(golden):
    g, meta = golden
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "logits_process.npz")) < 100 * 1024
    assert [g["a_" + h].shape[1] for h in ("h0", "h1", "h2", "h300")] == [0, 1, 2, 300]
    long = g["a_h300"]
    assert all(len(set(r.tolist())) <= 6 for r in long) and {0, 999} <= set(long.reshape(-1).tolist())
    assert np.isneginf(g["a_logits"]).sum() >= 1
    ns = {o.get("no_repeat_ngram_size") for o in meta["a_options"]}
    assert {1, 2, 3, 4} <= ns
    assert {o.get("min_new_tokens") for o in meta["a_options"]} >= {1, 2}          # both sides of t = 1 and of t = 2
    # a multi-token bad word whose prefix is, and one whose prefix is not, at the end of the long history
    bad = next(o["bad_words_ids"] for o in meta["a_options"] if set(o) == {"bad_words_ids"})
    h = long[0].tolist()
    assert any(len(w) > 1 and h[-(len(w) - 1):] == w[:-1] for w in bad) and any(len(w) > 1 and h[-(len(w) - 1):] != w[:-1] for w in bad)


def test_restatement_equals_transformers_golden_exactly(golden):
    g, _ = golden
    logits, eos = torch.from_numpy(g["a_logits"]), g["a_eos"].tolist()
    n = 0
    for name, o, hist, exp in _golden_a_cases(golden):
        got = R.process(hist.tolist(), logits, 1000, o, eos)
        assert _same_bytes(got, exp), (name, o, (got != exp).nonzero().tolist()[:8])
        n += 1
    assert n == 48
    # duplicates do not compound: the 300-token history over 6 ids penalises 6 entries once
    row = R.process_row(g["a_h300"][1].tolist(), logits[1], 1000, dict(repetition_penalty=1.3))
    changed = (row != logits[1]).nonzero().reshape(-1).tolist()
    assert set(changed) <= {0, 999, 1, 2, 3, 4} and len(changed) >= 5
    x = logits[1, 3]
    assert float(row[3]) == float(torch.where(x < 0, x * torch.tensor(1.3), x / torch.tensor(1.3)))


def _generate_with_restatement(emb, W, t, n, o, eos):
    """the oracle's Llama + the restatement + first-index argmax: HF's generate(inputs_embeds=...) with these processors"""
    E, head = W[O.LM + "embed_tokens.weight"], O.lm_head_weight(W, t)
    cache = O.KVCache(t.num_hidden_layers)
    h = O.llama_forward(emb, W, t, cache)
    seq = []
    for _ in range(n):
        row = torch.nn.functional.linear(h[0, -1], head)
        tok = R.first_argmax(R.process_row(seq, row, t.vocab_size, o, eos))
        seq.append(tok)
        if tok in eos:
            break
        h = O.llama_forward(torch.nn.functional.embedding(torch.tensor([tok]), E).unsqueeze(1), W, t, cache)
    return seq


def _tiny_llama(golden_dir):
    from test_oracle_goldens import _tcfg
    g = np.load(os.path.join(golden_dir, "llama_tiny.npz"))
    W = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("W:")}
    return torch.from_numpy(g["inputs_embeds"]), W, _tcfg()


def test_oracle_loop_with_restatement_reproduces_transformers_generate(golden, golden_dir):
    g, meta = golden
    emb, W, t = _tiny_llama(golden_dir)
    plain = g["b_plain"].tolist()
    assert _generate_with_restatement(emb, W, t, len(plain), {}, []) == plain
    assert len(meta["b_options"]) == 3
    for i, (o, eos) in enumerate(zip(meta["b_options"], meta["b_eos"])):
        want = g[f"b_seq{i}"].tolist()
        assert want != plain[:len(want)], o                 # the options act
        assert _generate_with_restatement(emb, W, t, 40, o, eos) == want, o
    combo = meta["b_options"][2]
    assert {"min_new_tokens", "suppress_tokens", "begin_suppress_tokens", "bad_words_ids"} <= set(combo) and meta["b_eos"][2]


def test_restatement_against_live_transformers(golden, golden_dir):
    pytest.importorskip("transformers")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import capture_logits_process_goldens as C
    g, meta = golden
    logits, eos = torch.from_numpy(g["a_logits"]), g["a_eos"].tolist()
    for name, o, hist, _ in _golden_a_cases(golden):
        assert _same_bytes(C.hf_apply(o, eos, hist, logits), R.process(hist.tolist(), logits, 1000, o, eos)), name
    emb, W, t = _tiny_llama(golden_dir)
    m, emb2 = C.tiny_llama()
    assert torch.equal(emb, emb2)
    for o, eos in zip(meta["b_options"], meta["b_eos"]):
        seq, margin = C.hf_generate(m, emb, o, eos)
        assert margin >= C.MARGIN
        assert _generate_with_restatement(emb, W, t, 40, o, eos) == seq.tolist(), o


def test_logits_processing_argument_checks():
    from gar_amd import LogitsProcessing
    from gar_amd.logits_processing import BLOCK_WORDS, _Refused
    assert LogitsProcessing().neutral and LogitsProcessing.coerce(None).neutral and LogitsProcessing.coerce({}).neutral
    assert LogitsProcessing(repetition_penalty=1, no_repeat_ngram_size=0, suppress_tokens=[], bad_words_ids=None).neutral
    P = LogitsProcessing.coerce(dict(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=[[1, 2], [3]]))
    assert not P.neutral and P.bad_words_ids == ((1, 2), (3,)) and LogitsProcessing.coerce(P) is P
    with pytest.raises(Exception):                            # frozen
        P.repetition_penalty = 2.0
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty=2),
                dict(repetition_penalty="1.2"), dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True),
                dict(min_new_tokens=-1), dict(min_new_tokens=1.5), dict(bad_words_ids=[[]]), dict(bad_words_ids=[3]),
                dict(bad_words_ids=[[1, -2]]), dict(bad_words_ids=[[1.5]]), dict(suppress_tokens=[1.5])):
        with pytest.raises(ValueError):
            LogitsProcessing(**bad)
    with pytest.raises(TypeError, match="no_repeat"):
        LogitsProcessing.coerce(dict(no_repeat=3))
    with pytest.raises(TypeError):
        LogitsProcessing.coerce(1.2)
    # the device block: header, lists, offsets; HF drops a one-token bad word that equals an eos id
    w = LogitsProcessing(repetition_penalty=1.5, no_repeat_ngram_size=3, min_new_tokens=4, suppress_tokens=[7, 8],
                         begin_suppress_tokens=[9], bad_words_ids=[[5], [1, 2, 3], [6]]).pack(100, eos_ids=[5])
    assert w == [0x3FC00000, 3, 4, 2, 1, 2, 4, 0, 7, 8, 9, 0, 3, 4, 1, 2, 3, 6]
    assert LogitsProcessing(suppress_tokens=[3]).pack(10) == [0x3F800000, 0, 0, 1, 0, 0, 0, 0, 3]
    # ids outside the vocabulary and lists beyond the block: refused, never truncated
    for bad in (dict(suppress_tokens=[100]), dict(suppress_tokens=[-1]), dict(begin_suppress_tokens=[100]), dict(bad_words_ids=[[1, 100]])):
        with pytest.raises(_Refused, match="outside"):
            LogitsProcessing(**bad).pack(100)
    assert len(LogitsProcessing(suppress_tokens=list(range(BLOCK_WORDS - 8))).pack(10 ** 5)) == BLOCK_WORDS
    with pytest.raises(_Refused, match=str(BLOCK_WORDS)):
        LogitsProcessing(suppress_tokens=list(range(BLOCK_WORDS - 7))).pack(10 ** 5)


class _Refusing:
    """a model stand-in for generate_begin's checks that come before any device work"""
    from gar_amd.configuration_gar import GARConfig
    config = GARConfig.tiny()
    kv_cache_dtype = None
    device = "cpu"


def test_refused_combinations_raise_by_name():
    from gar_amd import LogitsProcessing, hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    assert inspect.signature(GARModel.generate_begin).parameters["logits_processing"].default is None
    begin = inspect.unwrap(GARModel.generate_begin)
    P = LogitsProcessing(repetition_penalty=1.2)
    ids = torch.zeros(1, 4, dtype=torch.int64)
    for kw, name in ((dict(forced_tokens=torch.zeros(1, 2, dtype=torch.int64)), "forced_tokens"), (dict(return_logprobs=True), "return_logprobs"),
                     (dict(top_logprobs=2), "top_logprobs"), (dict(candidate_token_ids=[1]), "candidate_token_ids")):
        with pytest.raises(hip.GarError, match=name):
            begin(_Refusing(), input_ids=ids, logits_processing=P, **kw)
        with pytest.raises(hip.GarError, match=name):
            begin(_Refusing(), input_ids=ids, logits_processing=dict(no_repeat_ngram_size=2), **kw)
    with pytest.raises(ValueError, match="penalty"):
        begin(_Refusing(), input_ids=ids, logits_processing=dict(repetition_penalty=0.0))
    with pytest.raises(hip.GarError, match="logits_processing"):
        ContinuousBatcher(object(), 4, logits_processing=P)
    src = inspect.getsource(ContinuousBatcher.submit)
    assert "logits_processing" in src and "GarError" in src


def test_generation_config_spellings_stay_refused():
    from gar_amd import hip
    from gar_amd.modeling_gar import _GENERATION_KWARGS, _option_reader, _refuse_non_greedy
    assert "logits_processing" not in _GENERATION_KWARGS      # a parameter of generate_begin's own, not a generation option
    for name, v in (("repetition_penalty", 1.2), ("no_repeat_ngram_size", 3), ("min_new_tokens", 4), ("min_length", 4),
                    ("suppress_tokens", [1]), ("begin_suppress_tokens", [1]), ("bad_words_ids", [[1]])):
        for get in (_option_reader(None, {name: v}), _option_reader({name: v}, None)):
            with pytest.raises(hip.GarError, match=name) as e:
                _refuse_non_greedy(get)
            assert "logits_processing" in str(e.value)        # the refusal points to the parameter that does it
    with pytest.raises(hip.GarError, match="num_beams") as e:
        _refuse_non_greedy(_option_reader(None, dict(num_beams=4)))
    assert "logits_processing" not in str(e.value)


def test_header_and_both_libraries_export_gar_logits_process():
    from gar_amd import hip, ops
    hdr = open(os.path.join(ROOT, "include", "gar_hip.h")).read()
    assert "int gar_logits_process(int dtype, void* logits," in hdr and "#define GAR_ABI_VERSION 16" in hdr
    assert "gar_logits_process" in hip.SIGNATURES
    for path in (hip.LIB_PATH, hip.LIB_F16_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert " T gar_logits_process\n" in syms, path
    assert hip.load_library().gar_logits_process_max_vocab() == hip.load_library(f16=True).gar_logits_process_max_vocab() >= 128256
    ps = list(inspect.signature(ops.logits_process).parameters)
    assert ps == ["logits", "V", "out_tokens", "step_dev", "eos_ids", "params"]
    assert "fast-math" not in open(os.path.join(ROOT, "grasp-any-region_amd", "csrc", "Makefile")).read()
