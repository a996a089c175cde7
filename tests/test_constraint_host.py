"""CPU: host side of generate(constraint=PhraseConstraint(...)) — the restatement tests/constraint_ref.py against
what transformers' PrefixConstrainedLogitsProcessor did (tests/golden/constraint.npz, written by
tools/capture_constraint_goldens.py) and, where transformers is importable, against a live run; PhraseConstraint's argument
checks, its packed trie read back by an independent reader; the refused combinations; phrase_index; the exported symbol."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import constraint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "constraint.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cases(golden):
    g, meta = golden
    for i, c in enumerate(meta["cases"]):
        yield c, torch.from_numpy(g[f"raw{i}"]), torch.from_numpy(g[f"scores{i}"]), g[f"seq{i}"].astype(np.int64).tolist()


def test_golden_covers_the_cases_of_the_issue(golden):
    g, meta = golden
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "constraint.npz")) < 64 * 1024
    cases = meta["cases"]
    assert {(c["batch"], c["per_prompt"], len(c["eos"])) for c in cases} == {(b, p, e) for b in (1, 3) for p in (False, True) for e in (1, 2)}
    assert meta["vocab"] == 37
    T = meta["max_new_tokens"]
    for c in cases:         # every batch size and both layouts see each kind of phrase
        if c["per_prompt"] and c["batch"] == 1:
            continue            # prompt 0's own set alone: the long phrase belongs to prompt 1
        every = [tuple(p) for s in c["sets"] for p in s]
        assert any(len(p) == 1 for p in every) and any(len(p) > T for p in every) and len(set(every)) < len(every)
        assert any(a != b and b[:len(a)] == a for a in every for b in every)          # a proper prefix of another
    seqs = [row for _, _, _, seq in _cases(golden) for row in seq]
    # rows that end a phrase that is a prefix of another, rows that go on to the longer one, a one-token phrase, a cut row
    assert any(r[:3] in ([5, 6, 2], [5, 6, 33]) for r in seqs) and any(r[:3] == [5, 6, 7] for r in seqs)
    assert any(r[0] == 9 for r in seqs) and any(r == [3, 4, 8, 10, 11, 12] for r in seqs)
    assert any(r[-1] == meta["pad_token_id"] for r in seqs)                          # finished rows fed pad: the eos-only state


def test_restatement_equals_transformers_golden_exactly(golden):
    _, meta = golden
    V, pad, n = meta["vocab"], meta["pad_token_id"], 0
    for c, raw, scores, seq in _cases(golden):
        assert raw.shape == scores.shape == (len(seq[0]), c["batch"], V)
        done = [False] * c["batch"]
        for t in range(raw.shape[0]):
            hist = [row[:t] for row in seq]
            got = R.mask(c["sets"], hist, raw[t], V, c["eos"])
            assert _same_bytes(got, scores[t]), (c, t)
            for b in range(c["batch"]):     # HF's greedy loop: the argmax of the scores, pad behind a row's eos
                want = pad if done[b] else R.first_argmax(got[b])
                assert seq[b][t] == want, (c, t, b)
                done[b] = done[b] or want in c["eos"]
            n += 1
        # finite exactly at the allowed ids, whose values are the raw ones
        assert torch.equal(torch.isfinite(scores), scores == raw)
    assert n >= 30


def test_restatement_against_live_transformers(golden):
    pytest.importorskip("transformers")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import capture_constraint_goldens as C
    _, meta = golden
    model, emb = C.build_model(), C.inputs_embeds()
    for (c, raw, scores, seq), live in zip(_cases(golden), C.cases()):
        assert live == c
        raw2, scores2, seq2, seen = C.hf_generate(model, emb[:c["batch"]], c["sets"], c["eos"])
        assert seq2.tolist() == seq and seen[0][1] == []            # the callback's history: the generated tokens only
        for t in range(scores2.shape[0]):
            assert _same_bytes(R.mask(c["sets"], [r[:t] for r in seq], raw2[t], meta["vocab"], c["eos"]), scores2[t])


def test_pack_round_trips_through_an_independent_reader(golden):
    from gar_amd import PhraseConstraint
    from gar_amd.constrained import BLOCK_WORDS, HEADER_WORDS
    _, meta = golden
    for c in meta["cases"]:
        pc = PhraseConstraint(c["sets"] if c["per_prompt"] else c["sets"][0])
        assert pc.per_prompt == c["per_prompt"]
        for N in (1, 3):
            words = pc.pack(meta["vocab"], c["batch"], N)
            assert all(-2 ** 31 <= w < 2 ** 31 for w in words) and words[2] == c["batch"] * N and len(words) <= BLOCK_WORDS
            rows = R.unpack(words)
            assert rows == [{tuple(p) for p in c["sets"][b]} for b in range(c["batch"]) for _ in range(N)]
            roots = words[HEADER_WORDS:HEADER_WORDS + c["batch"] * N]
            assert all(roots[b * N + i] == roots[b * N] for b in range(c["batch"]) for i in range(N))
    # equal sets share one trie; the walk of the block follows the restatement
    shared = PhraseConstraint([[5, 6], [5, 6, 7], [9]])
    per = PhraseConstraint([[[5, 6], [5, 6, 7], [9]]] * 3)
    assert shared.pack(37, 3)[:2] == per.pack(37, 3)[:2] == [5, 4]
    w = shared.pack(37, 2)
    assert R.walk(w, 1, [5, 6], 37) >= 0 and R.walk(w, 1, [5, 7], 37) == R.DEAD and R.walk(w, 0, [9, 2], 37) == R.DEAD
    assert R.walk(w, 0, [40], 37) == R.DEAD
    # terminal bits beyond one word, negative as int32 when bit 31 is set
    many = PhraseConstraint([[i] for i in range(100)]).pack(200, 1)
    assert R.unpack(many) == [{(i,) for i in range(100)}]
    # coerce, as the siblings
    assert PhraseConstraint.coerce(None) is None and PhraseConstraint.coerce(shared) is shared
    assert PhraseConstraint.coerce(dict(phrases=[[1, 2]])).sets == (((1, 2),),)
    for bad in (dict(phrase=[[1]]), dict(phrases=[[1]], more=1), 3, [[1]]):
        with pytest.raises(TypeError):
            PhraseConstraint.coerce(bad)


class _Tok:
    """the call form of a tokenizer: one id per character, no special tokens unless asked"""
    def __call__(self, texts, add_special_tokens=True):
        return {"input_ids": [([1] if add_special_tokens else []) + [ord(ch) - 60 for ch in s] for s in texts]}


def test_from_text_encodes_without_special_tokens():
    from gar_amd import PhraseConstraint
    pc = PhraseConstraint.from_text(_Tok(), ["AB", "C"])
    assert not pc.per_prompt and pc.sets == (((5, 6), (7,)),) and pc.text_of(0, 1) == "C" and pc.text_of(0, -1) is None
    pp = PhraseConstraint.from_text(_Tok(), [["AB", "C"], ["D"]])
    assert pp.per_prompt and pp.sets == (((5, 6), (7,)), ((8,),)) and pp.text_of(1, 0) == "D"
    with pytest.raises(ValueError):
        PhraseConstraint.from_text(_Tok(), ["", "A"])


def test_pack_refuses_malformed_input():
    from gar_amd import PhraseConstraint
    from gar_amd.constrained import BLOCK_WORDS, _Refused
    for bad in ([], [[]], [[1], []], [[[1]], []], [[1.5]], [[True]], "ab", ["ab"], [[[1]], [[]]], 7):
        with pytest.raises(ValueError):
            PhraseConstraint(bad)
    for bad in ([[37]], [[1, -1]], [[[1]], [[2, 99]]]):
        with pytest.raises(_Refused, match="outside"):
            PhraseConstraint(bad).pack(37, 2)
    with pytest.raises(ValueError, match="3 per-prompt"):
        PhraseConstraint([[[1]], [[2]], [[3]]]).pack(37, 2)
    assert len(PhraseConstraint([[1]]).pack(37, 5)) == 4 + 5 + 3 + 2 + 1
    # capacity: refused, never truncated — 1200 names of 8 tokens fit, as the block was sized for
    names = [[1 + (i * 7 + j * 13) % 5000 for j in range(8)] + [i] for i in range(1200)]
    assert len(PhraseConstraint([n[:8] for n in names]).pack(128256, 64)) <= BLOCK_WORDS
    with pytest.raises(_Refused, match=str(BLOCK_WORDS)):
        PhraseConstraint([[i, i + 1, j] for i in range(200) for j in range(120)]).pack(10 ** 5, 1)
    # duplicates merge, the first index wins
    pc = PhraseConstraint([[5, 6], [9], [5, 6]])
    assert pc.phrase_index(0, [5, 6, 2], [2]) == 0 and pc.pack(37, 1)[:2] == [4, 3]


class _Refusing:
    """a model stand-in for generate_begin's checks that come before any device work"""
    from gar_amd.configuration_gar import GARConfig
    config = GARConfig.tiny()
    kv_cache_dtype = None
    device = "cpu"


def test_refused_combinations_raise_by_name_before_device_work():
    from gar_amd import BeamSearch, PhraseConstraint, hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel, GenerationPipeline
    assert inspect.signature(GARModel.generate_begin).parameters["constraint"].default is None
    begin = inspect.unwrap(GARModel.generate_begin)
    pc = PhraseConstraint([[1, 2], [3]])
    ids = torch.zeros(1, 4, dtype=torch.int64)
    for kw, name in ((dict(beam_search=BeamSearch(num_beams=2)), "beam_search"),
                     (dict(forced_tokens=torch.zeros(1, 2, dtype=torch.int64)), "forced_tokens"),
                     (dict(_row_words=[[0] * 8]), "ContinuousBatcher"), (dict(_row_proc=[[0] * 8]), "ContinuousBatcher")):
        for c in (pc, dict(phrases=[[1, 2]])):
            with pytest.raises(hip.GarError, match=name) as e:
                begin(_Refusing(), input_ids=ids, constraint=c, eos_token_id=2, **kw)
            assert "is not implemented (DESIGN 7.13)" in str(e.value)
    # an eos id on the device is part of the request
    for eos in (None, [], list(range(GARModel.MAX_EOS_IDS + 1))):
        with pytest.raises(hip.GarError, match="eos_token_id"):
            begin(_Refusing(), input_ids=ids, constraint=pc, eos_token_id=eos)
    with pytest.raises(ValueError, match="per-prompt"):
        begin(_Refusing(), input_ids=ids, constraint=PhraseConstraint([[[1]], [[2]]]), eos_token_id=2)
    with pytest.raises(ValueError, match="empty"):
        begin(_Refusing(), input_ids=ids, constraint=dict(phrases=[]), eos_token_id=2)
    with pytest.raises(hip.GarError, match=r"GenerationPipeline.*DESIGN 7\.13"):
        GenerationPipeline(object(), constraint=pc)
    p = GenerationPipeline(object())
    with pytest.raises(hip.GarError, match=r"GenerationPipeline.*DESIGN 7\.13"):
        p.submit(dict(input_ids=ids, constraint=pc))
    submit = ContinuousBatcher.submit
    for kw in (dict(sample=dict(input_ids=ids), constraint=pc), dict(sample=dict(input_ids=ids, constraint=pc))):
        with pytest.raises(hip.GarError, match=r"ContinuousBatcher\.submit is not implemented \(DESIGN 7\.13\)"):
            submit(object(), **kw)


def test_phrase_index_on_hand_made_sequences():
    from gar_amd import PhraseConstraint
    from gar_amd.modeling_gar import GenerateOutput, phrase_indices
    assert "phrase_index" in GenerateOutput.__dataclass_fields__
    pc = PhraseConstraint([[[5, 6], [5, 6, 7], [9], [5, 6]], [[3, 4, 8], [3, 4]]])
    eos = {2, 33}
    rows = [[5, 6, 2, 0],       # complete, a prefix of another: the first of the duplicates
            [5, 6, 7, 33],      # the longer one, the second eos id
            [5, 2, 0, 0],       # never completed
            [3, 4, 8, 2],       # prompt 1's own list
            [3, 4, 0, 0],       # no eos: all four tokens count, and they are no phrase
            [9, 0, 0, 0]]       # no phrase of prompt 1
    got = phrase_indices(pc, rows, eos, fanout=3)
    assert got.dtype == torch.int32 and got.tolist() == [0, 1, -1, 0, -1, -1]
    cut = PhraseConstraint([[3, 4, 8, 10], [3, 4], [3, 4, 8]])
    assert phrase_indices(cut, [[3, 4, 8], [3, 4], [3], [3, 4, 8, 10]], {2}).tolist() == [2, 1, -1, 0]      # cut rows: all their tokens
    for row in rows:
        assert pc.phrase_index(0, row, eos) == R.phrase_index(pc.set_of(0), row, eos)


def test_header_and_both_libraries_export_gar_constrain():
    from gar_amd import hip, ops
    from gar_amd import constrained
    hdr = open(os.path.join(ROOT, "include", "gar_hip.h")).read()
    assert "int gar_constrain(int dtype, void* logits," in hdr and "#define GAR_ABI_VERSION 16" in hdr
    assert "gar_constrain" in hip.SIGNATURES
    for path in (hip.LIB_PATH, hip.LIB_F16_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert " T gar_constrain\n" in syms, path
    assert ops.CONSTRAINT_WORDS == constrained.BLOCK_WORDS >= 65536 and ops.CONSTRAINT_HEADER == constrained.HEADER_WORDS
    assert ops.CONSTRAINT_DEAD == constrained.DEAD == R.DEAD
    assert list(inspect.signature(ops.constrain).parameters) == ["logits", "V", "out_tokens", "step_dev", "eos_ids", "trie", "nodes"]
    assert "constrain.hip" in open(os.path.join(ROOT, "grasp-any-region_amd", "csrc", "Makefile")).read()
