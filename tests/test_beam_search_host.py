"""CPU: generate(beam_search=BeamSearch(...)) — the restatement tests/beam_search_ref.py against transformers (goldens recorded by
tools/capture_beam_goldens.py, and the live functions where transformers imports), BeamSearch's argument checks, and every refusal
that needs no device."""
import importlib.util
import inspect
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from beam_search_ref import beam_search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARLY = (False, True, "never")


@pytest.fixture(scope="module")
def goldens(golden_dir):
    z = np.load(os.path.join(golden_dir, "beam_search.npz"))
    table = {}
    for key, row in zip(z["logits_keys"], z["logits"]):
        table[(int(key[0]), tuple(int(x) for x in key[2:2 + key[1]]))] = torch.from_numpy(row)
    return z, table


def _table_logits(table, V):
    def fn(hist, t):
        B, K, _ = hist.shape
        out = torch.full((B, K, V), float("nan"))
        for b in range(B):
            for j in range(K):
                row = table.get((b, tuple(int(x) for x in hist[b, j])))
                if row is not None:         # a prompt that is done keeps a history HF never fed: its rows are not read
                    out[b, j] = row
        return out
    return fn


def test_restatement_reproduces_transformers_goldens(goldens):
    z, table = goldens
    V, max_new, pad = int(z["vocab"]), int(z["max_new_tokens"]), int(z["pad_token_id"])
    assert list(z["case_fields"]) == "K n_eos eos0 eos1 early lp n batch rows width".split()
    assert len(z["cases"]) == 2 * 2 * 3 * 3 * 2 * 2
    lengths = set()
    for case, want_seq, want_sc in zip(z["cases"], z["sequences"], z["sequences_scores"]):
        K, n_eos, eos0, eos1, early, lp, n, batch, rows, width = (int(x) for x in case)
        eos = [eos0] if n_eos == 1 else [eos0, eos1]
        seq, sc, st = beam_search_ref(_table_logits(table, V), batch, K, max_new, EARLY[early], float(lp), eos, V, n, pad)
        assert rows == batch * n
        assert seq.tolist() == want_seq[:rows, :width].astype(np.int64).tolist(), case
        assert torch.allclose(sc, torch.from_numpy(want_sc[:rows]), rtol=0, atol=1e-6), (case, sc, want_sc[:rows])
        assert st["tied_candidates"] == 0, case        # no result here rests on the order of equal scores
        lengths.update(int(x) for x in st["fin_len"].reshape(-1))
    assert min(lengths) <= 3 and max(lengths) == max_new       # eos is met early, and some hypotheses run to the end


def _tool():
    spec = importlib.util.spec_from_file_location("capture_beam_goldens", os.path.join(ROOT, "tools", "capture_beam_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_reproduces_live_transformers():
    pytest.importorskip("transformers")
    tool = _tool()
    model = tool.build_model()
    prompts = torch.tensor([[3, 8, 44], [17, 29, 6], [40, 1, 12]])

    def logits_fn(hist, t):
        B, K, _ = hist.shape
        ids = torch.cat((prompts[:B, None, :].expand(B, K, -1), hist.to(torch.int64)), 2).reshape(B * K, -1)
        with torch.no_grad():
            return model(input_ids=ids).logits[:, -1].float().reshape(B, K, -1)

    with torch.no_grad():
        free = model.generate(prompts, attention_mask=torch.ones_like(prompts), num_beams=4, do_sample=False, max_new_tokens=8,
                              pad_token_id=1, use_cache=False)[:, 3:]
    eos_sets = ([int(free[0, 2])], [int(free[1, 3]), int(free[2, 1])])
    for K, eos, early, lp, batch in ((2, eos_sets[0], False, 1.0, 3), (4, eos_sets[1], True, 0.0, 3), (4, eos_sets[0], "never", 2.0, 1),
                                     (3, eos_sets[1], False, 0.5, 2), (2, eos_sets[1], "never", -1.0, 3)):
        with torch.no_grad():
            o = model.generate(prompts[:batch], attention_mask=torch.ones_like(prompts[:batch]), num_beams=K, do_sample=False,
                               max_new_tokens=8, eos_token_id=eos, pad_token_id=1, early_stopping=early, length_penalty=lp,
                               num_return_sequences=K, return_dict_in_generate=True, output_scores=True, use_cache=False)
        seq, sc, st = beam_search_ref(logits_fn, batch, K, 8, early, lp, eos, tool.V, K, 1)
        assert seq.tolist() == o.sequences[:, 3:].tolist(), (K, eos, early, lp, batch)
        assert torch.allclose(sc, o.sequences_scores, rtol=0, atol=1e-6)
        assert st["tied_candidates"] == 0


def test_length_penalty_table_is_hfs_division():
    """gar_beam_step divides by len_pow[t] = float32(float(t + 1) ** length_penalty); HF divides an f32 tensor by the Python float
    (t + 1) ** length_penalty. The same bits, checked through HF's own _update_finished_beams and _check_early_stop_heuristic."""
    tf = pytest.importorskip("transformers")
    from gar_amd import BeamSearch
    G = tf.generation.utils.GenerationMixin
    g = G()
    torch.manual_seed(5)
    K, M, P = 4, 8, 3
    for lp in (0.0, 0.5, 1.0, 2.0, -1.0, 1.7):
        table = torch.tensor(BeamSearch(K, length_penalty=lp).length_powers(64), dtype=torch.float32)
        for t in (0, 1, 2, 6, 30, 63):
            x = -torch.rand(1, M) * 20 - 0.1
            x = x.sort(descending=True)[0]
            seqs = torch.zeros(1, K, 80, dtype=torch.int64)
            out = g._update_finished_beams(
                sequences=seqs, topk_running_sequences=torch.zeros(1, M, 80, dtype=torch.int64),
                beam_scores=torch.full((1, K), -1.0e9), topk_log_probs=x.clone(),
                beam_indices=torch.zeros(1, K, 80, dtype=torch.int32), topk_running_beam_indices=torch.zeros(1, M, 80, dtype=torch.int32),
                is_early_stop_heuristic_unsatisfied=torch.ones(1, 1, dtype=torch.bool), is_sent_finished=torch.zeros(1, K, dtype=torch.bool),
                next_token_hits_stopping_criteria=torch.ones(1, M, dtype=torch.bool),
                top_num_beam_mask=torch.arange(M) < K, num_beams=K, cur_len=P + t, decoder_prompt_len=P, length_penalty=lp,
                early_stopping=False)
            ours = (x[0, :K] / table[t]).sort(descending=True)[0]
            assert torch.equal(out[1][0], ours), (lp, t)
            # the heuristic's division, at the current length and ("never", positive penalty) at max_length
            run = x[:, :K].clone()
            fin = out[1]
            for early, want_len in ((False, t + 1), ("never", 64 if lp > 0 else t + 1)):
                h = G._check_early_stop_heuristic(torch.ones(1, 1, dtype=torch.bool), run, fin, torch.ones(1, K, dtype=torch.bool),
                                                  cur_len=P + t + 1, max_length=P + 64, decoder_prompt_len=P, early_stopping=early,
                                                  length_penalty=lp)
                assert bool(h) == bool(run[0, 0] / table[want_len - 1] > fin.min()), (lp, t, early)


def test_beam_search_argument_checks():
    from gar_amd import BeamSearch
    from gar_amd.beam_search import BeamBudgetError
    b = BeamSearch(4)
    assert (b.num_beams, b.length_penalty, b.early_stopping, b.num_return_sequences) == (4, 1.0, False, 1)
    assert BeamSearch.coerce(None) is None and BeamSearch.coerce(b) is b
    assert BeamSearch.coerce(dict(num_beams=2, early_stopping="never")) == BeamSearch(2, early_stopping="never")
    with pytest.raises(TypeError, match="beam_search"):
        BeamSearch.coerce(4)
    for bad in (1, 0, -2, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="num_beams"):
            BeamSearch(bad)
    for bad in ("always", 1, 0, None, "True"):
        with pytest.raises(ValueError, match="early_stopping"):
            BeamSearch(2, early_stopping=bad)
    for ok in (False, True, "never"):
        assert BeamSearch(2, early_stopping=ok).early_stopping is ok or ok == "never"
    for bad in (0, 5, -1, 1.0, True):
        with pytest.raises(ValueError, match="num_return_sequences"):
            BeamSearch(4, num_return_sequences=bad)
    assert BeamSearch(4, num_return_sequences=4).num_return_sequences == 4
    for bad in ("1", None, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="length_penalty"):
            BeamSearch(2, length_penalty=bad)
    # HF's beams_to_keep against gar_topk_lp's k = 32, known when the eos ids are
    assert BeamSearch(16).candidates(0) == 32 and BeamSearch(16).candidates(1) == 32 and BeamSearch(4).candidates(3) == 16
    assert BeamSearch(8).candidates(3) == 32 and BeamSearch(2).candidates(15) == 32
    for K, n_eos in ((17, 0), (16, 2), (8, 4), (2, 16), (11, 2)):
        with pytest.raises(BeamBudgetError, match="32"):
            BeamSearch(K).candidates(n_eos)
    assert BeamSearch(4, 2.0, "never").pack(8, [5, 9]) == [8, 2, 1, 2, 5, 9] + [-1] * 14
    assert BeamSearch(4, 0.0, True).pack(8, [])[:4] == [8, 1, 0, 0] and BeamSearch(4, -1.0).pack(3, [1])[:5] == [3, 0, 0, 1, 1]
    assert BeamSearch(2, 2.0).length_powers(3) == [1.0, 4.0, 9.0] and BeamSearch(2, 0.0).length_powers(2) == [1.0, 1.0]


class _Refusing:
    """a model stand-in for generate_begin's checks that come before any device work"""
    from gar_amd.configuration_gar import GARConfig
    config = GARConfig.tiny()
    kv_cache_dtype = None
    device = "cpu"


def test_refused_combinations_raise_by_name():
    from gar_amd import BeamSearch, LogitsProcessing, SamplingWarpers, hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel, GenerateOutput, GenerationPipeline
    for fn in (GARModel.generate_begin,):
        assert inspect.signature(fn).parameters["beam_search"].default is None
    assert GenerateOutput(sequences=None).sequences_scores is None
    begin = inspect.unwrap(GARModel.generate_begin)
    ids = torch.zeros(1, 4, dtype=torch.int64)
    BS = BeamSearch(4)
    for kw, name in ((dict(do_sample=True), "do_sample"), (dict(generation_config=dict(do_sample=True)), "do_sample"),
                     (dict(do_sample=True, sampling_warpers=SamplingWarpers(min_p=0.1)), "sampling_warpers"),
                     (dict(logits_processing=LogitsProcessing(repetition_penalty=1.2)), "logits_processing"),
                     (dict(logits_processing=dict(no_repeat_ngram_size=2)), "logits_processing"),
                     (dict(return_logprobs=True), "return_logprobs"), (dict(top_logprobs=2), "top_logprobs"),
                     (dict(candidate_token_ids=[1]), "candidate_token_ids"),
                     (dict(forced_tokens=torch.zeros(4, 2, dtype=torch.int64)), "forced_tokens")):
        for bs in (BS, dict(num_beams=4)):
            with pytest.raises(hip.GarError, match=name) as e:
                begin(_Refusing(), input_ids=ids, beam_search=bs, **kw)
            assert "beam_search" in str(e.value)
    fp8 = _Refusing()
    fp8.kv_cache_dtype = "fp8"
    with pytest.raises(hip.GarError, match="fp8"):
        begin(fp8, input_ids=ids, beam_search=BS)
    # the beam budget, known once the eos ids are: K * max(2, 1 + n_eos) <= 32
    for bs, eos in ((BeamSearch(16), [1, 2]), (BeamSearch(8), [1, 2, 3, 4]), (BeamSearch(17), None), (BeamSearch(11), [1, 2])):
        with pytest.raises(hip.GarError, match="32"):
            begin(_Refusing(), input_ids=ids, beam_search=bs, eos_token_id=eos, max_new_tokens=4)
    with pytest.raises(ValueError, match="num_beams"):
        begin(_Refusing(), input_ids=ids, beam_search=dict(num_beams=1))
    # the drivers that hold several requests in flight
    with pytest.raises(hip.GarError, match="beam_search"):
        GenerationPipeline(object(), beam_search=BS)
    with pytest.raises(hip.GarError, match="beam_search"):
        GARModel.generate_pipelined(object(), [dict(input_ids=ids)], beam_search=BS)
    with pytest.raises(hip.GarError, match="beam_search"):
        GenerationPipeline(object()).submit(dict(input_ids=ids, beam_search=BS))
    cb = ContinuousBatcher(types.SimpleNamespace(MAX_EOS_IDS=8, _check_decode_rows=lambda rows, what: None), 4, max_new_tokens=16)
    with pytest.raises(hip.GarError, match="beam_search"):
        cb.submit(dict(input_ids=ids), beam_search=BS)
    with pytest.raises(hip.GarError, match="beam_search"):
        cb.submit(dict(input_ids=ids, beam_search=dict(num_beams=2)))
    for kw in (dict(num_beams=2), dict(length_penalty=2.0)):
        with pytest.raises(hip.GarError, match=next(iter(kw))):
            cb.submit(dict(input_ids=ids), **kw)
    assert not cb.queue


def test_generation_config_spellings_stay_refused():
    """generate(num_beams=4) is refused as before; the message now points to the parameter that does it"""
    from gar_amd import hip
    from gar_amd.modeling_gar import GARModel, _GENERATION_KWARGS, _option_reader, _refuse_non_greedy
    assert "beam_search" not in _GENERATION_KWARGS
    for name, v in (("num_beams", 4), ("num_beams", 2), ("length_penalty", 2.0), ("length_penalty", 0.0)):
        for get in (_option_reader(None, {name: v}), _option_reader({name: v}, None)):
            with pytest.raises(hip.GarError, match=name) as e:
                _refuse_non_greedy(get)
            assert "beam_search=BeamSearch" in str(e.value)
    _refuse_non_greedy(_option_reader(None, dict(num_beams=1, length_penalty=1.0)))
    with pytest.raises(hip.GarError, match="num_beam_groups") as e:
        _refuse_non_greedy(_option_reader(None, dict(num_beam_groups=2)))
    assert "beam_search" not in str(e.value)
    begin = inspect.unwrap(GARModel.generate_begin)
    with pytest.raises(hip.GarError, match="num_beams"):
        begin(_Refusing(), input_ids=torch.zeros(1, 4, dtype=torch.int64), num_beams=4)
    with pytest.raises(hip.GarError, match="num_beams"):
        begin(_Refusing(), input_ids=torch.zeros(1, 4, dtype=torch.int64), generation_config=dict(num_beams=4, length_penalty=2.0))


def test_header_and_both_libraries_export_the_beam_kernels():
    from gar_amd import hip, ops
    hdr = open(os.path.join(ROOT, "include", "gar_hip.h")).read()
    assert "int gar_beam_step(const gar_beam_state* state, gar_stream_t stream);" in hdr and "#define GAR_ABI_VERSION 16" in hdr
    assert "int gar_kv_beam_reorder(void* Kc, void* Vc, int elem_size," in hdr
    assert hdr.index("EXTRAS") < hdr.index("gar_beam_step")
    from gar_amd.beam_search import MAX_EOS, PARAM_WORDS
    assert f"#define GAR_BEAM_MAX_EOS {MAX_EOS}" in hdr and PARAM_WORDS == ops.BEAM_PARAM_WORDS == 4 + MAX_EOS
    for path in (hip.LIB_PATH, hip.LIB_F16_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert " T gar_beam_step\n" in syms and " T gar_kv_beam_reorder\n" in syms, path
    assert [f for f, _ in hip.BeamState._fields_][-5:] == ["B", "K", "M", "T", "V"]
