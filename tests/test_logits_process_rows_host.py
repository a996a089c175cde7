"""CPU: the host side of per-request logits processing in ContinuousBatcher — a row's parameter block
(continuous.pack_process_row), the declaration / export / binding of gar_logits_process_rows, and what submit() accepts, records and
refuses before any device work."""
import inspect
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 1000


def _everything():
    from gar_amd import LogitsProcessing
    return LogitsProcessing(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=4, suppress_tokens=[7, 8],
                            begin_suppress_tokens=[9], bad_words_ids=[[11], [12, 13, 14], [5]])


def test_pack_process_row_is_pack_with_col0_in_word_7():
    from gar_amd import LogitsProcessing
    from gar_amd.continuous import pack_process_row
    from gar_amd.logits_processing import HEADER_WORDS
    for proc, eos in ((_everything(), [5, 6]), (LogitsProcessing(repetition_penalty=0.5), []),
                      (LogitsProcessing(suppress_tokens=[1]), [2])):
        base = proc.pack(V, eos)
        assert base[7] == 0 and base[0] != 0                 # word 0: the f32 bits of a penalty > 0, never 0
        for col0 in (0, 17, 2 ** 31 - 1, -3):
            w = pack_process_row(proc, V, eos, col0)
            assert w[7] == col0 and w[:7] == base[:7] and w[8:] == base[8:] and len(w) == len(base)
            assert all(isinstance(x, int) and -2 ** 31 <= x < 2 ** 31 for x in w)
        assert proc.pack(V, eos) == base                     # pack()'s own words are not touched
    # a one-token bad word equal to an eos id is dropped, as pack() drops it
    assert pack_process_row(_everything(), V, [5, 6], 3)[5] == 2 and pack_process_row(_everything(), V, [], 3)[5] == 3
    # no request: the all-zero header, whatever col0
    assert HEADER_WORDS == 8
    assert pack_process_row(None, V, [5], 0) == [0] * 8 and pack_process_row(None, V, [5], 23) == [0] * 8


def test_pack_process_row_refusals():
    from gar_amd import LogitsProcessing
    from gar_amd.continuous import pack_process_row
    from gar_amd.logits_processing import BLOCK_WORDS, _Refused
    for col0 in (2 ** 31, -2 ** 31 - 1):
        with pytest.raises(ValueError, match="col0"):
            pack_process_row(_everything(), V, [], col0)
        with pytest.raises(ValueError, match="col0"):
            pack_process_row(None, V, [], col0)
    with pytest.raises(_Refused, match="outside"):
        pack_process_row(LogitsProcessing(suppress_tokens=[V]), V, [], 0)
    with pytest.raises(_Refused, match=str(BLOCK_WORDS)):
        pack_process_row(LogitsProcessing(suppress_tokens=list(range(BLOCK_WORDS - 7))), 10 ** 5, [], 0)
    assert len(pack_process_row(LogitsProcessing(suppress_tokens=list(range(BLOCK_WORDS - 8))), 10 ** 5, [], 9)) == BLOCK_WORDS


def test_header_declares_and_libraries_export_gar_logits_process_rows():
    subprocess.run(["make", "-C", os.path.join(ROOT, "grasp-any-region_amd", "csrc"), "-j8"], check=True, capture_output=True)
    from gar_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "gar_hip.h")).read()
    assert "#define GAR_ABI_VERSION 16" in src                      # additive: the ABI number stands
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+gar_logits_process_rows\s*\(([^;]*)\)\s*;", src)
    assert decl, "gar_logits_process_rows is not declared in include/gar_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 14 == len(hip.SIGNATURES["gar_logits_process_rows"][0])
    assert any(a.startswith("const int32_t*") and a.endswith("row_params") for a in args) and args[-2] == "int row_words"
    # gar_logits_process keeps its signature, and the two differ in the block's name only
    old = re.search(r"\bint\s+gar_logits_process\s*\(([^;]*)\)\s*;", src)
    assert old and len(old.group(1).split(",")) == 14
    assert hip.SIGNATURES["gar_logits_process_rows"] == hip.SIGNATURES["gar_logits_process"]
    for f16 in (False, True):
        lib = hip.load_library(f16=f16)
        assert hasattr(lib, "gar_logits_process_rows") and lib.gar_abi_version() == 16
    for name in ("libgar_hip.so", "libgar_hip_f16.so"):
        out = subprocess.run(["nm", "-D", os.path.join(ROOT, "grasp-any-region_amd", "gar_amd", name)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        for sym in ("gar_logits_process_rows", "gar_logits_process"):
            assert any(ln.split()[-1] == sym and " T " in ln for ln in out.stdout.splitlines()), (name, sym)
    assert list(inspect.signature(ops.logits_process_rows).parameters) == ["logits", "V", "out_tokens", "step_dev", "eos_ids", "row_params"]
    assert list(inspect.signature(ops.logits_process).parameters) == ["logits", "V", "out_tokens", "step_dev", "eos_ids", "params"]
    assert ops.LOGITS_PROCESS_WORDS == 4096 and ops.LOGITS_PROCESS_HEADER == 8


def _stub_model(vocab=V):
    """what ContinuousBatcher's constructor and submit() touch before any device work"""
    text = types.SimpleNamespace(vocab_size=vocab)
    cfg = types.SimpleNamespace(mllm_config=types.SimpleNamespace(text_config=text))
    return types.SimpleNamespace(MAX_EOS_IDS=8, _check_decode_rows=lambda rows, what: None, config=cfg)


def _sample():
    import torch
    return dict(input_ids=torch.zeros(1, 4, dtype=torch.int64))


def test_submit_needs_the_flag_and_takes_neutral_requests_without_it():
    from gar_amd import LogitsProcessing, hip
    from gar_amd.continuous import ContinuousBatcher
    ps = inspect.signature(ContinuousBatcher.__init__).parameters
    assert list(ps)[-1] == "processing" and ps["processing"].default is False          # appended to the signature
    assert inspect.signature(ContinuousBatcher.submit).parameters["logits_processing"].default is None
    plain = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, eos_token_id=[5, 9])
    assert plain.processing is False
    for req in (dict(repetition_penalty=1.3), LogitsProcessing(no_repeat_ngram_size=2), dict(suppress_tokens=[1])):
        with pytest.raises(hip.GarError, match=r"processing=True"):
            plain.submit(_sample(), logits_processing=req)
    assert not plain.queue and plain._next_ticket == 0 and not plain._processing       # a refused request takes no ticket
    # a neutral request is a ticket without processing, on either kind of batcher
    flagged = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, eos_token_id=[5, 9], processing=True)
    for cb in (plain, flagged):
        ts = [cb.submit(_sample(), logits_processing=req)
              for req in (None, {}, LogitsProcessing(), dict(repetition_penalty=1.0, no_repeat_ngram_size=0), dict(repetition_penalty=1))]
        assert ts == [0, 1, 2, 3, 4] and len(cb.queue) == 5 and not cb._processing


def test_submit_records_and_validates_on_a_batcher_with_the_flag():
    from gar_amd import LogitsProcessing, hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.logits_processing import BLOCK_WORDS
    cb = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, eos_token_id=[5, 9], processing=True, sampling=True)
    assert cb.processing is True and cb.sampling is True
    t0 = cb.submit(_sample())
    t1 = cb.submit(_sample(), logits_processing=dict(repetition_penalty=1.3))
    t2 = cb.submit(_sample(), logits_processing=_everything())
    t3 = cb.submit(_sample(), do_sample=True, seed=7, logits_processing=dict(no_repeat_ngram_size=2))    # sampled and processed
    assert [t0, t1, t2, t3] == [0, 1, 2, 3]
    assert cb._processing == {t1: LogitsProcessing(repetition_penalty=1.3), t2: _everything(), t3: LogitsProcessing(no_repeat_ngram_size=2)}
    assert cb.seeds == {t3: 7}
    # refused at submit, as generate refuses them — and no ticket is taken, no seed drawn
    before = (len(cb.queue), cb._next_ticket, dict(cb._processing), dict(cb.seeds))
    with pytest.raises(ValueError, match="penalty"):
        cb.submit(_sample(), logits_processing=dict(repetition_penalty=0.0))
    with pytest.raises(TypeError, match="no_repeat"):
        cb.submit(_sample(), logits_processing=dict(no_repeat=3))
    with pytest.raises(TypeError, match="logits_processing"):
        cb.submit(_sample(), logits_processing=[1.3])
    for bad in (dict(suppress_tokens=[V]), dict(begin_suppress_tokens=[-1]), dict(bad_words_ids=[[1, V]])):
        with pytest.raises(hip.GarError, match="outside"):
            cb.submit(_sample(), logits_processing=bad)
    big = ContinuousBatcher(_stub_model(10 ** 5), 4, processing=True)
    with pytest.raises(hip.GarError, match=str(BLOCK_WORDS)):
        big.submit(_sample(), logits_processing=dict(suppress_tokens=list(range(BLOCK_WORDS - 7))))
    assert big.submit(_sample(), logits_processing=dict(suppress_tokens=list(range(BLOCK_WORDS - 8)))) == 0
    with pytest.raises(hip.GarError, match="outside"):
        cb.submit(_sample(), do_sample=True, logits_processing=dict(suppress_tokens=[V]))
    assert before == (len(cb.queue), cb._next_ticket, dict(cb._processing), dict(cb.seeds))
    # a vocabulary above the kernel's two LDS bitmaps
    from gar_amd import ops
    huge = ContinuousBatcher(_stub_model(ops.logits_process_max_vocab() + 1), 4, processing=True)
    with pytest.raises(hip.GarError, match="vocab_size"):
        huge.submit(_sample(), logits_processing=dict(repetition_penalty=1.3))
    assert huge.submit(_sample(), logits_processing={}) == 0 and huge._next_ticket == 1
    # min_new_tokens with more eos ids than the device table holds (the constructor refuses such a list; a table that shrank)
    few = ContinuousBatcher(_stub_model(), 4, eos_token_id=[1, 2, 3], processing=True)
    few.model.MAX_EOS_IDS = 2
    with pytest.raises(hip.GarError, match="min_new_tokens"):
        few.submit(_sample(), logits_processing=dict(min_new_tokens=3))
    assert few.submit(_sample(), logits_processing=dict(repetition_penalty=1.3)) == 0


def test_the_three_old_refusals_still_raise_by_name():
    from gar_amd import hip
    from gar_amd.continuous import ContinuousBatcher
    for kw in (dict(), dict(processing=True)):
        with pytest.raises(hip.GarError, match="logits_processing"):          # batcher-wide
            ContinuousBatcher(_stub_model(), 4, logits_processing=dict(repetition_penalty=1.2), **kw)
        cb = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, **kw)
        with pytest.raises(hip.GarError, match="logits_processing"):          # a key inside the sample dict
            cb.submit(dict(_sample(), logits_processing={}))
        with pytest.raises(hip.GarError, match="logits_processing"):
            cb.submit(dict(_sample(), logits_processing=dict(repetition_penalty=1.2)))
        for name, v in (("repetition_penalty", 1.2), ("no_repeat_ngram_size", 2), ("min_new_tokens", 3), ("suppress_tokens", [1]),
                        ("bad_words_ids", [[1]])):                            # HF's spellings
            with pytest.raises(hip.GarError, match=name):
                cb.submit(_sample(), **{name: v})
            with pytest.raises(hip.GarError, match=name):
                cb.submit(_sample(), generation_config={name: v})
        for key, val in (("return_logprobs", True), ("top_logprobs", 2), ("candidate_token_ids", [1])):
            with pytest.raises(hip.GarError, match=key):
                cb.submit(dict(_sample(), **{key: val}), logits_processing=dict(repetition_penalty=1.2))
        assert not cb.queue and cb._next_ticket == 0


def test_bench_loops_flags():
    from gar_amd import bench_loops as L
    ap = L.base_parser("loop", "tiny", "cache", "images")
    a = ap.parse_args(["--anno_file", "x.json", "--repetition_penalty", "1.2", "--no_repeat_ngram_size", "3", "--batch_size", "4"])
    assert L.processing_options(a) == dict(repetition_penalty=1.2, no_repeat_ngram_size=3)
    assert L.processing_options(ap.parse_args(["--anno_file", "x.json"])) == {}
    assert a.continuous is False                              # the other loops exit with a message, as --do_sample does
    with pytest.raises(SystemExit, match="repetition_penalty"):
        L.make_runner(None, None, a, True)
