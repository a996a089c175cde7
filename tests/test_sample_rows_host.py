"""CPU: the host side of per-request sampling in ContinuousBatcher — the eight request words of a row
(continuous.pack_sample_row), the declaration / export / binding of gar_sample_rows, and the refusals of submit() that need no
device."""
import inspect
import os
import re
import struct
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u32(w):
    return w & 0xffffffff


def _f32(w):
    return struct.unpack("<f", struct.pack("<I", _u32(w)))[0]


def test_pack_greedy_words_are_zero_except_col0():
    from gar_amd.continuous import SAMPLE_ROW_WORDS, pack_sample_row
    assert SAMPLE_ROW_WORDS == 8
    assert pack_sample_row(None, None, 0) == [0] * 8
    assert pack_sample_row(None, None, 17) == [0, 0, 0, 0, 0, 0, 17, 0]
    assert pack_sample_row(None, 12345, 3, counter_row=9) == [0, 0, 0, 0, 0, 0, 3, 0]     # a greedy row draws nothing: no key, no counter


def test_pack_sampled_words_round_trip():
    import numpy as np
    from gar_amd.continuous import pack_sample_row
    for temperature, top_p, top_k in [(1.0, 1.0, 0), (0.7, 0.9, 50), (1.3, 0.999, 20000), (1e-3, 1e-6, 1), (2.0, 0.5, 2 ** 31 - 1)]:
        w = pack_sample_row((temperature, top_p, top_k), 7, 5, counter_row=3)
        assert len(w) == 8 and all(isinstance(x, int) and -2 ** 31 <= x < 2 ** 31 for x in w)
        assert w[0] == 1 and w[3] == top_k and w[6] == 5 and w[7] == 3
        # the floats are the IEEE binary32 bits of the values as float32 holds them
        assert _f32(w[1]) == float(np.float32(temperature)) and _f32(w[2]) == float(np.float32(top_p))
    np.array(pack_sample_row((0.7, 0.9, 50), 2 ** 63 - 1, 0), dtype=np.int32)      # fits the device table's type as it stands


def test_pack_seed_splits_into_two_words():
    from gar_amd.continuous import pack_sample_row
    for seed in (0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 123456789012345, 2 ** 61 + 7, 0x2AAAAAAA_D5555555, 2 ** 62 - 1, 2 ** 63 - 1):
        w = pack_sample_row((1.0, 1.0, 0), seed, 0)
        assert _u32(w[4]) == seed & 0xffffffff and _u32(w[5]) == seed >> 32
        assert _u32(w[4]) | (_u32(w[5]) << 32) == seed


def test_pack_refuses_bad_words():
    from gar_amd.continuous import pack_sample_row
    ok = (0.8, 0.9, 40)
    for mode in (2, -1, True, 1.5):
        with pytest.raises(ValueError, match="mode"):
            pack_sample_row(ok, 1, 0, mode=mode)
    with pytest.raises(ValueError, match="mode"):          # a mode that contradicts the parameters
        pack_sample_row(ok, 1, 0, mode=0)
    with pytest.raises(ValueError, match="mode"):
        pack_sample_row(None, 1, 0, mode=1)
    for t in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            pack_sample_row((t, 0.9, 40), 1, 0)
    for p in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            pack_sample_row((0.8, p, 40), 1, 0)
    for k in (-1, 2.5, 2 ** 31):
        with pytest.raises(ValueError, match="top_k"):
            pack_sample_row((0.8, 0.9, k), 1, 0)
    for seed in (-1, 2 ** 63, None, 1.5):
        with pytest.raises(ValueError, match="seed"):
            pack_sample_row(ok, seed, 0)
    with pytest.raises(ValueError, match="col0"):
        pack_sample_row(ok, 1, 2 ** 31)
    with pytest.raises(ValueError, match="counter_row"):
        pack_sample_row(ok, 1, 0, counter_row=-1)


def test_header_declares_and_libraries_export_gar_sample_rows():
    subprocess.run(["make", "-C", os.path.join(ROOT, "grasp-any-region_amd", "csrc"), "-j8"], check=True, capture_output=True)
    from gar_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "gar_hip.h")).read()
    assert "#define GAR_ABI_VERSION 16" in src                      # additive: the ABI number stands
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+gar_sample_rows\s*\(([^;]*)\)\s*;", src)
    assert decl, "gar_sample_rows is not declared in include/gar_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 15 == len(hip.SIGNATURES["gar_sample_rows"][0])
    assert any(a.startswith("const int32_t*") and a.endswith("row_words") for a in args)
    # gar_sample / gar_sample_lp / gar_argmax keep their signatures
    assert [len(hip.SIGNATURES[n][0]) for n in ("gar_sample", "gar_sample_lp", "gar_argmax")] == [17, 19, 15]
    for f16 in (False, True):
        lib = hip.load_library(f16=f16)
        assert hasattr(lib, "gar_sample_rows") and lib.gar_abi_version() == 16
    for name in ("libgar_hip.so", "libgar_hip_f16.so"):
        out = subprocess.run(["nm", "-D", os.path.join(ROOT, "grasp-any-region_amd", "gar_amd", name)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert any(ln.split()[-1] == "gar_sample_rows" and " T " in ln for ln in out.stdout.splitlines()), name
    ps = list(inspect.signature(ops.sample_rows).parameters)
    assert ps == ["logits", "V", "out_tokens", "out_stride", "step_dev", "cur_tokens", "row_words", "eos_ids", "finished", "done_count"]
    assert ops.SAMPLE_ROW_WORDS == 8


def _stub_model():
    """what ContinuousBatcher's constructor and submit() touch before any device work"""
    return types.SimpleNamespace(MAX_EOS_IDS=8, _check_decode_rows=lambda rows, what: None)


def _sample():
    import torch
    return dict(input_ids=torch.zeros(1, 4, dtype=torch.int64))


def test_submit_refusals_that_need_no_device():
    from gar_amd import hip
    from gar_amd.continuous import ContinuousBatcher
    assert inspect.signature(ContinuousBatcher.__init__).parameters["sampling"].default is False
    ps = inspect.signature(ContinuousBatcher.submit).parameters
    assert ps["generation_config"].default is None and ps["seed"].default is None
    greedy = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, eos_token_id=[5, 9])
    assert greedy.sampling is False
    # do_sample on a batcher without the flag: the refusal names the constructor flag
    for kw in (dict(do_sample=True), dict(generation_config=dict(do_sample=True, temperature=0.7))):
        with pytest.raises(hip.GarError, match=r"sampling=True"):
            greedy.submit(_sample(), **kw)
    cb = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, eos_token_id=[5, 9], sampling=True)
    with pytest.raises(hip.GarError, match="num_return_sequences.*call generate"):
        cb.submit(_sample(), do_sample=True, num_return_sequences=2)
    with pytest.raises(hip.GarError, match="num_return_sequences"):
        greedy.submit(_sample(), num_return_sequences=2)
    with pytest.raises(hip.GarError, match="max_new_tokens"):
        cb.submit(_sample(), do_sample=True, max_new_tokens=8)
    with pytest.raises(hip.GarError, match="max_new_tokens"):
        cb.submit(_sample(), generation_config=dict(max_new_tokens=17))
    with pytest.raises(hip.GarError, match="eos_token_id"):
        cb.submit(_sample(), eos_token_id=7)
    with pytest.raises(hip.GarError, match="typical_p"):
        cb.submit(_sample(), do_sample=True, typical_p=0.5)
    with pytest.raises(hip.GarError, match="min_p"):
        cb.submit(_sample(), generation_config=dict(do_sample=True, min_p=0.1))
    with pytest.raises(hip.GarError, match="num_beams"):
        cb.submit(_sample(), num_beams=2)
    with pytest.raises(hip.GarError, match="repetition_penalty"):
        cb.submit(_sample(), repetition_penalty=1.2)
    with pytest.raises(TypeError, match="no_such_option"):
        cb.submit(_sample(), no_such_option=1)
    with pytest.raises(ValueError, match="temperature"):
        cb.submit(_sample(), do_sample=True, temperature=0.0)
    with pytest.raises(ValueError, match="seed"):
        cb.submit(_sample(), do_sample=True, seed=-3)
    # still refused by name, exactly as before
    for key, val in (("return_logprobs", True), ("top_logprobs", 2), ("candidate_token_ids", [1]), ("logits_processing", {})):
        with pytest.raises(hip.GarError, match=key):
            cb.submit(dict(_sample(), **{key: val}))
        with pytest.raises(hip.GarError, match=key):
            ContinuousBatcher(_stub_model(), 4, sampling=True, **{key: val if key != "logits_processing" else dict(repetition_penalty=1.2)})
    assert not cb.queue and not cb.seeds and cb._next_ticket == 0          # a refused request takes no ticket


def test_submit_records_requests_and_seeds():
    import torch
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import _draw_seed
    cb = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, eos_token_id=[5, 9], sampling=True)
    t0 = cb.submit(_sample())                                                         # greedy
    t1 = cb.submit(_sample(), do_sample=True, seed=1001)                              # HF's defaults: top_k 50
    t2 = cb.submit(_sample(), generation_config=dict(do_sample=True, temperature=0.7, top_k=0), top_p=0.9, seed=2 ** 61 + 5,
                   max_new_tokens=16, eos_token_id=[9, 5])                            # the batcher's own values pass
    t3 = cb.submit(_sample(), do_sample=False, temperature=0.3, seed=5)               # sampling knobs without do_sample: greedy, as in HF
    torch.manual_seed(11)
    want = _draw_seed()
    torch.manual_seed(11)
    t4 = cb.submit(_sample(), do_sample=True)                                         # the key generate() would draw
    assert [t0, t1, t2, t3, t4] == [0, 1, 2, 3, 4] and len(cb.queue) == 5
    assert cb.seeds == {t1: 1001, t2: 2 ** 61 + 5, t4: want} and 0 <= want < 2 ** 62
    assert cb._requests[t1] == ((1.0, 1.0, 50), 1001) and cb._requests[t2] == ((0.7, 0.9, 0), 2 ** 61 + 5)
    assert t0 not in cb._requests and t3 not in cb._requests
    # a batcher without the flag takes option-free and greedy requests as before
    g = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16)
    assert g.submit(_sample()) == 0 and g.submit(_sample(), do_sample=False, max_new_tokens=16) == 1 and not g.seeds
