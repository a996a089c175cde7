"""CPU: host side of generate(return_logprobs=True) — the option path, the eos mask / sum / count helper of generate_finish, and
the float64 references tests/test_gpu_logprobs.py compares the kernels with (tests/logprob_ref.py)."""
import inspect

import numpy as np
import pytest
import torch

from logprob_ref import MARGIN, check_warped, raw_logprob_at, raw_logprobs_f64, topp_neighbour_sets


def test_return_logprobs_is_an_option_of_generate_and_the_hf_flags_stay_inert():
    from gar_amd import hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import _GENERATION_KWARGS, GARModel, GenerateOutput, _option_reader, _refuse_non_greedy
    for fn in (GARModel.generate_begin, GARModel._generate_begin_fanout):
        p = inspect.signature(fn).parameters["return_logprobs"]
        assert p.default is False
    # generate_begin's own parameter, not a GenerationConfig field that **generate_kwargs would have to know
    assert "return_logprobs" not in _GENERATION_KWARGS
    # the HF flags for the dense tuples: accepted, read by nothing, refused by nothing — as before
    assert {"output_scores", "output_logits", "return_dict_in_generate"} <= _GENERATION_KWARGS
    get = _option_reader(None, dict(output_scores=True, output_logits=True, return_dict_in_generate=True))
    _refuse_non_greedy(get)
    fields = GenerateOutput.__dataclass_fields__
    for name in ("token_logprobs", "token_logprobs_warped", "sum_logprobs", "sum_logprobs_warped", "n_tokens"):
        assert fields[name].default is None
    # the continuous batcher does not carry the planes: asked for them, it says so by name
    with pytest.raises(hip.GarError, match="return_logprobs"):
        ContinuousBatcher(object(), 4, return_logprobs=True)


def test_ops_wrappers_take_the_planes():
    from gar_amd import hip, ops
    for fn in (ops.argmax, ops.sample):
        ps = inspect.signature(fn).parameters
        assert ps["logprobs"].default is None and ps["logprobs_warped"].default is None
    assert {"gar_argmax_lp", "gar_argmax_lp_workspace", "gar_sample_lp"} <= set(hip.SIGNATURES)
    # the existing entry points keep their signatures: the new ones are theirs plus the two planes
    assert len(hip.SIGNATURES["gar_argmax_lp"][0]) == len(hip.SIGNATURES["gar_argmax"][0]) + 2
    assert len(hip.SIGNATURES["gar_sample_lp"][0]) == len(hip.SIGNATURES["gar_sample"][0]) + 2


def test_eos_mask_sum_and_count():
    from gar_amd.modeling_gar import logprob_outputs
    n = 5
    raw = -torch.arange(1, 4 * n + 1, dtype=torch.float32).reshape(4, n) / 8          # exact in f32, sums too
    warped = raw / 2
    # finished_at = tokens up to and INCLUDING the first eos: a row ending at column 0, a row with no eos, two ragged rows
    finished_at = [1, None, 3, 5]
    tl, tw, sl, sw, nt = logprob_outputs(raw, warped, finished_at)
    assert nt.tolist() == [1, 5, 3, 5] and nt.dtype == torch.int32
    for r, end in enumerate([1, 5, 3, 5]):
        assert torch.equal(tl[r, :end], raw[r, :end]) and not tl[r, end:].any()
        assert torch.equal(tw[r, :end], warped[r, :end]) and not tw[r, end:].any()
        assert float(sl[r]) == float(raw[r, :end].sum()) and float(sw[r]) == float(warped[r, :end].sum())
    assert tl.dtype == torch.float32 and tuple(tl.shape) == (4, n) and tuple(sl.shape) == (4,)
    # stale values behind an eos never reach the sums, whatever they are (the steps keep writing those columns)
    dirty = raw.clone()
    dirty[0, 1:] = float("nan")
    dirty[2, 3:] = float("inf")
    tl2, _, sl2, _, _ = logprob_outputs(dirty, warped, finished_at)
    assert torch.equal(tl2, tl) and torch.equal(sl2, sl)
    # no eos anywhere: everything counts; a finished_at past the width (cannot happen) is clipped, not an index error
    tl3, _, sl3, _, nt3 = logprob_outputs(raw, warped, [None, None, None, 9])
    assert torch.equal(tl3, raw) and nt3.tolist() == [n] * 4 and torch.equal(sl3, raw.sum(1))
    # the inputs are left as they were
    assert float(raw[0, 1]) == -2 / 8


def test_float64_reference_against_torch_log_softmax_with_minus_inf():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 1000, generator=g) * 2.5
    x[1, 17] = float("-inf")
    x[1, 500:520] = float("-inf")
    ref = torch.log_softmax(x.double(), -1)
    got = raw_logprobs_f64(x)
    finite = torch.isfinite(ref)
    assert torch.equal(finite, torch.isfinite(got)) and not finite[1, 17] and got[1, 17] == float("-inf")
    assert float((got[finite] - ref[finite]).abs().max()) < 1e-12
    tok = torch.tensor([3, 18, 999])
    assert torch.equal(raw_logprob_at(x, tok), got[torch.arange(3), tok])
    # 16-bit logits are read as stored
    xb = x.to(torch.bfloat16)
    assert float((raw_logprobs_f64(xb)[finite] - torch.log_softmax(xb.double(), -1)[finite]).abs().max()) < 1e-12
    # one finite logit: probability 1
    one = torch.full((1, 37), float("-inf"))
    one[0, 5] = 0.5
    assert float(raw_logprob_at(one, torch.tensor([5]))) == 0.0


@pytest.mark.parametrize("setting", [(1.3, 0, 0.9), (0.6, 40, 0.8), (1.0, 5, 0.5), (2.0, 20000, 0.999), (0.7, 50, 1.0)])
def test_top_p_neighbour_sets_restate_the_oracle(setting):
    """the helper that names the acceptable neighbouring cuts computes the oracle's own kept set first: pinned here, so that
    the allowance in check_warped cannot drift from oracle/sampling.py"""
    from oracle import sampling as S
    T, k, p = setting
    g = torch.Generator().manual_seed(1000)
    x = (torch.randn(8, 1000, generator=g) * 2.5).numpy()
    x[3, 10:14] = x[3, 10]                    # a run of equal logits
    for b in range(8):
        z, keep = S.warp(x[b], T, min(k, 1000), p)
        mine, alts = topp_neighbour_sets(z, min(k, 1000), p)
        assert np.array_equal(mine, keep)
        for a in alts:                        # an alternative differs by whole runs on one side only
            assert (a <= keep).all() or (keep <= a).all()
            assert not np.array_equal(a, keep)
        # the reference value of a kept token, and the allowance refusing a value that is simply wrong
        tok = int(np.flatnonzero(keep)[0])
        zz = z.astype(np.float64)
        ref = zz[tok] - (zz[keep].max() + np.log(np.exp(zz[keep] - zz[keep].max()).sum()))
        assert check_warped(x[b], tok, float(ref), T, min(k, 1000), p) == 0
        with pytest.raises(AssertionError):
            check_warped(x[b], tok, float(ref) + 0.01, T, min(k, 1000), p)
    assert MARGIN == 2e-5
