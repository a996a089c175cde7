"""CPU: host side of generate(top_logprobs=, candidate_token_ids=) — the float64 reference tests/test_gpu_top_logprobs.py compares
the kernel with (tests/top_logprobs_ref.py), the argument refusals, the eos mask of the output fields, the GAR-Bench loop's option
letters and the parsers' new flags."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from logprob_ref import raw_logprobs_f64
from top_logprobs_ref import candidates_ref, close_or_both_minus_inf, topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(row, k):
    """the k best (index, value) of a list by repeated scan: larger value first, equal values by smaller index"""
    left = list(range(len(row)))
    out = []
    for _ in range(k):
        best = left[0]
        for i in left[1:]:
            if row[i] > row[best]:          # strict: the first index of a run of equal values wins
                best = i
        out.append(best)
        left.remove(best)
    return out


def test_reference_against_a_brute_force_sort_with_ties_and_minus_inf():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(6, 23, generator=g)
    x[1] = 0.25                                             # every entry ties: ids 0..k-1
    x[2, [3, 9, 10]] = float(x[2].max()) + 1.0              # a three-way tie at the top
    x[3] = float("-inf")
    x[3, [20, 4, 11]] = torch.tensor([0.5, 0.5, -1.0])      # three finite entries, the rest -inf by index
    x[4, 5:9] = float("-inf")
    x[5] = x[5].to(torch.bfloat16).float()                  # a coarse grid: genuine ties
    for k in (1, 5, 23):
        ids, lp = topk_ref(x, k)
        assert ids.dtype == torch.int64 and tuple(ids.shape) == tuple(lp.shape) == (6, k)
        full = raw_logprobs_f64(x)
        for b in range(6):
            assert ids[b].tolist() == _brute(x[b].tolist(), k), (b, k)
            assert torch.equal(lp[b], full[b, ids[b]])
    assert topk_ref(x, 5)[0][1].tolist() == [0, 1, 2, 3, 4]
    assert topk_ref(x, 3)[0][2].tolist() == [3, 9, 10]
    ids, lp = topk_ref(x, 6)
    assert ids[3].tolist() == [4, 20, 11, 0, 1, 2] and torch.isneginf(lp[3, 3:]).all() and torch.isfinite(lp[3, :3]).all()
    # 16-bit logits are compared as stored; leading axes are kept
    xb = x.to(torch.bfloat16).view(2, 3, 23)
    ids, lp = topk_ref(xb, 4)
    assert tuple(ids.shape) == (2, 3, 4) and ids[1, 2].tolist() == _brute(xb[1, 2].float().tolist(), 4)
    c = candidates_ref(x, [0, 22, 4])
    assert tuple(c.shape) == (6, 3) and torch.equal(c[:, 1], raw_logprobs_f64(x)[:, 22]) and torch.isneginf(c[3, 0])
    # the comparison helper: -inf must sit exactly where the reference has it
    assert close_or_both_minus_inf(c.float(), c, 1e-6) <= 1e-6
    with pytest.raises(AssertionError):
        close_or_both_minus_inf(torch.zeros_like(c), c, 1e-6)
    with pytest.raises(AssertionError):
        close_or_both_minus_inf(c + torch.where(torch.isneginf(c), 0.0, 1e-3), c, 1e-4)


def test_argument_refusals():
    from gar_amd import hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import _GENERATION_KWARGS, GARModel, GenerateOutput, top_logprob_options
    V = 1000
    assert top_logprob_options(0, None, V) == (0, [])
    assert top_logprob_options(32, range(64), V) == (32, list(range(64)))
    assert top_logprob_options(5, [0, V - 1, np.int64(7)], V) == (5, [0, V - 1, 7])
    assert top_logprob_options(20, None, 20) == (20, [])
    for k in (33, -1, 2.0, "5", True, None):
        with pytest.raises(ValueError, match="top_logprobs"):
            top_logprob_options(k, None, V)
    with pytest.raises(ValueError, match="top_logprobs"):          # k > V
        top_logprob_options(21, None, 20)
    with pytest.raises(ValueError, match="65 ids"):
        top_logprob_options(0, list(range(65)), V)
    for bad in (V, -1, 2.5):
        with pytest.raises(ValueError, match="candidate_token_ids"):
            top_logprob_options(0, [1, bad], V)
    # explicit parameters of generate, like return_logprobs — not generation-config options
    for fn, names in ((GARModel.generate_begin, ("top_logprobs", "candidate_token_ids")),
                      (GARModel._generate_begin_fanout, ("top_k_lp", "cands"))):
        ps = inspect.signature(fn).parameters
        assert all(n in ps for n in names)
    ps = inspect.signature(GARModel.generate_begin).parameters
    assert ps["top_logprobs"].default == 0 and ps["candidate_token_ids"].default is None
    assert not {"top_logprobs", "candidate_token_ids"} & set(_GENERATION_KWARGS)
    for name in ("top_logprob_ids", "top_logprobs", "candidate_logprobs"):
        assert GenerateOutput.__dataclass_fields__[name].default is None
    with pytest.raises(hip.GarError, match="top_logprobs"):
        ContinuousBatcher(object(), 4, top_logprobs=1)
    with pytest.raises(hip.GarError, match="candidate_token_ids"):
        ContinuousBatcher(object(), 4, candidate_token_ids=[3])


def test_bindings_and_wrapper():
    from gar_amd import hip, ops
    assert {"gar_topk_lp", "gar_topk_lp_workspace"} <= set(hip.SIGNATURES)
    assert len(hip.SIGNATURES["gar_topk_lp"][0]) == 18 and len(hip.SIGNATURES["gar_topk_lp_workspace"][0]) == 3
    assert hip.ABI_VERSION == 16
    ps = inspect.signature(ops.topk_lp).parameters
    assert all(ps[n].default is None for n in ("top_ids", "top_lp", "cand_ids", "cand_lp"))
    assert (ops.TOPK_MAX, ops.TOPK_CAND_MAX) == (32, 64)
    # one group's halves go together (checked before any pointer is taken)
    with pytest.raises(hip.GarError, match="goes with"):
        ops.topk_lp(torch.zeros(2, 64), 37, None, torch.zeros(8, dtype=torch.uint8), top_ids=torch.zeros(2, 1, 1, dtype=torch.int32))


def test_output_fields_are_masked_behind_the_first_eos():
    from gar_amd.modeling_gar import top_logprob_outputs
    R, T, n, k, C = 3, 8, 5, 2, 3
    ids = torch.arange(R * T * k, dtype=torch.int32).view(R, T, k)
    lp = -torch.arange(R * T * k, dtype=torch.float32).view(R, T, k) - 1
    cl = -torch.arange(R * T * C, dtype=torch.float32).view(R, T, C) - 1
    cl[0, 0, 1] = float("-inf")
    tk = dict(k=k, C=C, ids=ids, lp=lp, cand_ids=torch.zeros(C, dtype=torch.int32), cand_lp=cl)
    out = top_logprob_outputs(tk, n, [2, None, 5])
    assert out["top_logprob_ids"].dtype == torch.int64 and out["top_logprobs"].dtype == torch.float32
    assert tuple(out["top_logprob_ids"].shape) == (R, n, k) and tuple(out["candidate_logprobs"].shape) == (R, n, C)
    for r, end in enumerate((2, 5, 5)):
        assert torch.equal(out["top_logprob_ids"][r, :end], ids[r, :end].long()) and (out["top_logprob_ids"][r, end:] == -1).all()
        assert torch.equal(out["top_logprobs"][r, :end], lp[r, :end]) and not out["top_logprobs"][r, end:].any()
        assert torch.equal(out["candidate_logprobs"][r, :end], cl[r, :end]) and not out["candidate_logprobs"][r, end:].any()
    assert float(out["candidate_logprobs"][0, 0, 1]) == float("-inf")            # a -inf value in a kept column stays
    # either group alone
    only = top_logprob_outputs(dict(tk, ids=None, lp=None), n, [None] * R)
    assert set(only) == {"candidate_logprobs"} and torch.equal(only["candidate_logprobs"], cl[:, :n])
    only = top_logprob_outputs(dict(tk, cand_ids=None, cand_lp=None), n, [None] * R)
    assert set(only) == {"top_logprob_ids", "top_logprobs"}


def test_option_letters_and_their_token_ids():
    from gar_amd.bench_loops import option_letters, option_token_ids
    from gar_amd.processing import StubTokenizer
    item = {"choices": ["A. <Prompt0>", "B. the one on the left. Really", "C.", " D . x", "Yes"]}
    assert option_letters(item) == ["A", "B", "C", "D", "Yes"]
    tk = StubTokenizer.tiny()
    assert option_token_ids(tk, ["A", "B", "C"]) == [tk.encode("A")[0], tk.encode("B")[0], tk.encode("C")[0]]
    with pytest.raises(ValueError, match="'Yes'"):
        option_token_ids(tk, ["A", "Yes"])
    with pytest.raises(ValueError, match="''"):
        option_token_ids(tk, [""])


def test_parsers_accept_the_new_flags():
    from gar_amd.bench_loops import gar_bench_parser, run_gar_bench
    a = gar_bench_parser().parse_args(["--anno_file", "x.json", "--mode", "vqa", "--option_logprobs", "--batch_size", "4"])
    assert a.option_logprobs is True
    assert gar_bench_parser().parse_args(["--anno_file", "x.json", "--mode", "vqa"]).option_logprobs is False
    # refused by name before anything is loaded: with --continuous, and outside --mode vqa
    with pytest.raises(SystemExit, match="--continuous"):
        run_gar_bench(["--anno_file", "x.json", "--mode", "vqa", "--option_logprobs", "--continuous", "--batch_size", "4"])
    with pytest.raises(SystemExit, match="--mode vqa"):
        run_gar_bench(["--anno_file", "x.json", "--mode", "simple", "--option_logprobs"])
    sys.path.insert(0, os.path.join(ROOT, "demo"))
    try:
        import _common
    finally:
        sys.path.remove(os.path.join(ROOT, "demo"))
    ap = _common.base_parser("t")
    assert ap.parse_args(["--top_logprobs", "5"]).top_logprobs == 5 and ap.parse_args([]).top_logprobs == 0
