"""Float64 reference for gar_topk_lp and generate(top_logprobs=, candidate_token_ids=) (tests/test_top_logprobs_host.py pins it on
the CPU, tests/test_gpu_top_logprobs.py compares the kernel and generate() with it): the log-probabilities are
tests/logprob_ref.py's raw_logprobs_f64 of the logits as stored, the order is (value descending, index ascending) by np.lexsort —
not torch.topk, whose order among equal values is unspecified."""
import numpy as np
import torch

from logprob_ref import raw_logprobs_f64


def topk_ref(logits: torch.Tensor, k: int):
    """(ids int64 [..., k], lp float64 [..., k]) of ``logits`` [..., V] (any dtype, compared as stored): the k largest entries,
    equal values by ascending index, -inf entries last (by index), with lp = x - logsumexp(x) in float64."""
    x = logits.detach().to("cpu", torch.float64).numpy()
    lp = raw_logprobs_f64(logits).numpy()
    flat, flp = x.reshape(-1, x.shape[-1]), lp.reshape(-1, x.shape[-1])
    idx = np.arange(x.shape[-1])
    ids = np.stack([np.lexsort((idx, -row))[:k] for row in flat])
    vals = np.take_along_axis(flp, ids, 1)
    shape = x.shape[:-1] + (k,)
    return torch.from_numpy(ids.reshape(shape).astype(np.int64)), torch.from_numpy(vals.reshape(shape))


def candidates_ref(logits: torch.Tensor, cand_ids):
    """float64 [..., C]: raw_logprobs_f64(logits) at the ids of ``cand_ids``"""
    return raw_logprobs_f64(logits)[..., torch.as_tensor(list(cand_ids), dtype=torch.int64)]


def close_or_both_minus_inf(got: torch.Tensor, ref: torch.Tensor, tol: float):
    """max |got - ref| over the finite reference entries (float); asserts that got is -inf exactly where ref is"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    minf = torch.isneginf(ref)
    assert torch.equal(torch.isneginf(got), minf), "-inf entries differ"
    if bool(minf.all()):
        return 0.0
    err = float((got[~minf] - ref[~minf]).abs().max())
    assert err <= tol, (err, tol)
    return err
