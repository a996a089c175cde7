"""Float64 references for the log-probability tests (tests/test_logprobs_host.py pins them on the CPU, tests/test_gpu_logprobs.py
compares the kernels and generate(return_logprobs=True) with them)."""
import numpy as np
import torch

LP_TOL = 1e-4        # kernel against float64 on the same stored logits, absolute, on one log-probability: a float32 sum of <= 128256
#                      non-negative terms (~125 per thread, then a tree) with __expf and logf is bounded near 2e-5; this is ~5x that
MARGIN = 2e-5        # tests/test_gpu_sampling.py: how close (relative to the mass) a float32 sum may sit to a boundary and fall across


def raw_logprobs_f64(logits: torch.Tensor) -> torch.Tensor:
    """log_softmax over the last axis in float64 of the logits as stored (any dtype): x - max - log sum exp(x - max). A -inf
    entry contributes exp(-inf) = 0 and its own log-probability is -inf."""
    x = logits.detach().to("cpu", torch.float64)
    m = x.max(-1, keepdim=True).values
    return x - m - torch.log(torch.exp(x - m).sum(-1, keepdim=True))


def raw_logprob_at(logits: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """[...]: raw_logprobs_f64(logits) [..., V] gathered at ``tokens`` [...]"""
    return raw_logprobs_f64(logits).gather(-1, tokens.detach().cpu().to(torch.int64)[..., None])[..., 0]


def _lse64(v: np.ndarray) -> float:
    v = v.astype(np.float64)
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def topp_neighbour_sets(z: np.ndarray, top_k: int, top_p: float):
    """(keep, alternatives): ``keep`` restates oracle/sampling.py's warp on z = logits / T (float32); ``alternatives`` are the kept
    sets with the one neighbouring run of equal logits at the top-p cut dropped / added — listed only when the oracle's own cut
    lies within MARGIN of top_p x Z1 (relative to Z1), which is where a float32 mass sum may legitimately land on the other side."""
    V = z.shape[-1]
    keep_k = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        keep_k &= z >= np.sort(z)[V - top_k]
    if not top_p < 1.0:
        return keep_k, []
    m = z[keep_k].max()
    e = np.where(keep_k, np.exp((z - m).astype(np.float64)), 0.0)
    Z1 = e.sum()
    lim = top_p * Z1
    u, inv = np.unique(z[keep_k], return_inverse=True)
    mass = np.bincount(inv.ravel(), weights=e[keep_k], minlength=len(u))[::-1]
    u = u[::-1]                                                   # runs of equal logits, largest first
    above = np.concatenate([[0.0], np.cumsum(mass)[:-1]])         # mass of the strictly larger logits
    r = int(np.flatnonzero(above < lim)[-1])                      # the last run that stays (run 0 always does)
    alts = []
    if r > 0 and (lim - above[r]) / Z1 < MARGIN:
        alts.append(keep_k & (z > u[r]))
    if r + 1 < len(u) and (above[r + 1] - lim) / Z1 < MARGIN:
        alts.append(keep_k & (z >= u[r + 1]))
    return keep_k & (z >= u[r]), alts


def check_warped(logits_row: np.ndarray, tok: int, got: float, temperature: float, top_k: int, top_p: float) -> int:
    """The warped log-probability ``got`` of token ``tok`` against z[tok] - logsumexp(z[keep]) in float64 with the oracle's keep
    (oracle/sampling.py warp). Returns 0 when it matches within LP_TOL, 1 when it matches only with the neighbouring run at a
    top-p cut that lies within MARGIN added or dropped (the caller caps those at 1 % of its cases); asserts otherwise."""
    from oracle import sampling as S
    z, keep = S.warp(logits_row, temperature, top_k, top_p)
    ref = float(z[tok]) - _lse64(z[keep])
    if abs(got - ref) <= LP_TOL:
        return 0
    for alt in topp_neighbour_sets(z, top_k, top_p)[1]:
        if abs(got - (float(z[tok]) - _lse64(z[alt]))) <= LP_TOL:
            return 1
    raise AssertionError(f"warped log-probability {got} of token {tok}: float64 {ref} (T {temperature}, top_k {top_k}, top_p {top_p})")
