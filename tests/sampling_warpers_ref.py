"""TEST INFRASTRUCTURE: float64 numpy restatement of HF's four further sampling warpers — MinPLogitsWarper, TypicalLogitsWarper,
EpsilonLogitsWarper, EtaLogitsWarper (transformers 5.15 generation/logits_process.py) in GenerationMixin._get_logits_processor's
order, min_tokens_to_keep = 1 — extending ``oracle.sampling.warp``'s (z, keep). tests/golden/sampling_warpers.npz pins it against
the warper classes themselves (tests/test_sampling_warpers_host.py).

Every stage's probabilities are the softmax over the set the stage before it left (HF has set the rest to -inf). A token whose
score is -inf is never "kept": HF cannot tell it from a removed one.

``warp_ext`` also returns the AMBIGUOUS ids of a row: tokens kept so far whose statistic lies within a relative band of a cut, so
that a float32 evaluation may legitimately decide them the other way. The band is 1e-4 = 5 x the MARGIN = 2e-5 tests/
test_gpu_sampling.py grants one 128 k-term f32 sum: a cut compares a ratio of two such sums, or a quantity built on an f32 entropy.
"""
import functools

import numpy as np

from oracle import sampling as S

BAND = 1e-4


def _strict_mass_before(order_key, e):
    """for every token: the mass (sum of e) of the tokens whose order_key is STRICTLY smaller; equal keys share one value"""
    order = np.argsort(order_key, kind="stable")
    ks, es = order_key[order], e[order]
    before = np.concatenate([[0.0], np.cumsum(es)[:-1]])
    first = np.r_[True, ks[1:] != ks[:-1]]
    strict = np.maximum.accumulate(np.where(first, before, -1.0))
    out = np.empty_like(strict)
    out[order] = strict
    return out


def warp_ext(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, band=BAND,
             with_distance=False):
    """(z, keep, ambiguous): z = logits / temperature in float32, keep = the final kept set (bool [V]), ambiguous = bool [V].
    ``with_distance``: a fourth value, float [V] — per token the smallest relative distance from a cut it was compared with while
    kept (inf for a token no stage compared), the quantity the band is a bound on."""
    z, keep = S.warp(logits, temperature, top_k, top_p)
    V = z.shape[-1]
    zd = z.astype(np.float64)
    finite = zd > -np.inf
    amb = np.zeros(V, dtype=bool)
    dist = np.full(V, np.inf)

    def mark(mask, rel, strict=False):
        nonlocal amb, dist
        amb |= mask & ((rel < band) if strict else (rel <= band))
        dist = np.minimum(dist, np.where(mask, rel, np.inf))
    # top-p's own cut, restated for its band (oracle.sampling.warp: keep iff the mass of the strictly larger logits < top_p x Z1)
    if top_p < 1.0:
        k1 = np.ones(V, dtype=bool)
        if 0 < top_k < V:
            k1 &= z >= np.sort(z)[V - top_k]
        e = np.where(k1, np.exp(zd - zd[k1].max()), 0.0)
        above = _strict_mass_before(np.where(k1, -zd, np.inf), e) / e.sum()
        assert np.array_equal(k1 & (above < top_p), keep), "restated top-p differs from oracle.sampling.warp"
        mark(k1 & finite, np.abs(above - top_p) / top_p)
    keep = keep & finite

    def probs(k):
        e = np.where(k, np.exp(zd - zd[k].max()), 0.0)
        return e / e.sum()

    def entropy(p):
        nz = p > 0
        return float(-(p[nz] * np.log(p[nz])).sum())

    if min_p > 0.0:                                         # MinPLogitsWarper: probs < min_p * max(probs) removed
        p = probs(keep)
        thr = min_p * p.max()
        mark(keep & (zd < zd[keep].max()), np.abs(p - thr) / thr)
        keep = keep & (p >= thr)
    if 0.0 < typical_p < 1.0:                               # TypicalLogitsWarper
        p = probs(keep)
        H = entropy(p)
        with np.errstate(divide="ignore"):
            s = np.where(keep, np.abs(-np.log(p) - H), np.inf)
        before = _strict_mass_before(s, p)
        stay = keep & (before < typical_p)
        s_cut = s[stay].max()
        mark(keep & (p > 0), np.abs(before - typical_p) / typical_p)
        with np.errstate(invalid="ignore"):
            mark(keep & (s != s_cut) & (p > 0), np.abs(s - s_cut) / max(1.0, H), strict=True)
        keep = stay
    for cutoff, eta_form in ((epsilon_cutoff, False), (eta_cutoff, True)):
        if 0.0 < cutoff < 1.0:                              # EpsilonLogitsWarper / EtaLogitsWarper
            p = probs(keep)
            thr = min(cutoff, np.sqrt(cutoff) * np.exp(-entropy(p))) if eta_form else cutoff
            top = zd == zd[keep].max()
            mark(keep & ~top, np.abs(p - thr) / thr)
            keep = keep & ((p >= thr) | top)
    return (z, keep, amb, dist) if with_distance else (z, keep, amb)


def sample_ext(logits, params, seed, row, step):
    """(token, margin, keep, ambiguous) of the draw gar_sample_ext makes: params = (temperature, top_k, top_p, min_p, typical_p,
    epsilon_cutoff, eta_cutoff)"""
    t, k, p, mp, typ, eps, eta = params
    z, keep, amb = warp_ext(logits, t, k, p, mp, typ, eps, eta)
    tok, margin = S.draw(z, keep, S.uniform(seed, row, step))
    return tok, margin, keep, amb


def warped_logprob(z, keep, tok):
    """log-probability of ``tok`` under softmax over the kept set"""
    zd = z.astype(np.float64)
    m = zd[keep].max()
    return float(zd[tok] - m - np.log(np.exp(zd[keep] - m).sum()))


# ---- the fixtures and parameter sets of tests/test_sampling_warpers_host.py and tests/test_gpu_sampling_warpers.py ----------------
# (temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff)
PARAM_SETS = [(1.0, 0, 1.0, .05, 1.0, 0.0, 0.0), (.7, 0, 1.0, .2, 1.0, 0.0, 0.0), (1.0, 0, 1.0, 0.0, .9, 0.0, 0.0),
              (1.3, 0, 1.0, 0.0, .2, 0.0, 0.0), (1.0, 0, 1.0, 0.0, 1.0, 3e-4, 0.0), (1.0, 0, 1.0, 0.0, 1.0, 0.0, 2e-3),
              (.8, 50, .95, .02, .95, 1e-3, 2e-3), (1.5, 0, .9, 0.0, .5, 0.0, 6e-4), (1.0, 0, 1.0, 0.0, 1.0, .9, 0.0),
              (1.0, 0, 1.0, 1.0, 1.0, 0.0, 0.0)]
SEEDS_STEPS = [(1, 0), (123456789012345, 3), (2 ** 61 + 7, 5)]
FIXTURES = ("flat37", "flat1000", "peaked128256")


def fixture(name):
    """the [8, V] float32 rows of a fixture (torch CPU tensor); cast to the dtype under test by the caller"""
    import torch
    if name.startswith("flat"):
        V = int(name[4:])
        g = torch.Generator().manual_seed(V)
        return torch.randn(8, V, generator=g) * 2.5
    V = int(name[len("peaked"):])
    g = torch.Generator().manual_seed(V)
    x = torch.randn(8, V, generator=g) - 12
    for b in range(8):
        ids = torch.randperm(V, generator=g)[:256]
        x[b, ids] = torch.randn(256, generator=g) * 3
    return x


DTYPES = ("float32", "bfloat16", "float16")


@functools.lru_cache(maxsize=None)
def group(name, dtype_name):
    """(logits, sets) of one (fixture, dtype) group, computed once per process and shared: logits = the fixture cast to the dtype,
    read back as float32 numpy [8, V]; sets[i][b] = (kept ids, ambiguous ids) of row b under PARAM_SETS[i]"""
    import torch
    lg = fixture(name).to(getattr(torch, dtype_name)).float().numpy()
    sets = []
    for params in PARAM_SETS:
        t, k, p, mp, typ, eps, eta = params
        rows = []
        for b in range(lg.shape[0]):
            _, keep, amb = warp_ext(lg[b], t, min(k, lg.shape[1]), p, mp, typ, eps, eta)
            rows.append((np.flatnonzero(keep), np.flatnonzero(amb)))
        sets.append(rows)
    return lg, sets


def ambiguous_rows(name, dtype_name):
    """how many of the group's 80 (set, row) pairs have an ambiguous token"""
    return sum(len(amb) > 0 for rows in group(name, dtype_name)[1] for _, amb in rows)
