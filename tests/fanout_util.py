"""float64 restatement of decode attention over a shared prompt prefix plus a private suffix (generate(num_return_sequences = N);
csrc/attention_decode.hip, gar_attention_decode_fanout) for the tests: plain softmax attention, and the same result put
together the way the kernel does it — (m, l, O) partials of the prefix splits and of the suffix, merged as one softmax.
Scores are in the log2 domain (the query carries head_dim ** -0.5 * log2(e)), so the softmax is exp2-based like the kernels'."""
import torch


def softmax_attention(q, K, V):
    """q [hd], K / V [n, hd] (n >= 1) -> [hd], float64"""
    s = K.double() @ q.double()
    p = torch.exp2(s - s.max())
    return (p[:, None] * V.double()).sum(0) / p.sum()


def partial(q, K, V):
    """un-normalised partial of one block of keys: (m, l, O) with O = sum_j 2^(s_j - m) v_j; no keys: (-inf, 0, 0)"""
    hd = q.shape[0]
    if K.shape[0] == 0:
        return float("-inf"), 0.0, torch.zeros(hd, dtype=torch.float64)
    s = K.double() @ q.double()
    m = float(s.max())
    p = torch.exp2(s - m)
    return m, float(p.sum()), (p[:, None] * V.double()).sum(0)


def merge(parts):
    """decode_combine_kernel: partials (m, l, O) of one softmax -> the normalised output"""
    m = max(p[0] for p in parts)
    m_use = 0.0 if m == float("-inf") else m
    l = sum(2.0 ** (p[0] - m_use) * p[1] for p in parts if p[0] != float("-inf"))
    acc = sum((2.0 ** (p[0] - m_use) * p[2] for p in parts if p[0] != float("-inf")), torch.zeros_like(parts[0][2]))
    return acc / l if l > 0 else acc


def prefix_split_ranges(P, left_pad, nsplit):
    """cache-row ranges [lo, hi) the kernel's prefix splits take: the 64-row tiles from the one holding left_pad to the last,
    dealt in equal runs; rows outside left_pad .. P - 1 are masked"""
    lo = max(min(left_pad, P - 1), 0)
    ntiles, t_lo = (P + 63) // 64, lo // 64
    per = (ntiles - t_lo + nsplit - 1) // nsplit
    out = []
    for s in range(nsplit):
        t0 = t_lo + s * per
        t1 = min(ntiles, t0 + per)
        out.append((max(lo, t0 * 64), max(lo, min(P, t1 * 64))) if t0 < t1 else (lo, lo))
    return out


def fanout_attention(q, Kp, Vp, P, left_pad, Ks, Vs, t, nsplit):
    """One (row, head): q [hd]; the prompt's Kp / Vp [Sp, hd], rows left_pad .. P - 1 live; the row's own Ks / Vs [T, hd], rows
    0 .. t live (row t = the step's new token, already appended). The kernel's order: prefix splits, suffix, merge."""
    parts = [partial(q, Kp[a:b], Vp[a:b]) for a, b in prefix_split_ranges(P, left_pad, nsplit)]
    parts.append(partial(q, Ks[:t + 1], Vs[:t + 1]))
    return merge(parts)


def batched_attention(Q, K, V, lo, n):
    """Q [R, Hq, hd], K / V [R, Hkv, S, hd], keys lo[r] .. n - 1 of every row -> [R, Hq, hd] float64 (any device)"""
    R, Hq, hd = Q.shape
    Hkv = K.shape[1]
    G = Hq // Hkv
    Kd = K[:, :, :n].double().repeat_interleave(G, 1)
    Vd = V[:, :, :n].double().repeat_interleave(G, 1)
    s = torch.einsum("rhd,rhnd->rhn", Q.double(), Kd)
    hidden = torch.arange(n, device=Q.device)[None, None, :] < lo.to(Q.device)[:, None, None]
    s = s.masked_fill(hidden, float("-inf"))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return torch.einsum("rhn,rhnd->rhd", p, Vd) / p.sum(-1, keepdim=True)
