"""float64 restatement of the attention kernels (csrc/attention_bf16.hip: attn_bf16_v2_kernel; csrc/attention.hip: attn_f32_kernel;
csrc/attention_decode.hip: the split-KV decode kernels) for the tests, with a bound on |kernel - restatement| PER ELEMENT, and the
input families that put a row's weight on one chosen key. Pure torch, no GPU library: it runs on the CPU and, in float64, on the device.

Layouts: Q [B, Hq, n, hd] ALREADY carries head_dim ** -0.5 * log2(e) and is rounded to the kernel's type, K and V [B, Hkv, rows, hd]
(V row-major) are rounded to it too: the restatement sees exactly the kernel's inputs. The softmax is exp2-based, as the kernels'.

What is stated ONCE here:
    GQA        query head h reads kv head h // (Hq // Hkv) (torch's repeat_interleave of the kv heads by Hq // Hkv; done as a
               [B, Hkv, G * rows, hd] view of Q, so that no copy of K is made)
    causal     key kv is visible to query row q iff kv <= q + coff, coff = kv_len - q_len
    left pad   a key is visible iff kv_lo <= kv <= max(q + coff, kv_lo) (attention_bf16.hip): a row in front of kv_lo sees key kv_lo alone
    kv_len     rows >= kv_len of K / V are never visible

THE BOUND (attention_bound), term by term, from the arithmetic the kernels do. p_j = the normalised softmax weights in f64,
ref_d = sum_j p_j v_jd, A_d = sum_j p_j |v_jd| (so |ref| <= A), u = the unit roundoff of the 16-bit type: round-to-nearest-even
of x errs by at most u |x|, u = 2^-8 for bfloat16 (8 significand bits) and 2^-11 for float16. (2^-9 / 2^-12 is that error at the
TOP of a binade, not a bound: 1 + 2^-8 rounds to 1 or to 1 + 2^-7.)
  16-bit kernels (prefill, ViT, decode — the same three steps in each):
    1. P -> 16 bits before the PV MFMA (cvt_pk): the numerator sum_j p_j v_jd takes |sum_j delta_j p_j v_jd| <= u A_d.
    2. the row sum l is taken from the UNROUNDED f32 p (ps += p[r] before the pack): the denominator carries no 16-bit error, so
       there is no second P term (with l from the rounded P it would be u (A + |ref|)).
    3. the output O / l is rounded ONCE to 16 bits (st4 / f2bf): u |ref|.
    so 16-bit: u (A + |ref|) <= 2 u A = 4 * 2^-9 A in bfloat16; where a row averages many keys |ref| << A and it is 2 * 2^-9 A.
    float16 only: a P below 2^-14 is subnormal in float16, its error is absolute, 2^-25 (at worst it flushes to 0). In the kernel's units
       l >= 1 (its base m is never above the row's true max), so such a key's weight errs by <= 2^-25 / L, L = sum_j 2^(s_j - max s):
       attention_ref counts every visible key with 2^(s_j - max s) < 2^-14 into A with the weight 2^-14 / L instead of p_j, and
       u * 2^-14 = 2^-25: the term rides in u A.
  every kernel, in f32 (these are the f32 kernel's only terms; with 16 bits they are small against u but not against float16's u
  at scores of 24 log2 units):
    4. a score is a chain of hd f32 multiply-adds (16-bit products are exact, f32 ones round too), in the v2 kernel started from
       -m: every partial sum is below 2 smag, smag = |q| max_j |k_j| >= sum_d |q_d k_jd|, so |ds| <= 2 (hd + 1) 2^-24 smag and
       p_j is off by the factor 2^ds: ln2 |ds| relative. v_exp_f32 / exp2f and the subtraction of m: 2^-22.
       Numerator and denominator both carry it: (ln2 |ds| + 2^-22) (A + |ref|).
    5. O and l are f32 sums of n_keys terms in some order, rescaled once per 64-key tile, merged over 4 waves and up to 64 splits:
       (n_keys (1 + 1/64) + 72) 2^-24 of sum |terms|, i.e. of A for O and of |ref| for l.
    6. f32 output: 1 / l and the product, 2^-23 |ref|.
  second-order products of the above: the sum times (1 + 2^-6).
  floor: the output's own subnormal spacing (float16: half of 2^-24; otherwise 1e-30).
Nothing in it is fitted to what a kernel gives; a case above it is a finding."""
import math

import torch

UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # unit roundoff of the 16-bit types
F16_MIN_NORMAL = 2.0 ** -14
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634


def visible(qi, kj, lo, kv_len, coff, causal):
    """the visibility rule: qi [c, 1] query rows, kj [1, k] key rows, lo [B, 1, 1] first live key per sequence -> bool [B, c, k]"""
    lim = torch.maximum(qi + coff, lo).clamp(max=kv_len - 1) if causal else torch.full_like(lo, kv_len - 1)
    return (kj >= lo) & (kj <= lim)


def _kv_lo(kv_lo, B, kv_len, device):
    if kv_lo is None:
        return torch.zeros(B, dtype=torch.long, device=device)
    return torch.as_tensor(kv_lo, dtype=torch.long, device=device).clamp(max=kv_len - 1).clamp(min=0)    # as the kernels clamp kv_start


def score_chunks(Q, K, causal, kv_lo=None, kv_len=None, chunk=None, rule=visible):
    """yields (r0, r1, s): the masked log2-domain scores of query rows r0 .. r1 - 1 in f64, [B, Hkv, G, r1 - r0, kv_len] (-inf where a
    key is not visible). ``chunk`` rows at a time (default: 2^26 scores, 512 MB); ``rule`` replaces the visibility rule (the host
    test puts its defects there)."""
    B, Hq, n, hd = Q.shape
    Hkv = K.shape[1]
    G = Hq // Hkv
    kv_len = K.shape[2] if kv_len is None else int(kv_len)
    lo = _kv_lo(kv_lo, B, kv_len, Q.device)[:, None, None]
    Kt = K[:, :, :kv_len].double().transpose(-1, -2)
    kj = torch.arange(kv_len, device=Q.device)[None, :]
    if chunk is None:
        chunk = max(1, min(n, (1 << 26) // (B * Hq * kv_len)))
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        q = Q[:, :, r0:r1].double().reshape(B, Hkv, G * (r1 - r0), hd)
        s = (q @ Kt).view(B, Hkv, G, r1 - r0, kv_len)
        vis = rule(torch.arange(r0, r1, device=Q.device)[:, None], kj, lo, kv_len, kv_len - n, causal)
        s.masked_fill_(~vis[:, None, None], float("-inf"))
        yield r0, r1, s


def attention_ref(Q, K, V, causal, kv_lo=None, kv_len=None, chunk=None):
    """-> (ref, A), both f64 [B, Hq, n, hd]: ref = sum_j p_j v_j and A_d = sum_j p_j |v_jd| with the normalised weights p — the scale
    the kernel's roundings act on. With float16 inputs a visible key whose unnormalised weight is below 2^-14 counts in A with
    2^-14 / L (term 1 of the module's derivation). ``kv_lo``: a list / tensor [B] or None."""
    B, Hq, n, hd = Q.shape
    Hkv = K.shape[1]
    kv_len = K.shape[2] if kv_len is None else int(kv_len)
    Vd = V[:, :, :kv_len].double()
    Va = Vd.abs()
    ref = torch.empty(B, Hq, n, hd, dtype=torch.float64, device=Q.device)
    A = torch.empty_like(ref)
    for r0, r1, s in score_chunks(Q, K, causal, kv_lo, kv_len, chunk):
        live = s > float("-inf")
        e = torch.exp2(s - s.amax(-1, keepdim=True))
        L = e.sum(-1, keepdim=True)
        rows = (B, Hkv, -1, kv_len)
        ref[:, :, r0:r1] = ((e / L).view(rows) @ Vd).view(B, Hq, r1 - r0, hd)
        if Q.dtype == torch.float16:
            e = torch.where(live & (e < F16_MIN_NORMAL), torch.full_like(e, F16_MIN_NORMAL), e)
        A[:, :, r0:r1] = ((e / L).view(rows) @ Va).view(B, Hq, r1 - r0, hd)
    return ref, A


def key_weight(Q, K, idx, causal, kv_lo=None, kv_len=None, chunk=None):
    """the normalised weight p of key idx[b, h, i] in row (b, h, i) -> f64 [B, Hq, n] (0 where that key is not visible)"""
    B, Hq, n, _ = Q.shape
    out = torch.empty(B, Hq, n, dtype=torch.float64, device=Q.device)
    for r0, r1, s in score_chunks(Q, K, causal, kv_lo, kv_len, chunk):
        e = torch.exp2(s - s.amax(-1, keepdim=True))
        p = (e / e.sum(-1, keepdim=True)).view(B, Hq, r1 - r0, -1)
        out[:, :, r0:r1] = p.gather(-1, idx[:, :, r0:r1, None].to(Q.device)).squeeze(-1)
    return out


def score_scale(Q, K, kv_len=None):
    """smag [B, Hq, n, 1] = |q_i| max_j |k_j| over the kv head's rows < kv_len: a bound on sum_d |q_id k_jd| for every key"""
    B, Hq, n, _ = Q.shape
    Hkv = K.shape[1]
    kmax = K[:, :, :kv_len].double().norm(dim=-1).amax(-1)                               # [B, Hkv]
    return Q.double().norm(dim=-1, keepdim=True) * kmax.repeat_interleave(Hq // Hkv, 1)[:, :, None, None]


def attention_bound(A, ref, dt, n_keys, smag):
    """the allowed |out - ref| per element (the module's docstring derives every term). ``dt``: the kernel's type, ``n_keys``: the
    largest number of keys a row sums, ``smag``: score_scale(Q, K)."""
    hd = ref.shape[-1]
    both = A + ref.abs()
    f32 = both * (LN2 * 2 * (hd + 1) * 2.0 ** -24 * smag + 2.0 ** -22) \
        + both * (n_keys * (1 + 1 / 64) + 72) * 2.0 ** -24                                  # terms 4, 5
    if dt == torch.float32:
        return (f32 + ref.abs() * 2.0 ** -23) * (1 + 2.0 ** -6) + 1e-30                     # term 6
    u = UNIT[dt]
    floor = 2.0 ** -25 if dt == torch.float16 else 1e-30
    return (u * A + u * ref.abs() + f32) * (1 + 2.0 ** -6) + floor                          # terms 1 (2 is empty), 3


def worst(out, ref, bound):
    """-> (max err / bound, its index tuple, err there, bound there); a NaN in ``out`` gives inf"""
    err = (out.double() - ref).abs()
    r = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    k = int(r.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(k), r.shape))
    return float(r.flatten()[k]), idx, float(err.flatten()[k]), float(bound.flatten()[k])


# ---- input families --------------------------------------------------------------------------------------------------------------
# gauss      Q, K, V Gaussian (the inputs of tests/test_gpu_ops.py): no key matters much to any row
# addressed  unit-norm random codes g_j; K_j = g_j, Q_i = peak * g_target(i): row i scores `peak` (log2 units) on its target and
#            N(0, peak^2 / hd) elsewhere, so it puts most of its weight on ONE chosen key — an edge key that is dropped, doubled or read from
#            the wrong head moves the row by a large part of |v|
# future     Q_i aims at the first key the causal mask hides (i + 1; with a left pad every other row at kv_lo - 1 instead)
CAUSAL_TARGETS = ("diagonal i", "i - 1", "first live key kv_lo", "last key of the previous 64-tile", "first key of the row's 64-tile",
                  "i - 64", "i - 127", "i - 128")


def causal_targets(n, Hq, kv_lo, device="cpu"):
    """target key of row i of head h of sequence b, [B, Hq, n]: CAUSAL_TARGETS cycled by (i + h) % 8, clamped into [kv_lo, max(i, kv_lo)]"""
    i = torch.arange(n, device=device)
    lo = torch.as_tensor(kv_lo, dtype=torch.long, device=device)[:, None, None]
    tile = i // 64 * 64
    cands = torch.stack([i, i - 1, torch.zeros_like(i) - 1, tile - 1, tile, i - 64, i - 127, i - 128])          # -1: replaced by kv_lo below
    mode = (i[None, :] + torch.arange(Hq, device=device)[:, None]) % 8                                          # [Hq, n]
    t = cands.gather(0, mode)[None].expand(lo.shape[0], Hq, n)
    t = torch.where(mode[None] == 2, lo.expand_as(t), t)
    return torch.minimum(torch.maximum(t, lo), torch.maximum(i[None, None, :], lo))


def vit_targets(N, H, device="cpu"):
    """non-causal, N keys in tiles of 64 (ntiles of them; with kv_prefix = 1 the tiles start at key 1): row r of head h takes, by
    (r + h) % 4: 0: key 0 (the cls key kv_prefix folds in) or, every other time, the last key N - 1; 1: key 64 t; 2: key 64 t - 1
    (the tile edges with and without the prefix shift; t = 1 + (r // 4) % ((N - 1) // 64)); 3: the sweep — kv tile r % ntiles, so that
    every (128-row q-block, kv tile) pair is the main contributor of at least one row of every full q-block."""
    r = torch.arange(N, device=device)
    ntiles = (N + 63) // 64
    t = 1 + (r // 4) % ((N - 1) // 64)
    sweep = (64 * (r % ntiles) + (r * 7) % 64).clamp(max=N - 1)
    cands = torch.stack([torch.where((r // 4) % 2 == 0, torch.zeros_like(r), torch.full_like(r, N - 1)), 64 * t, 64 * t - 1, sweep])
    mode = (r[None, :] + torch.arange(H, device=device)[:, None]) % 4
    return cands.gather(0, mode)                                                                                # [H, N]


def decode_targets(kv_len, kv_lo, nsplit):
    """keys the single decode query is aimed at in turn: the first live key, the appended key kv_len - 1, and the first and last key of
    every split's range (plain_work of attention_decode.hip: the 64-key tiles from kv_lo's on, dealt in runs of `per` to the splits)"""
    ntiles, t_lo = (kv_len + 63) // 64, kv_lo // 64
    per = (ntiles - t_lo + nsplit - 1) // nsplit
    out = [kv_lo, kv_len - 1]
    for s in range(nsplit):
        t0, t1 = t_lo + s * per, min(ntiles, t_lo + (s + 1) * per)
        if t0 < t1:
            out += [max(t0 * 64, kv_lo), min(t1 * 64, kv_len) - 1]
    return out


def _codes(shape, gen, device):
    return torch.nn.functional.normalize(torch.randn(*shape, generator=gen, device=device), dim=-1)


def make_inputs(family, B, Hq, Hkv, n, rows, hd, dt, seed, target=None, peak=12.0, device="cpu"):
    """-> Q [B, Hq, n, hd], K, V [B, Hkv, rows, hd] in ``dt`` for n queries over keys 0 .. n - 1 (rows >= n: whatever lies behind).
    'gauss', or 'addressed' with ``target`` [B, Hq, n] (key rows < ``rows``). Rows >= n of K come out as 2 x a code ('addressed': what
    a 'future' row aims at) or as Gaussian rows; the caller overwrites the pad rows it wants adversarial."""
    gen = torch.Generator(device=device).manual_seed(seed)
    G = Hq // Hkv
    V = torch.randn(B, Hkv, rows, hd, generator=gen, device=device)
    if family == "gauss":
        Q = torch.randn(B, Hq, n, hd, generator=gen, device=device) * (hd ** -0.5 * LOG2E)
        K = torch.randn(B, Hkv, rows, hd, generator=gen, device=device)
    else:
        K = _codes((B, Hkv, rows, hd), gen, device)
        kq = K.repeat_interleave(G, 1)                                                       # [B, Hq, rows, hd]
        Q = peak * kq.gather(2, target.to(device)[..., None].expand(B, Hq, n, hd))
        K[:, :, n:] *= 2.0
    return Q.to(dt), K.to(dt), V.to(dt)


def adversarial_pad(Q, K, V, kv_len):
    """rows >= kv_len in place: K rows that would score highest for the last query rows (8 x the direction of a query of the kv head's
    first q head: a score of 8 |q|), V rows of 1e4. Finite on purpose: they meet P = 0 only, and 0 * NaN would hide nothing."""
    G = Q.shape[1] // K.shape[1]
    npad = K.shape[2] - kv_len
    if npad <= 0:
        return
    qd = torch.nn.functional.normalize(Q[:, ::G].float(), dim=-1)                            # [B, Hkv, n, hd]
    take = (Q.shape[2] - 1 - torch.arange(npad, device=Q.device) % Q.shape[2])
    K[:, :, kv_len:] = (8.0 * qd[:, :, take]).to(K.dtype)
    V[:, :, kv_len:] = 1e4
