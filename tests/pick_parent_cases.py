"""TEST INFRASTRUCTURE: the inputs, the requests and the replay of tests/golden/pick_parent.npz — shared by
tools/capture_pick_goldens.py (which records what the PARENT commit's libraries answer) and tests/test_gpu_pick_parent.py (which
replays the same calls on the current build and compares bit for bit).

Inputs: B = 6 rows per vocabulary size, rebuilt from numpy.random.default_rng(SEED_ROWS + V): two rows quantised to multiples of
1/8 inside (-16, 16) (exact in bf16 and f16: ties at the k-th value and at the top-p cut), two continuous f32 rows, one row of -inf
but three entries, one row of equal entries. The leading dimension is padded past V with a sentinel that would win any maximum."""
import hashlib

import numpy as np

SEED_ROWS = 20260
VS = (37, 1000, 4133)               # under one wave / one element per thread, some threads empty / five per thread, trailing chunks empty
PAD = 24
B = 6
QUANT_ROWS, FINITE3_ROW, EQUAL_ROW = (0, 1), 4, 5
SEED = (0x5EED1234 << 32) | 0x9E3779B9          # one 64-bit Philox key with a non-zero high word
STEPS = (0, 3)
ROW_OFFSETS = (0, 5)
COLS = 8
SENTINEL = 12345.0

# (temperature, top_k, top_p); top_k = -1 stands for "V + 3" (top_k >= V: no top-k)
PLAIN = [(1.0, 0, 1.0), (1.3, 5, 1.0), (0.7, 0, 0.5), (0.8, 50, 0.9), (1.0, -1, 0.8)]
# (temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff): each further warper alone, all four, and a typical_p small
# enough to remove the row maximum followed by epsilon (the kernel's second-maximum path)
EXT = [(1.0, 0, 1.0, 0.1, 1.0, 0.0, 0.0), (1.0, 0, 1.0, 0.0, 0.9, 0.0, 0.0), (1.0, 0, 1.0, 0.0, 1.0, 3e-3, 0.0),
       (1.0, 0, 1.0, 0.0, 1.0, 0.0, 2e-3), (0.8, 50, 0.95, 0.02, 0.95, 1e-3, 2e-3), (1.3, 0, 1.0, 0.0, 0.2, 3e-3, 0.0)]
EOS_PLAIN, EOS_EXT = 3, 4           # the requests that run with the eos latches on
DTYPES = ("float32", "bfloat16", "float16")


def top_k_of(k, V):
    return V + 3 if k < 0 else k


def rows(V):
    """float32 [B, V]"""
    rng = np.random.default_rng(SEED_ROWS + V)
    x = np.empty((B, V), dtype=np.float32)
    for b in QUANT_ROWS:
        x[b] = rng.integers(-127, 128, size=V).astype(np.float32) / 8.0
    x[2] = (rng.standard_normal(V) * 2.5).astype(np.float32)
    x[3] = (rng.standard_normal(V) * 0.6 - 3.0).astype(np.float32)
    x[FINITE3_ROW] = -np.inf
    x[FINITE3_ROW, [V // 5, V // 2, V - 2]] = np.array([0.5, -1.25, 0.5], dtype=np.float32)
    x[EQUAL_ROW] = np.float32(rng.integers(-40, 40) / 8.0)
    return x


def rows_sha256():
    h = hashlib.sha256()
    for V in VS:
        h.update(rows(V).tobytes())
    return h.hexdigest()


def row_ids(dtype_name):
    """f16 runs through the twin library on the quantised rows only"""
    return list(QUANT_ROWS) if dtype_name == "float16" else list(range(B))


def logits_seen(V, dtype_name):
    """float32 numpy [rows, V]: the values the kernels read for this dtype"""
    import torch
    x = torch.from_numpy(rows(V)[row_ids(dtype_name)])
    return x.to(getattr(torch, dtype_name)).float().numpy()


def eos_ids(V):
    """two ids some rows do draw (row 0's maximum, one of the -inf row's three entries) and an entry that never matches"""
    return [int(np.argmax(rows(V)[0])), V // 2, -1]


def rows_batches(V, n):
    """two gar_sample_rows batches over n rows: per row None (greedy) or a PLAIN index; col0 = 2 and counter row = 5 + row"""
    a = [None, 1, 2, 3, None, 0][:n] if n == B else [None, 3]
    b = [2, None, 3, None, 1, None][:n] if n == B else [1, None]
    return [a, b]


ROWS_COL, ROWS_COL0 = 5, 2


def replay(device="cuda:0"):
    """every call, in a fixed order: dict of numpy arrays (tokens int64, planes as uint32 bits, n_kept / finished / done int32)"""
    import torch
    from gar_amd import ops
    from gar_amd.continuous import pack_sample_row
    toks, raw, warped, nkept, fin, done = [], [], [], [], [], []
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)

    def latches(n, V, on):
        if not on:
            return {}
        return dict(eos_ids=torch.tensor(eos_ids(V), dtype=torch.int64, device=device),
                    finished=torch.full((n,), -1, dtype=torch.int32, device=device), done_count=torch.zeros(1, dtype=torch.int32, device=device))

    def record(out, cur, col, planes, kw, n):
        torch.cuda.synchronize()
        rest = torch.ones(COLS, dtype=torch.bool)
        rest[col] = False
        assert torch.equal(out[:, col], cur) and bool((out[:, rest] == -1).all())
        toks.append(cur.cpu().numpy())
        for dst, p in zip((raw, warped), planes or ()):
            assert bool((p[:, rest] == SENTINEL).all())
            dst.append(p[:, col].contiguous().view(torch.int32).cpu().numpy().view(np.uint32))
        if kw:
            fin.append(kw["finished"].cpu().numpy())
            done.append(kw["done_count"].cpu().numpy())

    for V in VS:
        for dn in DTYPES:
            dt = getattr(torch, dn)
            ids = row_ids(dn)
            n = len(ids)
            buf = torch.full((n, V + PAD), 6.0e4 if dn == "float16" else 3.0e38, dtype=torch.float32)
            buf[:, :V] = torch.from_numpy(rows(V)[ids])
            x = buf.to(dt).to(device)[:, :V]
            seed = torch.tensor([SEED], dtype=torch.int64, device=device)
            for ext, reqs in ((False, PLAIN), (True, EXT)):
                for ri, rq in enumerate(reqs):
                    p8 = [rq[0], rq[2], float(top_k_of(rq[1], V)), 0.0] + (list(rq[3:]) if ext else [0.0, 1.0, 0.0, 0.0])
                    params = torch.tensor(p8 if ext else p8[:4], dtype=torch.float32, device=device)
                    for lp in (False, True):
                        for step in STEPS:
                            for off in ROW_OFFSETS:
                                out = torch.full((n, COLS), -1, dtype=torch.int64, device=device)
                                cur = torch.full((n,), -1, dtype=torch.int64, device=device)
                                planes = [torch.full((n, COLS), SENTINEL, dtype=torch.float32, device=device) for _ in range(2)] if lp else None
                                kw = latches(n, V, ri == (EOS_EXT if ext else EOS_PLAIN))
                                more = dict(kw, row_offset=off)
                                if lp:
                                    more.update(logprobs=planes[0], logprobs_warped=planes[1])
                                if ext:
                                    nk = torch.full((n,), -7, dtype=torch.int32, device=device)
                                    ops.sample_ext(x, V, out, COLS, i32([step]), cur, params, seed, n_kept=nk, **more)
                                else:
                                    ops.sample(x, V, out, COLS, i32([step]), cur, params, seed, **more)
                                record(out, cur, step, planes, kw, n)
                                if ext:
                                    nkept.append(nk.cpu().numpy())
            for batch in rows_batches(V, n):
                words = [pack_sample_row(None if r is None else (PLAIN[r][0], PLAIN[r][2], top_k_of(PLAIN[r][1], V)), SEED, ROWS_COL0, 5 + b)
                         for b, r in enumerate(batch)]
                out = torch.full((n, COLS), -1, dtype=torch.int64, device=device)
                cur = torch.full((n,), -1, dtype=torch.int64, device=device)
                kw = latches(n, V, True)
                ops.sample_rows(x, V, out, COLS, i32([ROWS_COL]), cur, i32(words), **kw)
                record(out, cur, ROWS_COL, None, kw, n)
    cat = lambda a, d: np.concatenate(a).astype(d)
    return {"tokens": cat(toks, np.int64), "lp_raw": cat(raw, np.uint32), "lp_warped": cat(warped, np.uint32), "n_kept": cat(nkept, np.int32),
            "finished": cat(fin, np.int32), "done_count": cat(done, np.int32)}


def calls():
    """the calls of replay() in its order, for the host checks: (kind, V, dtype name, request, step, row_offset) with kind
    'plain' / 'ext' / 'rows' (request = the batch); each owns len(row_ids(dtype)) consecutive entries of 'tokens'"""
    out = []
    for V in VS:
        for dn in DTYPES:
            for kind, reqs in (("plain", PLAIN), ("ext", EXT)):
                for rq in reqs:
                    for _lp in (False, True):
                        for step in STEPS:
                            for off in ROW_OFFSETS:
                                out.append((kind, V, dn, rq, step, off))
            for batch in rows_batches(V, len(row_ids(dn))):
                out.append(("rows", V, dn, batch, ROWS_COL - ROWS_COL0, 5))
    return out


def check_sane(tokens):
    """the golden tokens against the CPU restatements, no GPU: a plain request's token lies in oracle/sampling.py's kept set, an ext
    request's in tests/sampling_warpers_ref.py's, a greedy row's is the first maximum. Returns the number of tokens checked."""
    import functools
    import sampling_warpers_ref as R
    from oracle import sampling as S

    @functools.lru_cache(maxsize=None)
    def kept(V, dn, b, rq):
        x = logits_seen(V, dn)[b]
        if len(rq) == 3:
            return S.warp(x, rq[0], top_k_of(rq[1], V), rq[2])[1] & (x > -np.inf)
        return R.warp_ext(x, rq[0], top_k_of(rq[1], V), *rq[2:])[1]

    at = 0
    for kind, V, dn, rq, _step, _off in calls():
        n = len(row_ids(dn))
        for b in range(n):
            tok = int(tokens[at + b])
            req = rq if kind != "rows" else (None if rq[b] is None else PLAIN[rq[b]])
            if req is None:
                assert tok == int(np.argmax(logits_seen(V, dn)[b])), (kind, V, dn, b, tok)
            else:
                assert 0 <= tok < V and kept(V, dn, b, tuple(req))[tok], (kind, V, dn, req, b, tok)
        at += n
    assert at == len(tokens), (at, len(tokens))
    return at
