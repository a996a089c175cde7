"""The six logits processors of generate(logits_processing=...) restated in torch on (row history, logits row): the expected
value of the host tests (against transformers' own classes, tests/golden/logits_process.npz) and of the kernel tests
(gar_logits_process, bit for bit). Semantics: HF's processors over an `input_ids` that holds the generated tokens only
(DESIGN 7.7). Not the product: gar_amd never imports this."""
import torch

FIELDS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens", "bad_words_ids")


def options(P) -> dict:
    """the six fields of a LogitsProcessing / a dict, with the neutral defaults"""
    d = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_new_tokens": 0, "suppress_tokens": (),
         "begin_suppress_tokens": (), "bad_words_ids": ()}
    for k in FIELDS:
        v = P.get(k) if isinstance(P, dict) else getattr(P, k)
        if v is not None:
            d[k] = v
    return d


def banned_ids(history, V: int, P, eos_ids=()) -> set:
    """ids whose score becomes -inf at step t = len(history)"""
    o = options(P)
    h = [int(x) for x in history]
    t = len(h)
    eos = [int(e) for e in eos_ids]
    ban = set()
    n = int(o["no_repeat_ngram_size"])
    if n > 0 and t + 1 >= n:                                # HF _calc_banned_ngram_tokens
        tail = h[t - n + 1:t]
        for j in range(0, t - n + 1):
            if h[j:j + n - 1] == tail:
                ban.add(h[j + n - 1])
    if t < int(o["min_new_tokens"]):                        # HF MinNewTokensLengthLogitsProcessor (prompt length 0)
        ban.update(eos)
    ban.update(int(i) for i in o["suppress_tokens"])
    if t == 0:
        ban.update(int(i) for i in o["begin_suppress_tokens"])
    for w in o["bad_words_ids"]:                            # HF NoBadWordsLogitsProcessor -> SequenceBiasLogitsProcessor
        w = [int(i) for i in w]
        if len(w) == 1:
            if w[0] not in eos:                             # HF drops a one-token entry that equals an eos id
                ban.add(w[0])
        elif len(w) <= t and h[t - (len(w) - 1):] == w[:-1]:    # HF ignores an entry longer than the context
            ban.add(w[-1])
    return {i for i in ban if 0 <= i < V}                   # an id outside the vocabulary names no entry


def process_row(history, row: torch.Tensor, V: int, P, eos_ids=()) -> torch.Tensor:
    """the processed copy of one logits row (any float dtype, columns V.. untouched): the penalty in f32 on the stored value,
    rounded back to the row's dtype; bans are -inf"""
    o = options(P)
    out = row.clone()
    p = float(o["repetition_penalty"])
    if p != 1.0:
        ids = sorted({int(x) for x in history if 0 <= int(x) < V})
        if ids:
            ix = torch.tensor(ids, dtype=torch.int64)
            x = row[ix].to(torch.float32)
            pt = torch.tensor(p, dtype=torch.float32)
            out[ix] = torch.where(x < 0, x * pt, x / pt).to(row.dtype)
    ban = sorted(banned_ids(history, V, P, eos_ids))
    if ban:
        out[torch.tensor(ban, dtype=torch.int64)] = float("-inf")
    return out


def process(histories, logits: torch.Tensor, V: int, P, eos_ids=()) -> torch.Tensor:
    """rows of ``logits`` [B, ld] with their histories (a list of B id lists)"""
    return torch.stack([process_row(h, logits[b], V, P, eos_ids) for b, h in enumerate(histories)])


def first_argmax(row: torch.Tensor) -> int:
    """greedy pick with the first-index tie rule of gar_argmax"""
    x = row.to(torch.float32)
    return int((x == x.max()).nonzero()[0, 0])
