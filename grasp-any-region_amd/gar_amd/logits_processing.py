"""``generate(logits_processing=...)``: the request's logits processors, checked on the host and packed into the int32 block
``gar_logits_process`` reads on the device (include/gar_hip.h). Pure Python: importing it needs neither torch nor the library.

Semantics are those of HF's processors as the reference's call sees them: it runs ``self.mllm.generate(inputs_embeds=...)`` without
``input_ids`` (reference modeling_gar.py:418-426), so the processors' ``input_ids`` start at width 0 and grow by the generated
tokens only — the prompt is never penalised or scanned. The history of a row at step t is ``sequences[row, :t]``.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, fields
from typing import List, Sequence, Tuple

HEADER_WORDS = 8          # gar_logits_process: [penalty f32 bits, n, m, n_suppress, n_begin, n_bad, n_bad_tokens, 0]
BLOCK_WORDS = 4096        # int32 words of the block a KV state keeps: the header and every id list of a request have to fit


class _Refused(Exception):
    """raised as GarError by the caller that owns gar_amd.hip (this module stays importable without the library)"""


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _id_tuple(name: str, ids) -> Tuple[int, ...]:
    if ids is None:
        return ()
    ids = tuple(ids)
    for i in ids:
        if not _is_int(i):
            raise ValueError(f"`{name}` has to be a list of integers, but holds {i!r}")
    return tuple(int(i) for i in ids)


@dataclass(frozen=True)
class LogitsProcessing:
    """The logits processors of one ``generate()`` request, applied on the device to every step's logits before the pick (greedy
    search) or before temperature / top-k / top-p (``do_sample=True``), in HF's list order. "Ban" = the score becomes -inf.

    ``repetition_penalty`` p > 0 (1.0 = off): every distinct token of the history has its score x replaced by x * p if x < 0, else
    x / p — once, however often it occurs.
    ``no_repeat_ngram_size`` n >= 0 (0 = off): when t + 1 >= n, every token that would complete an n-gram already in the history is
    banned (n = 1: every history token).
    ``min_new_tokens`` m >= 0: while t < m the request's eos ids are banned (with the empty prompt HF's ``min_length`` is the same).
    ``suppress_tokens``: always banned. ``begin_suppress_tokens``: banned at t == 0 only.
    ``bad_words_ids``: a one-token entry is always banned (HF drops one that equals an eos id; so does this); the last token of a
    longer entry of L tokens is banned when the history ends with its first L - 1 tokens and — HF's SequenceBiasLogitsProcessor
    ignores an entry longer than the context — t >= L.

    Capacity: 8 + len(suppress_tokens) + len(begin_suppress_tokens) + len(bad_words_ids) + 1 + (tokens of all bad words) int32
    words have to fit the 4096-word block of a state (``GarError`` otherwise, never truncation); ids outside [0, vocab) are a
    ``GarError`` too."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0
    suppress_tokens: Sequence[int] = ()
    begin_suppress_tokens: Sequence[int] = ()
    bad_words_ids: Sequence[Sequence[int]] = ()

    def __post_init__(self):
        p = self.repetition_penalty
        p = 1.0 if p is None else p
        # HF RepetitionPenaltyLogitsProcessor: a strictly positive float (the neutral 1 never reaches HF's check, so int 1 passes)
        if not (_is_int(p) and p == 1) and (not isinstance(p, float) or not p > 0):
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {p!r}")
        if not 1e-30 <= float(p) <= 1e30:       # the kernel computes with its f32 value
            raise ValueError(f"`penalty` has to be a strictly positive float within [1e-30, 1e30], but is {p!r}")
        n = 0 if self.no_repeat_ngram_size is None else self.no_repeat_ngram_size
        if not _is_int(n) or n < 0:     # HF NoRepeatNGramLogitsProcessor: a strictly positive integer; 0 = the processor is absent
            raise ValueError(f"`ngram_size` has to be a strictly positive integer (0 = off), but is {n!r}")
        m = 0 if self.min_new_tokens is None else self.min_new_tokens
        if not _is_int(m) or m < 0:     # HF MinNewTokensLengthLogitsProcessor
            raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {m!r}")
        bad = self.bad_words_ids
        bad = () if bad is None else tuple(bad)
        words: List[Tuple[int, ...]] = []
        for w in bad:                   # HF NoBadWordsLogitsProcessor / SequenceBiasLogitsProcessor
            if isinstance(w, (str, bytes)) or not hasattr(w, "__iter__"):
                raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {list(bad)!r}")
            w = tuple(w)
            if len(w) == 0 or any(not _is_int(i) or i < 0 for i in w):
                raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of non-negative integers, but is {list(bad)!r}")
            words.append(tuple(int(i) for i in w))
        set_ = object.__setattr__
        set_(self, "repetition_penalty", float(p))
        set_(self, "no_repeat_ngram_size", int(n))
        set_(self, "min_new_tokens", int(m))
        set_(self, "suppress_tokens", _id_tuple("suppress_tokens", self.suppress_tokens))
        set_(self, "begin_suppress_tokens", _id_tuple("begin_suppress_tokens", self.begin_suppress_tokens))
        set_(self, "bad_words_ids", tuple(words))

    @classmethod
    def coerce(cls, value) -> "LogitsProcessing":
        """``generate(logits_processing=value)``: None, a LogitsProcessing, or a dict with its field names"""
        if value is None:
            return cls()
        if isinstance(value, cls):
            return value
        if isinstance(value, dict):
            unknown = sorted(set(value) - {f.name for f in fields(cls)})
            if unknown:
                raise TypeError(f"logits_processing: unknown keys {unknown} (fields: {[f.name for f in fields(cls)]})")
            return cls(**value)
        raise TypeError(f"logits_processing: a LogitsProcessing, a dict or None, not {type(value).__name__}")

    @property
    def neutral(self) -> bool:
        """nothing to do at any step: the request takes the path of one without the parameter"""
        return (self.repetition_penalty == 1.0 and self.no_repeat_ngram_size == 0 and self.min_new_tokens == 0
                and not self.suppress_tokens and not self.begin_suppress_tokens and not self.bad_words_ids)

    def pack(self, vocab_size: int, eos_ids: Sequence[int] = ()) -> List[int]:
        """the int32 words of gar_logits_process's parameter block for a model of ``vocab_size``; ``eos_ids``: the request's, for
        HF's rule that a one-token bad word equal to an eos id is dropped. Raises :class:`_Refused` (the caller's GarError) for an
        id outside [0, vocab_size) and for lists beyond the block's capacity."""
        V = int(vocab_size)
        eos = set(int(e) for e in eos_ids)
        bad = [w for w in self.bad_words_ids if not (len(w) == 1 and w[0] in eos)]
        for name, ids in (("suppress_tokens", self.suppress_tokens), ("begin_suppress_tokens", self.begin_suppress_tokens),
                          ("bad_words_ids", [i for w in bad for i in w])):
            for i in ids:
                if not 0 <= i < V:
                    raise _Refused(f"logits_processing: {name} id {i} is outside [0, vocab_size = {V})")
        offs, toks = [0], []
        for w in bad:
            toks.extend(w)
            offs.append(len(toks))
        words = [struct.unpack("<i", struct.pack("<f", self.repetition_penalty))[0], min(self.no_repeat_ngram_size, 2 ** 31 - 1),
                 min(self.min_new_tokens, 2 ** 31 - 1), len(self.suppress_tokens), len(self.begin_suppress_tokens), len(bad),
                 len(toks), 0]
        words += list(self.suppress_tokens) + list(self.begin_suppress_tokens) + (offs if bad else []) + toks
        if len(words) > BLOCK_WORDS:
            raise _Refused(f"logits_processing: {len(words)} words of ids (8 + suppress_tokens + begin_suppress_tokens + "
                           f"bad_words_ids entries + 1 + their tokens), the device block holds {BLOCK_WORDS}")
        return words
