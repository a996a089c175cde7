"""``generate(beam_search=BeamSearch(...))``: beam search on the device, checked on the host and packed into the words
``gar_beam_step`` reads (include/gar_hip.h). Pure Python: importing it needs neither torch nor the library.

Semantics are those of transformers' ``GenerationMixin._beam_search`` with ``do_sample=False``: ``num_beams`` running beams per
prompt, ``max(2, 1 + n_eos) * num_beams`` candidates kept per step, a finished set of ``num_beams`` hypotheses scored
``sum of log-probabilities / length ** length_penalty``, and HF's three ``early_stopping`` modes. The GenerationConfig fields
``num_beams`` / ``length_penalty`` / ``early_stopping`` stay refused by :meth:`GARModel.generate`: the feature comes under this
parameter, as ``logits_processing=`` and ``sampling_warpers=`` do.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import List, Sequence, Union

TOPK_MAX = 32               # gar_topk_lp's largest k: the candidates a row can bring to a step
MAX_EOS = 16                # GAR_BEAM_MAX_EOS
PARAM_WORDS = 4 + MAX_EOS   # GAR_BEAM_PARAM_WORDS
EARLY_STOPPING_CODES = {False: 0, True: 1, "never": 2}


class BeamBudgetError(ValueError):
    """num_beams * max(2, 1 + n_eos) above gar_topk_lp's k = 32 (GARModel raises it as GarError)"""


@dataclass(frozen=True)
class BeamSearch:
    """One beam-search request.

    ``num_beams`` K >= 2: running beams per prompt. ``length_penalty``: a finished hypothesis of n tokens scores
    ``sum_logprobs / n ** length_penalty`` (HF: > 0 favours longer ones). ``early_stopping``: ``False`` (HF's default heuristic:
    stop when the best running beam, at its current length, cannot beat the worst kept hypothesis), ``True`` (stop when K
    hypotheses are kept) or ``"never"`` (the heuristic at ``max_new_tokens`` with a positive penalty: canonical beam search with
    ``length_penalty=0``). ``num_return_sequences`` in 1..K: hypotheses returned per prompt, best first."""
    num_beams: int
    length_penalty: float = 1.0
    early_stopping: Union[bool, str] = False
    num_return_sequences: int = 1

    def __post_init__(self):
        k = self.num_beams
        if isinstance(k, bool) or not isinstance(k, int) or k < 2:
            raise ValueError(f"`num_beams` has to be an integer >= 2 (1 is greedy search: pass no beam_search), but is {k!r}")
        lp = self.length_penalty
        if isinstance(lp, bool) or not isinstance(lp, (int, float)) or lp != lp or lp in (float("inf"), float("-inf")):
            raise ValueError(f"`length_penalty` has to be a finite float, but is {lp!r}")
        object.__setattr__(self, "length_penalty", float(lp))
        es = self.early_stopping
        if not (es is True or es is False or (isinstance(es, str) and es == "never")):
            raise ValueError(f"`early_stopping` has to be False, True or \"never\", but is {es!r}")
        n = self.num_return_sequences
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= k:
            raise ValueError(f"`num_return_sequences` has to be an integer in 1..num_beams = {k}, but is {n!r}")

    @classmethod
    def coerce(cls, value):
        """``generate(beam_search=value)``: None, a BeamSearch, or a dict with its field names"""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            return cls(**value)
        raise TypeError(f"beam_search: a BeamSearch, a dict or None, not {type(value).__name__}")

    def candidates(self, n_eos: int) -> int:
        """M = HF's ``beams_to_keep``: candidates per prompt that survive a step. Known when the request is armed (n_eos);
        refused when a row cannot bring that many (gar_topk_lp's k <= 32)."""
        m = max(2, 1 + int(n_eos)) * self.num_beams
        if m > TOPK_MAX:
            raise BeamBudgetError(f"beam_search: num_beams = {self.num_beams} x max(2, 1 + {n_eos} eos ids) = {m} candidates per step, "
                                  f"above gar_topk_lp's k = {TOPK_MAX}")
        return m

    def pack(self, max_new_tokens: int, eos_ids: Sequence[int]) -> List[int]:
        """the int32 parameter block of gar_beam_step: [max_new_tokens, early_stopping code, length_penalty > 0, n_eos, eos ids...]"""
        eos = [int(e) for e in eos_ids]
        if len(eos) > MAX_EOS:
            raise BeamBudgetError(f"beam_search: {len(eos)} eos ids, at most {MAX_EOS}")
        words = [int(max_new_tokens), EARLY_STOPPING_CODES[self.early_stopping], int(self.length_penalty > 0.0), len(eos)] + eos
        return words + [-1] * (PARAM_WORDS - len(words))

    def length_powers(self, n: int) -> List[float]:
        """len_pow[t] = float32(float(t + 1) ** length_penalty), t < n: HF divides an f32 score by this Python float, which torch
        rounds to f32 first — so the penalty is one f32 division on the device"""
        def f32(x):
            try:
                return struct.unpack("f", struct.pack("f", x))[0]
            except OverflowError:
                return float("inf")
        return [f32(float(t + 1) ** self.length_penalty) for t in range(n)]
